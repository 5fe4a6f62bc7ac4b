# -*- coding: utf-8 -*-
"""MI355X: the on-device nested sampler (csrc/nested.hip) replayed batch by batch against tests/nested_ref.py, its bit
contracts, its stopping rule, its statistics against quadrature and importance sampling, and the public interface."""
import numpy as np
import pytest

import hmc_ref as hr
import nested_ref as nr

pytestmark = pytest.mark.gpu


def _mcmc():
    from approxposterior_amd import mcmc
    return mcmc


def _switch_n(D):
    """The smallest N whose training stream the kernel no longer stages in LDS, from the kernel's own budget."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    n = 1
    while lib.apgp_nested_xlds(n, D) == 1:
        n += 1
    assert lib.apgp_nested_xlds(n - 1, D) == 1 and lib.apgp_nested_xlds(n, D) == 0
    return n


# (D, n, kernel, nlive, batch, nsteps, nruns, box, seed): n = None is one size above the switch of the training stream from
# LDS to L2; box "wide" is the ensemble replay's, "tight" a small box around the bulk whose faces cut the live cloud.
# The seeds were chosen on the CPU (tools/nested_reference.py seeds: nested_ref.run_one on the oracle's mean): the
# reference's own closest decision |mu - L*| is 3.9e-9 or more in every run of every case, against a mean budget of
# 3.5e-12 or less.  (Seeds 101 and 107 of the first case were passed over: a zero move between two copies of a stuck walker
# proposes a live point again, whose mean is the threshold itself.)
REPLAY_CASES = [
    (2, 90, "se", 16, 4, 5, 3, "wide", 108),
    (2, 90, "amp", 64, 16, 5, 1, "tight", 102),
    (8, 130, "selin1", 64, 1, 1, 1, "wide", 103),
    (8, 130, "se", 64, 4, 1, 3, "wide", 104),
    (9, 130, "se", 64, 4, 5, 3, "wide", 105),
    (9, None, "se", 64, 16, 5, 1, "wide", 106),
]
REPLAY_BATCHES = 40
_DEV = {}


def _case_id(c):
    return "D%d-n%s-%s-live%d-b%d-s%d-r%d-%s" % c[:8]


def _device_run(c, nruns=None, debug=True):
    """The device's run of a replay case (cached: the replay, the bit tests and the stopping tests share it)."""
    D, n, kern, nlive, batch, nsteps, runs, box, seed = c
    n = _switch_n(D) if n is None else n
    nruns = runs if nruns is None else nruns
    key = (c, nruns, debug)
    if key not in _DEV:
        X, y, gp, gpo, model, _, _ = hr.case_inputs((D, 1, n, kern, 0, 0, 0, 0, "wide"))
        b = hr.case_box(D, box)
        if not gp.computed:
            gp.compute(X)
        res = gp.sample_nested(y, b, nlive=nlive, batch=batch, nsteps=nsteps, nruns=nruns, dlogz=0.0,
                               maxBatches=REPLAY_BATCHES, seed=seed, debug=debug)
        _DEV[key] = (res, gp, y, model, b)
    return _DEV[key]


@pytest.mark.parametrize("c", REPLAY_CASES, ids=_case_id)
def test_replay_batch_by_batch(c):
    D, n, kern, nlive, batch, nsteps, nruns, box, seed = c
    res, gp, y, model, b = _device_run(c)
    assert np.all(res.nbatch == REPLAY_BATCHES) and len(res.logL) == nruns * (nlive + batch * REPLAY_BATCHES)
    tot = {"ndecisions": 0, "nnear": 0, "nwrong": 0}
    for r in range(nruns):
        m = res.run == r
        f = nr.forced(model, b[:, 0], b[:, 1], model.sc, nlive, batch, nsteps, seed, r, res.points[m], res.logL[m],
                      res.logLBirth[m], res.info["record"][m], REPLAY_BATCHES, res.info["trace"][r])
        print("run %d: start %.2f ulp, proposals %.3f of budget, mean %.3f of budget, %d decisions, %d near, %d wrong, "
              "%d accepted, %d stuck" % (r, f["start_err"], f["prop_err"], f["mu_err"], f["ndecisions"], f["nnear"], f["nwrong"],
                                       f["naccept"], f["stuck"]))
        assert f["start_err"] <= 2.0                   # fma(span, u, lo) against lo + span u: one rounding each
        assert f["dead_ok"] and f["final_ok"] and f["box_ok"]
        assert f["prop_err"] <= 1.0 and f["mu_err"] <= 1.0
        assert f["nwrong"] == 0
        assert (f["ncall"], f["naccept"], f["stuck"]) == (res.ncall[r], res.naccept[r], res.nstuck[r])
        for k in tot:
            tot[k] += f[k]
    assert tot["ndecisions"] > 0 and tot["nnear"] <= nr.NEAR_CAP * tot["ndecisions"]
    if box == "tight":                                 # the faces did cut: some proposals were never evaluated
        assert np.isnan(res.info["trace"][:, :, :, :, D]).any()


@pytest.mark.parametrize("c", REPLAY_CASES, ids=_case_id)
def test_start_logl_is_the_ensemble_kernels_bits(c):
    D, n, kern, nlive, batch, nsteps, nruns, box, seed = c
    res, gp, y, model, b = _device_run(c)
    for r in range(nruns):
        m = (res.run == r) & np.isneginf(res.logLBirth)
        assert m.sum() == nlive
        th, ll = res.points[m], res.logL[m]
        reps = 1 if nlive >= 2 * D else 2               # the ensemble entry wants 2 D walkers at least
        ens = gp.sample_ensemble(y, np.concatenate([th] * reps), 0, b, store=False)
        assert np.array_equal(ens["final_log_prob"][:nlive], ll)


def test_same_call_same_bytes_and_run_independence():
    c = REPLAY_CASES[4]
    res, gp, y, model, b = _device_run(c)
    again = gp.sample_nested(y, b, nlive=c[3], batch=c[4], nsteps=c[5], nruns=c[6], dlogz=0.0, maxBatches=REPLAY_BATCHES,
                             seed=c[8], debug=True)
    for k in ("points", "logL", "logLBirth", "run", "ncall", "naccept", "nstuck"):
        assert getattr(res, k).tobytes() == getattr(again, k).tobytes()
    assert res.info["trace"].tobytes() == again.info["trace"].tobytes() and res.logZ == again.logZ
    one, five = _device_run(c, nruns=1, debug=False)[0], _device_run(c, nruns=5, debug=False)[0]
    for other in (one, five):
        for r in range(min(other.nruns, res.nruns)):
            for k in ("points", "logL", "logLBirth"):
                assert np.array_equal(getattr(other, k)[other.run == r], getattr(res, k)[res.run == r])
    assert not np.array_equal(res.points[res.run == 0][:16], res.points[res.run == 1][:16])


def test_stopping_rule_max_batches_and_final_flush():
    mcmc = _mcmc()
    X, y, gp, b = _gauss(2)
    nlive, batch, dlogz = 64, 8, 0.05
    res = gp.sample_nested(y, b, nlive=nlive, batch=batch, nsteps=10, nruns=3, dlogz=dlogz, maxBatches=400, seed=3)
    for r in range(3):
        m = res.run == r
        l, bt, rec = res.logL[m], res.logLBirth[m], res.info["record"][m]
        nb = int(res.nbatch[r])
        assert 1 <= nb < 400 and len(l) == nb * batch + nlive
        assert np.all(rec[-nlive:] == -1) and np.all(rec[:-nlive] == np.repeat(np.arange(nb), batch))
        assert np.all(np.diff(l[-nlive:]) >= 0.0)
        # the host's recomputation of the criterion before every batch k >= 1: nested_weights over the points written so
        # far plus the live set of that moment (the rows not dead yet that were born by then: birth <= the last L*)
        first = None
        for k in range(1, nb + 1):
            last = l[k * batch - 1]
            rows = np.arange(len(l))
            sel = np.concatenate([rows[:k * batch], rows[k * batch:][bt[k * batch:] <= last]])
            assert len(sel) == k * batch + nlive
            w = mcmc.nested_weights(l[sel], bt[sel])
            assert np.array_equal(w["order"][:k * batch], np.arange(k * batch))
            lz = float(np.logaddexp.reduce(w["logWt"][:k * batch]))
            if np.logaddexp(lz, np.max(l[sel[k * batch:]]) + w["logX"][k * batch - 1]) - lz < dlogz:
                first = k
                break
        print("run %d: stopped after %d batches, host criterion first crossed before batch %s; device logZ %.4f logX %.4f" %
              (r, nb, first, res.info["deviceLogZ"][r], res.info["deviceLogX"][r]))
        assert first is not None and abs(first - nb) <= 1
        lz, lx = nr.run_sums(l[:nb * batch], nlive, batch)            # the run's own sums, by its own rule
        assert abs(lz - res.info["deviceLogZ"][r]) <= 1e-9 and abs(lx - res.info["deviceLogX"][r]) <= 1e-9
    capped = gp.sample_nested(y, b, nlive=nlive, batch=batch, nsteps=2, nruns=2, dlogz=1e-9, maxBatches=7, seed=3)
    assert np.all(capped.nbatch == 7) and len(capped.logL) == 2 * (7 * batch + nlive)
    assert np.all(capped.info["record"].reshape(2, -1)[:, -nlive:] == -1)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
# nsteps of the three problems below, from the CPU (tools/nested_reference.py nsteps: tests/nested_ref.py on the oracle's
# mean, these settings, seeds 21 .. 25, these criteria).  The reference alone passed 5 of 5 at nsteps 10, 20 and 40 on all
# three problems (its misses at 2 and 5 are in DESIGN.md "Nested sampling").  At D = 8 its logZ at 10 and 20 steps sat
# above the truth for 9 seeds of 10, by up to 3 logZErr (+0.18, +0.20): inside the criterion, but a bias; at 40 steps the
# offsets were within 1.1 logZErr.  So D = 8 uses 40, which is also the default max(20, 5 D), and D = 2 uses the default 20.
NSTEPS_D2, NSTEPS_D8, NSTEPS_WELLS = 20, 40, 20
_GAUSS = {}


def _gauss(D):
    import test_gpu_hmc as th
    if D not in _GAUSS:
        _GAUSS[D] = th._gauss_problem(D, 120 if D == 2 else 300, 11 if D == 2 else 12)
    return _GAUSS[D]


def _moments_within(res, mean, cov, mean_err, cov_err):
    """Posterior mean and covariance from logWt within 4 standard errors computed from ess (the reference's own error
    added in quadrature)."""
    p = res.weights()
    sd = np.sqrt(np.diag(cov))
    se_m = sd / np.sqrt(res.ess)
    assert np.all(np.abs(res.mean - mean) <= 4.0 * np.sqrt(se_m ** 2 + np.asarray(mean_err) ** 2))
    # var of a product of two Gaussian coordinates: cov_ii cov_jj + cov_ij^2
    se_c = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / res.ess)
    r = res.points - mean
    c = (r * p[:, None]).T @ r
    assert np.all(np.abs(c - cov) <= 4.0 * np.sqrt(se_c ** 2 + np.asarray(cov_err).reshape(cov.shape) ** 2))


def test_d2_gaussian_against_quadrature():
    X, y, gp, b = _gauss(2)

    def grid(m):
        e = [lo + (np.arange(m) + 0.5) * ((hi - lo) / m) for lo, hi in b]
        pts = np.array(np.meshgrid(*e, indexing="ij")).reshape(2, -1).T
        mu = np.asarray(gp.predict(y, pts, return_cov=False), dtype=np.float64).ravel()
        w = np.exp(mu - mu.max())
        lz = np.log(np.sum(w) * np.prod((b[:, 1] - b[:, 0]) / m)) + mu.max()
        w /= w.sum()
        mean = w @ pts
        return lz, mean, (pts - mean).T @ ((pts - mean) * w[:, None])
    (z1, m1, c1), (z2, m2, c2) = grid(256), grid(512)
    res = gp.sample_nested(y, b, nlive=256, batch=16, nsteps=NSTEPS_D2, nruns=8, dlogz=0.01, seed=21)
    print("logZ %.4f +- %.4f (runs +- %.4f), quadrature %.4f +- %.1e, H %.3f, ess %.0f, efficiency %.3f, stuck %d" %
          (res.logZ, res.logZErr, res.logZRunsErr, z2, abs(z2 - z1), res.H, res.ess, res.efficiency, res.nstuck.sum()))
    assert abs(res.logZ - z2) <= 4.0 * np.sqrt(res.logZErr ** 2 + (z2 - z1) ** 2)
    _moments_within(res, m2, c2, np.abs(m2 - m1), np.abs(c2 - c1))


def test_d8_gaussian_against_evidence():
    from approxposterior_amd import approx
    D = 8
    X, y, gp, b = _gauss(D)
    ap = approx.ApproxPosterior(theta=X, y=y, gp=gp, lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                                priorSample=lambda m: np.random.uniform(b[:, 0], b[:, 1], size=(m, D)), bounds=b,
                                algorithm="agp", distributed=False)
    # a mixture proposal of high ess: one Gaussian with the box estimate's own moments, widened
    box = ap.evidence(nSamples=2 ** 21, proposal="box", seed=1)
    ev = ap.evidence(nSamples=2 ** 19, proposal=([1.0], [box["mean"]], [np.asarray(box["cov"])]), covScale=1.5, seed=2)
    assert ev["ess"] >= 0.2 * 2 ** 19
    res = ap.runNested(nlive=256, batch=16, nsteps=NSTEPS_D8, nruns=8, dlogz=0.01, seed=22)
    assert res is ap.nested
    print("logZ %.4f +- %.4f (runs +- %.4f), evidence() %.4f +- %.4f (ess %.0f), H %.3f, ess %.0f, efficiency %.3f, stuck %d"
          % (res.logZ, res.logZErr, res.logZRunsErr, ev["logZ"], ev["logZErr"], ev["ess"], res.H, res.ess, res.efficiency,
             res.nstuck.sum()))
    assert abs(res.logZ - ev["logZ"]) <= 4.0 * np.sqrt(res.logZErr ** 2 + ev["logZErr"] ** 2)
    cov = np.asarray(ev["cov"])
    sd = np.sqrt(np.diag(cov))
    _moments_within(res, np.asarray(ev["mean"]), cov, sd / np.sqrt(ev["ess"]),
                    np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / ev["ess"]))


def test_two_wells_against_quadrature():
    import test_gpu_tempering as tt
    z = tt._two_wells()
    gp, y, truth, qerr = z["gp"], z["y"], z["truth"], z["qerr"]
    b = np.array(z["bounds"], dtype=np.float64)
    nlive, nruns = 256, 8
    res = gp.sample_nested(y, b, nlive=nlive, batch=16, nsteps=NSTEPS_WELLS, nruns=nruns, dlogz=0.01, seed=23)
    lz, lzerr = float(truth["logint"][0]), float(qerr["logint"][0])
    p = res.weights()
    mass = float(np.sum(p[res.points[:, 0] > 0.0]))
    tm = float(truth["mass"])
    # the error bar of a well's mass: the live points split between the wells binomially when the wells separate, and
    # the posterior weights add their own scatter (ess)
    merr = np.sqrt(tm * (1.0 - tm) * (1.0 / (nlive * nruns) + 1.0 / res.ess) + float(qerr["mass"]) ** 2)
    print("logZ %.4f +- %.4f (runs +- %.4f), quadrature %.4f +- %.1e; mass of the second well %.4f +- %.4f, quadrature %.4f; "
          "H %.3f, ess %.0f, efficiency %.3f, stuck %d" % (res.logZ, res.logZErr, res.logZRunsErr, lz, lzerr, mass, merr, tm,
                                                         res.H, res.ess, res.efficiency, res.nstuck.sum()))
    assert abs(res.logZ - lz) <= 4.0 * np.sqrt(res.logZErr ** 2 + lzerr ** 2)
    assert abs(mass - tm) <= 4.0 * merr


# ---------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True], ids=["box", "joint-prior"])
def test_run_nested_api(joint):
    import test_gpu_hmc as th
    import approxposterior_amd as apm
    ap = th._ap(joint)
    p0 = np.random.RandomState(2).uniform(-0.2, 0.2, size=(16, 2))
    np.random.seed(4)
    ap.runMCMC(samplerKwargs={"nwalkers": 16}, mcmcKwargs={"iterations": 50, "initial_state": p0}, cache=False,
               estBurnin=False, thinChains=False, onDevice=True)
    sampler = ap.sampler
    chain = sampler.get_chain().copy()
    res = apm.runNested(ap, nlive=64, batch=8, nsteps=10, nruns=4, dlogz=0.1, seed=5)
    assert res is ap.nested and isinstance(res, _mcmc().NestedResult)
    assert ap.sampler is sampler and np.array_equal(sampler.get_chain(), chain)
    b = np.asarray(ap.bounds, dtype=np.float64)
    assert np.all((res.points >= b[:, 0]) & (res.points <= b[:, 1]))
    assert res.logVolume == float(np.sum(np.log(b[:, 1] - b[:, 0]))) and res.nruns == 4 and res.logZRuns.shape == (4,)
    assert np.isfinite(res.logZ) and res.logZErr > 0.0 and res.H > 0.0 and 0.0 < res.efficiency <= 1.0
    again = ap.runNested(nlive=64, batch=8, nsteps=10, nruns=4, dlogz=0.1, seed=5)
    assert again.logZ == res.logZ and np.array_equal(again.points, res.points)
    np.random.seed(8)
    a = ap.runNested(nlive=64, batch=8, nsteps=10, nruns=2, dlogz=0.1)
    np.random.seed(8)
    c = ap.runNested(nlive=64, batch=8, nsteps=10, nruns=2, dlogz=0.1)
    assert a.logZ == c.logZ and a.logZ != res.logZ
    eq = res.samples_equal(2000, seed=1)
    se = np.sqrt(np.diag(res.cov)) * np.sqrt(1.0 / 2000 + 1.0 / res.ess)
    assert eq.shape == (2000, 2) and np.all(np.abs(eq.mean(axis=0) - res.mean) <= 4.0 * se)
    assert np.all(np.abs(eq.var(axis=0) - np.diag(res.cov)) <= 4.0 * np.diag(res.cov) * np.sqrt(2.0 * (1.0 / 2000 + 1.0 / res.ess)))
    default = ap.gp.sample_nested(ap.y, b, nlive=16, batch=4, nsteps=2, dlogz=0.0, maxBatches=2)     # nruns from the device
    import torch
    assert default.nruns == torch.cuda.get_device_properties(0).multi_processor_count
    for bad in (dict(nlive=16, batch=16), dict(batch=17), dict(dlogz=-1.0), dict(nsteps=0), dict(nruns=0), dict(maxBatches=0)):
        with pytest.raises(ValueError):
            ap.runNested(**bad)
    assert ap.nested is c
