# -*- coding: utf-8 -*-
"""CPU: the nested sampler's accounting (mcmc.nested_weights, mcmc.NestedResult) against exact nested sampling of a
Gaussian in a box and against hand-built arrays; the NumPy restatement of the whole run (tests/nested_ref.py) on an
analytic two-well target; and the argument checks of the entry points, which run before anything reaches a device."""
import ctypes

import numpy as np
import pytest

import nested_ref as nr
from approxposterior_amd import _lib
from approxposterior_amd import gp as agp
from approxposterior_amd import mcmc

# ---- 1. the accounting alone -----------------------------------------------------------------------------------------
D_ACC, S_ACC, R_ACC, NLIVE_ACC, NSEEDS, NRUNS = 2, 0.3, 2.0, 32, 20, 16
_EXACT = {}


def _exact(batch):
    """NSEEDS x NRUNS exact runs at this batch size (built once, shared): lists of (logL, birth)."""
    if batch not in _EXACT:
        nb = -(-11 * NLIVE_ACC // batch)            # down to logX = -11: the live points left hold e^-11 V of the box
        _EXACT[batch] = [[nr.exact_run(np.random.RandomState(7000 + 100 * batch + 17 * s + r), D_ACC, S_ACC, R_ACC,
                                       NLIVE_ACC, batch, nb) for r in range(NRUNS)] for s in range(NSEEDS)]
    return _EXACT[batch]


def _merge(runs):
    return (np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]),
            np.concatenate([np.full(len(r[0]), k) for k, r in enumerate(runs)]))


@pytest.mark.parametrize("batch", [1, 4, 16])
def test_exact_gaussian_evidence_within_its_error_and_merges_shrink(batch):
    truth = nr.IsoGaussian(np.zeros(D_ACC), S_ACC).truth([-R_ACC] * D_ACC, [R_ACC] * D_ACC)
    est = {}
    for k in (1, 4, 16):
        vals = []
        for s in range(NSEEDS):
            w = mcmc.nested_weights(*_merge(_exact(batch)[s][:k]))
            print("batch %d, %2d runs, seed %2d: logZ - truth %+.4f, logZErr %.4f, H %.3f" % (batch, k, s, w["logZ"] - truth,
                                                                                             w["logZErr"], w["H"]))
            assert abs(w["logZ"] - truth) <= 4.0 * w["logZErr"]
            vals.append(w["logZ"])
        est[k] = np.std(vals, ddof=1)
    # the standard deviation of NSEEDS values is known to 1 / sqrt(2 (NSEEDS - 1)) of itself; a ratio of two to sqrt 2 more
    tol = 4.0 * np.sqrt(2.0 / (2.0 * (NSEEDS - 1)))
    for k in (4, 16):
        print("batch %d: spread of %2d merged runs x sqrt(runs) / spread of one run = %.3f" % (batch, k, est[k] * np.sqrt(k) / est[1]))
        assert abs(np.log(est[k] * np.sqrt(k) / est[1])) <= tol


def test_vectorised_accounting_is_the_definition():
    runs = _exact(4)[0][:3]
    l, b, r = _merge(runs)
    w, d = mcmc.nested_weights(l, b, r), nr.weights(l, b, r)
    assert np.array_equal(w["order"], d["order"])
    assert np.array_equal(w["nlive"][w["order"]], d["nlive"])
    assert np.allclose(w["logX"][w["order"]], d["logX"], rtol=0, atol=1e-12)
    assert np.allclose(w["logWt"][w["order"]], d["logWt"], rtol=0, atol=1e-11)
    assert abs(w["logZ"] - d["logZ"]) <= 1e-12 and abs(w["H"] - d["H"]) <= 1e-9 and abs(w["logZErr"] - d["logZErr"]) <= 1e-9


def test_ties_flush_counts_and_one_run_merge():
    # ties: equal logL die in (run, serial) order, each with one live point fewer
    w = mcmc.nested_weights([1.0, 1.0, 2.0, 1.0], [-np.inf] * 4)
    assert np.array_equal(w["order"], [0, 1, 3, 2]) and np.array_equal(w["nlive"], [4, 3, 1, 2])
    w = mcmc.nested_weights([1.0, 1.0, 1.0, 1.0], [-np.inf] * 4, run=[1, 0, 1, 0])
    assert np.array_equal(w["order"], [1, 3, 0, 2]) and np.array_equal(w["nlive"], [2, 4, 1, 3])
    # a point born AT a threshold is not live at a point of that same logL (its birth is not below it)
    w = mcmc.nested_weights([0.0, 1.0, 2.0, 1.5], [-np.inf, -np.inf, -np.inf, 1.0])
    assert np.array_equal(w["nlive"], [3, 2, 1, 2])
    assert np.allclose(w["logX"], [-1 / 3, -1 / 3 - 1 / 2, -1 / 3 - 1 / 2 - 1 / 2 - 1, -1 / 3 - 1 / 2 - 1 / 2])
    # a batched run: n, n - 1, ... inside a batch; the final flush n, n - 1, ..., 1; two merged runs: the counts add
    l, b = _exact(4)[1][0]
    w = mcmc.nested_weights(l, b)
    n = w["nlive"]
    assert np.array_equal(n[:8], [32, 31, 30, 29, 32, 31, 30, 29])
    assert np.array_equal(n[-NLIVE_ACC:], np.arange(NLIVE_ACC, 0, -1))
    l2, b2, r2 = _merge(_exact(4)[1][:2])
    w2 = mcmc.nested_weights(l2, b2, r2)
    assert w2["nlive"][w2["order"]][0] == 64 and np.array_equal(np.sort(w2["nlive"])[:2], [1, 2])
    # a one-run merge is the plain run, bit for bit
    w1 = mcmc.nested_weights(l, b, run=np.zeros(len(l), dtype=int))
    for k in ("order", "nlive", "logX", "logWt"):
        assert np.array_equal(w[k], w1[k])
    assert w["logZ"] == w1["logZ"] and w["logZErr"] == w1["logZErr"] and w["H"] == w1["H"]
    with pytest.raises(ValueError):
        mcmc.nested_weights([1.0, np.nan], [-np.inf, -np.inf])
    with pytest.raises(ValueError):
        mcmc.nested_weights([1.0, 2.0], [-np.inf])


def test_nested_result_moments_and_resampling():
    rs = np.random.RandomState(3)
    runs = [nr.run_one(nr.IsoGaussian([0.3, -0.2], 0.25), [-2, -2], [2, 2], np.ones(2), 64, 4, 10, 400, 0.01, 5, r) for r in range(4)]
    res = mcmc.NestedResult(*nr.merged(runs), logVolume=np.log(16.0),
                            counts=[[r["nbatch"], r["ncall"], r["naccept"], r["nstuck"]] for r in runs], nlive=64)
    truth = nr.IsoGaussian([0.3, -0.2], 0.25).truth([-2, -2], [2, 2]) + np.log(16.0)
    print("logZ %.4f +- %.4f (runs: +- %.4f), truth %.4f, ess %.0f, efficiency %.3f" % (res.logZ, res.logZErr, res.logZRunsErr,
                                                                                      truth, res.ess, res.efficiency))
    assert abs(res.logZ - truth) <= 4.0 * res.logZErr and res.logZRuns.shape == (4,)
    se = 0.25 / np.sqrt(res.ess)
    assert np.all(np.abs(res.mean - [0.3, -0.2]) <= 4.0 * se)
    assert np.all(np.abs(np.diag(res.cov) - 0.0625) <= 4.0 * 0.0625 * np.sqrt(2.0 / res.ess))
    assert 0.0 < res.efficiency <= 1.0 and np.all(res.ncall > 64)
    eq = res.samples_equal(4000, seed=1)
    assert eq.shape == (4000, 2) and np.array_equal(eq, res.samples_equal(4000, seed=1))
    assert np.all(np.abs(eq.mean(axis=0) - res.mean) <= 4.0 * 0.25 / np.sqrt(4000) + 1e-3)
    assert np.all(np.abs(eq.var(axis=0) - np.diag(res.cov)) <= 0.2 * 0.0625)
    assert len(res.samples_equal()) == int(res.ess)
    del rs


# ---- 2. the full reference run ---------------------------------------------------------------------------------------
TW = nr.TwoWell([-1.2, 0.3], [1.4, -0.8], 0.25, 0.15, 2.0)
TW_BOX = ([-3.0, -3.0], [3.0, 3.0])
TW_ARGS = dict(nlive=64, batch=4, nsteps=10, maxBatches=2000, dlogz=0.02)
_TW = {}


def _tw(seed, nruns, **kw):
    key = (seed, nruns, tuple(sorted(kw.items())))
    if key not in _TW:
        a = dict(TW_ARGS, **kw)
        _TW[key] = nr.run(TW, TW_BOX[0], TW_BOX[1], np.ones(2), a["nlive"], a["batch"], a["nsteps"], a["maxBatches"], a["dlogz"],
                          seed, nruns)
    return _TW[key]


def test_reference_run_finds_both_wells_and_stops_at_dlogz():
    runs = _tw(11, 5)
    res = mcmc.NestedResult(*nr.merged(runs))
    truth, m1 = TW.truth(*TW_BOX), TW.mass1(*TW_BOX)
    p = res.weights()
    got = float(np.sum(p[res.points[:, 0] > 0.0]))
    print("logZ %.4f +- %.4f, truth %.4f; mass of well 1: %.4f, truth %.4f, ess %.0f; batches %s" %
          (res.logZ, res.logZErr, truth, got, m1, res.ess, [r["nbatch"] for r in runs]))
    assert abs(res.logZ - truth) <= 4.0 * res.logZErr
    # the error bar of a well's mass: the live points split between the wells binomially when the wells separate
    # (5 x 64 live points in all), and the posterior weights add their own scatter (ess)
    assert abs(got - m1) <= 4.0 * np.sqrt(m1 * (1.0 - m1) * (1.0 / (5 * 64) + 1.0 / res.ess))
    for r in runs:
        assert 1 <= r["nbatch"] < TW_ARGS["maxBatches"]
        assert len(r["logL"]) == r["nbatch"] * 4 + 64 and np.all(r["rec"][-64:] == -1)
        assert np.all(np.diff(r["logL"][-64:]) >= 0.0)
        # the rule: not yet at the batch before, crossed at the stop
        lz, lx = nr.run_sums(r["logL"][:r["nbatch"] * 4], 64, 4)
        assert abs(lz - r["logZ"]) <= 1e-9 and abs(lx - r["logX"]) <= 1e-9
        w = nr.weights(r["logL"], r["birth"])                     # (a run's rows are already in the order of the accounting)
        assert np.array_equal(w["order"], np.arange(len(r["logL"])))
        # the accounting's counts are the run's own but for exact ties split by a batch boundary (nested_ref.run_sums)
        assert abs(np.logaddexp.reduce(w["logWt"][:r["nbatch"] * 4]) - r["logZ"]) <= 0.02
        assert nr.logaddexp(r["logZ"], r["logL"][-1] + r["logX"]) - r["logZ"] < TW_ARGS["dlogz"]


def test_reference_run_stops_at_max_batches_seeds_and_run_independence():
    a = _tw(11, 1, dlogz=0.0, maxBatches=30)[0]
    assert a["nbatch"] == 30 and len(a["logL"]) == 30 * 4 + 64
    r3, r5 = _tw(11, 3), _tw(11, 5)
    for k in range(3):
        for key in ("points", "logL", "birth", "rec"):
            assert np.array_equal(r3[k][key], r5[k][key])
    again = nr.run(TW, TW_BOX[0], TW_BOX[1], np.ones(2), 64, 4, 10, 2000, 0.02, 11, 1)[0]
    assert np.array_equal(again["points"], r5[0]["points"]) and again["logZ"] == r5[0]["logZ"]
    other = _tw(12, 1)[0]
    assert not np.array_equal(other["points"][:64], r5[0]["points"][:64])
    assert not np.array_equal(r5[0]["points"][:64], r5[1]["points"][:64])


# ---- 3. argument checks, without a device ----------------------------------------------------------------------------
def test_python_argument_checks():
    ok = dict(D=2, bounds=[(-1, 1), (-2, 2)], nlive=64, batch=16, nsteps=None, nruns=None, dlogz=0.01, maxBatches=None,
              sigma=1e-5, gamma0=None)
    b, nlive, batch, nsteps, nruns, dlogz, mb, sigma, g0 = agp.GP._nested_arguments(**ok)
    assert (nlive, batch, nsteps, nruns, mb, g0) == (64, 16, 20, None, 200, 0.0) and b.shape == (2, 2)
    for bad in (dict(batch=0), dict(batch=17), dict(nlive=3, batch=1), dict(nlive=31), dict(nlive=4097), dict(nsteps=0),
                dict(nruns=0), dict(dlogz=-1.0), dict(dlogz=np.nan), dict(dlogz=np.inf), dict(sigma=-1.0), dict(gamma0=-1.0),
                dict(gamma0=np.inf), dict(maxBatches=0), dict(bounds=[(-1, 1)]), dict(bounds=[(-1, 1), (2, 2)]),
                dict(bounds=[(-1, np.inf), (-2, 2)]), dict(bounds=[(-np.inf, 1), (-2, 2)]), dict(bounds=[(np.nan, 1), (-2, 2)])):
        with pytest.raises(ValueError):
            agp.GP._nested_arguments(**dict(ok, **bad))
    gp = agp.GP(kernel=agp.ExpSquaredKernel([1.0, 1.0], ndim=2))
    with pytest.raises(ValueError):
        gp.sample_nested(np.zeros(3), [(-1, 1), (-np.inf, 2)])
    with pytest.raises(ValueError):
        gp.sample_nested(np.zeros(3), [(-1, 1), (-2, 2)], nlive=16, batch=16)


def test_run_nested_refuses_an_infinite_box_and_is_exported():
    import approxposterior_amd as ap
    from approxposterior_amd import approx, priors as P
    assert ap.runNested is ap.ApproxPosterior.runNested
    X = np.random.RandomState(0).uniform(-1, 1, size=(10, 2))
    y = -np.sum(X * X, axis=1)
    gp = agp.GP(kernel=agp.ExpSquaredKernel([1.0, 1.0], ndim=2))

    def make(lnprior, bounds, sample):
        return approx.ApproxPosterior(theta=X.copy(), y=y.copy(), gp=gp, lnprior=lnprior, lnlike=lambda t, *a, **k: 0.0,
                                      priorSample=sample, bounds=bounds, algorithm="agp", distributed=False)
    a = make(lambda t: 0.0, [(-1, 1), (-np.inf, 1)], lambda m: np.zeros((int(m), 2)))
    with pytest.raises(ValueError):
        a.runNested(nruns=1)
    J = P.JointPrior([P.UniformPrior(-1.0, 1.0), P.GaussianPrior(0.0, 1.0)])
    a = make(J, [(-1, 1), (-np.inf, np.inf)], J.sample)          # the Gaussian factor's support is the whole line
    with pytest.raises(ValueError):
        a.runNested(nruns=1)
    a = make(J, [(-1, 1), (-3, 3)], J.sample)
    with pytest.raises(ValueError):
        a.runNested(nruns=1, nlive=8, batch=8)                   # refused before a device is asked for
    assert not hasattr(a, "nested") or a.nested is None


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.apgp_nested_work_len(2, 64, 3) == 3 * 64 * 3 and lib.apgp_nested_work_len(8, 4096, 1) == 4096 * 9
    for bad in ((0, 64, 1), (_lib.MAX_DIM + 1, 64, 1), (2, 3, 1), (2, 4097, 1), (2, 64, 0)):
        assert lib.apgp_nested_work_len(*bad) == -1
    # the switch of the training stream between LDS and L2: 96 KiB of Npad x (DPAD + 2) doubles
    assert lib.apgp_nested_xlds(3072, 2) == 1 and lib.apgp_nested_xlds(3073, 2) == 0
    assert lib.apgp_nested_xlds(1024, 8) == 1 and lib.apgp_nested_xlds(1025, 8) == 0
    assert lib.apgp_nested_xlds(512, 9) == 1 and lib.apgp_nested_xlds(513, 9) == 0
    assert lib.apgp_nested_xlds(0, 2) == -1 and lib.apgp_nested_xlds(10, 0) == -1
    ks = _lib.KernelStruct()
    ks.ndim, ks.amp = 2, 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    arr = ctypes.c_double * _lib.MAX_DIM
    lo, hi = arr(*([-1.0] * _lib.MAX_DIM)), arr(*([1.0] * _lib.MAX_DIM))
    ok = dict(xs=p, n=4, ks=ctypes.byref(ks), lo=lo, hi=hi, nlive=64, batch=16, nsteps=5, mb=10, dlogz=0.01, sigma=1e-5,
              g0=0.0, nruns=2, work=p, points=p, logl=p, birth=p, rec=p, counts=p, logz=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.apgp_nested_sample(a["xs"], a["n"], a["ks"], 0.0, a["lo"], a["hi"], a["nlive"], a["batch"], a["nsteps"],
                                      a["mb"], a["dlogz"], a["sigma"], a["g0"], a["nruns"], 1, a["work"], a["points"],
                                      a["logl"], a["birth"], a["rec"], a["counts"], a["logz"], None, None)
    for name in ("xs", "ks", "lo", "hi", "work", "points", "logl", "birth", "rec", "counts", "logz"):
        assert call(**{name: None}) == -1 and b"apgp_nested_sample" in lib.apgp_last_error(), name
    inf_hi, empty, nan_lo = arr(*([1.0] * _lib.MAX_DIM)), arr(*([1.0] * _lib.MAX_DIM)), arr(*([-1.0] * _lib.MAX_DIM))
    inf_hi[1], empty[0], nan_lo[0] = float("inf"), -1.0, float("nan")
    for kw in (dict(n=0), dict(n=(1 << 24) + 1), dict(nlive=3, batch=1), dict(nlive=4097), dict(nlive=31), dict(batch=0),
               dict(batch=17), dict(nsteps=0), dict(mb=0), dict(nruns=0), dict(dlogz=-0.1), dict(dlogz=float("nan")),
               dict(dlogz=float("inf")), dict(sigma=-1.0), dict(g0=float("nan")), dict(g0=-1.0), dict(hi=inf_hi),
               dict(hi=empty), dict(lo=nan_lo)):
        assert call(**kw) == -1, kw
    ks.amp = 0.0
    assert call() == -1
    ks.amp, ks.ndim = 1.0, _lib.MAX_DIM + 1
    assert call() == -1
