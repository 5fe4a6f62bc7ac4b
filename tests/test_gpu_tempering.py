"""MI355X: parallel tempering of the device ensemble sampler (csrc/tempering.hip, GP.sample_tempered,
mcmc.TemperedChain, runMCMC(tempering=...)).

* A ladder of one rung beta = 1 IS the ensemble sampler: bit for bit, through segment boundaries.
* Every move and every exchange of small ladders is replayed against the NumPy restatement (tests/tempering_ref.py) with
  the oracle's GP mean, teacher-forced as test_gpu_ensemble_moves.py replays the moves and with its near-tie rule: a
  decision is a near-tie when |log u - rhs| <= 1e-8 max(1, S) or the proposal lies within 1e-12 (of the span) of a face.
* On a two-well surrogate whose wells a single-temperature ensemble cannot cross, the rungs' means of mu, the cold chain's
  mass in the second well and the thermodynamic-integration evidence agree with quadrature of GP.predict.
Problems, starts, bounds and the oracle are those of test_gpu_ensemble_replay.py."""
import ctypes

import numpy as np
import pytest

import ensemble_moves_ref as emr
import tempering_ref as tr
import test_gpu_ensemble_replay as rp

pytestmark = pytest.mark.gpu

MIX = [(("stretch", 2.0), .4), (("de", 1e-5, None), .4), (("snooker", 1.7), .2)]


def _mcmc():
    from approxposterior_amd import mcmc
    return mcmc


def _objects(spec):
    mcmc = _mcmc()
    make = {"stretch": lambda m: mcmc.StretchMove(m[1]), "de": lambda m: mcmc.DEMove(m[1], m[2] if len(m) > 2 else None),
            "snooker": lambda m: mcmc.DESnookerMove(m[1])}
    if isinstance(spec[0], str):
        return make[spec[0]](spec)
    return [(make[m[0][0]](m[0]), m[1]) for m in spec]


def _ties(margin, face, S):
    return (margin <= 1e-8 * max(1.0, S)) | (face <= 1e-12)


def _single_workgroup(gp, y, p0, iters, b, seed, moves):
    """GP.sample_ensemble on the single-workgroup kernel: apgp_ensemble_sample_moves(mode = 1, nensembles = len(p0))."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    prev = lib.apgp_ensemble_mode(1)
    try:
        return gp.sample_ensemble(y, p0, iters, b, seed=seed, moves=moves)
    finally:
        lib.apgp_ensemble_mode(prev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. one rung
# ---------------------------------------------------------------------------------------------------------------------
# D, W, n, L, kernel.  n = 600 at D = 8 stages the training stream in LDS, n = 1536 (120 KiB) leaves it in L2; D = 12 takes the
# one-proposal path.  W = 2 cannot hold DE or the snooker: its "mixture" is a stretch move at another scale.
IDENTITY = [(1, 2, 40, 3, "se"), (2, 8, 90, 3, "amp"), (8, 64, 600, 2, "se"), (8, 16, 1536, 2, "amp"), (12, 24, 200, 2, "amp")]


@pytest.mark.parametrize("mixture", [False, True], ids=["default", "mixture"])
@pytest.mark.parametrize("D,W,n,L,kern", IDENTITY, ids=["D%d-W%d-n%d" % c[:3] for c in IDENTITY])
def test_one_rung_is_the_ensemble_sampler_bit_for_bit(D, W, n, L, kern, mixture):
    """betas = [1], 37 iterations in segments of 5 (a tail segment of 2): chain, log_prob, coords, final log_prob and
    naccept equal the single-workgroup ensemble kernel's for L ensembles, bit for bit."""
    seed = 2 ** 32 + 19
    X, y, gp, gpo = rp._problem(D, n, kern, seed)
    p0, b = rp._start(L, W, D, seed), rp._bounds(D)
    spec = None if not mixture else (MIX if W >= 6 else ("stretch", 1.5))
    moves = None if spec is None else _objects(spec)
    want = _single_workgroup(gp, y, p0, 37, b, seed, moves)
    got = gp.sample_tempered(y, p0[:, None], 37, b, [1.0], swapEvery=5, seed=seed, ladders=L, moves=moves)
    for key in ("chain", "log_prob", "coords", "final_log_prob", "naccept"):
        assert np.array_equal(got[key], want[key]), "%s differs from the ensemble sampler" % key
    assert want["naccept"].sum() > 0 and got["swap_proposed"].shape == (L, 0)
    assert np.array_equal(got["rung_mean_log_prob"][:, :, 0], want["log_prob"].reshape(37, L, W).mean(axis=2)) or \
        np.allclose(got["rung_mean_log_prob"][:, :, 0], want["log_prob"].reshape(37, L, W).mean(axis=2), rtol=1e-13, equal_nan=True)


@pytest.mark.parametrize("D,W,n,L,kern", [(2, 8, 90, 2, "amp"), (8, 64, 600, 1, "se")])
def test_cold_rungs_without_an_exchange_are_independent_ensembles(D, W, n, L, kern):
    """betas = [1, 1, 1] with swap_every > iterations: no exchange round, the 3 L rungs are ensembles 0 .. 3 L - 1."""
    seed = 41
    X, y, gp, gpo = rp._problem(D, n, kern, seed)
    p0, b = rp._start(3 * L, W, D, seed), rp._bounds(D)
    want = _single_workgroup(gp, y, p0, 30, b, seed, _objects(MIX))
    got = gp.sample_tempered(y, p0.reshape(L, 3, W, D), 30, b, [1.0, 1.0, 1.0], swapEvery=31, seed=seed, ladders=L,
                             storeRungs=3, moves=_objects(MIX), swapLog=True)
    assert np.array_equal(got["rung_chain"].reshape(30, 3 * L * W, D), want["chain"])
    assert np.array_equal(got["rung_log_prob"].reshape(30, 3 * L * W), want["log_prob"])
    assert np.array_equal(got["rung_coords"].reshape(3 * L * W, D), want["coords"])
    assert np.array_equal(got["rung_final_log_prob"].reshape(-1), want["final_log_prob"])
    assert np.array_equal(got["rung_naccept"].reshape(-1), want["naccept"])
    assert got["swap_log"].shape == (0, L, 2, W) and not got["swap_proposed"].any() and not got["swap_accepted"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. replay
# ---------------------------------------------------------------------------------------------------------------------
# T, D, W, swap_every, L, n, kernel, moves, seed: every T of 2 .. 5 (odd T: a rung sits every round out), W = 2 D and 64,
# D = 2 and 8, swap_every 1 and 3.  The seeds are such that the reference's free run meets few enough near-ties (checked).
REPLAY = [
    (2, 2, 4, 1, 2, 120, "se", None, 17),
    (3, 2, 64, 3, 1, 120, "amp", MIX, 8),
    (4, 8, 16, 1, 1, 300, "se", None, 9),
    (5, 8, 64, 3, 1, 300, "amp", None, 10),
    (3, 8, 16, 3, 2, 300, "amp", MIX, 11),
    (5, 2, 4, 1, 1, 120, "se", None, 12),
    (2, 8, 64, 1, 1, 300, "se", MIX, 13),
    (4, 2, 64, 3, 1, 120, "amp", None, 24),
]


@pytest.mark.parametrize("T,D,W,se,L,n,kern,spec,seed", REPLAY, ids=["T%d-D%d-W%d-every%d" % c[:4] for c in REPLAY])
def test_ladder_replays_move_by_move_and_exchange_by_exchange(T, D, W, se, L, n, kern, spec, seed):
    N = 60
    X, y, gp, gpo = rp._problem(D, n, kern, seed)
    b, sc = rp._bounds(D), rp._scales(gp, D)
    lp, S = rp._oracle(gpo, y, D), rp._size(gpo, y, X)
    betas = _mcmc().tempering_ladder(T, 0.05)
    tab = emr.table(spec if spec is not None else ("stretch", 2.0), D)
    p0 = rp._start(L * T, W, D, seed).reshape(L, T, W, D)
    # before anything goes to the device: the reference's own free run on these seeds
    free = tr.run(lp, p0, N, b, tab, betas, se, seed=seed, sc=sc, ladders=L)
    ftie = int(_ties(free["decisions"]["margin"], free["decisions"]["face"], S).sum())
    assert ftie * 10 ** 4 <= free["decisions"]["margin"].size, "the reference meets %d near-ties" % ftie
    assert not (free["decisions"]["swap_margin"] <= 1e-8 * max(1.0, S)).any(), "the reference meets an exchange near-tie"
    assert free["swap_acc"].sum() > 0 and (free["swap_log"] == 1).sum() > 0

    moves = None if spec is None else _objects(spec)
    dev = gp.sample_tempered(y, p0, N, b, betas, swapEvery=se, seed=seed, ladders=L, storeRungs=T, moves=moves, swapLog=True)
    ch, mu = dev["rung_chain"], dev["rung_log_prob"]
    assert ch.shape == (N, L, T, W, D) and mu.shape == (N, L, T, W)
    assert not np.isnan(ch).any() and not np.isnan(mu).any()
    f = tr.forced(lp, p0, ch, dev["swap_log"], b, tab, betas, se, seed=seed, sc=sc)

    # exchanges: the device's log against the reference's decision from the same positions
    R = tr.rounds_of(N, se)
    log, ref = dev["swap_log"], f["swaps"]
    assert log.shape == (R, L, T - 1, W)
    stie = ref["margin"] <= 1e-8 * max(1.0, S)
    assert not stie.any(), "an exchange near-tie"
    assert np.array_equal(log, ref["log"]), "%d exchange decisions differ from the replay" % (log != ref["log"]).sum()
    for r in range(R):
        assert not log[r, :, (r + 1) % 2::2].any(), "a pair that sits round %d out has a logged decision" % r
    assert np.array_equal(dev["swap_proposed"], (log >= 1).sum(axis=(0, 3)))
    assert np.array_equal(dev["swap_accepted"], (log == 2).sum(axis=(0, 3)))
    assert (log == 2).sum() > 0 and (log == 1).sum() > 0

    # moves: every half-step of every rung against the forced replay
    m = f["moves"]
    w = m["walker"].reshape(L, T, N, 2, W // 2)
    t = np.arange(N)[None, None, :, None, None]
    li, ki = np.arange(L)[:, None, None, None, None], np.arange(T)[None, :, None, None, None]
    before, after = f["prev"][t, li, ki, w], ch[t, li, ki, w]
    moved = np.any(after != before, axis=-1)
    moved[:, :, 0] = np.any(np.abs(after[:, :, 0] - before[:, :, 0]) > np.spacing(np.abs(before[:, :, 0])), axis=-1)   # (x sc) / sc
    acc = m["accept"].reshape(moved.shape)
    tie = _ties(m["margin"], m["face"], S).reshape(moved.shape)
    bad = (moved != acc) & ~tie
    assert not bad.any(), "%d move decisions differ from the replay (first at %s)" % (bad.sum(), np.argwhere(bad)[0])
    assert int(tie.sum()) * 10 ** 4 <= tie.size, "%d near-ties in %d proposals" % (tie.sum(), tie.size)
    both = moved & acc
    lpq = m["lpq"].reshape(moved.shape)
    assert np.all(np.abs(mu[t, li, ki, w][both] - lpq[both]) <= 1e-9 * S), "stored mu of an accepted move"
    # (the positions' rounding bounds are test_gpu_ensemble_moves.py's subject; here: the stored row is the proposal)
    q = m["q"].reshape(moved.shape + (D,))
    assert np.all(np.abs(after - q)[both] <= 1e-9 * np.maximum(1.0, np.abs(q[both]))), "stored position of an accepted move"
    # mu rides along with an exchange, and a walker that did not move keeps it to the bit
    still = ~moved & ~acc
    still[:, :, 0] = False
    prev_mu = np.concatenate([np.full((1, L, T, W), np.nan), mu[:-1]], axis=0)
    for r in range(R):
        tr.apply_exchange(log[r], (prev_mu[(r + 1) * se],))
    assert np.array_equal(mu[t, li, ki, w][still], prev_mu[t, li, ki, w][still]), "mu of a walker that stayed"
    # the accept counters stay with the rung
    count = np.zeros((L, T, W), dtype=np.int64)
    np.add.at(count, (np.broadcast_to(li, w.shape)[moved], np.broadcast_to(ki, w.shape)[moved], w[moved]), 1)
    assert np.array_equal(dev["rung_naccept"], count), "rung_naccept is not the number of moves the chain shows"
    assert np.array_equal(dev["rung_coords"], ch[-1]) and np.array_equal(dev["rung_final_log_prob"], mu[-1])
    assert np.array_equal(dev["rung_mean_log_prob"], mu.mean(axis=3)) or \
        np.allclose(dev["rung_mean_log_prob"], mu.mean(axis=3), rtol=1e-13, atol=0, equal_nan=True)

    # storing the cold rung alone changes nothing
    cold = gp.sample_tempered(y, p0, N, b, betas, swapEvery=se, seed=seed, ladders=L, moves=moves)
    assert np.array_equal(cold["chain"], ch[:, :, 0].reshape(N, L * W, D)) and np.array_equal(cold["chain"], dev["chain"])
    assert np.array_equal(cold["log_prob"], mu[:, :, 0].reshape(N, L * W))
    assert np.array_equal(cold["swap_accepted"], dev["swap_accepted"]) and "rung_chain" not in cold
    print("T %d D %d W %d every %d: %d near-ties in %d proposals, exchanges accepted %s of %s, move acceptance per rung %s" % (
        T, D, W, se, tie.sum(), tie.size, dev["swap_accepted"].sum(axis=0), dev["swap_proposed"].sum(axis=0),
        np.round(dev["rung_naccept"].mean(axis=(0, 2)) / N, 2)))


# ---------------------------------------------------------------------------------------------------------------------
# 3. equal betas
# ---------------------------------------------------------------------------------------------------------------------
def test_equal_betas_accept_every_proposed_exchange():
    D, W, N, L, seed = 2, 8, 25, 2, 5
    X, y, gp, gpo = rp._problem(D, 90, "se", seed)
    p0, b = rp._start(L * 2, W, D, seed).reshape(L, 2, W, D), rp._bounds(D)
    dev = gp.sample_tempered(y, p0, N, b, [1.0, 1.0], swapEvery=1, seed=seed, ladders=L, storeRungs=2, swapLog=True)
    log, mu = dev["swap_log"], dev["rung_log_prob"]
    assert log.shape == (N - 1, L, 1, W)
    finite = np.isfinite(mu[:-1, :, 0]) & np.isfinite(mu[:-1, :, 1])            # round r follows iteration r
    print("exchanges not proposed for a mu that is not finite:", int((~finite[::2]).sum()))
    for r in range(N - 1):
        want = np.where(finite[r], 2, 0) if r % 2 == 0 else np.zeros((L, W), dtype=int)
        assert np.array_equal(log[r, :, 0], want), "round %d" % r
    assert np.array_equal(dev["swap_accepted"], dev["swap_proposed"]) and np.all(dev["swap_proposed"] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. stationarity and evidence on a two-well surrogate
# ---------------------------------------------------------------------------------------------------------------------
_WELLS = {}


def _two_wells():
    """A GP fitted to an 8 x 8 grid of log(exp(-|x - a|^2 / 2 s^2) + 0.5 exp(-|x - c|^2 / 2 s^2)), a = (-1.25, -0.25), c = (1.25,
    0.25), s = 0.15, on [-2, 2]^2: two wells of the GP mean with a saddle some 27 nats below them and a third of the mass in
    the second; and the truth by quadrature of GP.predict on a midpoint grid of
    spacing h = 1 / 128 and of h / 2: per beta, E_beta[mu] and log int exp(beta mu); at beta = 1 the mass in x_0 > 0.  The
    difference between the two grids bounds the quadrature error of each."""
    if _WELLS:
        return _WELLS
    from approxposterior_amd import gp as agp
    g = np.linspace(-1.75, 1.75, 8)
    X = np.array([(u, v) for u in g for v in g])
    a, c, s = np.array([-1.25, -0.25]), np.array([1.25, 0.25]), 0.15
    y = np.logaddexp(-0.5 * np.sum((X - a) ** 2, axis=1) / s ** 2, np.log(0.5) - 0.5 * np.sum((X - c) ** 2, axis=1) / s ** 2)
    gp = agp.GP(kernel=np.var(y) * agp.ExpSquaredKernel([0.5, 0.5], ndim=2), fit_mean=True, mean=float(np.mean(y)),
                white_noise=-8.0, fit_white_noise=False)
    gp.compute(X)
    betas = _mcmc().tempering_ladder(6, 0.005)

    def grid(m):
        e = -2.0 + (np.arange(m) + 0.5) * (4.0 / m)
        pts = np.array(np.meshgrid(e, e, indexing="ij")).reshape(2, -1).T
        mu = np.asarray(gp.predict(y, pts, return_cov=False), dtype=np.float64).ravel()
        out = {"mean": [], "logint": []}
        for beta in betas:
            wgt = np.exp(beta * (mu - mu.max()))
            out["mean"].append(np.sum(wgt * mu) / np.sum(wgt))
            out["logint"].append(np.log(np.sum(wgt) * (4.0 / m) ** 2) + beta * mu.max())
        wgt = np.exp(mu - mu.max())
        out["mass"] = np.sum(wgt[pts[:, 0] > 0.0]) / np.sum(wgt)
        return {k: np.asarray(v) for k, v in out.items()}
    coarse, fine = grid(512), grid(1024)
    _WELLS.update(gp=gp, X=X, y=y, betas=betas, truth=fine,
                  qerr={k: np.abs(fine[k] - coarse[k]) for k in fine}, bounds=[(-2.0, 2.0), (-2.0, 2.0)])
    return _WELLS


def test_two_wells_rung_means_cold_mass_and_evidence():
    """8 ladders of 6 rungs ending at beta = 0, 8 walkers, 4000 iterations (the first 1000 discarded), every walker started
    in the first well.  Each rung's mean of mu, the cold chain's mass in the second well and log_evidence lie within 5
    standard errors (between ladders) plus the quadrature bound of the grid's values; log_evidence is compared with the
    SAME ladder's trapezoid of the true rung means, which takes the discretisation out.  The single-temperature ensemble
    from the same start is run for comparison and not asserted on."""
    from approxposterior_amd import approx
    z = _two_wells()
    gp, y, betas, truth, qerr, b = z["gp"], z["y"], z["betas"], z["truth"], z["qerr"], z["bounds"]
    L, T, W, N, discard = 8, len(betas), 8, 4000, 1000
    rs = np.random.RandomState(3)
    p0 = np.array([-1.25, -0.25]) + 0.05 * rs.standard_normal((W, 2))
    res = gp.sample_tempered(y, p0, N, b, betas, seed=77, ladders=L)
    chain = _mcmc().TemperedChain(res)
    per = chain.rung_means(discard)                                            # (L, T)
    mean, se = per.mean(axis=0), per.std(axis=0, ddof=1) / np.sqrt(L)
    print("betas", betas)
    print("rung means of mu", mean, "truth", truth["mean"], "se", se, "quadrature", qerr["mean"])
    print("exchange acceptance", chain.swap_acceptance_fraction, "move acceptance", chain.rung_acceptance_fraction)
    assert np.all(np.abs(mean - truth["mean"]) <= 5.0 * se + qerr["mean"])
    right = (chain.get_chain(discard=discard)[:, :, 0] > 0.0).reshape(N - discard, L, W).mean(axis=(0, 2))
    mse = right.std(ddof=1) / np.sqrt(L)
    plain = gp.sample_ensemble(y, p0, N, b, seed=77)
    print("mass in the second well: tempered %.4f +- %.4f, truth %.4f, single-temperature ensemble %.4f" % (
        right.mean(), mse, truth["mass"], (plain["chain"][discard:, :, 0] > 0.0).mean()))
    assert 0.05 < truth["mass"] < 0.95
    assert abs(right.mean() - truth["mass"]) <= 5.0 * mse + qerr["mass"]
    logz, disc, mc = chain.log_evidence(discard=discard)
    w = _mcmc()._trapezoid_weights(betas)
    same = np.log(16.0) + float(np.dot(w, truth["mean"]))
    grid_logz = float(truth["logint"][0])
    ap = approx.ApproxPosterior(theta=z["X"], y=y, gp=gp, lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                                priorSample=lambda m: np.random.uniform(-2, 2, size=(m, 2)), bounds=b, algorithm="agp",
                                distributed=False)
    imp = ap.evidence(nSamples=2 ** 18, proposal="box", seed=1)
    print("logZ: tempering %.4f (discErr %.3f, mcErr %.4f), trapezoid of the true rung means %.4f, grid %.4f (gap %.3f), "
          "evidence(box) %.4f +- %.4f" % (logz, disc, mc, same, grid_logz, same - grid_logz, imp["logZ"], imp["logZErr"]))
    assert abs(logz - same) <= 5.0 * mc + float(np.dot(w, qerr["mean"]))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_the_device():
    from approxposterior_amd import _lib, gp as agp
    lib = _lib.load()
    D = 2
    X, y, gp, gpo = rp._problem(D, 40, "se", 1)
    ks = gp._kernel_struct()
    one = ctypes.c_void_p(8)                      # never dereferenced: the checks come before any HIP call
    lo, hi = agp._box(rp._bounds(D), D, optional=False)
    inf_hi = (ctypes.c_double * _lib.MAX_DIM)(*([2.0, np.inf] + [0.0] * (_lib.MAX_DIM - 2)))
    ok = dict(n=40, lo=lo, hi=hi, W=8, T=3, L=2, betas=[1.0, 0.5, 0.0], iters=10, se=2, nstore=1, moves=None, nmoves=0,
              xs=one, work=one, sprop=one)

    def call(**kw):
        a = dict(ok, **kw)
        bb = (ctypes.c_double * max(len(a["betas"]), 1))(*a["betas"])
        return lib.apgp_tempered_sample(a["xs"], a["n"], ctypes.byref(ks), 0.0, a["lo"], a["hi"], a["W"], a["T"], a["L"], bb,
                                        a["iters"], a["se"], 1, one, one, one, a["nstore"], one, one, a["sprop"], one, None,
                                        a["moves"], a["nmoves"], a["work"], None)
    bad_move = (_lib.EnsMove * 1)()
    bad_move[0].kind, bad_move[0].weight, bad_move[0].p0 = _lib.ENS_MOVE_STRETCH, 1.0, 0.5
    rows = [(dict(T=0, betas=[]), b"ntemps"), (dict(T=65, betas=[1.0] * 65), b"ntemps"),
            (dict(betas=[1.0, np.nan, 0.0]), b"betas"), (dict(betas=[1.0, np.inf, 0.0]), b"betas"),
            (dict(betas=[1.5, 0.5, 0.0]), b"betas"), (dict(betas=[1.0, 0.5, -0.1]), b"betas"),
            (dict(betas=[1.0, 0.2, 0.5]), b"betas must not increase"),
            (dict(hi=inf_hi), b"beta = 0"), (dict(se=0), b"swap_every"), (dict(nstore=-1), b"nstore"),
            (dict(nstore=4), b"nstore"), (dict(L=1 << 30), b"grid limit"), (dict(L=0), b"nladders"),
            # ... and what apgp_ensemble_sample_moves refuses
            (dict(xs=None), b"null pointer"), (dict(work=None), b"null pointer"), (dict(sprop=None), b"swap_prop"),
            (dict(n=0), b"n, iterations"), (dict(iters=-1), b"n, iterations"), (dict(W=7), b"nwalkers"),
            (dict(W=2), b"nwalkers"), (dict(W=258), b"nwalkers"), (dict(nmoves=1), b"moves is NULL"),
            (dict(moves=bad_move, nmoves=1), b"stretch scale")]
    for bad, text in rows:
        assert call(**bad) == -1, bad
        msg = lib.apgp_last_error()
        assert b"apgp_tempered_sample" in msg and b"bad argument" in msg and text in msg, (bad, msg)
    assert lib.apgp_tempered_work_len(8, 3, 2, 2) == 2 * 2 * 3 * 8 * 3
    assert lib.apgp_tempered_work_len(64, 8, 1, 8) == 2 * 8 * 64 * 9
    for bad in ((1, 3, 2, 2), (258, 3, 2, 2), (8, 0, 2, 2), (8, 65, 2, 2), (8, 3, 0, 2), (8, 3, 2, 33), (8, 64, 1 << 26, 2)):
        assert lib.apgp_tempered_work_len(*bad) == -1, bad
    with pytest.raises(ValueError, match="start at 1"):
        gp.sample_tempered(y, rp._start(1, 8, D, 1)[0], 5, rp._bounds(D), [0.9, 0.5])
    with pytest.raises(ValueError, match="initial_state"):
        gp.sample_tempered(y, rp._start(2, 8, D, 1), 5, rp._bounds(D), [1.0, 0.5, 0.1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the product API
# ---------------------------------------------------------------------------------------------------------------------
def _box_ap(joint):
    from approxposterior_amd import approx, gp as agp, priors as P
    z = _two_wells()
    b = z["bounds"]
    gp = agp.GP(kernel=np.var(z["y"]) * agp.ExpSquaredKernel([0.5, 0.5], ndim=2), fit_mean=True, mean=float(np.mean(z["y"])),
                white_noise=-8.0, fit_white_noise=False)
    gp.compute(z["X"])
    lo, hi = np.array(b)[:, 0], np.array(b)[:, 1]
    if joint:
        J = P.JointPrior([P.UniformPrior(*r) for r in b])
        lnprior, sample = J, J.sample
    else:
        lnprior = lambda t: 0.0 if np.all((np.asarray(t) >= lo) & (np.asarray(t) <= hi)) else -np.inf      # noqa: E731
        sample = lambda m: np.random.uniform(lo, hi, size=(int(m), 2))                                     # noqa: E731
    lnlike = lambda t, *a, **k: float(np.logaddexp(-np.sum((np.asarray(t) - [-1.25, -0.25]) ** 2) / 0.045,     # noqa: E731
                                                   np.log(0.5) - np.sum((np.asarray(t) - [1.25, 0.25]) ** 2) / 0.045))
    return approx.ApproxPosterior(theta=z["X"].copy(), y=z["y"].copy(), gp=gp, lnprior=lnprior, lnlike=lnlike,
                                  priorSample=sample, bounds=b, algorithm="agp", distributed=False)


@pytest.mark.parametrize("joint,device_tau", [(False, False), (True, False), (False, True)],
                         ids=["box", "joint-prior", "device-autocorr"])
def test_run_mcmc_with_tempering(joint, device_tau):
    mcmc = _mcmc()
    ap = _box_ap(joint)
    W, N = 8, 600
    rs = np.random.RandomState(2)
    p0 = np.array([-1.25, -0.25]) + 0.05 * rs.standard_normal((W, 2))
    np.random.seed(4)
    sampler, iburn, ithin = ap.runMCMC(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": N, "initial_state": p0},
                                       cache=False, estBurnin=True, thinChains=True, onDevice=True, tempering=4,
                                       deviceAutocorr=device_tau)
    assert isinstance(sampler, mcmc.TemperedChain) and sampler is ap.sampler
    assert sampler.get_chain().shape == (N, W, 2) and sampler.get_log_prob().shape == (N, W)
    assert np.array_equal(sampler.betas, mcmc.tempering_ladder(4)) and sampler.betas[-1] == 0.0
    assert sampler.swap_acceptance_fraction.shape == (3,) and sampler.rung_acceptance_fraction.shape == (4,)
    assert np.all(sampler.rung_acceptance_fraction > 0)
    assert 0 <= iburn < N and ithin >= 1 and ap._chainCut == (iburn, ithin)
    assert (sampler._chain_device is not None) == device_tau
    blobs = sampler.get_blobs()
    if joint:
        assert blobs.shape == (N, W) and np.allclose(blobs, -np.log(16.0))
    else:
        assert blobs is None
    logz, disc, mc = sampler.log_evidence(discard=iburn)
    assert np.isfinite(logz) and disc >= 0 and mc > 0
    # a dict: the ladder itself, several ladders, the exchange interval
    np.random.seed(4)
    sampler, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": 50, "initial_state": p0},
                               cache=False, estBurnin=False, thinChains=False, onDevice=True,
                               tempering={"betas": [1.0, 0.3, 0.0], "ladders": 3, "swapEvery": 4})
    assert sampler.get_chain().shape == (50, 3 * W, 2) and sampler.nladders == 3 and sampler.swap_every == 4
    assert sampler._swap_proposed.shape == (3, 2)
    with pytest.raises(ValueError):
        ap.runMCMC(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": 5, "initial_state": p0}, cache=False,
                   onDevice=True, tempering={"rungs": 3})


def test_run_with_tempering_completes():
    ap = _box_ap(False)
    n0 = len(ap.y)
    np.random.seed(6)
    with np.errstate(all="ignore"):
        ap.run(m=2, nmax=1, nGPRestarts=1, cache=False, verbose=False, onDevice=True, estBurnin=True, thinChains=False,
               gpOptions={"maxiter": 3, "xtol": 1e-2, "ftol": 1e-2}, nMinObjRestarts=2, minObjOptions={"maxiter": 20},
               samplerKwargs={"nwalkers": 8}, mcmcKwargs={"iterations": 200}, tempering={"ntemps": 3, "swapEvery": 5})
    assert len(ap.y) == n0 + 2 and isinstance(ap.sampler, _mcmc().TemperedChain)
    assert ap.sampler.get_chain().shape == (200, 8, 2) and len(ap.iburns) == 1
