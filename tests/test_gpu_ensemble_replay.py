"""MI355X: the on-device ensemble sampler (csrc/ensemble.hip, ensemble_kernel and ensemble_mw_kernel) replayed move by move
against the NumPy restatement of its stretch move (tests/ensemble_ref.py) with the oracle's GP mean in float64.

The move is a deterministic function of (seed, ensemble, iteration, half-step, slot) and the state, so the check is exact
rather than statistical: every half-step is replayed from the state the device's own chain records (teacher forcing), and
each decision, each accepted position and each log-probability is compared.  The only latitude is a near-tie -- a
proposal whose acceptance hinges on the last bits of the GP mean or of the position (|log u - diff| within
1e-8 max(1, S) or the proposal within 1e-12 of a face, in units of the span), where S = sum|alpha| max|k| is the size of the
GP mean's terms; near-ties are counted and printed, and more than one per 1e4 proposals fails the case.

Position bound of an accepted move: the kernel holds x * sc (sc = sqrt(inv_metric / 2)), forms
q = x_j - (x_j - x_s) zz there with one fused multiply-add, and stores q / sc; the forced replay starts from the stored
(rounded) state.  Each step adds at most a few ulps of max(|x_j|, |x_s|) times (1 + a): 16 (1 + a) eps max(|x_j|, |x_s|)
covers them with room.  A free-running replay does not stay that close over hundreds of iterations -- the ensemble's
affine moves amplify one-ulp differences, by 1e7 over 300 iterations at W = 8 in a NumPy experiment -- so the whole
chain is compared to 1e-6 of the span there, with every accept / reject decision equal."""
import numpy as np
import pytest

import ensemble_ref as er

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _mods():
    import george_oracle as go
    from approxposterior_amd import gp as agp
    return go, agp


def _bounds(D):
    return np.array([(-2.0 - 0.1 * d, 2.0 + 0.05 * d) for d in range(D)])


def _problem(D, n, kern, seed):
    """Training set in the box, y a tilted quadratic with a ripple (the posterior sits inside the box, not on a face)."""
    rs = np.random.RandomState(1000 + 37 * D + n)
    b = _bounds(D)
    X = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(size=(n, D))
    c = rs.uniform(-0.5, 0.5, D)
    y = -0.5 * np.sum((X - c) ** 2 / (0.3 + 0.1 * np.arange(D)), axis=1) + 0.2 * np.sin(2.0 * X[:, 0])
    metric = np.linspace(0.6, 1.6, D) * max(1.0, D / 2.0)

    def make(mod):
        k = mod.ExpSquaredKernel(metric, ndim=D)
        if kern.startswith("amp"):
            k = 2.5 * k
        if "lin" in kern:
            k = k + 0.3 * mod.kernels.LinearKernel(log_gamma2=0.4, order=int(kern[-1]), bounds=None, ndim=D)
        return mod.GP(kernel=k, fit_mean=True, mean=float(np.median(y)), white_noise=-4.0,
                      fit_white_noise=False)
    go, agp = _mods()
    gp, gpo = make(agp), make(go)
    gp.compute(X)
    gpo.compute(X)
    return X, y, gp, gpo


def _start(E, W, D, seed):
    """Walkers inside the box, one outside it, one on a lower and one on an upper face."""
    rs = np.random.RandomState(seed % 1000 + W)
    b = _bounds(D)
    mid, half = 0.5 * (b[:, 0] + b[:, 1]), 0.5 * (b[:, 1] - b[:, 0])
    p0 = mid + 0.8 * half * rs.uniform(-1, 1, size=(E, W, D))
    p0[0, 0, 0] = b[0, 1] + 0.5                   # outside: -inf until it takes a proposal
    if W > 1:
        p0[0, 1, 0] = b[0, 0]                     # exactly on the lower face of dimension 0
    if W > 2:
        p0[-1, 2, D - 1] = b[D - 1, 1]            # exactly on the upper face of the last dimension
    return p0


def _oracle(gpo, y, D):
    chunk = max(64, int(4e6 // len(gpo._x)))

    def lp(pts):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, D)
        return np.concatenate([np.atleast_1d(gpo.predict(y, pts[i:i + chunk], return_cov=False))
                               for i in range(0, len(pts), chunk)]) if len(pts) else np.empty(0)
    return lp


def _size(gpo, y, X):
    """S = sum|alpha| max|k(x, x')|: the size of the GP mean's terms (sum|alpha| for a unit ExpSquared kernel)."""
    return np.abs(gpo._compute_alpha(y, False)).sum() * max(1.0, np.abs(gpo.kernel.get_value(X)).max())


def _scales(gp, D):
    ks = gp._kernel_struct()
    return np.sqrt(0.5 * np.array(ks.inv_metric[:D]))


def _expected_groups(E, W, iters, mode):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = W // 2
    if G * E > cus:
        G = cus // E
    return (G if mode == 0 and G >= 2 and iters > 0 else 1), cus


def _check_chain(dev, p0, bounds, a, seed, sc, lp, S, label, free=None):
    """Every half-step of the device's chain against the forced replay; returns the number of near-ties."""
    E, W, D = p0.shape
    EW, H = E * W, W // 2
    ch, lpc = dev["chain"], dev["log_prob"]
    T = ch.shape[0]
    f = er.forced(lp, p0, ch, bounds, a=a, seed=seed, sc=sc)
    t = np.arange(T)[None, :, None, None]
    w = f["walker"]
    prev = np.concatenate([p0.reshape(1, EW, D), ch[:-1]], axis=0)
    prev_lp = np.concatenate([np.full((1, EW), np.nan), lpc[:-1]], axis=0)
    before, after = prev[t, w], ch[t, w]                                 # (E, T, 2, H, D)
    moved = np.any(after != before, axis=-1)
    moved[:, 0] = np.any(np.abs(after[:, 0] - before[:, 0]) > np.spacing(np.abs(before[:, 0])), axis=-1)  # (x sc) / sc
    tie = (f["margin"] <= 1e-8 * max(1.0, S)) | (f["face"] <= 1e-12)
    nprop = moved.size
    ntie = int(tie.sum())
    bad = (moved != f["accept"]) & ~tie
    assert not bad.any(), "%s: %d decisions differ from the replay (first at %s: device %s, replay %s, margin %.3e)" % (
        label, bad.sum(), np.argwhere(bad)[0], moved[bad][0], f["accept"][bad][0], f["margin"][bad][0])
    assert ntie * 10 ** 4 <= nprop, "%s: %d near-ties in %d proposals" % (label, ntie, nprop)
    both = moved & f["accept"]
    tol = 16.0 * (1.0 + a) * EPS * np.maximum(f["scale"], np.finfo(np.float64).tiny)
    dq = np.abs(after - f["q"])
    assert np.all(dq[both] <= tol[both]), "%s: accepted position off by %.3g ulps of (1 + a) max|x|" % (
        label, (dq[both] / ((1 + a) * EPS * np.maximum(f["scale"][both], 1e-300))).max())
    lp_after = lpc[t, w]
    assert np.all(np.abs(lp_after[both] - f["lpq"][both]) <= 1e-9 * S), "%s: stored log-probability of an accepted move" % label
    rej = ~moved & ~f["accept"]
    rej1 = rej.copy()
    rej1[:, 0] = False
    assert np.array_equal(after[rej1], before[rej1]), "%s: a rejected walker moved" % label
    pl = prev_lp[t, w]
    assert np.array_equal(lp_after[rej1], pl[rej1]), "%s: a rejected walker's log-probability changed" % label
    r0 = rej[:, 0]
    l0, o0 = lp_after[:, 0][r0], f["lps"][:, 0][r0]
    assert np.array_equal(np.isneginf(l0), np.isneginf(o0))
    assert np.all(np.abs(l0[np.isfinite(o0)] - o0[np.isfinite(o0)]) <= 1e-9 * S), "%s: initial log-probability" % label
    # totals
    dev_count = np.bincount(w[moved], minlength=EW)
    assert np.array_equal(dev["naccept"], dev_count), "%s: naccept is not the number of moves in the chain" % label
    if not (moved != f["accept"]).any():
        assert np.array_equal(dev["naccept"], np.bincount(w[f["accept"]], minlength=EW))
    if T:
        assert np.array_equal(dev["coords"], ch[-1]) and np.array_equal(dev["final_log_prob"], lpc[-1])
    # the free-running replay reproduces the whole chain when neither run meets a near-tie
    if free is not None and ntie == 0:
        ftie = int(((free["decisions"]["margin"] <= 1e-8 * max(1.0, S)) | (free["decisions"]["face"] <= 1e-12)).sum())
        if ftie == 0:
            span = np.ptp(bounds, axis=1)
            assert np.all(np.abs(free["chain"] - ch) <= 1e-6 * span), "%s: free-running replay diverged" % label
            assert np.array_equal(free["naccept"], dev["naccept"])
            fin = np.isfinite(free["log_prob"])
            assert np.array_equal(fin, np.isfinite(lpc)) and np.all(np.abs(free["log_prob"][fin] - lpc[fin]) <= 1e-9 * S)
        else:
            print("%s: free-running replay met %d near-ties of its own; whole-chain comparison not applicable" % (label, ftie))
    return ntie, nprop


# D, W, n, E, kernel, seed, a, iterations, kernels to run (0: several workgroups where possible, 1: one)
CASES = [
    (1, 2, 200, 1, "se", 5, 2.0, 300, (0, 1)),                        # W = 2D = 2
    (2, 6, 300, 3, "amp", 2 ** 32 + 17, 1.5, 200, (0, 1)),            # odd half, k1 != 0
    (3, 34, 400, 1, "se+lin1", -7, 3.0, 120, (0, 1)),                 # odd half, negative seed
    (5, 70, 700, 3, "amp+lin2", 123, 2.0, 60, (0, 1)),                # odd half, DPAD 8
    (8, 64, 300, 1, "se", -(2 ** 40) - 3, 1.5, 100, (0, 1)),          # DPAD 8, training stream in LDS
    (8, 256, 2500, 3, "amp+lin1", 2 ** 33 + 1, 3.0, 24, (0,)),        # W max, stream in L2, G clipped by the CUs
    (9, 18, 300, 1, "amp", 77, 2.0, 100, (0, 1)),                     # DPAD 16 (one proposal per pass), LDS
    (9, 18, 700, 1, "se+lin2", -99, 1.5, 80, (0, 1)),                 # DPAD 16, stream in L2
    (17, 34, 300, 1, "se", 2 ** 35, 3.0, 60, (0, 1)),                 # DPAD 32
    (32, 64, 200, 1, "amp", 31, 2.0, 60, (0, 1)),                     # DPAD 32, W = 2D
    (2, 4, 100, 1, "amp+lin1", -1, 3.0, 1, (0, 1)),                   # one iteration
]


@pytest.mark.parametrize("D,W,n,E,kern,seed,a,iters,modes", CASES,
                         ids=["D%d-W%d-n%d-E%d-%s-it%d" % (c[0], c[1], c[2], c[3], c[4], c[7]) for c in CASES])
def test_device_sampler_replays_move_by_move(D, W, n, E, kern, seed, a, iters, modes):
    from approxposterior_amd import _lib
    lib = _lib.load()
    X, y, gp, gpo = _problem(D, n, kern, seed)
    p0 = _start(E, W, D, seed)
    b = _bounds(D)
    sc = _scales(gp, D)
    lp = _oracle(gpo, y, D)
    S = _size(gpo, y, X)
    free = er.run(lp, p0, iters, b, a=a, seed=seed, sc=sc)
    for mode in modes:
        G, cus = _expected_groups(E, W, iters, mode)
        fb0 = getattr(gp, "ensemble_fallbacks", 0)
        prev = lib.apgp_ensemble_mode(mode)
        try:
            dev = gp.sample_ensemble(y, p0, iters, b, a=a, seed=seed)
        finally:
            lib.apgp_ensemble_mode(prev)
        fb = getattr(gp, "ensemble_fallbacks", 0) - fb0
        label = "D=%d W=%d n=%d E=%d %s seed=%d a=%g T=%d mode %d" % (D, W, n, E, kern, seed, a, iters, mode)
        ntie, nprop = _check_chain(dev, p0, b, a, seed, sc, lp, S, label, free)
        print("%s: G = %d workgroups per ensemble (%d CUs), %d fallbacks, %d near-ties in %d proposals, acceptance %.3f"
              % (label, G, cus, fb, ntie, nprop, dev["naccept"].sum() / max(1, nprop)))


def test_zero_iterations_leaves_the_start():
    """iterations = 0: coordinates as given (to the 1 ulp of the x sc / sc round trip), log-probability the oracle's mean
    or -inf outside the box (the start on a face is inside), no move counted -- on both kernel choices."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    D, W, E = 3, 6, 3
    X, y, gp, gpo = _problem(D, 100, "se", 4)
    p0 = _start(E, W, D, 4)
    b = _bounds(D)
    S = _size(gpo, y, X)
    want = gpo.predict(y, p0.reshape(-1, D), return_cov=False)
    inside = np.all((p0.reshape(-1, D) >= b[:, 0]) & (p0.reshape(-1, D) <= b[:, 1]), axis=1)
    assert not inside.all() and inside.sum() == E * W - 1
    for mode in (0, 1):
        prev = lib.apgp_ensemble_mode(mode)
        try:
            dev = gp.sample_ensemble(y, p0, 0, b, seed=4)
        finally:
            lib.apgp_ensemble_mode(prev)
        assert dev["chain"].shape == (0, E * W, D) and np.all(dev["naccept"] == 0)
        assert np.all(np.abs(dev["coords"] - p0.reshape(-1, D)) <= np.spacing(np.abs(p0.reshape(-1, D))))
        lpd = dev["final_log_prob"]
        assert np.all(np.isneginf(lpd[~inside])) and np.all(np.abs(lpd[inside] - want[inside]) <= 1e-9 * S)


def test_run_mcmc_on_device_honours_the_stretch_scale():
    """runMCMC(onDevice=True, samplerKwargs={"a": 3.0}) runs the sampler at a = 3 with the seed runMCMC draws from NumPy's
    stream: the chain is the replay's at a = 3.0 and not the replay's at the default a = 2.0; the chain records its a."""
    from approxposterior_amd import approx
    D, W, T = 2, 10, 80
    X, y, gp, gpo = _problem(D, 150, "se", 8)
    b = _bounds(D)
    lnprior = lambda t: 0.0 if np.all((np.asarray(t) >= b[:, 0]) & (np.asarray(t) <= b[:, 1])) else -np.inf
    ap = approx.ApproxPosterior(theta=X, y=y, gp=gp, lnprior=lnprior, lnlike=lambda t: 0.0,
                                priorSample=lambda m: np.random.uniform(b[:, 0], b[:, 1], size=(m, D)),
                                bounds=[tuple(r) for r in b], algorithm="agp", distributed=False)
    p0 = _start(1, W, D, 8)[0]
    np.random.seed(2024)
    seed = np.random.randint(0, 2 ** 31 - 1)                  # what runMCMC draws for its one ensemble
    np.random.seed(2024)
    with np.errstate(all="ignore"):
        sampler, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": W, "a": 3.0}, mcmcKwargs={"iterations": T, "initial_state": p0},
                                   cache=False, estBurnin=False, thinChains=False, onDevice=True)
    assert sampler.a == 3.0
    dev = {"chain": sampler.get_chain(), "log_prob": sampler.get_log_prob(), "naccept": sampler._naccepted.astype(np.int64),
           "coords": sampler._coords, "final_log_prob": sampler._lp}
    lp, S, sc = _oracle(gpo, y, D), _size(gpo, y, X), _scales(gp, D)
    free = er.run(lp, p0, T, b, a=3.0, seed=seed, sc=sc)
    ntie, nprop = _check_chain(dev, p0[None], b, 3.0, seed, sc, lp, S, "runMCMC a=3.0", free)
    print("runMCMC(onDevice=True, a=3.0): seed %d, %d near-ties in %d proposals" % (seed, ntie, nprop))
    with pytest.raises(AssertionError):
        _check_chain(dev, p0[None], b, 2.0, seed, sc, lp, S, "runMCMC replayed at a=2.0")
