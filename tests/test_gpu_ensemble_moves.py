"""MI355X: the ensemble moves of the on-device sampler (csrc/ens_moves.h, called by ensemble_kernel and ensemble_mw_kernel)
-- differential evolution, the snooker update and weighted mixtures -- replayed move by move against their NumPy
restatement (tests/ensemble_moves_ref.py) with the oracle's GP mean, as test_gpu_ensemble_replay.py does for the stretch
move and with its problems, starts, bounds and near-tie rule: a proposal is a near-tie when |log u - diff| <=
1e-8 max(1, S) or it lies within 1e-12 (of the span) of a face; near-ties are counted and printed, more than one per 1e4
proposals fails the case.

Position bound of an accepted move.  The kernel holds the scaled state x sc, forms the proposal there and stores q / sc;
the forced replay restarts every half-step from the stored state, so each of its inputs x sc differs from the kernel's by
the two roundings of (x sc) / sc and x sc: 2 eps relative.  eps = 2^-52; the constant 16 is the stretch test's.
* stretch (a mixture's stretch iterations): the stretch test's bound, 16 (1 + a) eps max(|x_j|, |x_s|).
* DE, q = s + gamma (c_j - c_k), per coordinate: the inputs carry 2 eps (|s| + |gamma| (|c_j| + |c_k|)), the difference
  rounds once (eps |gamma| |c_j - c_k|), the device's fused multiply-add once and the replay's multiply and add twice
  (eps (|s| + |gamma| |c_j - c_k|) each), the division by sc once more: under 8 eps (|s| + |gamma| (|c_j| + |c_k|)), bounded
  by 16 eps (|s| + (1 + |gamma|) (|c_j| + |c_k|)).  gamma = g0 (1 + sigma n) itself: its two roundings are inside that room;
  the normal n = sqrt(-2 log u1) cospi(2 u2) differs between the device's log / cospi and NumPy's by a few ulps OF n (the
  cosine's argument is reduced exactly on both sides; |n| <= 8.7 for 53-bit uniforms), which moves q by at most
  |c_j - c_k| g0 sigma |n| 16 eps.
* snooker, q = s + c v, v = s - z, c = gammas (v . w) / (v . v), w = z1 - z2, norms and dot products over the scaled
  coordinates (|.| below is the Euclidean norm there; D is the dimension).  With c given, the DE argument with
  (gamma, c_j, c_k) -> (c, s, z) gives 16 eps (|s_d| + (1 + |c|) (|s_d| + |z_d|)).  The error of c, times |v_d| <= |v|: the two
  D-term sums round D times each and the product and quotient twice more -- the (D + 16) eps gammas |w| that the issue
  gives for this move.  THIS BOUND DEPARTS FROM THAT FORM, by two rounding steps it leaves out.  The first is the
  cancellation in v = s - z: its inputs' 2 eps (|s| + |z|) plus its own rounding is an error of up to 3 eps (|s| + |z|) in
  |v|, i.e. 3 eps kappa relative with kappa = (|s| + |z|) / |v| >= 1, and it enters c three times (once through the dot
  product, twice through |v|^2): 9 eps kappa gammas |w|.  The direction (s - z) / |s - z| is ill-conditioned in exactly
  this way when s is close to z, so no bound without kappa can hold for every pair, and the bound grows without limit
  as s approaches z.  The second is w's own inputs: 3 eps gammas (|z1| + |z2|).
  Together eps gammas ((D + 16) (1 + kappa) |w| + 3 (|z1| + |z2|)), which dominates (2 D + 2 + 9 kappa) |w| + 3 (...) and
  is at least twice the issue's term.  In plain coordinates every term is divided by sc_d.  Every case prints the
  largest fraction of its bound that an accepted position used.
None of the constants is fitted to what the device gives."""
import ctypes

import numpy as np
import pytest

import ensemble_moves_ref as emr
import test_gpu_ensemble_replay as rp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny


def _mcmc():
    from approxposterior_amd import mcmc
    return mcmc


def _objects(spec):
    """mcmc move objects (what the product API takes) for a reference spec (what emr.table takes)."""
    mcmc = _mcmc()
    make = {"stretch": lambda m: mcmc.StretchMove(m[1]), "de": lambda m: mcmc.DEMove(m[1], m[2] if len(m) > 2 else None),
            "snooker": lambda m: mcmc.DESnookerMove(m[1])}
    if isinstance(spec[0], str):
        return make[spec[0]](spec)
    return [(make[m[0][0]](m[0]), m[1]) if not isinstance(m[0], str) else make[m[0]](m) for m in spec]


def _ties(margin, face, S):
    return (margin <= 1e-8 * max(1.0, S)) | (face <= 1e-12)


def _position_tolerance(f, tab, sc, D):
    """The module docstring's bound per accepted coordinate, (E, T, 2, H, D), in plain coordinates."""
    kind, c = f["kind"], np.abs(f["mult"])[..., None]
    xs, xj, xk, xl = (np.abs(f[k]) for k in ("xs", "xj", "xk", "xl"))
    a = f["par"][..., 0][..., None]
    stretch = 16.0 * (1.0 + a) * EPS * np.maximum(np.maximum(xj, xs), TINY)
    sigma, g0 = f["par"][..., 0][..., None], f["par"][..., 1][..., None]
    de = 16.0 * EPS * (xs + (1.0 + c) * (xj + xk)) + np.abs(f["xj"] - f["xk"]) * g0 * sigma * np.abs(f["normal"])[..., None] * 16.0 * EPS
    norm = lambda v: np.sqrt(np.sum((v * sc) ** 2, axis=-1))[..., None]
    with np.errstate(all="ignore"):
        kappa = (norm(f["xs"]) + norm(f["xj"])) / norm(f["xs"] - f["xj"])
        gammas = f["par"][..., 0][..., None]
        sn = 16.0 * EPS * (xs + (1.0 + c) * (xs + xj)) + EPS * gammas * (
            (D + 16.0) * (1.0 + kappa) * norm(f["xk"] - f["xl"]) + 3.0 * (norm(f["xk"]) + norm(f["xl"]))) / sc
    k3 = kind[..., None]
    return np.where(k3 == emr.STRETCH, stretch, np.where(k3 == emr.DE, de, sn))


def _check(dev, p0, bounds, tab, seed, sc, lp, S, label, free=None):
    """Every half-step of the device's chain against the forced replay under the move table; returns the near-ties."""
    E, W, D = p0.shape
    EW = E * W
    ch, lpc = dev["chain"], dev["log_prob"]
    T = ch.shape[0]
    f = emr.forced(lp, p0, ch, bounds, tab, seed=seed, sc=sc)
    t = np.arange(T)[None, :, None, None]
    w = f["walker"]
    prev = np.concatenate([p0.reshape(1, EW, D), ch[:-1]], axis=0)
    prev_lp = np.concatenate([np.full((1, EW), np.nan), lpc[:-1]], axis=0)
    before, after = prev[t, w], ch[t, w]
    moved = np.any(after != before, axis=-1)
    moved[:, 0] = np.any(np.abs(after[:, 0] - before[:, 0]) > np.spacing(np.abs(before[:, 0])), axis=-1)      # (x sc) / sc
    tie = _ties(f["margin"], f["face"], S)
    nprop, ntie = moved.size, int(tie.sum())
    bad = (moved != f["accept"]) & ~tie
    assert not bad.any(), "%s: %d decisions differ from the replay (first at %s: device %s, replay %s, margin %.3e, kind %d)" % (
        label, bad.sum(), np.argwhere(bad)[0], moved[bad][0], f["accept"][bad][0], f["margin"][bad][0], f["kind"][bad][0])
    assert ntie * 10 ** 4 <= nprop, "%s: %d near-ties in %d proposals" % (label, ntie, nprop)
    both = moved & f["accept"]
    tol = _position_tolerance(f, tab, sc, D)
    dq = np.abs(after - f["q"])
    for kind, name in ((emr.STRETCH, "stretch"), (emr.DE, "DE"), (emr.SNOOKER, "snooker")):
        sel = both & (f["kind"] == kind)
        if sel.any():
            worst = (dq[sel] / tol[sel]).max()
            print("%s: %s positions use %.3f of their bound over %d accepted moves" % (label, name, worst, sel.sum()))
            assert np.all(dq[sel] <= tol[sel]), "%s: accepted %s position off by %.3g of its bound" % (label, name, worst)
    lp_after = lpc[t, w]
    assert np.all(np.abs(lp_after[both] - f["lpq"][both]) <= 1e-9 * S), "%s: stored log-probability of an accepted move" % label
    rej = ~moved & ~f["accept"]
    rej1 = rej.copy()
    rej1[:, 0] = False
    assert np.array_equal(after[rej1], before[rej1]), "%s: a rejected walker moved" % label
    assert np.array_equal(lp_after[rej1], prev_lp[t, w][rej1]), "%s: a rejected walker's log-probability changed" % label
    r0 = rej[:, 0]
    l0, o0 = lp_after[:, 0][r0], f["lps"][:, 0][r0]
    assert np.array_equal(np.isneginf(l0), np.isneginf(o0))
    assert np.all(np.abs(l0[np.isfinite(o0)] - o0[np.isfinite(o0)]) <= 1e-9 * S), "%s: initial log-probability" % label
    assert not np.isnan(ch).any() and not np.isnan(lpc).any(), "%s: NaN in the chain" % label
    dev_count = np.bincount(w[moved], minlength=EW)
    assert np.array_equal(dev["naccept"], dev_count), "%s: naccept is not the number of moves in the chain" % label
    if not (moved != f["accept"]).any():
        assert np.array_equal(dev["naccept"], np.bincount(w[f["accept"]], minlength=EW))
    if T:
        assert np.array_equal(dev["coords"], ch[-1]) and np.array_equal(dev["final_log_prob"], lpc[-1])
    return ntie, nprop


DE, SN, ST = ("de", 1e-5, None), ("snooker", 1.7), ("stretch", 2.0)
# D, W, n, E, kernel, seeds, moves, iterations, kernels to run (0: several workgroups where possible, 1: one)
CASES = [
    (1, 4, 200, 1, "se", (6,), DE, 300, (0, 1)),                                      # H = 2, the smallest pair set
    (1, 6, 200, 1, "se", (6,), SN, 300, (0, 1)),                                      # H = 3, D - 1 = 0
    (2, 6, 300, 3, "amp", (2 ** 32 + 17,), [(DE, .8), (SN, .2)], 200, (0, 1)),        # odd half, several ensembles, k1 != 0
    (5, 70, 700, 3, "amp+lin2", (123,), [(ST, .5), (DE, .4), (("de", 1e-5, 1.0), .1)], 60, (0, 1)),      # DPAD 8, odd half
    (8, 64, 300, 1, "se", (-(2 ** 40) - 3,), ("de", 0.3, None), 100, (0, 1)),         # the normal matters, stream in LDS
    (8, 256, 2500, 3, "amp+lin1", (125,), SN, 24, (0,)),                             # W max, stream in L2, G clipped
    (9, 18, 300, 1, "amp", (77,), SN, 100, (0, 1)),                                   # DPAD 16, one proposal per pass
    (32, 64, 200, 1, "amp", (31,), [ST, DE, SN], 60, (0, 1)),                         # DPAD 32
    # a single iteration takes ONE move: the case runs once per seed, and the seeds are chosen so that one takes each
    (2, 6, 100, 1, "se", (3, 5), [(DE, .5), (SN, .5)], 1, (0, 1)),
]


def _case_id(c):
    name = lambda m: m[0] if isinstance(m[0], str) else "+".join(x[0][0] if not isinstance(x[0], str) else x[0] for x in m)
    return "D%d-W%d-n%d-E%d-%s-%s-it%d" % (c[0], c[1], c[2], c[3], c[4], name(c[6]), c[7])


@pytest.mark.parametrize("D,W,n,E,kern,seeds,spec,iters,modes", CASES, ids=[_case_id(c) for c in CASES])
def test_device_moves_replay_move_by_move(D, W, n, E, kern, seeds, spec, iters, modes):
    from approxposterior_amd import _lib
    lib = _lib.load()
    X, y, gp, gpo = rp._problem(D, n, kern, seeds[0])
    b, sc = rp._bounds(D), rp._scales(gp, D)
    lp, S = rp._oracle(gpo, y, D), rp._size(gpo, y, X)
    tab = emr.table(spec, D)
    # before anything goes to the device: the free-running reference meets few enough near-ties of its own, and a mixture
    # exercises every listed move (over the case's seeds)
    frees, chosen = {}, set()
    for seed in seeds:
        p0 = rp._start(E, W, D, seed)
        free = emr.run(lp, p0, iters, b, tab, seed=seed, sc=sc)
        ftie = int(_ties(free["decisions"]["margin"], free["decisions"]["face"], S).sum())
        assert ftie * 10 ** 4 <= free["decisions"]["margin"].size, "seed %d: the reference meets %d near-ties" % (seed, ftie)
        chosen |= set(free["move"].ravel().tolist())
        frees[seed] = (p0, free)
    assert chosen == set(range(len(tab))), "the mixture never took move(s) %s" % sorted(set(range(len(tab))) - chosen)
    for seed in seeds:
        p0, free = frees[seed]
        for mode in modes:
            G, cus = rp._expected_groups(E, W, iters, mode)
            fb0 = getattr(gp, "ensemble_fallbacks", 0)
            prev = lib.apgp_ensemble_mode(mode)
            try:
                dev = gp.sample_ensemble(y, p0, iters, b, seed=seed, moves=_objects(spec))
            finally:
                lib.apgp_ensemble_mode(prev)
            fb = getattr(gp, "ensemble_fallbacks", 0) - fb0
            label = "%s seed=%d mode %d" % (_case_id((D, W, n, E, kern, seeds, spec, iters)), seed, mode)
            ntie, nprop = _check(dev, p0, b, tab, seed, sc, lp, S, label, free)
            print("%s: G = %d workgroups per ensemble (%d CUs), %d fallbacks, %d near-ties in %d proposals, acceptance %.3f, "
                  "moves taken %s" % (label, G, cus, fb, ntie, nprop, dev["naccept"].sum() / max(1, nprop),
                                      np.bincount(free["move"].ravel(), minlength=len(tab)).tolist()))


def _old_entry_point(gp, y, p0, iters, b, a, seed, mode):
    """apgp_ensemble_sample_ex as it was called before the move table existed, through ctypes."""
    import torch
    from approxposterior_amd import _lib, gp as agp
    lib = _lib.load()
    E, W, D = p0.shape
    gp.recompute()
    _, dev, _ = gp._rt()
    yy = gp._check_dimensions(y)
    gp._ensure_xs(yy)
    lo, hi = agp._box(b, D, optional=False)
    ks = gp._kernel_struct()
    coords = torch.from_numpy(np.ascontiguousarray(p0)).to(dev)
    logp = torch.empty((E, W), dtype=torch.float64, device=dev)
    nacc = torch.empty((E, W), dtype=torch.int64, device=dev)
    chain = torch.empty((iters, E, W, D), dtype=torch.float64, device=dev)
    lchain = torch.empty((iters, E, W), dtype=torch.float64, device=dev)
    _lib.check(lib.apgp_ensemble_sample_ex(gp._xs.data_ptr(), len(gp._x), ctypes.byref(ks), float(gp.mean.value), lo, hi, W, E,
                                           iters, float(a), agp._seed64(seed), coords.data_ptr(), logp.data_ptr(),
                                           chain.data_ptr(), lchain.data_ptr(), nacc.data_ptr(), mode,
                                           gp._stream(torch)), "apgp_ensemble_sample_ex")
    torch.cuda.synchronize()
    return {"chain": chain.cpu().numpy().reshape(iters, E * W, D), "log_prob": lchain.cpu().numpy().reshape(iters, E * W),
            "naccept": nacc.cpu().numpy().reshape(E * W), "coords": coords.cpu().numpy().reshape(E * W, D),
            "final_log_prob": logp.cpu().numpy().reshape(E * W)}


@pytest.mark.parametrize("D,W,n,E,kern,seed,a,iters", [(2, 6, 300, 3, "amp", 2 ** 32 + 17, 1.5, 200),
                                                      (8, 64, 300, 1, "se", -(2 ** 40) - 3, 1.5, 100)])
def test_default_chain_is_unchanged_by_the_move_table(D, W, n, E, kern, seed, a, iters):
    """moves=None, moves=[StretchMove(a)] and the old C entry point give the same chain bit for bit, on both kernels."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    mcmc = _mcmc()
    X, y, gp, gpo = rp._problem(D, n, kern, seed)
    p0, b = rp._start(E, W, D, seed), rp._bounds(D)
    for mode in (0, 1):
        fb0 = getattr(gp, "ensemble_fallbacks", 0)
        prev = lib.apgp_ensemble_mode(mode)
        try:
            plain = gp.sample_ensemble(y, p0, iters, b, a=a, seed=seed)
            listed = gp.sample_ensemble(y, p0, iters, b, seed=seed, moves=[mcmc.StretchMove(a)])
            old = _old_entry_point(gp, y, p0, iters, b, a, seed, mode)
        finally:
            lib.apgp_ensemble_mode(prev)
        assert getattr(gp, "ensemble_fallbacks", 0) == fb0
        for key in ("chain", "log_prob", "naccept", "coords", "final_log_prob"):
            assert np.array_equal(plain[key], listed[key]), "mode %d: %s differs with moves=[StretchMove(a)]" % (mode, key)
            assert np.array_equal(plain[key], old[key]), "mode %d: %s differs from apgp_ensemble_sample_ex" % (mode, key)
        assert plain["naccept"].sum() > 0
        with pytest.raises(ValueError):
            gp.sample_ensemble(y, p0, iters, b, a=a, seed=seed, moves=[mcmc.StretchMove(a)])      # a beside moves


def test_snooker_from_duplicate_walkers_on_the_device():
    """D = 2, W = 6, three walkers at one point and three at another: a walker whose pivot is a copy of itself proposes NaN
    (the reference's draws say that it happens), which is rejected -- everything stored is finite or -inf, nothing is NaN,
    the chain still moves and the launch does not fall back; the chain is the replay's."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    D, W, T, seed = 2, 6, 50, 21
    X, y, gp, gpo = rp._problem(D, 100, "se", seed)
    b, sc = rp._bounds(D), rp._scales(gp, D)
    lp, S = rp._oracle(gpo, y, D), rp._size(gpo, y, X)
    p0 = np.array([[[0.4, -0.3]] * 3 + [[-0.2, 0.5]] * 3])
    tab = emr.table(SN, D)
    for mode in (0, 1):
        fb0 = getattr(gp, "ensemble_fallbacks", 0)
        prev = lib.apgp_ensemble_mode(mode)
        try:
            dev = gp.sample_ensemble(y, p0, T, b, seed=seed, moves=_mcmc().DESnookerMove())
        finally:
            lib.apgp_ensemble_mode(prev)
        assert getattr(gp, "ensemble_fallbacks", 0) == fb0, "the launch fell back"
        for key in ("chain", "coords"):
            assert np.all(np.isfinite(dev[key])), key
        for key in ("log_prob", "final_log_prob"):
            assert not np.isnan(dev[key]).any() and np.all(np.isfinite(dev[key]) | np.isneginf(dev[key])), key
        f = emr.forced(lp, p0, dev["chain"], b, tab, seed=seed, sc=sc)
        nanq = np.any(np.isnan(f["q"]), axis=-1)
        assert nanq.any(), "the start never produced s == z: the test shows nothing"
        assert not f["accept"][nanq].any() and not f["inside"][nanq].any()
        # the chain against the replay.  Among copies the snooker also proposes q == s exactly (z1 and z2 copies of one
        # point: the projection is 0), a move the chain cannot show: those slots are left out of the comparison, and the
        # device's count of accepted moves lies between the moves the chain shows and those plus the invisible ones.
        ch = dev["chain"]
        t, w = np.arange(T)[None, :, None, None], f["walker"]
        prev = np.concatenate([p0.reshape(1, W, D), ch[:-1]], axis=0)
        before, after = prev[t, w], ch[t, w]
        moved = np.any(after != before, axis=-1)
        moved[:, 0] = np.any(np.abs(after[:, 0] - before[:, 0]) > np.spacing(np.abs(before[:, 0])), axis=-1)
        null = np.all(np.abs(f["q"] - f["before"]) <= np.spacing(np.abs(f["before"])), axis=-1)
        tie = _ties(f["margin"], f["face"], S)
        assert not moved[nanq].any(), "a NaN proposal moved its walker"
        cmp_ = ~null & ~tie
        assert np.array_equal(moved[cmp_], f["accept"][cmp_]), "mode %d: decisions differ from the replay" % mode
        assert int(tie.sum()) * 10 ** 4 <= tie.size
        both = moved & f["accept"] & cmp_
        tol = _position_tolerance(f, tab, sc, D)
        assert np.all(np.abs(after - f["q"])[both] <= tol[both])
        shown = np.bincount(w[moved], minlength=W)
        hidden = np.bincount(w[null & f["accept"]], minlength=W)
        assert np.all(dev["naccept"] >= shown) and np.all(dev["naccept"] <= shown + hidden)
        assert moved.sum() > 0
        print("duplicate walkers, mode %d: %d NaN proposals and %d proposals q == s of %d, %d moves, %d near-ties" % (
            mode, nanq.sum(), null.sum(), moved.size, moved.sum(), tie.sum()))


def test_run_mcmc_on_device_honours_the_moves():
    """runMCMC(onDevice=True, samplerKwargs={"moves": [(DEMove(), .8), (DESnookerMove(), .2)]}) runs that mixture with the
    seed runMCMC draws from NumPy's stream: the chain is the replay's under these moves and not the stretch replay's; the
    chain records its move table."""
    from approxposterior_amd import approx
    mcmc = _mcmc()
    D, W, T = 2, 10, 80
    X, y, gp, gpo = rp._problem(D, 150, "se", 8)
    b = rp._bounds(D)
    lnprior = lambda t: 0.0 if np.all((np.asarray(t) >= b[:, 0]) & (np.asarray(t) <= b[:, 1])) else -np.inf
    ap = approx.ApproxPosterior(theta=X, y=y, gp=gp, lnprior=lnprior, lnlike=lambda t: 0.0,
                                priorSample=lambda m: np.random.uniform(b[:, 0], b[:, 1], size=(m, D)),
                                bounds=[tuple(r) for r in b], algorithm="agp", distributed=False)
    p0 = rp._start(1, W, D, 8)[0]
    np.random.seed(2024)
    seed = np.random.randint(0, 2 ** 31 - 1)                  # what runMCMC draws for its one ensemble
    np.random.seed(2024)
    de, sn = mcmc.DEMove(), mcmc.DESnookerMove()
    with np.errstate(all="ignore"):
        sampler, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": W, "moves": [(de, .8), (sn, .2)]},
                                   mcmcKwargs={"iterations": T, "initial_state": p0},
                                   cache=False, estBurnin=False, thinChains=False, onDevice=True)
    assert [m for m, _ in sampler.moves] == [de, sn] and np.allclose([w for _, w in sampler.moves], [.8, .2])
    dev = {"chain": sampler.get_chain(), "log_prob": sampler.get_log_prob(), "naccept": sampler._naccepted.astype(np.int64),
           "coords": sampler._coords, "final_log_prob": sampler._lp}
    lp, S, sc = rp._oracle(gpo, y, D), rp._size(gpo, y, X), rp._scales(gp, D)
    tab = emr.table([(DE, .8), (SN, .2)], D)
    free = emr.run(lp, p0, T, b, tab, seed=seed, sc=sc)
    assert set(free["move"].ravel().tolist()) == {0, 1}
    ntie, nprop = _check(dev, p0[None], b, tab, seed, sc, lp, S, "runMCMC moves", free)
    print("runMCMC(onDevice=True, moves): seed %d, %d near-ties in %d proposals" % (seed, ntie, nprop))
    with pytest.raises(AssertionError):
        rp._check_chain(dev, p0[None], b, 2.0, seed, sc, lp, S, "runMCMC replayed as a stretch chain")
