"""MI355X: candidates drawn from a priors.JointPrior and its log-density on the device (csrc/ensemble.hip
prior_candidates_kernel, prior_lnprior_kernel), the device ensemble sampler under the prior's support with the lnprior
blobs, and the ApproxPosterior paths that use them.

Gaussian dimensions of the candidate matrix are compared with the NumPy replay (tests/prior_ref.py), which uses scipy's
erfcinv where the device uses its own: |device - replay| <= GAUSS_K eps (sigma (1 + |z|) + |x|), z = (x - mu) / sigma.
Measured on an MI355X: the largest ratio was 1.97 over the mixed-prior cases below and 1.33 over rows in the tails
(|z| up to 5.3); GAUSS_K = 4 keeps a factor of two above that (the tests print the ratio they see)."""
import numpy as np
import pytest
import scipy.stats as ss

import ensemble_ref as er
import prior_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GAUSS_K = 4.0


def _P():
    from approxposterior_amd import priors
    return priors


def _gp(D):
    """A computed GP of dimension D (the candidate and log-density entries only need its device and stream)."""
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(D)
    X = rs.uniform(-1, 1, size=(40, D))
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.ones(D), ndim=D), fit_mean=True, mean=0.0, white_noise=-8.0,
               fit_white_noise=False)
    g.compute(X)
    return g


def _mixed(D, seed=0):
    """Alternating Uniform and Gaussian factors with varied scales (odd dimensions Gaussian)."""
    P = _P()
    rs = np.random.RandomState(100 + seed)
    out = []
    for d in range(D):
        if d % 2 == 0:
            lo = rs.uniform(-50, 10)
            out.append(P.UniformPrior(lo, lo + rs.uniform(0.1, 30)))
        else:
            out.append(P.GaussianPrior(rs.uniform(-5, 5), 10.0 ** rs.uniform(-2, 1.5)))
    return P.JointPrior(out)


def _uniform_only(D):
    P = _P()
    lo = -1.0 - 0.37 * np.arange(D)
    hi = 2.0 + 0.21 * np.arange(D)
    return P.JointPrior([P.UniformPrior(a, b) for a, b in zip(lo, hi)]), lo, hi


def test_uniform_only_priors_are_the_box_candidates():
    for D in range(1, 33):
        J, lo, hi = _uniform_only(D)
        g = _gp(D)
        for seed, off, m in ((12345, 0, 1000), (2 ** 40 + 9, 2 ** 33 + 7, 513)):
            a = g.prior_candidates(m, J, seed, idx_offset=off).cpu().numpy()
            b = g.box_candidates(m, np.stack([lo, hi], axis=1), seed, idx_offset=off).cpu().numpy()
            assert a.shape == (m, D) and np.array_equal(a.view(np.int64), b.view(np.int64)), "D=%d seed=%d" % (D, seed)


def _gauss_ratio(dev, rep, J):
    kind, mu, sigma = J.records()
    g = kind == 1
    z = (rep[:, g] - mu[g]) / sigma[g]
    bound = EPS * (sigma[g] * (1.0 + np.abs(z)) + np.abs(rep[:, g]))
    return np.abs(dev[:, g] - rep[:, g]) / bound


def test_mixed_priors_against_the_replay():
    worst = 0.0
    for D, seed, off in ((1, 3, 0), (2, 77, 5), (5, -4, 2 ** 32 - 3), (8, 2 ** 35 + 1, 0), (17, 901, 10 ** 6), (32, 6, 0)):
        J = _mixed(D, seed % 97)
        g = _gp(D)
        m = 4096
        dev = g.prior_candidates(m, J, seed, idx_offset=off).cpu().numpy()
        rep = prior_ref.prior_candidates_numpy(m, *J.records(), seed, off)
        u = J.kinds == 0
        assert np.array_equal(dev[:, u].view(np.int64), rep[:, u].view(np.int64)), "Uniform dimensions, D=%d" % D
        if (~u).any():
            r = _gauss_ratio(dev, rep, J)
            worst = max(worst, float(r.max()))
            assert np.all(np.isfinite(dev)) and r.max() <= GAUSS_K, "D=%d: %.2f > %g" % (D, r.max(), GAUSS_K)
    print("Gaussian dimensions: largest |device - replay| / (eps (sigma (1 + |z|) + |x|)) = %.3f" % worst)


def test_tails_against_the_replay():
    """Rows whose uniforms lie close to 0 and 1 (the tails of erfcinv), found by scanning the replay's stream."""
    P = _P()
    J = P.JointPrior([P.GaussianPrior(0.5, 2.0), P.GaussianPrior(-1.0, 0.5)])
    u = prior_ref.uniforms(2 ** 20, 2, 2024, 0)
    rows = np.flatnonzero(np.any((u < 1e-4) | (u > 1 - 1e-4), axis=1))
    assert len(rows) > 100
    g = _gp(2)
    dev = np.concatenate([g.prior_candidates(1, J, 2024, idx_offset=int(r)).cpu().numpy() for r in rows[:200]])
    rep = np.concatenate([prior_ref.prior_candidates_numpy(1, *J.records(), 2024, int(r)) for r in rows[:200]])
    r = _gauss_ratio(dev, rep, J)
    print("tails: largest ratio %.3f, |z| up to %.2f" % (r.max(), np.abs((rep - [0.5, -1.0]) / [2.0, 0.5]).max()))
    assert r.max() <= GAUSS_K


def test_shards_concatenate_to_the_whole_matrix():
    J = _mixed(7, 1)
    g = _gp(7)
    whole = g.prior_candidates(10007, J, 31337).cpu().numpy()
    cuts = [0, 1, 256, 3000, 3001, 10007]
    parts = [g.prior_candidates(b - a, J, 31337, idx_offset=a).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts).view(np.int64), whole.view(np.int64))
    assert g.prior_candidates(0, J, 31337).shape == (0, 7)


def test_a_million_draws_have_the_prior_moments():
    P = _P()
    pri = [P.GaussianPrior(3.0, 0.5), P.UniformPrior(-2.0, 6.0), P.GaussianPrior(-100.0, 20.0), P.UniformPrior(0.0, 1e-3)]
    J = P.JointPrior(pri)
    g = _gp(4)
    n = 10 ** 6
    x = g.prior_candidates(n, J, 8675309).cpu().numpy()
    for d, p in enumerate(pri):
        m, s = p.dist.mean(), p.dist.std()
        assert abs(x[:, d].mean() - m) <= 5 * s / np.sqrt(n), d
        assert abs(x[:, d].std() - s) <= 5 * s * np.sqrt(0.5 / n) * (1.0 if isinstance(p, P.GaussianPrior) else 1.2), d
        ks = ss.kstest(x[:, d], p.dist.cdf)
        assert ks.pvalue > 1e-3, (d, ks)
    assert np.all((x[:, 1] >= -2.0) & (x[:, 1] <= 6.0)) and np.all((x[:, 3] >= 0.0) & (x[:, 3] <= 1e-3))


def _lnprior_device(g, J, X):
    import torch
    from approxposterior_amd import _lib
    lib = _lib.load()
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0")
    out = torch.empty(len(X), dtype=torch.float64, device="cuda:0")
    kind, p0, p1 = J.records()
    _lib.check(lib.apgp_prior_lnprior(Xd.data_ptr(), len(X), J.ndim, kind.ctypes.data, p0.ctypes.data, p1.ctypes.data,
                                      out.data_ptr(), None), "apgp_prior_lnprior")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_lnprior_agrees_with_get_lnprior():
    P = _P()
    for D in (1, 3, 8, 32):
        J = _mixed(D, D)
        rs = np.random.RandomState(D)
        sup = J.support()
        bnd = np.array(J.bounds())
        lo, hi = bnd[:, 0], bnd[:, 1]
        X = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rs.uniform(size=(5000, D))
        X[:50] = np.clip(X[:50], lo, hi)
        uni = np.flatnonzero(J.kinds == 0)
        X[50, uni] = sup[uni, 0]                              # exactly on the lower faces
        X[51, uni] = sup[uni, 1]                              # exactly on the upper faces
        X[52:56, 0] = [np.inf, -np.inf, np.nan, np.nan]
        if D > 1:
            X[56:59, 1] = [np.inf, -np.inf, np.nan]
        X[60:80] = J.sample(20)
        got = _lnprior_device(None, J, X)
        with np.errstate(invalid="ignore"):
            want = np.array([P.get_lnprior(x, J.priors) for x in X])
        assert np.array_equal(np.isneginf(got), ~np.isfinite(want)) and not np.isnan(got).any(), D
        f = np.isfinite(want)
        assert np.all(np.abs(got[f] - want[f]) <= 1e-12 * (1.0 + np.abs(want[f]))), D
        assert np.isfinite(got[50]) and np.isfinite(got[51]) and np.isneginf(got[52:56]).all()
        assert np.array_equal(np.isfinite(got), np.isfinite(J.batch(X)))


# ------------------------------------------------------------------------ the ensemble sampler under a JointPrior
def _replay_mod():
    import test_gpu_ensemble_replay as R
    return R


def _finite_face(q, lo, hi):
    """ensemble_ref._face over the dimensions with finite edges only (an open dimension has no face)."""
    lo, hi = np.broadcast_to(lo, q.shape), np.broadcast_to(hi, q.shape)
    fin = np.isfinite(lo) & np.isfinite(hi)
    with np.errstate(invalid="ignore"):
        d = np.minimum(np.abs(q - lo), np.abs(hi - q)) / (hi - lo)
    return np.min(np.where(fin, d, np.inf), axis=-1)


def _ens_prior(D):
    """Uniform factors on dimension 0 and D - 1 (the box of the replay test's start, walkers outside and on faces there),
    Gaussian factors elsewhere, centred on the training box."""
    P = _P()
    b = _replay_mod()._bounds(D)
    fac = []
    for d in range(D):
        if d == 0 or d == D - 1:
            fac.append(P.UniformPrior(b[d, 0], b[d, 1]))
        else:
            fac.append(P.GaussianPrior(0.5 * (b[d, 0] + b[d, 1]), 0.3 * (b[d, 1] - b[d, 0])))
    return P.JointPrior(fac)


ENS_CASES = [
    (3, 8, 200, 1, "se", 5, 2.0, 150),
    (4, 10, 300, 3, "amp+lin1", 2 ** 33 + 1, 1.5, 80),
    (9, 18, 300, 1, "amp", -7, 2.0, 60),
    (17, 34, 250, 1, "se", 123, 3.0, 40),
]


@pytest.mark.parametrize("D,W,n,E,kern,seed,a,iters", ENS_CASES, ids=["D%d-W%d-E%d" % (c[0], c[1], c[3]) for c in ENS_CASES])
def test_sampler_under_a_joint_prior_replays_move_by_move(monkeypatch, D, W, n, E, kern, seed, a, iters):
    R = _replay_mod()
    from approxposterior_amd import _lib
    lib = _lib.load()
    monkeypatch.setattr(er, "_face", _finite_face)
    J = _ens_prior(D)
    sup = J.support()
    assert np.isinf(sup[1:-1]).all()
    X, y, gp, gpo = R._problem(D, n, kern, seed)
    p0 = R._start(E, W, D, seed)
    sc, lp, S = R._scales(gp, D), R._oracle(gpo, y, D), R._size(gpo, y, X)
    free = er.run(lp, p0, iters, sup, a=a, seed=seed, sc=sc)
    for mode in (0, 1):
        prev = lib.apgp_ensemble_mode(mode)
        try:
            dev = gp.sample_ensemble(y, p0, iters, None, a=a, seed=seed, prior=J)
        finally:
            lib.apgp_ensemble_mode(prev)
        label = "JointPrior D=%d W=%d E=%d %s mode %d" % (D, W, E, kern, mode)
        ntie, nprop = R._check_chain(dev, p0, sup, a, seed, sc, lp, S, label, free)
        # on the Uniform dimensions the walkers with a finite log-probability stay in [low, high] (to the ulp of the
        # kernel's x sc / sc round trip)
        ch = dev["chain"].reshape(-1, D)
        b = R._bounds(D)[[0, D - 1]]
        tol = 4 * EPS * np.abs(b).max(axis=1)
        inside = (ch[:, [0, D - 1]] >= b[:, 0] - tol) & (ch[:, [0, D - 1]] <= b[:, 1] + tol)
        assert np.all(inside | ~np.isfinite(dev["log_prob"].reshape(-1, 1)))
        # blobs: the prior's log-density at every stored state, NaN where it is -inf (the walker outside the box)
        bl = dev["blobs"]
        want = J.batch(ch).reshape(iters, E * W)
        assert bl.shape == dev["log_prob"].shape
        assert np.array_equal(np.isnan(bl), np.isneginf(want))
        f = np.isfinite(want)
        assert np.all(np.abs(bl[f] - want[f]) <= 1e-12 * (1.0 + np.abs(want[f]))), label
        assert np.all(np.isnan(bl[np.isneginf(dev["log_prob"])])), label
        print("%s: %d near-ties in %d proposals, acceptance %.3f, open-dimension range %.2f"
              % (label, ntie, nprop, dev["naccept"].sum() / max(1, nprop), np.ptp(ch[:, 1:-1]) if D > 2 else 0.0))


# ------------------------------------------------------------------------------------------- ApproxPosterior
def _ap_problem(D=3, n=120, seed=0, first=(-2.0, 2.0)):
    """GP over a smooth bump whose mean constant lies well below the data: the surrogate falls off away from the
    training set, so a chain on the open (Gaussian) dimensions stays near it.  Dimension 0 is Uniform on ``first``."""
    from approxposterior_amd import approx, gp as agp
    P = _P()
    J = P.JointPrior([P.UniformPrior(*first)] + [P.GaussianPrior(0.3 * d, 0.8) for d in range(1, D)])
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2.5, 2.5, size=(n, D))
    y = -0.5 * np.sum((X - 0.3) ** 2 / 0.6, axis=1)
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 1.5), ndim=D), fit_mean=True, mean=float(y.min()) - 5.0,
               white_noise=-6.0, fit_white_noise=False)
    g.compute(X)
    ap = approx.ApproxPosterior(theta=X, y=y, gp=g, lnprior=J, lnlike=lambda t: 0.0, priorSample=J.sample,
                                bounds=J.bounds(), algorithm="agp", distributed=False)
    return ap, J


def test_run_mcmc_on_device_with_a_gaussian_prior():
    ap, J = _ap_problem()
    W, T, burn = 32, 2000, 500
    rs = np.random.RandomState(9)
    p0 = np.column_stack([rs.uniform(-0.5, 0.5, W)] + [0.3 + 0.2 * rs.randn(W) for _ in range(2)])
    kw = dict(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": T, "initial_state": p0}, cache=False,
              estBurnin=False, thinChains=False)
    np.random.seed(1)
    dev, _, _ = ap.runMCMC(onDevice=True, **kw)
    np.random.seed(1)
    host, _, _ = ap.runMCMC(onDevice=False, **kw)
    bd, bh = dev.get_blobs(), host.get_blobs()
    assert bd is not None and bd.shape == bh.shape == (T, W)
    cd = dev.get_chain(discard=burn, flat=True)
    ch = host.get_chain(discard=burn, flat=True)
    f = np.isfinite(bd)
    assert f.mean() > 0.99
    want = J.batch(dev.get_chain().reshape(-1, 3)).reshape(T, W)
    assert np.all(np.abs(bd[f] - want[f]) <= 1e-12 * (1.0 + np.abs(want[f])))
    sd = np.std(ch, axis=0)

    def mcse(s):
        # Monte Carlo error of the mean: the spread of the per-walker means over sqrt(walkers)
        return np.std(s.get_chain(discard=burn).mean(axis=0), axis=0, ddof=1) / np.sqrt(W)
    err = np.sqrt(mcse(dev) ** 2 + mcse(host) ** 2)
    diff = np.abs(cd.mean(axis=0) - ch.mean(axis=0))
    print("runMCMC device vs host: marginal means %s vs %s, |diff| / MC error %s" % (cd.mean(axis=0), ch.mean(axis=0),
                                                                                diff / err))
    assert np.all(diff < 5.0 * err), diff / err
    assert np.all(np.abs(np.std(cd, axis=0) / sd - 1.0) < 0.25)
    assert np.all((cd[:, 0] >= -2.0) & (cd[:, 0] <= 2.0))


def test_find_next_point_draws_from_the_prior_on_the_device():
    from approxposterior_amd import utility as ut
    ap, J = _ap_problem(D=4, seed=3)
    M = 20000
    np.random.seed(42)
    point = ap.findNextPoint(computeLnLike=False, nCandidates=M, deviceCandidates=True, verbose=False, cache=False)
    np.random.seed(42)
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    T = ap.gp.prior_candidates(M, J, seed).cpu().numpy()
    want, _ = ut.sweepObjective(ap.utility, ap.y, ap.gp, T, bounds=[tuple(r) for r in J.support()])
    assert np.array_equal(point, want)


def test_host_candidate_sweep_is_gated_by_the_support():
    """priorSample draws outside the Uniform factor [-2, 0], which excludes the bump at 0.3: the sweep must not pick
    them (the ungated winner lies out there), and the winner is sweepObjective's under the support's gate."""
    from approxposterior_amd import utility as ut
    ap, J = _ap_problem(D=3, seed=5, first=(-2.0, 0.0))
    rs = np.random.RandomState(0)
    cand = rs.uniform(-6.0, 6.0, size=(5000, 3))
    ap.priorSample = lambda m: cand[:m]
    point = ap.findNextPoint(computeLnLike=False, nCandidates=5000, deviceCandidates=False, verbose=False, cache=False)
    assert -2.0 <= point[0] <= 0.0
    want, _ = ut.sweepObjective(ap.utility, ap.y, ap.gp, cand, bounds=[tuple(r) for r in J.support()])
    free, _ = ut.sweepObjective(ap.utility, ap.y, ap.gp, cand)
    assert np.array_equal(point, want) and not -2.0 <= free[0] <= 0.0
    print("ungated winner %s, gated winner %s" % (free, point))
