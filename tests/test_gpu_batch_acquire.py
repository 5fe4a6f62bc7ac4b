"""GPU (``-m gpu``): batch design-point selection (GP.acquire_batch, apgp_acquire_fantasy; DESIGN.md "Batch design
points") against the slow path it replaces -- the device GP extended by the picks at their predicted means through
compute(previous=) and swept again in full -- and against the NumPy restatement in tests/fantasy_ref.py; then
findNextPoint(batchSize=...) end to end."""
import concurrent.futures
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fantasy_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _fixture(n, d, m, seed, fit_amp=True, gated=True):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(seed)
    X = rs.uniform(-5.0, 5.0, size=(n, d))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1) / 1000.0
    ell = 1.5 * 10.0 / n ** (1.0 / d) * rs.uniform(1.0, 2.0, size=d)
    log_c = np.log(rs.uniform(0.5, 2.0) * np.std(y) ** 2 / d) if fit_amp else None
    amp = d * np.exp(log_c) if fit_amp else 1.0
    wn = float(np.log(1e-6 * amp))
    k = agp.ExpSquaredKernel(ell ** 2, ndim=d)
    if fit_amp:
        k = agp.Product(agp.ConstantKernel(log_c, ndim=d), k)
    mean = float(np.mean(y))
    gp = agp.GP(kernel=k, fit_mean=True, mean=mean, white_noise=wn, fit_white_noise=False)
    gp.compute(X)
    T = rs.uniform(-5.5, 5.5, size=(m, d))
    bounds = mask = None
    if gated:
        bounds = [(-5.0, 5.0)] * d
        mask = rs.rand(m) > 0.1
    ref = dict(amp=amp, inv_metric=1.0 / ell ** 2, diag_add=float(np.exp(wn)), mean=mean, lin_coef=0.0, lin_order=1)
    return gp, X, y, T, bounds, mask, amp, ref


def _slow_step(gp, X, y, T, picks, mus, kind, bounds, mask, mode):
    """The slow path at one step: the GP extended by the picks at their predicted means (hyper-parameters unchanged),
    then a full sweep."""
    from approxposterior_amd import gp as agp
    if not picks:
        g = gp
    else:
        g = agp.GP(kernel=gp.kernel, fit_mean=True, mean=gp.mean, white_noise=gp.white_noise, fit_white_noise=False)
        g.set_parameter_vector(gp.get_parameter_vector())
        g.compute(np.vstack([X, T[picks]]), previous=gp)
    g.variance_mode = mode
    ye = np.concatenate([y, mus])
    return g.acquire(ye, T, kind, bounds=bounds, mask=mask, return_all=True)


def _tol_u(kind, mu, var, tmu, tvar, ybest):
    """The utility's own conditioning applied to the mu / sigma^2 tolerances (test_gpu_parity.py style)."""
    h = max(tvar, 1e-3 * abs(var), 1e-300)
    dv = abs(fr.utility(kind, mu, var + h, ybest=ybest) - fr.utility(kind, mu, max(var - h, 0.5 * var), ybest=ybest)) \
        / (h + min(h, 0.5 * var))
    return 10.0 * (2.0 * tmu + tvar * dv) + 1e-12 * abs(fr.utility(kind, mu, var, ybest=ybest))


@pytest.mark.parametrize("mode", ["inverse", "solve"])
@pytest.mark.parametrize("kind", ["agp", "bape", "jones"])
def test_q1_is_acquire_bit_for_bit(kind, mode):
    gp, X, y, T, bounds, mask, amp, _ = _fixture(300, 8, 5000, 11)
    gp.variance_mode = mode
    bi, bu = gp.acquire(y, T, kind, bounds=bounds, mask=mask)
    idx, ub = gp.acquire_batch(y, T, kind, 1, bounds=bounds, mask=mask)
    assert idx.tolist() == [bi]
    assert np.float64(ub[0]).tobytes() == np.float64(bu).tobytes()


CASES = [  # n, d, m, q, kind, mode, seed
    (50, 2, 2000, 5, "bape", "inverse", 1),
    (50, 2, 2000, 8, "agp", "solve", 2),
    (300, 8, 2000, 8, "jones", "inverse", 3),
    (300, 2, 200000, 5, "agp", "inverse", 4),
    (1152, 8, 200000, 8, "bape", "solve", 5),
    (1152, 2, 2000, 2, "jones", "solve", 6),
    (300, 8, 200000, 2, "bape", "inverse", 7),
    (1152, 8, 2000, 5, "agp", "inverse", 8),
]


@pytest.mark.parametrize("n, d, m, q, kind, mode, seed", CASES)
def test_batch_against_the_slow_path(n, d, m, q, kind, mode, seed):
    gp, X, y, T, bounds, mask, amp, _ = _fixture(n, d, m, seed)
    gp.variance_mode = mode
    cond = gp.cond_estimate
    assert cond <= 1e8
    tol = max(1e-12, 200 * cond * EPS)
    tvar, tmu = tol * amp, tol * max(1.0, np.abs(y).max())
    idx, ub, u_f, mu_f, var_f = gp.acquire_batch(y, T, kind, q, bounds=bounds, mask=mask, return_all=True)
    assert np.all(idx >= 0)
    picks, mus = [], []
    for j in range(q):
        _, _, u_s, mu_s, var_s = _slow_step(gp, X, y, T, picks, mus, kind, bounds, mask, mode)
        ybest = max(float(np.max(y)), max(mus) if mus else -np.inf)
        b = fr.argmin(u_s)
        t_u = _tol_u(kind, mu_s[b], var_s[b], tmu, tvar, ybest)
        # the fast pick is optimal on the slow path up to rounding ...
        assert u_s[idx[j]] <= u_s[b] + t_u, (j, idx[j], b, u_s[idx[j]], u_s[b], t_u)
        assert abs(ub[j] - u_s[idx[j]]) <= t_u
        # ... and the same pick wherever the slow path's runner-up is further away than that
        w = np.where(np.isnan(u_s), np.inf, u_s)
        w[b] = np.inf
        if np.min(w) - u_s[b] > 2 * t_u:
            assert idx[j] == b, j
        assert np.abs(mu_s - mu_f).max() <= 10 * tmu
        picks.append(int(idx[j]))
        mus.append(float(mu_f[idx[j]]))
    # the final variance (q - 1 fantasies) is the slow path's
    assert np.abs(var_s - var_f).max() <= max(1e-9, 10 * tol) * amp


@pytest.mark.parametrize("n, d, m, q, kind, mode, seed", [c for c in CASES if c[2] <= 2000])
def test_batch_against_the_numpy_recursion(n, d, m, q, kind, mode, seed):
    gp, X, y, T, bounds, mask, amp, ref = _fixture(n, d, m, seed)
    gp.variance_mode = mode
    tol = max(1e-12, 200 * gp.cond_estimate * EPS)
    idx, ub, u_f, mu_f, var_f = gp.acquire_batch(y, T, kind, q, bounds=bounds, mask=mask, return_all=True)
    idx_r, ub_r, mu_r, vs_r = fr.fantasy_batch(X, y, T, kind, q, ref, bounds=bounds, mask=mask)
    assert np.array_equal(idx, idx_r), (idx, idx_r)
    assert np.abs(mu_f - mu_r).max() <= 10 * tol * max(1.0, np.abs(y).max())
    assert np.abs(var_f - vs_r[-1]).max() <= max(1e-9, 10 * tol) * amp
    assert np.allclose(ub, ub_r, rtol=1e-6, atol=1e-9)


def test_device_candidates_take_the_tensor_path():
    from approxposterior_amd import priors
    gp, X, y, T, bounds, mask, amp, _ = _fixture(300, 2, 10, 21, gated=False)
    box = [(-5.0, 5.0), (-5.0, 5.0)]
    Td = gp.box_candidates(50000, box, seed=123)
    a = gp.acquire_batch(y, Td, "bape", 4, bounds=box)
    b = gp.acquire_batch(y, Td.cpu().numpy(), "bape", 4, bounds=box)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    assert a[0][0] == gp.acquire(y, Td, "bape", bounds=box)[0]
    joint = priors.JointPrior([priors.UniformPrior(-5.0, 5.0), priors.GaussianPrior(0.5, 1.5)])
    Tp = gp.prior_candidates(50000, joint, seed=7)
    gate = [tuple(r) for r in joint.support()]
    a = gp.acquire_batch(y, Tp, ["agp", "bape", "agp"], 3, bounds=gate)
    b = gp.acquire_batch(y, Tp.cpu().numpy(), ["agp", "bape", "agp"], 3, bounds=gate)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    assert np.all(a[0] >= 0)


def test_no_admissible_candidate():
    gp, X, y, T, bounds, mask, amp, _ = _fixture(50, 2, 500, 3)
    idx, ub = gp.acquire_batch(y, T, "bape", 3, mask=np.zeros(len(T), dtype=bool))
    assert idx.tolist() == [-1, -1, -1] and np.all(np.isposinf(ub))


def _rosen_ap(m0, seed):
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    np.random.seed(seed)
    theta = np.array(lh.rosenbrockSample(m0))
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y)
    return approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                  priorSample=lh.rosenbrockSample, bounds=[(-5, 5), (-5, 5)], algorithm="bape")


def test_find_next_point_batches_with_and_without_a_pool(tmp_path, monkeypatch):
    from approxposterior_amd import likelihood as lh
    monkeypatch.chdir(tmp_path)
    out = []
    for pool in (None, concurrent.futures.ThreadPoolExecutor(2)):
        ap = _rosen_ap(50, 5)
        with np.errstate(all="ignore"):
            theta, val = ap.findNextPoint(nCandidates=20000, numNewPoints=6, batchSize=3, computeLnLike=True,
                                          pool=pool, seed=5, verbose=False)
        if pool is not None:
            pool.shutdown()
        assert theta.shape == (6, 2) and val.shape == (6, 1)
        assert len(ap.y) == 56 and len(ap.gp._x) == 56
        assert np.array_equal(ap.theta[50:], theta)
        want = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
        assert np.array_equal(ap.y[50:], want) and np.array_equal(val[:, 0], want)
        assert len(set(map(tuple, theta))) == 6
        out.append((theta, ap.y.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("device", [False, True])
def test_batch_size_one_is_the_point_by_point_search(device, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    res = []
    for bs in (None, 1):
        ap = _rosen_ap(40, 9)
        with np.errstate(all="ignore"):
            ap.findNextPoint(nCandidates=20000, numNewPoints=3, batchSize=bs, computeLnLike=True, seed=9,
                             deviceCandidates=device, verbose=False)
        res.append((ap.theta, ap.y))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _min_pairwise(p):
    return min(np.linalg.norm(p[i] - p[k]) for i in range(len(p)) for k in range(i))


def test_a_batch_is_spread_out_where_independent_picks_are_not(tmp_path, monkeypatch):
    """What the feature is for: without absorbing anything, ``numNewPoints=q`` alone re-picks near one utility optimum;
    the batch's fantasies push the later picks away from the earlier ones."""
    monkeypatch.chdir(tmp_path)
    q = 5
    ap = _rosen_ap(50, 13)
    with np.errstate(all="ignore"):
        np.random.seed(13)
        plain = ap.findNextPoint(nCandidates=20000, numNewPoints=q, computeLnLike=False, verbose=False)
        np.random.seed(13)
        batch = ap.findNextPoint(nCandidates=20000, numNewPoints=q, batchSize=q, computeLnLike=False, verbose=False)
    assert batch.shape == (q, 2) and len(set(map(tuple, batch))) == q
    assert _min_pairwise(batch) > _min_pairwise(plain), (batch, plain)
