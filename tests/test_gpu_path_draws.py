"""GPU (``-m gpu``): posterior function draws (apgp_path_draws, GP.sample_paths, GP.thompson_batch; DESIGN.md "Posterior
function draws") against the NumPy restatement and the rounding budget of tests/pathdraw_ref.py, the arg-min contract,
the two exact consequences of Matheron's rule through the GP layer, the moments of many draws, Thompson batches,
sample_conditional, and findNextPoint / bayesOpt with batchMethod="thompson" end to end."""
import concurrent.futures
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ref as fref  # noqa: E402
import kvalue_ref as kr  # noqa: E402
import pathdraw_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300


def _ks(k):
    from approxposterior_amd import _lib
    ks = _lib.KernelStruct()
    ks.ndim, ks.lin_order, ks.amp, ks.diag_add, ks.lin_coef = k.ndim, k.lin_order, k.amp, k.diag_add, k.lin_coef
    ks.inv_metric[:k.ndim] = k.inv_metric.tolist()
    return ks


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _box(bounds):
    from approxposterior_amd import _lib
    if bounds is None:
        return None, None
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    arr = ctypes.c_double * _lib.MAX_DIM
    return arr(*b[:, 0]), arr(*b[:, 1])


def dev_path_draws(T, X, V, Z, b, W, Wl, k, mean, bounds=None, mask=None, idx_offset=0, with_f=True):
    """apgp_path_draws through the C ABI: (F (S, M) pre-filled with a sentinel or None, indices (S,), u (S,))."""
    import torch
    from approxposterior_amd import _lib
    lib = _lib.load()
    ks = _ks(k)
    m, S, R = len(T), len(W), len(Z)
    xs_d = None
    if V is not None:
        n = len(X)
        xs_d = torch.empty(lib.apgp_packed_train_len(n, k.ndim), dtype=torch.float64, device="cuda:0")
        Xd, ad = _dev(X), _dev(np.full(n, np.nan))          # (the alpha column is not read)
        assert lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs_d.data_ptr(), None) == 0
    Td, Zd, bd, Wd = _dev(T), _dev(Z), _dev(b), _dev(W)
    Wld = _dev(Wl) if Wl is not None else None
    Vd = _dev(V) if V is not None else None
    md = _dev(mask, np.uint8) if mask is not None else None
    F = torch.full((S, m), SENTINEL, dtype=torch.float64, device="cuda:0") if with_f else None
    part = torch.empty(max(lib.apgp_path_draws_work_len(m, S), 2), dtype=torch.float64, device="cuda:0")
    best = torch.empty(2 * S, dtype=torch.float64, device="cuda:0")
    lo, hi = _box(bounds)
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    rc = lib.apgp_path_draws(Td.data_ptr(), m, idx_offset, ptr(xs_d), len(X) if V is not None else 0, ctypes.byref(ks),
                             mean, ptr(Vd), Zd.data_ptr(), bd.data_ptr(), Wd.data_ptr(), ptr(Wld), R, S, lo, hi,
                             ptr(md), ptr(F), part.data_ptr(), best.data_ptr(), None)
    assert rc == 0, lib.apgp_last_error()
    torch.cuda.synchronize()
    bb = best.cpu().numpy().reshape(S, 2)
    return (F.cpu().numpy() if with_f else None), bb[:, 1].copy().view(np.int64), bb[:, 0].copy()


# n, m, R, S, D, P, idx_offset: every value of the issue's lists appears; one and several LDS tiles of training rows and
# of features (64 rows each) both meet the one-draw kernel, the 8-, 16- and 32-column kernels
# (the `form` fixture runs each with the vector contraction and, where that kernel exists, the matrix-core one)
CASES = [
    (50, 1, 1, 1, 1, None, 0),
    (50, 63, 100, 17, 3, 0, 0),
    (130, 1000, 1028, 5, 8, 1, 7),
    (600, 63, 100, 32, 20, 2, 0),
    (600, 63, 1028, 16, 8, None, 0),
    (130, 63, 1, 16, 3, None, 0),
    (50, 63, 1028, 1, 20, 1, 3),
    (600, 63, 1, 5, 1, 2, 0),
    (50, 1000, 100, 32, 3, None, 10 ** 10),
]


@functools.lru_cache(maxsize=None)
def _reference(n, m, R, S, D, P, with_v=True):
    c = pr.case(n, m, R, S, D, order=P, seed=n + m + R + S + D)
    V = c["V"] if with_v else None
    F = pr.draws(c["T"], c["X"], V, c["Z"], c["b"], c["W"], c["Wl"], c["k"], c["mean"])
    bud, mag = pr.budget(c["T"], c["X"], V, c["Z"], c["b"], c["W"], c["Wl"], c["k"], c["mean"])
    for a in (F, bud, mag):
        a.setflags(write=False)
    return c, F, bud, mag


@pytest.fixture(params=["vector", "matrix"])
def form(request):
    """Both contractions (apgp_path_draws_mode): 1 the vector units for every shape, 2 the matrix cores wherever that
    kernel exists (more than one draw, D <= 8) and the vector units elsewhere."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    was = lib.apgp_path_draws_mode({"vector": 1, "matrix": 2}[request.param])
    yield request.param
    lib.apgp_path_draws_mode(was)


@pytest.mark.parametrize("n, m, R, S, D, P, off", CASES)
def test_draws_within_the_budget(n, m, R, S, D, P, off, form):
    c, F_ref, bud, mag = _reference(n, m, R, S, D, P)
    F, idx, u = dev_path_draws(c["T"], c["X"], c["V"], c["Z"], c["b"], c["W"], c["Wl"] if P is not None else None,
                               c["k"], c["mean"], idx_offset=off)
    ratio = np.abs(F - F_ref) / bud
    print("max error / budget %.3f, budget / magnitude %.2e" % (ratio.max(), (bud / mag).max()))
    assert F.shape == (S, m) and np.all(np.isfinite(F))
    assert ratio.max() <= 1.0
    # the records: the arg-min of u = -f of the device's own values, ties to the lowest index
    for s in range(S):
        assert (idx[s], u[s]) == pr.argmin(F[s], np.ones(m, dtype=bool), off), s


@pytest.mark.parametrize("n, m, R, S, D, P, off", [CASES[1], CASES[2], CASES[6]])
def test_prior_draws_alone_with_a_null_v(n, m, R, S, D, P, off, form):
    c, F_ref, bud, mag = _reference(n, m, R, S, D, P, with_v=False)
    F, idx, u = dev_path_draws(c["T"], None, None, c["Z"], c["b"], c["W"], c["Wl"], c["k"], c["mean"], idx_offset=off)
    ratio = np.abs(F - F_ref) / bud
    print("max error / budget %.3f" % ratio.max())
    assert ratio.max() <= 1.0


def test_argmin_contract(form):
    n, m, R, S, D = 50, 300, 100, 5, 3
    c = pr.case(n, m, R, S, D, seed=77)
    T = c["T"].copy()
    args = (c["X"], c["V"], c["Z"], c["b"], c["W"], None, c["k"], c["mean"])
    F0, idx0, _ = dev_path_draws(T, *args)
    # every draw's winning row duplicated further down AND further up: the lowest index wins
    w = int(idx0[0])
    T[(w + 100) % m] = T[w]
    lowest = min(w, (w + 100) % m)
    # a NaN-coordinate row, a masked row and an out-of-box row -- each a copy of draw 1's winner, so each would win
    w1 = next(int(g) for g in idx0[1:] if g not in (w, (w + 100) % m))
    rows =[r for r in range(m) if r not in (w, (w + 100) % m, w1)][:3]
    T[rows] = T[w1]
    T[rows[0], 1] = np.nan
    mask = np.ones(m, dtype=np.uint8)
    mask[rows[1]] = 0
    bounds = [(-2.2, 2.2)] * D
    T[rows[2], 0] = 2.3
    mask[w1] = 0                                           # and draw 1's own winner is masked too
    F, idx, u = dev_path_draws(T, *args, bounds=bounds, mask=mask, idx_offset=1000)
    adm = pr.admissible(T, bounds, mask)
    assert not adm[rows].any() and not adm[w1]
    assert np.all(np.isnan(F[:, ~adm])) and np.all(np.isfinite(F[:, adm]))
    assert idx[0] == 1000 + lowest
    for s in range(S):
        assert (idx[s], u[s]) == pr.argmin(F[s], adm, 1000), s
        assert idx[s] - 1000 not in rows and idx[s] - 1000 != w1
    # without F the records are the same
    _, idx2, u2 = dev_path_draws(T, *args, bounds=bounds, mask=mask, idx_offset=1000, with_f=False)
    assert np.array_equal(idx, idx2) and u.tobytes() == u2.tobytes()
    # everything masked
    F, idx, u = dev_path_draws(T, *args, mask=np.zeros(m, dtype=np.uint8))
    assert idx.tolist() == [-1] * S and np.all(np.isposinf(u)) and np.all(np.isnan(F))


def _gp_fixture(n, d, seed, diag_rel=1e-6):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(seed)
    X = rs.uniform(-5.0, 5.0, size=(n, d))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1) / 1000.0
    ell = 1.5 * 10.0 / n ** (1.0 / d) * rs.uniform(1.0, 2.0, size=d)
    log_c = np.log(rs.uniform(0.5, 2.0) * np.std(y) ** 2 / d)
    amp = d * np.exp(log_c)
    wn = float(np.log(diag_rel * amp))
    k = agp.Product(agp.ConstantKernel(log_c, ndim=d), agp.ExpSquaredKernel(ell ** 2, ndim=d))
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(np.mean(y)), white_noise=wn, fit_white_noise=False)
    gp.compute(X)
    ref = kr.kern(1.0 / ell ** 2, amp=amp, diag_add=float(np.exp(wn)))
    return gp, X, y, ref


@pytest.mark.parametrize("mode", ["inverse", "solve"])
@pytest.mark.parametrize("n, d", [(130, 2), (600, 8)])
def test_zero_weights_reproduce_the_predictive_mean(n, d, mode):
    gp, X, y, k = _gp_fixture(n, d, 3 * n + d)
    gp.variance_mode = mode
    rs = np.random.RandomState(1)
    T = rs.uniform(-5.0, 5.0, size=(200, d))
    mu = gp.predict(y, T, return_cov=False)
    R, S = 100, 3
    paths = gp._paths_from(y, rs.standard_normal((R, d)), rs.uniform(0, 2 * np.pi, R), np.zeros((S, R)),
                           np.zeros((S, d)), np.zeros((S, n)))
    F = paths.evaluate(T)
    alpha = gp._alpha.cpu().numpy()
    V = paths.V.cpu().numpy()
    # both sides are sum_n k(t, x_n) alpha_n + mean with the same alpha: each within the mean kernel's budget of the
    # exact sum -- kvalue_ref's bound of every k times |alpha|, n + 2 roundings of the running sum
    assert np.array_equal(V, np.repeat(alpha[:, None], S, axis=1))
    kabs = np.abs(kr.truth_ld(T, X, k).astype(np.float64))
    tol = kr.budget(T, X, k) @ np.abs(alpha) + (n + 2) * pr.U * (abs(gp.mean.value) + kabs @ np.abs(alpha))
    ratio = np.abs(F - mu[None, :]) / (2.0 * tol)
    print("max |f - mu| / budget %.3f" % ratio.max())
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("mode", ["inverse", "solve"])
@pytest.mark.parametrize("n, d", [(130, 2), (600, 8)])
def test_training_point_identity_with_the_device_solves(n, d, mode):
    """f_s(X) = y - eps_s - diag_add v_s: the residual of K v = rhs, which backward-stable solves against the computed
    factor keep below c n u (|L| |L^T| |v|): factor_ref's Cholesky bound (n + 1 + C_CHOL) and one (n + C_TRSV) per
    triangular solve, c n = 3 n + 1 + C_CHOL + 2 C_TRSV; plus the evaluation's own budget."""
    gp, X, y, k = _gp_fixture(n, d, 5 * n + d, diag_rel=1e-4)
    gp.variance_mode = mode
    rs = np.random.RandomState(2)
    R, S = 200, 4
    Z, b = rs.standard_normal((R, d)), rs.uniform(0, 2 * np.pi, R)
    W, Wl = rs.standard_normal((S, R)), np.zeros((S, d))
    eps = np.sqrt(k.diag_add) * rs.standard_normal((S, n))
    paths = gp._paths_from(y, Z, b, W, Wl, eps)
    F = paths.evaluate(X)
    V = paths.V.cpu().numpy()
    L = np.tril(gp._L[:n, :n].cpu().numpy())
    want = y[None, :] - eps - k.diag_add * V.T
    back = (3 * n + 1 + fref.C_CHOL + 2 * fref.C_TRSV) * pr.U * (np.abs(L) @ (np.abs(L.T) @ np.abs(V))).T
    bud, _ = pr.budget(X, X, V, Z, b, W, Wl, k, gp.mean.value)
    ratio = np.abs(F - want) / (back + 2.0 * bud)          # (g_s(X) is evaluated twice: in the right-hand side and in f)
    print("max residual / budget %.3f" % ratio.max())
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("seed", [0, 3])
def test_moments_of_many_draws_on_the_device(seed):
    """The moment test of tests/test_pathdraw_ref.py with the device evaluating g_s(X) and f_s(T): same seeds, same caps."""
    fx = pr.moment_fixture(seed)
    k, y, mean, X, T, Z, b = fx["k"], fx["y"], fx["mean"], fx["X"], fx["T"], fx["Z"], fx["b"]
    rs = np.random.RandomState(1000 + seed)
    F = []
    for _ in range(4096 // 32):
        W = rs.standard_normal((32, fx["phiT"].shape[1]))
        eps = np.sqrt(k.diag_add) * rs.standard_normal((32, len(y)))
        Wf, Wl = np.ascontiguousarray(W[:, :len(Z)]), np.ascontiguousarray(W[:, len(Z):])
        gX = dev_path_draws(X, None, None, Z, b, Wf, Wl, k, 0.0)[0]
        V = fx["solve"]((y - mean)[:, None] - gX.T - eps.T)
        F.append(dev_path_draws(T, X, V, Z, b, Wf, Wl, k, mean)[0])
    F = np.vstack(F)
    mu = mean + fx["Kxt"].T @ fx["solve"](y - mean)
    vhat = pr.surrogate_variance(fx["phiT"], fx["phiX"], fx["Kxt"], fx["solve"], k.diag_add)
    zm, zv = pr.moment_scores(F, mu, vhat)
    print("max |z| mean %.2f variance %.2f" % (np.abs(zm).max(), np.abs(zv).max()))
    assert np.abs(zm).max() <= 5.0 and np.abs(zv).max() <= 5.0


def test_paths_refuse_a_changed_factor_and_check_their_arguments():
    gp, X, y, _ = _gp_fixture(50, 2, 8)
    with pytest.raises(ValueError):
        gp.sample_paths(y, 0)
    with pytest.raises(ValueError):
        gp.sample_paths(y, 33)
    with pytest.raises(ValueError):
        gp.sample_paths(y, 2, nFeatures=0)
    with pytest.raises(ValueError):
        gp.thompson_batch(y, X, 33)
    paths = gp.sample_paths(y, 2, nFeatures=64)
    assert paths.evaluate(X[:5]).shape == (2, 5) and paths.evaluate(np.empty((0, 2))).shape == (2, 0)
    assert paths.argmax(np.empty((0, 2)))[0].tolist() == [-1, -1]
    p = gp.get_parameter_vector()
    gp.set_parameter_vector(p + 0.1)
    gp.recompute()
    with pytest.raises(RuntimeError):
        paths.evaluate(X[:5])


def test_thompson_batch():
    gp, X, y, _ = _gp_fixture(130, 2, 21)
    rs = np.random.RandomState(4)
    T = rs.uniform(-5.5, 5.5, size=(3000, 2))
    bounds = [(-5.0, 5.0)] * 2
    mask = rs.rand(len(T)) > 0.1
    q = 6
    np.random.seed(11)
    idx, draws = gp.thompson_batch(y, T, q, bounds=bounds, mask=mask, idx_offset=50, nFeatures=512, return_draws=True)
    assert idx.dtype == np.int64 and len(idx) == q and np.all(idx >= 50)
    assert len(set(idx.tolist())) == q
    adm = pr.admissible(T, bounds, mask)
    assert adm[idx - 50].all()
    # replay the rounds from the same seed: every index is the arg-max of its own draw, recomputed from evaluate()
    np.random.seed(11)
    chosen = []
    for rnd in range(max(r for r, _ in draws) + 1):
        paths = gp.sample_paths(y, min(32, 2 * (q - len(chosen))), 512)
        F = paths.evaluate(T)
        for j, (r, s) in enumerate(draws):
            if r == rnd:
                assert idx[j] == pr.argmin(F[s], adm, 50)[0], (j, r, s)
                chosen.append(idx[j])
        win, val = paths.argmax(T, bounds=bounds, mask=mask, idx_offset=50)
        assert [pr.argmin(F[s], adm, 50)[0] for s in range(paths.size)] == win.tolist()
        assert np.array_equal(val, F[np.arange(paths.size), win - 50])
    assert draws == sorted(draws) and len(chosen) == q
    # q = 1: the arg-max of the first draw; device candidates take the tensor path
    np.random.seed(12)
    one = gp.thompson_batch(y, T, 1, bounds=bounds, mask=mask, nFeatures=512)
    np.random.seed(12)
    first = gp.sample_paths(y, 2, 512).argmax(T, bounds=bounds, mask=mask)[0][0]
    assert one.tolist() == [first]
    np.random.seed(12)
    assert gp.thompson_batch(y, gp._candidates(T), 1, bounds=bounds, mask=mask, nFeatures=512).tolist() == [first]
    # nothing admissible: -1 in every slot, and the GP is untouched
    key = gp._factor_key()
    assert gp.thompson_batch(y, T, 3, mask=np.zeros(len(T), dtype=bool), nFeatures=64).tolist() == [-1, -1, -1]
    assert gp._factor_key() == key and gp.computed


def test_sample_conditional_is_multivariate_normal_of_predict():
    gp, X, y, _ = _gp_fixture(50, 2, 13)
    T = np.random.RandomState(0).uniform(-5, 5, size=(7, 2))
    mu, cov = gp.predict(y, T, return_cov=True)
    for size in (1, 4):
        np.random.seed(5)
        got = gp.sample_conditional(y, T, size=size)
        np.random.seed(5)
        want = np.random.multivariate_normal(mu, cov, size)
        assert np.array_equal(got, want[0] if size == 1 else want)


def _rosen_ap(m0, seed, algorithm="bape"):
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    np.random.seed(seed)
    theta = np.array(lh.rosenbrockSample(m0))
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y)
    return approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                  priorSample=lh.rosenbrockSample, bounds=[(-5, 5), (-5, 5)], algorithm=algorithm)


def test_find_next_point_and_bayes_opt_with_thompson_batches(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _rosen_ap(30, 5)
    pool = concurrent.futures.ThreadPoolExecutor(2)
    with np.errstate(all="ignore"):
        theta, val = ap.findNextPoint(nCandidates=2000, numNewPoints=4, batchSize=4, batchMethod="thompson",
                                      computeLnLike=True, pool=pool, seed=5, verbose=False)
    assert theta.shape == (4, 2) and len(set(map(tuple, theta))) == 4
    assert np.all(np.abs(theta) <= 5.0)
    assert len(ap.y) == 34 and len(ap.theta) == 34 and len(ap.gp._x) == 34
    ap = _rosen_ap(30, 6, algorithm="jones")
    start = float(np.max(ap.y))
    with np.errstate(all="ignore"):
        soln = ap.bayesOpt(nmax=3, batchSize=4, nCandidates=2000, batchMethod="thompson", pool=pool, findMAP=False,
                           kmax=5, seed=6, verbose=False, cache=False)
    pool.shutdown()
    assert soln["nev"] == 12 and len(ap.y) == 42
    assert soln["valBest"] >= start


def test_believer_batches_are_acquire_batch_as_before(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from approxposterior_amd import likelihood as lh
    ap = _rosen_ap(30, 7)
    np.random.seed(3)
    cands = np.asarray(lh.rosenbrockSample(2000), dtype=float).reshape(2000, -1)
    want, _ = ap.gp.acquire_batch(ap.y, cands, ["bape"] * 4, 4, bounds=ap.bounds)
    for kw in (dict(), dict(batchMethod="believer")):
        np.random.seed(3)
        got = ap.findNextPoint(nCandidates=2000, numNewPoints=4, batchSize=4, computeLnLike=False, verbose=False, **kw)
        assert np.array_equal(got, cands[want])
