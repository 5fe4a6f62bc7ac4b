# -*- coding: utf-8 -*-
"""MI355X: the kernel value k(x, x') itself, at every entry point of the C ABI that hands one out -- apgp_gram,
apgp_kernel_cross and, as a probe of k*, apgp_predict_mean / apgp_predict_mean_host on a training set whose alpha is a
unit vector (mu_i = k(t_i, x_0): the other rows add exact zeros) -- against tests/kvalue_ref.py:

  * every value within ``budget`` (derived from rounding counts, not fitted) of the exact value;
  * on the dyadic lattice within 2.1 ulp;
  * the same BITS as ``restate`` (the device arithmetic restated with an exactly rounded fma) wherever that is owed:
    everywhere for the Gram and cross kernels, for the pure squared-exponential kernel in the mean kernel;
  * the promise of apgp_common.h: Gram, cross and k* agree to the bit for the squared-exponential kernel (with a
    linear term: Gram and cross do, the mean kernel's agreement is reported per order);
  * sentinels above the diagonal and in the row padding come back byte-identical;
  * what a NaN / +inf / -inf coordinate does at each entry point, and that GP.compute refuses it as the oracle does.

Worst figures are printed (pytest -s) and recorded in docs/experiments.md."""
import ctypes

import numpy as np
import pytest

import kvalue_ref as kr

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300
FLOOR = kr.exp_restate(-700.0)          # what the clamp turns exp(-inf) and exp(NaN) into


@pytest.fixture(scope="module")
def lib_loaded():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_abi_version() == _lib.ABI_VERSION
    return lib


def _ks(k):
    from approxposterior_amd import _lib
    ks = _lib.KernelStruct()
    ks.ndim, ks.lin_order, ks.amp, ks.diag_add, ks.lin_coef = k.ndim, k.lin_order, k.amp, k.diag_add, k.lin_coef
    ks.inv_metric[:k.ndim] = k.inv_metric.tolist()
    return ks


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.apgp_last_error())


def dev_gram(lib, X, k, ldk):
    """(K as an n x ldk array pre-filled with the sentinel)."""
    import torch
    n = len(X)
    K = torch.full((n, ldk), SENTINEL, dtype=torch.float64, device="cuda:0")
    Xd = _dev(X)
    _ok(lib, lib.apgp_gram(Xd.data_ptr(), n, ctypes.byref(_ks(k)), K.data_ptr(), ldk, None), "apgp_gram")
    torch.cuda.synchronize()
    return K.cpu().numpy()


def dev_cross(lib, X1, X2, k, ldc):
    import torch
    m, n = len(X1), len(X2)
    C = torch.full((m, ldc), SENTINEL, dtype=torch.float64, device="cuda:0")
    a, b = _dev(X1), _dev(X2)
    _ok(lib, lib.apgp_kernel_cross(a.data_ptr(), m, b.data_ptr(), n, ctypes.byref(_ks(k)), C.data_ptr(), ldc, None),
        "apgp_kernel_cross")
    torch.cuda.synchronize()
    return C.cpu().numpy()


def dev_mean(lib, T, X, alpha, k, mean=0.0, host=False):
    """mu (m,) of apgp_predict_mean[_host] on the training set X packed with ``alpha``."""
    import torch
    n, m, D = len(X), len(T), k.ndim
    ks = _ks(k)
    xs = torch.empty(lib.apgp_packed_train_len(n, D), dtype=torch.float64, device="cuda:0")
    Xd, ad = _dev(X), _dev(alpha)
    _ok(lib, lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs.data_ptr(), None), "apgp_pack_train")
    if host:
        Th = np.ascontiguousarray(T, dtype=np.float64)
        mu = np.full(m, SENTINEL)
        work = torch.empty(m * D + m, dtype=torch.float64, device="cuda:0")
        _ok(lib, lib.apgp_predict_mean_host(Th.ctypes.data, m, xs.data_ptr(), n, ctypes.byref(ks), mean, mu.ctypes.data,
                                            work.data_ptr(), None), "apgp_predict_mean_host")
        torch.cuda.synchronize()
        return mu
    Td = _dev(T)
    mu = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda:0")
    _ok(lib, lib.apgp_predict_mean(Td.data_ptr(), m, xs.data_ptr(), n, ctypes.byref(ks), mean, mu.data_ptr(), None),
        "apgp_predict_mean")
    torch.cuda.synchronize()
    return mu.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def sample_pairs(m, n, gram, cap=5000, seed=0):
    idx = [(i, j) for i in range(m) for j in range(i + 1 if gram else n)]
    if len(idx) <= cap:
        return idx
    rs = np.random.RandomState(seed)
    keep = set(rs.choice(len(idx), size=cap, replace=False).tolist()) | {0, len(idx) - 1}
    return [idx[t] for t in sorted(keep)]


def assert_bits_of_restate(V, X1, X2, k, site, pairs=None):
    R = kr.restate(X1, X2, k, site=site, pairs=pairs)
    sel = ~np.isnan(R)
    bad = sel & (np.where(sel, V, 0.0).view(np.int64) != np.where(sel, R, 0.0).view(np.int64))
    assert not bad.any(), ("%d of %d entries differ from the restatement, first at %r: device %r, restated %r"
                           % (bad.sum(), sel.sum(), tuple(np.argwhere(bad)[0]), V[bad][0], R[bad][0]))


# every n of {1, 63, 64, 65, 129, 200} and every D of {1, 2, 3, 4, 5, 8, 9, 16, 17, 32} (each dpad class and each odd D
# below a class boundary), every class at a partial and at more than one tile
ND = [(1, 1), (1, 3), (1, 32), (63, 2), (63, 5), (63, 17), (64, 1), (64, 4), (64, 9), (64, 32), (65, 2), (65, 3), (65, 8),
      (65, 16), (65, 17), (129, 1), (129, 4), (129, 5), (129, 16), (200, 3), (200, 8), (200, 9), (200, 32)]
LINEAR = [(0, 65, 3), (1, 65, 3), (2, 65, 3), (3, 65, 3), (16, 65, 3), (2, 64, 17), (3, 63, 1), (16, 65, 32), (1, 129, 8)]


def make(family, n, D, order=None):
    if family == "general":
        return kr.general(n, D, seed=n + D)
    if family == "lattice":
        return kr.lattice_nd(n, D, seed=n + D, amp=2.0 ** ((n + D) % 5 - 2), diag_add=2.0 ** -10)
    if family == "coincident":
        return kr.coincident(n, D, seed=n + D)
    return kr.linear(n, D, order, seed=n + D)


def check_gram(lib, X, k, family):
    n = len(X)
    B = kr.budget(X, None, k)
    T = kr.truth_ld(X, None, k)
    low = np.tril(np.ones((n, n), dtype=bool))
    worst = None
    for ldk in (n, n + 3):
        K = dev_gram(lib, X, k, ldk)
        assert same_bits(K[:, :n][~low], np.full((~low).sum(), SENTINEL)), "written above the diagonal"
        assert same_bits(K[:, n:], np.full((n, ldk - n), SENTINEL)), "written into the row padding"
        V = K[:, :n].copy()
        assert np.all(np.isfinite(V[low]))
        err = np.abs(V.astype(np.longdouble) - T).astype(np.float64)
        ratio = (err[low] / B[low]).max()
        live = low & (T.astype(np.float64) > k.amp * 1e-304)
        ulps = (err[live] / kr.ulp(T.astype(np.float64))[live]).max()
        print("gram %-10s n=%-4d D=%-2d ldk=%-4d worst |err| / budget %.3f, %.3f ulp" % (family, n, k.ndim, ldk, ratio, ulps))
        assert ratio <= 1.0
        if family == "lattice":
            assert (B[live] / kr.ulp(T.astype(np.float64))[live]).max() <= 2.1 and ulps <= 2.1
        if worst is None:
            worst = V
        else:
            assert same_bits(np.where(low, V, 0.0), np.where(low, worst, 0.0)), "the leading dimension changed a value"
    i = np.arange(n)
    if family in ("general", "lattice", "coincident"):
        assert same_bits(worst[i, i], np.full(n, k.amp + k.diag_add))      # x' = x: amp + diag_add exactly
    if n <= 65:
        assert_bits_of_restate(worst, X, None, k, "gram")
    return worst


@pytest.mark.parametrize("n,D", ND)
@pytest.mark.parametrize("family", ["general", "lattice"])
def test_gram_values(lib_loaded, family, n, D):
    X, k = make(family, n, D)
    check_gram(lib_loaded, X, k, family)


@pytest.mark.parametrize("order,n,D", LINEAR)
def test_gram_values_linear_term(lib_loaded, order, n, D):
    X, k = make("linear", n, D, order)
    check_gram(lib_loaded, X, k, "linear-P%d" % order)


def test_gram_values_coincident(lib_loaded):
    X, k = make("coincident", 65, 3)
    check_gram(lib_loaded, X, k, "coincident")


def test_gram_lattice_1d_257(lib_loaded):
    """32 896 distinct exact arguments, each value within 2.1 ulp; a seeded 5000 of them also bit for bit."""
    X, k = kr.lattice_1d()
    V = check_gram(lib_loaded, X, k, "lattice")
    assert_bits_of_restate(V, X, None, k, "gram", pairs=sample_pairs(257, 257, True))


def test_gram_2100_tile_decode(lib_loaded):
    """33 block rows, 561 tiles: the sqrt-based tile decode.  Every entry of the lower triangle against plain fp64
    NumPy (a misplaced tile is an error of order one), the first and last row of every block row against the
    long-double truth within the budget."""
    n, D = 2100, 3
    X, k = kr.general(n, D, seed=2100, diag_add=0.0, width=4.0)
    K = dev_gram(lib_loaded, X, k, n)
    low = np.tril(np.ones((n, n), dtype=bool))
    assert same_bits(K[~low], np.full((~low).sum(), SENTINEL))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 * k.inv_metric).sum(-1)
    plain = k.amp * np.exp(-0.5 * d2)
    assert np.abs(K - plain)[low].max() <= 1e-12 * k.amp
    rows = sorted(set([r for b in range(33) for r in (64 * b, min(64 * b + 63, n - 1))]))
    B = kr.budget(X[rows], X, k)
    T = kr.truth_ld(X[rows], X, k)
    sel = np.arange(n)[None, :] <= np.array(rows)[:, None]
    err = np.abs(K[rows].astype(np.longdouble) - T).astype(np.float64)
    ratio = (err[sel] / B[sel]).max()
    print("gram general    n=2100 D=3: worst |err| / budget %.3f over %d entries" % (ratio, sel.sum()))
    assert ratio <= 1.0


CROSS = [(1, 1, 1), (1, 63, 3), (1, 257, 8), (5, 1, 2), (5, 63, 17), (5, 257, 5), (64, 1, 32), (64, 63, 4), (64, 257, 9)]


def check_cross(lib, X1, X2, k, family):
    m, n = len(X1), len(X2)
    C = dev_cross(lib, X1, X2, k, n + 2)
    assert same_bits(C[:, n:], np.full((m, 2), SENTINEL)), "written into the row padding"
    V = C[:, :n].copy()
    assert np.all(np.isfinite(V))
    ratio, ulps = kr.err_over_budget(V, X1, X2, k)
    print("cross %-10s m=%-3d n=%-4d D=%-2d worst |err| / budget %.3f, %.3f ulp" % (family, m, n, k.ndim, ratio, ulps))
    assert ratio <= 1.0
    if family == "lattice":
        assert ulps <= 2.1
    assert_bits_of_restate(V, X1, X2, k, "cross", pairs=sample_pairs(m, n, False))
    return V


@pytest.mark.parametrize("m,n,D", CROSS)
@pytest.mark.parametrize("family", ["general", "lattice", "linear"])
def test_cross_values(lib_loaded, family, m, n, D):
    X, k = make(family, m + n, D, order=(0, 1, 2, 3, 16)[(m + n + D) % 5])
    check_cross(lib_loaded, X[:m], X[m:], k, family)


def test_cross_lattice_edges(lib_loaded):
    """Arguments on either side of the reduction boundaries (k + 1/2) ln2/32 over the whole range, 0, either side of
    the clamp at 700 and 1e6 -- all exact: within 2.1 ulp, and the restatement's bits."""
    E = kr.lattice_edges_points()
    k = kr.kern([2.0])
    V = check_cross(lib_loaded, E, np.zeros((1, 1)), k, "lattice")
    assert V[0, 0] == 1.0 and V[-1, 0] == FLOOR                 # s = 0 and s = 1e6
    assert 0.0 < FLOOR < 1e-304


PROBE = [(1, 0), (130, 70)]             # (training points, the one whose alpha is 1): the second crosses a 64-lane stride


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("n,row", PROBE)
@pytest.mark.parametrize("family,D", [("general", 1), ("general", 3), ("general", 8), ("general", 17), ("general", 32),
                                      ("lattice", 2), ("lattice", 5), ("lattice", 9), ("linear", 3), ("linear", 16)])
def test_kstar_probe(lib_loaded, family, D, n, row, host):
    m = 41
    X, k = make(family, n + m, D, order=2 + (D & 1))
    T, X = X[:m].copy(), X[m:]
    T[m - 1] = X[row]                   # a candidate on the training point
    alpha = np.zeros(n)
    alpha[row] = 1.0
    mu = dev_mean(lib_loaded, T, X, alpha, k, host=host)
    V = mu[:, None]
    ratio, ulps = kr.err_over_budget(V, T, X[row:row + 1], k)
    print("k* %-8s D=%-2d n=%-3d host=%d worst |err| / budget %.3f, %.3f ulp" % (family, D, n, host, ratio, ulps))
    assert ratio <= 1.0
    if family == "lattice":
        assert ulps <= 2.1
    if family != "linear":
        assert_bits_of_restate(V, T, X[row:row + 1], k, "mean")
        assert mu[m - 1] == k.amp


def _promise(lib, X, k):
    """(cross == gram everywhere, k* == gram everywhere) for the rows 0, 17, 63, 64 of a 65-point set."""
    n = len(X)
    K = dev_gram(lib, X, k, n)
    K = np.where(np.tril(np.ones((n, n), dtype=bool)), K, K.T)
    j = np.arange(n)
    # (the diagonal carries diag_add: compared apart)
    cross_ok = mean_ok = True
    for i in (0, 17, 63, 64):
        off = j != i
        C = dev_cross(lib, X[i:i + 1], X, k, n)[0]
        alpha = np.zeros(n)
        alpha[i] = 1.0
        mu = dev_mean(lib, X, X, alpha, k)          # mu_j = k(x_j, x_i)
        cross_ok &= same_bits(C[off], K[i][off]) and C[i] + k.diag_add == K[i, i]
        mean_ok &= same_bits(mu[off], K[i][off]) and mu[i] + k.diag_add == K[i, i]
    return cross_ok, mean_ok


@pytest.mark.parametrize("family,D", [("general", 3), ("general", 17), ("general", 32), ("lattice", 5), ("coincident", 2)])
def test_promise_gram_cross_kstar_same_bits(lib_loaded, family, D):
    """A candidate that sits on a training point sees the row the factor was built from."""
    X, k = make(family, 65, D)
    cross_ok, mean_ok = _promise(lib_loaded, X, k)
    assert cross_ok and mean_ok


def test_promise_with_linear_term(lib_loaded):
    """Gram and cross share apgp_gram_value: the same bits at every order.  The mean kernel is compiled with contraction
    allowed: whether its k* has the Gram kernel's bits is reported per order, and the budget is what is asserted
    (test_kstar_probe)."""
    for order in kr.LIN_ORDERS:
        for D in (3, 17):
            X, k = make("linear", 65, D, order)
            cross_ok, mean_ok = _promise(lib_loaded, X, k)
            print("linear term, order %-2d D=%-2d: cross == gram %s, k* == gram %s" % (order, D, cross_ok, mean_ok))
            assert cross_ok


# ----------------------------------------------------------------------------------------------------------------------
# non-finite coordinates
# ----------------------------------------------------------------------------------------------------------------------
BAD = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)]


@pytest.mark.parametrize("name,bad", BAD)
def test_nonfinite_training_coordinate_gram_and_cross(lib_loaded, name, bad):
    """The documented domain of apgp_gram / apgp_kernel_cross is finite coordinates.  What a non-finite one does is
    pinned here so that it cannot change unnoticed: the clamp of apgp_exp maps the NaN / -inf argument to -700, every
    entry of the point's row and column -- its diagonal included (inf - inf = NaN) -- is amp exp(-700) ~ amp 1e-304
    [+ diag_add], finite, and every other entry keeps its bits.  (george: NaN there; GP.compute refuses such an X.)"""
    X, k = kr.general(65, 3, seed=7)
    clean = dev_gram(lib_loaded, X, k, 65)
    Xb = X.copy()
    Xb[40, 1] = bad
    K = dev_gram(lib_loaded, Xb, k, 65)
    want = clean.copy()
    want[40, :40] = k.amp * FLOOR
    want[41:, 40] = k.amp * FLOOR
    want[40, 40] = k.amp * FLOOR + k.diag_add
    assert same_bits(K, want)
    cclean = dev_cross(lib_loaded, X[:5], X[5:], k, 60)
    Xb = X.copy()
    Xb[2, 0] = bad                       # in X1
    C = dev_cross(lib_loaded, Xb[:5], Xb[5:], k, 60)
    want = cclean.copy()
    want[2, :] = k.amp * FLOOR
    assert same_bits(C, want)
    Xb = X.copy()
    Xb[5 + 33, 2] = bad                  # in X2
    C = dev_cross(lib_loaded, Xb[:5], Xb[5:], k, 60)
    want = cclean.copy()
    want[:, 33] = k.amp * FLOOR
    assert same_bits(C, want)


@pytest.mark.parametrize("name,bad", BAD)
def test_nonfinite_training_coordinate_is_refused_as_the_oracle_does(lib_loaded, name, bad):
    """GP.compute, and its factor-extension path, raise what the oracle raises; the model stays as it was."""
    import george_oracle as go
    from approxposterior_amd import gp as agp
    X, _ = kr.general(66, 3, seed=8)
    Xb = X.copy()
    Xb[65, 1] = bad

    def model(mod):
        return mod.GP(kernel=mod.ExpSquaredKernel(np.full(3, 0.7), ndim=3), fit_mean=True, mean=0.3, white_noise=-10.0,
                      fit_white_noise=False)
    with pytest.raises(Exception) as oracle_says:
        model(go).compute(Xb)
    kind = oracle_says.type
    assert kind is ValueError
    with pytest.raises(kind):
        model(agp).compute(Xb)
    prev = model(agp)
    prev.compute(X[:65])
    nxt = model(agp)
    with pytest.raises(kind):
        nxt.compute(Xb, previous=prev)               # (the extension: one appended row)
    assert not nxt.computed
    Xb = X.copy()
    Xb[0, 0] = bad
    with pytest.raises(kind):
        model(agp).compute(Xb[:1])                   # a single point
    ok = model(agp)
    ok.compute(X, previous=prev)
    assert ok.computed


@pytest.mark.parametrize("host", [False, True])
def test_nonfinite_candidate_mean(lib_loaded, host):
    """predict_mean: a NaN candidate gives NaN; an infinite one is infinitely far from every training point, exp(-inf) =
    0 and mu = mean, within the floor the clamp leaves (sum |alpha| amp 1e-304); the rows beside them keep their bits."""
    X, k = kr.general(130, 3, seed=9)
    rs = np.random.RandomState(9)
    alpha = rs.normal(size=130)
    T = X[:8] + 0.01
    clean = dev_mean(lib_loaded, T, X, alpha, k, mean=0.7, host=host)
    Tb = T.copy()
    Tb[1, 2], Tb[3, 0], Tb[6, 1] = np.nan, np.inf, -np.inf
    mu = dev_mean(lib_loaded, Tb, X, alpha, k, mean=0.7, host=host)
    assert np.isnan(mu[1])
    floor = np.abs(alpha).sum() * k.amp * 1e-304
    assert abs(mu[3] - 0.7) <= floor and abs(mu[6] - 0.7) <= floor
    keep = [0, 2, 4, 5, 7]
    assert same_bits(mu[keep], clean[keep])
