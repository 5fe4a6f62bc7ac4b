# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): the evidence over posterior function draws (apgp_path_importance, GP.importance_paths,
ApproxPosterior.evidence(surrogateDraws=); DESIGN.md "Evidence over path draws").  The log-weights against
apgp_path_draws' own F bit for bit and against the long-double truth within tests/pathdraw_ref.py's budget, the records
against the restatement of the device's own log-weights within tests/evidence_ref.py's budget, the gate, the plug-in
column against apgp_importance_pass, determinism, the moments' tile loop, the identity mean_s Z_s = Z[exp(mu + v / 2)]
with the device evaluating, and evidence() end to end.  Every C-ABI case runs with the vector contraction and, where
that kernel exists (more than one draw, D <= 8), with the matrix-core one."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import pathdraw_ref as pr  # noqa: E402
import pathevidence_ref as per  # noqa: E402
import test_gpu_evidence as tge  # noqa: E402
import test_gpu_importance as tgi  # noqa: E402
import test_gpu_path_draws as tpd  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = tpd.SENTINEL
U = pr.U


@pytest.fixture(params=["vector", "matrix"])
def form(request):
    """Both contractions (apgp_path_draws_mode, which apgp_path_importance honours): 1 the vector units for every shape,
    2 the matrix cores wherever that kernel exists and the vector units elsewhere."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    was = lib.apgp_path_draws_mode({"vector": 1, "matrix": 2}[request.param])
    yield request.param
    lib.apgp_path_draws_mode(was)


def dev_path_importance(T, X, V, Z, b, W, Wl, k, mean, lnq=None, bounds=None, centre=None, with_logw=True):
    """apgp_path_importance through the C ABI: (logw (S, M) pre-filled with a sentinel or None, record dicts (S))."""
    import torch
    from approxposterior_amd import _lib
    from approxposterior_amd import gp as agp
    lib = _lib.load()
    ks = tpd._ks(k)
    m, S, R, n = len(T), len(W), len(Z), len(X)
    _dev = tpd._dev
    xs_d = torch.empty(lib.apgp_packed_train_len(n, k.ndim), dtype=torch.float64, device="cuda:0")
    Xd, ad = _dev(X), _dev(np.full(n, np.nan))              # (the alpha column is not read)
    assert lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs_d.data_ptr(), None) == 0
    Td, Zd, bd, Wd = _dev(T), _dev(Z), _dev(b), _dev(W)
    Wld = _dev(Wl) if Wl is not None else None
    Vd = _dev(V) if V is not None else None
    qd = _dev(lnq) if lnq is not None else None
    c = np.zeros(k.ndim) if centre is None else np.asarray(centre, dtype=np.float64)
    cc = (ctypes.c_double * _lib.MAX_DIM)(*c)
    logw = torch.full((S, m), SENTINEL, dtype=torch.float64, device="cuda:0") if with_logw else None
    nstat = lib.apgp_importance_stats_len(k.ndim)
    stats = torch.full((S, nstat), SENTINEL, dtype=torch.float64, device="cuda:0")
    need = lib.apgp_path_importance_work_len(m, S)
    assert need == per.work_len(m, S)
    work = torch.full((need - (S * m if with_logw else 0),), SENTINEL, dtype=torch.float64, device="cuda:0")
    lo, hi = tpd._box(bounds)
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    rc = lib.apgp_path_importance(Td.data_ptr(), m, ptr(qd), xs_d.data_ptr(), n, ctypes.byref(ks), mean, ptr(Vd),
                                  Zd.data_ptr(), bd.data_ptr(), Wd.data_ptr(), ptr(Wld), R, S, lo, hi,
                                  ctypes.addressof(cc), ptr(logw), stats.data_ptr(), work.data_ptr(), None)
    assert rc == 0, lib.apgp_last_error()
    torch.cuda.synchronize()
    r = stats.cpu().numpy()
    return (logw.cpu().numpy() if with_logw else None), [agp.GP._importance_record(r[s], c) for s in range(S)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _stat_bits(recs):
    return b"".join(_bits([r["lmax"], r["S0"], r["S2"], r["cnt"]]) + _bits(r["s1"]) + _bits(r["S"]) for r in recs)


# (n, m, R, S, D, linear order): a single row and feature; sizes one off the 64-row tiles and the 256-row workgroups; the
# one-draw kernel, the 8-, 16- and 32-column kernels and both column-block counts of the matrix form; D on both sides of
# the matrix form's limit of 8
SHAPES = [
    (1, 1, 1, 1, 1, None),
    (63, 257, 64, 3, 2, None),
    (64, 700, 100, 8, 3, 1),
    (65, 256, 65, 9, 8, None),
    (130, 700, 128, 16, 8, 2),
    (130, 300, 64, 17, 9, None),
    (64, 257, 64, 32, 32, None),
]
BOX = 2.1                   # the rows are uniform in [-2.2, 2.2]^D: some fall outside


@functools.lru_cache(maxsize=None)
def _problem(n, m, R, S, D, P):
    c = pr.case(n, m, R, S, D, order=P, seed=3 * n + m + R + S + D)
    lnq = np.random.RandomState(n + m).normal(size=m) - 1.0
    centre = c["X"][0].copy()
    return c, lnq, [(-BOX, BOX)] * D, centre


def _args(c, P, with_v=True):
    return (c["T"], c["X"], c["V"] if with_v else None, c["Z"], c["b"], c["W"], c["Wl"] if P is not None else None,
            c["k"], c["mean"])


def _expect_from_f(F, T, lnq, bounds):
    """What the pass must store given apgp_path_draws' F for the same inputs: F - lnq in one rounded subtraction on the
    admissible rows, -inf elsewhere."""
    want = per.logw(F, T, lnq, bounds)
    assert want.dtype == np.float64
    return want


@pytest.mark.parametrize("n, m, R, S, D, P", SHAPES)
def test_logw_is_path_draws_f_minus_lnq_bit_for_bit(n, m, R, S, D, P, form):
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    a = _args(c, P)
    F = tpd.dev_path_draws(*a)[0]
    assert np.all(np.isfinite(F))
    lw, recs = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    want = _expect_from_f(F, c["T"], lnq, bounds)
    adm = per.gate(c["T"], lnq, bounds)
    print("%d of %d rows admissible" % (adm.sum(), m))
    assert np.all(np.isneginf(lw[:, ~adm]))
    assert _bits(lw) == _bits(want)
    for s in range(S):
        assert recs[s]["lmax"] == want[s].max() and recs[s]["cnt"] == float(adm.sum())
    # no ln q, no box: F itself; and the records do not need logw_out
    lw0, recs0 = dev_path_importance(*a, centre=centre)
    assert _bits(lw0) == _bits(F)
    _, recs1 = dev_path_importance(*a, centre=centre, with_logw=False)
    assert _stat_bits(recs0) == _stat_bits(recs1)


def test_prior_draws_alone_with_a_null_v(form):
    n, m, R, S, D, P = SHAPES[1]
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    a = _args(c, P, with_v=False)
    F = tpd.dev_path_draws(c["T"], None, None, *a[3:])[0]
    lw, recs = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    assert _bits(lw) == _bits(_expect_from_f(F, c["T"], lnq, bounds))
    for s in range(S):
        tgi._check_record(recs[s], lw[s], c["T"], centre)


@functools.lru_cache(maxsize=None)
def _truth(n, m, R, S, D, P):
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    a = _args(c, P)
    F = pr.draws(*a)
    bud, mag = pr.budget(*a)
    for x in (F, bud):
        x.setflags(write=False)
    return F, bud


@pytest.mark.parametrize("n, m, R, S, D, P", [SHAPES[3], SHAPES[2]])
def test_logw_within_the_budget_and_records_restated(n, m, R, S, D, P, form):
    """|logw - truth| <= pathdraw_ref.budget + u (|f| + |ln q|): the draw's own budget and the one rounded subtraction
    (u |f - ln q| <= u (|f| + |ln q|)).  The records: the restatement of the DEVICE's log-weights -- lmax and cnt exact,
    the sums within evidence_ref.record_budget."""
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    F, bud = _truth(n, m, R, S, D, P)
    lw, recs = dev_path_importance(*_args(c, P), lnq=lnq, bounds=bounds, centre=centre)
    adm = per.gate(c["T"], lnq, bounds)
    truth = F[:, adm].astype(np.longdouble) - lnq[adm].astype(np.longdouble)
    tol = bud[:, adm] + U * (np.abs(F[:, adm]) + np.abs(lnq[adm]))
    ratio = np.abs(lw[:, adm].astype(np.longdouble) - truth).astype(np.float64) / tol
    print("max |logw - truth| / budget %.3f" % ratio.max())
    assert np.all(np.isneginf(lw[:, ~adm])) and ratio.max() <= 1.0
    worst = max(tgi._check_record(recs[s], lw[s], c["T"], centre) for s in range(S))
    print("max record error / budget %.3f" % worst)


def test_gate(form):
    n, m, R, S, D, P = SHAPES[2]
    assert m == 700
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    T, lnq = c["T"].copy(), lnq.copy()
    inside = np.flatnonzero(per.gate(T, lnq, bounds))
    rows = inside[[3, 40, 41, 42, 300, 301, 302, len(inside) - 1]]
    T[rows[0], 1] = BOX + 0.05             # outside the box
    T[rows[1], 0] = np.nan
    T[rows[2], 2] = np.inf
    T[rows[3], 1] = -np.inf
    lnq[rows[4]], lnq[rows[5]], lnq[rows[6]] = np.nan, np.inf, -np.inf
    T[rows[7], 0] = -BOX - 1e-9
    a = (T,) + _args(c, P)[1:]
    F = tpd.dev_path_draws(*a)[0]
    lw, recs = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    adm = per.gate(T, lnq, bounds)
    assert not adm[rows].any() and adm.sum() == len(inside) - len(rows)
    assert np.all(np.isneginf(lw[:, ~adm])) and _bits(lw[:, adm]) == _bits((F - lnq[None, :])[:, adm])
    for s in range(S):
        assert recs[s]["cnt"] == float(adm.sum())
        tgi._check_record(recs[s], lw[s], T, centre)
    # without a box only the non-finite rows are gated; an infinite coordinate never weighs
    lw2, _ = dev_path_importance(*a, lnq=lnq, centre=centre)
    adm2 = per.gate(T, lnq, None)
    assert adm2.sum() == m - 6 and np.all(np.isneginf(lw2[:, ~adm2])) and np.all(np.isfinite(lw2[:, adm2]))
    # every row gated for every draw: the empty record
    lw3, recs3 = dev_path_importance(*a, lnq=lnq, bounds=[(5.0, 6.0)] * D, centre=centre)
    assert np.all(np.isneginf(lw3))
    for r in recs3:
        assert r["lmax"] == -np.inf and r["S0"] == 0.0 and r["S2"] == 0.0 and r["cnt"] == 0.0
        assert not r["s1"].any() and not r["S"].any()
        assert _bits(r["s1"]) == _bits(np.zeros(D)) and _bits([r["S0"], r["S2"], r["cnt"]]) == _bits(np.zeros(3))


def test_weights_more_than_700_below_the_maximum_are_exactly_zero(form):
    """ln q raised by 1500 on the second half of the rows puts their log-weights 1500 below the others': e = 0 exactly,
    so S0, S2, s1 and S carry the bits of the call in which those rows are gated (ln q = +inf), while cnt still counts
    them -- adding an exact zero changes no partial sum."""
    n, m, R, S, D, P = SHAPES[2]
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    a = _args(c, P)
    far, gone = lnq.copy(), lnq.copy()
    far[m // 2:] += 1500.0
    gone[m // 2:] = np.inf
    lw_f, rec_f = dev_path_importance(*a, lnq=far, bounds=bounds, centre=centre)
    lw_g, rec_g = dev_path_importance(*a, lnq=gone, bounds=bounds, centre=centre)
    fin = np.isfinite(lw_f)
    assert fin[:, m // 2:].any() and np.all(np.isneginf(lw_g[:, m // 2:]))
    for s in range(S):
        top = lw_f[s].max()
        assert top == rec_f[s]["lmax"] == rec_g[s]["lmax"]
        assert np.all(lw_f[s, m // 2:][fin[s, m // 2:]] - top < -700.0)
        assert rec_f[s]["cnt"] == float(fin[s].sum()) > rec_g[s]["cnt"]
        for key in ("S0", "S2", "s1", "S"):
            assert np.array_equal(rec_f[s][key], rec_g[s][key]), (s, key)
        tgi._check_record(rec_f[s], lw_f[s], c["T"], centre)


@pytest.mark.parametrize("N, D", [(130, 8), (64, 2)])
def test_plug_in_column_agrees_with_importance_pass(N, D, form):
    """W = Wl = 0 and eps = 0 make every draw the predictive mean (V[:, s] = alpha exactly), so the pass must agree with
    apgp_importance_pass.  Both log-weights lie within their own budget of the same truth -- evidence_ref.logw_truth's
    for the mean pass, pathdraw_ref.budget + u (|f| + |ln q|) for this one -- hence within the sum D = bud_a + bud_b of
    each other.  Records: cnt equal; lmax within max D; with e = exp(logw - lmax), a shift of at most Dmax in every
    log-weight and in lmax changes each e by a factor within exp(+-2 Dmax), so S0 (and s1, S termwise) move by at most
    expm1(2 Dmax) relative to sum e |term| and S2 by expm1(4 Dmax), on top of the two record budgets."""
    g, X, y = tgi._gp(D, N)
    k = tgi._kern(g)
    alpha = tgi._alpha(g, y)
    T, lnq = tgi._rows(D, 300, 11 * D + N)
    bounds = [(-2.4, 2.4)] * D
    rs = np.random.RandomState(5)
    R, S = 64, 3
    Z, b = rs.standard_normal((R, D)), rs.uniform(0, 2 * np.pi, R)
    paths = g._paths_from(y, Z, b, np.zeros((S, R)), np.zeros((S, D)), np.zeros((S, N)))
    V = paths.V.cpu().numpy()
    assert np.array_equal(V, np.repeat(alpha[:, None], S, axis=1))
    rec_a, lw_a = g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True)
    recs, lw_b = g.importance_paths(y, T, paths, lnq=lnq, bounds=bounds, return_logw=True)
    lw_a, lw_b = lw_a.cpu().numpy(), lw_b.cpu().numpy()
    assert lw_b.shape == (S, len(T)) and len(recs) == S
    truth, bud_a = er.logw_truth(T, X, alpha, k, float(g.mean.value), lnq=lnq, bounds=bounds)
    fin = np.asarray(truth > -np.inf)
    bud_p, _ = pr.budget(T, X, V, Z, b, np.zeros((S, R)), np.zeros((S, D)), k, float(g.mean.value))
    f_abs = np.abs(truth.astype(np.float64) + np.where(fin, lnq, 0.0))
    c = X[int(np.argmax(y))]
    dx = np.abs(T[fin] - c)
    for s in range(S):
        tol = bud_a + bud_p[s] + U * (f_abs + np.abs(lnq))
        assert np.array_equal(np.isneginf(lw_b[s]), ~fin) and np.array_equal(np.isneginf(lw_a), ~fin)
        ratio = np.abs(lw_b[s][fin] - lw_a[fin]) / tol[fin]
        assert ratio.max() <= 1.0, ratio.max()
        dmax = float(tol[fin].max())
        r, w = recs[s], rec_a
        assert np.array_equal(r["centre"], w["centre"]) and r["cnt"] == w["cnt"]
        assert abs(r["lmax"] - w["lmax"]) <= dmax
        a0, a2, a1, aS = er.record_budget(lw_a, T, c)
        b0, b2, b1, bS = er.record_budget(lw_b[s], T, c)
        e = np.exp(lw_a[fin] - w["lmax"])
        assert abs(r["S0"] - w["S0"]) <= (a0 + b0 + np.expm1(2 * dmax)) * w["S0"]
        assert abs(r["S2"] - w["S2"]) <= (a2 + b2 + np.expm1(4 * dmax)) * w["S2"]
        assert np.all(np.abs(r["s1"] - w["s1"]) <= a1 + b1 + np.expm1(2 * dmax) * (e[:, None] * dx).sum(axis=0))
        assert np.all(np.abs(r["S"] - w["S"]) <= aS + bS + np.expm1(2 * dmax) * np.einsum("m,mi,mj->ij", e, dx, dx))
    print("N=%d D=%d: max |logw_paths - logw_pass| / (sum of budgets) %.3f" % (N, D, ratio.max()))


@pytest.mark.parametrize("n, m, R, S, D, P", [SHAPES[4], SHAPES[6]])
def test_determinism_and_independence_of_the_draws(n, m, R, S, D, P, form):
    c, lnq, bounds, centre = _problem(n, m, R, S, D, P)
    a = _args(c, P)
    lw1, rec1 = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    lw2, rec2 = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    assert _bits(lw1) == _bits(lw2) and _stat_bits(rec1) == _stat_bits(rec2)
    # every other draw's weights replaced: draw `keep` keeps its log-weights and its record to the bit
    rs = np.random.RandomState(9)
    for keep in (0, S - 1, S // 2):
        W, Wl, V = 5.0 * rs.standard_normal(c["W"].shape), rs.standard_normal(c["Wl"].shape), -3.0 * c["V"]
        W[keep], Wl[keep], V[:, keep] = c["W"][keep], c["Wl"][keep], c["V"][:, keep]
        lw3, rec3 = dev_path_importance(c["T"], c["X"], V, c["Z"], c["b"], W, Wl if P is not None else None, c["k"],
                                        c["mean"], lnq=lnq, bounds=bounds, centre=centre)
        assert _bits(lw3[keep]) == _bits(lw1[keep]) and _stat_bits([rec3[keep]]) == _stat_bits([rec1[keep]])
        other = (keep + 1) % S
        assert _bits(lw3[other]) != _bits(lw1[other])


def test_a_moments_workgroup_takes_a_second_tile():
    """The moments run in at most APGP_IMP_MAX_BLOCKS = 2048 workgroups of 256-row tiles: one tile beyond 524288 rows
    workgroup 0 of every draw takes a second one (the first stage never loops: 2049 workgroups).  Bit identity with
    apgp_path_draws on ALL rows, the record against the restatement on ALL rows."""
    n, R, S, D = 64, 64, 1, 2
    m = per.ROW_CAP + 256
    c = pr.case(n, m, R, S, D, seed=17)
    lnq = np.random.RandomState(18).normal(size=m)
    bounds, centre = [(-BOX, BOX)] * D, c["X"][0].copy()
    a = _args(c, None)
    F = tpd.dev_path_draws(*a)[0]
    lw, recs = dev_path_importance(*a, lnq=lnq, bounds=bounds, centre=centre)
    assert _bits(lw) == _bits(_expect_from_f(F, c["T"], lnq, bounds))
    assert np.isfinite(lw[0, per.ROW_CAP:]).any()
    print("second tile: record error / budget %.3f" % tgi._check_record(recs[0], lw[0], c["T"], centre))


def _fixture_gp(fx):
    """A GP holding the moment fixture's training set and kernel."""
    from approxposterior_amd import gp as agp
    k, D = fx["k"], fx["k"].ndim
    kern = agp.Product(agp.ConstantKernel(float(np.log(k.amp / D)), ndim=D),
                       agp.ExpSquaredKernel(1.0 / np.asarray(k.inv_metric), ndim=D))
    g = agp.GP(kernel=kern, fit_mean=True, mean=fx["mean"], white_noise=float(np.log(k.diag_add)), fit_white_noise=False)
    g.compute(fx["X"])
    ks = g._kernel_struct()
    assert np.isclose(ks.amp, k.amp, rtol=1e-14) and np.isclose(ks.diag_add, k.diag_add, rtol=1e-14)
    assert np.allclose(np.array(ks.inv_metric[:D]), k.inv_metric, rtol=1e-14) and ks.lin_coef == 0.0
    return g


@pytest.mark.parametrize("seed", [0, 1])
def test_identity_of_the_expected_posterior_on_the_device(seed):
    """tests/test_pathevidence_ref.py's identity with the device solving for V (GP._paths_from) and integrating
    (GP.importance_paths): the same seeds, the same host numbers, the same threshold of 5 standard errors."""
    fx, numbers, _ = per.moment_draws(seed)
    g = _fixture_gp(fx)
    R = len(fx["Z"])
    Zs = []
    for W, eps in numbers:
        paths = g._paths_from(fx["y"], fx["Z"], fx["b"], W[:, :R], W[:, R:], eps)
        recs = g.importance_paths(fx["y"], fx["T"], paths, centre=np.zeros(fx["k"].ndim))
        Zs.append(per.evidences(recs, len(fx["T"])))
    Zs = np.concatenate(Zs)
    assert Zs.shape == (256,) and np.all(np.isfinite(Zs))
    z, zplug = per.identity_scores(Zs, fx)
    print("seed %d: |z| = %.2f against exp(mu + v / 2), %.2f against exp(mu)" % (seed, z, zplug))
    assert z <= 5.0
    assert zplug > 5.0


OLD_KEYS = ("logZ", "logZErr", "ess", "mean", "cov", "nInside")
NEW_KEYS = ("logZDraws", "essDraws", "meanDraws", "covDraws", "logZSurrogateErr", "meanSurrogateErr", "logZExpected")


def _same_bits(a, b):
    for key in OLD_KEYS:
        assert _bits(a[key]) == _bits(b[key]), key


def test_evidence_with_surrogate_draws():
    a = tge._ap()
    M = 2 ** 14
    plain = a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M)
    assert set(plain) == set(OLD_KEYS)
    np.random.seed(21)
    s32 = a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M, surrogateDraws=32, nFeatures=512)
    _same_bits(s32, plain)
    assert set(s32) == set(OLD_KEYS + NEW_KEYS + ("nEmptyDraws",)) and s32["nEmptyDraws"] == 0
    for key in NEW_KEYS:
        assert np.all(np.isfinite(s32[key])), key
    assert s32["logZDraws"].shape == (32,) and s32["essDraws"].shape == (32,)
    assert s32["meanDraws"].shape == (32, 2) and s32["covDraws"].shape == (32, 2, 2) and s32["meanSurrogateErr"].shape == (2,)
    assert s32["logZSurrogateErr"] > 0.0 and np.all(s32["essDraws"] > 1.0)
    print("logZ %.6f +- %.6f (sampling) +- %.6f (surrogate); logZExpected %.6f" %
          (s32["logZ"], s32["logZErr"], s32["logZSurrogateErr"], s32["logZExpected"]))
    # 40 draws are two groups: the first group's sample_paths uses NumPy's stream exactly as the 32-draw call did
    np.random.seed(21)
    s40 = a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M, surrogateDraws=40, nFeatures=512)
    _same_bits(s40, plain)
    assert s40["logZDraws"].shape == (40,) and _bits(s40["logZDraws"][:32]) == _bits(s32["logZDraws"])
    assert s40["nEmptyDraws"] == 0 and all(np.all(np.isfinite(s40[key])) for key in NEW_KEYS)
    # two chunks: the plug-in keys carry the bits of the plain two-chunk call, the draws merge to rounding
    plain2 = a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M // 2)
    np.random.seed(21)
    c40 = a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M // 2, surrogateDraws=40, nFeatures=512)
    _same_bits(c40, plain2)
    assert np.allclose(c40["logZDraws"], s40["logZDraws"], rtol=0, atol=1e-11)
    assert np.allclose(c40["meanDraws"], s40["meanDraws"], rtol=0, atol=1e-10)
    assert abs(c40["logZExpected"] - s40["logZExpected"]) <= 1e-11 and c40["nEmptyDraws"] == 0
    # surrogateDraws = 0 is the plain call; a negative count is refused; seed=None is reproducible from NumPy's state
    _same_bits(a.evidence(nSamples=M, proposal="box", seed=tge.SEED, chunk=M, surrogateDraws=0), plain)
    with pytest.raises(ValueError):
        a.evidence(nSamples=M, proposal="box", surrogateDraws=-1)
    np.random.seed(22)
    u1 = a.evidence(nSamples=4096, proposal="box", surrogateDraws=3, nFeatures=64)
    np.random.seed(22)
    u2 = a.evidence(nSamples=4096, proposal="box", surrogateDraws=3, nFeatures=64)
    assert _bits(u1["logZDraws"]) == _bits(u2["logZDraws"]) and u1["logZ"] == u2["logZ"]


def test_importance_paths_checks_its_arguments():
    g, X, y, _ = tpd._gp_fixture(50, 2, 8)
    other, _, y2, _ = tpd._gp_fixture(50, 2, 9)
    paths = g.sample_paths(y, 2, nFeatures=64)
    T = X[:7]
    recs = g.importance_paths(y, T, paths)
    assert len(recs) == 2 and set(recs[0]) == set(g.importance_pass(y, T))
    assert np.array_equal(recs[0]["centre"], X[int(np.argmax(y))])
    with pytest.raises(ValueError):
        g.importance_paths(y, np.empty((0, 2)), paths)
    with pytest.raises(ValueError):
        g.importance_paths(y, T, paths, centre=[0.0, np.nan])
    with pytest.raises(ValueError):
        g.importance_paths(y, T, paths, lnq=np.zeros(3))
    with pytest.raises(ValueError):
        other.importance_paths(y2, T, paths)               # another GP's draws
    with pytest.raises(ValueError):
        g.importance_paths(y, T, None)
    g.set_parameter_vector(g.get_parameter_vector() + 0.1)
    g.recompute()
    with pytest.raises(RuntimeError):
        g.importance_paths(y, T, paths)
