# -*- coding: utf-8 -*-
"""MI355X: ONE call of the fantasy pass (apgp_acquire_fantasy, fantasy_kernel in csrc/sweep.hip) through the C ABI, handed
the bits it is judged on -- a planted beta, planted earlier columns, a planted input variance -- against
tests/fantasy_ref.py: the column C_j and the variance v_j of every live row within a budget counted off the kernel's
source (no multiplier, no cond(K); tests/test_fantasy_ref.py holds NumPy and the restated device order to the same bar on
the same inputs and shows that the bar catches its mutants).

  1. budget       every case of fantasy_ref.BUDGET_CASES: n beside the 128-row tile, the four lanes and the 512-row
                  padding; every DPAD; linear terms; m beside the 256-row workgroup; j = 1, 2, 31; a realistic beta;
  2. k(t, x)      the epilogue's value (beta = 0, j = 1, s = 1: the column IS k(t, x_j)) has the bits of one of
                  kvalue_ref's restatements, or with a linear term is within kvalue_ref.budget; the tile loop's value
                  (beta = e_r, the pick out at the clamp floor) for r in every lane, at the tile edge and at n - 1;
  3. footprint    ldc = m + 3, j + 2 columns: nothing but rows [0, m) of column j - 1 changes; inputs untouched;
                  u = NULL gives the same best;
  4. downdate     j in 1, 2, 31 with the pick row in the first workgroup, in the last one and at m - 1;
  5. chain        31 calls that ping-pong the variance buffers, each judged from the device's own earlier output;
  6. idx_offset   2^33 + 5;
  7. determinism  the same call twice, the same bytes.

Worst err / budget per case is printed (pytest -s) and recorded in docs/experiments.md."""
import ctypes

import numpy as np
import pytest

import fantasy_ref as fr
import kvalue_ref as kr
import sweep_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300
UTIL_AGP = 0


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
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0")    # (a copy: the shared inputs are read-only)


def _full(shape, value=SENTINEL):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device="cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Train(object):
    """The packed training stream of (X, kern) on the device; its alpha slot holds a value no beta has, so that a pass
    that summed the stream's own slot instead of beta could not stay within any budget."""

    def __init__(self, lib, X, k):
        import torch
        self.n, self.k, self.ks = len(X), k, _ks(k)
        self.xs = _full((int(lib.apgp_packed_train_len(self.n, k.ndim)),))
        Xd, ad = _dev(X), _dev(np.full(self.n, 1e30))
        rc = lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), self.n, ctypes.byref(self.ks), self.xs.data_ptr(), None)
        assert rc == 0, lib.apgp_last_error()
        torch.cuda.synchronize()


def run_pass(lib, train, T, beta, pick, Cprev, var_in, mu, ldc=None, ncols=None, with_u=True, idx_offset=0, tail=8):
    """One call.  Every output buffer is pre-filled with the sentinel and is ``tail`` (or ldc - m) entries longer than
    the call may write.  Returns a dict of host copies: the whole C buffer before and after, C_j, v_j, u, best, and the
    inputs as they came back."""
    import torch
    m, n = len(T), train.n
    Cprev = np.asarray(Cprev, dtype=np.float64).reshape(-1, m)
    j = len(Cprev) + 1
    ldc = m if ldc is None else ldc
    ncols = j if ncols is None else ncols
    C0 = np.full((ncols, ldc), SENTINEL)
    C0[:j - 1, :m] = Cprev
    Td, bd, Cd, mud, vin = _dev(T), _dev(beta), _dev(C0), _dev(mu), _dev(var_in)
    vout, ud = _full((m + tail,)), _full((m + tail,))
    nwork = int(lib.apgp_acquire_fantasy_work_len(m))
    assert nwork == 2 * ((m + 255) // 256)
    part = _full((nwork + tail,))
    best = torch.full((2,), 0x7ff8dead7ff8dead, dtype=torch.int64, device="cuda:0")
    rc = lib.apgp_acquire_fantasy(Td.data_ptr(), m, idx_offset, train.xs.data_ptr(), n, ctypes.byref(train.ks),
                                  bd.data_ptr(), pick, j, Cd.data_ptr(), ldc, mud.data_ptr(), vin.data_ptr(),
                                  vout.data_ptr(), UTIL_AGP, None, None, None, 0.01, 0.0,
                                  ud.data_ptr() if with_u else None, part.data_ptr(), best.data_ptr(), None)
    assert rc == 0, lib.apgp_last_error()
    torch.cuda.synchronize()
    C1 = Cd.cpu().numpy()
    b = best.cpu().numpy()
    return {"C0": C0, "C1": C1, "C": C1[j - 1, :m].copy(), "v": vout.cpu().numpy()[:m].copy(), "vout": vout.cpu().numpy(),
            "u": ud.cpu().numpy(), "best_u": b[:1].view(np.float64)[0], "best_i": int(b[1]), "part_tail": part.cpu().numpy()[nwork:],
            "T": Td.cpu().numpy(), "beta": bd.cpu().numpy(), "mu": mud.cpu().numpy(), "var_in": vin.cpu().numpy(), "j": j, "m": m}


_SHARED = {}


def shared(lib, case):
    """(inputs, Pass, truth, budget, Train) of a case: computed once, shared by the tests that use it, never changed."""
    if case.name not in _SHARED:
        inp = fr.pass_inputs(case)
        P = fr.Pass(inp["T"], inp["X"], inp["k"])
        call = (inp["beta"], inp["pick"], inp["Cprev"], inp["var_in"])
        _SHARED[case.name] = (inp, P, P.truth(*call), P.budget(*call), Train(lib, inp["X"], inp["k"]))
    return _SHARED[case.name]


def call_case(lib, case, **kw):
    inp, P, truth, bud, train = shared(lib, case)
    return run_pass(lib, train, inp["T"], inp["beta"], inp["pick"], inp["Cprev"], inp["var_in"], inp["mu"], **kw)


def judge(out, truth, bud, what):
    """Every live row of C_j and v_j within the budget -- nothing is left out; the ratios are printed first."""
    rC, rv = fr.ratio(out["C"], truth[0], bud[0]), fr.ratio(out["v"], truth[1], bud[1])
    print("fantasy pass %-14s m=%-4d j=%-2d worst |C - truth| / budget %.3f, |v - truth| / budget %.3f"
          % (what, out["m"], out["j"], rC, rv))
    assert len(out["C"]) == len(out["v"]) == out["m"] == len(bud[0])
    assert rC <= 1.0, (what, "C_j", rC)
    assert rv <= 1.0, (what, "v_j", rv)
    return rC, rv


# ----------------------------------------------------------------------------------------------------------------------
# 1. budget
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.BUDGET_CASES, ids=lambda c: c.name)
def test_column_and_variance_within_budget(lib_loaded, case):
    inp, P, truth, bud, train = shared(lib_loaded, case)
    judge(call_case(lib_loaded, case), truth, bud, case.name)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the two k(t, x) sites
# ----------------------------------------------------------------------------------------------------------------------
def probe_set(n, D, order, seed):
    """(X, T, k): sweep_ref.case's points with amp = 1 and no noise, the candidates within 3.5 length scales of x_0 ..
    and row 0 ON x_0 (the coincident pair: k = amp exactly)."""
    X, _, Tb, k, _ = sr.case(n, D, order)
    k = k._replace(amp=1.0, diag_add=0.0)
    rs = np.random.RandomState(9500 + seed)
    ell = 1.0 / np.sqrt(k.inv_metric)
    T = X[0] + ell * rs.uniform(-1.0, 1.0, size=(sr.BASE, D)) * 3.5 / np.sqrt(D)
    T[0] = X[0]
    return X, T, k


@pytest.mark.parametrize("D", fr.PASS_D)
def test_epilogue_kvalue_has_restated_bits(lib_loaded, D):
    """beta = 0, j = 1, diag_add = 0, var_in[pick] = 1: C = (kx - 0) / sqrt(1) = k(t, x_j), every operation after kx
    exact.  Pure squared-exponential kernel: the bits of kvalue_ref's plain restatement (site "cross") or of the fused
    one (site "sweep", fused: the scaling of one of the two points contracted into the subtraction; the kernel is compiled
    with contraction allowed and both t sc and x_j sc are formed in the epilogue's reach)."""
    lib = lib_loaded
    m = 257
    X, Tb, k = probe_set(129, D, None, D)
    T = sr.tiled(Tb, m)
    train = Train(lib, X, k)
    counts = {}
    for pick in (0, 77, m - 1):
        xj = T[pick:pick + 1]
        out = run_pass(lib, train, T, np.zeros(len(X)), pick, np.zeros((0, m)), np.ones(m), np.zeros(m))
        plain = kr.restate(Tb, xj, k, site="cross")[:, 0]
        assert same_bits(plain, kr.restate(Tb, xj, k, site="sweep")[:, 0])
        fused_t = kr.restate(Tb, xj, k, site="sweep", fused=True)[:, 0]          # df = fma(t, sc, -x_j sc)
        fused_x = kr.restate(xj, Tb, k, site="sweep", fused=True)[0, :]          # df = fma(-x_j, sc, t sc): the same square
        got = out["C"].view(np.int64)
        rep = np.arange(m) % len(Tb)
        hit = [got == w[rep].view(np.int64) for w in (plain, fused_t, fused_x)]
        bad = np.nonzero(~(hit[0] | hit[1] | hit[2]))[0]
        assert len(bad) == 0, (D, pick, "k(t, x_j) has the bits of no restatement", len(bad), bad[:8], out["C"][bad[:8]], plain[rep][bad[:8]])
        assert out["C"][pick] == k.amp
        assert same_bits(out["v"], [kr.fma(-float(c), float(c), 1.0) for c in out["C"]]), "v_j is not fma(-C, C, var_in)"
        differ = plain[rep].view(np.int64) != fused_t[rep].view(np.int64)
        differ_x = plain[rep].view(np.int64) != fused_x[rep].view(np.int64)
        counts[pick] = (int(hit[0].sum()), int((hit[1] & differ).sum()), int((hit[2] & differ_x).sum()), int((differ | differ_x).sum()))
    print("epilogue k(t, x_j) D=%-2d: per pick (rows with the plain restatement's bits, rows that have only the bits with "
          "t's scaling fused, only with x_j's scaling fused, rows where the restatements differ at all) of %d: %s" % (D, m, counts))


@pytest.mark.parametrize("order,D", [(0, 3), (1, 8), (2, 32), (2, 3)])
def test_epilogue_kvalue_with_linear_term_within_budget(lib_loaded, order, D):
    lib = lib_loaded
    m = 257
    X, Tb, k = probe_set(129, D, order, 40 + D + order)
    T = sr.tiled(Tb, m)
    train = Train(lib, X, k)
    for pick in (0, 77):
        out = run_pass(lib, train, T, np.zeros(len(X)), pick, np.zeros((0, m)), np.ones(m), np.zeros(m))
        with np.errstate(all="ignore"):
            t = kr.truth_ld(Tb, T[pick:pick + 1], k)[:, 0]
            b = kr.budget(Tb, T[pick:pick + 1], k)[:, 0]
        rep = np.arange(m) % len(Tb)
        r = fr.ratio(out["C"], t[rep], b[rep])
        print("epilogue k(t, x_j) P=%d D=%-2d pick %-3d worst err / kvalue budget %.3f" % (order, D, pick, r))
        assert r <= 1.0


PROBE_N = 257


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("r", [0, 1, 2, 3, 127, 128, PROBE_N - 1])
def test_tile_loop_kvalue_within_budget(lib_loaded, D, r):
    """beta = e_r, j = 1, s = 1, and the pick row 40 length scales out in every coordinate: its k(t, x_j) sits at the
    clamp floor amp exp(-700) for every other row, so -C = k(t, x_r) - floor: the tile loop's value through apgp_exp4,
    lane r & 3, exactly (the lanes add zeros).  Bar: kvalue_ref.budget + the floor."""
    lib = lib_loaded
    n, m = PROBE_N, 257
    X, _, _, k, _ = sr.case(n, D, None)
    k = k._replace(amp=1.0, diag_add=0.0)
    rs = np.random.RandomState(9600 + r)
    ell = 1.0 / np.sqrt(k.inv_metric)
    Tb = X[r] + ell * rs.uniform(-1.0, 1.0, size=(sr.BASE, D)) * 3.5 / np.sqrt(D)
    Tb[0] = X[r]
    T = sr.tiled(Tb, m)
    pick = m - 2
    T[pick] = X.mean(0) + 40.0 * ell
    floor = k.amp * 1e-304
    others = np.arange(m) != pick
    with np.errstate(all="ignore"):
        assert np.all(kr.truth_ld(T[others], T[pick:pick + 1], k) < floor)
    beta = np.zeros(n)
    beta[r] = 1.0
    out = run_pass(lib, Train(lib, X, k), T, beta, pick, np.zeros((0, m)), np.ones(m), np.zeros(m))
    with np.errstate(all="ignore"):
        t = kr.truth_ld(T, X[r:r + 1], k)[:, 0]
        b = kr.budget(T, X[r:r + 1], k)[:, 0]
    assert t[others].min() >= 2.0 ** -20
    ratio = fr.ratio(-out["C"][others], t[others], b[others] + floor * (1.0 + 2.0 ** -20))
    want = [kr.restate(Tb, X[r:r + 1], k, site="sweep", fused=f)[:, 0][np.arange(m) % len(Tb)] for f in (False, True)]
    hits = [int(((-out["C"]).view(np.int64) == w.view(np.int64))[others].sum()) for w in want]
    print("tile loop k(t, x_r) D=%d r=%-3d worst err / (kvalue budget + floor) %.3f; rows with the plain restatement's bits "
          "%d, with the fused one's %d, of %d" % (D, r, ratio, hits[0], hits[1], int(others.sum())))
    assert ratio <= 1.0
    assert out["C"][0] == -k.amp                                  # the coincident pair t = x_r
    assert t[pick] < floor and out["C"][pick] == k.amp            # the pick row itself: k(x_j, x_j) = amp, k(x_j, x_r) at the floor


# ----------------------------------------------------------------------------------------------------------------------
# 3. nothing else is written
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["j1", "j2", "j31", "m1", "m255", "m1000"])
def test_nothing_else_is_written(lib_loaded, name):
    lib = lib_loaded
    case = fr.CASE_BY_NAME[name]
    inp, P, truth, bud, train = shared(lib, case)
    m, j = case.m, case.j
    out = call_case(lib, case, ldc=m + 3, ncols=j + 2)
    judge(out, truth, bud, name + " ldc=m+3")
    keep = np.ones(out["C0"].shape, dtype=bool)
    keep[j - 1, :m] = False
    assert same_bits(out["C1"][keep], out["C0"][keep]), "C was written outside rows [0, m) of column j - 1"
    assert same_bits(out["C1"][:j - 1, :m], inp["Cprev"])
    assert not np.any(out["C1"][j - 1, :m] == SENTINEL)
    assert same_bits(out["var_in"], inp["var_in"]) and same_bits(out["mu"], inp["mu"])
    assert same_bits(out["T"], inp["T"]) and same_bits(out["beta"], inp["beta"])
    assert same_bits(out["vout"][m:], np.full(len(out["vout"]) - m, SENTINEL)), "var_out written beyond m"
    assert same_bits(out["u"][m:], np.full(len(out["u"]) - m, SENTINEL)), "u written beyond m"
    assert same_bits(out["part_tail"], np.full(len(out["part_tail"]), SENTINEL)), "scratch written beyond its length"
    dense = call_case(lib, case)
    assert same_bits(dense["C"], out["C"]) and same_bits(dense["v"], out["v"]), "the leading dimension changed a bit"
    nou = call_case(lib, case, with_u=False)
    assert same_bits(nou["u"], np.full(len(nou["u"]), SENTINEL))
    assert nou["best_i"] == dense["best_i"]
    assert np.float64(nou["best_u"]).view(np.int64) == np.float64(dense["best_u"]).view(np.int64)
    assert same_bits(nou["C"], dense["C"]) and same_bits(nou["v"], dense["v"])


# ----------------------------------------------------------------------------------------------------------------------
# 4. downdate
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.DOWNDATE_CASES, ids=lambda c: c.name)
def test_downdate_by_the_earlier_columns(lib_loaded, case):
    inp, P, truth, bud, train = shared(lib_loaded, case)
    if case.j > 1:
        assert (inp["Cprev"] > 0).any() and (inp["Cprev"] < 0).any()
    judge(call_case(lib_loaded, case), truth, bud, case.name)


# ----------------------------------------------------------------------------------------------------------------------
# 5. a 31-step chain
# ----------------------------------------------------------------------------------------------------------------------
def test_chain_of_31_steps_each_within_the_one_step_budget(lib_loaded):
    """31 successive calls write columns 0 .. 30 of one buffer and ping-pong two variance buffers; beta is planted per
    step; the pick is the row whose current (device) variance is largest.  Step j is judged against the truth computed
    from the bits of the device's own columns 0 .. j - 2 and variance j - 1: the bar is the one-step budget."""
    import torch
    lib = lib_loaded
    n, m, D, steps = 257, 257, 8, 31
    X, _, Tb, k, _ = sr.case(n, D, None)
    k = k._replace(diag_add=fr.DIAG_ADD)
    T = sr.tiled(Tb, m)
    P = fr.Pass(T, X, k)
    train = Train(lib, X, k)
    rs = np.random.RandomState(9700)
    ldc = m + 3
    Td, mud = _dev(T), _dev(rs.normal(size=m))
    Cd = _full((steps + 1, ldc))
    v0 = 1e3 * rs.uniform(1.0, 2.0, size=m)
    var = [_dev(np.r_[v0, np.full(8, SENTINEL)]), _full((m + 8,))]
    ud = _full((m,))
    part = _full((int(lib.apgp_acquire_fantasy_work_len(m)),))
    best = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    worst = (0.0, 0.0)
    for j in range(1, steps + 1):
        src, dst = var[(j - 1) & 1], var[j & 1]
        v_in = src.cpu().numpy()[:m].copy()
        Cprev = Cd.cpu().numpy()[:j - 1, :m].copy()
        pick = int(np.argmax(v_in))
        assert np.all(np.isfinite(v_in)) and v_in[pick] + k.diag_add > 0.0
        beta = fr.planted_beta(rs, n) / 100.0
        bd = _dev(beta)
        rc = lib.apgp_acquire_fantasy(Td.data_ptr(), m, 0, train.xs.data_ptr(), n, ctypes.byref(train.ks), bd.data_ptr(),
                                      pick, j, Cd.data_ptr(), ldc, mud.data_ptr(), src.data_ptr(), dst.data_ptr(), UTIL_AGP,
                                      None, None, None, 0.01, 0.0, ud.data_ptr(), part.data_ptr(), best.data_ptr(), None)
        assert rc == 0, lib.apgp_last_error()
        torch.cuda.synchronize()
        C1 = Cd.cpu().numpy()
        assert same_bits(C1[:j - 1, :m], Cprev), "an earlier column changed"
        assert same_bits(src.cpu().numpy()[:m], v_in), "the input variance changed"
        tC, tv = P.truth(beta, pick, Cprev, v_in)
        bC, bv = P.budget(beta, pick, Cprev, v_in)
        rC, rv = fr.ratio(C1[j - 1, :m], tC, bC), fr.ratio(dst.cpu().numpy()[:m], tv, bv)
        worst = (max(worst[0], rC), max(worst[1], rv))
        assert rC <= 1.0 and rv <= 1.0, (j, pick, rC, rv)
    C1 = Cd.cpu().numpy()
    assert same_bits(C1[steps], np.full(ldc, SENTINEL)) and same_bits(C1[:, m:], np.full((steps + 1, 3), SENTINEL))
    assert same_bits(var[0].cpu().numpy()[m:], np.full(8, SENTINEL)) and same_bits(var[1].cpu().numpy()[m:], np.full(8, SENTINEL))
    print("fantasy chain of %d steps n=%d m=%d: worst one-step |C - truth| / budget %.3f, |v - truth| / budget %.3f"
          % (steps, n, m, worst[0], worst[1]))


# ----------------------------------------------------------------------------------------------------------------------
# 6. idx_offset, 7. determinism
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m1000", "j31-pick520"])
def test_idx_offset_and_best(lib_loaded, name):
    lib = lib_loaded
    case = fr.CASE_BY_NAME[name]
    off = 2 ** 33 + 5
    out = call_case(lib, case, idx_offset=off)
    u = out["u"][:case.m]
    assert np.isfinite(u).sum() >= 20 and np.isnan(u).sum() >= 20, "the planted variance leaves v_j on both sides of zero"
    want = fr.argmin(u)
    assert want >= 0 and out["best_i"] - off == want, (out["best_i"], want)
    assert np.float64(out["best_u"]).view(np.int64) == u[want].view(np.int64)
    base = call_case(lib, case)
    assert base["best_i"] == want and same_bits(base["u"], out["u"])


@pytest.mark.parametrize("name", ["n513-D8", "P2-D32", "j31-pick599"])
def test_same_call_twice_same_bytes(lib_loaded, name):
    lib = lib_loaded
    case = fr.CASE_BY_NAME[name]
    a, b = call_case(lib, case), call_case(lib, case)
    for key in ("C1", "vout", "u"):
        assert same_bits(a[key], b[key]), key
    assert a["best_i"] == b["best_i"]
    assert np.float64(a["best_u"]).view(np.int64) == np.float64(b["best_u"]).view(np.int64)
