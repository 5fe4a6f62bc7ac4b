# -*- coding: utf-8 -*-
"""MI355X: ONE call of the integrated acquisition pass (apgp_acquire_integrated, csrc/integrated.hip) through the C ABI,
handed the bits it is judged on -- a planted B, planted log-weights, a planted variance -- against
tests/integrated_ref.py: the columns c_j and u of every live row within a budget counted off the kernel's source (no
multiplier, no cond(K); tests/test_integrated_ref.py holds NumPy and the restated device order to the same bar on the
same inputs and shows that the bar catches its mutants).

  1. budget       every case of integrated_ref.ALL_CASES: n beside the 64-row tile and the 512-row padding, m beside the
                  256-row workgroup, every DPAD the pass takes (D <= 16), linear terms, J = 1, both sides of every column-tile width, three passes,
                  APGP_MAX_REFS; log-weights spread over 1e3 and tau^2 up to 2000 (a naive exp overflows);
  2. k(., .)      B = 0: column j IS k(t, r_j), with the bits of kvalue_ref's restatement (within kvalue_ref.budget with
                  a linear term); B = e_r: the column is k(t, r_j) - k(t, x_r), bit for bit, r in every lane of a step,
                  at the tile edge and at n - 1;
  3. footprint    ldc = m + 3 and sentinel tails: nothing but rows [0, m) of the J columns, u[0:m] and the work length
                  changes; inputs untouched; C = NULL and u = NULL give the same best;
  4. gate         rows outside the box, masked, with a NaN coordinate or with s <= 0: u = +inf, NaN in C, never the
                  winner; all gated: (-1, +inf); a column with a = -inf changes no bit of u;
  5. arg-min      best is the lowest-index minimum of the device's own u across workgroups, with exact ties and with
                  idx_offset = 2^33 + 5;
  6. rows         a row's u and C have the same bits in a call over a subset of the rows; the same call twice gives the
                  same bytes;
  7. both forms   the vector contraction (apgp_integrated_mode(1)) is within the same budget where the matrix cores are
                  the default.

Worst err / budget per case is printed (pytest -s) and recorded in docs/experiments.md."""
import ctypes

import numpy as np
import pytest

import integrated_ref as ir
import kvalue_ref as kr

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300


@pytest.fixture(scope="module")
def lib_loaded():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_abi_version() == _lib.ABI_VERSION
    assert lib.apgp_integrated_mode(-1) == 0
    return lib


def _ks(k):
    from approxposterior_amd import _lib
    ks = _lib.KernelStruct()
    ks.ndim, ks.lin_order, ks.amp, ks.diag_add, ks.lin_coef = k.ndim, k.lin_order, k.amp, k.diag_add, k.lin_coef
    ks.inv_metric[:k.ndim] = k.inv_metric.tolist()
    return ks


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to("cuda:0")      # (a copy: the shared inputs are read-only)


def _full(n, value=SENTINEL):
    import torch
    return torch.full((int(n),), value, dtype=torch.float64, device="cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Train(object):
    """The packed training stream of (X, kern) on the device; its alpha slot holds a value no B has."""

    def __init__(self, lib, X, k):
        import torch
        self.n, self.k, self.ks = len(X), k, _ks(k)
        self.xs = _full(lib.apgp_packed_train_len(self.n, k.ndim))
        Xd, ad = _dev(X), _dev(np.full(self.n, 1e30))
        rc = lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), self.n, ctypes.byref(self.ks), self.xs.data_ptr(), None)
        assert rc == 0, lib.apgp_last_error()
        torch.cuda.synchronize()


_TRAIN = {}


def train_of(lib, case):
    if case.name not in _TRAIN:
        inp = ir.inputs(case)
        _TRAIN[case.name] = Train(lib, inp["X"], inp["k"])
    return _TRAIN[case.name]


TAIL = 7


def call(lib, tr, T, R, B, a, var, bounds=None, mask=None, with_C=True, with_u=True, idx_offset=0, pad=0, check_inputs=False):
    """(C (m, J) or None, u (m,) or None, (index, u)); ``pad``: ldc = m + pad.  Every output buffer has a sentinel tail
    that must survive, and C's padding rows too."""
    import torch
    from approxposterior_amd import _lib
    m, J, D = len(T), len(R), tr.k.ndim
    ldc = m + pad
    ins = [_dev(T), _dev(R), _dev(B), _dev(a), _dev(var)]
    mk = None if mask is None else _dev(mask, np.uint8)
    xs0 = tr.xs.clone()
    wl = int(lib.apgp_integrated_work_len(m, J))
    assert wl == ir.work_len(m, J)
    part = _full(wl + TAIL)
    Cd = _full(J * ldc + TAIL) if with_C else None
    ud = _full(m + TAIL) if with_u else None
    best = _full(2 + TAIL)
    lo = hi = None
    if bounds is not None:
        arr = ctypes.c_double * _lib.MAX_DIM
        bb = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        lo, hi = arr(*bb[:, 0]), arr(*bb[:, 1])
    rc = lib.apgp_acquire_integrated(ins[0].data_ptr(), m, int(idx_offset), tr.xs.data_ptr(), tr.n, ctypes.byref(tr.ks),
                                     ins[1].data_ptr(), J, ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), lo, hi,
                                     None if mk is None else mk.data_ptr(), None if Cd is None else Cd.data_ptr(), ldc,
                                     None if ud is None else ud.data_ptr(), part.data_ptr(), best.data_ptr(), None)
    assert rc == 0, lib.apgp_last_error()
    torch.cuda.synchronize()
    sent = np.float64(SENTINEL)
    assert np.all(part[wl:].cpu().numpy() == sent) and np.all(best[2:].cpu().numpy() == sent)
    C = u = None
    if with_C:
        ch = Cd.cpu().numpy()
        assert np.all(ch[J * ldc:] == sent)
        cm = ch[:J * ldc].reshape(J, ldc)
        assert np.all(cm[:, m:] == sent)
        C = cm[:, :m].T.copy()
    if with_u:
        uh = ud.cpu().numpy()
        assert np.all(uh[m:] == sent)
        u = uh[:m].copy()
    if check_inputs:
        for d, h in zip(ins, (T, R, B, a, var)):
            assert same_bits(d.cpu().numpy().reshape(-1), np.asarray(h, dtype=np.float64).reshape(-1))
        assert torch.equal(tr.xs.view(torch.int64), xs0.view(torch.int64))
    bb = best[:2].cpu().numpy()
    return C, u, (int(bb[1:2].view(np.int64)[0]), float(bb[0]))


def case_call(lib, case, **kw):
    inp = ir.inputs(case)
    return call(lib, train_of(lib, case), inp["T"], inp["R"], inp["B"], inp["a"], inp["var"], **kw)


# ---- 1. budget -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ir.ALL_CASES, ids=lambda c: c.name)
def test_budget(lib_loaded, case):
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    C, ud, best = case_call(lib_loaded, case)
    rc, ru = ir.ratio(C, c, bc), ir.ratio(ud, u, bu)
    print("%s c %.3f u %.3f (largest tau^2 %.0f)" % (case.name, rc, ru, float(tau2.max())))
    assert rc <= 1.0 and ru <= 1.0
    assert best == ir.argmin(ud)


# ---- 7. the vector form where the matrix cores are the default -------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ir.N_CASES + ir.J_CASES + ir.LIN_CASES + ir.D_CASES if kr.dpad(c.D) <= 8],
                         ids=lambda c: c.name)
def test_budget_vector_form(lib_loaded, case):
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    assert lib_loaded.apgp_integrated_mode(1) == 0
    try:
        C, ud, best = case_call(lib_loaded, case)
    finally:
        assert lib_loaded.apgp_integrated_mode(0) == 1
    rc, ru = ir.ratio(C, c, bc), ir.ratio(ud, u, bu)
    print("%s vector c %.3f u %.3f" % (case.name, rc, ru))
    assert rc <= 1.0 and ru <= 1.0
    assert best == ir.argmin(ud)


def test_vector_form_is_the_restatement(lib_loaded):
    """The vector form's order IS integrated_ref.restate's: the columns agree bit for bit (u differs by the two
    logarithms, the device's and math.log: test_budget_vector_form holds it to the budget)."""
    case = ir.CASE_BY_NAME["J17"]
    inp = ir.inputs(case)
    rows = ir.restate_rows(case)
    lib_loaded.apgp_integrated_mode(1)
    try:
        C, ud, _ = case_call(lib_loaded, case)
    finally:
        lib_loaded.apgp_integrated_mode(0)
    gc, gu = ir.restate(*ir.args(inp), rows=rows)
    assert same_bits(C[rows], gc)


# ---- 2. kernel values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("D1", "D4", "D8", "D9", "D16", "P1-D3", "P2-D8", "P1-D16"))
@pytest.mark.parametrize("mode", (0, 1))
def test_zero_B_gives_the_kernel_value(lib_loaded, name, mode):
    case = ir.CASE_BY_NAME[name]
    inp = ir.inputs(case)
    k = inp["k"]
    lib_loaded.apgp_integrated_mode(mode)
    try:
        C, _, _ = call(lib_loaded, train_of(lib_loaded, case), inp["T"], inp["R"], np.zeros_like(inp["B"]), inp["a"], inp["var"])
    finally:
        lib_loaded.apgp_integrated_mode(0)
    rows = np.arange(min(case.m, 131))
    if k.lin_coef == 0.0:
        want = kr.restate(inp["T"][rows], inp["R"], k, site="cross")
        assert same_bits(C[rows], want)
        assert same_bits(C, C[np.arange(case.m) % 131])          # the tiled rows repeat them
    else:
        ratio, _ = kr.err_over_budget(C[rows], inp["T"][rows], inp["R"], k)
        print("%s mode %d k(t, r) / kvalue budget %.3f" % (name, mode, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize("mode", (0, 1))
def test_unit_B_gives_the_training_kernel_value(lib_loaded, mode):
    case = ir.CASE_BY_NAME["D8"]                                  # n = 129: three tiles
    inp = ir.inputs(case)
    k, n = inp["k"], case.n
    picks = [0, 1, 2, 3, 62, 63, 64, 65, n - 1]
    far = inp["X"].mean(0) + 1e4 / np.sqrt(k.inv_metric)          # k(t, r) sits at the clamp floor amp exp(-700)
    R = np.tile(far, (len(picks), 1))
    B = np.zeros((n, len(picks)))
    B[picks, np.arange(len(picks))] = 1.0
    lib_loaded.apgp_integrated_mode(mode)
    try:
        C, _, _ = call(lib_loaded, train_of(lib_loaded, case), inp["T"], R, B, np.zeros(len(picks)), inp["var"])
    finally:
        lib_loaded.apgp_integrated_mode(0)
    rows = np.arange(131)
    kx = kr.restate(inp["T"][rows], inp["X"][picks], k, site="cross")
    kfar = kr.restate(inp["T"][rows], R, k, site="cross")
    assert np.all(kfar < 1e-300)
    assert same_bits(C[rows], kfar - kx)


# ---- 3. footprint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("m255", "J65", "D16"))
def test_footprint(lib_loaded, name):
    case = ir.CASE_BY_NAME[name]
    C0, u0, b0 = case_call(lib_loaded, case)
    C1, u1, b1 = case_call(lib_loaded, case, pad=3, check_inputs=True)        # (call() asserts the sentinels)
    assert same_bits(C0, C1) and same_bits(u0, u1) and b0 == b1
    _, _, b2 = case_call(lib_loaded, case, with_C=False, with_u=False)
    assert b2 == b0


# ---- 4. gate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("m257", "D9"))
def test_gate(lib_loaded, name):
    case = ir.CASE_BY_NAME[name]
    inp = ir.inputs(case)
    tr = train_of(lib_loaded, case)
    C0, u0, b0 = case_call(lib_loaded, case)
    win = b0[0]
    T = np.array(inp["T"])
    var = np.array(inp["var"])
    mask = np.ones(case.m, dtype=np.uint8)
    lo, hi = T.min(0) - 1.0, T.max(0) + 1.0
    gated = {"box": win, "mask": (win + 1) % case.m, "nan": (win + 2) % case.m, "s0": (win + 3) % case.m,
             "sneg": (win + 4) % case.m, "snan": (win + 5) % case.m}
    T[gated["box"], 0] = hi[0] + 0.5
    mask[gated["mask"]] = 0
    T[gated["nan"], case.D - 1] = np.nan
    var[gated["s0"]] = -inp["k"].diag_add
    var[gated["sneg"]] = -1.0
    var[gated["snan"]] = np.nan
    C, u, b = call(lib_loaded, tr, T, inp["R"], inp["B"], inp["a"], var, bounds=np.stack([lo, hi], 1), mask=mask)
    rows = sorted(gated.values())
    live = np.setdiff1d(np.arange(case.m), rows)
    assert np.all(u[rows] == np.inf) and np.all(np.isnan(C[rows]))
    assert same_bits(u[live], u0[live]) and same_bits(C[live], C0[live])
    assert b == ir.argmin(u) and b[0] not in rows
    _, u_all, b_all = call(lib_loaded, tr, T, inp["R"], inp["B"], inp["a"], var, mask=np.zeros(case.m, dtype=np.uint8))
    assert np.all(u_all == np.inf) and b_all == (-1, np.inf)


@pytest.mark.parametrize("name,mode", (("J17", 0), ("J65", 0), ("J17", 1), ("J17-D9", 0)))
def test_minus_infinity_column_changes_no_bit(lib_loaded, name, mode):
    case = ir.CASE_BY_NAME[name]
    inp = ir.inputs(case)
    tr = train_of(lib_loaded, case)
    lib_loaded.apgp_integrated_mode(mode)
    try:
        for drop in (0, 5, case.J - 1):
            a = np.array(inp["a"])
            a[drop] = -np.inf
            _, u0, b0 = call(lib_loaded, tr, inp["T"], inp["R"], inp["B"], a, inp["var"])
            keep = np.arange(case.J) != drop
            _, u1, b1 = call(lib_loaded, tr, inp["T"], inp["R"][keep], inp["B"][:, keep], a[keep], inp["var"])
            assert np.all(np.isfinite(u0)) and same_bits(u0, u1) and b0 == b1
    finally:
        lib_loaded.apgp_integrated_mode(0)


# ---- 5. arg-min contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx_offset", (0, 2 ** 33 + 5))
def test_argmin_contract_across_workgroups_with_ties(lib_loaded, idx_offset):
    case = ir.CASE_BY_NAME["J33"]
    inp = ir.inputs(case)
    tr = train_of(lib_loaded, case)
    m = 700                                                        # three workgroups; rows i and i + 131 are the same point
    T = inp["T"][np.arange(m) % 131]
    var = np.array(inp["var"][np.arange(m) % 131])
    _, u, b = call(lib_loaded, tr, T, inp["R"], inp["B"], inp["a"], var, idx_offset=idx_offset)
    assert same_bits(u, u[np.arange(m) % 131])                     # exact ties, in different workgroups
    assert b == ir.argmin(u, idx_offset) and b[0] - idx_offset < 131
    first = b[0] - idx_offset
    mask = np.ones(m, dtype=np.uint8)
    mask[first] = 0                                                # the tie's next copy takes over, in the same or the next workgroup
    _, u2, b2 = call(lib_loaded, tr, T, inp["R"], inp["B"], inp["a"], var, idx_offset=idx_offset, mask=mask)
    assert b2 == (idx_offset + first + 131, b[1])


# ---- 6. row independence, determinism ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", (("J65", 0), ("J17", 1), ("D16", 0)))
def test_rows_are_independent_and_calls_repeat(lib_loaded, name, mode):
    case = ir.CASE_BY_NAME[name]
    inp = ir.inputs(case)
    tr = train_of(lib_loaded, case)
    lib_loaded.apgp_integrated_mode(mode)
    try:
        C0, u0, b0 = case_call(lib_loaded, case)
        C1, u1, b1 = case_call(lib_loaded, case)
        assert C0.tobytes() == C1.tobytes() and u0.tobytes() == u1.tobytes() and b0 == b1
        rows = np.array([250, 3, 77, 256, 19])
        Cs, us, _ = call(lib_loaded, tr, inp["T"][rows], inp["R"], inp["B"], inp["a"], inp["var"][rows])
        assert same_bits(Cs, C0[rows]) and same_bits(us, u0[rows])
    finally:
        lib_loaded.apgp_integrated_mode(0)
