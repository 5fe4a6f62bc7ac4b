# -*- coding: utf-8 -*-
"""MI355X: apgp_predict_grad through the C ABI, kernel by kernel, each stage judged on the bits it was handed -- which the
call leaves in the caller's ``work`` (tests/predgrad_ref.py: ``work_views``) -- against the budgets of
tests/predgrad_ref.py's docstring.  The budgets are rounding counts read off csrc/predgrad.hip, not fitted to device
output, and contain no condition number; tests/test_predgrad_ref.py pins the layout against the source, holds a float64
restatement of the device order and NumPy / SciPy to the same bars on the same inputs, and shows that every bar catches
its mutants.

  k       pg_kstar_kernel: kbuf against kvalue_ref's truth to kvalue_ref's budget, the pad n .. ns exactly zero;
  v       pg_fwd_body: W k from the device's k;            w   pg_bwd_body: every partial plane from the device's v;
  solve   pg_solve_body: |L v - k| and |L^T w - v| row by row;
  finish  pg_finish_kernel: mu, var, dmu, dvar from the stream's bits, the device's v and partial planes;
  chain   util_grad.h: u through util_ref.judge, du against mpmath's derivatives at the device's (mu, var).

Before every call ``work`` is filled with NaN and the outputs with a sentinel; W / L carry NaN above the diagonal and in
the row padding: a NaN in any output of an in-box row is a read outside the contract.  Every case runs with two leading
dimensions, which must not change a bit.  Worst ratios are printed (pytest -s) and recorded in docs/experiments.md,
round 24."""
import ctypes

import numpy as np
import pytest

import kvalue_ref as kr
import predgrad_ref as ref
import util_ref

pytestmark = pytest.mark.gpu

SENTINEL = ref.SENTINEL
NONE = 3
WORST = {}


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


def _full(shape, value=SENTINEL):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device="cuda:0")


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.apgp_last_error())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Device(object):
    """The planted model of a ``ref.Case`` on the device: the packed stream (apgp_pack_train) and its bits."""

    def __init__(self, lib, case):
        import torch
        self.lib, self.case = lib, case
        self.ks = _ks(case.k)
        dp = kr.dpad(case.D)
        self.xs = _full((int(lib.apgp_packed_train_len(case.n, case.D)),))
        Xd, ad = _dev(case.X), _dev(case.alpha)
        _ok(lib, lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), case.n, ctypes.byref(self.ks), self.xs.data_ptr(), None),
            "apgp_pack_train")
        torch.cuda.synchronize()
        self.xs_bits = self.xs.cpu().numpy()[:case.n * (dp + 2)].reshape(case.n, dp + 2).copy()
        self.panels = {}

    def call(self, T, ld, kind=NONE, box=None, zeta=ref.UTIL_ZETA, ybest=ref.UTIL_YBEST, keep_work=True):
        """One call: the record ``ref.judge`` takes, plus "u" and "du".  ``work`` starts as NaN, the outputs as the
        sentinel."""
        import torch
        lib, case = self.lib, self.case
        n, D = case.n, case.D
        T = np.ascontiguousarray(T, dtype=np.float64)
        m = len(T)
        if ld not in self.panels:
            self.panels = {ld: _dev(case.panel(ld))}           # (one at a time: 134 MB at n = 4097)
        Ad = self.panels[ld]
        wl = int(lib.apgp_predict_grad_work_len(m, n))
        assert wl == ref.work_len(m, n)
        work = _full((wl,), float("nan"))
        Td = _dev(T)
        o = {key: _full((m,)) for key in ("mu", "var", "u")}
        o.update({key: _full((m, D)) for key in ("dmu", "dvar", "du")})
        lo = hi = None
        if box is not None:
            lo, hi = (ctypes.c_double * D)(*box[0]), (ctypes.c_double * D)(*box[1])
        inverse = case.route == "inverse"
        _ok(lib, lib.apgp_predict_grad(Td.data_ptr(), m, self.xs.data_ptr(), n, ctypes.byref(self.ks), case.mean,
                                       Ad.data_ptr() if inverse else None, ld if inverse else 0,
                                       None if inverse else Ad.data_ptr(), 0 if inverse else ld,
                                       kind, lo, hi, zeta, ybest, o["mu"].data_ptr(), o["var"].data_ptr(),
                                       o["u"].data_ptr(), o["dmu"].data_ptr(), o["dvar"].data_ptr(), o["du"].data_ptr(),
                                       work.data_ptr(), None), "apgp_predict_grad")
        torch.cuda.synchronize()
        rec = {key: t.cpu().numpy() for key, t in o.items()}
        rec["xs"] = self.xs_bits
        if keep_work and m <= ref.chunk(m, n):
            vw = ref.work_views(work.cpu().numpy(), m, n, case.route)
            rec.update({"k": vw["k"], "v": vw["v"], "w": vw["w"]})
        return rec


OUTS = ("mu", "var", "dmu", "dvar")


def check(lib, c, name):
    case = ref.Case(*c)
    dev = Device(lib, case)
    first = None
    for ld in case.leading_dims():
        rec = dev.call(case.T, ld)
        for key in OUTS:
            assert np.all(np.isfinite(rec[key])), "%s: NaN or sentinel in %s with ld = %d: a read outside the contract" % (
                ref.case_id(c), key, ld)
        assert same_bits(rec["u"], np.full(case.m, SENTINEL)) and same_bits(rec["du"], np.full((case.m, case.D), SENTINEL)), \
            "APGP_UTIL_NONE wrote u or du"
        if first is None:
            first = rec
        else:
            for key in OUTS + ("v",):
                assert same_bits(rec[key], first[key]), "%s: the leading dimension changed a bit of %s" % (ref.case_id(c), key)
    r = ref.judge(case, first)
    for key, val in r.items():
        if val > WORST.get((name, key), (-1.0, None))[0]:
            WORST[name, key] = (val, ref.case_id(c))
    extra = ""
    if case.route == "inverse" and case.n <= 65 and case.order is None:
        bits = kr.restate(case.T, case.X, case.k, site="cross")
        extra = "  kbuf with site cross's bits: %d of %d" % (int((bits.view(np.int64) == np.ascontiguousarray(
            first["k"][:, :case.n]).view(np.int64)).sum()), bits.size)
    print("%s %s: %s%s" % (name, ref.case_id(c), "  ".join("%s %.3f" % kv for kv in sorted(r.items())), extra))
    assert max(r.values()) <= 1.0, r


CASES = ref.budget_cases()


@pytest.mark.parametrize("c", CASES["inverse_n"], ids=ref.case_id)
def test_inverse_route_n(lib_loaded, c):
    check(lib_loaded, c, "inverse_n")


@pytest.mark.parametrize("c", CASES["inverse_m"], ids=ref.case_id)
def test_inverse_route_m(lib_loaded, c):
    check(lib_loaded, c, "inverse_m")


@pytest.mark.parametrize("c", CASES["solve_n"], ids=ref.case_id)
def test_solve_route_n(lib_loaded, c):
    check(lib_loaded, c, "solve_n")


@pytest.mark.parametrize("c", CASES["solve_m"], ids=ref.case_id)
def test_solve_route_m(lib_loaded, c):
    check(lib_loaded, c, "solve_m")


@pytest.mark.parametrize("c", CASES["dims"], ids=ref.case_id)
def test_dimensions(lib_loaded, c):
    check(lib_loaded, c, "dims")


@pytest.mark.parametrize("c", CASES["linear"], ids=ref.case_id)
def test_linear_term(lib_loaded, c):
    check(lib_loaded, c, "linear")


@pytest.mark.parametrize("kind", sorted(ref.UTIL_KINDS))
@pytest.mark.parametrize("route", ["inverse", "solve"])
def test_utilities(lib_loaded, route, kind):
    case = ref.Case(ref.UTIL_N, ref.UTIL_D, ref.UTIL_M, route, util=True)
    dev = Device(lib_loaded, case)
    zeta, ybest = ref.UTIL_ZETA, ref.UTIL_YBEST
    rec = dev.call(case.T, case.leading_dims()[0], kind=ref.UTIL_KINDS[kind], box=(case.lo, case.hi))
    plain = dev.call(case.T, case.leading_dims()[1], box=(case.lo, case.hi))
    mu, var, dmu, dvar, u, du = (rec[key] for key in OUTS + ("u", "du"))
    inside, judged = ref.util_rows(case, var)
    for key in OUTS:
        assert same_bits(rec[key], plain[key]), "the utility or the leading dimension changed a bit of %s" % key
    # the header's non-finite table: outside the box, and sigma^2 <= 0 inside it
    out = ~inside
    assert out.sum() == ref.UTIL_OUT
    assert np.all(np.isnan(mu[out])) and np.all(np.isnan(var[out])) and np.all(np.isnan(dmu[out])) and np.all(np.isnan(dvar[out]))
    assert np.all(np.isposinf(u[out])) and np.all(du[out] == 0.0)
    for key in OUTS:
        assert np.all(np.isfinite(rec[key][inside])), "NaN in %s of an in-box row: a read outside the contract" % key
    flat = inside & ~judged
    assert flat.sum() >= 1 and (out.sum() + flat.sum()) <= ref.UTIL_CAP * case.m
    if kind == "agp":
        assert np.all(np.isnan(u[flat])) and np.all(np.isnan(du[flat]))
    elif kind == "bape":
        assert np.all(np.isposinf(u[flat])) and np.all(du[flat] == 0.0)
    elif kind == "jones":
        assert np.all(u[flat] == 0.0) and np.all(du[flat] == 0.0)
    # the finish stage on this case too (its in-box rows)
    case.rows = np.nonzero(inside)[0]
    r = ref.judge(case, rec)
    # the value and the chain rule on the judged rows
    if kind == "negmean":
        assert same_bits(u[inside], -mu[inside]) and same_bits(du[inside], -dmu[inside])
        r["u"] = r["du"] = 0.0
    else:
        classes, ru = util_ref.judge_all(kind, u[judged], mu[judged], var[judged], zeta, ybest)
        assert set(classes) == {"value"}
        r["u"] = float(ru.max())
        r["du"] = float(ref.du_ratio(kind, du[judged], mu[judged], var[judged], dmu[judged], dvar[judged], zeta, ybest).max())
    for key, val in r.items():
        if val > WORST.get(("utility", key), (-1.0, None))[0]:
            WORST["utility", key] = (val, "%s-%s" % (route, kind))
    print("utility %s %s (%d rows judged, %d flat, %d outside): %s" % (route, kind, judged.sum(), flat.sum(), out.sum(),
                                                                     "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    assert max(r.values()) <= 1.0, r


def test_chunk_boundary_rows_have_the_bits_of_their_own_calls(lib_loaded):
    """n = 65, m = 4100: pg_chunk gives 4096, the last four rows are a second chunk of single points.  Rows 4088 .. 4099
    -- the last full block of the first chunk and the whole second -- against the same twelve rows as a batch of their
    own (a block of eight and four single points) and against twelve calls of one row."""
    m = 4100
    assert ref.chunk(m, 65) == 4096
    case = ref.Case(65, 3, m, "inverse")
    dev = Device(lib_loaded, case)
    ld = case.leading_dims()[0]
    keys = OUTS + ("u", "du")
    whole = dev.call(case.T, ld, kind=ref.UTIL_KINDS["bape"], keep_work=False)
    for key in keys:
        assert not np.any(whole[key] == SENTINEL), key
    tail = slice(4088, 4100)
    batch = dev.call(case.T[tail], ld, kind=ref.UTIL_KINDS["bape"], keep_work=False)
    for key in keys:
        assert same_bits(whole[key][tail], batch[key]), "rows 4088 .. 4099 of the call differ from their own batch in %s" % key
    for i in range(4088, 4100):
        one = dev.call(case.T[i:i + 1], ld, kind=ref.UTIL_KINDS["bape"], keep_work=False)
        for key in keys:
            assert same_bits(whole[key][i:i + 1], one[key]), "row %d of the call differs from its own call in %s" % (i, key)


def test_worst_ratios_summary():
    """Prints what docs/experiments.md records (pytest -s); asserts nothing new."""
    for (name, key), (val, where) in sorted(WORST.items()):
        print("worst %-10s %-9s %.3f at %s" % (name, key, val, where))
    assert all(v[0] <= 1.0 for v in WORST.values())
