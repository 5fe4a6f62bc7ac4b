# -*- coding: utf-8 -*-
"""MI355X: the two large-n evaluators of the restarted Nelder-Mead search (csrc/nmsearch.hip: FORM 1, nm_kstar +
nm_quad_inverse through the dense inverse at n > 256; FORM 2, nm_kstar + nm_quad_solve through the factor) through the C
ABI, each handed the bits it is judged on, against tests/nm_eval_ref.py: a long-double truth of (mu, sigma^2) and budgets
counted off the kernel source, not fitted to device output (tests/test_nm_eval_ref.py holds NumPy / SciPy and the
restated device order to the same bars on the same inputs, and shows that the bars catch the mutants).

apgp_nm_search is called with maxfev = 1, a trace and one restart per candidate: record 0 of restart r is then
(x, mu, var, u) at candidate r, and all 131 candidates of a case go in one launch of 131 workgroups.  The kind is
APGP_UTIL_NEG_MEAN, so that a planted W that is not an inverse cannot produce a NaN utility.  Per case: mu and var within
budget, the traced x with the bits of the start, u with the bits of -mu, (x_out, f_out, stats) = (start, u, 1, 1, 1),
every input unchanged, the sentinel tails of `work` and of the trace intact, and the same bits from a second call on the
used `work`.

Worst figures are printed (pytest -s) and recorded in docs/experiments.md."""
import ctypes

import numpy as np
import pytest

import nm_eval_ref as ne

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300
TAIL = 64


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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def search(lib, form, A, ld, X, alpha, k, mean, starts, maxfev=1, lo=None, hi=None):
    """One apgp_nm_search call, twice.  Returns (trace (R, maxfev, D + 3), x_out, f_out, stats, work (R, wstride)) after
    the checks every case shares: inputs unchanged, sentinel tails intact, the second call's bits the first's."""
    import torch
    from approxposterior_amd import _lib
    n, D = X.shape
    R = len(starts)
    ks = _ks(k)
    xs = _full((int(lib.apgp_packed_train_len(n, D)),))
    Xd, ad = _dev(X), _dev(alpha)
    rc = lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs.data_ptr(), None)
    assert rc == 0, ("apgp_pack_train", rc, lib.apgp_last_error())
    torch.cuda.synchronize()
    xs0 = xs.cpu().numpy()
    P = ne.panel(A, ld, np.nan if form == "inverse" else SENTINEL)
    Pd, Sd = _dev(P), _dev(starts)
    wlen = int(lib.apgp_nm_search_work_len(R, n))
    assert wlen == R * ((n + 63) // 64 * 64)
    work = _full((wlen + TAIL,))
    opt = _lib.NmOptions(kind=_lib.UTIL_NEG_MEAN, maxiter=1, maxfev=maxfev, reserved=0, zeta=0.01, ybest=0.0, xatol=1e-4,
                         fatol=1e-4, rho=1.0, chi=2.0, psi=0.5, sigma=0.5)
    box = [None, None]
    if lo is not None:
        box = [(ctypes.c_double * _lib.MAX_DIM)(*(list(v) + [0.0] * (_lib.MAX_DIM - len(v)))) for v in (lo, hi)]
    inv = (Pd.data_ptr(), ld, None, 0) if form == "inverse" else (None, 0, Pd.data_ptr(), ld)
    tlen = R * maxfev * (D + 3)
    got = []
    for _ in range(2):
        trace, x_out, f_out = _full((tlen + TAIL,)), _full((R * D + TAIL,)), _full((R + TAIL,))
        stats = torch.full((3 * R + TAIL,), -7, dtype=torch.int32, device="cuda:0")
        rc = lib.apgp_nm_search(Sd.data_ptr(), R, xs.data_ptr(), n, ctypes.byref(ks), mean, *inv, box[0], box[1],
                                ctypes.byref(opt), x_out.data_ptr(), f_out.data_ptr(), stats.data_ptr(),
                                trace.data_ptr(), None, work.data_ptr(), None)
        assert rc == 0, ("apgp_nm_search", rc, lib.apgp_last_error())
        torch.cuda.synchronize()
        got.append([t.cpu().numpy() for t in (trace, x_out, f_out, stats, work)])
    for tr, xo, fo, st, wk in got:
        assert same_bits(tr[tlen:], np.full(TAIL, SENTINEL)), "written past the trace"
        assert same_bits(xo[R * D:], np.full(TAIL, SENTINEL)) and same_bits(fo[R:], np.full(TAIL, SENTINEL))
        assert np.all(st[3 * R:] == -7), "written past stats"
        assert same_bits(wk[wlen:], np.full(TAIL, SENTINEL)), "written past the work slices"
    assert same_bits(Sd.cpu().numpy(), starts) and same_bits(xs.cpu().numpy(), xs0), "an input was written"
    assert np.array_equal(Pd.cpu().numpy().view(np.int64), P.view(np.int64)), "the operand was written"
    a, b = got
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and np.array_equal(a[3], b[3]), \
        "a second identical call changed a bit"
    tr, xo, fo, st, wk = a
    return (tr[:tlen].reshape(R, maxfev, D + 3), xo[:R * D].reshape(R, D), fo[:R], st[:3 * R].reshape(R, 3),
            wk[:wlen].reshape(R, -1))


_SEEN = {}


def one_evaluation(lib, form, n, D, order, family, ld, box=False):
    """A case through one launch; returns the worst (mu, var) ratios.  A case that runs with two leading dimensions
    must give the same bits with both."""
    (X, alpha, T, k, mean), A, truth = ne.truth(form, n, D, order, family)
    lo, hi = ne.box_of(T) if box else (None, None)
    rec, x_out, f_out, stats, work = search(lib, form, A, ld, X, alpha, k, mean, T, lo=lo, hi=hi)
    rec = rec[:, 0]
    mu, var, u = rec[:, D], rec[:, D + 1], rec[:, D + 2]
    inside = np.ones(len(T), dtype=bool) if not box else ~((T < lo) | (T > hi)).any(1)
    assert same_bits(rec[:, :D], T), "the traced x is not the start"
    assert same_bits(x_out, T), "x_out is not the start"
    assert np.all(np.isnan(mu[~inside])) and np.all(np.isnan(var[~inside])) and np.all(np.isposinf(u[~inside]))
    assert np.all(np.isfinite(mu[inside])) and np.all(np.isfinite(var[inside])), "a read outside the contract"
    assert same_bits(u[inside], -mu[inside]), "u is not -mu"
    assert same_bits(f_out, u)
    assert np.all(stats == 1), "stats is not (nfev 1, nit 1, status 1)"
    if box:
        assert len(T) // 4 <= int((~inside).sum()) <= len(T) // 2
        assert np.all(work[~inside].view(np.int64) == np.float64(SENTINEL).view(np.int64)), "a refused point was evaluated"
    if not box:
        first = _SEEN.setdefault((form, n, D, order, family), (mu, var))
        assert same_bits(first[0], mu) and same_bits(first[1], var), "the leading dimension changed a bit"
    rm, rv = truth.ratios(mu, var, inside)
    print("nm %-7s %-7s n=%-3d ld=%-3d D=%-2d P=%-4s%s worst |mu - truth| / budget %.3f, |var - truth| / budget %.3f"
          % (form, family, n, ld, D, order, " box" if box else "", rm, rv))
    assert rm <= 1.0, (form, n, D, order, rm)
    assert rv <= 1.0, (form, n, D, order, rv)
    return rm, rv


F1 = [c + (ld,) for c in ne.cases("inverse") for ld in (ne.ldw_of(c[0]) if c[1:3] == (ne.D_N, None) else ne.ldw_of(c[0])[:1])]
F2 = [c + (ld,) for c in ne.cases("solve") for ld in (ne.ldl_of(c[0]) if c[1:] == (ne.D_N, None, "planted") else ne.ldl_of(c[0])[:1])]


@pytest.mark.parametrize("n,D,order,family,ldw", F1, ids=["n%d-D%d-P%s-%s-ldw%d" % c for c in F1])
def test_form1_within_budget(lib_loaded, n, D, order, family, ldw):
    """The planted W (it need not be an inverse), NaN strictly above the diagonal and in the padding columns: a NaN
    result is a read outside the contract.  n beside the 64-lane stride (319 / 320 / 321), the 4-wavefront stride
    (n mod 4 = 1, 3, 0, 1, 1) and the 256-thread stride (257, 513)."""
    assert n > 256 and ldw >= n and ldw % 2 == 0
    one_evaluation(lib_loaded, "inverse", n, D, order, family, ldw)


@pytest.mark.parametrize("n,D,order,family,ldl", F2, ids=["n%d-D%d-P%s-%s-ldl%d" % c for c in F2])
def test_form2_within_budget(lib_loaded, n, D, order, family, ldl):
    """The planted factor, and the ill-conditioned one with a long-double |L^-1| for the bound, with a sentinel above
    the diagonal and in the padding: one row, one ragged block, a full block, one row past it, two blocks and a ragged
    fifth."""
    one_evaluation(lib_loaded, "solve", n, D, order, family, ldl)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_box_refuses_without_evaluating(lib_loaded, form):
    """About a third of the candidates outside lo / hi: mu = var = NaN, u = +inf, and the restart's slice of `work`
    keeps its sentinel; the others are within budget."""
    n = ne.BOX_N[form]
    ld = ne.ldw_of(n)[0] if form == "inverse" else n
    one_evaluation(lib_loaded, form, n, ne.D_N, None, "planted", ld, box=True)


def test_form2_no_state_carried_between_evaluations(lib_loaded):
    """One restart, maxfev = D + 1, n = 65 (a ragged second block): the D + 1 vertices of the first simplex, whose k*
    differ strongly, are evaluated one after the other in the same slice of `work`, which the substitution solves in
    place.  Every record is within budget: an r[] entry carried over from the evaluation before would not be."""
    X, alpha, V, k, mean, start = ne.stale_case()
    n, D = X.shape
    L, _ = ne.operand("solve", n)
    rec, x_out, f_out, stats, _ = search(lib_loaded, "solve", L, n, X, alpha, k, mean, start[None, :], maxfev=D + 1)
    rec = rec[0]
    assert same_bits(rec[:, :D], V), "the traced points are not the first simplex"
    mu, var, u = rec[:, D], rec[:, D + 1], rec[:, D + 2]
    assert same_bits(u, -mu)
    truth = ne.Truth(L, X, alpha, V, k, mean, form="solve")
    rm = truth.mu_ratio(mu)
    rv = truth.var_ratio(var)
    print("nm solve stale-state n=%d D=%d: worst |mu - truth| / budget %.3f, |var - truth| / budget %.3f over %d records"
          % (n, D, rm.max(), rv.max(), len(V)))
    assert rm.max() <= 1.0 and rv.max() <= 1.0, (rm, rv)
    best = int(np.argmin(u))
    assert same_bits(x_out[0], V[best]) and same_bits(f_out, u[best:best + 1])
    assert stats.tolist() == [[D + 1, 1, 1]]
