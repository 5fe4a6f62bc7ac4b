# -*- coding: utf-8 -*-
"""Reference of the appended-row factor chain -- GP._try_extend's apgp_kernel_cross + apgp_trsv (or apgp_winv_apply on the
parent's resident W = L^-1) + apgp_append_diag per new row and one apgp_fit_summary at the end -- with CONDITION-FREE
error budgets.  Plain NumPy (long double), on top of tests/factor_ref.py and tests/sweep_ref.py: no GPU, no library import.

Every bound is a rounding count read off csrc/linalg.hip times u = 2^-53 times a sum of absolute terms; none contains
cond(K), and none was fitted to device output.

row          The appended row j solves L[:j, :j] l = k(x_j, X[:j]) by forward substitution: apgp_trsv with n = j, the
    store's leading dimension, shift 0, trans 0, the solution written into row j of the same buffer (the kernels read
    rows < j only).  It is the call factor_ref's C_TRSV = 3 was counted for (trsv_kernel below j = 256, the persistent
    kernel from there on), so ``row_ratio`` is ``factor_ref.trsv_ratio`` unchanged:
    |L l - k|_i <= u ((i + 1 + C_TRSV) (|L||l|)_i + |k_i|).
pivot        append_diag_kernel: ``d2 = kdiag - *ss`` is ONE subtraction (relative error delta_1), ``*ljj = sqrt(d2)`` ONE
    correctly rounded square root (IEEE: the library is built without fast-math; relative error delta_2) that enters the
    comparison squared: d^2 = (kdiag - ss)(1 + delta_1)(1 + delta_2)^2, three factors: C_PIV = 3 (confirmed against the
    source: the kernel has no other arithmetic).  *ss is not l.l but the device's reduction of it, within factor_ref's
    ``sumsq_bound`` B_ss (trsv_kernel's closing loop / the persistent kernel's block sums on the substitution route,
    sumsq_kernel on the W route: one fma, six shuffle levels, 16 partials or one addition per 64-row block):
        |d^2 - (kdiag - l.l)| <= B_ss(l) + C_PIV u d^2.
    kdiag is taken as the bits the host hands over (GP._try_extend forms k(x, x) + diag_add in Python).  A difference
    in the subnormal range is exact and its root is a normal number: the ratio is formed in long double throughout.
W route      The first appended row, when the parent's dense W is resident and trusted, is apgp_winv_apply(W, ldw, n0, k,
    shift 0, trans 0): ``winv_row_ratio`` is ``sweep_ref.winv_apply_ratio`` on the parent panel's own bits:
    |l - W k|_i <= u depth_i (|W||k|)_i, depth_i = ceil((i + 1) / 128) + 8 (sweep_ref.winv_depth).  This is a FORWARD
    bound on the product with the W at hand; how far such a row sits from substitution's backward bound depends on how
    good an inverse W is and is reported, not asserted.
summary      logdet_kernel (apgp_fit_summary, apgp_logdet), one workgroup of 1024 threads: thread t adds log(L_ii) for
    i = t, t + 1024, ...: ceil(n / 1024) additions (the first onto 0.0); six __shfl_xor levels; thread 0 adds the 16
    wavefront partials in order; the closing 2.0 * s is exact.  SUM_DEPTH(n) = ceil(n / 1024) + 6 + 16.
      out[0]  |out[0] - 2 sum log L_ii| <= u (SUM_DEPTH + E_LOG) 2 sum |log L_ii|.  E_LOG = 3: the OpenCL full-profile
              accuracy of double log, 3 ulp, which ROCm's device library implements (it documents 1 ulp for this
              function); the bar counts an ulp as one u of the value, the stricter reading of the two (an ulp is at most
              2 u of it).  Not measured on the code under test.
      out[1], out[2]  fmin / fmax select: the exact bits of the diagonal's min and max.
      out[3]  z.z: one fma per element (the product is not rounded), then the same tree: |out[3] - z.z| <= u SUM_DEPTH
              sum z_i^2 -- factor_ref.sumsq_bound's form with THIS kernel's order (no per-block additions; the strided
              trips counted in full).  0.0 exactly without z.
      out[4]  (double)*info, 0.0 without info.
    Only the n diagonal entries and z are read: the leading dimension and whatever lies off the diagonal cannot matter.

``restate_append`` restates the chain in float64 (factor_ref.trsv_restate per row) and carries the mutants a test of the
chain must catch; tests/test_extend_ref.py holds it to every bar on the inputs the GPU test uses, and every mutant out
of one.  The shape tables at the end are shared by tests/test_extend_ref.py and tests/test_gpu_factor_extend.py.
"""
import math

import numpy as np

import factor_ref as fr
import kvalue_ref as kr
import sweep_ref as sr

U = fr.U
LD = np.longdouble
C_PIV = 3
E_LOG = 3


# ----------------------------------------------------------------------------------------------------------------------
# ratios and bounds
# ----------------------------------------------------------------------------------------------------------------------
def row_ratio(L, l, k):
    """factor_ref.trsv_ratio of the appended row ``l`` (j entries) against the first j rows and columns of ``L`` and the
    right-hand side ``k``: one ratio per entry."""
    j = len(l)
    L = np.asarray(L, dtype=np.float64)
    return fr.trsv_ratio(L[:j, :j], l, np.asarray(k, dtype=np.float64)[:j], 0.0, 0)


def pivot_ratio(d, kdiag, l, ss=None):
    """|d^2 - (kdiag - l.l)| / (B_ss + C_PIV u d^2), in long double.  ``ss``: judge against kdiag - ss instead, for a call
    of apgp_append_diag alone that was handed ``ss`` itself (B_ss = 0 then).  A zero bound demands a zero error; a
    non-finite or non-positive pivot is inf."""
    if not (np.isfinite(d) and d > 0.0):
        return np.inf
    d2 = LD(d) * LD(d)
    if ss is None:
        t, b_ss = fr.sumsq_bound(l)
    else:
        t, b_ss = LD(ss), 0.0
    err = abs(d2 - (LD(kdiag) - t))
    bound = LD(b_ss) + LD(C_PIV * U) * d2
    if err == 0:
        return 0.0
    return float(err / bound) if (np.isfinite(err) and bound > 0) else np.inf


def winv_row_ratio(W_panel, l, k):
    """sweep_ref.winv_apply_ratio (trans 0, shift 0) of the row ``l`` = W k on the bits of the parent's panel
    (n0 rows, leading dimension >= n0; only the lower triangle is used)."""
    n0 = len(l)
    W = np.asarray(W_panel, dtype=np.float64)[:n0, :n0]
    return sr.winv_apply_ratio(W, l, np.asarray(k, dtype=np.float64)[:n0], 0.0, 0)


def sum_depth(n):
    return (n + 1023) // 1024 + 6 + 16


def summary_bounds(L, z=None, info=None):
    """What logdet_kernel may write for the factor ``L`` (n x n, only its diagonal is used): a dict with
    "logdet": (truth in long double, bound), "min" / "max": the exact doubles, "zz": (truth, bound) ((0, 0) without
    z), "info": the info word as a double."""
    dg = np.diag(np.asarray(L, dtype=np.float64)).copy() if np.ndim(L) == 2 else np.asarray(L, dtype=np.float64)
    n = len(dg)
    depth = sum_depth(n)
    lg = np.log(dg.astype(LD))
    out = {"logdet": (2 * lg.sum(), U * (depth + E_LOG) * 2.0 * float(np.abs(lg).sum())),
           "min": float(dg.min()), "max": float(dg.max()),
           "zz": (LD(0), 0.0), "info": float(0 if info is None else int(info))}
    if z is not None:
        t = (np.asarray(z, dtype=np.float64).astype(LD) ** 2).sum()
        out["zz"] = (t, U * depth * float(t))
    return out


def summary_ratios(out5, bounds):
    """{"logdet", "zz": |out - truth| / bound (zero bound: zero error or inf), "exact": True when out[1], out[2] and
    out[4] have exactly the bits they must}."""
    out5 = np.asarray(out5, dtype=np.float64)

    def one(o, tb):
        t, b = tb
        if not np.isfinite(o):
            return np.inf
        e = float(abs(LD(o) - t))
        return 0.0 if e == 0.0 else (np.inf if b == 0.0 else e / b)
    exact = (fr_same_bits(out5[1], bounds["min"]) and fr_same_bits(out5[2], bounds["max"])
             and fr_same_bits(out5[4], bounds["info"]))
    return {"logdet": one(out5[0], bounds["logdet"]), "zz": one(out5[3], bounds["zz"]), "exact": exact}


def fr_same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement of the append, and its mutants
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("cols_minus_1", "no_diag_add", "stale_ss", "drop_last_term", "info_last")


def restate_append(L0, Krows, kdiag, diag_add=0.0, mutant=None):
    """GP._try_extend in float64: ``L0`` (n0 x n0 lower factor), ``Krows[r]`` the cross row k(x_j, X[:j]) of the new row
    j = n0 + r (at least j entries), ``kdiag[r]`` = k(x_j, x_j) + diag_add as the host restates it.  Returns
    (L, info, ss): the (n1 x n1) extended factor, the LAPACK-style info word (0, or the order j + 1 of the FIRST failed
    pivot, which is set to 1.0) and the list of the sums of squares the pivots were formed from.

    Mutants: "cols_minus_1" the row solved against j - 1 columns (the last entry stays the store's zero);
    "no_diag_add" the pivot from k(x, x) alone; "stale_ss" the pivot from the previous row's sum of squares (the first
    new row: the parent's last row's); "drop_last_term" l.l without its last term; "info_last" the info word keeps the
    last failure, not the first."""
    L0 = np.tril(np.asarray(L0, dtype=np.float64))
    n0 = len(L0)
    n1 = n0 + len(Krows)
    L = np.zeros((n1, n1))
    L[:n0, :n0] = L0
    info = 0
    sums = []
    prev_ss = float(L0[n0 - 1, :n0 - 1] @ L0[n0 - 1, :n0 - 1])
    for r, j in enumerate(range(n0, n1)):
        k = np.asarray(Krows[r], dtype=np.float64)[:j]
        if mutant == "cols_minus_1":
            l = np.zeros(j)
            if j > 1:
                l[:j - 1] = fr.trsv_restate(L[:j - 1, :j - 1], k[:j - 1], 0.0, 0)
        else:
            l = fr.trsv_restate(L[:j, :j], k, 0.0, 0)
        L[j, :j] = l
        ss = float(l[:-1] @ l[:-1]) if mutant == "drop_last_term" else float(l @ l)
        used = prev_ss if mutant == "stale_ss" else ss
        prev_ss = ss
        sums.append(used)
        d2 = (kdiag[r] - diag_add if mutant == "no_diag_add" else kdiag[r]) - used
        if d2 > 0.0 and d2 < np.inf:
            L[j, j] = math.sqrt(d2)
        else:
            L[j, j] = 1.0
            if info == 0 or mutant == "info_last":
                info = j + 1
    return L, info, sums


def judge_append(L, n0, Krows, kdiag):
    """Worst (row ratio, pivot ratio) over the appended rows n0 .. of the extended factor ``L`` (device or restated),
    and the worst factor_ref.chol_ratio is left to the caller (it needs the parent's Gram)."""
    wr = wp = 0.0
    for r, j in enumerate(range(n0, len(L))):
        l = L[j, :j]
        wr = max(wr, float(row_ratio(L, l, Krows[r]).max()))
        wp = max(wp, pivot_ratio(L[j, j], kdiag[r], l))
    return wr, wp


# ----------------------------------------------------------------------------------------------------------------------
# shape tables and seeded inputs (shared by tests/test_extend_ref.py and tests/test_gpu_factor_extend.py)
# ----------------------------------------------------------------------------------------------------------------------
# apgp_append_diag alone: (name, kdiag, ss, info before, order, succeeds)
TINY = 2.0 ** -1022
APPEND_DIAG = (
    ("normal", 2.5, 1.25, 0, 7, True),
    ("kdiag == ss", 1.0, 1.0, 0, 8, False),
    ("kdiag < ss", 1.0, 1.0 + 2.0 ** -52, 0, 9, False),
    ("ss NaN", 1.0, float("nan"), 0, 10, False),
    ("kdiag +inf", float("inf"), 1.0, 0, 11, False),
    ("subnormal difference", TINY, TINY - 5 * 2.0 ** -1074, 0, 12, True),
    ("info set, failing", 1.0, 2.0, 5, 13, False),
    ("info set, succeeding", 2.0, 1.0, 5, 14, True),
)
APPEND_DIAG_TWICE = ((1.0, 2.0, 21), (1.0, 3.0, 22))       # two failures on one info word: it keeps order 21

SUMMARY_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def summary_lds(n):
    return (n, n + 3, (n + 63) // 64 * 64 + 64)


def summary_case(n):
    """(L, z): a lower factor whose diagonal spans four decades (logs of both signs) and a z over four decades."""
    rs = np.random.RandomState(4100 + n)
    L = np.tril(rs.normal(size=(n, n)) * 0.05, -1) + np.diag(10.0 ** rs.uniform(-2.0, 2.0, size=n))
    return L, rs.normal(size=n) * 10.0 ** rs.uniform(-2.0, 2.0, size=n)


# name: (n0, n1, D, log white noise, linear order or None).  One GP object per appended row.
#   readme   the README sizes: one store of capacity 128, never grown
#   blocks   crosses the 64- and 128-row block boundaries; the first store (capacity 128) is full at n1 = 129: the one
#            grow-and-copy case (new capacity 256)
#   switch   crosses apgp_trsv's n = 256 switch from one workgroup to the persistent kernel
#   rule     crosses n1 = 512, where the cost rule stops appending two rows at a time
CHAINS = {"readme": (50, 90, 2, -12.0, None), "blocks": (60, 131, 3, math.log(1e-6), None),
          "switch": (254, 258, 5, -12.0, None), "rule": (511, 513, 8, math.log(1e-6), None)}
for _P in kr.LIN_ORDERS:        # a linear term of every order tests/kvalue_ref.py pins for the kernel value (0 .. 3, 16)
    CHAINS["linear%d" % _P] = (65, 70, 3, math.log(1e-6), _P)
LIN_COEF = 0.05
MANY = (100, 164, 165, 2)        # extend_max_rows = 64: 100 -> 164 extends, 100 -> 165 refactorises (D = 2)
W_N0 = (63, 64, 65, 129, 300)    # the W route: parent sizes (two rows appended, D = 3)
STORE_N = 70                     # the store tests' base size (D = 3)
FAIL_METRIC = 1.0                # the failure case's metric: without white noise its Gram must factorise on its own


def points(n, D, seed, width=3.0):
    return np.random.RandomState(seed).uniform(-width, width, size=(n, D))


def chain_case(name):
    """(X, y, metric, log white noise, lin order): n1 seeded points in [-3, 3]^D ([-1.2, 1.2]^D with a linear term: its
    order-16 powers stay below 350), the metric D on every axis, y a smooth function of the points."""
    n0, n1, D, wn, P = CHAINS[name]
    X = points(n1, D, 5000 + 10 * n1 + D + (0 if P is None else 100 + P), 3.0 if P is None else 1.2)
    return X, target(X), np.full(D, float(D)), wn, P


def target(X):
    return np.sin(X).sum(1) + 0.1 * (X ** 2).sum(1)


def host_kernel(X1, X2, metric, P=None):
    """k(x, x') in float64 NumPy (the CPU tests' Gram; the GPU tests take the device's own bits instead)."""
    d2 = (((X1[:, None, :] - X2[None, :, :]) ** 2) / metric).sum(-1)
    k = np.exp(-0.5 * d2)
    if P is not None:
        k = k + LIN_COEF * ((X1[:, None, :] * X2[None, :, :]) ** P).sum(-1)
    return k


def failure_case():
    """(X, y): STORE_N + 1 base points (D = 3) and four more rows, the second and the fourth a copy of X[0].  With no
    white noise (e^-800 underflows to 0) and unit amplitude L[0, 0] = 1 and L[i, 0] = K_i0 exactly, so a copy of X[0]
    solves to l = (1, 0, ..., 0) EXACTLY, l.l = 1 = k(x, x) and the pivot's difference is an exact zero: a failure in
    any arithmetic, at orders n0 + 2 and n0 + 4 (the failed row is (1, 0, ..., 0 | 1), so the second copy fails too)."""
    base = points(STORE_N + 1, 3, 7700)
    extra = points(4, 3, 7701)
    extra[1] = base[0]
    extra[3] = base[0]
    X = np.vstack([base, extra])
    return X, target(X)
