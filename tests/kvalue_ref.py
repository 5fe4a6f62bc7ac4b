# -*- coding: utf-8 -*-
"""Reference of ONE kernel value k(x, x') as csrc/apgp_common.h evaluates it.  Plain Python (mpmath, NumPy): no GPU, no
library import.

    k(x, x') = amp exp(-1/2 sum_d inv_metric_d (x_d - x'_d)^2) + lin_coef sum_d (x_d x'_d)^P   [+ diag_add on K_ii]

``truth``    the exact value of the fp64 inputs and hyper-parameters, mpmath at DPS digits (one entry at a time).
``truth_ld`` the same for whole matrices in numpy.longdouble: the exponent argument and the linear sum are formed in
             double-double (error-free transformations, ~2^-100), the exponential too (``_dd_exp_neg``), and the
             sum is rounded once to long double: 2^-11 ulp of a double even where a negative linear term cancels
             against the exponential part; <= 2^-9 ulp is what tests/test_kvalue_ref.py asserts against ``truth``.
``budget``   a per-entry bound of |device value - truth| for the fp64 operation sequence below (derivation beside it).
``restate``  the device arithmetic operation by operation with an exactly rounded fma; its switches (``mutant``) are
             the defects the budget has to catch.

The device's operation sequence (apgp_make_kernconst, the x * sc at load time, apgp_gram_value, apgp_exp):

    sc_d = sqrt(0.5 inv_metric_d)      lw_d = 2 / inv_metric_d             (host, once)
    xs_d = x_d sc_d                    padded coordinates: xs = 0          (at load time)
    s  = fma(df_d, df_d, s)  for even d,  s3 likewise for odd d,  df_d = xs_d - xs'_d
    e  = apgp_exp(-(s + s3))           clamp to [-700, 700], 32-entry table, degree-6 polynomial
    k  = amp e
    k  = fma(lin_coef, ls, k)          ls = sum_d q_d, q_d = p_d^P by repeated products, p_d = (xs_d xs'_d) lw_d
    k  = k + diag_add                  on the diagonal of the Gram matrix only

Budget, term by term (u = 2^-53; ulp(v) = the spacing of doubles at |v|; everything first order, the argument part
carries a factor 1 + 2^-20 for the second order).  A rounding that is EXACT for the inputs at hand is not charged: the
error-free transformations (two_sum, two_prod) say so, which is what makes the bound collapse on a lattice of dyadic
points and keeps a loosened budget from hiding there.

  sc      sqrt rounds once (0.5 inv_metric is exact): a relative error <= u COMMON to xs and xs', i.e. relative in df,
          2 u df_d^2 in the argument.  Not charged when sc_d^2 == 0.5 inv_metric_d exactly.
  xs      x sc rounds once, independently for the two points: |xs_d| u and |xs'_d| u in df_d, i.e.
          2 |df_d| (|xs_d| + |xs'_d|) u in the argument -- the cancellation term: two distant-from-origin points that
          are close to each other lose the low bits of their difference.  Not charged per point when x sc is exact.
  df      the subtraction rounds once (exact by Sterbenz for nearby points): 2 u df_d^2.
  sums    each lane does one rounded fma per coordinate pair and s + s3 rounds once: at most D + 1 roundings for
          every D (ceil(dpad / 2) + 1 <= D + 1), each at most u times the final sum S.  Counted from the first
          inexact step of a lane on; zero when every partial sum is exact.
  An error da in the argument is a relative error expm1(da) ~ da in k: for distant points (S ~ 700) the budget is
  loose by the factor S, inherent to fp64.
  exp     E_EXP ulp(e), e = exp(-S), times amp.  E_EXP = 1.5: the CPU restatement's worst case is 1.017 ulp
          (docs/experiments.md).  Coincident points (every coordinate the same bits) have df = 0, r = 0, table entry 0
          = 1.0 and e = 1 exactly by construction: not charged.
  amp *   one rounding: 1/2 ulp(amp e).  Coincident points: exact.
  linear  lw rounds once, sc^2 lw = 1 up to 3 u, the two xs 2 u, the two products 2 u: p_d within 7 u; q_d = p_d^P adds
          P - 1 products: (8 P - 1) u; the D additions at most u sum|q| each; lin_coef sum|q| ((8 P - 1) + D) u.
          A contracted variant of the same expression (fma in place of product and sum) has fewer roundings, and the
          raw form (x x')^P has fewer still: the term holds for them.  P = 0: ls = D exactly.
          The closing fma rounds once: 1/2 ulp(k).
  diag    one rounding: 1/2 ulp(k + diag_add).
  clamp   below -700 the device returns amp exp(-700) ~ amp 9.9e-305 for a true value under it: amp 1e-304 is added
          whenever the argument, with its error, can reach 700.
  floor   2^-1074: below the normal range the relative model ends (amp e can be subnormal for a small amp).
"""
import collections
import math
import struct

import mpmath as mp
import numpy as np

DPS = 60
U = 2.0 ** -53
E_EXP = 1.5
SITES = ("gram", "cross", "mean", "sweep")
MUTANTS = ("no_720", "no_ln2lo", "tab4", "skip_last_odd", "pad_nonzero", "transpose")

Kern = collections.namedtuple("Kern", "ndim amp diag_add inv_metric lin_coef lin_order")


def kern(inv_metric, amp=1.0, diag_add=0.0, lin_coef=0.0, lin_order=1):
    im = np.ascontiguousarray(inv_metric, dtype=np.float64)
    return Kern(len(im), float(amp), float(diag_add), im, float(lin_coef), int(lin_order))


def dpad(d):
    return 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def ulp(v):
    """Spacing of the doubles at |v| (2^-1074 below the normal range); array in, array out."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(v, 2.0 ** -1022)))
    # (log2 of a double just below a power of two may round up to it: step back where 2^e > v)
    e = np.where(np.ldexp(1.0, e.astype(np.int64)) > np.maximum(v, 2.0 ** -1022), e - 1, e)
    return np.ldexp(1.0, (e - 52).astype(np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# truth
# ----------------------------------------------------------------------------------------------------------------------
def truth1(x, xp, k, diagonal=False):
    """One exact value (mpf): x, xp are rows of fp64 numbers."""
    with mp.workdps(DPS):
        s = mp.mpf(0)
        ls = mp.mpf(0)
        for d in range(k.ndim):
            a, b = mp.mpf(float(x[d])), mp.mpf(float(xp[d]))
            s += mp.mpf(float(k.inv_metric[d])) * (a - b) ** 2
            ls += (a * b) ** k.lin_order
        v = mp.mpf(k.amp) * mp.exp(-s / 2)
        if k.lin_coef != 0.0:
            v += mp.mpf(k.lin_coef) * ls
        if diagonal:
            v += mp.mpf(k.diag_add)
        return v


def truth(X1, X2, k, pairs=None):
    """Exact values as a dict {(i, j): mpf}.  X2 None: the Gram matrix of X1 (diag_add on i == j), lower triangle.
    ``pairs``: only those entries."""
    X1 = np.atleast_2d(X1)
    gram = X2 is None
    X2 = X1 if gram else np.atleast_2d(X2)
    if pairs is None:
        pairs = [(i, j) for i in range(len(X1)) for j in range(i + 1 if gram else len(X2))]
    return {(i, j): truth1(X1[i], X2[j], k, gram and i == j) for i, j in pairs}


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    e = e + (a[1] + b[1])
    h = s + e
    return h, e - (h - s)


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    e = e + (a[0] * b[1] + a[1] * b[0])
    h = p + e
    return h, e - (h - p)


def _dd_const(x):
    h = float(x)
    return h, float(x - mp.mpf(h))


with mp.workdps(DPS):
    _LN2_DD = _dd_const(mp.log(2))
    _INVFACT_DD = [_dd_const(mp.mpf(1) / mp.factorial(i)) for i in range(11)]


def _dd_exp_neg(S):
    """exp(-S) for a double-double S >= 0 (arrays), as a double-double good to ~2^-95: -S = kk ln2 + r, expm1(r / 512)
    by its Taylor series to the 10th power, nine doublings (1 + p)^2 - 1 = 2 p + p^2; returned as (e, kk) with
    exp(-S) = e 2^kk, the scaling left to the caller (the low word would fall below the normal range for S > 660).
    S is cut at 11000 (2^-15870: inside long double's range and nothing against the smallest double)."""
    big = S[0] > 11000.0
    h = (-np.where(big, 11000.0, S[0]), -np.where(big, 0.0, S[1]))
    kk = np.rint(h[0] / _LN2_DD[0])
    r = _dd_add(h, _dd_mul((-kk, np.zeros_like(kk)), _LN2_DD))
    m = (r[0] / 512.0, r[1] / 512.0)
    p = (np.full_like(kk, _INVFACT_DD[10][0]), np.full_like(kk, _INVFACT_DD[10][1]))
    for i in range(9, 0, -1):
        p = _dd_add(_dd_mul(p, m), _INVFACT_DD[i])
    p = _dd_mul(p, m)
    for _ in range(9):
        p = _dd_add((2.0 * p[0], 2.0 * p[1]), _dd_mul(p, p))
    e = _dd_add(p, (1.0, 0.0))
    return e, kk.astype(np.int64)


def truth_ld(X1, X2, k):
    """The whole matrix in numpy.longdouble (m x n; X2 None: the full symmetric Gram matrix with diag_add)."""
    X1 = np.ascontiguousarray(np.atleast_2d(X1), dtype=np.float64)
    gram = X2 is None
    X2 = X1 if gram else np.ascontiguousarray(np.atleast_2d(X2), dtype=np.float64)
    if np.finfo(np.longdouble).nmant < 63:       # no 80-bit type on this host: entry by entry
        t = truth(X1, X2 if not gram else None, k, [(i, j) for i in range(len(X1)) for j in range(len(X2))])
        return np.array([[float(t[i, j]) for j in range(len(X2))] for i in range(len(X1))], dtype=np.longdouble)
    shape = (len(X1), len(X2))
    S = (np.zeros(shape), np.zeros(shape))
    L = (np.zeros(shape), np.zeros(shape))
    with np.errstate(all="ignore"):
        for d in range(k.ndim):
            a, b = X1[:, d][:, None], X2[:, d][None, :]
            df = _two_sum(a, -b)                                        # exact
            t = _dd_mul(df, df)
            half = 0.5 * k.inv_metric[d]
            S = _dd_add(S, _dd_mul(t, (half, 0.0)))
            if k.lin_coef != 0.0 and k.lin_order >= 1:
                p = _two_prod(a, b)                                     # exact
                q = p
                for _ in range(1, k.lin_order):
                    q = _dd_mul(q, p)
                L = _dd_add(L, q)
        e, kk = _dd_exp_neg(S)
        e = _dd_mul(e, (k.amp, 0.0))
        deep = kk < -900                                                # scaled in long double's exponent range instead
        small = np.ldexp(e[0].astype(np.longdouble) + e[1].astype(np.longdouble), kk)
        kk = np.where(deep, -2000, kk)
        v = (np.ldexp(e[0], kk), np.ldexp(e[1], kk))
        if k.lin_coef != 0.0:
            if k.lin_order == 0:
                L = (np.full(shape, float(k.ndim)), np.zeros(shape))
            v = _dd_add(v, _dd_mul(L, (k.lin_coef, 0.0)))
        if gram and k.diag_add != 0.0:
            v = _dd_add(v, (np.diag(np.full(len(X1), k.diag_add)), np.zeros(shape)))
    return (v[0].astype(np.longdouble) + v[1].astype(np.longdouble)) + np.where(deep, small, np.longdouble(0.0))


# ----------------------------------------------------------------------------------------------------------------------
# budget
# ----------------------------------------------------------------------------------------------------------------------
def budget(X1, X2, k):
    """Per-entry absolute bound (m x n float64; X2 None: the full symmetric Gram matrix, diagonal with diag_add) of
    |fp64 device value - truth|; the derivation is the module's docstring."""
    X1 = np.ascontiguousarray(np.atleast_2d(X1), dtype=np.float64)
    gram = X2 is None
    X2 = X1 if gram else np.ascontiguousarray(np.atleast_2d(X2), dtype=np.float64)
    m, n, D = len(X1), len(X2), k.ndim
    half = 0.5 * k.inv_metric
    sc = np.sqrt(half)
    p, e = _two_prod(sc, sc)
    e_sc = np.where((p == half) & (e == 0.0), 0.0, U)
    da = np.zeros((m, n))                       # error of the exponent argument
    same = np.ones((m, n), dtype=bool)          # coincident points
    lane = [(np.zeros((m, n)), np.zeros((m, n))), (np.zeros((m, n)), np.zeros((m, n)))]
    dirty = [np.zeros((m, n), dtype=bool), np.zeros((m, n), dtype=bool)]
    cnt = np.zeros((m, n))
    sabs = np.zeros((m, n))                     # sum |q_d| of the linear term
    P = k.lin_order
    with np.errstate(all="ignore"):
        for d in range(D):
            xa, ea = _two_prod(X1[:, d], sc[d])
            xb, eb = _two_prod(X2[:, d], sc[d])
            ra = np.where(ea == 0.0, 0.0, U)[:, None] * np.abs(xa)[:, None]
            rb = np.where(eb == 0.0, 0.0, U)[None, :] * np.abs(xb)[None, :]
            df, edf = _two_sum(xa[:, None], -xb[None, :])
            same &= X1[:, d][:, None] == X2[:, d][None, :]
            da += 2.0 * np.abs(df) * (ra + rb) + df * df * (2.0 * e_sc[d] + np.where(edf == 0.0, 0.0, 2.0 * U))
            # the lane's fma: exact iff df^2 + (partial sum) is a double
            ln = d & 1
            t = _dd_add(lane[ln], _two_prod(df, df))
            dirty[ln] |= t[1] != 0.0
            cnt += dirty[ln]
            lane[ln] = t
            if k.lin_coef != 0.0 and P >= 1:
                sabs += np.abs(X1[:, d][:, None] * X2[:, d][None, :]) ** P
        tot = _dd_add(lane[0], lane[1])
        cnt += dirty[0] | dirty[1] | (tot[1] != 0.0)
        S = tot[0]
        da = (da + cnt * U * S) * (1.0 + 2.0 ** -20)
        e = np.exp(-np.minimum(S, 745.0))
        e_hi = e * np.exp(da)
        b = k.amp * e_hi * np.expm1(da)
        b += np.where(same, 0.0, k.amp * E_EXP * ulp(e_hi) + 0.5 * ulp(k.amp * e_hi))
        b += np.where(S + da >= 700.0, k.amp * 1e-304, 0.0)
        kv = k.amp * e_hi
        if k.lin_coef != 0.0:
            if P >= 1:
                b += k.lin_coef * sabs * ((8 * P - 1) + D) * U * (1.0 + 2.0 ** -20)
                kv = kv + k.lin_coef * sabs
            else:
                kv = kv + k.lin_coef * D
            b += 0.5 * ulp(kv)
        if gram and k.diag_add != 0.0:
            i = np.arange(m)
            b[i, i] += 0.5 * ulp(kv[i, i] + k.diag_add)
        b += 2.0 ** -1074
    return b


# ----------------------------------------------------------------------------------------------------------------------
# restate
# ----------------------------------------------------------------------------------------------------------------------
EXP_TAB_HEX = (
    "0x1.0000000000000p+0", "0x1.059b0d3158574p+0", "0x1.0b5586cf9890fp+0", "0x1.11301d0125b51p+0",
    "0x1.172b83c7d517bp+0", "0x1.1d4873168b9aap+0", "0x1.2387a6e756238p+0", "0x1.29e9df51fdee1p+0",
    "0x1.306fe0a31b715p+0", "0x1.371a7373aa9cbp+0", "0x1.3dea64c123422p+0", "0x1.44e086061892dp+0",
    "0x1.4bfdad5362a27p+0", "0x1.5342b569d4f82p+0", "0x1.5ab07dd485429p+0", "0x1.6247eb03a5585p+0",
    "0x1.6a09e667f3bcdp+0", "0x1.71f75e8ec5f74p+0", "0x1.7a11473eb0187p+0", "0x1.82589994cce13p+0",
    "0x1.8ace5422aa0dbp+0", "0x1.93737b0cdc5e5p+0", "0x1.9c49182a3f090p+0", "0x1.a5503b23e255dp+0",
    "0x1.ae89f995ad3adp+0", "0x1.b7f76f2fb5e47p+0", "0x1.c199bdd85529cp+0", "0x1.cb720dcef9069p+0",
    "0x1.d5818dcfba487p+0", "0x1.dfc97337b9b5fp+0", "0x1.ea4afa2a490dap+0", "0x1.f50765b6e4540p+0")
EXP_TAB = tuple(float.fromhex(h) for h in EXP_TAB_HEX)
_MAGIC = 6755399441055744.0                              # 1.5 * 2^52
_INV = float.fromhex("0x1.71547652b82fep+5")             # 32 / ln2
_LN2HI = -float.fromhex("0x1.62e42fefa39efp-6")
_LN2LO = -float.fromhex("0x1.abc9e3b39803fp-61")
_C6, _C5, _C4, _C3 = 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0
_TAB4 = list(EXP_TAB)
_TAB4[17] = struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", EXP_TAB[17]))[0] + 4))[0]
_TAB4 = tuple(_TAB4)


def fma(a, b, c):
    """round(a b + c) with ONE rounding: the exact rational a b + c as an integer ratio, whose true division CPython
    rounds correctly (to nearest, ties to even).  Finite arguments; a zero result is +0.0 (what IEEE gives unless
    product and addend are both -0.0, which no caller produces)."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def fma_mp(a, b, c):
    """The same through mpmath's exact product and sum (no intermediate rounding at any width), rounded once to 53
    bits: the cross-check of ``fma``."""
    return float(mp.fadd(mp.fmul(mp.mpf(a), mp.mpf(b), exact=True), mp.mpf(c), exact=True))


def exp_restate(x, mutant=None):
    """apgp_exp, operation by operation (Python floats are IEEE doubles; +, -, * round once)."""
    if x != x:
        x = -700.0                                       # fmax(NaN, -700) = -700: the clamp swallows NaN
    x = min(max(x, -700.0), 700.0)
    t = fma(x, _INV, _MAGIC)
    kf = t - _MAGIC
    j = struct.unpack("<i", struct.pack("<d", t)[:4])[0]          # __double2loint
    r = fma(kf, _LN2HI, x)
    if mutant != "no_ln2lo":
        r = fma(kf, _LN2LO, r)
    p = _C5 if mutant == "no_720" else fma(r, _C6, _C5)
    p = fma(r, p, _C4)
    p = fma(r, p, _C3)
    p = fma(r, p, 0.5)
    p = fma(r * r, p, r)
    T = (_TAB4 if mutant == "tab4" else EXP_TAB)[j & 31]
    res = fma(T, p, T)
    return math.ldexp(res, j >> 5)                       # the exponent-field addition (normal range: j >> 5 >= -1010)


def kernconst(k):
    """apgp_make_kernconst: (sc, lw) as lists of length dpad, zero past ndim."""
    dp = dpad(k.ndim)
    sc = [math.sqrt(0.5 * float(k.inv_metric[d])) if d < k.ndim else 0.0 for d in range(dp)]
    lw = [2.0 / float(k.inv_metric[d]) if d < k.ndim else 0.0 for d in range(dp)]
    return sc, lw


def _scaled(X, sc, D, dp, mutant):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if mutant == "transpose":
        X = np.ascontiguousarray(X.T).reshape(X.shape)   # element (i, d) read at flat index d n + i
    rows = []
    for i in range(len(X)):
        rows.append([float(X[i, d]) * sc[d] if d < D else 0.0 for d in range(dp)])
    return rows


def value_restate(xi, xc, k, lw, diagonal, mutant=None, fuse_sc=None):
    """apgp_gram_value on two rows of scaled coordinates (contraction off: every product and sum rounds).
    ``fuse_sc``: xi holds RAW coordinates and its scaling is contracted into the subtraction, df = fma(x, sc, -xc)
    (site "sweep", fused)."""
    dp = len(xi)
    s = s3 = 0.0
    for d in range(0, dp, 2):
        if fuse_sc is not None:
            df0 = fma(xi[d], fuse_sc[d], -xc[d])
            df1 = fma(xi[d + 1], fuse_sc[d + 1], -xc[d + 1])
        else:
            df0 = xi[d] - xc[d]
            df1 = xi[d + 1] - xc[d + 1]
        if mutant == "skip_last_odd" and (k.ndim & 1):
            if d == k.ndim - 1:
                df0 = 0.0
        s = fma(df0, df0, s)
        s3 = fma(df1, df1, s3)
    v = k.amp * exp_restate(-(s + s3), mutant)
    if k.lin_coef != 0.0:
        if k.lin_order == 0:
            ls = float(k.ndim)
        else:
            ls = 0.0
            for d in range(dp):
                p = (xi[d] * xc[d]) * lw[d]
                q = p
                for _ in range(1, k.lin_order):
                    q *= p
                ls += q
        v = fma(k.lin_coef, ls, v)
    if diagonal:
        v = v + k.diag_add
    return v


def restate(X1, X2, k, site="gram", mutant=None, pairs=None, fused=False):
    """The device's values as an m x n float64 array (NaN where not evaluated).  ``site``: "gram" (X2 None; lower
    triangle, diag_add on the diagonal), "cross" (apgp_kernel_cross: no diagonal term) or "mean" (the k* of
    predict_mean_kernel: the same arithmetic for the squared-exponential kernel; with a linear term the device kernel
    is compiled with contraction allowed, so there the restatement is the Gram association, not a promise).
    "sweep": the k*(t, x) of sweep2_kernel's produce_b, X1 the candidates, pure squared-exponential kernels only.  The
    kernel is compiled with contraction allowed and holds the scaled candidate tt = t sc in registers: in the
    steady-state loop tt is a rounded product and the value has "cross"'s bits (``fused`` False); where produce_b is
    inlined behind load_candidates -- the first tile a workgroup generates -- hipcc contracts the scaling into the
    subtraction, df = fma(t, sc, -xs) (``fused`` True; docs/experiments.md, round 14).  A device value has the bits of
    one of the two.
    ``pairs``: only those entries."""
    if site not in SITES:
        raise ValueError(site)
    X1 = np.atleast_2d(np.asarray(X1, dtype=np.float64))
    gram = site == "gram"
    if gram != (X2 is None):
        raise ValueError("site 'gram' takes X2 = None, the other sites two point sets")
    if site == "sweep" and k.lin_coef != 0.0:
        raise ValueError("site 'sweep' restates pure squared-exponential kernels only")
    if fused and site != "sweep":
        raise ValueError("only site 'sweep' has a fused variant")
    sc, lw = kernconst(k)
    dp = len(sc)
    a = _scaled(X1, sc, k.ndim, dp, mutant)
    if fused:
        a = [[float(X1[i, d]) if d < k.ndim else 0.0 for d in range(dp)] for i in range(len(X1))]
    b = a if gram else _scaled(np.atleast_2d(np.asarray(X2, dtype=np.float64)), sc, k.ndim, dp, mutant)
    if mutant == "pad_nonzero" and dp > k.ndim:
        a = [row[:k.ndim] + [row[0]] * (dp - k.ndim) for row in a]      # the row point's padding keeps a stale value
        if gram:
            b = _scaled(X1, sc, k.ndim, dp, None)
    out = np.full((len(a), len(b)), np.nan)
    if pairs is None:
        pairs = [(i, j) for i in range(len(a)) for j in range(i + 1 if gram else len(b))]
    for i, j in pairs:
        out[i, j] = value_restate(a[i], b[j], k, lw, gram and i == j, mutant, sc if fused else None)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# input families (seeded, tiny).  Each case: (name, X1, X2 or None, Kern)
# ----------------------------------------------------------------------------------------------------------------------
LN2_32 = math.log(2.0) / 32.0


def exp_edge_arguments():
    """Arguments of apgp_exp at the reduction boundaries (k + 1/2) ln2/32 -/+ up to 3 ulp for k over the whole range,
    at 0 and around the clamp (negated: the callers pass x <= 0)."""
    out = [0.0, -0.0, 1e-300, 2.0 ** -60, 700.0, math.nextafter(700.0, 0.0), math.nextafter(700.0, 1e9), 745.2, 1e6]
    for kk in list(range(0, 200)) + list(range(200, 32320, 37)):
        c = (kk + 0.5) * LN2_32
        for step in (-3, -1, 0, 1, 3):
            v = c
            for _ in range(abs(step)):
                v = math.nextafter(v, math.inf if step > 0 else -math.inf)
            out.append(v)
    return [-v for v in out]


def lattice_edges_points():
    """1-D points on the 2^-16 grid whose squared distance from 0 sits on either side of a reduction boundary, at 0,
    on either side of 700 and at 1e6; all below 2^10, so that every pairwise difference has at most 26 bits and its
    square is exact."""
    xs = [0.0, 1000.0]
    for kk in list(range(0, 64)) + list(range(64, 32320, 101)):
        x = math.floor(math.sqrt((kk + 0.5) * LN2_32) * 65536.0) / 65536.0
        xs += [x, x + 2.0 ** -16]
    x = math.floor(math.sqrt(700.0) * 65536.0) / 65536.0
    xs += [x, x + 2.0 ** -16]
    return np.array(sorted(set(xs)))[:, None]


def lattice_1d(n=257, seed=0, log4=1, amp=1.0, diag_add=0.0):
    """n points of a 1-D dyadic lattice: xs on the 2^-16 grid in [0, 32), inv_metric = 2 * 4^log4 (sc = 2^log4 exactly):
    xs, df, df^2 and the sums are exact and n (n - 1) / 2 arguments are (nearly all) distinct."""
    rs = np.random.RandomState(100 + seed)
    r = np.sort(rs.choice(1 << 21, size=n, replace=False)).astype(np.float64)
    r[0] = 0.0
    xs = r * 2.0 ** -16
    return xs[:, None] / 2.0 ** log4, kern([2.0 * 4.0 ** log4], amp=amp, diag_add=diag_add)


def lattice_nd(n, D, seed=0, amp=1.0, diag_add=0.0):
    """D-dimensional dyadic lattice: xs on the 2^-8 grid in [0, 4), inv_metric_d = 2 * 4^k_d with k_d cycling through
    -1, 0, 1, 2."""
    rs = np.random.RandomState(200 + seed)
    kd = np.array([(d % 4) - 1 for d in range(D)], dtype=np.float64)
    xs = rs.randint(0, 1 << 10, size=(n, D)).astype(np.float64) * 2.0 ** -8
    return xs / 2.0 ** kd, kern(2.0 * 4.0 ** kd, amp=amp, diag_add=diag_add)


def general(n, D, seed=0, amp=2.7, diag_add=1e-3, lin_coef=0.0, lin_order=1, width=6.0):
    """Uniform coordinates in a box ``width`` length scales wide (around an offset of a few length scales: the
    cancellation term is alive), unequal metrics: one is 1e-3 and one 1e3 when D >= 2, the rest log-uniform."""
    rs = np.random.RandomState(300 + seed)
    im = 10.0 ** rs.uniform(-1.5, 1.5, size=D)
    im[0] = 1e-3
    if D >= 2:
        im[D - 1] = 1e3
    ell = 1.0 / np.sqrt(im)
    X = (rs.uniform(-0.5, 0.5, size=(n, D)) * width / math.sqrt(D) + rs.uniform(-3.0, 3.0, size=D)) * ell
    return X, kern(im, amp=amp, diag_add=diag_add, lin_coef=lin_coef, lin_order=lin_order)


def coincident(n, D, seed=0):
    """Pairs (x, x) and (x, nextafter(x)) inside a general set: row 2 i + 1 is row 2 i moved by one ulp in one
    coordinate (i odd: in every coordinate), and the last row repeats row 0."""
    X, k = general(n, D, seed=seed + 50)
    rs = np.random.RandomState(400 + seed)
    for i in range(0, n - 1, 2):
        X[i + 1] = X[i]
        if (i // 2) & 1:
            X[i + 1] = np.nextafter(X[i], np.inf)
        else:
            d = rs.randint(D)
            X[i + 1, d] = np.nextafter(X[i, d], -np.inf)
    X[n - 1] = X[0]
    return X, k


LIN_ORDERS = (0, 1, 2, 3, 16)
LIN_COEFS = {0: 1e-6, 1: 1e3, 2: 0.3, 3: 1e-2, 16: 1e-3}


def linear(n, D, order, seed=0):
    """Mixed-sign coordinates of order one, a linear term of the given order (lin_coef from 1e-6 to 1e3 across the
    orders) next to a squared-exponential part of comparable size."""
    rs = np.random.RandomState(500 + seed + order)
    im = 10.0 ** rs.uniform(-0.5, 0.5, size=D)
    X = rs.uniform(-1.2, 1.2, size=(n, D))
    return X, kern(im, amp=1.3, diag_add=1e-6, lin_coef=LIN_COEFS[order], lin_order=order)


def err_over_budget(values, X1, X2, k, pairs=None, mp_truth=False):
    """(worst |err| / budget, worst |err| in ulp of the truth) of ``values`` (m x n) over ``pairs`` (default: the lower
    triangle for a Gram matrix, everything otherwise; NaN entries of ``values`` are an error).  The ulp figure leaves
    out the entries the clamp at -700 governs (truth below amp 1e-304), where an ulp means nothing."""
    gram = X2 is None
    B = budget(X1, X2, k)
    T = truth_ld(X1, X2, k)
    m, n = B.shape
    if pairs is None:
        sel = np.tril(np.ones((m, n), dtype=bool)) if gram else np.ones((m, n), dtype=bool)
    else:
        sel = np.zeros((m, n), dtype=bool)
        ii, jj = zip(*pairs)
        sel[list(ii), list(jj)] = True
    if mp_truth:
        idx = list(zip(*np.nonzero(sel)))
        t = truth(X1, X2, k, idx)
        err = np.zeros((m, n))
        with mp.workdps(DPS):
            for (i, j) in idx:
                err[i, j] = float(abs(mp.mpf(float(values[i, j])) - t[i, j]))
    else:
        err = np.abs(np.asarray(values, dtype=np.longdouble) - T).astype(np.float64)
    if not np.all(np.isfinite(np.asarray(values)[sel])):
        return np.inf, np.inf
    norm = sel & (np.abs(T.astype(np.float64)) > k.amp * 1e-304) & np.isfinite(err)
    with np.errstate(over="ignore"):
        ratio = float((err[sel] / B[sel]).max())
        worst_ulp = float((err[norm] / ulp(T.astype(np.float64))[norm]).max()) if norm.any() else 0.0
    return ratio, worst_ulp
