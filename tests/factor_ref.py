# -*- coding: utf-8 -*-
"""Reference of the factor layer -- apgp_potrf, apgp_trsv, apgp_kinv_solve, the W^T W product and the reduction of
apgp_grad_loglik -- with CONDITION-FREE error budgets.  Plain Python (NumPy long double; mpmath only in the tests'
spot checks): no GPU, no library import.

Every kernel here substitutes for real (no inverted diagonal block is used as a multiplier), so the componentwise
backward-error bounds of Higham, *Accuracy and Stability of Numerical Algorithms*, Thm 10.3 (Cholesky) and Thm 8.5 /
Lemma 8.4 (substitution) hold for ANY order of the sums: a term's error factor is the product of the (1 + delta) of the
roundings it passes through, and the bound is u times the LARGEST such count times sum |terms|.  The counts below are
read off the kernel source; none contains cond(K).  u = 2^-53.

C_CHOL = 4   |A - L L^T|_ij <= u (min(i,j) + 1 + C_CHOL) (|L||L^T|)_ij.
    The textbook count for entry (i, j), m = min(i, j), is m + 1: m subtractions and the pivot.  The device differs in
    two places.  (a) csrc/potrf.hip panel_factor_wave: the pivot is r = v_rsq_f64 + one third-order step (its last fma
    rounds once and its e = fma(-p r, r, 1) carries the rounding of p r: 1.5 u), an off-diagonal entry is sacc * r
    (one rounding) and the diagonal sqrt(p) is a Newton-corrected p r (one rounding): l_ij l_jj = sacc (1 + 3.5 u),
    where the textbook has 2 u (division, square root): + 1.5.  (b) the right-looking trailing update
    (potrf_step_kernel, "two products, each accumulated from zero and subtracted in turn", potrf.hip:61): a term of block
    column J' < J = m // 64 passes through at most 64 accumulations of its own tile product (csrc/mma16.h: 16 chained
    v_mfma_f64_4x4x4, four k each), then one subtraction per block column before J, then the m % 64 fmas of the panel:
    64 + J + m % 64 + 3.5 against m + 1 = 64 J + m % 64 + 1, which is worst at J = 1: + 3.5 (J = 0: + 2.5).  Rounded
    up: 4.
C_TRSV = 3   |op(L) x - (b - shift)|_i <= u ((n_i + C_TRSV) (|op(L)||x|)_i + |b_i - shift|), n_i terms in row i.
    b - shift rounds once (the |b_i - shift| term; Lemma 8.4 leaves the right-hand side unperturbed otherwise).  The
    pivot is a division in trsv_kernel (its two substitution loops: one rounding), a product with a rounded reciprocal
    in trsv_step4_kernel / trsv_persist_kernel (`inv = 1.0 / Lb[lane][lane]`, then `* inv`: two), and zacc * r with
    the 1.5 u reciprocal square root against the 1 u diagonal in the solve that rides along apgp_potrf (potrf.hip:331: 3.5 u on
    the diagonal term l_ii x_i).  Off-diagonal tiles are 16-term fma chains added pairwise and subtracted in block
    order (trsv_tile_chain, trsv_tile_sum): 16 + 2 + J + i % 64 + 2 <= n_i + 1 from the second block row on; trsv_kernel's
    transposed sweep (its `r[c] -= acc` loop) subtracts a chain of up to 64 terms per block: kmax + 1 + (63 - i % 64) + 1
    = n_i + 1.  The largest excess over n_i is therefore the first row of potrf's solve, n_i = 1 with 3.5 roundings:
    + 2.5, rounded up: 3.
C_SYRK = 1   |sum_k W_ki W_kj - truth| <= u (n - max(i,j) + C_SYRK) sum_k |W_ki||W_kj|   (grad.hip:40, syrk_wtw_kernel).
    The n - max(i, j) non-zero terms are accumulated in k order by chained matrix instructions; the leading zero terms
    (k < max(i, j), W is lower triangular) add exact zeros.  + 1 for a product that the instruction may round before
    it adds (the ISA guide does not promise a fused product).
x.x          |ss - x.x| <= u depth sum x_i^2: one product, six shuffle levels, then 16 wavefront partials in order
    (trsv_kernel's closing loop, sumsq_kernel) or one addition per 64-row block (trsv_step4_kernel / persistent,
    trsv_block_sumsq); sumsq_kernel's strided loop adds ceil(n / 1024) - 1.
gradient     see ``grad_record``.
"""
import math

import numpy as np

import kvalue_ref as kr

U = 2.0 ** -53
C_CHOL = 4
C_TRSV = 3
C_SYRK = 1
TILE = 64
MAX_DIM = 32
LD = np.longdouble

# the shapes of tests/test_gpu_factor_budget.py (tests/test_factor_ref.py runs the reference alone on the same ones)
POTRF_N = (1, 2, 63, 64, 65, 127, 128, 129, 193, 257, 449)
TRSV_N = (1, 2, 63, 64, 65, 255, 256, 257, 449)
KINV_N = (1, 63, 64, 65, 127, 128, 129, 200, 257)
GRAD_N = (1, 63, 64, 65, 128, 129, 200)
GRAD_D = (1, 2, 3, 5, 8, 9, 17, 32)
GRAD_LIN = ((0, 65, 3), (1, 65, 3), (2, 129, 2), (3, 65, 5), (1, 128, 17), (2, 63, 1), (3, 200, 8), (0, 129, 32))
GRAD_BIG = (2881, 2)          # nb = 46, 1081 tiles: grad_final_kernel's strided loop takes a second trip


def nblocks(n):
    return (n + TILE - 1) // TILE


def lower_tile_mask(n):
    """True where (i, j) lies in a 64 x 64 tile on or below the block diagonal: what the K^-1 kernels write and
    grad_tile_kernel reads (the upper halves of the diagonal tiles included)."""
    b = np.arange(n) // TILE
    return b[:, None] >= b[None, :]


# ----------------------------------------------------------------------------------------------------------------------
# matrix families (seeded)
# ----------------------------------------------------------------------------------------------------------------------
def se_gram(n):
    """The recipe of test_cholesky_c_abi_against_lapack: squared-exponential Gram of uniform points, jitter 1e-6
    (cond up to 4e7), and a right-hand side."""
    rs = np.random.RandomState(100 + n)
    X = rs.uniform(-3, 3, size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2) + 1e-6 * np.eye(n), rs.randn(n)


def ill_gram(n, decades=13.0):
    """Q diag(lambda) Q^T with lambda log-spaced from 1 down to 10^-decades and a seeded orthogonal Q: dense, mixed
    signs, cond 1e13 for every n >= 2 (n = 1: the 1 x 1 matrix [1]).  LAPACK factors it at every size the tests use
    (tests/test_factor_ref.py asserts that)."""
    rs = np.random.RandomState(700 + n)
    Q, _ = np.linalg.qr(rs.normal(size=(n, n)))
    lam = np.logspace(0.0, -decades, n) if n > 1 else np.ones(1)
    K = (Q * lam) @ Q.T
    return 0.5 * (K + K.T), rs.randn(n)


def gram(family, n):
    return {"se": se_gram, "ill": ill_gram}[family](n)


def planted_factor(n):
    """The factor of test_persistent_trsv_bit_identical_to_multi_launch: well conditioned, mixed signs."""
    rs = np.random.RandomState(n)
    return np.tril(rs.normal(size=(n, n)) * 0.05) + np.diag(1.0 + rs.uniform(size=n)), rs.normal(size=n)


def factor(family, n):
    """(L, b): "planted", or "ill" = NumPy's Cholesky factor of ``ill_gram``."""
    if family == "planted":
        return planted_factor(n)
    K, b = ill_gram(n)
    return np.linalg.cholesky(K), b


# ----------------------------------------------------------------------------------------------------------------------
# ratios and bounds
# ----------------------------------------------------------------------------------------------------------------------
def chol_ratio(A, L):
    """|A - L L^T|_ij / (u (min(i,j) + 1 + C_CHOL) (|L||L^T|)_ij) on the lower triangle (n x n; the strict upper
    triangle is returned as 0).  The residual is formed in long double from the bits of A's lower triangle and of L's;
    a zero bound demands a zero residual (ratio inf otherwise); a non-finite L gives inf."""
    A = np.asarray(A, dtype=np.float64)
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(A)
    low = np.tril(np.ones((n, n), dtype=bool))
    if not np.all(np.isfinite(L)):
        return np.where(low, np.inf, 0.0)
    Ll = L.astype(LD)
    res = np.abs(np.tril(A).astype(LD) - Ll @ Ll.T).astype(np.float64)
    aL = np.abs(L)
    m = np.minimum.outer(np.arange(n), np.arange(n)) + 1 + C_CHOL
    den = U * m * (aL @ aL.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(res == 0.0, 0.0, res / den)
    return np.where(low, r, 0.0)


def trsv_ratio(L, x, b, shift, trans):
    """|op(L) x - (b - shift)|_i / (u ((n_i + C_TRSV) (|op(L)||x|)_i + |b_i - shift|)), n_i = i + 1 (trans = 0) or
    n - i (trans = 1); residual in long double (b - shift exactly, from the bits of b and shift)."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if not np.all(np.isfinite(x)):
        return np.full(n, np.inf)
    T = L.T if trans else L
    rhs = np.asarray(b, dtype=np.float64).astype(LD) - LD(shift)
    res = np.abs(T.astype(LD) @ x.astype(LD) - rhs).astype(np.float64)
    ni = (n - np.arange(n)) if trans else (np.arange(n) + 1)
    den = U * ((ni + C_TRSV) * (np.abs(T) @ np.abs(x)) + np.abs(rhs).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(res == 0.0, 0.0, res / den)


def sumsq_bound(x):
    """(truth of x.x in long double, bound of |device sum - truth|): depth = 1 + 6 + max(16, blocks) + strided trips."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    depth = 1 + 6 + max(16, nblocks(n)) + (n + 1023) // 1024 - 1
    t = (x.astype(LD) ** 2).sum()
    return t, U * depth * float(t)


def _dd_div_d(x, d):
    """Double-double x over the double d: quotient, exact remainder (two_prod), correction."""
    q1 = x[0] / d
    p = kr._two_prod(q1, d)
    r = kr._dd_add(x, (-p[0], -p[1]))
    return kr._two_sum(q1, (r[0] + r[1]) / d)


def kinv_truth(L):
    """(L L^T)^-1 from the bits of L as an n x n long-double matrix: a forward and a backward substitution against the
    identity, column-oriented, in DOUBLE-DOUBLE (kvalue_ref's error-free transformations, ~2^-100), rounded once to long
    double.  Plain long-double substitutions are 0.004 ulp of a double off at cond 1e12 and
    1e13 (n = 70, relative to max |truth|), twice the 2^-9 ulp that tests/test_factor_ref.py asks for; this form is at
    0.0002 ulp and takes 0.2 s at n = 200.  Only the lower triangle is solved for; the upper one is its mirror."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    Xh, Xl = np.eye(n), np.zeros((n, n))
    with np.errstate(all="ignore"):
        for k in range(n):                              # X = L^-1: row k is final, then leaves the rows below
            rh, rl = _dd_div_d((Xh[k, :k + 1], Xl[k, :k + 1]), L[k, k])
            Xh[k, :k + 1], Xl[k, :k + 1] = rh, rl
            if k + 1 < n:
                c = L[k + 1:, k][:, None]
                ph, pl = kr._dd_mul((rh[None, :], rl[None, :]), (c, np.zeros_like(c)))
                Xh[k + 1:, :k + 1], Xl[k + 1:, :k + 1] = kr._dd_add((Xh[k + 1:, :k + 1], Xl[k + 1:, :k + 1]), (-ph, -pl))
        for k in range(n - 1, -1, -1):                  # Y = L^-T X, columns j <= i only (Y is symmetric)
            rh, rl = _dd_div_d((Xh[k, :k + 1], Xl[k, :k + 1]), L[k, k])
            Xh[k, :k + 1], Xl[k, :k + 1] = rh, rl
            if k:
                c = L[k, :k][:, None]
                ph, pl = kr._dd_mul((rh[None, :k], rl[None, :k]), (c, np.zeros_like(c)))
                Xh[:k, :k], Xl[:k, :k] = kr._dd_add((Xh[:k, :k], Xl[:k, :k]), (-ph, -pl))
    Y = np.tril(Xh).astype(LD) + np.tril(Xl).astype(LD)
    return Y + np.tril(Y, -1).T


def kinv_tile_errors(Kinv, truth):
    """{(bi, bj): (worst |Kinv - truth| in the tile, max |truth| in the tile)} over the lower tiles."""
    n = len(truth)
    out = {}
    err = np.abs(np.asarray(Kinv, dtype=np.float64).astype(LD) - truth).astype(np.float64)
    at = np.abs(truth).astype(np.float64)
    for bi in range(nblocks(n)):
        for bj in range(bi + 1):
            r, c = slice(TILE * bi, min(n, TILE * bi + TILE)), slice(TILE * bj, min(n, TILE * bj + TILE))
            e = err[r, c]
            out[bi, bj] = (np.inf if not np.all(np.isfinite(e)) else float(e.max()), float(at[r, c].max()))
    return out


def kinv_bar_ratio(Kinv, L):
    """Worst over the lower tiles of err / max(3 x scipy cho_solve's worst error in that tile on the same L,
    n u max|truth in tile|): the bar of tests/test_gpu_factor_budget.py (c)."""
    from scipy.linalg import cho_solve
    n = len(L)
    T = kinv_truth(L)
    mine = kinv_tile_errors(Kinv, T)
    ref = kinv_tile_errors(cho_solve((np.tril(L), True), np.eye(n)), T)
    worst = 0.0
    for key, (e, tmax) in mine.items():
        worst = max(worst, e / max(3.0 * ref[key][0], n * U * tmax))
    return worst


def syrk_bound(W):
    """(truth, bound) of Kinv_ij = sum_k W_ki W_kj for lower-triangular W: the truth in long double from W's bits, the
    bound u (n - max(i,j) + C_SYRK) sum_k |W_ki||W_kj|."""
    W = np.tril(np.asarray(W, dtype=np.float64))
    n = len(W)
    Wl = W.astype(LD)
    aW = np.abs(W)
    cnt = n - np.maximum.outer(np.arange(n), np.arange(n)) + C_SYRK
    return Wl.T @ Wl, U * cnt * (aW.T @ aW)


# ----------------------------------------------------------------------------------------------------------------------
# the gradient record
# ----------------------------------------------------------------------------------------------------------------------
E_A = 2          # alpha_i alpha_j rounds once, the subtraction of Kinv_ij once: each <= u (|alpha_i alpha_j| + |Kinv_ij|)
E_AK = 1         # A * k  (A * lin_coef for the linear term)


def grad_depth(n):
    """Summation depth of grad_tile_kernel + grad_final_kernel (grad.hip:240-279, 289-300): 16 serial adds per thread,
    6 shuffle levels, 4 partials, then ceil(nblk / 1024) strided adds, 6 shuffle levels, 16 partials."""
    nb = nblocks(n)
    nblk = nb * (nb + 1) // 2
    return 16 + 6 + 4 + (nblk + 1023) // 1024 + 6 + 16


def final_depth(n):
    return (n + 1023) // 1024 + 6 + 16


def grad_record(X, alpha, Kinv, kern):
    """The five quantities of apgp_grad_loglik in long double from the given bits, and a budget for each.

    values / budgets: dicts with "sum_alpha" (out[0]), "amp" (out[1]), "metric" (out[2 + d], arrays of ndim), "trace"
    (out[2 + MAX_DIM]) and "lin" (out[3 + MAX_DIM]).  Only the lower 64 x 64 tiles of ``Kinv`` are read (the whole
    diagonal tiles: the kernel reads their upper halves); an off-diagonal tile counts twice.  Formed one block row at a
    time (64 x n long doubles), so n = 2881 needs no n x n long-double matrix.

    With A_ij = alpha_i alpha_j - Kinv_ij, k_ij the squared-exponential part (amp included) and q_ij = lin_coef
    sum_d (x_id x_jd)^P:   amp = 1/2 sum A k,   metric_d = 1/2 sum A k h_d (h_d = inv_metric_d (x_id - x_jd)^2 / 2),
    lin = 1/2 sum A q,  trace = 1/2 sum_i (alpha_i^2 - Kinv_ii).

    Budget = u/2 sum_ij w (|alpha_i alpha_j| + |Kinv_ij|) |dK_ij| (E_A + E_AK + e_k,ij + depth):
      e_k,ij  kvalue_ref.budget of the pair over u |k_ij| -- grad_tile_kernel's two fma chains over even and odd
              coordinates and its amp * apgp_exp are apgp_gram_value's (grad.hip:245-255), so the count is the same;
      h_d     df_d * df_d rounds once and inherits the error of df_d (the scaling of the two points and the
              subtraction: kvalue_ref's "xs" and "df" terms): |dh_d| <= u (2 |df_d| (|xs_id| + |xs_jd|) + 5 df_d^2)
              + 4 u^2 (|xs_id| + |xs_jd|)^2, added as an absolute term times |k_ij|;
      q       kvalue_ref's linear count (8 P - 1) + D on sum_d |x_id x_jd|^P;
      depth   ``grad_depth``: the fma into the thread's sum is the first of its 16 adds.  Not n^2.
    trace: alpha_i^2 and the subtraction round once each, then ``final_depth``; sum_alpha: ``final_depth``."""
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    n, D = X.shape
    kse = kr.kern(kern.inv_metric, amp=kern.amp)
    sc = np.sqrt(0.5 * kern.inv_metric)
    half = 0.5 * kern.inv_metric.astype(LD)
    P = kern.lin_order
    depth = grad_depth(n)
    val = {"amp": LD(0), "metric": np.zeros(D, dtype=LD), "lin": LD(0)}
    bud = {"amp": 0.0, "metric": np.zeros(D), "lin": 0.0}
    al = alpha.astype(LD)
    for bi in range(nblocks(n)):
        r0, r1 = TILE * bi, min(n, TILE * bi + TILE)
        Xr, Xc = X[r0:r1], X[:r1]
        w = np.where(np.arange(r1) < r0, 2.0, 1.0)[None, :]
        Kt = np.asarray(Kinv[r0:r1, :r1], dtype=np.float64)
        A = np.outer(al[r0:r1], al[:r1]) - Kt.astype(LD)
        absA = np.abs(np.outer(alpha[r0:r1], alpha[:r1])) + np.abs(Kt)
        k = kr.truth_ld(Xr, Xc, kse)
        ak = np.abs(k).astype(np.float64)
        Bk = kr.budget(Xr, Xc, kse)
        E = E_A + E_AK + depth
        val["amp"] += (w * A * k).sum()
        bud["amp"] += float((w * absA * (U * E * ak + Bk)).sum())
        for d in range(D):
            df = Xr[:, d].astype(LD)[:, None] - Xc[:, d].astype(LD)[None, :]
            h = half[d] * df * df
            hd = h.astype(np.float64)
            xa, xb = np.abs(Xr[:, d] * sc[d])[:, None], np.abs(Xc[:, d] * sc[d])[None, :]
            dfd = np.sqrt(hd)
            Bh = U * (2.0 * dfd * (xa + xb) + 5.0 * hd) + 4.0 * U * U * (xa + xb) ** 2
            val["metric"][d] += (w * A * k * h).sum()
            bud["metric"][d] += float((w * absA * (hd * (U * E * ak + Bk) + ak * Bh)).sum())
        if kern.lin_coef != 0.0:
            if P == 0:
                q = np.full(A.shape, float(D), dtype=LD)
                sabs, cnt = np.full(A.shape, float(D)), 0
            else:
                q = np.zeros(A.shape, dtype=LD)
                sabs = np.zeros(A.shape)
                for d in range(D):
                    p = Xr[:, d].astype(LD)[:, None] * Xc[:, d].astype(LD)[None, :]
                    q += p ** P
                    sabs += np.abs(Xr[:, d][:, None] * Xc[:, d][None, :]) ** P
                cnt = (8 * P - 1) + D
            val["lin"] += LD(kern.lin_coef) * (w * A * q).sum()
            bud["lin"] += float((w * absA * abs(kern.lin_coef) * sabs * U * (E + cnt)).sum())
    dg = np.diag(np.asarray(Kinv, dtype=np.float64)) if n > 1 else np.asarray(Kinv, dtype=np.float64).reshape(1)
    val = {"sum_alpha": al.sum(), "amp": 0.5 * val["amp"], "metric": 0.5 * val["metric"],
           "trace": 0.5 * (al * al - dg.astype(LD)).sum(), "lin": 0.5 * val["lin"]}
    fd = final_depth(n)
    bud = {"sum_alpha": U * fd * float(np.abs(alpha).sum()), "amp": 0.5 * bud["amp"], "metric": 0.5 * bud["metric"],
           "trace": 0.5 * U * (2 + fd) * float((alpha * alpha + np.abs(dg)).sum()), "lin": 0.5 * bud["lin"]}
    return val, bud


def grad_ratios(out, val, bud, ndim, lin):
    """{name: worst |out - value| / budget} for a device (or restated) ``out`` vector of 4 + MAX_DIM doubles.  A zero
    budget demands a zero error; a non-finite output is inf.  ``lin``: the kernel has a linear term (the slot is only
    meaningful then)."""
    out = np.asarray(out, dtype=np.float64)

    def one(o, v, b):
        if not np.isfinite(o):
            return np.inf
        e = float(abs(LD(o) - v))
        return 0.0 if e == 0.0 else (np.inf if b == 0.0 else e / b)
    r = {"sum_alpha": one(out[0], val["sum_alpha"], bud["sum_alpha"]), "amp": one(out[1], val["amp"], bud["amp"]),
         "metric": max(one(out[2 + d], val["metric"][d], bud["metric"][d]) for d in range(ndim)),
         "trace": one(out[2 + MAX_DIM], val["trace"], bud["trace"])}
    if lin:
        r["lin"] = one(out[3 + MAX_DIM], val["lin"], bud["lin"])
    return r


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatements of the device order (NumPy's own sums inside a tile: accurate enough to carry the mutants)
# ----------------------------------------------------------------------------------------------------------------------
CHOL_MUTANTS = ("fp32_product", "drop_k", "ragged_last_row", "fp32_pivot")
KINV_MUTANTS = ("pass1_late", "pass0_stale_nan")
GRAD_MUTANTS = ("weight1", "diag_twice", "skip_last_odd", "lin_sign", "transposed_read")


def chol_restate(A, mutant=None):
    """Blocked right-looking Cholesky with 64-column steps: the panel by columns with a reciprocal pivot, then every
    trailing tile minus a product accumulated from zero.  Mutants (CHOL_MUTANTS) hit the first step / the last tile row."""
    A = np.asarray(A, dtype=np.float64)
    n = len(A)
    L = np.tril(A).copy()
    nb = nblocks(n)
    for J in range(nb):
        j0, j1 = TILE * J, min(n, TILE * J + TILE)
        for j in range(j0, j1):
            piv = L[j, j]
            r = 1.0 / math.sqrt(piv) if piv > 0.0 else float("nan")
            if mutant == "fp32_pivot" and j == 0:
                r = float(np.float32(r))
            L[j, j] = math.sqrt(piv) if piv > 0.0 else float("nan")
            L[j + 1:, j] *= r
            if j + 1 < j1:
                L[j + 1:, j + 1:j1] -= np.outer(L[j + 1:, j], L[j + 1:j1, j])
        L = np.tril(L)
        for bj in range(J + 1, nb):
            c0, c1 = TILE * bj, min(n, TILE * bj + TILE)
            for bi in range(bj, nb):
                r0, r1 = TILE * bi, min(n, TILE * bi + TILE)
                a, b = L[r0:r1, j0:j1], L[c0:c1, j0:j1]
                Pm = a @ b.T
                hit = J == 0 and bi == nb - 1 and bj == max(1, nb - 2)
                if hit and mutant in ("fp32_product", "drop_k"):
                    i, j = r1 - r0 - 1, 0
                    terms = a[i] * b[j]
                    kk = int(np.argmax(np.abs(terms)))
                    Pm[i, j] += (float(np.float32(terms[kk])) if mutant == "fp32_product" else 0.0) - terms[kk]
                if hit and mutant == "ragged_last_row":
                    Pm[r1 - r0 - 1, :] = 0.0
                L[r0:r1, c0:c1] -= Pm
        L = np.tril(L)
    return L


def _blk_fwd(Lb, R):
    Xb = np.array(R, dtype=np.float64)
    for i in range(len(Lb)):
        if i:
            Xb[i] -= Lb[i, :i] @ Xb[:i]
        Xb[i] /= Lb[i, i]
    return Xb


def _blk_bwd(Lb, R):
    Xb = np.array(R, dtype=np.float64)
    m = len(Lb)
    for i in range(m - 1, -1, -1):
        if i + 1 < m:
            Xb[i] -= Lb[i + 1:, i] @ Xb[i + 1:]
        Xb[i] /= Lb[i, i]
    return Xb


def trsv_restate(L, b, shift, trans):
    """Blocked substitution: 64-row blocks, the solved blocks subtracted tile by tile in solving order."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    r = np.asarray(b, dtype=np.float64) - shift
    nb = nblocks(n)
    order = range(nb - 1, -1, -1) if trans else range(nb)
    for jb in order:
        s = slice(TILE * jb, min(n, TILE * jb + TILE))
        r[s] = _blk_bwd(L[s, s], r[s]) if trans else _blk_fwd(L[s, s], r[s])
        for ob in (range(jb - 1, -1, -1) if trans else range(jb + 1, nb)):
            o = slice(TILE * ob, min(n, TILE * ob + TILE))
            r[o] -= (L[s, o].T @ r[s]) if trans else (L[o, s] @ r[s])
    return r


def kinv_restate(L, mutant=None, sentinel=np.nan, stale=None):
    """apgp_kinv_solve's two passes on the padded np x np layout (identity rows past n): pass 0 X = L^-1 block row by
    block row, rows and columns past n stored as zero; pass 1 Y = L^-T X from the last block row up, lower tiles only.
    Returns the n x n ``kinv`` buffer pre-filled with ``sentinel``.  ``stale``: a value pass 0 leaves in the rows past
    n of X instead of the zero (a finite one must not change a bit of the result: those rows meet zeros of L only)."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    nb = nblocks(n)
    npad = TILE * nb
    Lp = np.eye(npad)
    Lp[:n, :n] = L
    X = np.zeros((npad, npad))
    Y = np.full((n, n), sentinel)
    if mutant == "pass0_stale_nan":
        stale = np.nan
    for j in range(nb):
        r = slice(TILE * j, TILE * j + TILE)
        ce = TILE * (j + 1)
        rhs = np.eye(npad)[r, :ce] - Lp[r, :TILE * j] @ X[:TILE * j, :ce]
        X[r, :ce] = _blk_fwd(Lp[r, r], rhs)
        X[n:, :] = 0.0 if stale is None else stale
        X[:, n:] = 0.0
    for j in range(nb - 1, -1, -1):
        r = slice(TILE * j, TILE * j + TILE)
        ce = TILE * (j + 1)
        k0 = TILE * (j + 1) + (TILE if mutant == "pass1_late" else 0)
        acc = np.zeros((TILE, ce))
        if k0 < n:
            acc = Lp[k0:n, r].T @ Y[k0:n, :ce]
        with np.errstate(invalid="ignore"):
            sol = _blk_bwd(Lp[r, r], X[r, :ce] - acc)
        rr = min(n, TILE * j + TILE) - TILE * j
        Y[TILE * j:TILE * j + rr, :min(n, ce)] = sol[:rr, :min(n, ce)]
    return Y


def grad_restate(X, alpha, Kinv, kern, mutant=None):
    """The tiled gradient sum in float64 as an ``out`` vector of 4 + MAX_DIM doubles: one partial per lower tile (the
    scaled coordinates, k = amp exp(-(sum of squares)), A = alpha_i alpha_j - Kinv_ij), off-diagonal tiles twice."""
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(len(X), len(X))
    n, D = X.shape
    sc, lw = np.sqrt(0.5 * kern.inv_metric), 2.0 / kern.inv_metric
    Xs = X * sc
    Duse = D - 1 if (mutant == "skip_last_odd" and D % 2 == 1) else D
    part = np.zeros(2 + D)
    for bi in range(nblocks(n)):
        for bj in range(bi + 1):
            r, c = slice(TILE * bi, min(n, TILE * bi + TILE)), slice(TILE * bj, min(n, TILE * bj + TILE))
            df2 = (Xs[r, None, :] - Xs[None, c, :]) ** 2
            df2[:, :, Duse:] = 0.0
            k = kern.amp * np.exp(-df2.sum(-1))
            Kt = Kinv[c, r].T if (mutant == "transposed_read" and bi != bj) else Kinv[r, c]
            A = np.outer(alpha[r], alpha[c]) - Kt
            wt = 1.0 if bi == bj else 2.0
            if mutant == "weight1":
                wt = 1.0
            if mutant == "diag_twice":
                wt = 2.0
            Ak = A * k
            part[0] += wt * Ak.sum()
            part[1:1 + D] += wt * (Ak[:, :, None] * df2).sum((0, 1))
            if kern.lin_coef != 0.0:
                if kern.lin_order == 0:
                    ls = np.full(A.shape, float(D))
                else:
                    ls = (((Xs[r, None, :] * Xs[None, c, :]) * lw) ** kern.lin_order).sum(-1)
                part[1 + D] += wt * (A * kern.lin_coef * ls).sum() * (-1.0 if mutant == "lin_sign" else 1.0)
    out = np.zeros(4 + MAX_DIM)
    out[0] = alpha.sum()
    out[1] = 0.5 * part[0]
    out[2:2 + D] = 0.5 * part[1:1 + D]
    out[2 + MAX_DIM] = 0.5 * (alpha * alpha - np.diag(Kinv)).sum()
    out[3 + MAX_DIM] = 0.5 * part[1 + D]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inputs of the gradient tests (seeded)
# ----------------------------------------------------------------------------------------------------------------------
def grad_case(n, D, lin_order=None, seed=0, poison=np.nan):
    """(X, alpha, Kinv, kern): points a few length scales wide with unequal metrics, amp = 2.7, alpha with mixed signs
    and magnitudes over four decades, and a symmetric random ``Kinv`` on the lower tiles (whole diagonal tiles) with
    every tile strictly above the block diagonal set to ``poison``."""
    rs = np.random.RandomState(9000 + 37 * n + D + 1000 * (0 if lin_order is None else 1 + lin_order) + seed)
    if lin_order is None:
        X, k = kr.general(n, D, seed=n + D, amp=2.7, diag_add=0.0, width=4.0)
    else:
        X, k = kr.linear(n, D, lin_order, seed=n + D)
        k = k._replace(diag_add=0.0, amp=1.3)
    alpha = rs.normal(size=n) * 10.0 ** rs.uniform(-2.0, 2.0, size=n)
    S = rs.normal(size=(n, n)) * 10.0 ** rs.uniform(-1.0, 1.0, size=(n, n))
    Kinv = np.tril(S) + np.tril(S, -1).T
    Kinv[~lower_tile_mask(n)] = poison
    return X, alpha, Kinv, k
