# -*- coding: utf-8 -*-
"""Reference of the acquisition sweep's contraction and of the two packed factor images it streams -- apgp_trtri_pack's
image of W = L^-1, apgp_pack_lsolve's image of L, and mu / sigma^2 of apgp_acquire / apgp_acquire_solve -- with
CONDITION-FREE error budgets.  Plain Python (NumPy long double, kvalue_ref's exactly rounded fma): no GPU, no library
import.

Images (bit for bit)
    ``pack_linv``    restates pack_linv_kernel (csrc/linalg.hip): packed tile (ib, kc) holds, at e =
                     ((s 2 + kp) 64 + p) 2 + q, W[512 ib + 16 s + (p & 15)][16 kc + 4 (2 kp + q) + (p >> 4)], zero above
                     the diagonal and from row n on; row block ib has chunks 0 .. 32 (ib + 1) - 1.
    ``pack_lsolve``  restates pack_lsolve_kernel (csrc/sweep.hip:2113-2160) operation by operation: -L where the
                     16-column block lies below the row's, and in sub-block slot kc - 32 ib of a diagonal chunk the 256
                     doubles Ts[(4 q + q') 16 + 4 i + k]: -L (q' < q), column k of the inverse of the 4 x 4 diagonal
                     block by substitution (x_k = 1 / L_kk rounded, x_r = -sacc (1 / L_rr), sacc an fma chain), zero
                     above.  A negation is exact; an exact zero of L below the diagonal becomes -0.0.
    ``tile_decode``  the sqrt-based tile -> (ib, kc) decode of both kernels.

The contraction: what the device does to one candidate t (sweep2_kernel, csrc/sweep.hip)
    k*_j   produce_b (sweep.hip:713-744): tt = t sc, df = tt - xs_j, two fma lanes over even / odd coordinates,
           apgp_exp4 (apgp_common.h:226-260: apgp_exp's operations, interleaved four at a time), times amp, and with a
           linear term fma(lin_coef, lsum, .), lsum += q0 + q1 per coordinate PAIR.  A term of the pairwise sum passes
           through 1 + dpad / 2 <= D additions for every D >= 2 (D = 1: the partner is an exact zero), which is the D
           that kvalue_ref.budget charges: its count holds and is not extended.  e_k = kvalue_ref.budget.
    v_r    sum_j W_rj k*_j on the matrix cores: chained v_mfma_f64_4x4x4 over the chunks in column order
           (sweep.hip:303-311); the columns past r are exact zeros of the image.  r + 1 terms, hence at most r + 1
           additions on a term's way, + C_V = 1 for a product that the instruction may round before it adds (the ISA
           guide does not promise a fused product; factor_ref's C_SYRK):
               dv_r = u (r + 1 + C_V) (|W||k^|)_r + (|W| e_k)_r.
    q      per 256-row block (sweep.hip:616-631) each lane squares its 16 accumulators of a rotation into one fma chain
           (16 roundings, the square fused), adds the three other rotations (3), two shuffle levels over the row lanes
           (2), and the block's share joins qtot (one addition per row block; sweep_finish_kernel adds the split shares
           in the same order, sweep.hip:1044):  C_Q(nrb) = 16 + 3 + 2 + nrb = 21 + nrb,
               dq = sum_r (2 |v_r| dv_r + dv_r^2) + u C_Q q.
    var    ktt - q rounds once: |var - (ktt - q)| <= dq + dktt + u |var|.  ktt = amp, or with a linear term
           fma(lin_coef, ktl, amp), ktl = sum_d (t_d t_d)^P (sweep.hip:688-709): t_d t_d rounds once, P - 1 more
           products, at most D additions, and the fma rounds once:
               dktt = u (P + D) |lin_coef| sum_d t_d^(2P) + u |ktt|           (P = 0: ktl = D exactly).
    mu     produce_b (sweep.hip:745-756): lane k-quarter kq runs ONE fma chain over its columns of a row block
           (min(64, ceil(n / 4)) of them, the product fused), two shuffle levels, one addition per row block into
           mu_tot, then + mean (sweep.hip:787; the finish kernel likewise, sweep.hip:1044-1045):
               MU_DEPTH(n) = min(64, ceil(n / 4)) + 2 + nrb   (<= n + 3 for every n),
               dmu = u MU_DEPTH sum_j |alpha_j||k^_j| + sum_j |alpha_j| e_k,j + u |mu|.

The substitution form (MODE 1 / 2; micro solve sweep.hip:421-455 and 522-554)
    Row i, 4-row block q = i // 4, T_i = 4 q terms before its diagonal block.  acc = -sum_{j < 16 (i // 16)} L_ij v_j by
    the same chained instructions, + k*_i (one addition, sweep.hip:434), then up to three more instructions add the 12
    columns of the 16 x 16 diagonal block left of block q:
        |y_i - (k*_i - sum_{j < T_i} L_ij v_j)| <= u (T_i + 2) sum_{j < T_i} |L_ij||v_j| + 13 u |k*_i|
    (a term: at most T_i + 1 additions and its product; k*: its own addition and the 12 that follow).  Then
    v_q = X_q y_q with X_q the INVERTED 4 x 4 diagonal block, one instruction from a zero accumulator (4 roundings):
    pack_lsolve_kernel's columns satisfy |L_qq X_q - I| <= 5 u |L_qq||X_q| (an fma chain of at most 3 terms, the
    product with the rounded reciprocal: 2; the diagonal: 1), so
        |L_qq v_q - y_q| <= 9 u |L_qq||X_q||y_q| <= 9 u M_q (|L_qq||v_q|),   M_q = |L_qq||X_q|  (4 x 4, from the bits).
    Higham's Theorem 8.5 has a 1 where M_q stands: this is the price of the inverted block (``kappa4`` reports
    max_q ||M_q||_inf).  The residual of row i is therefore bounded by
        rho_i = u (T_i + 2) (|L_left||v|)_i + 13 u |k^_i| + 9 u (M_q |L_qq||v_q|)_i + e_k,i
    and the forward error componentwise by dv = |L^-1| rho (times 1 + 2^-20 for the second order).  Every v^2 passes
    through the qmic chain (64 fma per row block and lane), qs += qmic, two shuffle levels and qtot:
        C_Q_SOLVE(nrb) = 64 + 1 + 2 + nrb = 67 + nrb.

The inverse's right residual (``trtri_bound``), apgp_winv_apply (``winv_depth``) and apgp_predict1_host
(``predict1_counts``) carry their derivations in their docstrings.  The sweep's k* itself is kvalue_ref's site "sweep".

u = 2^-53.  None of the constants was fitted to device output; none contains cond(K).
"""
import numpy as np

import kvalue_ref as kr

U = 2.0 ** -53
LD = np.longdouble
ROWS = 512                   # APGP_ROW_BLOCK
KC = 16                      # APGP_K_CHUNK
CPB = ROWS // KC             # chunks per packed row-block width
TILE = ROWS * KC
S2_ROWS = 256                # rows per row block of sweep2_kernel
BASE = 131                   # distinct candidate rows of a case: coprime to 64
C_V = 1
SECOND = 1.0 + 2.0 ** -20


def npad(n):
    return (n + ROWS - 1) // ROWS * ROWS


def nrb(n):
    """256-row blocks of the sweep."""
    return (n + S2_ROWS - 1) // S2_ROWS


def ntiles(n):
    b = npad(n) // ROWS
    return CPB * b * (b + 1) // 2


def packed_len(n):
    return ntiles(n) * TILE


def c_q(n, solve=False):
    return (67 if solve else 21) + nrb(n)


def mu_depth(n):
    return min(64, (n + 3) // 4) + 2 + nrb(n)


def tile_decode(tile):
    """(ib, kc) of a packed tile as both pack kernels find it: a float64 sqrt, then two correcting loops."""
    ib = int((np.sqrt(8.0 * float(tile) / CPB + 1.0) - 1.0) * 0.5)
    while CPB * (ib + 1) * (ib + 2) // 2 <= tile:
        ib += 1
    while CPB * ib * (ib + 1) // 2 > tile:
        ib -= 1
    return ib, tile - CPB * ib * (ib + 1) // 2


def tile_list(n):
    """[(ib, kc)] in storage order, by enumeration (no decode)."""
    return [(ib, kc) for ib in range(npad(n) // ROWS) for kc in range(CPB * (ib + 1))]


def index_map(n):
    """(row, col) of every packed double in the A-fragment order, two int32 arrays of shape (ntiles, TILE)."""
    e = np.arange(TILE)
    q, lane, kp, s = e & 1, (e >> 1) & 63, (e >> 7) & 1, e >> 8
    r_in = (16 * s + (lane & 15)).astype(np.int32)
    c_in = (4 * (2 * kp + q) + (lane >> 4)).astype(np.int32)
    tl = np.array(tile_list(n), dtype=np.int32)
    return tl[:, 0][:, None] * ROWS + r_in[None, :], tl[:, 1][:, None] * KC + c_in[None, :]


def packed_index(r, c):
    """Flat index of W[r][c] (c <= r) in the packed image."""
    ib, kc = r // ROWS, c // KC
    s, i, kk, kq = (r % ROWS) // 16, r % 16, (c % KC) // 4, c % 4
    e = ((s * 2 + (kk >> 1)) * 64 + (i + 16 * kq)) * 2 + (kk & 1)
    return (CPB * ib * (ib + 1) // 2 + kc) * TILE + e


def pack_linv(W, n):
    """pack_linv_kernel: ``W`` any array whose [:n, :n] lower triangle is the inverse (the device's padded panel or a
    compact n x n matrix)."""
    W = np.asarray(W, dtype=np.float64)
    row, col = index_map(n)
    ok = (row < n) & (col <= row)
    out = np.zeros(row.shape)
    out[ok] = W[row[ok], col[ok]]
    return out.reshape(-1)


def unpack_linv(packed, n):
    """The dense n x n lower-triangular matrix of a packed image (and whether everything else in it is +0.0)."""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1, TILE)
    row, col = index_map(n)
    ok = (row < n) & (col <= row)
    W = np.zeros((n, n))
    W[row[ok], col[ok]] = packed[ok]
    rest = packed[~ok]
    return W, bool(np.all(rest.view(np.int64) == 0))


def inv4_column(B, k, i, ulp_off=None):
    """Entry (i, k), k <= i, of the inverse of the 4 x 4 lower-triangular block ``B`` as pack_lsolve_kernel forms it."""
    x = [0.0, 0.0, 0.0, 0.0]
    x[k] = 1.0 / float(B[k][k])
    for r in range(k + 1, i + 1):
        sacc = 0.0
        for c in range(k, r):
            sacc = kr.fma(float(B[r][c]), x[c], sacc)
        x[r] = -sacc * (1.0 / float(B[r][r]))
    return x[i]


def diag_slot(L, n, C, mutant=None):
    """The 256 doubles of the prepared 16 x 16 diagonal block C (rows 16 C .. 16 C + 15)."""
    Ts = np.zeros(256)
    for q in range(4):
        r0 = KC * C + 4 * q
        for q2 in range(q + 1):
            c0 = KC * C + 4 * q2
            for i in range(4):
                if r0 + i >= n:
                    continue
                for k in range(4):
                    f = (4 * q + q2) * 16 + 4 * i + k
                    if q2 < q:
                        Ts[f] = -L[r0 + i, c0 + k]
                    elif k <= i:
                        Ts[f] = inv4_column(L[r0:r0 + 4, r0:r0 + 4], k, i)
    if mutant == "inv4_ulp":                      # one entry of one 4 x 4 inverse off by one ulp
        f = (4 * 1 + 1) * 16 + 4 * 1 + 0 if KC * C + 5 < n else 0
        Ts[f] = np.nextafter(Ts[f], np.inf)
    return Ts


def pack_lsolve(L, n, mutant=None):
    """pack_lsolve_kernel on the lower triangle of ``L`` (n x n, or wider: only [:n, :n] below the diagonal and the
    diagonal are read)."""
    L = np.asarray(L, dtype=np.float64)
    row, col = index_map(n)
    ok = (row < n) & ((col >> 4) < (row >> 4))
    out = np.zeros(row.shape)
    out[ok] = -L[row[ok], col[ok]]
    for t, (ib, kc) in enumerate(tile_list(n)):
        s = kc - ib * CPB
        if 0 <= s < CPB:
            out[t, 256 * s:256 * s + 256] = diag_slot(L, n, kc, mutant if kc == 0 else None) if KC * kc < n else 0.0
    return out.reshape(-1)


def lsolve_slot_mask(n):
    """True at the packed doubles that belong to a prepared diagonal slot."""
    m = np.zeros((ntiles(n), TILE), dtype=bool)
    for t, (ib, kc) in enumerate(tile_list(n)):
        s = kc - ib * CPB
        if 0 <= s < CPB:
            m[t, 256 * s:256 * s + 256] = True
    return m.reshape(-1)


# ----------------------------------------------------------------------------------------------------------------------
# input families (seeded)
# ----------------------------------------------------------------------------------------------------------------------
LIN_COEF = {0: 0.05, 1: 0.3, 2: 0.1, 3: 0.04}      # (order 3: tests/predgrad_ref.py's cases)


def planted_w(n):
    """tril(N(0, 1)) / sqrt(n): any lower-triangular matrix may be planted, it need not be an inverse."""
    rs = np.random.RandomState(5000 + n)
    return np.tril(rs.normal(size=(n, n))) / np.sqrt(n)


def case(n, D, order=None, seed=0):
    """(X, alpha, T, kern, mean): n training points and BASE candidates in a box several length scales wide with unequal
    metrics and an offset (kvalue_ref.general; with a linear term kvalue_ref.linear).  The candidates are moved radially
    about the centre by factors 0.25 .. 1.9 and the first eight sit next to a training point, so that k^ runs from
    nearly amp down through many decades; alpha has mixed signs and magnitudes over two decades and is then corrected
    (least squares, minimum norm) so that k^ . alpha nearly cancels on every third candidate."""
    rs = np.random.RandomState(6000 + 41 * n + D + 1000 * (0 if order is None else 1 + order) + seed)
    if order is None:
        Z, k = kr.general(n + BASE, D, seed=n + D + seed, amp=2.7, diag_add=0.0, width=7.0)
    else:
        Z, k = kr.linear(n + BASE, D, order, seed=n + D + seed)
        k = k._replace(diag_add=0.0, lin_coef=LIN_COEF[order])
    X, T = Z[:n].copy(), Z[n:].copy()
    ell = 1.0 / np.sqrt(k.inv_metric)
    c = Z.mean(0)
    T = c + (T - c) * np.linspace(0.25, 1.9, BASE)[:, None]
    near = rs.randint(n, size=8)
    T[:8] = X[near] + 0.05 * ell * rs.normal(size=(8, D))
    alpha = rs.normal(size=n) * 10.0 ** rs.uniform(-1.0, 1.0, size=n)
    mean = 0.37
    rows = np.arange(0, BASE, 3)
    with np.errstate(all="ignore"):
        Kr = kr.truth_ld(T[rows], X, k).astype(np.float64)
    target = -mean + 0.01 * rs.normal(size=len(rows)) * (np.abs(Kr) @ np.abs(alpha))
    alpha = alpha + np.linalg.lstsq(Kr, target - Kr @ alpha, rcond=1e-8)[0]
    return X, alpha, T, k, mean


def tiled(T, m):
    """m candidate rows: the BASE distinct ones over and over (BASE is coprime to 64: every row meets every lane)."""
    return T[np.arange(m) % len(T)]


# ----------------------------------------------------------------------------------------------------------------------
# truth and budgets
# ----------------------------------------------------------------------------------------------------------------------
def ktt_truth(T, k):
    """(k(t, t) without noise in long double, bound of the device's error before the closing rounding)."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    if k.lin_coef == 0.0:
        return np.full(len(T), LD(k.amp)), np.zeros(len(T))
    P, D = k.lin_order, k.ndim
    s = np.full(len(T), LD(D)) if P == 0 else ((T.astype(LD) ** 2) ** P).sum(1)
    ktt = LD(k.lin_coef) * s + LD(k.amp)
    d = 0.0 if P == 0 else U * (P + D) * abs(k.lin_coef) * s.astype(np.float64) * SECOND
    return ktt, d + U * np.abs(ktt).astype(np.float64)


class Truth(object):
    """mu, q and var of the BASE candidates from the bits of (A, X, alpha, T, kern, mean), and their budgets.
    ``form`` "inverse": A = W, v = W k^.  ``form`` "solve": A = L, v = L^-1 k^ by a blocked long-double substitution;
    ``linv_abs``: |L^-1| for the bound (default: a float64 inverse inflated by 1 + 1e-6, for well-conditioned L; pass
    a long-double one otherwise).  ``consumer`` "predict1": the same quantities with the counts of apgp_predict1_host
    (``predict1_counts``)."""

    def __init__(self, A, X, alpha, T, k, mean, form="inverse", linv_abs=None, consumer="sweep"):
        A = np.tril(np.asarray(A, dtype=np.float64))
        X = np.ascontiguousarray(X, dtype=np.float64)
        T = np.ascontiguousarray(np.atleast_2d(T), dtype=np.float64)
        alpha = np.asarray(alpha, dtype=np.float64)
        n = len(X)
        self.n, self.form, self.k, self.T, self.X = n, form, k, T, X
        with np.errstate(all="ignore"):
            self.kh = kr.truth_ld(T, X, k)                      # m x n long double
            self.ek = kr.budget(T, X, k)
        ak = np.abs(self.kh).astype(np.float64)
        p1 = consumer == "predict1"
        if form == "inverse":
            self.v = (A.astype(LD) @ self.kh.T).T
            r = predict1_counts(n)["v"] if p1 else np.arange(n) + 1 + C_V
            aA = np.abs(A)
            self.dv = (U * r[None, :] * (ak @ aA.T) + self.ek @ aA.T) * SECOND
        else:
            self.v = solve_ld(A, self.kh.T).T
            self.dv = solve_forward_bound(A, self.v, ak, self.ek, linv_abs, trsv=p1)
        av = np.abs(self.v).astype(np.float64)
        self.q = (self.v * self.v).sum(1)
        qd = self.q.astype(np.float64)
        cq = predict1_counts(n)["q_solve" if form != "inverse" else "q"] if p1 else c_q(n, form != "inverse")
        self.dq = (2.0 * av * self.dv + self.dv * self.dv).sum(1) + U * cq * qd
        self.ktt, self.dktt = ktt_truth(T, k)
        self.var = self.ktt - self.q
        self.mu = self.kh @ alpha.astype(LD) + LD(mean)
        self.sabs = ak @ np.abs(alpha)
        self.dmu0 = U * (predict1_counts(n)["mu"] if p1 else mu_depth(n)) * self.sabs + self.ek @ np.abs(alpha)

    def _rep(self, a, m):
        return a[np.arange(m) % len(a)]

    def var_ratio(self, var):
        """|var - truth| / (dq + dktt + u |var|) for m >= BASE device rows (row i is candidate i mod BASE)."""
        var = np.asarray(var, dtype=np.float64)
        m = len(var)
        if not np.all(np.isfinite(var)):
            return np.where(np.isfinite(var), 0.0, np.inf)
        err = np.abs(var.astype(LD) - self._rep(self.var, m)).astype(np.float64)
        return err / (self._rep(self.dq + self.dktt, m) + U * np.abs(var))

    def mu_ratio(self, mu):
        mu = np.asarray(mu, dtype=np.float64)
        m = len(mu)
        if not np.all(np.isfinite(mu)):
            return np.where(np.isfinite(mu), 0.0, np.inf)
        err = np.abs(mu.astype(LD) - self._rep(self.mu, m)).astype(np.float64)
        return err / (self._rep(self.dmu0, m) + U * np.abs(mu))

    def guards(self):
        """(worst dq / q, decades that the squared-exponential part of k^ spans, rows with sum|alpha||k^| >= 10 |mu|)."""
        kse = self.kh if self.k.lin_coef == 0.0 else kr.truth_ld(self.T, self.X, self.k._replace(lin_coef=0.0))
        a = np.abs(kse).astype(np.float64)
        a = a[a > 0.0]
        return (float((self.dq / self.q.astype(np.float64)).max()), float(np.log10(a.max() / a.min())),
                int((self.sabs >= 10.0 * np.abs(self.mu).astype(np.float64)).sum()))


def solve_ld(L, B, blk=64):
    """L^-1 B in long double (L n x n lower, B n x m long double): 64-row blocks, the solved rows leave the block below
    through a long-double matrix product, the block itself row by row."""
    L = np.tril(np.asarray(L, dtype=np.float64)).astype(LD)
    n = len(L)
    V = np.array(B, dtype=LD)
    for b0 in range(0, n, blk):
        b1 = min(n, b0 + blk)
        if b0:
            V[b0:b1] -= L[b0:b1, :b0] @ V[:b0]
        for i in range(b0, b1):
            if i > b0:
                V[i] -= L[i, b0:i] @ V[b0:i]
            V[i] /= L[i, i]
    return V


def inv_ld(L):
    """L^-1 in long double (for |L^-1| of an ill-conditioned factor)."""
    return solve_ld(L, np.eye(len(L), dtype=LD))


def m4_blocks(L):
    """[M_q] = |L_qq||X_q| for every 4 x 4 diagonal block, X_q the block's inverse (float64 substitution: the bound
    needs three digits of it)."""
    n = len(L)
    out = []
    for r0 in range(0, n, 4):
        B = np.tril(L[r0:r0 + 4, r0:r0 + 4])
        Xq = np.linalg.solve(B, np.eye(len(B)))
        out.append(np.abs(B) @ np.abs(np.tril(Xq)))
    return out


def kappa4(L):
    return max(float(M.sum(1).max()) for M in m4_blocks(np.asarray(L, dtype=np.float64)))


def solve_residual_bound(L, v, ak, ek):
    """rho (m x n): the bound of |L v^ - k^| row by row (module docstring)."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    aL = np.abs(L)
    av = np.abs(np.asarray(v)).astype(np.float64)              # m x n
    q4 = np.arange(n) // 4
    left = aL * (np.arange(n)[None, :] < (4 * q4)[:, None])    # columns before the row's 4 x 4 diagonal block
    rho = U * (4 * q4 + 2)[None, :] * (av @ left.T) + 13.0 * U * ak + ek
    Ms = m4_blocks(L)
    for b, M in enumerate(Ms):
        s = slice(4 * b, min(n, 4 * b + 4))
        rho[:, s] += 9.0 * U * (av[:, s] @ aL[s, s].T) @ M.T
    return rho * SECOND


def predict1_counts(n):
    """Roundings on a term's way in apgp_predict1_host (csrc/linalg.hip: pred1_kstar_kernel, pred1_final_kernel;
    the single-launch kernel for n <= 256, pred1_small_kernel, forms every sum in the same order):
      mu       kv * alpha (1), six shuffle levels, (red0 + red1) + (red2 + red3) (2), one addition per 256-row part;
      v        through winv: winv_gemv_kernel with shift = 0 (``winv_depth`` less the subtraction); through L: apgp_trsv,
               factor_ref's C_TRSV residual |L v - k*|_i <= u ((i + 1 + C_TRSV) (|L||v|)_i + |k*_i|);
      q        pred1_final_kernel: one fma per 1024-stride trip, six shuffle levels, 16 partials; through L: the sum
               that rides along apgp_trsv (factor_ref.sumsq_bound's depth)."""
    import factor_ref as fr
    return {"mu": 1 + 6 + 2 + (n + 255) // 256, "v": winv_depth(n, 0) - 1, "q": (n + 1023) // 1024 + 6 + 16,
            "q_solve": 1 + 6 + max(16, fr.nblocks(n)) + (n + 1023) // 1024 - 1}


def trsv_residual_bound(L, v, ak, ek):
    import factor_ref as fr
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    av = np.abs(np.asarray(v)).astype(np.float64)
    return (U * ((np.arange(n) + 1 + fr.C_TRSV)[None, :] * (av @ np.abs(L).T) + ak) + ek) * SECOND


def solve_forward_bound(L, v, ak, ek, linv_abs=None, trsv=False):
    """dv = |L^-1| rho (m x n); ``trsv``: rho of apgp_trsv (a true substitution) instead of the sweep's."""
    if linv_abs is None:
        from_f64 = np.linalg.solve(np.tril(np.asarray(L, dtype=np.float64)), np.eye(len(L)))
        linv_abs = np.abs(np.tril(from_f64)) * (1.0 + 1e-6)
    rho = trsv_residual_bound(L, v, ak, ek) if trsv else solve_residual_bound(L, v, ak, ek)
    return rho @ np.asarray(linv_abs, dtype=np.float64).T


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement of the device order (NumPy's own sums inside one 4-column instruction: accurate enough to carry
# the mutants; the k* it starts from is the truth rounded to double)
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_row", "stale_rows", "skip_chunk", "col_shift", "parked_prev_block", "split_twice")


def restate(W, X, alpha, T, k, mean, kf=None, mutant=None, form="inverse"):
    """(mu, var) of every row of T in the sweep's order: row blocks of 256, columns in chunks of 16 and instructions of
    4, the fold of a row block's squares (16-accumulator chain per rotation, rotations 0 .. 3, row lanes pairwise), mu
    per k-lane chain, shares added in row-block order.  ``form`` "solve": ``W`` is L and every 4 x 4 block row is solved
    with the inverted diagonal block (float64 inverse of the block), squares through one chain per row block.
    Mutants (MUTANTS): the defects the budgets have to catch."""
    W = np.tril(np.asarray(W, dtype=np.float64))
    n = len(W)
    m = len(T)
    if kf is None:
        with np.errstate(all="ignore"):
            kf = kr.truth_ld(T, X, k).astype(np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    nb = nrb(n)
    npd = nb * S2_ROWS
    Wp = np.zeros((npd, npd))
    Wp[:n, :n] = W
    Kp = np.zeros((m, npd))
    Kp[:, :n] = kf
    al = np.zeros(npd)
    al[:n] = alpha
    cgrp = (np.arange(m) % 64 % 16) >> 2                        # candidate group b' of a row of T
    q_sh, mu_sh = [], []
    Vall = np.zeros((npd, m))
    for jb in range(nb):
        r0 = S2_ROWS * jb
        nkc = min(S2_ROWS // KC * (jb + 1), (n + KC - 1) // KC)
        V = np.zeros((S2_ROWS, m))
        if form == "solve":
            for b0 in range(r0, min(n, r0 + S2_ROWS), 4):
                b1 = min(n, b0 + 4)
                y = Kp[:, b0:b1].T - Wp[b0:b1, :b0] @ Vall[:b0]
                Vall[b0:b1] = np.tril(np.linalg.solve(Wp[b0:b1, b0:b1], np.eye(b1 - b0))) @ y
            V = Vall[r0:r0 + S2_ROWS].copy()
        else:
            for kc in range(nkc):
                if mutant == "skip_chunk" and kc == nkc // 2 and jb == nb - 1:
                    continue
                for kk in range(4):
                    c0 = KC * kc + 4 * kk
                    B = Kp[:, c0:c0 + 4].T
                    if mutant == "col_shift" and jb == nb - 1 and kc == 0 and kk == 0:
                        B = B[[0, 0, 2, 3]]                     # column c read for c + 1
                    if mutant == "parked_prev_block" and kc < S2_ROWS // KC * jb and kc == 0 and kk == 0:
                        B = np.roll(B, 64, axis=1)              # the operand parked for the previous 64 candidates
                    V += Wp[r0:r0 + S2_ROWS, c0:c0 + 4] @ B
        rows_here = min(n - r0, S2_ROWS)
        if mutant == "drop_last_row" and jb == nb - 1:
            V[rows_here - 1] = 0.0
        if mutant == "stale_rows" and jb == nb - 1 and rows_here < S2_ROWS:
            p1 = (rows_here + 31) >> 5                          # pairs the body works through; stale beyond them
            if 32 * p1 < S2_ROWS:
                V[32 * p1:] = V[:S2_ROWS - 32 * p1]
        Vr = V.reshape(16, 4, 4, m)                              # row = 16 s + 4 b + i
        if form == "solve":
            qs = np.zeros((4, m))
            for s_ in range(16):
                for b in range(4):
                    qs = qs + Vr[s_, b] * Vr[s_, b]
        else:
            qs = np.zeros((4, m))                               # [row lane i][candidate]
            for r in range(4):
                b = (cgrp - r) & 3
                qr = np.zeros((4, m))
                for s_ in range(16):
                    vv = Vr[s_, b, :, np.arange(m)].T            # rows 16 s + 4 b + i of each candidate
                    qr = qr + vv * vv
                qs = qr if r == 0 else qs + qr
        q_sh.append((qs[0] + qs[1]) + (qs[2] + qs[3]))
        mc = np.zeros((4, m))
        for j in range(r0, min(npd, r0 + S2_ROWS), 4):
            mc = mc + Kp[:, j:j + 4].T * al[j:j + 4, None]
        mu_sh.append((mc[0] + mc[1]) + (mc[2] + mc[3]))
    if mutant == "split_twice":
        q_sh.append(q_sh[0])
        mu_sh.append(mu_sh[0])
    q = np.zeros(m)
    mu = np.zeros(m)
    for a, b in zip(q_sh, mu_sh):
        q = q + a
        mu = mu + b
    Tm = np.atleast_2d(np.asarray(T, dtype=np.float64))
    if k.lin_coef != 0.0:
        ktl = np.full(m, float(k.ndim)) if k.lin_order == 0 else ((Tm * Tm) ** k.lin_order).sum(1)
        ktt = k.lin_coef * ktl + k.amp
    else:
        ktt = np.full(m, k.amp)
    return mu + mean, ktt - q


# ----------------------------------------------------------------------------------------------------------------------
# apgp_trtri_pack: the right residual L W - I, entry by entry
# ----------------------------------------------------------------------------------------------------------------------
def trtri_bound(L, W):
    """Entrywise bound of |L W^ - I| (n x n, lower triangle) for the device's inverse, by its own recursion.

    Diagonal 64-blocks (trtri_diag_kernel, csrc/linalg.hip): column c by substitution, x_i = -srow r_i with
    srow an fma chain over the i - c non-zero terms and r_i = 1 / L_ii rounded:
        |L_D X_D - I|_ic <= u (i - c + 2) (|L_D||X_D|)_ic,  <= u |L_cc x_c| on the diagonal.
    Merge of two halves at level s (trtri_merge_kernel, linalg.hip; apgp_gemm64_tile chains its instructions
    over the k range, csrc/mma16.h:89-132): T^ = L21 W11 + E1 and W21 = -(W22 T^ + E2), each product a chain over at
    most 64 s columns, g = 64 s + 1 with the product's own rounding (negation exact).  Then
        (L W)_21 = L21 W11 + L22 W21 = -E1 - (L22 W22 - I) T^ - L22 E2,
        |R_21| <= u g B + |R_22| B + u g |L22||W22| B,     B = |L21||W11| >= |T^| / (1 + u g),
    with |R_22| bounded by this same function one level down: the bound is made of |L||W||L||W| products and holds for
    any cond(L).  Everything from the bits of L and W^; times 1 + 2^-20 per level for the second order."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    W = np.tril(np.asarray(W, dtype=np.float64))
    n = len(L)
    nb = (n + 63) // 64
    aL, aW = np.abs(L), np.abs(W)
    Rb = np.zeros((n, n))
    for j in range(nb):
        s = slice(64 * j, min(n, 64 * j + 64))
        m = s.stop - s.start
        cnt = np.maximum(np.subtract.outer(np.arange(m), np.arange(m)) + 2, 1)
        Rb[s, s] = np.tril(U * cnt * (aL[s, s] @ aW[s, s])) * SECOND
    lev = 1
    while lev < nb:
        g = 64 * lev + 1
        for first0 in range(0, nb, 2 * lev):
            second0 = first0 + lev
            if second0 >= nb:
                continue
            f = slice(64 * first0, 64 * second0)
            sb = slice(64 * second0, min(n, 64 * (second0 + lev)))
            B = aL[sb, f] @ aW[f, f]
            Rb[sb, f] = (U * g * B + Rb[sb, sb] @ B + U * g * ((aL[sb, sb] @ aW[sb, sb]) @ B)) * SECOND
        lev *= 2
    return Rb


def trtri_ratio(L, W, rows=None):
    """|L W^ - I| / trtri_bound on the lower triangle (residual in long double from the bits; ``rows``: only those rows
    of the residual are formed -- the bound is float64 work and always whole).  A zero bound demands a zero residual."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    W = np.tril(np.asarray(W, dtype=np.float64))
    n = len(L)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    if not np.all(np.isfinite(W)):
        return np.full((len(rows), n), np.inf)
    res = np.abs(L[rows].astype(LD) @ W.astype(LD) - np.eye(n, dtype=LD)[rows]).astype(np.float64)
    den = trtri_bound(L, W)[rows]
    low = np.arange(n)[None, :] <= rows[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(res == 0.0, 0.0, res / den)
    return np.where(low, r, 0.0)


def trtri_restate(L, mutant=None):
    """The device's recursion in float64: 64-blocks by column substitution, then merges level by level.  Mutants:
    "merge_sign" is too coarse to be worth a test; "drop_k" leaves one k out of one phase-2 product, "stale_T" uses the
    T of the level before for the last merge's first tile row."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    nb = (n + 63) // 64
    W = np.zeros((n, n))
    for j in range(nb):
        s = slice(64 * j, min(n, 64 * j + 64))
        W[s, s] = fr_blk_inverse(L[s, s])
    lev = 1
    while lev < nb:
        for first0 in range(0, nb, 2 * lev):
            second0 = first0 + lev
            if second0 >= nb:
                continue
            f = slice(64 * first0, 64 * second0)
            sb = slice(64 * second0, min(n, 64 * (second0 + lev)))
            T = L[sb, f] @ W[f, f]
            W22 = W[sb, sb].copy()
            if mutant == "drop_k" and 2 * lev >= nb:
                W22[-1, 0] = 0.0
            W[sb, f] = -(W22 @ T)
        lev *= 2
    return W


def fr_blk_inverse(B):
    m = len(B)
    X = np.zeros((m, m))
    for c in range(m):
        X[c, c] = 1.0 / B[c, c]
        for i in range(c + 1, m):
            X[i, c] = -(B[i, c:i] @ X[c:i, c]) * (1.0 / B[i, i])
    return X


TRTRI_N = (1, 63, 64, 65, 129, 193, 257, 449)
TRTRI_BIG = 2100                     # 33 blocks: the level-16 merge takes two complementary tiles per workgroup


def trtri_big_rows(n):
    """Rows of the residual that are formed at TRTRI_BIG (long double is slow): every 17th row of the blocks the paired
    merge writes, and the last."""
    return np.r_[np.arange(1024, n - 1, 17), n - 1]


# ----------------------------------------------------------------------------------------------------------------------
# apgp_winv_apply: x = W (b - shift) or W^T b through the dense panel (csrc/linalg.hip: winv_gemv_kernel, winv_gemvt_*_kernel)
# ----------------------------------------------------------------------------------------------------------------------
WA_RCH = 128


def winv_depth(n, trans):
    """Roundings on a term's way, per output entry.  trans = 0 (winv_gemv_kernel): lane l of row i's wavefront runs two
    fma chains over k = 2 l, 2 l + 128, ...: ceil((i + 1) / 128) links, then s0 + s1 and six shuffle levels; b_k - shift
    rounds once more.  trans = 1 (winv_gemvt_partial_kernel / winv_gemvt_reduce_kernel): two chains of at most 64 links
    per 128-row chunk, s0 + s1, then one addition per chunk in chunk order; no shift."""
    i = np.arange(n)
    if trans:
        return np.full(n, 64 + 1 + (n + WA_RCH - 1) // WA_RCH)
    return (i + 128) // 128 + 1 + 6 + 1


def winv_apply_ratio(W, x, b, shift, trans):
    """|x - truth|_i / (u depth_i (|op(W)||b - shift|)_i): the truth in long double from the bits of W's lower triangle
    and of b - shift formed exactly."""
    W = np.tril(np.asarray(W, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    n = len(W)
    if not np.all(np.isfinite(x)):
        return np.full(n, np.inf)
    A = W.T if trans else W
    rhs = np.asarray(b, dtype=np.float64).astype(LD) - LD(shift)
    err = np.abs(A.astype(LD) @ rhs - x.astype(LD)).astype(np.float64)
    den = U * winv_depth(n, trans) * (np.abs(A) @ np.abs(rhs).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / den)


def winv_restate(W, b, shift, trans, mutant=None):
    """The two kernels' order in float64 (a product and a sum where the device has an fma).  Mutants: "drop_last_row"
    (trans = 0: the last column of every row; trans = 1: the last row of every chunk), "chunk_twice"."""
    W = np.tril(np.asarray(W, dtype=np.float64))
    n = len(W)
    x = np.zeros(n)
    if not trans:
        r = np.asarray(b, dtype=np.float64) - shift
        for i in range(n):
            lanes = np.zeros((2, 64))
            hi = i if mutant == "drop_last_row" and i > 0 else i + 1
            for k in range(0, hi):
                lanes[k & 1, (k >> 1) & 63] += W[i, k] * r[k]
            s = lanes[0] + lanes[1]
            for o in (32, 16, 8, 4, 2, 1):
                s = s + s[np.arange(64) ^ o]
            x[i] = s[0]
        return x
    z = np.asarray(b, dtype=np.float64)
    nch = (n + WA_RCH - 1) // WA_RCH
    for c in range(nch):
        r0, r1 = WA_RCH * c, min(n, WA_RCH * c + WA_RCH)
        if mutant == "drop_last_row":
            r1 -= 1
        s = np.zeros((2, n))
        for i in range(r0, r1):
            k = np.arange(min(i + 1, n))
            par = (i - np.maximum(r0, k)) & 1
            s[par, k] += W[i, k] * z[i]
        share = s[0] + s[1]
        x = x + share
        if mutant == "chunk_twice" and c == nch - 1:
            x = x + share
    return x


def winv_case(n):
    """(W, b, shift): tril(N(0, 1)) / sqrt(n) and a right-hand side with mixed signs over four decades."""
    rs = np.random.RandomState(7000 + n)
    return planted_w(n), rs.normal(size=n) * 10.0 ** rs.uniform(-2.0, 2.0, size=n), 0.125


def winv_panel(W, poison=np.nan):
    """The n x ldw panel (ldw = n rounded up to 64) apgp_winv_apply is handed: ``poison`` everywhere above the diagonal
    and in the padding, except the f64x2 partner W[i][i + 1] of an even row i's diagonal entry, which winv_gemv_kernel
    loads (and does not use): a zero stays there."""
    n = len(W)
    ldw = (n + 63) // 64 * 64
    P = np.full((n, ldw), poison)
    low = np.tril(np.ones((n, n), dtype=bool))
    P[:, :n][low] = W[low]
    for i in range(0, n, 2):
        if i + 1 < ldw:
            P[i, i + 1] = 0.0
    return P


WINV_N = (1, 2, 127, 128, 129, 255, 256, 257, 449)
PRED1_N = (1, 255, 256, 257, 513)
PRED1_CASES = tuple((n, D, P) for n in PRED1_N for D, P in ((2, None), (8, None), (2, 1), (8, 2)))
PRED1_ROWS = 12                      # candidates per case: one call each


def predict1_restate(A, X, alpha, T, k, mean, kf, form="inverse"):
    """(mu, var) in apgp_predict1_host's order, float64: mu over 64-lane trees per 256 rows, v by the forward product's
    lanes (or a blocked substitution), q over 1024 strided threads."""
    n = len(X)
    m = len(T)
    mu = np.zeros(m)
    for p0 in range(0, n, 256):
        c = np.zeros((m, 256))
        w = min(n, p0 + 256) - p0
        c[:, :w] = kf[:, p0:p0 + w] * alpha[p0:p0 + w]
        c = c.reshape(m, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            c = c + c[:, :, np.arange(64) ^ o]
        mu = mu + ((c[:, 0, 0] + c[:, 1, 0]) + (c[:, 2, 0] + c[:, 3, 0]))
    if form == "inverse":
        v = np.stack([winv_restate(A, kf[a], 0.0, 0) for a in range(m)])
    else:
        import factor_ref as fr
        v = np.stack([fr.trsv_restate(A, kf[a], 0.0, 0) for a in range(m)])
    s = np.zeros((m, 1024))
    for i0 in range(0, n, 1024):
        w = min(n, i0 + 1024) - i0
        s[:, :w] = s[:, :w] + v[:, i0:i0 + w] * v[:, i0:i0 + w]
    s = s.reshape(m, 16, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, np.arange(64) ^ o]
    q = np.zeros(m)
    for i in range(16):
        q = q + s[:, i, 0]
    Tm = np.atleast_2d(np.asarray(T, dtype=np.float64))
    if k.lin_coef != 0.0:
        ktl = np.full(m, float(k.ndim)) if k.lin_order == 0 else ((Tm * Tm) ** k.lin_order).sum(1)
        ktt = k.lin_coef * ktl + k.amp
    else:
        ktt = np.full(m, k.amp)
    return mu + mean, ktt - q

# the shapes of tests/test_gpu_sweep_budget.py (tests/test_sweep_ref.py runs the reference alone on the same ones)
IMAGE_N = (1, 16, 17, 511, 512, 513, 1025)
IMAGE_BIG = 4097                     # nine packed row blocks, 1440 tiles: the sqrt decode past 1024
BODY_N = (1, 16, 17, 128, 129, 192, 193, 255, 256)
ROW_BLOCK_N = BODY_N + tuple(256 + v for v in BODY_N) + (769,)
FEEDER_D = (1, 3, 5, 8, 9, 16, 17, 32)
LIN_CASES = tuple((P, D) for P in (0, 1, 2) for D in (3, 8, 32))
SOLVE_D = (2, 8, 17)
M_SMALL = 130
GRID = 256                           # persistent workgroups (SW_GRID)
SPLIT_MAX = 184                      # S2_SPLIT_MAX: a last round of more candidate blocks runs on the persistent grid


def m_of_blocks(blocks, ragged=True):
    """Candidates that make ``blocks`` 64-row blocks, the last one ragged (37 rows)."""
    return 64 * (blocks - 1) + (37 if ragged else 64)
