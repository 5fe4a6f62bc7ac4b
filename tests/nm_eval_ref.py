# -*- coding: utf-8 -*-
"""Reference of the two large-n evaluators of the restarted Nelder-Mead search (csrc/nmsearch.hip: FORM 1, the dense
inverse at n > 256, nm_kstar + nm_quad_inverse; FORM 2, the factor L at any n, nm_kstar + nm_quad_solve) with
CONDITION-FREE error budgets.  Plain Python (NumPy long double): no GPU, no library import.  The truths, the k* budget,
the long-double solves and the factor families are sweep_ref's, kvalue_ref's and factor_ref's; only the rounding counts
of the two forms, their float64 restatement and its mutants live here.

Counts (a term's error factor is the product of the 1 + delta of the roundings it passes through; u = 2^-53; every line
number is csrc/nmsearch.hip's)

    k*_k   nm_kstar, lines 81-96: tt = xt sc rounds once (nm_eval, line 173), df = tt - xs, two fma lanes over even /
           odd coordinates, amp * apgp_exp(-(q0 + q1)), and with a linear term fma(lin_coef, APGP_LIN_SUM, kv): the
           operation sequence of apgp_gram_value.  e_k = kvalue_ref.budget, not extended.
    mu     line 97: contrib = fma(kv, alpha_k, contrib) once per 256-stride trip of a thread, ceil(n / 256) fused
           products; line 99: six shuffle levels; line 199: (red0 + red1) + (red2 + red3), two more (the `mu = 0.0;
           mu += ...` around it adds to an exact zero); line 200: + mean rounds once, which is the u |mu| of
           ``Truth.mu_ratio``:
               MU_DEPTH(n) = ceil(n / 256) + 6 + 2,
               dmu = u MU_DEPTH sum_k |alpha_k||k^_k| + sum_k |alpha_k| e_k + u |mu|.
    FORM 1 (nm_quad_inverse)
    v_i    line 111: lane l of row i's wavefront runs one fma chain over k = l, l + 64, ... <= i, at most
           ceil((i + 1) / 64) links; line 112: six shuffle levels:
               dv_i = u (ceil((i + 1) / 64) + 6) (|W||k^|)_i + (|W| e_k)_i.
    q      line 113: qw = fma(s0, s0, qw) once per row of the wavefront's stride (rows w, w + 4, ...: at most
           ceil(n / 4), the square fused); line 197: q = 0 + red2[0] + ... + red2[3], the first addition exact:
               C_Q(n) = ceil(n / 4) + 3,   dq = sum_i (2 |v_i| dv_i + dv_i^2) + u C_Q q.
    FORM 2 (nm_quad_solve): a true substitution -- the diagonal divides (line 148), nothing is multiplied by an inverted
    block -- so Higham's Lemma 8.2 applies row by row.  Row i, block start j0 = 64 floor(i / 64):
           line 133   part p of the row's four threads chains fma over k = p, p + 4, ... < j0: ceil(j0 / 4) links
           135-136    two shuffle additions                                                      2
           line 143   r_i -= acc                                                                 1
           line 150   ri = fma(-Lb[i][k], z_k, ri) for the k = j0 .. i - 1 of the block           i - j0
           line 148   z_i = ri / Lb[i][i]                                                        1
       which is ceil(j0 / 4) + 2 + 1 + (i - j0) + 1 roundings on the longest way; the count this reference was asked to
       hold the kernel to has one to spare,
               c_i = ceil(j0 / 4) + 2 + 1 + (i - j0) + 2,
               |L v^ - k^|_i <= u (c_i (|L||v^|)_i + |k^_i|) + e_k,i,
       carried forward by |L^-1| as sweep_ref.solve_forward_bound does.  Dividing the recurrence by the factors the
       right-hand side passes through (Lemma 8.2's step) leaves k^_i unperturbed, every term left of the block with
       ceil(j0 / 4) + 2, a term of the block with at most i - j0 and the diagonal term with i - j0 + 2 roundings: the
       count above dominates each of them and the u |k^_i| is spare.  It is kept as set; it is not fitted to anything.
    q      line 154: qacc = fma(ri, ri, qacc) once per block and lane, nblocks = ceil(n / 64) links; line 160: six
           shuffle levels; line 197 adds exact zeros:   C_Q_SOLVE(n) = ceil(n / 64) + 6.
    var    nm_ktt (lines 62-73) is apgp_predict1_host's host arithmetic, sweep_ref.ktt_truth's count; ktt - q rounds once.

None of the constants was fitted to device output; none contains cond(K)."""
import numpy as np

import factor_ref as fr
import kvalue_ref as kr
import sweep_ref as sr

U = sr.U
LD = sr.LD
NM_T = 256                   # threads of a workgroup
NM_B = 64                    # rows per block of the substitution
BASE = sr.BASE


def counts(n):
    """Roundings on a term's way (module docstring)."""
    i = np.arange(n)
    j0 = NM_B * (i // NM_B)
    return {"mu": (n + NM_T - 1) // NM_T + 6 + 2,
            "v": (i + 64) // 64 + 6,
            "q": (n + 3) // 4 + 3,
            "c": (j0 + 3) // 4 + 2 + 1 + (i - j0) + 2,
            "q_solve": fr.nblocks(n) + 6}


def residual_bound(L, v, ak, ek):
    """rho (m x n): the bound of |L v^ - k^| row by row for nm_quad_solve."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    av = np.abs(np.asarray(v)).astype(np.float64)
    return (U * (counts(len(L))["c"][None, :] * (av @ np.abs(L).T) + ak) + ek) * sr.SECOND


class Truth(sr.Truth):
    """sweep_ref.Truth (mu, q, var of every row of T from the bits of the inputs) with the budgets of FORM 1
    (``form`` "inverse") and FORM 2 ("solve") of apgp_nm_search in place of the sweep's."""

    def __init__(self, A, X, alpha, T, k, mean, form="inverse", linv_abs=None):
        sr.Truth.__init__(self, A, X, alpha, T, k, mean, form=form, linv_abs=linv_abs)
        A = np.tril(np.asarray(A, dtype=np.float64))
        c = counts(self.n)
        ak = np.abs(self.kh).astype(np.float64)
        if form == "inverse":
            aA = np.abs(A)
            self.dv = (U * c["v"][None, :] * (ak @ aA.T) + self.ek @ aA.T) * sr.SECOND
            cq = c["q"]
        else:
            if linv_abs is None:
                linv_abs = np.abs(np.tril(np.linalg.solve(A, np.eye(self.n)))) * (1.0 + 1e-6)
            self.dv = residual_bound(A, self.v, ak, self.ek) @ np.asarray(linv_abs, dtype=np.float64).T
            cq = c["q_solve"]
        av = np.abs(self.v).astype(np.float64)
        self.dq = (2.0 * av * self.dv + self.dv * self.dv).sum(1) + U * cq * self.q.astype(np.float64)
        self.dmu0 = U * c["mu"] * self.sabs + self.ek @ np.abs(np.asarray(alpha, dtype=np.float64))

    def ratios(self, mu, var, keep=None):
        """(worst mu ratio, worst var ratio) over the rows of ``keep`` (default: all)."""
        keep = np.ones(len(mu), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        rm = self.mu_ratio(np.where(keep, mu, 0.0))[keep]
        rv = self.var_ratio(np.where(keep, var, 0.0))[keep]
        return float(rm.max()), float(rv.max())


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement of the device order (a product and a sum where the device has an fma; the k* it starts from is the
# truth rounded to double)
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = {"inverse": ("drop_last_row", "mu_three_waves", "kstar_unscaled_pad"),
           "solve": ("lost_part", "stale_tail", "lb_col_shift", "q_skips_block", "mu_three_waves", "kstar_unscaled_pad")}
_XOR = tuple(np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1))


def _tree(c):
    """The six-level xor tree over the last axis (64 lanes); lane 0's value."""
    for p in _XOR:
        c = c + c[..., p]
    return c[..., 0]


def kstar(T, X, k, mutant=None):
    """k* (m x n float64).  "kstar_unscaled_pad": the first padded coordinate of the scaled point holds the scaled
    first coordinate instead of a zero (only where dpad > ndim)."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    with np.errstate(all="ignore"):
        kf = kr.truth_ld(T, X, k).astype(np.float64)
        if mutant == "kstar_unscaled_pad" and kr.dpad(k.ndim) > k.ndim:
            kse = kf if k.lin_coef == 0.0 else kr.truth_ld(T, X, k._replace(lin_coef=0.0)).astype(np.float64)
            pad = T[:, 0] * np.sqrt(0.5 * k.inv_metric[0])
            kf = kse * np.exp(-pad * pad)[:, None] + (kf - kse)
    return kf


def _mu(kf, alpha, mean, mutant):
    """The 256-stride k* . alpha: one chain per thread, the xor tree per wavefront, (red0 + red1) + (red2 + red3)."""
    m, n = kf.shape
    c = np.zeros((m, NM_T))
    for p0 in range(0, n, NM_T):
        w = min(n, p0 + NM_T) - p0
        c[:, :w] = c[:, :w] + kf[:, p0:p0 + w] * alpha[p0:p0 + w]
    red = _tree(c.reshape(m, 4, 64))
    if mutant == "mu_three_waves":
        red[:, 3] = 0.0                                          # red[3] is dropped
    return ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])) + mean


def _quad_inverse(W, kf, mutant):
    """nm_quad_inverse: the 64-lane row dot with the xor tree, then one chain of squares per wavefront (rows w, w + 4,
    ...) and 0 + red2[0] + ... + red2[3]."""
    m, n = kf.shape
    nch = (n + 63) // 64
    Wp = np.zeros((n, 64 * nch))
    Wp[:, :n] = W
    Kp = np.zeros((m, 64 * nch))
    Kp[:, :n] = kf
    S = np.zeros((m, n, 64))
    for c in range(nch):                                         # (columns past i are zeros: exact additions)
        S[:, 64 * c:] = S[:, 64 * c:] + Wp[None, 64 * c:, 64 * c:64 * c + 64] * Kp[:, None, 64 * c:64 * c + 64]
    v = _tree(S)
    rows = n - 1 if mutant == "drop_last_row" else n             # the wave striding stops one row early
    nq = (n + 3) // 4
    V2 = np.zeros((m, 4 * nq))
    V2[:, :rows] = v[:, :rows] * v[:, :rows]
    V2 = V2.reshape(m, nq, 4)
    qw = np.zeros((m, 4))
    for j in range(nq):
        qw = qw + V2[:, j]
    return ((qw[:, 0] + qw[:, 1]) + qw[:, 2]) + qw[:, 3]


def _quad_solve(L, kf, mutant):
    """nm_quad_solve: per 64-row block the 4-part dot against the solved part, the in-block substitution with the
    division, one chain of squares per lane, the xor tree."""
    m, n = kf.shape
    r = kf.copy()
    qacc = np.zeros((m, NM_B))
    nb = fr.nblocks(n)
    for jb in range(nb):
        j0 = NM_B * jb
        bs = min(NM_B, n - j0)
        if j0:
            Lr = L[j0:j0 + bs, :j0].reshape(bs, j0 // 4, 4)
            rr = r[:, :j0].reshape(m, j0 // 4, 4)
            acc = np.zeros((m, bs, 4))
            for s in range(j0 // 4):
                acc = acc + Lr[None, :, s, :] * rr[:, None, s, :]
            tot = acc[..., 0] + acc[..., 1]
            if mutant != "lost_part":                            # one of the 4 partials' pairs is not added
                tot = tot + (acc[..., 2] + acc[..., 3])
            r[:, j0:j0 + bs] = r[:, j0:j0 + bs] - tot
        Lb = L[j0:j0 + bs, j0:j0 + bs]
        Lo = np.roll(Lb, -1, axis=1) if mutant == "lb_col_shift" else Lb     # Lb is read one column off
        ri = r[:, j0:j0 + bs].copy()
        for k in range(bs):
            zk = ri[:, k] / Lb[k, k]
            ri[:, k] = zk
            if k + 1 < bs:
                ri[:, k + 1:] = ri[:, k + 1:] - Lo[None, k + 1:, k] * zk[:, None]
        r[:, j0:j0 + bs] = ri
        if not (mutant == "q_skips_block" and jb == nb - 1):     # the last block's ri^2 is not added
            qacc[:, :bs] = qacc[:, :bs] + ri * ri
        if mutant == "stale_tail" and bs < NM_B:                 # lanes past bs carry the evaluation before
            tail = np.roll(kf, 1, axis=0)[:, (j0 + np.arange(bs, NM_B)) % n]
            qacc[:, bs:] = qacc[:, bs:] + tail * tail
    return _tree(qacc)


def restate(A, X, alpha, T, k, mean, form, mutant=None, kf=None):
    """(mu, var) of every row of T in the device's order.  ``form`` "inverse": A = W (FORM 1); "solve": A = L (FORM 2).
    ``mutant``: one of MUTANTS[form], a one-line change that mimics a kernel bug; a mutant of the other form changes
    nothing."""
    A = np.tril(np.asarray(A, dtype=np.float64))
    alpha = np.asarray(alpha, dtype=np.float64)
    Tm = np.atleast_2d(np.asarray(T, dtype=np.float64))
    if kf is None or mutant == "kstar_unscaled_pad":
        kf = kstar(Tm, X, k, mutant)
    mu = _mu(kf, alpha, mean, mutant)
    q = _quad_inverse(A, kf, mutant) if form == "inverse" else _quad_solve(A, kf, mutant)
    m = len(Tm)
    if k.lin_coef != 0.0:
        ktl = np.full(m, float(k.ndim)) if k.lin_order == 0 else ((Tm * Tm) ** k.lin_order).sum(1)
        ktt = k.lin_coef * ktl + k.amp
    else:
        ktt = np.full(m, k.amp)
    return mu, ktt - q


# ----------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_nm_eval_budget.py (tests/test_nm_eval_ref.py runs the reference alone on the same ones)
# ----------------------------------------------------------------------------------------------------------------------
FORM1_N = (257, 319, 320, 321, 513)          # beside the 64-lane, the 4-wavefront and the 256-thread stride
FORM2_N = (1, 3, 63, 64, 65, 127, 129, 257, 300)
ILL_N = tuple(n for n in FORM2_N if n in fr.POTRF_N and n > 1)       # sizes tests/test_factor_ref.py factors "ill" at
DL = ((1, None), (2, None), (8, None), (17, None), (32, None), (2, 1), (8, 2))   # every apgp_by_dpad instantiation
N_DL = {"inverse": 321, "solve": 129}        # the size the instantiations run at
D_N = 8                                      # the instantiation the sizes run at
STALE = (65, 8)                              # (n, D) of the stale-state case
BOX_N = {"inverse": 321, "solve": 129}


def ldw_of(n):
    """The smallest even ldw >= n and the next multiple of 64."""
    return tuple(sorted({(n + 1) // 2 * 2, (n + 63) // 64 * 64}))


def ldl_of(n):
    return (n, n + 3)


def cases(form):
    """[(n, D, lin_order, family)]: every size at D_N, every (D, lin_order) at N_DL[form], "ill" at ILL_N."""
    sizes = FORM1_N if form == "inverse" else FORM2_N
    out = [(n, D_N, None, "planted") for n in sizes]
    out += [(N_DL[form], D, P, "planted") for D, P in DL if (D, P) != (D_N, None)]
    if form == "solve":
        out += [(n, D_N, None, "ill") for n in ILL_N]
    return out


def operand(form, n, family="planted"):
    """(A, |L^-1| or None): the planted W, or the factor with a long-double |L^-1| for the "ill" family."""
    if form == "inverse":
        return sr.planted_w(n), None
    L = fr.factor(family, n)[0]
    return L, (np.abs(sr.inv_ld(L)).astype(np.float64) * (1.0 + 1e-9) if family == "ill" else None)


def panel(M, ld, fill):
    """The n x ld buffer the device is handed: ``fill`` strictly above the diagonal and in the padding columns."""
    n = len(M)
    buf = np.full((n, ld), fill)
    low = np.tril(np.ones((n, n), dtype=bool))
    buf[:, :n][low] = np.asarray(M, dtype=np.float64)[low]
    return buf


CASE_SEED = {(321, 2, 1): 2}                 # seed 0 draws metrics under which k^ spans 2.6 decades only
SHELL_N = 8                                  # below it the cancellation in mu is planted on a shell


def case(n, D, order=None):
    """sweep_ref.case, changed where it cannot meet the input conditions that tests/test_nm_eval_ref.py asserts:
    another seed where the drawn metrics leave k^ under six decades, and for n < SHELL_N -- too few unknowns for the
    least-squares correction of alpha to cancel mu on a third of the candidates -- every third candidate of the near
    half (the far half keeps k^'s decades) is put on a thin shell (exponent 0.09, +- 2 %) about the first training
    point, where k^ is nearly one number, before the same correction is made."""
    X, alpha, T, k, mean = sr.case(n, D, order, seed=CASE_SEED.get((n, D, order), 0))
    if n < SHELL_N:
        rs = np.random.RandomState(8000 + 41 * n + D)
        rows = np.arange(0, BASE // 2, 3)
        u = rs.normal(size=(len(rows), D))
        u /= np.sqrt((u * u).sum(1))[:, None]
        rad = 0.3 * (1.0 + 0.01 * rs.uniform(-1.0, 1.0, size=len(rows)))
        T[rows] = X[0] + np.sqrt(2.0 / k.inv_metric) * rad[:, None] * u
        with np.errstate(all="ignore"):
            Kr = kr.truth_ld(T[rows], X, k).astype(np.float64)
        target = -mean + 0.01 * rs.normal(size=len(rows)) * (np.abs(Kr) @ np.abs(alpha))
        alpha = alpha + np.linalg.lstsq(Kr, target - Kr @ alpha, rcond=1e-8)[0]
    return X, alpha, T, k, mean


_TRUTHS = {}
_STALE = []


def truth(form, n, D, order=None, family="planted"):
    """((X, alpha, T, kern, mean), A, Truth) of a case: built once, shared, never changed."""
    key = (form, n, D, order, family)
    if key not in _TRUTHS:
        c = case(n, D, order)
        A, la = operand(form, n, family)
        _TRUTHS[key] = (c, A, Truth(A, *c, form=form, linv_abs=la))
    return _TRUTHS[key]


def box_of(T):
    """(lo, hi) that leaves about a third of the candidates outside: the first coordinate's lower tercile cuts."""
    lo = T.min(0) - 1.0
    hi = T.max(0) + 1.0
    lo[0] = np.sort(T[:, 0])[len(T) // 3]
    return lo, hi


def stale_case():
    """(X, alpha, verts, kern, mean, start): n = 65, the D + 1 vertices of the first simplex about the candidate whose
    vertices differ most in k* (``vertex_spread``): a k* entry left over from the evaluation before is then far outside
    any budget."""
    if not _STALE:
        n, D = STALE
        X, alpha, T, k, mean = case(n, D)
        start = T[int(np.argmax([vertex_spread(simplex(t), X, k) for t in T]))].copy()
        _STALE.append((X, alpha, simplex(start), k, mean, start))
    return _STALE[0]


def vertex_spread(V, X, k):
    """The smallest over the vertices 1 .. D of max_j |k*_vertex,j - k*_0,j| / max |k*|."""
    kf = kstar(V, X, k)
    return float((np.abs(kf[1:] - kf[0]).max(1) / np.abs(kf).max()).min())


def simplex(x0):
    """SciPy's first simplex (nmsearch.hip:247-251): x0, then coordinate k scaled by 1.05 (0.00025 for a zero)."""
    x0 = np.asarray(x0, dtype=np.float64)
    V = np.tile(x0, (len(x0) + 1, 1))
    for kk in range(len(x0)):
        V[kk + 1, kk] = (1.0 + 0.05) * x0[kk] if x0[kk] != 0.0 else 0.00025
    return V
