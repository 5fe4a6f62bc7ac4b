"""NumPy restatement of the batch design-point selection (GP.acquire_batch / apgp_acquire_fantasy; DESIGN.md "Batch
design points") and the naive re-conditioning it must agree with.

GP: k(x, x') = amp exp(-0.5 sum_d (x_d - x'_d)^2 inv_metric_d) + lin_coef sum_d (x_d x'_d)^P, K = k(X, X) + diag_add I,
predictive mean k(t, X) K^-1 (y - mean) + mean, variance k(t, t) - k(t, X) K^-1 k(X, t).

fantasy_batch: one full prediction, then per step j the rank-one downdate
    s_j = v_{j-1}(x_j) + diag_add,  beta_j = K^-1 k(X, x_j),
    c_j(t) = k(t, x_j) - k(t, X) beta_j - sum_{i<j} C_i(t) C_i(x_j),  C_j = c_j / sqrt(s_j),  v_j = v_{j-1} - C_j^2
recondition_batch: the slow path -- the training set extended by the picks at their predicted means, K refactorised
and mu / sigma^2 recomputed from scratch at every step.

ONE call of the pass alone (apgp_acquire_fantasy, fantasy_kernel in csrc/sweep.hip), for a GIVEN beta -- the second half
of this file: ``pass_truth`` (long double), ``pass_budget`` (roundings counted off the kernel, derivation beside it),
``pass_restate`` (the device's operation order with kvalue_ref's exactly rounded fma, and the mutants the budget has to
catch) and the case tables that tests/test_fantasy_ref.py (CPU) and tests/test_gpu_fantasy_budget.py (MI355X) share.
beta is planted, not solved for: nothing in the bar depends on cond(K)."""
import collections
import math

import numpy as np
from scipy.special import erfc

import kvalue_ref as kr
import sweep_ref as sr

KINDS = ("agp", "bape", "jones")


def kernel(A, B, amp, inv_metric, lin_coef=0.0, lin_order=1):
    A = np.atleast_2d(A)
    B = np.atleast_2d(B)
    d2 = (((A[:, None, :] - B[None, :, :]) ** 2) * np.asarray(inv_metric)[None, None, :]).sum(-1)
    K = amp * np.exp(-0.5 * d2)
    if lin_coef != 0.0:
        prod = A[:, None, :] * B[None, :, :]
        K = K + lin_coef * (np.sum(prod ** lin_order, axis=-1) if lin_order > 0 else A.shape[1])
    return K


def kdiag(T, amp, lin_coef=0.0, lin_order=1):
    out = np.full(len(T), float(amp))
    if lin_coef != 0.0:
        out = out + lin_coef * (np.sum((T * T) ** lin_order, axis=1) if lin_order > 0 else T.shape[1])
    return out


def utility(kind, mu, var, zeta=0.01, ybest=0.0):
    """The sweep's utilities (utility.py AGP / BAPE / Jones), element-wise."""
    mu = np.asarray(mu, dtype=float)
    var = np.asarray(var, dtype=float)
    with np.errstate(all="ignore"):
        if kind == "agp":
            return -(mu + 0.5 * np.log(2.0 * np.pi * np.e * var))
        if kind == "bape":
            lse = np.where(var <= 0.0, -np.inf, var + np.log(1.0 - np.exp(-var)))
            return -((2.0 * mu + var) + lse)
        sd = np.sqrt(var)
        imp = mu - ybest - zeta
        z = imp / sd
        cdf = 0.5 * erfc(-z / np.sqrt(2.0))
        pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
        return np.where(sd > 0.0, -(imp * cdf + sd * pdf), 0.0)


def admissible(T, bounds=None, mask=None):
    ok = np.ones(len(T), dtype=bool)
    if bounds is not None:
        b = np.asarray(bounds, dtype=float).reshape(-1, 2)
        ok &= np.all((T >= b[:, 0]) & (T <= b[:, 1]), axis=1)
    if mask is not None:
        ok &= np.asarray(mask).astype(bool)
    return ok


def argmin(u):
    """The sweep's arg-min contract: NaN and +inf never win, ties go to the lowest index; -1 if nothing is left."""
    w = np.where(np.isnan(u), np.inf, u)
    if not np.any(w < np.inf):
        return -1
    return int(np.argmin(w))


def _predict(X, y, T, gp):
    K = kernel(X, X, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"]) + gp["diag_add"] * np.eye(len(X))
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y - gp["mean"]))
    Ks = kernel(T, X, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"])
    V = np.linalg.solve(L, Ks.T)
    mu = Ks @ alpha + gp["mean"]
    var = kdiag(T, gp["amp"], gp["lin_coef"], gp["lin_order"]) - np.sum(V * V, axis=0)
    return mu, var, L


def _kinds(kind, q):
    return [kind] * q if isinstance(kind, str) else list(kind)


def fantasy_step(X, T, b, beta, cols, v, gp):
    """One step of the recursion for the pick T[b] and a given beta: (C_j, v_j) from the earlier columns and v_{j-1}."""
    xj = T[b:b + 1]
    c = kernel(T, xj, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"])[:, 0] \
        - kernel(T, X, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"]) @ beta
    for ci in cols:
        c = c - ci * ci[b]
    ch = c / np.sqrt(v[b] + gp["diag_add"])
    return ch, v - ch * ch


def fantasy_batch(X, y, T, kind, q, gp, bounds=None, mask=None, zeta=0.01):
    """(indices, u, mu, vars): vars[j] is the variance after j fantasies."""
    kinds = _kinds(kind, q)
    ok = admissible(T, bounds, mask)
    mu, v, L = _predict(X, y, T, gp)
    ybest = float(np.max(y))
    idx, ub, vs, cols = [], [], [v], []
    u = np.where(ok, utility(kinds[0], mu, v, zeta, ybest), np.inf)
    for j in range(q):
        b = argmin(u)
        if b < 0:
            idx += [-1] * (q - j)
            ub += [np.inf] * (q - j)
            break
        idx.append(b)
        ub.append(float(u[b]))
        if j == q - 1:
            break
        ybest = max(ybest, float(mu[b]))
        kx = kernel(X, T[b:b + 1], gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"])[:, 0]
        beta = np.linalg.solve(L.T, np.linalg.solve(L, kx))
        ch, v = fantasy_step(X, T, b, beta, cols, v, gp)
        cols.append(ch)
        vs.append(v)
        u = np.where(ok, utility(kinds[j + 1], mu, v, zeta, ybest), np.inf)
    return np.array(idx), np.array(ub), mu, vs


def recondition_batch(X, y, T, kind, q, gp, bounds=None, mask=None, zeta=0.01):
    """The slow path: (indices, u, mus, vars, us) with mus / vars / us of every step."""
    kinds = _kinds(kind, q)
    ok = admissible(T, bounds, mask)
    Xe, ye = np.array(X, dtype=float), np.array(y, dtype=float)
    idx, ub, mus, vs, us = [], [], [], [], []
    for j in range(q):
        mu, v, _ = _predict(Xe, ye, T, gp)
        u = np.where(ok, utility(kinds[j], mu, v, zeta, float(np.max(ye))), np.inf)
        mus.append(mu)
        vs.append(v)
        us.append(u)
        b = argmin(u)
        if b < 0:
            idx += [-1] * (q - j)
            ub += [np.inf] * (q - j)
            break
        idx.append(b)
        ub.append(float(u[b]))
        Xe = np.vstack([Xe, T[b:b + 1]])
        ye = np.append(ye, mu[b])
    return np.array(idx), np.array(ub), mus, vs, us


# ----------------------------------------------------------------------------------------------------------------------
# One call of the fantasy pass for a given beta: truth, budget, restated device order
# ----------------------------------------------------------------------------------------------------------------------
# What fantasy_kernel does to candidate row t (csrc/sweep.hip; u = 2^-53):
#
#   tt = t sc                                   rounded once per coordinate (kvalue_ref's xs)
#   tile loop, tiles of FT_ROWS = 128 training rows, four rows r, r + 1, r + 2, r + 3 per step:
#       k_r = k(t, x_r)                          kvalue_ref's sequence through apgp_exp4 (apgp_exp's operations)
#       acc[r & 3] = fma(k_r, beta_r, acc[r & 3])
#     rows from n to the end of the last tile carry beta = 0 and zero coordinates (the packed stream's padding): they add
#     fma(k, 0, acc) = acc, exactly.
#   kx = k(t, x_j)                               the same sequence through apgp_exp, x_j = T[pick] sc
#   c  = kx - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
#   c  = fma(-C_i(t), C_i(x_j), c)               i = 0 .. j - 2, in this order
#   ch = c / sqrt(var_in[pick] + diag_add)       -> C_j(t)
#   v  = fma(-ch, ch, var_in[t])                 -> v_j(t)
#
# Budget of |C_j - truth|, term by term (first order; the sum carries 1 + 2^-20 for the second order):
#   dot      e_dot = sum_r kvalue_ref.budget(t, x_r) |beta_r|  +  (ceil(n / 4) + 2) u sum_r |k_r beta_r|.
#            A term sits in one of four fma chains of at most ceil(n / 4) links (one rounding each), then passes the two
#            levels of (a0 + a1) + (a2 + a3).  |k_r| is taken as |truth| + its budget.  Padding rows: exact, not charged.
#   kx       kvalue_ref.budget(t, x_j): zero beyond 2^-1074 for the pick row itself (coincident points are exact there).
#   c0       kx - dot rounds once: u |c0|.
#   downdate step i is one fma: u (|c0| + sum_{i' <= i} |C_i'(t) C_i'(x_j)|), the running magnitude.
#   ch       s = var_in[pick] + diag_add rounds once (relative u, halved by the root; not charged when the sum is exact,
#            as with diag_add = 0), the root once (not charged when sqrt(s)^2 == s exactly), the quotient once:
#            e_ch = e_c / sqrt(s) + (u/2 [add] + u [sqrt] + u [div]) |ch|.
#            fp64 sqrt and division are correctly rounded on the device (the OpenCL-conformant lowerings hipcc uses).
#   v        fma(-ch, ch, var_in) rounds once: e_v = 2 |ch| e_ch + e_ch^2 + u |v|.
#   truth    numpy.longdouble (64-bit significand): kvalue_ref.truth_ld is good to 2^-9 ulp of a double (2^-61 relative),
#            the dot adds n terms in long double (<= (n + 2) 2^-64 sum|k beta|), the downdate j - 1 (<= (j + 2) 2^-64 of
#            the running magnitude), root and quotient 4 x 2^-64: ``Pass.truth_error``.  About 2^-9 of the budget's own
#            leading term; ADDED to the budget, not argued away, and checked against mpmath in tests/test_fantasy_ref.py.
# A contraction of t sc into the subtraction (df = fma(t, sc, -xs), which hipcc is free to do in sweep.hip and is known to
# do at the sweep's site) removes a rounding: kvalue_ref.budget holds for it, and ``pass_restate(fused=True)`` restates it
# at both sites (tile loop and epilogue).
# Nothing here was fitted to device output, and nothing contains cond(K).
FT_ROWS = 128
LDU = 2.0 ** -64
U = kr.U
LD = np.longdouble
PASS_MUTANTS = ("drop_last_rows", "stale_tile", "beta_on_padding", "lane_drop", "skip_last_column", "cx_from_row",
                "no_diag_add", "s_from_var_out", "lin_tile_only")


def dot_depth(n):
    """Roundings on a term's way through the four fma chains and the pairing of the lane sums."""
    return (n + 3) // 4 + 2


class Pass(object):
    """k(T, X) of the DISTINCT rows of T in long double with its kvalue budget, shared by every call on the same
    (T, X, kern): truth and budget of one call each cost one more column k(T, x_j)."""

    def __init__(self, T, X, k):
        self.T = np.ascontiguousarray(np.atleast_2d(T), dtype=np.float64)
        self.X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        self.k, self.n, self.m = k, len(self.X), len(self.T)
        self.Tu, inv = np.unique(self.T, axis=0, return_inverse=True)
        self.inv = np.asarray(inv).reshape(-1)
        with np.errstate(all="ignore"):
            self.kh = kr.truth_ld(self.Tu, self.X, k)
            self.ek = kr.budget(self.Tu, self.X, k)
        self.akh = np.abs(self.kh).astype(np.float64)

    def _column(self, pick):
        xj = self.T[pick:pick + 1]
        with np.errstate(all="ignore"):
            return kr.truth_ld(self.Tu, xj, self.k)[:, 0], kr.budget(self.Tu, xj, self.k)[:, 0]

    def _parts(self, beta, pick, Cprev, var_in):
        beta = np.asarray(beta, dtype=np.float64)
        Cprev = np.asarray(Cprev, dtype=np.float64).reshape(-1, self.m)
        var_in = np.asarray(var_in, dtype=np.float64)
        kx, ekx = self._column(pick)
        dot = self.kh @ beta.astype(LD)
        c0 = (kx - dot)[self.inv]
        c = c0.copy()
        for i in range(len(Cprev)):
            c = c - Cprev[i].astype(LD) * LD(Cprev[i, pick])
        s = LD(var_in[pick]) + LD(self.k.diag_add)
        ch = c / np.sqrt(s)
        v = var_in.astype(LD) - ch * ch
        return beta, Cprev, var_in, kx, ekx, c0, s, ch, v

    def truth(self, beta, pick, Cprev, var_in):
        p = self._parts(beta, pick, Cprev, var_in)
        return p[7], p[8]

    def _magnitudes(self, beta, pick, Cprev, kx, c0):
        """(sum_r |k_r beta_r| with |k| + its budget, the running magnitudes of the downdate: before it, after step i)."""
        sab = ((self.akh + self.ek) @ np.abs(beta))[self.inv]
        run = [np.abs(c0).astype(np.float64)]
        for i in range(len(Cprev)):
            run.append(run[-1] + np.abs(Cprev[i] * Cprev[i, pick]))
        return sab, run

    def truth_error(self, beta, pick, Cprev, var_in):
        """Bound of the long-double truth's own error in (C_j, v_j) (derivation above)."""
        beta, Cprev, var_in, kx, ekx, c0, s, ch, v = self._parts(beta, pick, Cprev, var_in)
        sab, run = self._magnitudes(beta, pick, Cprev, kx, c0)
        akx = np.abs(kx).astype(np.float64)[self.inv]
        ec = (2.0 ** -61 + (self.n + 2) * LDU) * sab + 2.0 ** -61 * akx + (len(Cprev) + 2) * LDU * (run[-1] + sab + akx)
        ach = np.abs(ch).astype(np.float64)
        ech = ec / math.sqrt(float(s)) + 4.0 * LDU * ach
        return ech, 2.0 * ach * ech + ech * ech + 2.0 * LDU * (np.abs(var_in) + ach * ach)

    def budget(self, beta, pick, Cprev, var_in):
        """Per-row bounds (|C_j - truth|, |v_j - truth|) of the device's fp64 sequence, the truth's own error included."""
        beta, Cprev, var_in, kx, ekx, c0, s, ch, v = self._parts(beta, pick, Cprev, var_in)
        sab, run = self._magnitudes(beta, pick, Cprev, kx, c0)
        e_dot = (self.ek @ np.abs(beta))[self.inv] + dot_depth(self.n) * U * sab
        ec = e_dot + ekx[self.inv] + U * run[0]
        for r in run[1:]:
            ec = ec + U * r
        ec = ec * sr.SECOND
        sf = var_in[pick] + self.k.diag_add
        _, e_add = kr._two_sum(float(var_in[pick]), float(self.k.diag_add))
        rt = math.sqrt(sf)
        p, e_rt = kr._two_prod(rt, rt)
        rel = (0.0 if e_add == 0.0 else 0.5 * U) + (0.0 if (p == sf and e_rt == 0.0) else U) + U
        ach = np.abs(ch).astype(np.float64)
        ech = (ec / rt + rel * ach) * sr.SECOND
        ev = (2.0 * ach * ech + ech * ech + U * np.abs(v).astype(np.float64)) * sr.SECOND
        tC, tv = self.truth_error(beta, pick, Cprev, var_in)
        return ech + tC, ev + tv


def pass_truth(T, X, beta, k, pick, Cprev, var_in, ctx=None):
    """(C_j, v_j) of every row of T in numpy.longdouble, from the bits of the arguments.  ``Cprev``: the earlier columns,
    (j - 1) x m.  ``ctx``: a Pass of the same (T, X, k) to share k(T, X)."""
    return (ctx or Pass(T, X, k)).truth(beta, pick, Cprev, var_in)


def pass_budget(T, X, beta, k, pick, Cprev, var_in, ctx=None):
    """Per-row bounds (|C_j - truth|, |v_j - truth|); the derivation is the comment block above."""
    return (ctx or Pass(T, X, k)).budget(beta, pick, Cprev, var_in)


def pass_numpy(T, X, beta, k, pick, Cprev, var_in):
    """The same call in plain float64 NumPy (``fantasy_step``: the recursion of fantasy_batch)."""
    gp = {"amp": k.amp, "inv_metric": k.inv_metric, "lin_coef": k.lin_coef, "lin_order": k.lin_order, "diag_add": k.diag_add}
    Cprev = np.asarray(Cprev, dtype=np.float64).reshape(-1, len(T))
    return fantasy_step(np.asarray(X), np.asarray(T), pick, np.asarray(beta), list(Cprev), np.asarray(var_in), gp)


def _lin_sum(tts, xc, lw, k):
    """APGP_LIN_SUM as written (no contraction: a contracted form has fewer roundings)."""
    if k.lin_order == 0:
        return float(k.ndim)
    ls = 0.0
    for d in range(len(tts)):
        p = tts[d] * xc[d] * lw[d]
        q = p
        for _ in range(1, k.lin_order):
            q *= p
        ls += q
    return ls


def _kval(traw, tts, xc, k, kse, sc, lw, fused, lin=True):
    """k(t, x) as the pass forms it at either site: the squared-exponential part by kvalue_ref.value_restate (``fused``:
    the candidate's scaling contracted into the subtraction), the linear term always from the scaled tt."""
    v = kr.value_restate(traw if fused else tts, xc, kse, lw, False, None, sc if fused else None)
    if lin and k.lin_coef != 0.0:
        v = kr.fma(k.lin_coef, _lin_sum(tts, xc, lw, k), v)
    return v


def pass_restate(T, X, beta, k, pick, Cprev, var_in, rows=None, fused=False, mutant=None, var_out0=None):
    """(C_j, v_j) of ``rows`` of T (default: all; exact rational arithmetic per fma is slow) in fantasy_kernel's order:
    tiles of 128 training rows, four lanes, (a0 + a1) + (a2 + a3), the epilogue and the downdate as listed above.
    ``fused``: df = fma(t, sc, -xs) at both sites.  ``var_out0``: what the output variance buffer held before the call
    (mutant "s_from_var_out").  ``mutant``: one of PASS_MUTANTS."""
    if mutant is not None and mutant not in PASS_MUTANTS:
        raise ValueError(mutant)
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, m, D = len(X), len(T), k.ndim
    Cprev = np.asarray(Cprev, dtype=np.float64).reshape(-1, m)
    rows = range(m) if rows is None else rows
    sc, lw = kr.kernconst(k)
    dp = len(sc)
    kse = k._replace(lin_coef=0.0)
    ntile = (n + FT_ROWS - 1) // FT_ROWS
    xs = kr._scaled(X, sc, D, dp, None) + [[0.0] * dp for _ in range(ntile * FT_ROWS - n)]
    bt = [float(b) for b in beta] + [float(beta[n - 1]) if mutant == "beta_on_padding" else 0.0] * (ntile * FT_ROWS - n)
    live_end = n - (n % 4) if mutant == "drop_last_rows" else n
    xj = kr._scaled(T[pick:pick + 1], sc, D, dp, None)[0]
    nd = len(Cprev) - (1 if mutant == "skip_last_column" else 0)
    sv = float(var_out0[pick]) if mutant == "s_from_var_out" else float(var_in[pick])
    s = sv if mutant == "no_diag_add" else sv + k.diag_add
    outC, outv = [], []
    for row in rows:
        traw = [float(T[row, d]) if d < D else 0.0 for d in range(dp)]
        tts = [traw[d] * sc[d] for d in range(dp)]
        acc = [0.0, 0.0, 0.0, 0.0]
        for ti in range(ntile):
            src = ti - 1 if (mutant == "stale_tile" and ti >= 1) else ti
            for r in range(FT_ROWS):
                R = src * FT_ROWS + r
                if bt[R] == 0.0 or (ti * FT_ROWS + r >= live_end and mutant == "drop_last_rows"):
                    continue                                     # fma(k, 0, acc) = acc
                kv = _kval(traw, tts, xs[R], k, kse, sc, lw, fused)
                acc[r & 3] = kr.fma(kv, bt[R], acc[r & 3])
        kx = _kval(traw, tts, xj, k, kse, sc, lw, fused, lin=mutant != "lin_tile_only")
        if mutant == "lane_drop":
            c = kx - ((acc[0] + acc[1]) + acc[2])
        else:
            c = kx - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        for i in range(nd):
            cx = float(Cprev[i, row]) if mutant == "cx_from_row" else float(Cprev[i, pick])
            c = kr.fma(-float(Cprev[i, row]), cx, c)
        ch = c / math.sqrt(s)
        outC.append(ch)
        outv.append(kr.fma(-ch, ch, float(var_in[row])))
    return np.array(outC), np.array(outv)


# ----------------------------------------------------------------------------------------------------------------------
# cases (seeded): the CPU test and the GPU test run the same inputs
# ----------------------------------------------------------------------------------------------------------------------
PASS_N = (1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 512, 513)
PASS_M = (1, 255, 256, 257, 1000)
PASS_D = (1, 3, 5, 8, 9, 16, 17, 32)
PASS_LIN = tuple((P, D) for P in (0, 1, 2) for D in (3, 8, 32))
PASS_J = (1, 2, 31)
DIAG_ADD = 0.01

Case = collections.namedtuple("Case", "name n D order m j pick kind")


def _case(name, n, D, order=None, m=257, j=2, pick=None, kind="planted"):
    return Case(name, n, D, order, m, j, (5 * m) // 7 if pick is None else pick, kind)


N_CASES = tuple(_case("n%d-D8" % n, n, 8) for n in PASS_N) + tuple(_case("n%d-D3-P1" % n, n, 3, 1) for n in PASS_N)
D_CASES = tuple(_case("D%d" % D, 129, D) for D in PASS_D)
LIN_CASES = tuple(_case("P%d-D%d" % (P, D), 129, D, P) for P, D in PASS_LIN)
M_CASES = tuple(_case("m%d" % m, 129, 8, m=m) for m in PASS_M)
J_CASES = tuple(_case("j%d" % j, 257, 8, j=j) for j in PASS_J)
# the downdate with the pick row in the first workgroup, in the last one and at m - 1 (three workgroups of 256 rows)
DOWNDATE_M = 600
DOWNDATE_CASES = tuple(_case("j%d-pick%d" % (j, p), 257, 8, m=DOWNDATE_M, j=j, pick=p)
                       for j in PASS_J for p in (5, 520, DOWNDATE_M - 1))
REALISTIC = _case("realistic", 129, 8, j=1, pick=3, kind="realistic")
BUDGET_CASES = N_CASES + D_CASES + LIN_CASES + M_CASES + J_CASES + (REALISTIC,)
ALL_CASES = BUDGET_CASES + DOWNDATE_CASES
CASE_BY_NAME = {c.name: c for c in ALL_CASES}
assert len(CASE_BY_NAME) == len(ALL_CASES)
# (mutant, case that has to catch it): the tail rows 128 / the second tile / the padding of the last tile / lane 3 /
# an earlier column / a non-zero diag_add / a linear term must be there for the defect to show
MUTANT_CASES = (("drop_last_rows", "n129-D8"), ("drop_last_rows", "n5-D8"), ("stale_tile", "n129-D8"), ("stale_tile", "n257-D8"),
                ("beta_on_padding", "n129-D3-P1"), ("beta_on_padding", "P0-D3"), ("lane_drop", "n4-D8"), ("lane_drop", "n129-D8"),
                ("skip_last_column", "j2"), ("skip_last_column", "j31"), ("cx_from_row", "j2"), ("cx_from_row", "j31"),
                ("no_diag_add", "n129-D8"), ("s_from_var_out", "n129-D8"), ("lin_tile_only", "P0-D3"),
                ("lin_tile_only", "P1-D8"), ("lin_tile_only", "P2-D32"))


def planted_beta(rs, n):
    """Mixed signs, magnitudes log-uniform over four decades; no entry is zero (the tail rows n mod 4 included)."""
    return rs.choice([-1.0, 1.0], size=n) * 10.0 ** rs.uniform(-2.0, 2.0, size=n)


def _chol_ld(K):
    K = np.array(K, dtype=LD)
    n = len(K)
    L = np.zeros((n, n), dtype=LD)
    for i in range(n):
        L[i, i] = np.sqrt(K[i, i] - L[i, :i] @ L[i, :i])
        if i + 1 < n:
            L[i + 1:, i] = (K[i + 1:, i] - L[i + 1:, :i] @ L[i, :i]) / L[i, i]
    return L


_INPUTS = {}


def pass_inputs(case):
    """dict(X, T (m x D, BASE distinct rows tiled), k, beta, pick, Cprev ((j - 1) x m), var_in, var_out0, mu) of a case;
    built once per process and never changed.
    planted:   sweep_ref.case's points (candidates from next to a training point out to many length scales), diag_add =
               DIAG_ADD; beta, the earlier columns (mixed signs, two decades, different on every row -- repeated
               candidates included) and var_in are planted: var_in is the float64 estimate of C_j^2 times 0.3 .. 3 plus a
               positive part, so that v_j comes out on either side of zero and var_in[pick] + diag_add > 0.
    realistic: beta = K^-1 k(X, x_j) solved in long double (Cholesky) and rounded to double, x_j a candidate beside a
               training point, var_in the model's own posterior variance: c nearly cancels beside the training points."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    rs = np.random.RandomState(9000 + 7 * case.n + 131 * case.D + 17 * case.m + case.j + (0 if case.order is None else 1000 * (case.order + 1)))
    X, _, Tb, k, _ = sr.case(case.n, case.D, case.order)
    k = k._replace(diag_add=DIAG_ADD)
    T = sr.tiled(Tb, case.m)
    m, n = case.m, case.n
    Cprev = rs.choice([-1.0, 1.0], size=(case.j - 1, m)) * 10.0 ** rs.uniform(-1.5, 0.5, size=(case.j - 1, m))
    if case.kind == "realistic":
        with np.errstate(all="ignore"):
            L = _chol_ld(kr.truth_ld(X, None, k))
            ks = kr.truth_ld(X, Tb, k)                                   # n x BASE
        V = _solve_lower_ld(L, ks)
        ktt, _ = sr.ktt_truth(Tb, k)
        v0 = (ktt - (V * V).sum(0)).astype(np.float64)
        beta = _solve_upper_ld(L, V[:, case.pick % len(Tb)]).astype(np.float64)
        var_in = v0[np.arange(m) % len(Tb)]
        assert var_in[case.pick] > 0.0
    else:
        beta = planted_beta(rs, n)
        var_in = np.ones(m)
        est, _ = pass_numpy(T, X, beta, k, case.pick, Cprev, var_in)     # (s = 1 + diag_add: rescaled below)
        s0 = k.amp * rs.uniform(0.2, 2.0)
        est = est * math.sqrt(1.0 + k.diag_add) / math.sqrt(s0 + k.diag_add)
        var_in = est * est * rs.uniform(0.3, 3.0, size=m) + k.amp * rs.uniform(0.01, 1.0, size=m)
        var_in[case.pick] = s0
    out = {"X": X, "T": T, "k": k, "beta": beta, "pick": case.pick, "Cprev": Cprev, "var_in": var_in,
           "var_out0": 1.37 * var_in + 0.1, "mu": rs.normal(size=m)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _INPUTS[case.name] = out
    return out


def _solve_lower_ld(L, B):
    V = np.array(B, dtype=LD)
    for i in range(len(L)):
        if i:
            V[i] -= L[i, :i] @ V[:i]
        V[i] /= L[i, i]
    return V


def _solve_upper_ld(L, b):
    """L^-T b."""
    x = np.array(b, dtype=LD)
    for i in range(len(L) - 1, -1, -1):
        if i + 1 < len(L):
            x[i] -= L[i + 1:, i] @ x[i + 1:]
        x[i] /= L[i, i]
    return x


def pass_args(inp):
    """The positional arguments of pass_truth / pass_budget / pass_restate / pass_numpy."""
    return inp["T"], inp["X"], inp["beta"], inp["k"], inp["pick"], inp["Cprev"], inp["var_in"]


def restate_rows(case):
    """The rows of a case that the (slow) restatement is run on: the pick, its neighbours, the candidates beside a
    training point, the last row and a stride through the rest."""
    m = case.m
    rows = {0, 1, 2, 3, case.pick, max(case.pick - 1, 0), min(case.pick + 1, m - 1), m - 1}
    rows.update(range(7, m, max(1, m // 6)))
    return sorted(r for r in rows if r < m)


def ratio(got, truth, bud):
    """Worst |got - truth| / budget over the rows (inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float((np.abs(got.astype(LD) - truth).astype(np.float64) / bud).max())
