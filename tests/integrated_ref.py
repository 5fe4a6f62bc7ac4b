# -*- coding: utf-8 -*-
"""Reference of ONE call of the integrated acquisition pass (apgp_acquire_integrated, csrc/integrated.hip; DESIGN.md
"Integrated acquisition").  Plain Python (NumPy, tests/kvalue_ref.py): no GPU, no library import.

    c_j(t) = k(t, r_j) - sum_n k(t, x_n) B[n, j]        s(t) = var(t) + diag_add        tau_j^2(t) = c_j(t)^2 / s(t)
    u(t)   = -log sum_j exp(a_j + tau_j^2(t))

B, a and var are INPUTS: B is planted, not solved for, so nothing in the bar depends on cond(K).

``truth``    c, tau^2 and u in numpy.longdouble from the bits of the arguments (kernel values: kvalue_ref.truth_ld).
``budget``   componentwise bounds of |device c - truth| and |device u - truth| counted off the kernel's operation order.
``restate``  the device's operation order (the vector form) with kvalue_ref's exactly rounded fma, and the mutants the
             budget has to catch.
``recondition`` the identity tau_j^2(t) = var(r_j) - var'(r_j), var' recomputed from scratch with t appended to the
             training set, in long double and in float64: the bar of the API-level comparison.

What the kernel does to candidate row t (u = 2^-53; every product and sum rounds where written, contraction off):

  tt = t sc, rs = r_j sc                    rounded once per coordinate (kvalue_ref's xs)
  per column j, over the training rows in order (tiles of 64 rows; rows past n carry B = 0: fma(k, 0, acc) = acc):
      k_n = k(t, x_n)                       kvalue_ref's sequence (apgp_gram_value's bits)
      acc = fma(k_n, B[n, j], acc)          the vector form: one chain of n links; the matrix-core form adds the four
                                            products of a 4-row step to the running sum in one instruction -- no more
                                            roundings per summand than one fma each (as tests/pathdraw_ref.py)
  kx  = k(t, r_j)                           the same sequence
  c   = kx - acc
  s   = var + diag_add
  e   = a_j + (c c) / s
  running (max, sum) over j ascending, skipping e = -inf:   d = e - mx;  x = apgp_exp(-|d|);
      d > 0: sm = fma(sm, x, 1), mx = e     else: sm = sm + x
  u   = -(mx + log(sm))

Budget, term by term (first order; the c part carries 1 + 2^-20 for the second order):
  c     e_c = sum_n kvalue_budget(t, x_n) |B[n,j]| + kvalue_budget(t, r_j)
              + (n + 1) u (|k(t, r_j)| + sum_n |k(t, x_n)| |B[n,j]|):
        a summand passes at most n roundings of the chain and the one of the subtraction, each at most u times a partial
        sum bounded by the sum of magnitudes (|k| taken as |truth| + its budget).
  e     s rounds once (not charged when the sum is exact), the square once, the quotient once (fp64 division is
        correctly rounded on the device), the sum with a_j once:
        e_e = (2 |c| e_c + e_c^2) / s + 3 u tau^2 + u |e|.
  u     a log-sum-exp moves by at most max_j e_e.  The running pair: a term's factor exp(e_j - mx) is formed as a product
        of at most J exponentials whose arguments telescope to e_j - max: each carries the rounding of its argument
        (u |d|, together u (max - e_j), and (max - e_j) exp(-(max - e_j)) <= 1/e against a sum >= 1), E_EXP ulp <= 4 u with
        the rounding of its fma or sum; the running sum rounds at most 2 J times.  Relative error of the sum below
        (4 (J + 1) + J / e + 2 J) u <= (7 J + 4) u, which is its absolute effect on log(sum).  apgp_exp's clamp returns
        1e-304 for an argument below -700: J 1e-303.  log rounds within an ulp (2 u |log sum|), the closing sum and
        negation once (u |u|).
  truth kvalue_ref.truth_ld is good to 2^-61 relative, the dot adds n terms in long double ((n + 2) 2^-64 of the
        magnitudes), quotient and sums 4 x 2^-64; through the same propagation as above.  ADDED to the budget.
Nothing here was fitted to device output, and nothing contains cond(K).
"""
import collections
import math

import numpy as np

import fantasy_ref as fr
import kvalue_ref as kr
import sweep_ref as sr

U = kr.U
LD = np.longdouble
LDU = 2.0 ** -64
SECOND = sr.SECOND
MAX_REFS = 4096
THREADS = 256             # candidates per workgroup (IV_THREADS)
TILE = 64                 # training rows per LDS tile (IV_ROWS)
COLUMN_TILES = (16, 32, 64)   # columns per pass: the vector form 16, the matrix-core form 16 / 32 / 64 by J
MUTANTS = ("no_kr", "no_diag_add", "col_shift", "no_a", "drop_last_row", "drop_tile_edge")


def work_len(m, nref):
    """apgp_integrated_work_len."""
    if m < 0 or m > 1 << 40 or nref < 1 or nref > MAX_REFS:
        return -1
    return 2 * ((m + THREADS - 1) // THREADS)


def admissible(T, var, diag_add, bounds=None, mask=None):
    T = np.asarray(T, dtype=np.float64)
    adm = ~np.isnan(T).any(axis=1)
    if bounds is not None:
        bb = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore"):
            adm &= np.all((T >= bb[:, 0]) & (T <= bb[:, 1]), axis=1)
    if mask is not None:
        adm &= np.asarray(mask).astype(bool)
    with np.errstate(invalid="ignore"):
        s = np.asarray(var, dtype=np.float64) + diag_add
        adm &= (s > 0.0) & (s < np.inf)
    return adm


def argmin(u, idx_offset=0):
    """The sweep's arg-min contract on an array of u: (global index, u); NaN and +inf never win, ties go to the lowest
    index; (-1, +inf) if nothing is left."""
    w = np.where(np.isnan(u), np.inf, np.asarray(u, dtype=np.float64))
    if not np.any(w < np.inf):
        return -1, np.inf
    i = int(np.argmin(w))
    return idx_offset + i, float(w[i])


def _lse_ld(e):
    """-log sum_j exp(e_j) per row of an (m, J) long-double array (-inf entries contribute nothing)."""
    mx = e.max(axis=1)
    with np.errstate(invalid="ignore"):
        sm = np.exp(e - mx[:, None]).sum(axis=1)
    return -(mx + np.log(sm)), mx, sm


class Pass(object):
    """k(T, X) and k(T, R) of the DISTINCT rows of T in long double with their kvalue budgets, shared by every call on
    the same (T, X, R, kern)."""

    def __init__(self, T, X, R, k):
        self.T = np.ascontiguousarray(np.atleast_2d(T), dtype=np.float64)
        self.X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        self.R = np.ascontiguousarray(np.atleast_2d(R), dtype=np.float64)
        self.k, self.n, self.m, self.J = k, len(self.X), len(self.T), len(self.R)
        self.Tu, inv = np.unique(self.T, axis=0, return_inverse=True)
        self.inv = np.asarray(inv).reshape(-1)
        with np.errstate(all="ignore"):
            self.kh = kr.truth_ld(self.Tu, self.X, k)
            self.ek = kr.budget(self.Tu, self.X, k)
            self.krh = kr.truth_ld(self.Tu, self.R, k)
            self.ekr = kr.budget(self.Tu, self.R, k)
        self.akh = np.abs(self.kh).astype(np.float64)
        self.akr = np.abs(self.krh).astype(np.float64)

    def truth(self, B, a, var):
        """(c (m, J), tau^2 (m, J), u (m,)) in long double."""
        B = np.asarray(B, dtype=np.float64).reshape(self.n, self.J)
        c = (self.krh - self.kh @ B.astype(LD))[self.inv]
        s = np.asarray(var, dtype=np.float64).astype(LD) + LD(self.k.diag_add)
        tau2 = c * c / s[:, None]
        u, _, _ = _lse_ld(np.asarray(a, dtype=np.float64).astype(LD)[None, :] + tau2)
        return c, tau2, u

    def budget(self, B, a, var):
        """(bound of |c - truth| (m, J), bound of |u - truth| (m,)), the truth's own error included."""
        B = np.asarray(B, dtype=np.float64).reshape(self.n, self.J)
        a = np.asarray(a, dtype=np.float64)
        var = np.asarray(var, dtype=np.float64)
        aB = np.abs(B)
        c, tau2, u = self.truth(B, a, var)
        mag = (self.akr + self.ekr + (self.akh + self.ek) @ aB)[self.inv]
        ec = ((self.ek @ aB + self.ekr)[self.inv] + (self.n + 1) * U * mag) * SECOND
        tc = (2.0 ** -61 + (self.n + 2) * LDU) * mag
        ec = ec + tc
        s = var + self.k.diag_add
        e_add = np.array([kr._two_sum(float(v), float(self.k.diag_add))[1] for v in var])
        ac = np.abs(c).astype(np.float64)
        t2 = tau2.astype(np.float64)
        e = a[None, :] + t2
        with np.errstate(invalid="ignore"):
            ee = (2.0 * ac * ec + ec * ec) / s[:, None] + (2.0 + (e_add != 0.0)[:, None]) * U * t2 \
                + U * np.where(np.isfinite(e), np.abs(e), 0.0) + 4.0 * LDU * (t2 + np.abs(np.where(np.isfinite(e), e, 0.0)))
        ee = np.where(np.isfinite(a)[None, :], ee, 0.0)            # a column with a = -inf contributes nothing
        _, mx, sm = _lse_ld(a.astype(LD)[None, :] + tau2)
        lsm = np.abs(np.log(sm)).astype(np.float64)
        J = self.J
        eu = ee.max(axis=1) * SECOND + (7 * J + 4) * U + J * 1e-303 + 2.0 * U * lsm + U * np.abs(u).astype(np.float64) \
            + (J + 4) * LDU * (1.0 + np.abs(u).astype(np.float64))
        return ec, eu


def numpy_pass(T, X, R, B, a, var, k):
    """The same call in plain float64 NumPy (fantasy_ref.kernel, scipy-free log-sum-exp)."""
    Ktx = fr.kernel(T, X, k.amp, k.inv_metric, k.lin_coef, k.lin_order)
    Ktr = fr.kernel(T, R, k.amp, k.inv_metric, k.lin_coef, k.lin_order)
    c = Ktr - Ktx @ np.asarray(B)
    e = np.asarray(a)[None, :] + c * c / (np.asarray(var) + k.diag_add)[:, None]
    mx = e.max(axis=1)
    return c, -(mx + np.log(np.exp(e - mx[:, None]).sum(axis=1)))


def _kval(tts, xc, k, kse, lw):
    v = kr.value_restate(tts, xc, kse, lw, False)
    if k.lin_coef != 0.0:
        v = kr.fma(k.lin_coef, _lin_sum(tts, xc, lw, k), v)
    return v


def _lin_sum(tts, xc, lw, k):
    """APGP_LIN_SUM with the product associated as apgp_gram_value has it: (t x) lw."""
    if k.lin_order == 0:
        return float(k.ndim)
    ls = 0.0
    for d in range(len(tts)):
        p = (tts[d] * xc[d]) * lw[d]
        q = p
        for _ in range(1, k.lin_order):
            q *= p
        ls += q
    return ls


def restate(T, X, R, B, a, var, k, rows=None, mutant=None):
    """(c (len(rows), J), u (len(rows),)) of ``rows`` of T (default: all; exact rational arithmetic per fma is slow) in
    the vector form's order.  ``mutant``: one of MUTANTS."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    B = np.asarray(B, dtype=np.float64)
    n, m, J, D = len(X), len(T), len(R), k.ndim
    rows = range(m) if rows is None else rows
    sc, lw = kr.kernconst(k)
    dp = len(sc)
    kse = k._replace(lin_coef=0.0)
    xs = kr._scaled(X, sc, D, dp, None)
    rs = kr._scaled(R, sc, D, dp, None)
    skip = {n - 1} if mutant == "drop_last_row" else {TILE} if mutant == "drop_tile_edge" else set()
    outc, outu = [], []
    for row in rows:
        tts = [float(T[row, d]) * sc[d] if d < D else 0.0 for d in range(dp)]
        kv = [_kval(tts, xs[r], k, kse, lw) for r in range(n)]
        s = float(var[row]) if mutant == "no_diag_add" else float(var[row]) + k.diag_add
        mx, sm = -math.inf, 0.0
        crow = []
        for j in range(J):
            jb = (j + 1) % J if mutant == "col_shift" else j
            acc = 0.0
            for r in range(n):
                if r in skip or B[r, jb] == 0.0:
                    continue                                         # fma(k, 0, acc) = acc
                acc = kr.fma(kv[r], float(B[r, jb]), acc)
            kx = 0.0 if mutant == "no_kr" else _kval(tts, rs[j], k, kse, lw)
            c = kx - acc
            crow.append(c)
            e = (0.0 if mutant == "no_a" and a[j] > -math.inf else float(a[j])) + (c * c) / s
            if e != -math.inf:
                d = e - mx
                gt = d > 0.0
                x = kr.exp_restate(-d if gt else d)
                sm = kr.fma(sm, x, 1.0) if gt else sm + x
                mx = e if gt else mx
        outc.append(crow)
        outu.append(-(mx + math.log(sm)) if sm > 0.0 else math.inf)
    return np.array(outc).reshape(len(outc), J), np.array(outu)


def ratio(got, truth, bud):
    """Worst |got - truth| / budget (inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float((np.abs(got.astype(LD) - truth).astype(np.float64) / bud).max())


# ----------------------------------------------------------------------------------------------------------------------
# cases (seeded): the CPU test and the GPU test run the same inputs
# ----------------------------------------------------------------------------------------------------------------------
PASS_N = (1, 63, 64, 65, 511, 513)
PASS_M = (1, 255, 256, 257)
PASS_D = (1, 2, 3, 4, 8, 9, 16)          # (the pass takes at most 16 dimensions)
PASS_LIN = ((1, 3), (2, 8), (1, 16))
# J = 1, both sides of every column-tile width (16 / 32 / 64), three passes of the widest tile
PASS_J = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
PASS_J_VECTOR = (15, 16, 17, 33)          # the vector form (D > 8, or the test switch): tiles of 16
DIAG_ADD = 0.01

Case = collections.namedtuple("Case", "name n D order m J spread")


def _case(name, n=129, D=8, order=None, m=257, J=40, spread=1e3):
    return Case(name, n, D, order, m, J, spread)


N_CASES = tuple(_case("n%d" % n, n=n) for n in PASS_N)
M_CASES = tuple(_case("m%d" % m, m=m, spread=2.0) for m in PASS_M)
D_CASES = tuple(_case("D%d" % D, D=D, J=20, spread=2.0 if D & 1 else 1e3) for D in PASS_D)
LIN_CASES = tuple(_case("P%d-D%d" % (P, D), D=D, order=P, J=20) for P, D in PASS_LIN)
J_CASES = tuple(_case("J%d" % J, n=65, J=J, spread=2.0 if J & 1 else 1e3) for J in PASS_J)
JV_CASES = tuple(_case("J%d-D9" % J, n=65, D=9, J=J) for J in PASS_J_VECTOR)
MAX_CASE = _case("Jmax", n=64, m=64, J=MAX_REFS)
ALL_CASES = N_CASES + M_CASES + D_CASES + LIN_CASES + J_CASES + JV_CASES + (MAX_CASE,)
CASE_BY_NAME = {c.name: c for c in ALL_CASES}
assert len(CASE_BY_NAME) == len(ALL_CASES)
# the restatement (slow) runs on these, and these catch the mutants: a second tile for the tile-edge row, two columns at
# least for the shift
RESTATE_CASES = ("n65", "n1", "J17", "J1", "P1-D3", "D9")
MUTANT_CASES = tuple((mu, c) for mu in MUTANTS for c in (("m257", "D8") if mu == "drop_tile_edge" else ("n65", "J17")))

_INPUTS = {}


def inputs(case):
    """dict(X, T (m x D, sweep_ref.BASE distinct rows tiled), R, k, B, a, var) of a case; built once per process and
    never changed.  sweep_ref.case's points, diag_add = DIAG_ADD; the reference points sit beside candidates and training
    points (k(t, r_j) runs from nearly amp down through many decades); B has mixed signs and magnitudes over three
    decades, no entry zero; a is uniform over ``spread``; var is chosen per row so that the largest tau^2 of the row is
    spread evenly in the logarithm over 1 .. 2000: the exponents differ by 700 and more on some rows and by less than one on others."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    rs = np.random.RandomState(12000 + 7 * case.n + 131 * case.D + 17 * case.m + 3 * case.J
                               + (0 if case.order is None else 1000 * (case.order + 1)))
    X, _, Tb, k, _ = sr.case(case.n, case.D, case.order)
    k = k._replace(diag_add=DIAG_ADD)
    T = sr.tiled(Tb, case.m)
    ell = 1.0 / np.sqrt(k.inv_metric)
    pool = np.vstack([Tb, X])
    R = pool[rs.randint(len(pool), size=case.J)] + 0.3 * ell * rs.normal(size=(case.J, case.D))
    B = rs.choice([-1.0, 1.0], size=(case.n, case.J)) * 10.0 ** rs.uniform(-2.0, 1.0, size=(case.n, case.J)) / math.sqrt(case.n)
    a = case.spread * rs.uniform(-0.5, 0.5, size=case.J)
    c_est, _ = numpy_pass(T, X, R, B, a, np.ones(case.m), k)
    s = (c_est * c_est).max(axis=1) / 10.0 ** rs.permutation(np.linspace(0.0, math.log10(2000.0), case.m))
    var = s - k.diag_add                        # (below zero where s < diag_add: the pass only asks for s > 0)
    out = {"X": X, "T": T, "R": R, "k": k, "B": B, "a": a, "var": var}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _INPUTS[case.name] = out
    return out


def args(inp):
    """The positional arguments of numpy_pass / restate."""
    return inp["T"], inp["X"], inp["R"], inp["B"], inp["a"], inp["var"], inp["k"]


_CTX = {}


def context(case):
    """(inputs, Pass, (c, tau^2, u) truth, (c, u) budget) of a case, computed once per process."""
    if case.name not in _CTX:
        inp = inputs(case)
        P = Pass(inp["T"], inp["X"], inp["R"], inp["k"])
        _CTX[case.name] = (inp, P, P.truth(inp["B"], inp["a"], inp["var"]), P.budget(inp["B"], inp["a"], inp["var"]))
    return _CTX[case.name]


def restate_rows(case):
    """The rows the (slow) restatement runs on: candidates beside a training point, the last row, a stride."""
    m = case.m
    return sorted({0, 3, m - 1} | set(range(7, m, max(1, m // 3))))


# ----------------------------------------------------------------------------------------------------------------------
# the identity tau_j^2(t) = var(r_j) - var'(r_j)
# ----------------------------------------------------------------------------------------------------------------------
def recondition(X, R, t, k):
    """(tau^2 (J,) long double from c and s, var(r) - var'(r) in long double with t appended to the training set and the
    Cholesky factor recomputed from scratch, the same difference in plain float64 NumPy).  var' is conditioned on an
    observation at t with noise diag_add, hyper-parameters unchanged."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    t = np.asarray(t, dtype=np.float64).reshape(1, -1)

    def var_ld(Xs, P):
        L = fr._chol_ld(kr.truth_ld(Xs, None, k))
        V = fr._solve_lower_ld(L, kr.truth_ld(Xs, P, k))
        ktt, _ = sr.ktt_truth(P, k)
        return ktt - (V * V).sum(0), L

    vr, L = var_ld(X, R)
    vr2, _ = var_ld(np.vstack([X, t]), R)
    Bt = fr._solve_lower_ld(L, kr.truth_ld(X, t, k))                   # L^-1 k(X, t)
    Br = fr._solve_lower_ld(L, kr.truth_ld(X, R, k))                   # L^-1 k(X, R)
    c = kr.truth_ld(t, R, k)[0] - (Bt[:, 0][:, None] * Br).sum(0)
    ktt, _ = sr.ktt_truth(t, k)
    s = ktt[0] - (Bt[:, 0] * Bt[:, 0]).sum() + LD(k.diag_add)
    gp = {"amp": k.amp, "inv_metric": k.inv_metric, "lin_coef": k.lin_coef, "lin_order": k.lin_order, "diag_add": k.diag_add,
          "mean": 0.0}
    v64 = fr._predict(X, np.zeros(len(X)), R, gp)[1] - fr._predict(np.vstack([X, t]), np.zeros(len(X) + 1), R, gp)[1]
    return c * c / s, vr - vr2, v64
