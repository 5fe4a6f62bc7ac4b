"""NumPy restatement of ``apgp_predict_grad`` (include/apgp.h): the kernel of ``apgp_kernel_t`` with its linear term and
its derivative in the query point, the posterior mean / variance and their gradients through both K^-1 routes (SciPy
triangular solves), the utilities with their (mu, var) derivatives, and the non-finite table.  The checker of
tests/test_predgrad_ref.py and tests/test_gpu_predict_grad.py, never the thing shipped.

    k_n = k(t, x_n)                      J_nd   = d k(t, x_n) / d t_d
    mu  = k.alpha + mean                 dmu_d  = sum_n alpha_n J_nd
    v   = L^-1 k,  w = L^-T v            var    = k(t,t) - |v|^2
    dvar_d = d k(t,t) / d t_d - 2 sum_n w_n J_nd

Stage budgets of ``apgp_predict_grad`` (csrc/predgrad.hip), second half of this module
-------------------------------------------------------------------------------------
Every kernel of the call is judged alone, on the bits it was handed, which the call leaves in the caller's ``work``
(``work_views``).  u = 2^-53; a count is the largest number of roundings a TERM of a sum passes through on its way to the
output, read off the source line named beside it; every product below is the first half of an fma and does not round.
Nothing here was fitted to device output and no condition number appears.  A first-order bound is multiplied by
SECOND = 1 + 2^-20 for the second order.

k   pg_kstar_kernel (predgrad.hip:66-113).  pg_kse / pg_kval restate apgp_gram_value operation by operation -- tt = T sc
    rounds once (:100, contraction is off, :29), df = tt - xs, one fma lane over the even and one over the odd
    coordinates, amp * apgp_exp(-(q0 + q1)), fma(lin_coef, ls, .) with ls += ((tt xs) lw)^P -- which is kvalue_ref's
    site "cross" (tests/test_gpu_predict_grad_budget.py prints how many values of kbuf have its bits).  Budget:
    kvalue_ref.budget(T, X, kern), truth kvalue_ref.truth_ld.  kbuf[p, n:ns] == +0.0 exactly (:111).
v   pg_fwd_body (:131-170).  Lane l of row i's wavefront runs the chains ax (even k) and ay (odd k) over k = 2 l + 128 j
    <= i: (i + 128) // 128 links at most (lane 0; the masked columns past i add exact zeros), ax + ay (:160) one, six
    shuffle levels (:161-164) six:
        FWD_DEPTH_i = (i + 128) // 128 + 1 + 6,     |v_i - sum_k W_ik k_k| <= u FWD_DEPTH_i sum_k |W_ik k_k|.
w   pg_bwd_body (:181-206), chunk r, column k, rows first = max(r rc, k) .. iend = min((r + 1) rc, n) (the rows from
    max(r rc, 64 (k // 64)) up to k add exact zeros, :195): four chains strided by 4 (:193), ceil((iend - first) / 4)
    links at most, and (a + b) + (c + d) (:203) two:
        BWD_DEPTH_rk = ceil((iend - first) / 4) + 2,   |wbuf[r]_k - sum_i W_ik v_i| <= u BWD_DEPTH_rk sum_i |W_ik v_i|.
    Planes r < k // rc are unspecified.  The sum of the planes belongs to the finish kernel.
solve  pg_solve_body (:228-301), row i = 64 jb + r of the forward substitution: the solved part leaves through a chain
    of jb links per lane (:242-246) and six shuffle levels (:250), then ONE subtraction (:251), then r fmas of the block
    substitution (:262) and the division (:260).  With Higham's Lemma 8.4 (divide through by the roundings the
    right-hand side passes: the subtraction, the r fmas, the division) the right-hand side is unperturbed, the diagonal
    term carries r + 2, the term of block column k' < r carries k' + 1 <= r, a term left of the block jb + 6:
        SOLVE_FWD_i = max(r + 2, jb + 6 if jb > 0 else 0),
        |L v - k_truth|_i <= u SOLVE_FWD_i (|L||v|)_i + e_k,i             (e_k: the k budget; k is this kernel's input)
    factor_ref's C_TRSV form u ((n_i + C)(|L||v|)_i + |b_i|) with the constant re-counted: n_i + C is replaced by the
    count itself (never larger than n_i + 1), and there is no shift, hence no |b_i| term.  Backward, column c = 64 jb +
    r, bs rows in the block: four chains over the rows below the block strided by 4 (:276-280), links =
    ceil((n - 64 jb - 64) / 4), the (a + b) + (c + d) combine and the subtraction (:291), bs - 1 - r fmas (:295), the
    division (:293):
        SOLVE_BWD_c = max(bs - 1 - r + 2, links + 2 if links > 0 else 0),   |L^T w - v_dev|_c <= u SOLVE_BWD_c (|L^T||w|)_c.
finish  pg_finish_kernel (:317-436).  Every sum: a per-thread fma chain over k = t, t + 256, ... (:342), ceil(n / 256)
    links, six shuffle levels (:373-382), (red0 + red1) + (red2 + red3) (:390) two:  FIN = ceil(n / 256) + 8.
    The truth is the exact value of the device's own formulas on the stream's bits (scaled x, alpha), T, sc, lw, the
    device's v and the device's partial planes of w.
      mu    |mu - truth| <= u FIN sum|k alpha| + sum|alpha| e_k + u |mu|                        (tot + mean, :408)
      var   |var - truth| <= u FIN sum v^2 + dktt + u |var|         (dktt: sweep_ref.ktt_truth, the same arithmetic, :399-407)
      J     the squared-exponential part (-2 sc_d)(tt_d - xs_d) k_se (:362): tt_d = T_d sc_d rounds once, an ABSOLUTE
            u |tt_d| inside the difference; the subtraction and the two products round (three), and k_se carries its
            kernel-value budget e_se:  2 |sc_d| (u |tt_d| k_se + |df_d| (3 u k_se + e_se)).
            The linear part fma(lin_coef q, xs_d lw_d sc_d, J) (:363-368): p_d = (tt_d xs_d) lw_d three roundings
            (tt and two products), q = P p_d^(P-1) by P - 1 products each with p_d's three: 4 (P - 1); lin_coef q one;
            xs_d lw_d sc_d two: (4 P - 1) u |J_lin|, and the fma rounds the whole of J once: u |J|.
      dmu   |dmu_d - truth| <= u FIN sum|alpha J_d| + sum|alpha| e_J,d                                (stored as summed)
      w_k   the planes k // rc .. nrc - 1 added in order from zero (:354): nrc - 1 - k // rc roundings,
            e_w,k = u (nrc - 1 - k // rc) sum_r |plane_r,k|.
      dvar  g_d = sum_k w_k J_kd:  e_g = sum_k ((u FIN |w_k| + e_w,k) |J_kd| + |w|_k e_J,kd), |w|_k = sum_r |plane_r,k|;
            d k(t,t)/d t_d = lin_coef (2 P t_d^(2P-1)) by 2 P - 1 products and one more (:426-428): 2 P u |.|;
            fma(-2, g, .) rounds once (:430):   |dvar_d - truth| <= 2 e_g + 2 P u |dktt_d| + u |dvar_d|.
utility chain  (util_grad.h:20-52; allowances of util_ref: exp and expm1 E_EXP = 3 ulp, erfc E_ERFC = 16 ulp, 1 ulp = 2 u;
    sqrt, division, product, sum correctly rounded).  du_d = fma(g_mu, dmu_d, g_var * dvar_d) (predgrad.hip:434):
        |du_d - (g_mu dmu_d + g_var dvar_d)| <= u (E_mu |g_mu dmu_d| + (E_var + 1) |g_var dvar_d|) + u |du_d|
    with g_mu, g_var from mpmath at the device's (mu, var) and dmu, dvar the device's bits.
      AGP    g_mu = -1 exact: E_mu = 0.  g_var = -0.5 / var, one division: E_var = 1.
      BAPE   g_mu = -2 exact: E_mu = 0.  g_var = -(2 + 1 / expm1(var)): expm1 2 E_EXP, the division 1, the sum 1 (both
             terms have one sign, so each relative error is relative to the sum): E_var = 2 E_EXP + 2.
      JONES  z = ((mu - ybest) - zeta) / sd: the first difference rounds relative to |mu - ybest|, the second, the
             square root and the division relative to z:  dz = 3 + |mu - ybest| / |imp| (in u, relative to z).
             g_mu = -(0.5 erfc(-z M_SQRT1_2)): the constant and the product 2, so the argument is off by (dz + 2) u
             relative, which Phi passes on as |z| phi(z) / Phi(z) times that -- the rounding of z through Phi:
                 E_mu = 2 E_ERFC + (dz + 2) |z| phi / Phi.
             g_var = -(exp(-0.5 z z) C) / (2 sd): the argument z^2 / 2 carries 2 dz + 1 (the product z z), absolute
             (z^2 / 2)(2 dz + 1) u in the exponent -- the inherent z^2 factor; exp 2 E_EXP; C and its product 2; sd's
             square root 1; the division 1:   E_var = 2 E_EXP + 4 + (z^2 / 2)(2 dz + 1).
      NEG_MEAN  u = -mu and du = -dmu bit for bit (fma(-1, dmu, 0 * dvar)).
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.special import erfc

import factor_ref as fr
import kvalue_ref as kr
import sweep_ref as sr
import util_ref

KINDS = ("agp", "bape", "jones", "negmean")


def params(ndim, log_M, log_constant=None, white_noise=-12.0, yerr=0.0, mean=0.0, lin=None):
    """The evaluated hyper-parameters, as ``GP._kernel_struct`` forms them.  ``lin``: (log_constant2, log_gamma2,
    order) of an added ``c2 * LinearKernel`` or None."""
    prm = {"ndim": int(ndim), "amp": 1.0 if log_constant is None else float(ndim * np.exp(log_constant)),
           "inv_metric": np.exp(-np.asarray(log_M, dtype=np.float64)) * np.ones(ndim),
           "diag_add": float(yerr) ** 2 + float(np.exp(white_noise)), "mean": float(mean),
           "lin_coef": 0.0, "lin_order": 0}
    if lin is not None:
        prm["lin_coef"] = float(ndim * np.exp(lin[0])) * float(np.exp(-lin[1]))
        prm["lin_order"] = int(lin[2])
    return prm


def fixture_params(g):
    """``params`` of a tests/golden fixture (the kernels tests/test_gpu_parity.py's ``build`` makes)."""
    D = g["theta"].shape[1]
    p = g["p"]
    if int(g["fit_amp"]):
        return params(D, p[2:], log_constant=p[1], white_noise=float(g["white_noise"]), mean=float(p[0]))
    return params(D, p[1:], white_noise=float(g["white_noise"]), mean=float(p[0]))


def kernel(T, X, prm):
    """k (M, N) and J (M, N, D) = d k(t_m, x_n) / d t_md."""
    T, X = np.atleast_2d(T), np.atleast_2d(X)
    diff = T[:, None, :] - X[None, :, :]
    kse = prm["amp"] * np.exp(-0.5 * np.sum(diff * diff * prm["inv_metric"], axis=2))
    k = kse.copy()
    J = -kse[:, :, None] * diff * prm["inv_metric"]
    c, P = prm["lin_coef"], prm["lin_order"]
    if c != 0.0:
        prod = T[:, None, :] * X[None, :, :]
        if P == 0:
            k += c * prm["ndim"]
        else:
            k += c * np.sum(prod ** P, axis=2)
            J = J + c * P * prod ** (P - 1) * X[None, :, :]
    return k, J


def kernel_diag(T, prm):
    """k(t, t) (M,) without the white noise, and its derivative (M, D)."""
    T = np.atleast_2d(T)
    c, P = prm["lin_coef"], prm["lin_order"]
    ktt = np.full(len(T), prm["amp"])
    dktt = np.zeros_like(T)
    if c != 0.0:
        if P == 0:
            ktt = ktt + c * prm["ndim"]
        else:
            ktt = ktt + c * np.sum((T * T) ** P, axis=1)
            dktt = c * 2 * P * T ** (2 * P - 1)
    return ktt, dktt


def gram(X, prm):
    K = kernel(X, X, prm)[0]
    K[np.diag_indices_from(K)] += prm["diag_add"]
    return K


def posterior(T, X, y, prm, route="solve", scales=False):
    """(mu, var, dmu, dvar) at the rows of T; ``route``: "solve" (two triangular solves against the factor) or
    "inverse" (products with the explicit L^-1).  ``scales``: also S_mu[d] = sum_n |alpha_n J_nd| and
    S_var[d] = |d k(t,t)/d t_d| + 2 sum_n |w_n J_nd|."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    L = cholesky(gram(X, prm), lower=True)
    alpha = cho_solve((L, True), np.asarray(y, dtype=np.float64) - prm["mean"])
    k, J = kernel(T, X, prm)
    if route == "inverse":
        W = solve_triangular(L, np.eye(len(X)), lower=True)
        v = W @ k.T
        w = W.T @ v
    elif route == "solve":
        v = solve_triangular(L, k.T, lower=True)
        w = solve_triangular(L.T, v, lower=False)
    else:
        raise ValueError(route)
    ktt, dktt = kernel_diag(T, prm)
    mu = k @ alpha + prm["mean"]
    var = ktt - np.sum(v * v, axis=0)
    dmu = np.einsum("n,mnd->md", alpha, J)
    dvar = dktt - 2.0 * np.einsum("nm,mnd->md", w, J)
    if scales:
        s_mu = np.einsum("n,mnd->md", np.abs(alpha), np.abs(J))
        s_var = np.abs(dktt) + 2.0 * np.einsum("nm,mnd->md", np.abs(w), np.abs(J))
        return mu, var, dmu, dvar, s_mu, s_var
    return mu, var, dmu, dvar


def utility(kind, mu, var, zeta=0.01, ybest=0.0):
    """(u, du/dmu, du/dvar, flat) elementwise; ``flat`` marks where the gradient is defined as zero."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    flat = np.zeros(mu.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if kind == "agp":
            u = -(mu + 0.5 * np.log(2.0 * np.pi * np.e * var))
            g_mu = np.where(var < 0, np.nan, -1.0)
            g_var = np.where(var < 0, np.nan, -0.5 / var)
        elif kind == "bape":
            flat = var <= 0
            u = np.where(flat, np.inf, -((2.0 * mu + var) + (var + np.log(1.0 - np.exp(-var)))))
            g_mu = np.where(flat, 0.0, -2.0)
            g_var = np.where(flat, 0.0, -(2.0 + 1.0 / np.expm1(var)))
        elif kind == "jones":
            sd = np.sqrt(var)
            flat = ~(sd > 0)
            imp = mu - ybest - zeta
            z = imp / sd
            cdf = 0.5 * erfc(-z / np.sqrt(2.0))
            pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
            u = np.where(flat, 0.0, -(imp * cdf + sd * pdf))
            g_mu = np.where(flat, 0.0, -cdf)
            g_var = np.where(flat, 0.0, -pdf / (2.0 * sd))
        elif kind == "negmean":
            flat = ~np.isfinite(mu)
            u = np.where(flat, np.inf, -mu)
            g_mu = np.where(flat, 0.0, -1.0)
            g_var = np.zeros(mu.shape)
        else:
            raise ValueError(kind)
    return u, g_mu, g_var, flat


def predict_grad(T, X, y, prm, kind=None, bounds=None, zeta=0.01, route="solve"):
    """What ``GP.predict_grad`` returns: (mu, var, dmu, dvar), or (u, du, mu, var) with a utility ``kind``; rows with
    a non-finite coordinate or outside ``bounds`` are NaN with u = +inf and du = 0."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    ok = np.all(np.isfinite(T), axis=1)
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore"):
            ok &= np.all((T >= b[:, 0]) & (T <= b[:, 1]), axis=1)
    mu, var, dmu, dvar = posterior(np.where(ok[:, None], T, 0.0), X, y, prm, route=route)
    mu, var = np.where(ok, mu, np.nan), np.where(ok, var, np.nan)
    dmu, dvar = np.where(ok[:, None], dmu, np.nan), np.where(ok[:, None], dvar, np.nan)
    if kind is None:
        return mu, var, dmu, dvar
    u, g_mu, g_var, flat = utility(kind, mu, var, zeta=zeta, ybest=float(np.max(y)))
    with np.errstate(all="ignore"):
        du = g_mu[:, None] * dmu + g_var[:, None] * dvar
    du = np.where((flat | ~ok)[:, None], 0.0, du)
    u = np.where(ok, u, np.inf)
    return u, du, mu, var


# ----------------------------------------------------------------------------------------------------------------------
# the call's scratch layout (csrc/predgrad.hip; tests/test_predgrad_ref.py pins every constant against the source)
# ----------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53
LD = np.longdouble
SECOND = 1.0 + 2.0 ** -20
PG_T = 256
PG_PB = 8
PG_PBS = 4
PG_FR = 8
PG_NRC = 8
PG_B = 64
PG_PER_POINT = 2 + PG_NRC
PG_CHUNK_DOUBLES = 1 << 24
PG_CHUNK_MAX = 4096
PG_RC_MIN = 512
FWD_STRIDE = 128
SENTINEL = -1.2345678901234567e300


def round_up(n, b):
    return (n + b - 1) // b * b


def ns_of(n):
    return round_up(n, PG_B)


def chunk(m, n):
    """pg_chunk: points per chunk of the call."""
    ch = PG_CHUNK_DOUBLES // (PG_PER_POINT * ns_of(n)) // PG_PB * PG_PB
    ch = max(PG_PB, min(PG_CHUNK_MAX, ch))
    return min(ch, round_up(m, PG_PB))


def work_len(m, n):
    return chunk(m, n) * PG_PER_POINT * ns_of(n)


def row_chunks(n, route):
    """(rc, nrc) of apgp_predict_grad: rows per chunk of the transposed product and the number of chunks."""
    if route != "inverse":
        return ns_of(n), 1
    rc = max(PG_RC_MIN, round_up((n + PG_NRC - 1) // PG_NRC, PG_B))
    return rc, (n + rc - 1) // rc


def work_views(work, m, n, route):
    """What one chunk of the call (m <= ch) leaves in ``work``: {"k": kbuf (m, ns) or None on the solve route, where v
    overwrites it, "v": (m, ns), "w": the partial planes (nrc, m, ns), "rc", "nrc"}.  Views, not copies."""
    work = np.asarray(work)
    ns = ns_of(n)
    ch = len(work) // (PG_PER_POINT * ns)
    if ch != chunk(m, n) or m > ch:
        raise ValueError("work of %d doubles is not one chunk of m = %d, n = %d" % (len(work), m, n))
    rc, nrc = row_chunks(n, route)
    kb = work[:ch * ns].reshape(ch, ns)[:m]
    vb = work[ch * ns:2 * ch * ns].reshape(ch, ns)[:m]
    wb = work[2 * ch * ns:PG_PER_POINT * ch * ns].reshape(PG_NRC, ch, ns)[:nrc, :m]
    if route == "inverse":
        return {"k": kb, "v": vb, "w": wb, "rc": rc, "nrc": nrc}
    return {"k": None, "v": kb, "w": wb, "rc": rc, "nrc": nrc}


# ----------------------------------------------------------------------------------------------------------------------
# cases (shared by tests/test_predgrad_ref.py and tests/test_gpu_predict_grad_budget.py)
# ----------------------------------------------------------------------------------------------------------------------
INV_N = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257, 511, 512, 513, 1025, 2049, 4096, 4097)
INV_M = (1, 7, 8, 9, 17)
SOLVE_N = (1, 2, 63, 64, 65, 129, 257, 449)
SOLVE_M = (1, 3, 4, 5, 9)
DIMS = (1, 2, 3, 5, 8, 9, 16, 17, 32)
LIN_CASES = tuple((P, D) for P in (0, 1, 2, 3) for D in (3, 8, 17))
M_OF = {"inverse": 9, "solve": 5}
BIG_N = 2049                        # from here on the truth is formed for BIG_ROWS only
BIG_ROWS = (0, 7, 8)                # one point of the full block, its last, and the single one
UTIL_N, UTIL_M, UTIL_D = 65, 64, 3
UTIL_KINDS = {"agp": 0, "bape": 1, "jones": 2, "negmean": 4}
UTIL_ZETA = 0.01
UTIL_CAP = 0.10
UTIL_OUT = 2
UTIL_SCALE = {"inverse": 0.3515625, "solve": 3.0625}
UTIL_YBEST = 0.25
_CASES = {}


def budget_cases():
    """{test name: [(n, D, m, route, order)]}: every input of tests/test_gpu_predict_grad_budget.py's budget tests."""
    both = ("inverse", "solve")
    return {"inverse_n": [(n, 3, M_OF["inverse"], "inverse", None) for n in INV_N],
            "inverse_m": [(129, 3, m, "inverse", None) for m in INV_M],
            "solve_n": [(n, 3, M_OF["solve"], "solve", None) for n in SOLVE_N],
            "solve_m": [(65, 3, m, "solve", None) for m in SOLVE_M],
            "dims": [(65, D, M_OF[rt], rt, None) for D in DIMS for rt in both],
            "linear": [(65, D, M_OF[rt], rt, P) for P, D in LIN_CASES for rt in both],
            "utility": [(UTIL_N, UTIL_D, UTIL_M, rt, None) for rt in both]}


def case_id(c):
    return "n%d-D%d-m%d-%s-P%s" % c


class Case(object):
    """One planted model: training set, alpha, m query rows and the mean from sweep_ref.case, W = sweep_ref.planted_w
    (route "inverse") or L = factor_ref.planted_factor (route "solve"), and the packed stream as apgp_pack_train forms
    it (x sc rounded once | alpha | 0)."""

    def __init__(self, n, D, m, route, order=None, util=False):
        key = (n, D, order)
        if key not in _CASES:
            _CASES.clear()                                     # (one at a time: the large ones are large)
            _CASES[key] = sr.case(n, D, order)
        self.X, self.alpha, Tb, self.k, self.mean = _CASES[key]
        self.n, self.D, self.m, self.route, self.order = n, D, m, route, order
        self.T = np.ascontiguousarray(sr.tiled(Tb, m))
        self.A = sr.planted_w(n) if route == "inverse" else fr.planted_factor(n)[0]
        self.rc, self.nrc = row_chunks(n, route)
        self.rows = np.array(BIG_ROWS) if (n >= BIG_N and m == M_OF["inverse"]) else np.arange(m)
        self.xs = pack_stream(self.X, self.alpha, self.k)
        self.lo = self.hi = None
        if util:
            # the utility case: the planted factor scaled (exactly representable factors, chosen on the CPU from the
            # float64 restatement) so that sigma^2 = k(t,t) - |v|^2 is positive on all but a few rows, and the last
            # UTIL_OUT rows moved out of the box that the others span
            self.A = self.A * UTIL_SCALE[route]
            self.lo, self.hi = self.T[:-UTIL_OUT].min(0), self.T[:-UTIL_OUT].max(0)
            for j in range(UTIL_OUT):
                d = j % D
                self.T[m - 1 - j] = 0.5 * (self.lo + self.hi)
                self.T[m - 1 - j, d] = (self.hi[d] + 0.25 * (self.hi[d] - self.lo[d])) if j & 1 else \
                    (self.lo[d] - 0.25 * (self.hi[d] - self.lo[d]))

    def leading_dims(self):
        n = self.n
        return (n + (n & 1), n + (n & 1) + 2) if self.route == "inverse" else (n, n + 3)

    def panel(self, ld):
        """The n x ld buffer handed to the device: NaN above the diagonal and in the padding."""
        P = np.full((self.n, ld), np.nan)
        low = np.tril(np.ones((self.n, self.n), dtype=bool))
        P[:, :self.n][low] = self.A[low]
        return P


def pack_stream(X, alpha, k):
    sc, _ = kr.kernconst(k)
    dp = len(sc)
    xs = np.zeros((len(X), dp + 2))
    xs[:, :k.ndim] = np.asarray(X, dtype=np.float64) * np.array(sc[:k.ndim])
    xs[:, dp] = alpha
    return xs


def _ratio(err, den):
    """err / den entry by entry: 0 where the error is zero, inf where the bound is zero or the error is not finite."""
    err, den = np.asarray(err, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / den)
    return np.where(np.isfinite(r), r, np.inf)


def _worst(r):
    r = np.asarray(r)
    return float(r.max()) if r.size else 0.0


# ---- k ---------------------------------------------------------------------------------------------------------------
def k_ratio(kb, T, X, k):
    """|kbuf - truth| / kvalue_ref.budget (m x n), and whether the pad n .. ns of every row is +0.0 to the bit."""
    n = len(X)
    with np.errstate(all="ignore"):
        t, b = kr.truth_ld(T, X, k), kr.budget(T, X, k)
    kb = np.asarray(kb, dtype=np.float64)
    err = np.abs(kb[:, :n].astype(LD) - t).astype(np.float64)
    pad_ok = bool(np.all(np.ascontiguousarray(kb[:, n:]).view(np.int64) == 0))
    return _ratio(err, b), pad_ok


# ---- v = W k ---------------------------------------------------------------------------------------------------------
def fwd_depth(n):
    return (np.arange(n) + FWD_STRIDE) // FWD_STRIDE + 1 + 6


def fwd_ratio(W, kbits, v, blk=512):
    """|v - W k| / (u FWD_DEPTH sum |W_ik k_k|) (m x n), the truth in long double from the bits of W's lower triangle and
    of ``kbits`` (m x n)."""
    n = kbits.shape[1]
    kl, ka = kbits.astype(LD), np.abs(kbits)
    out = np.zeros(kbits.shape)
    dep = fwd_depth(n)
    for i0 in range(0, n, blk):
        i1 = min(n, i0 + blk)
        Wb = np.tril(W[i0:i1, :i1], i0)
        t = kl[:, :i1] @ Wb.astype(LD).T
        den = U * dep[i0:i1] * (ka[:, :i1] @ np.abs(Wb).T)
        out[:, i0:i1] = _ratio(np.abs(v[:, i0:i1].astype(LD) - t).astype(np.float64), den)
    return out


# ---- the partial planes of w = W^T v -----------------------------------------------------------------------------------
def bwd_depth(n, rc, r):
    """BWD_DEPTH of chunk r for the columns 0 .. iend - 1."""
    iend = min(n, (r + 1) * rc)
    first = np.maximum(r * rc, np.arange(iend))
    return (iend - first + 3) // 4 + 2


def bwd_ratio(W, vbits, planes, n, rc, nrc):
    """Worst |plane_r,k - sum_i W_ik v_i| / (u BWD_DEPTH sum |W_ik v_i|) over the chunks r >= k // rc, per chunk."""
    out = []
    vl, va = vbits.astype(LD), np.abs(vbits)
    for r in range(nrc):
        i0, i1 = r * rc, min(n, (r + 1) * rc)
        Wc = np.tril(W[i0:i1, :i1], i0)
        t = vl[:, i0:i1] @ Wc.astype(LD)
        den = U * bwd_depth(n, rc, r) * (va[:, i0:i1] @ np.abs(Wc))
        out.append(_worst(_ratio(np.abs(planes[r][:, :i1].astype(LD) - t).astype(np.float64), den)))
    return out


# ---- the two substitutions -------------------------------------------------------------------------------------------
def solve_counts(n):
    i = np.arange(n)
    jb, r = i // PG_B, i % PG_B
    fwd = np.maximum(r + 2, np.where(jb > 0, jb + 6, 0))
    bs = np.minimum(PG_B, n - PG_B * jb)
    links = (np.maximum(n - PG_B * jb - PG_B, 0) + 3) // 4
    bwd = np.maximum(bs - 1 - r + 2, np.where(links > 0, links + 2, 0))
    return fwd, bwd


def solve_ratio(L, kh, ek, v, w):
    """(|L v - k_truth| / (u SOLVE_FWD |L||v| + e_k), |L^T w - v| / (u SOLVE_BWD |L^T||w|)), each m x n, from the bits
    of L's lower triangle, v and w."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    cf, cb = solve_counts(n)
    Ll, aL = L.astype(LD), np.abs(L)
    if not (np.all(np.isfinite(v)) and np.all(np.isfinite(w))):
        bad = np.where(np.isfinite(v) & np.isfinite(w), 0.0, np.inf)
        return bad, bad
    rf = np.abs(v.astype(LD) @ Ll.T - kh).astype(np.float64)
    df = U * cf * (np.abs(v) @ aL.T) * SECOND + ek
    rb = np.abs(w.astype(LD) @ Ll - v.astype(LD)).astype(np.float64)
    db = U * cb * (np.abs(w) @ aL) * SECOND
    return _ratio(rf, df), _ratio(rb, db)


# ---- finish ----------------------------------------------------------------------------------------------------------
def fin_depth(n):
    return (n + PG_T - 1) // PG_T + 6 + 2


def sum_planes(planes, n, rc, nrc, absolute=False):
    """(sum over the planes r >= k // rc in long double, or of their magnitudes; the number of roundings of that sum)."""
    kc = np.arange(n) // rc
    s = np.zeros(planes[0][:, :n].shape, dtype=LD)
    for r in range(nrc):
        p = np.where(kc <= r, planes[r][:, :n], 0.0).astype(LD)
        s = s + (np.abs(p) if absolute else p)
    return s, nrc - 1 - kc


def finish_truth(xs, T, X, k, mean, v, planes, rc, nrc):
    """({name: truth in long double}, {name: bound}) of mu, var (m), dmu, dvar (m x D) from the stream's bits, T, the
    device's v (m x n) and partial planes; ``X`` only for the kernel-value budgets (module docstring, "finish")."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    m, D = T.shape
    n = len(xs)
    scl, lwl = kr.kernconst(k)
    dp = len(scl)
    sc, lw = np.array(scl[:D]), np.array(lwl[:D])
    xd, alpha = xs[:, :D], xs[:, dp]
    c, P = k.lin_coef, k.lin_order
    with np.errstate(all="ignore"):
        th, tl = kr._two_prod(T, sc[None, :])
        dh, dl = kr._two_sum(th[:, None, :], -xd[None, :, :])
        df = dh.astype(LD) + (dl.astype(LD) + tl[:, None, :].astype(LD))           # m x n x D
        kse = LD(k.amp) * np.exp(-(df * df).sum(-1))
        e_k = kr.budget(T, X, k)
        e_se = kr.budget(T, X, k._replace(lin_coef=0.0)) if c != 0.0 else e_k
    ttl = th.astype(LD) + tl.astype(LD)
    J = -2.0 * sc.astype(LD) * df * kse[:, :, None]
    kse64, adf = np.abs(kse).astype(np.float64), np.abs(df).astype(np.float64)
    e_J = 2.0 * np.abs(sc) * (U * np.abs(th)[:, None, :] * kse64[:, :, None]
                              + adf * (3.0 * U * kse64 + e_se)[:, :, None])
    kv = kse
    if c != 0.0:
        if P == 0:
            kv = kse + LD(c) * LD(D)
        else:
            pd = ttl[:, None, :] * xd.astype(LD)[None] * lw.astype(LD)
            kv = kse + LD(c) * (pd ** P).sum(-1)
            Jl = LD(c) * LD(P) * pd ** (P - 1) * (xd.astype(LD) * lw.astype(LD) * sc.astype(LD))[None]
            J = J + Jl
            e_J = e_J + U * ((4 * P - 1) * np.abs(Jl) + np.abs(J)).astype(np.float64)
    e_J = e_J * SECOND
    aJ = np.abs(J).astype(np.float64)
    fin = fin_depth(n)
    al, aa = alpha.astype(LD), np.abs(alpha)
    val, bud = {}, {}
    val["mu"] = kv @ al + LD(mean)
    b = (U * fin * (np.abs(kv).astype(np.float64) @ aa) + e_k @ aa) * SECOND
    bud["mu"] = b + U * (np.abs(val["mu"]).astype(np.float64) + b)
    ktt, dktt = sr.ktt_truth(T, k)
    vl = v[:, :n].astype(LD)
    sq = (vl * vl).sum(1)
    val["var"] = ktt - sq
    b = U * fin * sq.astype(np.float64) * SECOND + dktt
    bud["var"] = b + U * (np.abs(val["var"]).astype(np.float64) + b)
    val["dmu"] = np.einsum("n,mnd->md", al, J)
    bud["dmu"] = (U * fin * np.einsum("n,mnd->md", aa, aJ) + np.einsum("n,mnd->md", aa, e_J)) * SECOND
    wk, nadd = sum_planes(planes, n, rc, nrc)
    wa = sum_planes(planes, n, rc, nrc, absolute=True)[0].astype(np.float64)
    g = np.einsum("mn,mnd->md", wk, J)
    e_g = (np.einsum("mn,mnd->md", U * (fin + nadd)[None, :] * wa, aJ) + np.einsum("mn,mnd->md", wa, e_J)) * SECOND
    if c != 0.0 and P > 0:
        dk = LD(c) * LD(2 * P) * T.astype(LD) ** (2 * P - 1)
    else:
        dk = np.zeros((m, D), dtype=LD)
    val["dvar"] = dk - 2.0 * g
    b = 2.0 * e_g + 2 * P * U * np.abs(dk).astype(np.float64) * SECOND
    bud["dvar"] = b + U * (np.abs(val["dvar"]).astype(np.float64) + b)
    return val, bud


def finish_ratios(out, val, bud):
    return {key: _worst(_ratio(np.abs(np.asarray(out[key], dtype=np.float64).astype(LD) - val[key]).astype(np.float64),
                               bud[key])) for key in ("mu", "var", "dmu", "dvar")}


# ---- one call, stage by stage ----------------------------------------------------------------------------------------
def judge(case, out):
    """{stage: worst ratio} of one call's record ``out``: "k" (m x ns, inverse route), "v" (m x ns), "w" (nrc x m x ns),
    "mu", "var" (m), "dmu", "dvar" (m x D), "xs" (the stream's bits).  Only ``case.rows`` are judged."""
    rows, n = case.rows, case.n
    T = case.T[rows]
    res = {}
    v = np.asarray(out["v"])[rows][:, :n]
    planes = [np.asarray(p)[rows] for p in out["w"]]
    if case.route == "inverse":
        kb = np.asarray(out["k"])[rows]
        r, pad_ok = k_ratio(kb, T, case.X, case.k)
        res["k"] = _worst(r) if pad_ok else np.inf
        res["v"] = _worst(fwd_ratio(case.A, kb[:, :n], v)) if np.all(np.isfinite(kb[:, :n])) else np.inf
        res["w"] = max(bwd_ratio(case.A, v, planes, n, case.rc, case.nrc)) if np.all(np.isfinite(v)) else np.inf
    else:
        with np.errstate(all="ignore"):
            kh, ek = kr.truth_ld(T, case.X, case.k), kr.budget(T, case.X, case.k)
        rf, rb = solve_ratio(case.A, kh, ek, v, planes[0][:, :n])
        res["solve_fwd"], res["solve_bwd"] = _worst(rf), _worst(rb)
    if np.all(np.isfinite(v)):
        val, bud = finish_truth(out["xs"], T, case.X, case.k, case.mean, v, planes, case.rc, case.nrc)
        res.update(finish_ratios({key: np.asarray(out[key])[rows] for key in ("mu", "var", "dmu", "dvar")}, val, bud))
    else:
        res.update({key: np.inf for key in ("mu", "var", "dmu", "dvar")})
    return res


# ---- the utility chain -----------------------------------------------------------------------------------------------
def util_grad_truth(kind, mu, var, zeta, ybest):
    """(g_mu, g_var, E_mu, E_var) at one (mu, var) (floats, var > 0): the derivatives by mpmath with 60 digits and the
    allowances of the module docstring, in units of u."""
    import mpmath as mp
    E_EXP, E_ERFC = util_ref.E_EXP, util_ref.E_ERFC
    with mp.workdps(util_ref.DPS):
        m, v = mp.mpf(float(mu)), mp.mpf(float(var))
        if kind == "agp":
            return -1.0, float(-1 / (2 * v)), 0.0, 1.0
        if kind == "bape":
            return -2.0, float(-(2 + 1 / mp.expm1(v))), 0.0, 2.0 * E_EXP + 2.0
        if kind == "negmean":
            return -1.0, 0.0, 0.0, 0.0
        sd = mp.sqrt(v)
        d1 = m - mp.mpf(float(ybest))
        imp = d1 - mp.mpf(float(zeta))
        z = imp / sd
        Phi, phi = mp.ncdf(z), mp.npdf(z)
        dz = 3 + (abs(d1) / abs(imp) if imp != 0 else mp.inf)
        e_mu = 2 * E_ERFC + (dz + 2) * abs(z) * phi / Phi
        e_var = 2 * E_EXP + 4 + (z * z / 2) * (2 * dz + 1)
        return float(-Phi), float(-phi / (2 * sd)), float(e_mu), float(e_var)


def du_ratio(kind, du, mu, var, dmu, dvar, zeta, ybest):
    """|du - (g_mu dmu + g_var dvar)| / bound for every row (m x D), the rows being in the box with var > 0."""
    import mpmath as mp
    du = np.atleast_2d(du)
    out = np.zeros(du.shape)
    for i in range(len(du)):
        g_mu, g_var, e_mu, e_var = util_grad_truth(kind, mu[i], var[i], zeta, ybest)
        for d in range(du.shape[1]):
            with mp.workdps(util_ref.DPS):
                a, b = mp.mpf(g_mu) * mp.mpf(float(dmu[i, d])), mp.mpf(g_var) * mp.mpf(float(dvar[i, d]))
                err = float(abs(mp.mpf(float(du[i, d])) - (a + b))) if np.isfinite(du[i, d]) else np.inf
                bound = U * (e_mu * float(abs(a)) + (e_var + 1.0) * float(abs(b))) * SECOND
                bound += U * abs(float(du[i, d])) + 2.0 ** -1074
                # below the normal range the relative model ends (util_ref's rule for an underflowed tail): a factor
                # under 2^-1022 may come back flushed to zero, and a subnormal one is a multiple of 2^-1074
                if abs(g_mu) < 2.0 ** -1022:
                    bound += float(abs(a)) + 2.0 ** -1074 * abs(float(dmu[i, d]))
                if abs(g_var) < 2.0 ** -1022:
                    bound += float(abs(b)) + 2.0 ** -1074 * abs(float(dvar[i, d]))
            out[i, d] = 0.0 if err == 0.0 else err / bound
    return out


def util_rows(case, var):
    """(in the box, judged): the rows inside [lo, hi], and of those the ones with var > 0 (the others are flat, or NaN
    for AGP: the header's non-finite table)."""
    inside = np.all((case.T >= case.lo) & (case.T <= case.hi), axis=1)
    with np.errstate(invalid="ignore"):
        return inside, inside & (np.asarray(var) > 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatements of the device order, and their mutants
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = {"fwd_skip_last_odd": ("inverse", 65, 3, None), "bwd_chunk_tail": ("inverse", 4097, 3, None),
           "finish_chunk_from_next": ("inverse", 513, 3, None), "finish_one_plane": ("inverse", 1025, 3, None),
           "solve_diag_no_identity": ("solve", 65, 3, None), "solve_bwd_off_by_block": ("solve", 129, 3, None),
           "j_no_scale": ("inverse", 65, 3, 2), "dktt_exponent": ("inverse", 65, 8, 1),
           "dim_group_offset": ("inverse", 65, 17, None), "fp32_v": ("inverse", 129, 3, None),
           "pad_not_zero": ("inverse", 129, 3, None)}


def _tree(s):
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., np.arange(64) ^ o]
    return s[..., 0]


def _chain(t, axis=1):
    """Sum over ``axis`` in index order."""
    t = np.moveaxis(t, axis, 0)
    acc = np.zeros(t.shape[1:])
    for j in range(len(t)):
        acc = acc + t[j]
    return acc


def kstar_restate(T, xs, k, ns, mutant=None):
    """kbuf (m x ns) from the stream: pg_kval in float64 (NumPy's exp for apgp_exp), the pad zeroed."""
    T = np.atleast_2d(T)
    n = len(xs)
    kv = _kvalues(T, xs, k)[1]
    kb = np.zeros((len(T), ns))
    kb[:, :n] = kv
    if mutant == "pad_not_zero" and ns > n:
        kb[:, n:] = np.nan                                   # (what the caller's work held)
    return kb


def _kvalues(T, xs, k):
    """(tt, kv, kse) as pg_kse / pg_kval form them."""
    D = k.ndim
    scl, lwl = kr.kernconst(k)
    dp = len(scl)
    sc, lw = np.array(scl), np.array(lwl)
    tt = np.zeros((len(T), dp))
    tt[:, :D] = T * sc[:D]
    xr = xs[:, :dp]
    df = tt[:, None, :] - xr[None]
    with np.errstate(all="ignore"):
        q0 = _chain(df[:, :, 0::2] ** 2, axis=2)
        q1 = _chain(df[:, :, 1::2] ** 2, axis=2)
        kse = k.amp * np.exp(np.maximum(-(q0 + q1), -700.0))
    kv = kse
    if k.lin_coef != 0.0:
        if k.lin_order == 0:
            ls = float(D)
        else:
            p = tt[:, None, :] * xr[None] * lw
            q = p.copy()
            for _ in range(1, k.lin_order):
                q = q * p
            ls = _chain(q, axis=2)
        # fma(lin_coef, ls, kse) through error-free transformations (one rounding, short of a rare double rounding):
        # with P = 0 nothing else of the linear term rounds, and a product rounded on its own would be a second one
        p, e = kr._two_prod(np.full(kse.shape, k.lin_coef), ls * np.ones(kse.shape))
        s, t = kr._two_sum(p, kse)
        kv = s + (t + e)
    return tt, kv, kse


def fwd_restate(W, kb, n, mutant=None):
    """v (m x n) = W k in pg_fwd_body's order from kbuf ``kb`` (m x ns, the pad included)."""
    Wt = np.tril(np.asarray(W)[:n, :n])
    m = len(kb)
    v = np.zeros((m, n))
    for i in range(n):
        i0 = i & ~1
        i1 = min(i0 + 1, n - 1)
        hi = i + 1
        if mutant == "fwd_skip_last_odd" and i == i1 and i1 > i0:
            hi = i                                           # the k + 1 <= i0 mask on row i1: its diagonal term is lost
        t = np.zeros((m, round_up(i1 + 1, FWD_STRIDE)))
        t[:, :hi] = kb[:, :hi] * Wt[i, :hi]
        acc = _chain(t.reshape(m, -1, 64, 2), axis=1)
        v[:, i] = _tree(acc[..., 0] + acc[..., 1])
    if n & 1:
        with np.errstate(invalid="ignore"):
            v[:, n - 1] = v[:, n - 1] + 0.0 * kb[:, n]       # the masked W[n-1][n] (a selected 0.0) times kbuf[n]
    if mutant == "fp32_v":
        v = v.astype(np.float32).astype(np.float64)
    return v


def bwd_restate(W, v, n, rc, nrc, mutant=None):
    """The partial planes (nrc x m x ns) in pg_bwd_body's order; NaN where the kernel writes nothing."""
    Wt = np.tril(np.asarray(W)[:n, :n])
    m, ns = len(v), ns_of(n)
    planes = np.full((nrc, m, ns), np.nan)
    for r in range(nrc):
        i0, i1 = r * rc, min(n, (r + 1) * rc)
        if mutant == "bwd_chunk_tail" and (r + 1) * rc > n and nrc > 1:
            planes[r] = 0.0                                  # the ragged last chunk dropped
            continue
        for c0 in range(0, ns, PG_B):
            ibeg = max(i0, c0)
            if ibeg >= i1:
                continue
            cc = min(c0 + PG_B, n)
            R = i1 - ibeg
            t = np.zeros((m, round_up(R, 4), PG_B))
            t[:, :R, :cc - c0] = v[:, ibeg:i1, None] * Wt[ibeg:i1, c0:cc][None]
            part = _chain(t.reshape(m, -1, 4, PG_B), axis=1)
            planes[r][:, c0:c0 + PG_B] = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
    return planes


def solve_restate(L, kv, n, mutant=None):
    """(v, w), each m x n, in pg_solve_body's order from the k values ``kv`` (m x n); w starts as NaN (the caller's
    work)."""
    Lt = np.tril(np.asarray(L)[:n, :n])
    m = len(kv)
    v = np.array(kv[:, :n], dtype=np.float64)
    nb = (n + PG_B - 1) // PG_B

    def diag(j0, bs):
        Lb = np.zeros((PG_B, PG_B)) if mutant == "solve_diag_no_identity" else np.eye(PG_B)
        Lb[:bs, :bs] = Lt[j0:j0 + bs, j0:j0 + bs]
        return Lb
    with np.errstate(all="ignore"):
        for jb in range(nb):
            j0 = PG_B * jb
            bs = min(PG_B, n - j0)
            if j0:
                t = v[:, None, :j0] * Lt[j0:j0 + bs, :j0][None]
                v[:, j0:j0 + bs] -= _tree(_chain(t.reshape(m, bs, jb, 64), axis=2))
            Lb = diag(j0, bs)
            ri = np.zeros((m, PG_B))
            ri[:, :bs] = v[:, j0:j0 + bs]
            for kk in range(PG_B):
                zk = ri[:, kk] / Lb[kk, kk]
                ri[:, kk] = zk
                ri[:, kk + 1:] = ri[:, kk + 1:] - Lb[kk + 1:, kk] * zk[:, None]
            v[:, j0:j0 + bs] = ri[:, :bs]
        w = np.full((m, n), np.nan)
        for jb in range(nb - 1, -1, -1):
            j0 = PG_B * jb
            bs = min(PG_B, n - j0)
            start = j0 if mutant == "solve_bwd_off_by_block" else j0 + PG_B
            R = max(n - start, 0)
            t = np.zeros((m, round_up(R, 4), bs))
            if R:
                t[:, :R] = w[:, start:n, None] * Lt[start:n, j0:j0 + bs][None]
            part = _chain(t.reshape(m, -1, 4, bs), axis=1) if R else np.zeros((m, 4, bs))
            Lb = diag(j0, bs)
            ri = np.zeros((m, PG_B))
            ri[:, :bs] = v[:, j0:j0 + bs] - ((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3]))
            for kk in range(PG_B - 1, -1, -1):
                wk = ri[:, kk] / Lb[kk, kk]
                ri[:, kk] = wk
                ri[:, :kk] = ri[:, :kk] - Lb[kk, :kk] * wk[:, None]
            w[:, j0:j0 + bs] = ri[:, :bs]
    return v, w


def _strided(t):
    """pg_finish_kernel's sum of the n terms of every row of ``t`` (m x n)."""
    m, n = t.shape
    p = np.zeros((m, round_up(n, PG_T)))
    p[:, :n] = t
    red = _tree(_chain(p.reshape(m, -1, PG_T), axis=1).reshape(m, 4, 64))
    return (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])


def finish_restate(xs, T, k, mean, v, planes, rc, nrc, mutant=None):
    """{"mu", "var", "dmu", "dvar"} in pg_finish_kernel's order."""
    T = np.atleast_2d(T)
    m, D = T.shape
    n = len(xs)
    scl, lwl = kr.kernconst(k)
    dp = len(scl)
    sc, lw = np.array(scl), np.array(lwl)
    alpha = xs[:, dp]
    c, P = k.lin_coef, k.lin_order
    tt, kv, kse = _kvalues(T, xs, k)
    kc = np.arange(n) // rc
    wk = np.zeros((m, n))
    for r in range(nrc):
        use = kc <= r
        if mutant == "finish_chunk_from_next":
            use = kc + 1 <= r
        if mutant == "finish_one_plane":
            use = np.full(n, r == nrc - 1)
        wk = np.where(use, wk + np.where(use, planes[r][:, :n], 0.0), wk)
    out = {"mu": _strided(kv * alpha) + mean}
    vv = v[:, :n]
    if c != 0.0:
        ktl = np.full(m, float(D)) if P == 0 else _chain((T * T) ** P, axis=1)
        ktt = c * ktl + k.amp
    else:
        ktt = np.full(m, k.amp)
    out["var"] = ktt - _strided(vv * vv)
    dmu, dvar = np.zeros((m, D)), np.zeros((m, D))
    for d in range(D):
        s = d % 8 if (mutant == "dim_group_offset" and D > 8) else d       # d0 ignored: every group sums dimensions 0 .. 7
        xdv, sd = xs[:, s], sc[s]
        J = (-2.0 * sd) * (tt[:, s][:, None] - xdv[None]) * kse
        if c != 0.0 and P > 0:
            pd = tt[:, s][:, None] * xdv[None] * lw[s]
            q = np.full(pd.shape, float(P))
            for _ in range(1, P):
                q = q * pd
            J = (c * q) * (xdv * lw[s] * (1.0 if mutant == "j_no_scale" else sd))[None] + J
        dmu[:, d] = _strided(alpha[None] * J)
        dk = 0.0
        if c != 0.0 and P > 0:
            q = np.full(m, 2.0 * P)
            for _ in range(1, 2 * P + (1 if mutant == "dktt_exponent" else 0)):
                q = q * T[:, s]
            dk = c * q
        dvar[:, d] = -2.0 * _strided(wk * J) + dk
    out["dmu"], out["dvar"] = dmu, dvar
    return out


def restate(case, mutant=None):
    """The whole call in the device's order: the record ``judge`` takes."""
    n, ns = case.n, ns_of(case.n)
    T = case.T
    out = {"xs": case.xs}
    kb = kstar_restate(T, case.xs, case.k, ns, mutant)
    if case.route == "inverse":
        out["k"] = kb
        v = fwd_restate(case.A, kb, n, mutant)
        planes = bwd_restate(case.A, v, n, case.rc, case.nrc, mutant)
    else:
        v, w = solve_restate(case.A, kb[:, :n], n, mutant)
        planes = np.zeros((1, len(T), ns))
        planes[0][:, :n] = w
    out["v"], out["w"] = v, planes
    with np.errstate(all="ignore"):
        out.update(finish_restate(case.xs, T, case.k, case.mean, v, planes, case.rc, case.nrc, mutant))
    return out


def scipy_route(case):
    """The same record by NumPy / SciPy in their own order: k from the raw coordinates (``kernel``), BLAS products or
    LAPACK substitutions, einsum for the sums."""
    n, ns, k = case.n, ns_of(case.n), case.k
    prm = {"ndim": k.ndim, "amp": k.amp, "inv_metric": k.inv_metric, "lin_coef": k.lin_coef, "lin_order": k.lin_order}
    T = case.T
    kv, J = kernel(T, case.X, prm)
    if k.lin_coef != 0.0 and k.lin_order == 0:
        # the constant joins in ONE rounding, as in the device's fma: ``kernel`` rounds c * D on its own first, a second
        # rounding for which the half ulp that the budget gives this step has no room (1.74 of it at D = 17)
        kse = kernel(T, case.X, dict(prm, lin_coef=0.0))[0]
        kv = (kse.astype(LD) + LD(k.lin_coef) * LD(k.ndim)).astype(np.float64)
    A = np.tril(case.A)
    out = {"xs": case.xs}
    planes = np.zeros((case.nrc, len(T), ns))
    if case.route == "inverse":
        out["k"] = np.zeros((len(T), ns))
        out["k"][:, :n] = kv
        v = kv @ A.T
        for r in range(case.nrc):
            i0, i1 = r * case.rc, min(n, (r + 1) * case.rc)
            planes[r][:, :n] = v[:, i0:i1] @ A[i0:i1]
        w = planes[:, :, :n].sum(0)
    else:
        v = solve_triangular(A, kv.T, lower=True).T
        w = solve_triangular(A.T, v.T, lower=False).T
        planes[0][:, :n] = w
    ktt, dktt = kernel_diag(T, prm)
    out.update({"v": v, "w": planes, "mu": kv @ case.alpha + case.mean, "var": ktt - np.sum(v * v, axis=1),
                "dmu": np.einsum("n,mnd->md", case.alpha, J), "dvar": dktt - 2.0 * np.einsum("mn,mnd->md", w, J)})
    return out
