# -*- coding: utf-8 -*-
"""Reference of the posterior function draws of csrc/pathdraw.hip (apgp_path_draws).  Plain Python (NumPy, math.fsum,
tests/kvalue_ref.py): no GPU, no library import.

    g_s(t) = A sum_r W[s,r] cos(sqrt2 Z[r,:].ts + b_r) + sqrt(lin_coef) sum_d Wl[s,d] t_d^P      A = sqrt(2 amp / R)
    f_s(t) = mean + g_s(t) + sum_n k(t, x_n) V[n,s]                                              ts_d = t_d sqrt(inv_metric_d / 2)

``draws``     f_s(t) = math.fsum of its n + R + D + 1 summands (an exactly rounded sum): kernel values from
              kvalue_ref.truth_ld, the cosines of the long-double phase, each summand rounded once to a double.
``budget``    a componentwise bound of |device f_s(t) - truth| counted from the kernel's roundings (below).
``surrogate_variance`` the variance the draws have for FIXED Z, b: what the moment tests compare the sample variance to.
``argmin``    the arg-min contract of the record apgp_path_draws leaves per draw.

The device's operation sequence and the budget, term by term (u = 2^-53, eps = 2 u):

  phase    in turns: zt_rd = Z_rd (sqrt2 / 2 pi), bt_r = b_r (1 / 2 pi), p = fma chain bt + sum_d zt_rd ts_d over the D
           coordinates.  Roundings per term: ts (1), the constant sqrt2 / 2 pi (1), the fold (1), the chain (at most D);
           (D + 3) u <= (D + 2) eps.  Charged as (D + 2) eps (sum_d |zt_rd ts_d| + |bt_r|) turns, times 2 pi radians, times
           |d cos| <= 1.  This is the accuracy limit of a cosine of a computed phase whatever evaluates it.
  cosine   f = p - rint(p) exact; h = 1/4 - |f| exact unless |p| < 1/8 (then <= 2^-56 turns: inside the term below);
           sin(2 pi h) by an odd Taylor polynomial of degree 23 in h (truncation < 1e-20): 11 Horner steps, each rounding
           at most u times a partial sum below sinh(2 pi h) / h, coefficients rounded once, h^2 and the final product
           once each: below E_COS u absolute, E_COS = 6 (tests/test_pathdraw_ref.py holds the restated polynomial,
           which rounds products and sums separately, to it: 3.2 u at worst over 3e5 phases).
  A        2 amp / R rounds once, the square root once, the product with the sum once: 3 u A sum_r |W cos|.
  linear   t^P by P - 1 products, sqrt(lin_coef) once, the product with it once, the fma once: (P + 2) u per term.
  k V      kvalue_ref.budget (the same operation sequence as the sweep's k*) times |V[n,s]|.
  sums     one running sum per draw, n + R + D fused multiply-adds, the scaling by A and the mean: every summand passes
           at most n + R + D + 2 roundings of a partial sum bounded by |mean| + sum |summands|.  (A single draw is summed
           in four interleaved partial sums: fewer roundings per summand.  The matrix-core form adds the four products
           of a 4-row step to one running sum per instruction: no more roundings per summand than one FMA each.)
  truth    every summand of the reference is rounded once (u), the long-double cosine's argument carries 2^-63 relative:
           2 u sum |summands|.
No condition number enters: V is an input here.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kvalue_ref as kr  # noqa: E402

U = 2.0 ** -53
EPS = 2.0 ** -52
E_COS = 6.0
LD = np.longdouble
INV_2PI = float.fromhex("0x1.45f306dc9c883p-3")
MAX_DRAWS = 32
MAX_FEATURES = 65536
THREADS = 256             # candidates per workgroup (PD_THREADS)
# sin(2 pi h) / h in h^2: (-1)^k (2 pi)^(2k+1) / (2k+1)!, k = 0 .. 11, as csrc/pathdraw.hip has them
COS_COEF = tuple(float.fromhex(h) for h in (
    "0x1.921fb54442d18p+2", "-0x1.4abbce625be53p+5", "0x1.466bc6775aae2p+6", "-0x1.32d2cce62bd86p+6",
    "0x1.50783487ee782p+5", "-0x1.e3074fde8871fp+3", "0x1.e8f434d018d63p+1", "-0x1.6fadb9f155744p-1",
    "0x1.aaec32af93359p-4", "-0x1.8a404211f9547p-7", "0x1.2877020d52cf0p-10", "-0x1.7215f879e1ac9p-14"))


def work_len(m, ndraws):
    """apgp_path_draws_work_len."""
    if m < 1 or ndraws < 1:
        return 0
    if m > 1 << 40 or ndraws > MAX_DRAWS:
        return -1
    return 2 * ndraws * ((m + THREADS - 1) // THREADS)


def cos_turns_restate(p):
    """The kernel's cosine of a phase in turns, operation by operation (products and sums rounded separately where the
    device fuses them: at most one rounding more per step)."""
    p = np.asarray(p, dtype=np.float64)
    h = 0.25 - np.abs(p - np.rint(p))
    h2 = h * h
    acc = np.full_like(h, COS_COEF[-1])
    for c in COS_COEF[-2::-1]:
        acc = acc * h2 + c
    return h * acc


def feature_amp(k, R):
    return math.sqrt(2.0 * k.amp / R)


def phases(T, Z, b, k):
    """(M, R) long double: sqrt2 Z.ts + b = sum_d Z_rd t_d sqrt(inv_metric_d) + b_r, in radians."""
    w = np.sqrt(np.asarray(k.inv_metric, dtype=LD))
    return (np.asarray(T, dtype=LD) * w) @ np.asarray(Z, dtype=LD).T + np.asarray(b, dtype=LD)


def phase_budget(T, Z, b, k):
    """(M, R): bound of the computed phase's error in radians."""
    sc = np.sqrt(0.5 * np.asarray(k.inv_metric, dtype=np.float64))
    turns = np.abs(np.asarray(T) * sc) @ np.abs(np.asarray(Z) * (math.sqrt(2.0) * INV_2PI)).T + np.abs(b) * INV_2PI
    return (k.ndim + 2) * EPS * turns * (2.0 * math.pi)


def linear_features(T, k):
    """(M, D): sqrt(lin_coef) t_d^P (zeros without a linear term)."""
    T = np.asarray(T, dtype=np.float64)
    if k.lin_coef == 0.0:
        return np.zeros_like(T)
    return math.sqrt(k.lin_coef) * T ** k.lin_order


def features(T, Z, b, k):
    """(M, R + D) float64: the feature map phi(t) whose weights (W | Wl) make g_s = phi . w_s."""
    c = np.cos(phases(T, Z, b, k)).astype(np.float64)
    return np.hstack([feature_amp(k, len(Z)) * c, linear_features(T, k)])


def draws(T, X, V, Z, b, W, Wl, k, mean):
    """(S, M): f_s(t), every sum exactly rounded."""
    S = len(W)
    kk = kr.truth_ld(T, X, k) if V is not None else None
    phi = features(T, Z, b, k)
    out = np.empty((S, len(T)))
    for s in range(S):
        w = np.concatenate([W[s], Wl[s] if Wl is not None else np.zeros(k.ndim)])
        cols = [np.full((len(T), 1), float(mean)), phi * w]
        if V is not None:
            cols.append((kk * np.asarray(V[:, s], dtype=LD)).astype(np.float64))
        tt = np.hstack(cols)
        out[s] = [math.fsum(row) for row in tt]
    return out


def budget(T, X, V, Z, b, W, Wl, k, mean):
    """(S, M): componentwise bound of |device f_s(t) - truth|, and (S, M) |mean| + sum |summands|."""
    T = np.asarray(T, dtype=np.float64)
    S, R, D = len(W), len(Z), k.ndim
    n = len(X) if V is not None else 0
    A = feature_amp(k, R)
    cosv = np.abs(np.cos(phases(T, Z, b, k)).astype(np.float64))                 # (M, R)
    dcos = phase_budget(T, Z, b, k) + E_COS * U                                  # (M, R)
    aW = np.abs(W)                                                               # (S, R)
    feat_abs = A * (aW @ cosv.T)                                                 # (S, M) sum |A W cos|
    bud = A * (aW @ dcos.T) + 3.0 * U * feat_abs
    mag = abs(float(mean)) + feat_abs
    if k.lin_coef != 0.0:
        lin_abs = np.abs(Wl) @ np.abs(linear_features(T, k)).T                   # (S, M)
        bud += (k.lin_order + 2) * U * lin_abs
        mag = mag + lin_abs
    if V is not None:
        kb = kr.budget(T, X, k)                                                  # (M, n)
        kabs = np.abs(kr.truth_ld(T, X, k).astype(np.float64))
        bud += (kb @ np.abs(V)).T
        mag = mag + (kabs @ np.abs(V)).T
    bud += (n + R + D + 2) * U * mag + 2.0 * U * mag
    return bud, mag


def fast_draws(phiT, phiX, Kxt, Kinv_solve, y, mean, W, eps):
    """(S, M) draws by plain matrix products (the moment tests: statistics, not roundings).  phiT (M, F), phiX (n, F):
    feature maps; Kxt (n, M) = k(X, T); Kinv_solve(B) = K^-1 B; W (S, F) the weights (W | Wl); eps (S, n)."""
    gX = W @ phiX.T                                                              # (S, n)
    V = Kinv_solve((y - mean)[:, None] - gX.T - eps.T)                           # (n, S)
    return mean + W @ phiT.T + (Kxt.T @ V).T, V


def surrogate_variance(phiT, phiX, Kxt, Kinv_solve, diag_add):
    """(M,): variance of f_s(t) over W, eps ~ N(0, .) for fixed features:
    phi(t).phi(t) - 2 k K^-1 Phi(X) phi(t) + k K^-1 (Phi(X) Phi(X)^T + diag_add I) K^-1 k^T."""
    B = Kinv_solve(Kxt)                                                          # (n, M) = K^-1 k(X, t)
    PB = phiX.T @ B                                                              # (F, M)
    return (np.sum(phiT * phiT, axis=1) - 2.0 * np.sum(phiT.T * PB, axis=0)
            + np.sum(PB * PB, axis=0) + diag_add * np.sum(B * B, axis=0))


def admissible(T, bounds=None, mask=None):
    T = np.asarray(T, dtype=np.float64)
    adm = ~np.isnan(T).any(axis=1)
    if bounds is not None:
        bb = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore"):
            adm &= np.all((T >= bb[:, 0]) & (T <= bb[:, 1]), axis=1)
    if mask is not None:
        adm &= np.asarray(mask).astype(bool)
    return adm


def argmin(F, adm, idx_offset=0):
    """The record of one draw: (global index, u) of the smallest u = -f over the admissible rows; the lowest index on
    ties; NaN never wins; (-1, +inf) when nothing is admissible."""
    u = np.where(adm, -np.asarray(F, dtype=np.float64), np.inf)
    u = np.where(np.isnan(u), np.inf, u)
    if not np.any(u < np.inf):
        return -1, np.inf
    i = int(np.argmin(u))          # the first of equal minima
    return idx_offset + i, float(u[i])


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
LIN_COEF = {0: 0.05, 1: 0.3, 2: 0.1}


def case(n, m, R, S, D, order=None, seed=0, with_v=True):
    """A problem of the given shape with host-made weights: the training points in [-2, 2]^D, length scales of the order
    of their spacing, V of the size K^-1 y has for a well-conditioned K (an input, not a solve)."""
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2.0, 2.0, size=(n, D))
    T = rs.uniform(-2.2, 2.2, size=(m, D))
    ell = 4.0 / max(n ** (1.0 / D), 2.0) * rs.uniform(1.0, 3.0, size=D)
    k = kr.kern(1.0 / ell ** 2, amp=rs.uniform(0.5, 3.0), diag_add=1e-4,
                lin_coef=0.0 if order is None else LIN_COEF[order], lin_order=1 if order is None else order)
    Z = rs.standard_normal((R, D))
    b = rs.uniform(0.0, 2.0 * np.pi, R)
    W = rs.standard_normal((S, R))
    Wl = rs.standard_normal((S, D))
    V = rs.standard_normal((n, S)) * rs.uniform(0.1, 10.0, size=(n, 1)) if with_v else None
    return dict(X=X, T=T, k=k, Z=Z, b=b, W=W, Wl=Wl, V=V, mean=float(rs.uniform(-3.0, 3.0)))


def moment_fixture(seed=0, n=64, D=2, R=4096, m=16):
    """The moment tests' problem: diag_add = 1e-4 amp; fixed Z, b; the weights are redrawn per batch by the tests."""
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2.0, 2.0, size=(n, D))
    T = rs.uniform(-2.5, 2.5, size=(m, D))
    y = np.sin(2.0 * X).sum(axis=1) + 0.1 * (X ** 2).sum(axis=1)
    amp = 1.7
    k = kr.kern(1.0 / np.array([0.8, 1.1])[:D] ** 2, amp=amp, diag_add=1e-4 * amp)
    Z = rs.standard_normal((R, D))
    b = rs.uniform(0.0, 2.0 * np.pi, R)
    K = kr.truth_ld(X, None, k).astype(np.float64)
    K = np.tril(K) + np.tril(K, -1).T
    Kxt = kr.truth_ld(X, T, k).astype(np.float64)
    L = np.linalg.cholesky(K)

    def solve(B):
        return np.linalg.solve(L.T, np.linalg.solve(L, B))
    return dict(X=X, T=T, y=y, k=k, Z=Z, b=b, K=K, Kxt=Kxt, solve=solve, mean=float(np.mean(y)),
                phiT=features(T, Z, b, k), phiX=features(X, Z, b, k))


def moment_scores(F, mu, vhat):
    """z-scores of the sample mean (against mu, standard error sqrt(vhat / S)) and of the sample variance (s^2 / vhat
    against 1, standard error sqrt(2 / S)) of S draws F (S, M)."""
    S = len(F)
    zm = (F.mean(axis=0) - mu) / np.sqrt(vhat / S)
    zv = (F.var(axis=0, ddof=1) / vhat - 1.0) / math.sqrt(2.0 / S)
    return zm, zv
