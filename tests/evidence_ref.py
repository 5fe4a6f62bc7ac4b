# -*- coding: utf-8 -*-
"""NumPy restatement of the evidence estimate (csrc/evidence.hip, utility.mergeImportance / importanceSummary,
ApproxPosterior.evidence) -- test infrastructure like philox_ref.py and prior_ref.py: the checker the device is held to,
never the thing shipped.  No GPU, no library import.

Mixture stream (mix_candidates_kernel).  Row g, key = seed: Philox4x32-10 with counter (g low, g high, j, 0x4d495854
"MIXT").  j = 0: u = u01(words 0, 1) picks the first component k with u < cumw[k] (cumw summed sequentially, the last
entry forced to 1.0).  j = 1 + d / 2: words 0, 1 give dimension d's uniform, words 2, 3 dimension d + 1's; z_d = sqrt(2)
erfcinv(2 (1 - u)) (prior_ref.gaussian(0, 1, u): scipy's erfcinv in place of the device's); t_i = c_i + sum_{j <= i}
A_ij z_j with A the lower Cholesky factor of covScale x covariance.

Weights (imp_logw_kernel).  logw = mu - lnq where every coordinate is finite and inside the gate and mu, lnq are finite,
else -inf; mu = sum_n k(t, x_n) alpha_n + mean, here from kvalue_ref.truth_ld (long double, 2^-9 ulp per value).

Record.  lmax = max logw; e = exp(logw - lmax), 0 below -700 and for -inf; S0 = sum e, S2 = sum e^2, cnt = finite rows,
s1 = sum e (t - c), S = sum e (t - c)(t - c)^T, all in long double here."""
import numpy as np

import kvalue_ref as kr
from philox_ref import philox4x32_10, u01
from prior_ref import gaussian

_MASK = np.uint64(0xFFFFFFFF)
MIX_TAG = 0x4D495854
LD = np.longdouble
U = 2.0 ** -53


# ----------------------------------------------------------------------------------------------------------------------
# mixture proposal
# ----------------------------------------------------------------------------------------------------------------------
def mix_uniforms(m, D, seed, offset):
    """(component uniforms (m,), dimension uniforms (m, D)) of rows offset .. offset + m - 1."""
    rows = np.arange(m, dtype=np.uint64) + np.uint64(offset)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF
    lo, hi = rows & _MASK, rows >> np.uint64(32)
    c = philox4x32_10(lo, hi, 0, MIX_TAG, k0, k1)
    uc = u01(c[0], c[1])
    u = np.empty((m, D))
    for d in range(0, D, 2):
        c = philox4x32_10(lo, hi, 1 + (d >> 1), MIX_TAG, k0, k1)
        u[:, d] = u01(c[0], c[1])
        if d + 1 < D:
            u[:, d + 1] = u01(c[2], c[3])
    return uc, u


def cumulative(weights):
    """The cumulative weights as the host forms them: normalised, summed sequentially, capped at 1, the last forced to 1."""
    w = np.asarray(weights, dtype=np.float64)
    w = w / w.sum()
    cum, run = np.empty(len(w)), 0.0
    for k in range(len(w)):
        run = min(run + w[k], 1.0)
        cum[k] = run
    cum[-1] = 1.0
    return w, cum


def mix_candidates_numpy(m, weights, means, covs, seed, offset=0, covScale=1.0):
    """Rows offset .. offset + m - 1 of the mixture draws: (T (m, D), component (m,), z (m, D), near (m,) bool -- the
    component uniform lies within 1 ulp of a cumulative weight, where the device may legitimately differ only if the
    host's cumulative sums did; they do not, so ``near`` rows are skipped for safety and counted)."""
    means = np.atleast_2d(np.asarray(means, dtype=np.float64))
    covs = np.asarray(covs, dtype=np.float64)
    K, D = means.shape
    _, cum = cumulative(weights)
    uc, u = mix_uniforms(m, D, seed, offset)
    comp = np.minimum(np.searchsorted(cum, uc, side="right"), K - 1)      # the first k with u < cum[k]
    near = np.zeros(m, dtype=bool)
    for k in range(K - 1):
        near |= np.abs(uc - cum[k]) <= np.spacing(cum[k])
    z = gaussian(0.0, 1.0, u)
    A = np.array([np.linalg.cholesky(covScale * covs[k]) for k in range(K)])
    T = means[comp] + np.einsum("mij,mj->mi", A[comp], z)
    return T, comp, z, near, A


def mix_draw_bound(T, comp, z, A, gauss_k):
    """|device - restatement| per entry: the Gaussian-draw bound of tests/test_gpu_priors.py (GAUSS_K eps (sigma (1 + |z|)
    + |x|), eps = 2^-52) carried through |A_k| row by row, plus the (i + 2) roundings of the fma chain and the closing
    addition on sum_j |A_ij z_j|."""
    eps = 2.0 ** -52
    absA = np.abs(A[comp])
    D = T.shape[1]
    spread = np.einsum("mij,mj->mi", absA, 1.0 + np.abs(z))
    mag = np.einsum("mij,mj->mi", absA, np.abs(z))
    return gauss_k * eps * (spread + np.abs(T)) + (np.arange(D)[None, :] + 2.0) * U * mag


# K, D, seed of the mixtures the GPU test draws (K in {1, 3, 16}, D in {1, 3, 8})
MIX_CASES = ((1, 1, 101), (3, 3, 102), (16, 8, 103), (3, 1, 104), (1, 8, 105), (16, 3, 106))


def mixture(K, D, seed):
    """A seeded full-covariance mixture: (weights (K,), means (K, D), covariances (K, D, D))."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.2, 1.0, size=K)
    means = rs.uniform(-2.0, 2.0, size=(K, D))
    B = rs.normal(size=(K, D, D))
    covs = 0.3 * np.einsum("kij,klj->kil", B, B) / D + 0.05 * np.eye(D)
    return w / w.sum(), means, covs


def mix_logpdf(T, weights, means, covs, covScale=1.0):
    """NumPy's mixture log-density of the rows of T in long double: (lnq (m,), budget (m,)).  The budget follows the
    device's operations per component: z = t - c rounds once (u |z_i|, amplified by |U| into y), y_j is an fma chain of
    j + 1 terms ((j + 2) u sum_i |z_i U_ij|), quad sums D squares ((D + 1) u quad, and 2 |y_j| dy_j): about D^2
    operations in all; then -0.5 (D log 2pi + quad) + log det + log w (4 roundings at the magnitude of the terms), exp
    and log of the log-sum-exp at 2 ulp each and K additions."""
    means = np.atleast_2d(np.asarray(means, dtype=np.float64))
    covs = np.asarray(covs, dtype=np.float64) * covScale
    K, D = means.shape
    w, _ = cumulative(weights)
    lp = np.empty((len(T), K), dtype=LD)
    bud = np.zeros((len(T), K))
    for k in range(K):
        A = np.linalg.cholesky(covs[k])
        Um = np.linalg.inv(A).T                                  # precision = U U^T
        zz = (T - means[k]).astype(LD)
        yv = zz @ Um.astype(LD)
        quad = np.sum(yv * yv, axis=1)
        logdet = np.sum(np.log(np.diag(Um)))
        with np.errstate(divide="ignore"):
            lw = np.log(w[k])
        lp[:, k] = -0.5 * (D * np.log(2 * np.pi) + quad) + logdet + lw
        absy = np.abs(zz).astype(np.float64) @ np.abs(Um)
        # (+ D cond(A): the device's U comes from a triangular solve on the host, backward-stable: |dU| <= D u cond |U|)
        dy = (np.arange(D)[None, :] + 3.0 + D * np.linalg.cond(A)) * U * absy
        bud[:, k] = (np.sum(2.0 * np.abs(yv).astype(np.float64) * dy, axis=1) + (D + 1) * U * quad.astype(np.float64)) * 0.5 \
            + 4 * U * (0.5 * (D * np.log(2 * np.pi) + quad.astype(np.float64)) + abs(logdet) + (abs(lw) if np.isfinite(lw) else 0.0))
    mx = lp.max(axis=1)
    lnq = mx + np.log(np.sum(np.exp(lp - mx[:, None]), axis=1))
    budget = bud.max(axis=1) * (1.0 + 2.0 ** -20) + (K + 4 + 1) * U * (1.0 + np.abs(lnq.astype(np.float64)))
    return lnq, budget


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
def mean_truth(T, X, alpha, k, mean, chunk=4096):
    """(mu (m,) long double, sum_n |k_n alpha_n| (m,), sum_n budget_n |alpha_n| (m,)) of the GP mean at the rows of T."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    al = np.asarray(alpha, dtype=np.float64)
    mu = np.empty(len(T), dtype=LD)
    mag, bud = np.empty(len(T)), np.empty(len(T))
    for i in range(0, len(T), chunk):
        kv = kr.truth_ld(T[i:i + chunk], X, k)
        mu[i:i + chunk] = kv @ al.astype(LD) + LD(mean)
        mag[i:i + chunk] = np.abs(kv).astype(np.float64) @ np.abs(al)
        bud[i:i + chunk] = kr.budget(T[i:i + chunk], X, k) @ np.abs(al)
    return mu, mag, bud


def admissible(T, lnq, mu, bounds):
    T = np.atleast_2d(T)
    ok = np.all(np.isfinite(T), axis=1) & np.isfinite(np.asarray(mu, dtype=np.float64))
    if lnq is not None:
        ok &= np.isfinite(lnq)
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore"):
            ok &= np.all((T >= b[:, 0]) & (T <= b[:, 1]), axis=1)
    return ok


def logw_truth(T, X, alpha, k, mean, lnq=None, bounds=None):
    """(logw (m,) long double with -inf for gated rows, budget (m,)): the issue's bound
    (N + 2) u sum_n |k_n alpha_n| + sum_n budget_n |alpha_n| + u (|mu| + |lnq|)."""
    mu, mag, bud = mean_truth(T, X, alpha, k, mean)
    ok = admissible(T, lnq, mu, bounds)
    lq = np.zeros(len(mu)) if lnq is None else np.asarray(lnq, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lw = np.where(ok, mu - np.where(ok, lq, 0.0).astype(LD), LD(-np.inf))
    budget = (len(X) + 2) * U * mag + bud + U * (np.abs(mu.astype(np.float64)) + np.where(ok, np.abs(lq), 0.0))
    return lw, budget


# ----------------------------------------------------------------------------------------------------------------------
# record, merge, summary
# ----------------------------------------------------------------------------------------------------------------------
def record(logw, T, centre):
    """The record of rows with log-weights ``logw`` (any float type; -inf = gated) about ``centre``, in long double."""
    lw = np.asarray(logw, dtype=LD)
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    c = np.asarray(centre, dtype=np.float64)
    D = len(c)
    fin = lw > -np.inf
    if not fin.any():
        return {"lmax": -np.inf, "S0": 0.0, "S2": 0.0, "cnt": 0.0, "s1": np.zeros(D), "S": np.zeros((D, D)), "centre": c}
    lmax = lw[fin].max()
    d = lw[fin] - lmax
    e = np.where(d < -700.0, LD(0.0), np.exp(np.maximum(d, LD(-700.0))))
    dx = (T[fin] - c).astype(LD)            # (the device rounds t - c once to double: restated)
    return {"lmax": float(lmax), "S0": float(e.sum()), "S2": float((e * e).sum()), "cnt": float(fin.sum()),
            "s1": (e[:, None] * dx).sum(axis=0).astype(np.float64),
            "S": np.einsum("m,mi,mj->ij", e, dx, dx).astype(np.float64), "centre": c}


def merge(a, b):
    """utility.mergeImportance restated."""
    assert np.array_equal(a["centre"], b["centre"])
    l = max(a["lmax"], b["lmax"])
    fa = np.exp(a["lmax"] - l) if a["lmax"] > -np.inf else 0.0
    fb = np.exp(b["lmax"] - l) if b["lmax"] > -np.inf else 0.0
    return {"lmax": l, "centre": a["centre"], "cnt": a["cnt"] + b["cnt"],
            "S0": fa * a["S0"] + fb * b["S0"], "S2": fa * fa * a["S2"] + fb * fb * b["S2"],
            "s1": fa * a["s1"] + fb * b["s1"], "S": fa * a["S"] + fb * b["S"]}


def summary(rec, m, logVolume=0.0):
    """utility.importanceSummary restated (records with S0 > 0)."""
    S0, S2 = rec["S0"], rec["S2"]
    d = rec["s1"] / S0
    return {"logZ": rec["lmax"] + np.log(S0) - np.log(float(m)) + logVolume,
            "logZErr": np.sqrt(max(m * S2 / S0 ** 2 - 1.0, 0.0) / m), "ess": S0 ** 2 / S2,
            "mean": rec["centre"] + d, "cov": rec["S"] / S0 - np.outer(d, d), "nInside": int(rec["cnt"])}


def record_budget(logw, T, centre, m=None):
    """Relative bounds of the device record against ``record`` of the SAME log-weights: (on S0, on S2, absolute on s1 (D,),
    absolute on S (D, D)).  Per row e carries E_EXP ulps of apgp_exp plus the rounding of logw - lmax (u |d| relative in
    e); the sums are recursive in some fixed order of m terms: m u relative on sums of non-negative terms (S0, S2; e^2
    doubles e's relative error and rounds once) and m u sum |term| on the signed ones, whose terms carry 2 (s1) or 3 (S)
    more roundings."""
    lw = np.asarray(logw, dtype=np.float64)
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    fin = lw > -np.inf
    m = len(lw) if m is None else m
    if not fin.any():
        D = T.shape[1]
        return 0.0, 0.0, np.zeros(D), np.zeros((D, D))
    d = lw[fin] - lw[fin].max()
    e = np.where(d < -700.0, 0.0, np.exp(np.maximum(d, -700.0)))
    rel = 2.0 * kr.E_EXP * U + U * np.abs(d) + U
    S0 = e.sum()
    b0 = m * U + (e * rel).sum() / S0
    b2 = m * U + ((e * e) * (2.0 * rel + U)).sum() / (e * e).sum()
    dx = np.abs(T[fin] - np.asarray(centre))
    t1 = e[:, None] * dx
    b1 = (m + 2) * U * t1.sum(axis=0) + (t1 * rel[:, None]).sum(axis=0)
    tS = np.einsum("m,mi,mj->mij", e, dx, dx)
    bS = (m + 3) * U * tS.sum(axis=0) + (tS * rel[:, None, None]).sum(axis=0)
    tiny = 2.0 ** -1000
    return b0, b2, b1 + tiny, bS + tiny


# ----------------------------------------------------------------------------------------------------------------------
# the D = 2 quadratic case of the end-to-end tests
# ----------------------------------------------------------------------------------------------------------------------
EVIDENCE_SEED = 20261020          # the seed of the box-proposal estimate, CPU and GPU (tests/test_evidence_ref.py checks it)
EVIDENCE_M = 2 ** 16
QUAD_BOUNDS = [(-3.0, 3.0), (-2.5, 3.5)]


def quadratic_case():
    """A surrogate fitted to a D = 2 quadratic log-density on N = 60 seeded points: (X, y, metric, mean, white_noise)."""
    rs = np.random.RandomState(60)
    b = np.asarray(QUAD_BOUNDS)
    X = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(size=(60, 2))
    P = np.array([[1.6, 0.5], [0.5, 0.9]])
    d = X - np.array([0.3, 0.6])
    y = -0.5 * np.einsum("ni,ij,nj->n", d, P, d) - 1.25
    return X, y, np.array([9.0, 12.0]), float(np.median(y)), -14.0


def oracle_gp(case):
    """The oracle GP of ``quadratic_case`` (oracle/george_oracle.py) and its alpha."""
    import george_oracle as go
    X, y, metric, mean, wn = case
    gp = go.GP(kernel=go.ExpSquaredKernel(metric, ndim=2), fit_mean=True, mean=mean, white_noise=wn, fit_white_noise=False)
    gp.compute(X)
    alpha = gp.apply_inverse(y - mean)
    return gp, np.asarray(alpha, dtype=np.float64).ravel()


def quadrature(case, n=400, bounds=None):
    """(log Z, mean (2,), cov (2, 2)) of exp(mu) over ``bounds`` (default QUAD_BOUNDS) by an n x n trapezoid rule on the
    oracle's mean."""
    gp, _ = oracle_gp(case)
    X, y = case[0], case[1]
    b = np.asarray(QUAD_BOUNDS if bounds is None else bounds)
    g0, g1 = np.linspace(b[0, 0], b[0, 1], n), np.linspace(b[1, 0], b[1, 1], n)
    G = np.stack(np.meshgrid(g0, g1, indexing="ij"), axis=-1).reshape(-1, 2)
    mu = np.asarray(gp.predict(y, G, return_cov=False)).reshape(n, n)
    w0, w1 = np.full(n, g0[1] - g0[0]), np.full(n, g1[1] - g1[0])
    w0[[0, -1]] *= 0.5
    w1[[0, -1]] *= 0.5
    mx = mu.max()
    f = np.exp(mu - mx) * w0[:, None] * w1[None, :]
    Z = f.sum()
    p = (f / Z).reshape(-1)
    mean = p @ G
    dG = G - mean
    return mx + np.log(Z), mean, np.einsum("m,mi,mj->ij", p, dG, dG)
