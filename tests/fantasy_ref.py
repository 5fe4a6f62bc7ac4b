"""NumPy restatement of the batch design-point selection (GP.acquire_batch / apgp_acquire_fantasy; DESIGN.md "Batch
design points") and the naive re-conditioning it must agree with.

GP: k(x, x') = amp exp(-0.5 sum_d (x_d - x'_d)^2 inv_metric_d) + lin_coef sum_d (x_d x'_d)^P, K = k(X, X) + diag_add I,
predictive mean k(t, X) K^-1 (y - mean) + mean, variance k(t, t) - k(t, X) K^-1 k(X, t).

fantasy_batch: one full prediction, then per step j the rank-one downdate
    s_j = v_{j-1}(x_j) + diag_add,  beta_j = K^-1 k(X, x_j),
    c_j(t) = k(t, x_j) - k(t, X) beta_j - sum_{i<j} C_i(t) C_i(x_j),  C_j = c_j / sqrt(s_j),  v_j = v_{j-1} - C_j^2
recondition_batch: the slow path -- the training set extended by the picks at their predicted means, K refactorised
and mu / sigma^2 recomputed from scratch at every step."""
import numpy as np
from scipy.special import erfc

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
        xj = T[b:b + 1]
        kx = kernel(X, xj, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"])[:, 0]
        beta = np.linalg.solve(L.T, np.linalg.solve(L, kx))
        c = kernel(T, xj, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"])[:, 0] \
            - kernel(T, X, gp["amp"], gp["inv_metric"], gp["lin_coef"], gp["lin_order"]) @ beta
        for ci in cols:
            c = c - ci * ci[b]
        ch = c / np.sqrt(v[b] + gp["diag_add"])
        cols.append(ch)
        v = v - ch * ch
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
