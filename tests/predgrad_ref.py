"""NumPy restatement of ``apgp_predict_grad`` (include/apgp.h): the kernel of ``apgp_kernel_t`` with its linear term and
its derivative in the query point, the posterior mean / variance and their gradients through both K^-1 routes (SciPy
triangular solves), the utilities with their (mu, var) derivatives, and the non-finite table.  The checker of
tests/test_predgrad_ref.py and tests/test_gpu_predict_grad.py, never the thing shipped.

    k_n = k(t, x_n)                      J_nd   = d k(t, x_n) / d t_d
    mu  = k.alpha + mean                 dmu_d  = sum_n alpha_n J_nd
    v   = L^-1 k,  w = L^-T v            var    = k(t,t) - |v|^2
    dvar_d = d k(t,t) / d t_d - 2 sum_n w_n J_nd
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.special import erfc

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
