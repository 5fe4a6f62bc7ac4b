"""NumPy restatement of Gaussian-mixture EM (test infrastructure, like philox_ref.py): the checker the device passes
of gmmUtils / csrc/gmm.hip are compared against, written from the formulas.

  log N(x | mu_k, Sigma_k) = -(D log 2 pi + |(x - mu_k) U_k|^2) / 2 + sum_d log (U_k)_dd,  U_k U_k^T = Sigma_k^-1
  log_prob_norm = logsumexp_k (log N_k + log w_k),  r_k = exp(log N_k + log w_k - log_prob_norm)
  M-step: nk = sum r + 10 eps, mu = sum r x / nk, Sigma by covariance type + reg_covar on the diagonal, w = nk / sum nk,
          U = inv(chol(Sigma))^T
"""
import numpy as np

EPS10 = 10.0 * np.finfo(np.float64).eps
LOG2PI = np.log(2.0 * np.pi)


def full_prec_chol(pc, cov_type, K, D):
    if cov_type == "full":
        return np.asarray(pc)
    if cov_type == "tied":
        return np.broadcast_to(pc, (K, D, D))
    if cov_type == "diag":
        return np.asarray(pc)[:, :, None] * np.eye(D)
    return np.asarray(pc)[:, None, None] * np.eye(D)


def weighted_log_prob(X, weights, means, U):
    """(n, K): log N(x | mu_k, Sigma_k) + log w_k, U: (K, D, D) upper precision Cholesky factors."""
    n, D = X.shape
    out = np.empty((n, len(weights)))
    with np.errstate(divide="ignore"):
        logw = np.log(weights)
    for k in range(len(weights)):
        y = (X - means[k]) @ U[k]
        out[:, k] = (-0.5 * (D * LOG2PI + np.sum(y * y, axis=1)) + np.sum(np.log(np.diag(U[k])))) + logw[k]
    return out


def e_step(X, weights, means, U):
    """(log_prob_norm (n), labels (n), responsibilities (n, K))"""
    lp = weighted_log_prob(X, weights, means, U)
    mx = lp.max(axis=1)
    lpn = mx + np.log(np.sum(np.exp(lp - mx[:, None]), axis=1))
    return lpn, np.argmax(lp, axis=1), np.exp(lp - lpn[:, None])


def centred_stats(X, w, centres):
    """the record of apgp_gmm_pass for row weights w (n, K) about centres c_k (G excluded):
    per component (sum w, sum w (x - c), packed upper sum w (x - c)(x - c)^T)"""
    D = X.shape[1]
    j = np.repeat(np.arange(D), np.arange(1, D + 1))
    i = np.concatenate([np.arange(c + 1) for c in range(D)])
    rec = []
    for k in range(w.shape[1]):
        z = X - centres[k]
        S = (w[:, k:k + 1] * z).T @ z
        rec.append(np.concatenate([[np.sum(w[:, k])], w[:, k] @ z, S[i, j]]))
    return np.concatenate(rec)


def em_pass(X, weights, means, U):
    """(record of an APGP_GMM_EM pass, log_prob_norm, labels)"""
    lpn, lab, r = e_step(X, weights, means, U)
    return np.concatenate([[np.sum(lpn)], centred_stats(X, r, means)]), lpn, lab


def kmeans_pass(X, centres):
    """(record of an APGP_GMM_KMEANS pass, squared distance, labels)"""
    d2 = np.stack([np.sum((X - c) ** 2, axis=1) for c in centres], axis=1)
    lab = np.argmin(d2, axis=1)
    best = d2[np.arange(len(X)), lab]
    onehot = np.zeros_like(d2)
    onehot[np.arange(len(X)), lab] = 1.0
    return np.concatenate([[np.sum(best)], centred_stats(X, onehot, centres)]), best, lab


def m_step(X, r, cov_type, reg):
    """(weights, means, covariances, precisions_cholesky) in the shapes of sklearn's attributes"""
    n, D = X.shape
    nk = r.sum(axis=0) + EPS10
    means = (r.T @ X) / nk[:, None]
    K = len(nk)
    full = np.empty((K, D, D))
    for k in range(K):
        z = X - means[k]
        full[k] = (r[:, k:k + 1] * z).T @ z / nk[k]
    if cov_type == "full":
        cov = full + reg * np.eye(D)
    elif cov_type == "tied":
        cov = np.sum(nk[:, None, None] * full, axis=0) / nk.sum() + reg * np.eye(D)
    else:
        diag = np.diagonal(full, axis1=1, axis2=2) + reg
        cov = diag if cov_type == "diag" else diag.mean(axis=1)
    if cov_type in ("full", "tied"):
        mats = cov if cov_type == "full" else cov[None]
        pc = np.array([np.linalg.inv(np.linalg.cholesky(c)).T for c in mats])
        pc = pc if cov_type == "full" else pc[0]
    else:
        pc = 1.0 / np.sqrt(cov)
    return nk / nk.sum(), means, cov, pc


def prec_chol_from_precisions(prec, cov_type):
    """upper U with U U^T = precision"""
    if cov_type in ("full", "tied"):
        mats = prec if cov_type == "full" else prec[None]
        J = np.eye(mats.shape[-1])[::-1]
        pc = np.array([J @ np.linalg.cholesky(J @ p @ J) @ J for p in mats])
        return pc if cov_type == "full" else pc[0]
    return np.sqrt(prec)


def em_fit(X, weights, means, precisions, cov_type, reg=1e-6, max_iter=100, tol=1e-3):
    """EM from explicit initial parameters: (weights, means, covariances, precisions_cholesky, lower_bound, n_iter)"""
    n, D = X.shape
    K = len(weights)
    w, mu, pc, cov = np.asarray(weights, float), np.asarray(means, float), prec_chol_from_precisions(
        np.asarray(precisions, float), cov_type), None
    lb, it = -np.inf, 0
    for it in range(1, max_iter + 1):
        prev = lb
        lpn, _, r = e_step(X, w, mu, full_prec_chol(pc, cov_type, K, D))
        w, mu, cov, pc = m_step(X, r, cov_type, reg)
        lb = lpn.mean()
        if abs(lb - prev) < tol:
            break
    return w, mu, cov, pc, lb, it
