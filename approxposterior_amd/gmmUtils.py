# -*- coding: utf-8 -*-
"""
:py:mod:`gmmUtils.py` - Gaussian Mixture Model Utilities
--------------------------------------------------------

``fitGMM`` (the reference's ``approxposterior.gmmUtils.fitGMM``): a Gaussian mixture
fitted to posterior samples, the number of components chosen by the BIC or by
5-fold cross-validation.  Every pass over the samples -- k-means assignment, the
E-step with its sufficient statistics, scoring -- is one HIP kernel
(csrc/gmm.hip, ``apgp_gmm_pass``); the per-iteration M-step (K Cholesky factors
of D x D) runs in NumPy on the host.  Each EM iteration is sklearn's
``GaussianMixture`` iteration, and the result IS a fitted
``sklearn.mixture.GaussianMixture`` whose ``bic``, ``score``, ``predict`` and
``sample`` work on the host unchanged.  sklearn is imported only when
``fitGMM`` runs.
"""

__all__ = ["fitGMM"]

import ctypes

import numpy as np

from . import _lib

_COV_TYPES = ("full", "tied", "diag", "spherical")
_OPTIONS = ("n_components", "covariance_type", "tol", "reg_covar", "max_iter", "n_init", "random_state",
            "weights_init", "means_init", "precisions_init", "init_params")
_DEFAULTS = dict(n_components=1, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 random_state=None, weights_init=None, means_init=None, precisions_init=None, init_params="kmeans")
_KMEANS_SUBSAMPLE = 1 << 16      # rows the host's k-means++ seeding sees
_KMEANS_MAX_ITER = 300
_NK_EPS = 10.0 * np.finfo(np.float64).eps
_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance "
                "(for instance caused by singleton or collapsed samples). Try to decrease the number of components, "
                "increase reg_covar, or scale the input data.")


def _triu_colmajor(D):
    """(rows, cols) of the upper triangle packed column by column: U[i][j] at j(j+1)/2 + i (include/apgp.h)."""
    j = np.repeat(np.arange(D), np.arange(1, D + 1))
    i = np.concatenate([np.arange(c + 1) for c in range(D)])
    return i, j


class _Device(object):
    """The samples on the device and the buffers of ``apgp_gmm_pass``."""

    def __init__(self, samples):
        import torch
        self.torch = torch
        if isinstance(samples, torch.Tensor):
            if not samples.is_cuda or samples.dtype != torch.float64:
                raise ValueError("samples: a tensor must be float64 on a CUDA device")
            if samples.dim() != 2 or not samples.is_contiguous():
                raise ValueError("samples: a tensor must be 2-D and contiguous")
            self.X = samples
        else:
            arr = np.ascontiguousarray(np.asarray(samples, dtype=np.float64))
            if arr.ndim != 2:
                raise ValueError("samples must be an (n, D) array")
            if not torch.cuda.is_available():
                raise RuntimeError("fitGMM needs a GPU: the mixture passes are HIP kernels (no CPU fallback)")
            self.X = torch.from_numpy(arr).to("cuda")          # the one upload of this fitGMM call
        n, D = self.X.shape
        if D < 1 or D > _lib.MAX_DIM:
            raise ValueError("samples: 1 <= D <= %d (APGP_MAX_DIM) required, got D = %d" % (_lib.MAX_DIM, D))
        if n < 1 or n >= 2 ** 31:
            raise ValueError("samples: 1 <= n < 2^31 rows required, got %d" % n)
        self.n, self.D = int(n), int(D)
        self.dev = self.X.device
        self.lib = _lib.load()
        self.tri = _triu_colmajor(self.D)
        self._bufs = {}

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _buffers(self, K):
        b = self._bufs.get(K)
        if b is None:
            torch = self.torch
            np_ = int(self.lib.apgp_gmm_params_len(self.D, K))
            ns = int(self.lib.apgp_gmm_stats_len(self.D, K))
            if np_ < 0 or ns < 0:
                raise ValueError("n_components must be in 1..%d, got %d" % (_lib.GMM_MAX_COMP, K))
            b = (torch.empty(np_, dtype=torch.float64, device=self.dev),
                 torch.empty(ns, dtype=torch.float64, device=self.dev))
            self._bufs[K] = b
        return b

    def run(self, X, params, mode, K, row_lp=None, row_label=None):
        """One pass over the rows of ``X`` (a contiguous device tensor) with the packed ``params``;
        returns the reduced statistics on the host."""
        torch = self.torch
        p_d, s_d = self._buffers(K)
        p_d.copy_(torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64).ravel()))
        st = self.lib.apgp_gmm_pass(
            ctypes.c_void_p(X.data_ptr()), int(X.shape[0]), self.D, K, ctypes.c_void_p(p_d.data_ptr()), mode,
            ctypes.c_void_p(s_d.data_ptr()),
            ctypes.c_void_p(row_lp.data_ptr() if row_lp is not None else None),
            ctypes.c_void_p(row_label.data_ptr() if row_label is not None else None), self.stream())
        _lib.check(st, "apgp_gmm_pass")
        if mode == _lib.GMM_SCORE:
            return s_d[:1].cpu().numpy()
        return s_d.cpu().numpy()

    # -- packing --------------------------------------------------------------------------------------------------
    def pack(self, weights, centres, prec_chol_full):
        """params of apgp_gmm_pass from log-weights, centres and (K, D, D) upper precision Cholesky factors."""
        i, j = self.tri
        with np.errstate(divide="ignore"):
            logw = np.log(weights)
        logdet = np.sum(np.log(np.diagonal(prec_chol_full, axis1=1, axis2=2)), axis=1)
        return np.concatenate([logw[:, None], logdet[:, None], centres, prec_chol_full[:, i, j]], axis=1)

    def kmeans_pack(self, centres):
        K, D = centres.shape
        return self.pack(np.ones(K), centres, np.broadcast_to(np.eye(D), (K, D, D)))

    def unpack_stats(self, st, K):
        """(G, s0 (K), s1 (K, D), S (K, D, D) symmetric) from apgp_gmm_pass's record."""
        D = self.D
        per = st[1:].reshape(K, 1 + D + D * (D + 1) // 2)
        i, j = self.tri
        S = np.zeros((K, D, D))
        S[:, i, j] = per[:, 1 + D:]
        S[:, j, i] = per[:, 1 + D:]
        return st[0], per[:, 0], per[:, 1:1 + D], S


# -- covariance-type algebra (host) -----------------------------------------------------------------------------------
def _full_prec_chol(pc, cov_type, K, D):
    """precisions_cholesky_ of any covariance type as (K, D, D) upper-triangular factors."""
    if cov_type == "full":
        return pc
    if cov_type == "tied":
        return np.broadcast_to(pc, (K, D, D))
    if cov_type == "diag":
        return pc[:, :, None] * np.eye(D)
    return pc[:, None, None] * np.eye(D)


def _prec_chol_from_cov(cov, cov_type):
    from scipy import linalg
    if cov_type in ("full", "tied"):
        mats = cov if cov_type == "full" else cov[None]
        out = np.empty_like(mats)
        for k, c in enumerate(mats):
            try:
                L = linalg.cholesky(c, lower=True)
            except linalg.LinAlgError:
                raise ValueError(_ILL_DEFINED)
            out[k] = linalg.solve_triangular(L, np.eye(c.shape[0]), lower=True).T
        return out if cov_type == "full" else out[0]
    if np.any(np.less_equal(cov, 0.0)):
        raise ValueError(_ILL_DEFINED)
    return 1.0 / np.sqrt(cov)


def _prec_chol_from_prec(prec, cov_type):
    """Upper U with U U^T = precision: the lower Cholesky factor of the row- and column-reversed matrix, reversed."""
    from scipy import linalg
    if cov_type in ("full", "tied"):
        mats = prec if cov_type == "full" else prec[None]
        out = np.array([linalg.cholesky(p[::-1, ::-1], lower=True)[::-1, ::-1] for p in mats])
        return out if cov_type == "full" else out[0]
    return np.sqrt(prec)


def _precisions(pc, cov_type):
    if cov_type == "full":
        return np.einsum("kij,klj->kil", pc, pc)
    if cov_type == "tied":
        return pc @ pc.T
    return pc ** 2


def _n_parameters(K, D, cov_type):
    cov = {"full": K * D * (D + 1) / 2.0, "diag": K * D, "tied": D * (D + 1) / 2.0, "spherical": K}[cov_type]
    return int(cov + K * D + K - 1)


def _m_step(dev, st, centres, K, cov_type, reg):
    """weights, means, covariances, precisions_cholesky_ from a pass's statistics about ``centres``
    (mu = c + delta, Sigma_k = S_k / nk - delta delta^T: no cancellation when |mu| >> sigma)."""
    D = dev.D
    _, s0, s1, S = dev.unpack_stats(st, K)
    nk = s0 + _NK_EPS
    delta = s1 / nk[:, None]
    means = centres + delta
    cov_full = S / nk[:, None, None] - delta[:, :, None] * delta[:, None, :]
    if cov_type == "full":
        cov = cov_full.copy()
        cov[:, np.arange(D), np.arange(D)] += reg
    elif cov_type == "tied":
        cov = np.sum(nk[:, None, None] * cov_full, axis=0) / np.sum(nk)
        cov[np.arange(D), np.arange(D)] += reg
    else:
        diag = np.diagonal(cov_full, axis1=1, axis2=2) + reg
        cov = diag if cov_type == "diag" else diag.mean(axis=1)
    return nk, means, cov, _prec_chol_from_cov(cov, cov_type)


# -- k-means initialisation -------------------------------------------------------------------------------------------
def _column_variance(dev, X):
    """per-feature variance of the rows of X: one k-means pass with a single centre at the first row."""
    c = X[:1].cpu().numpy()
    st = dev.run(X, dev.kmeans_pack(c), _lib.GMM_KMEANS, 1)
    _, s0, s1, S = dev.unpack_stats(st, 1)
    d = s1[0] / s0[0]
    return np.diagonal(S[0]) / s0[0] - d * d


def _kmeans_labels_stats(dev, X, K, rs):
    """k-means++ seeding on a uniform subsample (host), Lloyd iterations over all rows (device) with sklearn's
    stopping rule, and the pass at the final centres -- whose one-hot statistics are the initial M-step's."""
    from sklearn.cluster import kmeans_plusplus
    n = int(X.shape[0])
    m = min(n, _KMEANS_SUBSAMPLE)
    if m < n:
        idx = np.sort(rs.randint(0, n, size=m))
        sub = X[dev.torch.from_numpy(idx).to(dev.dev)].cpu().numpy()
    else:
        sub = X.cpu().numpy()
    centres, _ = kmeans_plusplus(sub, K, random_state=rs)
    tol = 1e-4 * float(np.mean(_column_variance(dev, X)))
    for _ in range(_KMEANS_MAX_ITER):
        st = dev.run(X, dev.kmeans_pack(centres), _lib.GMM_KMEANS, K)
        _, s0, s1, _S = dev.unpack_stats(st, K)
        new = centres.copy()
        filled = s0 > 0                      # an empty cluster keeps its centre
        new[filled] += s1[filled] / s0[filled, None]
        shift = float(np.sum((new - centres) ** 2))
        centres = new
        if shift <= tol:
            break
    return centres, dev.run(X, dev.kmeans_pack(centres), _lib.GMM_KMEANS, K)


# -- one GaussianMixture fit ------------------------------------------------------------------------------------------
def _options(gmmKwargs):
    opts = dict(_DEFAULTS)
    for key, val in (gmmKwargs or {}).items():
        if key not in _OPTIONS:
            raise NotImplementedError("fitGMM: GaussianMixture option %r is not supported on the device" % key)
        opts[key] = val
    if opts["init_params"] != "kmeans":
        raise NotImplementedError("fitGMM: init_params=%r is not supported on the device (only 'kmeans')"
                                  % (opts["init_params"],))
    if opts["covariance_type"] not in _COV_TYPES:
        raise ValueError("covariance_type must be one of %s, got %r" % (_COV_TYPES, opts["covariance_type"]))
    return opts


class _Fit(object):
    __slots__ = ("weights", "means", "cov", "pc", "converged", "n_iter", "lower_bound", "lower_bounds")


def _fit(dev, X, K, opts):
    """sklearn GaussianMixture.fit on the rows of device tensor X (n_init starts, the best lower bound kept)."""
    from sklearn.utils import check_random_state
    cov_type, reg, tol, max_iter = opts["covariance_type"], float(opts["reg_covar"]), opts["tol"], int(opts["max_iter"])
    n, D = int(X.shape[0]), dev.D
    if not 1 <= K <= _lib.GMM_MAX_COMP:
        raise ValueError("n_components must be in 1..%d, got %d" % (_lib.GMM_MAX_COMP, K))
    if n < max(2, K):
        raise ValueError("Expected n_samples >= n_components (and >= 2) but got n_components = %d, n_samples = %d"
                         % (K, n))
    if int(opts["n_init"]) < 1 or max_iter < 0 or tol < 0 or reg < 0:
        raise ValueError("n_init >= 1, max_iter >= 0, tol >= 0 and reg_covar >= 0 required")
    w_init, m_init, p_init = opts["weights_init"], opts["means_init"], opts["precisions_init"]
    if w_init is not None:
        w_init = np.asarray(w_init, dtype=np.float64).reshape(K)
    if m_init is not None:
        m_init = np.asarray(m_init, dtype=np.float64).reshape(K, D)
    if p_init is not None:
        shape = {"full": (K, D, D), "tied": (D, D), "diag": (K, D), "spherical": (K,)}[cov_type]
        p_init = np.asarray(p_init, dtype=np.float64).reshape(shape)
    rs = check_random_state(opts["random_state"])
    best = None
    for _ in range(int(opts["n_init"])):
        f = _Fit()
        f.cov = None
        if w_init is None or m_init is None or p_init is None:
            centres, st = _kmeans_labels_stats(dev, X, K, rs)
            nk, means, cov, pc = _m_step(dev, st, centres, K, cov_type, reg)
            f.weights = nk / n if w_init is None else w_init
            f.means = means if m_init is None else m_init
            f.cov, f.pc = cov, pc
        else:
            f.weights, f.means = w_init, m_init
        if p_init is not None:
            f.pc = _prec_chol_from_prec(p_init, cov_type)
        f.lower_bound, f.lower_bounds, f.converged, f.n_iter = -np.inf, [], False, 0
        for it in range(1, max_iter + 1):
            prev = f.lower_bound
            centres = f.means
            st = dev.run(X, dev.pack(f.weights, centres, _full_prec_chol(f.pc, cov_type, K, D)), _lib.GMM_EM, K)
            nk, f.means, f.cov, f.pc = _m_step(dev, st, centres, K, cov_type, reg)
            f.weights = nk / np.sum(nk)
            f.lower_bound = st[0] / n
            f.lower_bounds.append(f.lower_bound)
            f.n_iter = it
            if abs(f.lower_bound - prev) < tol:
                f.converged = True
                break
        if best is None or f.lower_bound > best.lower_bound:
            best = f
    return best


def _sklearn_version():
    import re
    import sklearn
    return tuple(int(v) for v in re.findall(r"\d+", sklearn.__version__)[:2])


def _estimator(fit, K, opts, D):
    """the fitted sklearn GaussianMixture carrying the device's parameters."""
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture
    gmm = GaussianMixture(**dict(opts, n_components=K))
    gmm.weights_ = np.asarray(fit.weights, dtype=np.float64)
    gmm.means_ = np.asarray(fit.means, dtype=np.float64)
    gmm.covariances_ = fit.cov
    gmm.precisions_cholesky_ = fit.pc
    gmm.precisions_ = _precisions(fit.pc, opts["covariance_type"])
    gmm.converged_ = bool(fit.converged)
    gmm.n_iter_ = int(fit.n_iter)
    gmm.lower_bound_ = float(fit.lower_bound)
    gmm.n_features_in_ = D
    if _sklearn_version() >= (1, 7):                             # GaussianMixture.fit sets lower_bounds_ from 1.7 on
        gmm.lower_bounds_ = list(fit.lower_bounds)
    if not fit.converged and int(opts["max_iter"]) > 0:
        warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase "
                      "max_iter, tol, or check for degenerate data.", ConvergenceWarning)
    return gmm


def _device_score(dev, X, fit, K, cov_type):
    """mean log-likelihood of the rows of X under a fit (the device's score pass)."""
    params = dev.pack(fit.weights, fit.means, _full_prec_chol(fit.pc, cov_type, K, dev.D))
    return float(dev.run(X, params, _lib.GMM_SCORE, K)[0]) / int(X.shape[0])


def _kfold_bounds(n, folds=5):
    """KFold(folds) without shuffling: contiguous folds, the first n % folds one row longer."""
    sizes = np.full(folds, n // folds)
    sizes[:n % folds] += 1
    ends = np.cumsum(sizes)
    return list(zip(ends - sizes, ends))


def fitGMM(samples, maxComp=3, covType="full", useBic=True, gmmKwargs=None):
    """
    Fit a Gaussian Mixture Model to the posterior samples to derive an
    approximation of the posterior density.  Fit for the number of components
    by either minimizing the Bayesian Information Criterior (BIC) or via
    cross-validation.

    Parameters
    ----------
    samples : numpy array or float64 CUDA tensor
        sampler.flatchain MCMC chain array of dimensions (nwalkers x nsteps, ndim).
        A CUDA tensor (contiguous) is used in place; an array is uploaded once.
    maxComp : int (optional)
        Maximum number of mixture model components to fit for.  Defaults to 3.
    covType : str (optional)
        GMM covariance type ("full", "tied", "diag", "spherical").  Defaults to "full".
    useBic : bool (optional)
        Minimize the BIC to pick the number of GMM components or use 5-fold
        cross validation?  Defaults to True (aka, use the BIC)
    gmmKwargs : dict (optional)
        keyword arguments for sklearn.mixture.GaussianMixture: n_components and
        covariance_type (both set by the selection, as in the reference), tol,
        reg_covar, max_iter, n_init, random_state, weights_init, means_init,
        precisions_init, init_params="kmeans".  Any other raises NotImplementedError.

    Returns
    -------
    GMM : sklearn.mixture.GaussianMixture
        fitted Gaussian mixture model (parameters computed on the device)

    Notes
    -----
    k-means initialisation: k-means++ seeding on the host on a uniform subsample
    of at most 2^16 rows drawn with ``random_state``, then Lloyd iterations over
    all rows on the device (sklearn's stopping rule; an empty cluster keeps its
    centre), then one M-step from the hard labels.
    ``useBic=False``: 5 contiguous folds (``KFold(5)``), n = 1..maxComp (the
    reference's grid also lists n = 0, which sklearn rejects), the best mean
    held-out score (ties: the smaller n), then ONE fit on all rows -- the
    reference fits that model a second time from a fresh initialisation, which
    only changes how many random draws are consumed.  Unlike the reference,
    whose cross-validation branch ignores ``gmmKwargs`` (GridSearchCV over a
    default GaussianMixture), every fit here -- the fold fits and the final one
    -- uses ``gmmKwargs`` (tol, reg_covar, n_init, random_state, ...) in both
    branches.
    """
    maxComp = int(maxComp)
    if not 1 <= maxComp <= _lib.GMM_MAX_COMP:
        raise ValueError("maxComp must be in 1..%d, got %d" % (_lib.GMM_MAX_COMP, maxComp))
    opts = _options(dict(gmmKwargs or {}, covariance_type=covType))
    dev = _Device(samples)
    torch = dev.torch
    with torch.cuda.device(dev.dev):
        X, n, D = dev.X, dev.n, dev.D
        if useBic:
            best_bic, best_n = np.inf, None
            for K in range(1, maxComp + 1):
                f = _fit(dev, X, K, opts)
                score = _device_score(dev, X, f, K, covType)
                bic = -2.0 * score * n + _n_parameters(K, D, covType) * np.log(n)
                if bic < best_bic:
                    best_bic, best_n = bic, K
            if best_n is None:
                raise ValueError("fitGMM: no finite BIC for n_components in 1..%d" % maxComp)
        else:
            if n < 5:
                raise ValueError("fitGMM: 5-fold cross-validation needs at least 5 samples, got %d" % n)
            totals = np.zeros(maxComp)
            for a, b in _kfold_bounds(n):
                train, test = torch.cat([X[:a], X[b:]]), X[a:b]
                for K in range(1, maxComp + 1):
                    f = _fit(dev, train, K, opts)
                    totals[K - 1] += _device_score(dev, test, f, K, covType)
                del train
            best_n = int(np.argmax(totals / 5.0)) + 1
        return _estimator(_fit(dev, X, best_n, opts), best_n, opts, D)


def _fit_fixed(samples, gmmKwargs=None):
    """One GaussianMixture fit with the given n_components (no selection): the device counterpart of
    ``GaussianMixture(**gmmKwargs).fit(samples)``."""
    opts = _options(gmmKwargs)
    dev = _Device(samples)
    with dev.torch.cuda.device(dev.dev):
        K = int(opts["n_components"])
        return _estimator(_fit(dev, dev.X, K, opts), K, opts, dev.D)


def _score_on_device(gmm, samples):
    """mean log-likelihood of ``samples`` under a fitted estimator, by the device's score pass."""
    dev = _Device(samples)
    with dev.torch.cuda.device(dev.dev):
        K = len(gmm.weights_)
        f = _Fit()
        f.weights, f.means, f.pc = gmm.weights_, gmm.means_, gmm.precisions_cholesky_
        return _device_score(dev, dev.X, f, K, gmm.covariance_type)
