"""GPU: the Gaussian-mixture passes (csrc/gmm.hip) against tests/gmm_ref.py, full EM against sklearn's host fit from
the same initial parameters, the reference's known-answer test through approxposterior_amd.fitGMM, and component
selection by BIC and by cross-validation."""
import ctypes
import warnings

import numpy as np
import pytest

import gmm_ref
from approxposterior_amd import _lib, gmmUtils

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _offset_data(rs, n, D, K, offset_sigma=1e3):
    """K clusters of unit-ish scale whose means sit 1e3 sigma from the origin (exercises the centring)."""
    base = rs.normal(size=D) * offset_sigma
    centres = base + rs.normal(scale=3.0, size=(K, D))
    lab = rs.randint(0, K, size=n)
    return centres[lab] + rs.normal(size=(n, D)), centres


def _params(rs, X, K, centres):
    D = X.shape[1]
    w = rs.dirichlet(np.ones(K) * 3)
    A = rs.normal(size=(K, D, D)) * (0.3 / np.sqrt(D))
    U = np.triu(A) + np.eye(D) * rs.uniform(0.6, 1.2, size=(K, 1, D))
    c = centres[rs.randint(0, len(centres), size=K)] + rs.normal(scale=0.5, size=(K, D))
    return w, c, U


def _abs_stats(X, w, centres):
    """sum |w| |a| |b| of every statistic (the scale its rounding error is measured against)"""
    rec = []
    for k in range(w.shape[1]):
        rec.append(gmm_ref.centred_stats(np.abs(X - centres[k]), np.abs(w[:, k:k + 1]), np.zeros((1, X.shape[1]))))
    return np.concatenate(rec)


def _run(X_d, D, K, params, mode, rows=True):
    torch = _torch()
    lib = _lib.load()
    n = X_d.shape[0]
    p_d = torch.from_numpy(np.ascontiguousarray(params).ravel()).cuda()
    s_d = torch.full((lib.apgp_gmm_stats_len(D, K),), np.nan, dtype=torch.float64, device="cuda")
    lp_d = torch.empty(n, dtype=torch.float64, device="cuda") if rows else None
    lab_d = torch.empty(n, dtype=torch.int32, device="cuda") if rows else None
    st = lib.apgp_gmm_pass(ctypes.c_void_p(X_d.data_ptr()), n, D, K, ctypes.c_void_p(p_d.data_ptr()), mode,
                           ctypes.c_void_p(s_d.data_ptr()), ctypes.c_void_p(lp_d.data_ptr() if rows else None),
                           ctypes.c_void_p(lab_d.data_ptr() if rows else None),
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "apgp_gmm_pass")
    torch.cuda.synchronize()
    out = s_d.cpu().numpy()
    return out, (lp_d.cpu().numpy() if rows else None), (lab_d.cpu().numpy() if rows else None)


def _labels_agree(lab, ref_lab, lp_all):
    """labels equal wherever the best two components are not within rounding of each other"""
    srt = np.sort(lp_all, axis=1)
    clear = (srt[:, -1] - srt[:, -2] > 1e-9 * np.abs(srt[:, -1]) + 1e-12) if lp_all.shape[1] > 1 else np.ones(len(lab), bool)
    return np.array_equal(lab[clear], ref_lab[clear])


CASES = [(1, 1, 1), (1, 2, 255), (2, 2, 255), (3, 5, 257), (2, 16, 100003), (8, 2, 257), (8, 16, 255), (8, 5, 100003),
         (8, 3, 1280000), (17, 5, 257), (17, 2, 100003), (32, 16, 257), (32, 1, 100003), (32, 5, 1)]


@pytest.mark.parametrize("D,K,n", CASES)
def test_em_pass_against_reference(D, K, n):
    torch = _torch()
    rs = np.random.RandomState(1000 * D + 10 * K + n % 7)
    X, centres = _offset_data(rs, n, D, max(K, 2))
    w, c, U = _params(rs, X, K, centres)
    dev = gmmUtils._Device(X)
    params = dev.pack(w, c, U)
    X_d = torch.from_numpy(X).cuda()
    st, lp, lab = _run(X_d, D, K, params, _lib.GMM_EM)
    ref, rlp, rlab = gmm_ref.em_pass(X, w, c, U)
    np.testing.assert_allclose(lp, rlp, rtol=1e-11)
    assert _labels_agree(lab, rlab, gmm_ref.weighted_log_prob(X, w, c, U))
    _, _, r = gmm_ref.e_step(X, w, c, U)
    scale = np.concatenate([[np.sum(np.abs(rlp))], _abs_stats(X, r, c)])
    assert np.all(np.abs(st - ref) <= 1e-12 * scale + 1e-300), np.max(np.abs(st - ref) / (scale + 1e-300))
    # bit-identical on a second call
    st2, lp2, lab2 = _run(X_d, D, K, params, _lib.GMM_EM)
    assert st.tobytes() == st2.tobytes() and lp.tobytes() == lp2.tobytes() and lab.tobytes() == lab2.tobytes()
    # the score pass: G only, the same per-row values
    sc, slp, slab = _run(X_d, D, K, params, _lib.GMM_SCORE)
    assert abs(sc[0] - ref[0]) <= 1e-12 * scale[0] and np.all(np.isnan(sc[1:]))
    np.testing.assert_allclose(slp, lp, rtol=1e-14)
    assert np.array_equal(slab, lab)


@pytest.mark.parametrize("D,K,n", [(1, 2, 255), (3, 5, 257), (8, 3, 100003), (17, 16, 257), (32, 5, 1000)])
def test_kmeans_pass_against_reference(D, K, n):
    torch = _torch()
    rs = np.random.RandomState(7 + D + K)
    X, centres = _offset_data(rs, n, D, K)
    c = centres + rs.normal(scale=0.5, size=centres.shape)
    dev = gmmUtils._Device(X)
    X_d = torch.from_numpy(X).cuda()
    st, d2, lab = _run(X_d, D, K, dev.kmeans_pack(c), _lib.GMM_KMEANS)
    ref, rd2, rlab = gmm_ref.kmeans_pass(X, c)
    np.testing.assert_allclose(d2, rd2, rtol=1e-11)
    assert _labels_agree(lab, rlab, -np.stack([np.sum((X - ck) ** 2, axis=1) for ck in c], axis=1))
    onehot = np.zeros((n, K))
    onehot[np.arange(n), rlab] = 1.0
    scale = np.concatenate([[np.sum(rd2)], _abs_stats(X, onehot, c)])
    assert np.all(np.abs(st - ref) <= 1e-12 * scale + 1e-300)


def _init_for(rs, X, K, cov_type):
    D = X.shape[1]
    w = rs.dirichlet(np.ones(K) * 5)
    mu = X[rs.choice(len(X), K, replace=False)]
    A = rs.normal(size=(K, D, D)) * 0.2
    prec = np.einsum("kij,klj->kil", A, A) + np.eye(D) * 0.5
    return w, mu, {"full": prec, "tied": prec[0], "diag": np.diagonal(prec, axis1=1, axis2=2).copy(),
                   "spherical": np.diagonal(prec, axis1=1, axis2=2).mean(axis=1)}[cov_type]


@pytest.mark.parametrize("cov_type", ["full", "tied", "diag", "spherical"])
def test_full_em_matches_sklearn_from_explicit_inits(cov_type):
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture
    rs = np.random.RandomState(11)
    centres = rs.normal(scale=5.0, size=(3, 4))
    lab = rs.randint(0, 3, size=20000)
    X = centres[lab] + rs.normal(size=(20000, 4)) * rs.uniform(0.5, 2.0, size=(3, 4))[lab]
    w, mu, prec = _init_for(rs, X, 3, cov_type)
    kw = dict(n_components=3, covariance_type=cov_type, tol=0.0, max_iter=25, weights_init=w, means_init=mu,
              precisions_init=prec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        sk = GaussianMixture(**kw).fit(X)
        g = gmmUtils._fit_fixed(X, kw)
    assert g.n_iter_ == sk.n_iter_ == 25
    for name in ("weights_", "means_", "covariances_", "lower_bound_"):
        np.testing.assert_allclose(getattr(g, name), getattr(sk, name), rtol=1e-9, err_msg=name)
    np.testing.assert_allclose(g.precisions_cholesky_, sk.precisions_cholesky_, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(g.precisions_, sk.precisions_, rtol=1e-8, atol=1e-12)
    if hasattr(sk, "lower_bounds_"):
        np.testing.assert_allclose(g.lower_bounds_, sk.lower_bounds_, rtol=1e-9)


def test_reference_known_answer():
    """approxposterior/tests/test_GMM.py of the reference, through approxposterior_amd.fitGMM."""
    import approxposterior_amd
    np.random.seed(57)
    shiftG = np.random.randn(500, 2) + np.array([5, 10])
    muShiftG = np.mean(shiftG, axis=0)
    c = np.array([[0., -0.7], [3.5, .7]])
    stretchG = np.dot(np.random.randn(300, 2), c)
    muStetchG = np.mean(stretchG, axis=0)
    data = np.vstack([shiftG, stretchG])
    np.random.shuffle(data)
    gmm = approxposterior_amd.fitGMM(data, maxComp=10, covType="full")
    assert gmm.n_components == 2
    assert np.allclose(muStetchG, gmm.means_[0]) or np.allclose(muStetchG, gmm.means_[1])
    assert np.allclose(muShiftG, gmm.means_[0]) or np.allclose(muShiftG, gmm.means_[1])


def _three_clusters(n=30000, D=8, seed=21):
    rs = np.random.RandomState(seed)
    centres = rs.normal(scale=6.0, size=(3, D)) + 50.0
    lab = rs.randint(0, 3, size=n)
    return centres[lab] + rs.normal(size=(n, D)) * rs.uniform(0.5, 1.5, size=(3, D))[lab]


def test_selection_bic_and_cross_validation():
    torch = _torch()
    X = _three_clusters()
    g = gmmUtils.fitGMM(X, maxComp=5, gmmKwargs={"random_state": 0})
    assert g.n_components == 3 and g.converged_
    dev_score = gmmUtils._score_on_device(g, X)
    np.testing.assert_allclose(g.score(X), dev_score, rtol=1e-10)
    k = g.n_components
    n_par = k * 8 * 9 / 2 + k * 8 + k - 1
    np.testing.assert_allclose(g.bic(X), -2 * dev_score * len(X) + n_par * np.log(len(X)), rtol=1e-10)
    assert g.predict(X[:100]).shape == (100,)
    assert g.sample(10)[0].shape == (10, 8)
    gt = gmmUtils.fitGMM(torch.from_numpy(X).cuda(), maxComp=5, gmmKwargs={"random_state": 0})
    for name in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
        assert np.array_equal(getattr(g, name), getattr(gt, name)), name
    assert gt.n_iter_ == g.n_iter_ and gt.lower_bound_ == g.lower_bound_
    gcv = gmmUtils.fitGMM(X, maxComp=5, useBic=False, gmmKwargs={"random_state": 0})
    assert gcv.n_components == 3


@pytest.mark.parametrize("cov_type", ["tied", "diag", "spherical"])
def test_selection_other_covariance_types(cov_type):
    X = _three_clusters(n=20000, D=4, seed=5)
    g = gmmUtils.fitGMM(X, maxComp=4, covType=cov_type, gmmKwargs={"random_state": 1, "n_init": 2})
    assert 1 <= g.n_components <= 4 and g.covariance_type == cov_type
    np.testing.assert_allclose(g.score(X), gmmUtils._score_on_device(g, X), rtol=1e-10)


def test_unsupported_and_limits_raise():
    torch = _torch()
    X = _three_clusters(n=1000, D=3)
    with pytest.raises(NotImplementedError, match="warm_start"):
        gmmUtils.fitGMM(X, gmmKwargs={"warm_start": True})
    with pytest.raises(ValueError):
        gmmUtils.fitGMM(np.zeros((100, 33)))
    with pytest.raises(ValueError):
        gmmUtils.fitGMM(torch.from_numpy(X).cuda().t())                    # not contiguous
    with pytest.raises(ValueError):
        gmmUtils.fitGMM(torch.from_numpy(X).cuda().float())                 # not float64
    with pytest.raises(ValueError):
        gmmUtils._fit_fixed(X, {"n_components": 17})
    with pytest.raises(ValueError, match="ill-defined"):
        gmmUtils._fit_fixed(np.ones((50, 2)), {"n_components": 2, "reg_covar": 0.0})
