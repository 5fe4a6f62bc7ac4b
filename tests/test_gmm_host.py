"""CPU: the Gaussian-mixture C ABI (apgp_gmm_*) is declared, exported and bound, refuses bad arguments before any HIP
call; tests/gmm_ref.py (the checker of the GPU tests) agrees with sklearn's GaussianMixture; fitGMM's host logic
(options, limits, folds, the centred M-step) without a GPU."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from approxposterior_amd import _lib, gmmUtils

import gmm_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_gmm_symbols_declared_exported_bound():
    header = open(os.path.join(ROOT, "include", "apgp.h")).read()
    lib = _lib.load()
    for name in ("apgp_gmm_pass", "apgp_gmm_params_len", "apgp_gmm_stats_len"):
        assert name + "(" in header
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.apgp_abi_version() == 8
    assert lib.apgp_gmm_params_len(8, 3) == 3 * (2 + 8 + 36)
    assert lib.apgp_gmm_stats_len(8, 3) == 1 + 3 * (1 + 8 + 36)
    assert lib.apgp_gmm_params_len(32, 16) == 16 * (2 + 32 + 528)
    for d, k in ((0, 1), (33, 1), (1, 0), (1, 17)):
        assert lib.apgp_gmm_params_len(d, k) == -1 and lib.apgp_gmm_stats_len(d, k) == -1


def test_gmm_pass_bad_arguments_refused_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(X=p, n=4, ndim=2, ncomp=1, params=p, mode=_lib.GMM_EM, stats=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.apgp_gmm_pass(a["X"], a["n"], a["ndim"], a["ncomp"], a["params"], a["mode"], a["stats"],
                                 None, None, None)

    for bad in (dict(X=None), dict(params=None), dict(stats=None)):
        assert call(**bad) == -1
        assert b"null pointer" in lib.apgp_last_error()
    for bad in (dict(ndim=0), dict(ndim=33), dict(ncomp=0), dict(ncomp=17), dict(n=0), dict(n=-3),
                dict(n=2 ** 31), dict(mode=3), dict(mode=-1)):
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.apgp_last_error()


def _clusters(rs, n, D, K, offset=0.0):
    centres = rs.normal(scale=4.0, size=(K, D)) + offset
    lab = rs.randint(0, K, size=n)
    return centres[lab] + rs.normal(size=(n, D)) * rs.uniform(0.5, 1.5, size=(K, D))[lab]


def _inits(rs, X, K, cov_type):
    D = X.shape[1]
    w = rs.dirichlet(np.ones(K) * 5)
    mu = X[rs.choice(len(X), K, replace=False)]
    A = rs.normal(size=(K, D, D)) * 0.2
    prec = np.einsum("kij,klj->kil", A, A) + np.eye(D)
    prec = {"full": prec, "tied": prec[0], "diag": np.diagonal(prec, axis1=1, axis2=2).copy(),
            "spherical": np.diagonal(prec, axis1=1, axis2=2).mean(axis=1)}[cov_type]
    return w, mu, prec


@pytest.mark.parametrize("cov_type", ["full", "tied", "diag", "spherical"])
def test_gmm_ref_matches_sklearn_two_iterations(cov_type):
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture
    rs = np.random.RandomState(3)
    X = _clusters(rs, 3000, 4, 3)
    w, mu, prec = _inits(rs, X, 3, cov_type)
    sk = GaussianMixture(3, covariance_type=cov_type, tol=0.0, max_iter=2, weights_init=w, means_init=mu,
                         precisions_init=prec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        sk.fit(X)
    rw, rmu, rcov, rpc, lb, it = gmm_ref.em_fit(X, w, mu, prec, cov_type, max_iter=2, tol=0.0)
    assert it == sk.n_iter_ == 2
    np.testing.assert_allclose(rw, sk.weights_, rtol=1e-12)
    np.testing.assert_allclose(rmu, sk.means_, rtol=1e-12)
    np.testing.assert_allclose(rcov, sk.covariances_, rtol=1e-12)
    np.testing.assert_allclose(rpc, sk.precisions_cholesky_, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(lb, sk.lower_bound_, rtol=1e-12)
    U = gmm_ref.full_prec_chol(sk.precisions_cholesky_, cov_type, 3, 4)
    lpn, lab, _ = gmm_ref.e_step(X, sk.weights_, sk.means_, U)
    np.testing.assert_allclose(lpn, sk.score_samples(X), rtol=1e-12)
    assert np.array_equal(lab, sk.predict(X))


def _host_device(D):
    dev = gmmUtils._Device.__new__(gmmUtils._Device)
    dev.D, dev.tri = D, gmmUtils._triu_colmajor(D)
    return dev


@pytest.mark.parametrize("cov_type", ["full", "tied", "diag", "spherical"])
def test_centred_m_step_matches_reference(cov_type):
    """The host M-step from statistics about the E-step's centres (mu = c + delta, Sigma = S / nk - delta delta^T)
    equals the direct formulas, also with means 1e3 sigma from the origin."""
    rs = np.random.RandomState(5)
    X = _clusters(rs, 4000, 3, 2, offset=3e3)
    r = rs.dirichlet(np.ones(2), size=len(X))
    centres = X[:2] + rs.normal(size=(2, 3))
    st = np.concatenate([[0.0], gmm_ref.centred_stats(X, r, centres)])
    nk, means, cov, pc = gmmUtils._m_step(_host_device(3), st, centres, 2, cov_type, 1e-6)
    w, rmu, rcov, rpc = gmm_ref.m_step(X, r, cov_type, 1e-6)
    np.testing.assert_allclose(nk / nk.sum(), w, rtol=1e-12)
    np.testing.assert_allclose(means, rmu, rtol=1e-12)
    np.testing.assert_allclose(cov, rcov, rtol=1e-9)
    np.testing.assert_allclose(pc, rpc, rtol=1e-9, atol=1e-12)


def test_packed_params_and_precisions_init():
    rs = np.random.RandomState(7)
    dev = _host_device(3)
    A = rs.normal(size=(2, 3, 3))
    prec = np.einsum("kij,klj->kil", A, A) + np.eye(3)
    U = gmmUtils._prec_chol_from_prec(prec, "full")
    assert np.allclose(np.tril(U, -1), 0.0)
    np.testing.assert_allclose(np.einsum("kij,klj->kil", U, U), prec, rtol=1e-12)
    np.testing.assert_allclose(U, gmm_ref.prec_chol_from_precisions(prec, "full"), rtol=1e-12)
    P = dev.pack(np.array([0.25, 0.75]), np.arange(6.0).reshape(2, 3), U)
    assert P.shape == (2, _lib.load().apgp_gmm_params_len(3, 2) // 2)
    np.testing.assert_allclose(P[:, 0], np.log([0.25, 0.75]))
    np.testing.assert_allclose(P[:, 1], np.log(np.diagonal(U, axis1=1, axis2=2)).sum(axis=1))
    # column-major upper packing: U[i][j] at j(j+1)/2 + i
    assert P[1, 5 + 3 * 2 // 2 + 1] == U[1, 1, 2]


def test_ill_defined_covariance_raises_value_error():
    with pytest.raises(ValueError, match="ill-defined"):
        gmmUtils._prec_chol_from_cov(np.array([[[1.0, 2.0], [2.0, 1.0]]]), "full")
    with pytest.raises(ValueError, match="ill-defined"):
        gmmUtils._prec_chol_from_cov(np.array([[1.0, 0.0]]), "diag")


def test_options_and_limits_raise_before_any_device_work():
    X = np.zeros((10, 2))
    with pytest.raises(NotImplementedError, match="warm_start"):
        gmmUtils.fitGMM(X, gmmKwargs={"warm_start": True})
    with pytest.raises(NotImplementedError, match="init_params"):
        gmmUtils.fitGMM(X, gmmKwargs={"init_params": "random"})
    with pytest.raises(ValueError, match="maxComp"):
        gmmUtils.fitGMM(X, maxComp=17)
    with pytest.raises(ValueError, match="covariance_type"):
        gmmUtils.fitGMM(X, covType="banded")


def test_kfold_bounds_are_sklearns():
    from sklearn.model_selection import KFold
    for n in (5, 6, 9, 1003):
        want = [(int(t[0]), int(t[-1]) + 1) for _, t in KFold(5).split(np.zeros((n, 1)))]
        assert [(int(a), int(b)) for a, b in gmmUtils._kfold_bounds(n)] == want


def test_import_does_not_need_sklearn():
    code = ("import sys; sys.modules['sklearn'] = None; import approxposterior_amd as a; "
            "assert callable(a.fitGMM); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr
