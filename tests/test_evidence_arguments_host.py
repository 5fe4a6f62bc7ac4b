# -*- coding: utf-8 -*-
"""CPU: the evidence entry points refuse bad arguments with -1 before any HIP call (there is no GPU here), and their
size functions agree with include/apgp.h -- in the style of tests/test_cabi_symbols.py."""
import ctypes

import numpy as np
import pytest

from approxposterior_amd import _lib
from approxposterior_amd import gp as agp
from approxposterior_amd import utility as ut


def _params(D, K):
    """A valid host record: equal weights, unit factors."""
    tri = D * (D + 1) // 2
    rec = np.zeros((K, 3 + D + 2 * tri))
    eye_u = np.array([1.0 if i == j else 0.0 for j in range(D) for i in range(j + 1)])
    eye_l = np.array([1.0 if i == j else 0.0 for i in range(D) for j in range(i + 1)])
    for k in range(K):
        rec[k, 0] = 1.0 if k == K - 1 else (k + 1.0) / K
        rec[k, 1] = -np.log(K)
        rec[k, 3 + D:3 + D + tri] = eye_u
        rec[k, 3 + D + tri:] = eye_l
    return rec


def test_sizes():
    lib = _lib.load()
    assert lib.apgp_mix_params_len(3, 2) == 2 * (3 + 3 + 12) and lib.apgp_mix_params_len(1, 1) == 6
    assert lib.apgp_mix_params_len(0, 1) == -1 and lib.apgp_mix_params_len(3, 17) == -1
    assert lib.apgp_mix_params_len(_lib.MAX_DIM + 1, 1) == -1 and lib.apgp_mix_params_len(3, 0) == -1
    assert lib.apgp_importance_stats_len(1) == 6 and lib.apgp_importance_stats_len(8) == 4 + 8 + 36
    assert lib.apgp_importance_stats_len(0) == -1 and lib.apgp_importance_stats_len(_lib.MAX_DIM + 1) == -1
    per = 1 + 3 + _lib.MAX_DIM + _lib.MAX_DIM * (_lib.MAX_DIM + 1) // 2
    assert lib.apgp_importance_work_len(1) == per + 1 and lib.apgp_importance_work_len(257) == 2 * per + 257
    big = _lib.IMP_BLOCK * _lib.IMP_MAX_BLOCKS
    assert lib.apgp_importance_work_len(big + 1) == _lib.IMP_MAX_BLOCKS * per + big + 1
    assert lib.apgp_importance_work_len(0) == 0 and lib.apgp_importance_work_len((1 << 40) + 1) == -1


def test_mix_candidates_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    T = ctypes.addressof(buf)
    good = _params(2, 2)
    call = lambda rec, m=4, D=2, K=2, off=0, t=T: lib.apgp_mix_candidates(  # noqa: E731
        t, None, m, D, K, rec.ctypes.data if rec is not None else None, 1, off, None)
    assert call(good, m=0) == 0                              # nothing to draw: no launch
    assert call(good, t=None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert call(None) == -1
    assert call(good, m=-1) == -1 and call(good, off=-1) == -1
    assert call(good, D=0) == -1 and call(_params(2, 2), D=_lib.MAX_DIM + 1) == -1
    assert call(good, K=0) == -1 and call(good, K=17) == -1
    for edit in (lambda r: r.__setitem__((1, 0), 0.999),        # the last cumulative weight is not 1.0
                 lambda r: r.__setitem__((0, 0), 1.5),
                 lambda r: r.__setitem__((1, 0), 0.25),          # falls (0.5, then 0.25)
                 lambda r: r.__setitem__((0, 0), np.nan),
                 lambda r: r.__setitem__((0, 1), 0.5),           # log weight > 0
                 lambda r: r.__setitem__((0, 2), np.inf),        # log-determinant
                 lambda r: r.__setitem__((0, 3), np.nan),        # centre
                 lambda r: r.__setitem__((0, 5), np.inf),        # U
                 lambda r: r.__setitem__((1, 8), 0.0),           # A[0][0] = 0
                 lambda r: r.__setitem__((1, 10), -1.0)):        # A[1][1] < 0
        bad = good.copy()
        edit(bad)
        assert call(bad) == -1, bad
        assert b"apgp_mix_candidates" in lib.apgp_last_error()
    assert call(good, m=0) == 0


def test_importance_pass_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    ks = _lib.KernelStruct()
    ks.ndim, ks.amp = 2, 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    arr = ctypes.c_double * _lib.MAX_DIM
    lo, hi, c = arr(), arr(*([1.0] * _lib.MAX_DIM)), arr()
    ok = dict(T=p, m=4, lnq=None, xs=p, n=4, ks=ctypes.byref(ks), lo=lo, hi=hi, c=ctypes.addressof(c), stats=p, work=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.apgp_importance_pass(a["T"], a["m"], a["lnq"], a["xs"], a["n"], a["ks"], 0.0, a["lo"], a["hi"], a["c"],
                                        None, a["stats"], a["work"], None)
    for name in ("T", "xs", "c", "stats", "work"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.apgp_last_error()
    assert call(ks=None) == -1
    assert call(m=0) == -1 and call(m=(1 << 40) + 1) == -1
    assert call(n=0) == -1 and call(n=(1 << 24) + 1) == -1
    assert call(lo=None) == -1 and call(hi=None) == -1
    nanc = arr(*([float("nan")] * _lib.MAX_DIM))
    assert call(c=ctypes.addressof(nanc)) == -1
    ks.ndim = _lib.MAX_DIM + 1
    assert call() == -1
    ks.ndim, ks.amp = 2, 0.0
    assert call() == -1


def test_mixture_params_of_the_python_layer():
    K, D, rec = agp.GP._mixture_params([1.0, 3.0], [[0.0, 1.0], [2.0, 3.0]], [np.eye(2), [[2.0, 0.6], [0.6, 1.0]]], 4.0)
    assert (K, D) == (2, 2) and rec.shape == (2, 3 + 2 + 6)
    assert rec[0, 0] == 0.25 and rec[1, 0] == 1.0 and np.allclose(rec[:, 1], np.log([0.25, 0.75]))
    A = np.linalg.cholesky(4.0 * np.array([[2.0, 0.6], [0.6, 1.0]]))
    assert np.allclose(rec[1, 8:], [A[0, 0], A[1, 0], A[1, 1]])
    U = np.linalg.inv(A).T
    assert np.allclose(rec[1, 5:8], [U[0, 0], U[0, 1], U[1, 1]]) and np.isclose(rec[1, 2], np.log(U[0, 0] * U[1, 1]))
    assert np.allclose(rec[1, 3:5], [2.0, 3.0])
    with pytest.raises(ValueError):
        agp.GP._mixture_params([1.0], [[0.0, 0.0]], [[[1.0, 2.0], [2.0, 1.0]]], 1.0)        # not positive definite
    with pytest.raises(ValueError):
        agp.GP._mixture_params([1.0, 1.0], [[0.0, 0.0]], [np.eye(2)], 1.0)
    with pytest.raises(ValueError):
        agp.GP._mixture_params(np.ones(17), np.zeros((17, 1)), np.ones((17, 1, 1)), 1.0)
    with pytest.raises(ValueError):
        agp.GP._mixture_params([-1.0, 2.0], np.zeros((2, 1)), np.ones((2, 1, 1)), 1.0)
    # the host record passes the library's own checks
    lib = _lib.load()
    flat = np.ascontiguousarray(rec.ravel())
    buf = (ctypes.c_double * 8)()
    assert lib.apgp_mix_candidates(ctypes.addressof(buf), None, 0, 2, 2, flat.ctypes.data, 1, 0, None) == 0


def test_public_names():
    import approxposterior_amd as ap
    assert ap.mergeImportance is ut.mergeImportance and ap.importanceSummary is ut.importanceSummary
    assert ap.evidence is ap.ApproxPosterior.evidence
