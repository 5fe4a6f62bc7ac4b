# -*- coding: utf-8 -*-
"""CPU: the integrated acquisition without a GPU -- the entry point of the C ABI (exported, bound, sized, refusing bad
arguments with -1 and a message before any HIP call), and the refusals of GP.acquire_integrated and
findNextPoint(integrated=...) before any device work."""
import ctypes

import numpy as np
import pytest

from approxposterior_amd import _lib
from approxposterior_amd import gp as agp
from approxposterior_amd import utility as ut


def test_entry_points_are_exported_bound_and_sized():
    lib = _lib.load()
    for name in ("apgp_acquire_integrated", "apgp_integrated_work_len", "apgp_integrated_mode"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.apgp_abi_version() == 8 and _lib.MAX_REFS == 4096
    # one (value, index) partial per 256-candidate workgroup, whatever the number of reference points
    for m, nblk in ((1, 1), (256, 1), (257, 2), (10 ** 6, 3907), (1 << 40, 1 << 32)):
        assert lib.apgp_integrated_work_len(m, 1) == 2 * nblk == lib.apgp_integrated_work_len(m, _lib.MAX_REFS)
    assert lib.apgp_integrated_work_len(0, 5) == 0
    assert lib.apgp_integrated_work_len(-1, 5) == -1 and lib.apgp_integrated_work_len((1 << 40) + 1, 5) == -1
    assert lib.apgp_integrated_work_len(5, 0) == -1 and lib.apgp_integrated_work_len(5, _lib.MAX_REFS + 1) == -1


def test_mode_switch():
    lib = _lib.load()
    assert lib.apgp_integrated_mode(-1) == 0
    assert lib.apgp_integrated_mode(1) == 0 and lib.apgp_integrated_mode(-1) == 1
    assert lib.apgp_integrated_mode(2) == -1 and lib.apgp_integrated_mode(-1) == 1
    assert lib.apgp_integrated_mode(0) == 1 and lib.apgp_integrated_mode(-1) == 0


def _call(lib, **kw):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ks = _lib.KernelStruct()
    ks.ndim = kw.get("ndim", 2)
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    a = dict(T=p, m=4, off=0, xs=p, n=4, ks=ctypes.byref(ks), R=p, nref=3, B=p, a=p, var=p, lo=None, hi=None, mask=None,
             C=p, ldc=4, u=p, part=p, best=p)
    a.update(kw)
    return lib.apgp_acquire_integrated(a["T"], a["m"], a["off"], a["xs"], a["n"], a["ks"], a["R"], a["nref"], a["B"],
                                       a["a"], a["var"], a["lo"], a["hi"], a["mask"], a["C"], a["ldc"], a["u"],
                                       a["part"], a["best"], None)


_BOX = (ctypes.c_double * _lib.MAX_DIM)()


@pytest.mark.parametrize("bad, message", [
    (dict(T=None), b"null pointer"), (dict(xs=None), b"null pointer"), (dict(ks=None), b"null pointer"),
    (dict(R=None), b"null pointer"), (dict(B=None), b"null pointer"), (dict(a=None), b"null pointer"),
    (dict(var=None), b"null pointer"), (dict(part=None), b"null pointer"), (dict(best=None), b"null pointer"),
    (dict(nref=0), b"APGP_MAX_REFS"), (dict(nref=-1), b"APGP_MAX_REFS"), (dict(nref=_lib.MAX_REFS + 1), b"APGP_MAX_REFS"),
    (dict(m=0), b"APGP_MAX_M"), (dict(m=-4), b"APGP_MAX_M"), (dict(m=(1 << 40) + 1), b"APGP_MAX_M"),
    (dict(n=0), b"APGP_MAX_N"), (dict(n=(1 << 24) + 1), b"APGP_MAX_N"),
    (dict(ldc=3), b"ldc"),
    (dict(lo=_BOX), b"together"), (dict(hi=_BOX), b"together"),
    (dict(ndim=_lib.MAX_DIM + 1), b"kernel parameters"), (dict(ndim=0), b"kernel parameters"),
    (dict(ndim=_lib.INTEGRATED_MAX_DIM + 1), b"APGP_INTEGRATED_MAX_DIM"), (dict(ndim=_lib.MAX_DIM), b"APGP_INTEGRATED_MAX_DIM"),
])
def test_bad_arguments_are_refused_without_a_gpu(bad, message):
    lib = _lib.load()
    assert _call(lib, **bad) == -1
    err = lib.apgp_last_error()
    assert b"apgp_acquire_integrated" in err and message in err


class _Computed(agp.GP):
    """A GP that claims to be computed: the argument checks come before any device work, which would fail here."""
    computed = True


def _gp():
    return _Computed(kernel=agp.kernels.ExpSquaredKernel([1.0, 1.0], ndim=2))


@pytest.mark.parametrize("refs", [np.zeros((0, 2)), np.zeros((3, 3)), np.zeros(4), np.zeros((_lib.MAX_REFS + 1, 2)),
                                  np.array([[0.0, np.nan]]), np.array([[np.inf, 0.0]])])
def test_acquire_integrated_refuses_bad_reference_points(refs):
    gp = _gp()
    with pytest.raises(ValueError, match="refs"):
        gp.acquire_integrated(np.zeros(3), np.zeros((5, 2)), refs, logWeights=np.zeros(len(refs)))
    with pytest.raises(ValueError, match="refs"):
        gp.integration_weights(np.zeros(3), refs)


@pytest.mark.parametrize("w", [np.zeros(2), np.array([0.0, np.nan, 0.0]), np.array([0.0, np.inf, 0.0]),
                               np.full(3, -np.inf)])
def test_acquire_integrated_refuses_bad_log_weights(w):
    with pytest.raises(ValueError, match="logWeights"):
        _gp().acquire_integrated(np.zeros(3), np.zeros((5, 2)), np.zeros((3, 2)), logWeights=w)


def test_integration_weights_refuses_an_unknown_density():
    with pytest.raises(ValueError, match="density"):
        _gp().integration_weights(np.zeros(3), np.zeros((3, 2)), density="prior")


def test_acquire_integrated_refuses_more_than_16_dimensions():
    gp = _Computed(kernel=agp.kernels.ExpSquaredKernel(np.ones(17), ndim=17))
    with pytest.raises(NotImplementedError, match="16 dimensions"):
        gp.acquire_integrated(np.zeros(3), np.zeros((5, 17)), np.zeros((3, 17)), logWeights=np.zeros(3))


def test_acquire_integrated_needs_a_computed_gp():
    gp = agp.GP(kernel=agp.kernels.ExpSquaredKernel([1.0, 1.0], ndim=2))
    with pytest.raises(RuntimeError, match="compute"):
        gp.acquire_integrated(np.zeros(3), np.zeros((5, 2)), np.zeros((3, 2)), logWeights=np.zeros(3))


def test_eiv_utility_is_not_a_sweep_kind():
    assert "EIVUtility" in ut.__all__
    with pytest.raises(ValueError):
        ut.utilityKind(ut.EIVUtility)
    assert ut.EIVUtility(np.zeros(2), None, None, lambda t: -np.inf, None, None) == np.inf     # the prior gates first


class _NoDevice(object):
    """A stand-in GP: any method call would be device work."""

    def __getattr__(self, name):
        raise AssertionError("device work before the argument checks: GP.%s" % name)


def _ap():
    from approxposterior_amd import approx, likelihood as lh
    theta = np.array([[0.0, 1.0], [1.0, 2.0], [-1.0, 0.5]])
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    return approx.ApproxPosterior(theta=theta, y=y, gp=_NoDevice(), lnprior=lh.rosenbrockLnprior,
                                  lnlike=lh.rosenbrockLnlike, priorSample=lh.rosenbrockSample,
                                  bounds=[(-5, 5), (-5, 5)], algorithm="bape", distributed=False)


@pytest.mark.parametrize("kw", [dict(integrated=8), dict(integrated=0, nCandidates=100),
                                dict(integrated=_lib.MAX_REFS + 1, nCandidates=100), dict(integrated=True, nCandidates=100),
                                dict(integrated=8, nCandidates=100, batchSize=2),
                                dict(integrated=8, nCandidates=100, polish=True)])
def test_find_next_point_integrated_arguments_are_checked_first(kw, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    with pytest.raises(ValueError, match="integrated"):
        ap.findNextPoint(computeLnLike=True, numNewPoints=2, verbose=False, **kw)
    with pytest.raises(ValueError, match="integrated"):
        ap.run(m=2, nmax=1, verbose=False, cache=False, initGPOpt=False, **kw)
    assert len(ap.y) == 3


def test_find_next_point_integrated_under_a_process_group_is_not_implemented(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    monkeypatch.setattr(ap, "_ranks", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="process group"):
        ap.findNextPoint(computeLnLike=False, numNewPoints=2, nCandidates=100, integrated=8, verbose=False)
