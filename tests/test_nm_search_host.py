# -*- coding: utf-8 -*-
"""CPU: the host side of the device point search with the device call stubbed -- the restart / redraw logic of
``utility.minimizeObjective(onDevice=True)``, option validation, the kind mapping (findMAP's -mu included), the gate
ApproxPosterior hands over (``bounds`` or a JointPrior's support) and the C ABI entry points' argument checks."""
import ctypes

import numpy as np
import pytest

from approxposterior_amd import _lib, approx, gp as agp, likelihood as lh, priors, utility as ut


def bowl(x, *args):
    x = np.asarray(x, dtype=float).ravel()
    return float(np.sum((x - 0.25) ** 2))


bowl.searchKind = "agp"          # (what the stubbed device search is told to minimise)


class StubGP(object):
    """Stands in for GP.nelder_mead_search: records the starts of every call and returns ``answer(starts)``."""

    def __init__(self, answer=None):
        self.calls = []
        self.answer = answer or (lambda s: s + 0.0)

    def nelder_mead_search(self, y, starts, kind, bounds=None, zeta=0.01, options=None, trace=False):
        starts = np.array(starts, dtype=float)
        self.calls.append(dict(starts=starts, kind=kind, bounds=bounds, options=options))
        x = self.answer(starts)
        R = len(starts)
        return x, np.zeros(R), np.ones(R, dtype=np.int32), np.ones(R, dtype=np.int32), np.zeros(R, dtype=np.int32)


def box_prior(x):
    x = np.asarray(x, dtype=float).ravel()
    return 0.0 if np.all(np.abs(x) <= 5) else -np.inf


def sample(n):
    return np.random.uniform(-5, 5, size=(n, 2))


def test_device_restarts_consume_the_random_stream_as_the_host_path():
    drawn = []

    def rec_sample(n):
        s = sample(n)
        drawn.append(np.array(s).ravel())
        return s

    np.random.seed(3)
    host = ut.minimizeObjective(bowl, None, None, rec_sample, box_prior, nRestarts=5)
    host_state = np.random.get_state()[1].copy()
    host_starts = np.array(drawn)
    drawn.clear()
    stub = StubGP(lambda s: np.full_like(s, 0.25))
    np.random.seed(3)
    dev = ut.minimizeObjective(bowl, None, stub, rec_sample, box_prior, nRestarts=5, onDevice=True,
                               bounds=[(-5, 5)] * 2)
    assert np.array_equal(np.random.get_state()[1], host_state)
    assert len(stub.calls) == 1 and np.array_equal(stub.calls[0]["starts"], host_starts)
    assert stub.calls[0]["kind"] == "agp" and stub.calls[0]["bounds"] == [(-5, 5)] * 2
    assert stub.calls[0]["options"] == {"adaptive": True}
    assert np.allclose(dev[0], 0.25) and np.allclose(host[0], 0.25, atol=1e-3)


def test_theta0_restarts_are_perturbed_as_on_the_host():
    stub = StubGP()
    np.random.seed(9)
    theta0 = np.array([1.5, 2.0])
    ut.minimizeObjective(bowl, None, stub, sample, box_prior, nRestarts=3, theta0=theta0, onDevice=True)
    np.random.seed(9)
    # (the host path draws randn(theta0.ndim): one number shared by the coordinates, the reference's own quirk)
    want = np.array([theta0 + np.min(theta0) * 1.0e-3 * np.random.randn(1) for _ in range(3)])
    assert np.array_equal(stub.calls[0]["starts"], want)


def test_refused_restarts_are_redrawn_in_order_and_searched_together():
    # restarts 1 and 3 come back outside the prior on the first launch, restart 3 once more on the second
    seen = [0]

    def answer(s):
        seen[0] += 1
        out = np.full_like(s, 0.25)
        if seen[0] == 1:
            out[1] = 9.0
            out[3] = np.nan
        elif seen[0] == 2:
            out[1] = 7.0          # (the second of the two relaunched restarts: restart 3)
        return out

    stub = StubGP(answer)
    np.random.seed(5)
    ut.minimizeObjective(bowl, None, stub, sample, box_prior, nRestarts=4, onDevice=True)
    np.random.seed(5)
    first = np.array([sample(1).ravel() for _ in range(4)])
    r1, r3 = sample(1).ravel(), sample(1).ravel()
    r3b = sample(1).ravel()
    assert [len(c["starts"]) for c in stub.calls] == [4, 2, 1]
    assert np.array_equal(stub.calls[0]["starts"], first)
    assert np.array_equal(stub.calls[1]["starts"], np.array([r1, r3]))
    assert np.array_equal(stub.calls[2]["starts"], r3b.reshape(1, -1))


def test_the_error_comes_after_maxIters_redraws():
    stub = StubGP(lambda s: np.full_like(s, 50.0))
    np.random.seed(1)
    with pytest.raises(RuntimeError, match="Cannot find a valid solution"):
        ut.minimizeObjective(bowl, None, stub, sample, box_prior, nRestarts=2, onDevice=True, maxIters=3)
    assert len(stub.calls) == 3


def test_on_device_is_nelder_mead_only():
    with pytest.raises(ValueError):
        ut.minimizeObjective(bowl, None, StubGP(), sample, box_prior, method="powell", onDevice=True)


def test_search_kinds():
    assert ut.searchKind(ut.AGPUtility) == "agp"
    assert ut.searchKind(ut.BAPEUtility) == "bape"
    assert ut.searchKind(ut.JonesUtility) == "jones"
    f = lambda x: 0.0   # noqa: E731
    f.searchKind = "negmean"
    assert ut.searchKind(f) == "negmean"
    with pytest.raises(ValueError):
        ut.searchKind(sample)
    assert agp.SEARCH_KINDS["negmean"] == _lib.UTIL_NEG_MEAN == 4
    assert set(agp.SEARCH_KINDS) == {"agp", "bape", "jones", "negmean"}


def test_option_validation_comes_before_any_device_work():
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.ones(2), ndim=2))
    with pytest.raises(ValueError, match="initial_simplex"):
        g.nelder_mead_search(np.zeros(3), np.zeros((1, 2)), "agp", options={"initial_simplex": None})
    with pytest.raises(ValueError, match="disp"):
        g.nelder_mead_search(np.zeros(3), np.zeros((1, 2)), "bape", options={"adaptive": True, "disp": True})
    with pytest.raises(ValueError, match="kind"):
        g.nelder_mead_search(np.zeros(3), np.zeros((1, 2)), "ei")
    with pytest.raises(RuntimeError, match="compute"):       # valid options: next is the GP's own state
        g.nelder_mead_search(np.zeros(3), np.zeros((1, 2)), "agp",
                             options={"adaptive": True, "maxiter": 5, "maxfev": 9, "xatol": 1e-6, "fatol": 1e-6})


def test_coefficients_and_limits_are_scipys():
    for D in (1, 2, 5, 8):
        dim = float(D)
        assert agp.nm_coefficients(D, True) == (1.0, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim)
        assert agp.nm_limits(D) == (200 * D, 200 * D)
    assert agp.nm_coefficients(3, False) == (1.0, 2.0, 0.5, 0.5)
    assert agp.nm_limits(2, maxiter=10) == (10, 3 + 9 * 4)
    assert agp.nm_limits(2, maxfev=30) == (30, 30)


def _ap(lnprior, bounds):
    theta = np.random.RandomState(0).uniform(-2, 2, size=(12, 2))
    y = -np.sum(theta ** 2, axis=1)
    return approx.ApproxPosterior(theta=theta, y=y, gp=object(), lnprior=lnprior, lnlike=lh.sphereLnlike,
                                  priorSample=sample, bounds=bounds, algorithm="bape")


def _capture(monkeypatch):
    seen = []

    def fake(fn, y, gp, sampleFn, priorFn, **kw):
        seen.append(dict(kw, fn=fn))
        return np.zeros(2), np.array([0.0])

    monkeypatch.setattr(approx.ut, "minimizeObjective", fake)
    return seen


def test_gate_is_the_bounds_or_the_joint_support(monkeypatch):
    seen = _capture(monkeypatch)
    ap = _ap(box_prior, ((-5, 5), (-4, 4)))
    ap.findNextPoint(computeLnLike=False, deviceSearch=True, verbose=False, cache=False)
    assert ap.deviceSearch is True
    assert seen[-1]["onDevice"] is True and tuple(map(tuple, seen[-1]["bounds"])) == ((-5, 5), (-4, 4))
    ap.findNextPoint(computeLnLike=False, verbose=False, cache=False)          # the attribute stays on
    assert seen[-1]["onDevice"] is True
    ap.findNextPoint(computeLnLike=False, deviceSearch=False, verbose=False, cache=False)
    assert seen[-1]["onDevice"] is False
    jp = priors.JointPrior([priors.UniformPrior(-3.0, 3.0), priors.GaussianPrior(0.5, 2.0)])
    ap = _ap(jp, ((-3, 3), (-9.5, 10.5)))
    ap.findNextPoint(computeLnLike=False, deviceSearch=True, verbose=False, cache=False)
    gate = [tuple(r) for r in seen[-1]["bounds"]]
    assert gate == [(-3.0, 3.0), (-np.inf, np.inf)]
    ap.findMAP(deviceSearch=True)
    assert seen[-1]["onDevice"] is True and [tuple(r) for r in seen[-1]["bounds"]] == gate
    assert ut.searchKind(seen[-1]["fn"]) == "negmean"
    ap2 = _ap(box_prior, ((-5, 5), (-4, 4)))
    ap2.findMAP()
    assert seen[-1]["onDevice"] is False


def test_polish_after_a_sweep_uses_the_device_search(monkeypatch):
    seen = _capture(monkeypatch)
    ap = _ap(box_prior, ((-5, 5), (-5, 5)))
    monkeypatch.setattr(approx.ut, "sweepObjective", lambda *a, **k: (np.zeros(2), 0.0))
    ap.findNextPoint(computeLnLike=False, nCandidates=16, polish=True, deviceSearch=True, verbose=False, cache=False)
    assert len(seen) == 1 and seen[0]["onDevice"] is True and seen[0]["nRestarts"] == 1


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.apgp_nm_search_work_len(5, 100) == 5 * 128
    assert lib.apgp_nm_search_work_len(0, 100) == -1
    assert lib.apgp_nm_search_work_len(_lib.NM_MAX_RESTARTS + 1, 100) == -1
    buf = (ctypes.c_double * 256)()
    p = ctypes.addressof(buf)
    ks = _lib.KernelStruct()
    ks.ndim = 2
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0

    def call(R=2, n=4, winv=p, ldw=64, L=None, ldl=0, starts=p, work=p, **o):
        opt = _lib.NmOptions(kind=_lib.UTIL_AGP, maxiter=10, maxfev=10, xatol=1e-4, fatol=1e-4, rho=1.0, chi=2.0,
                             psi=0.5, sigma=0.5)
        for k, v in o.items():
            setattr(opt, k, v)
        return lib.apgp_nm_search(starts, R, p, n, ctypes.byref(ks), 0.0, winv, ldw, L, ldl, None, None,
                                  ctypes.byref(opt), p, p, p, None, None, work, None)

    assert call(starts=None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert call(work=None) == -1
    assert call(R=0) == -1 and call(R=_lib.NM_MAX_RESTARTS + 1) == -1
    assert call(winv=None) == -1                           # neither form
    assert call(ldw=3) == -1 and call(ldw=65) == -1        # ldw < n / odd
    assert call(kind=_lib.UTIL_NONE) == -1 and b"kind" in lib.apgp_last_error()
    assert call(maxfev=0) == -1 and call(maxiter=_lib.NM_MAX_FEV + 1) == -1
    ks.ndim = _lib.MAX_DIM + 1
    assert call() == -1 and b"kernel parameters" in lib.apgp_last_error()
    ks.ndim = 2
