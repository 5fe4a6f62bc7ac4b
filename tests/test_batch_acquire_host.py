"""CPU: batch design-point selection without a GPU -- the fantasy entry point of the C ABI (exported, bound, refusing bad
arguments before any HIP call), the NumPy restatement of the recursion (tests/fantasy_ref.py) against naive
re-conditioning, and findNextPoint's batchSize argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

from approxposterior_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fantasy_ref as fr  # noqa: E402


def test_fantasy_entry_point_is_exported_bound_and_sized():
    lib = _lib.load()
    for name in ("apgp_acquire_fantasy", "apgp_acquire_fantasy_work_len"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.apgp_abi_version() == 8 and _lib.MAX_FANTASY == 32
    # one (value, index) partial per 256-candidate workgroup
    for m, nblk in ((1, 1), (256, 1), (257, 2), (10 ** 6, 3907)):
        assert lib.apgp_acquire_fantasy_work_len(m) == 2 * nblk
    assert lib.apgp_acquire_fantasy_work_len(0) == 0
    assert lib.apgp_acquire_fantasy_work_len(1 << 41) == -1


def _call(lib, **kw):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ks = _lib.KernelStruct()
    ks.ndim = 2
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    a = dict(T=p, m=4, off=0, xs=p, n=4, ks=ctypes.byref(ks), beta=p, pick=0, j=1, C=p, ldc=4, mu=p,
             vin=p, vout=p + 8 * 4, kind=_lib.UTIL_BAPE, lo=None, hi=None, mask=None, zeta=0.01, ybest=0.0,
             u=None, part=p, best=p)
    a.update(kw)
    if "ndim" in kw:
        ks.ndim = kw["ndim"]
    return lib.apgp_acquire_fantasy(a["T"], a["m"], a["off"], a["xs"], a["n"], a["ks"], a["beta"], a["pick"], a["j"],
                                    a["C"], a["ldc"], a["mu"], a["vin"], a["vout"], a["kind"], a["lo"], a["hi"],
                                    a["mask"], a["zeta"], a["ybest"], a["u"], a["part"], a["best"], None)


@pytest.mark.parametrize("bad, message", [
    (dict(T=None), b"null pointer"), (dict(beta=None), b"null pointer"), (dict(C=None), b"null pointer"),
    (dict(vin=None), b"null pointer"), (dict(part=None), b"null pointer"), (dict(best=None), b"null pointer"),
    (dict(j=0), b"APGP_MAX_FANTASY"), (dict(j=32), b"APGP_MAX_FANTASY"), (dict(j=-3), b"APGP_MAX_FANTASY"),
    (dict(pick=-1), b"pick_row"), (dict(pick=4), b"pick_row"),
    (dict(ldc=3), b"ldc"),
    (dict(vout=None), b"null pointer"),
    (dict(kind=_lib.UTIL_NONE), b"kind"),
    (dict(ndim=_lib.MAX_DIM + 1), b"kernel parameters"),
    (dict(m=0), b"m >= 1"),
])
def test_fantasy_bad_arguments_are_refused_without_a_gpu(bad, message):
    lib = _lib.load()
    assert _call(lib, **bad) == -1
    assert message in lib.apgp_last_error()


def test_fantasy_refuses_aliased_variance_buffers():
    lib = _lib.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert _call(lib, vin=p, vout=p) == -1
    assert b"must not overlap" in lib.apgp_last_error()
    assert _call(lib, vin=p, vout=p + 8) == -1          # partial overlap
    lo = (ctypes.c_double * _lib.MAX_DIM)()
    assert _call(lib, lo=lo) == -1                      # lo without hi
    assert b"together" in lib.apgp_last_error()


def _problem(seed, n, d, amp, lin, gated):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2.0, 2.0, size=(n, d))
    y = np.sin(X).sum(axis=1) - 0.1 * (X ** 2).sum(axis=1) + 0.01 * rs.randn(n)
    # length scales of the order of the spacing of the training points; noise keeps cond(K) moderate
    ell = 4.0 / max(n ** (1.0 / d), 2.0) * rs.uniform(1.0, 3.0, size=d)
    gp = dict(amp=amp, inv_metric=1.0 / ell ** 2, diag_add=1e-5 * amp, mean=float(np.mean(y)),
              lin_coef=0.05 if lin else 0.0, lin_order=1 if lin else 1)
    T = rs.uniform(-2.4, 2.4, size=(400, d))
    bounds = mask = None
    if gated:
        bounds = [(-2.0, 2.0)] * d
        mask = rs.rand(len(T)) > 0.2
    return X, y, T, gp, bounds, mask


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("n, d", [(30, 1), (120, 2), (200, 5)])
@pytest.mark.parametrize("amp, lin, gated", [(1.0, False, False), (3.7, True, True), (0.4, False, True)])
def test_recursion_agrees_with_naive_reconditioning(kind, n, d, amp, lin, gated):
    X, y, T, gp, bounds, mask = _problem(n * 7 + d, n, d, amp, lin, gated)
    q = 8 if d > 1 else 5
    idx, ub, mu, vs = fr.fantasy_batch(X, y, T, kind, q, gp, bounds=bounds, mask=mask)
    idx_r, ub_r, mus_r, vs_r, _ = fr.recondition_batch(X, y, T, kind, q, gp, bounds=bounds, mask=mask)
    assert np.array_equal(idx, idx_r), (idx, idx_r)
    if kind != "jones":
        # distinct picks: a fantasy lowers the pick's variance, which these utilities reward (Jones's expected
        # improvement can come back to a pick once everything else has none, and the slow path does the same)
        assert len(set(idx.tolist())) == q
    for j in range(q):
        # the mean does not move (alpha of the extended set is [alpha; 0]) ...
        assert np.abs(mus_r[j] - mu).max() <= 1e-8 * max(1.0, np.abs(mu).max())
        # ... and the variance is the rank-j downdate
        assert np.abs(vs_r[j] - vs[j]).max() <= 1e-10 * amp, j
    assert np.allclose(ub, ub_r, rtol=1e-6, atol=1e-8)


def test_alternating_kinds_and_an_empty_gate():
    X, y, T, gp, bounds, mask = _problem(3, 60, 2, 1.0, False, True)
    kinds = ["agp", "bape", "agp", "bape"]
    idx, _, _, _ = fr.fantasy_batch(X, y, T, kinds, 4, gp, bounds=bounds, mask=mask)
    idx_r, _, _, _, _ = fr.recondition_batch(X, y, T, kinds, 4, gp, bounds=bounds, mask=mask)
    assert np.array_equal(idx, idx_r)
    none = np.zeros(len(T), dtype=bool)
    idx, ub, _, _ = fr.fantasy_batch(X, y, T, "bape", 3, gp, mask=none)
    assert idx.tolist() == [-1, -1, -1] and np.all(np.isinf(ub))


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


@pytest.mark.parametrize("kw", [dict(batchSize=2), dict(batchSize=33, nCandidates=100),
                                dict(batchSize=0, nCandidates=100), dict(batchSize=2.5, nCandidates=100),
                                dict(batchSize=2, nCandidates=100, polish=True)])
def test_find_next_point_batch_arguments_are_checked_first(kw, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    with pytest.raises(ValueError):
        ap.findNextPoint(computeLnLike=True, numNewPoints=4, verbose=False, **kw)
    assert len(ap.y) == 3


def test_find_next_point_batch_under_a_process_group_is_not_implemented(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    monkeypatch.setattr(ap, "_ranks", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="process group"):
        ap.findNextPoint(computeLnLike=False, numNewPoints=4, nCandidates=100, batchSize=2, verbose=False)


def test_forward_model_of_a_batch_is_the_per_point_expression():
    import pickle
    from approxposterior_amd import approx, likelihood as lh
    f = approx._ForwardModel(lh.rosenbrockLnlike, lh.rosenbrockLnprior, (), {})
    g = pickle.loads(pickle.dumps(f))
    p = np.array([0.3, -1.2])
    assert g(p).shape == (1,) and g(p)[0] == lh.rosenbrockLnlike(p) + lh.rosenbrockLnprior(p)
