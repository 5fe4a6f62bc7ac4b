# -*- coding: utf-8 -*-
"""CPU: the quasi-random draws' definition (tests/sobol_ref.py) against torch's SobolEngine and the issue's anchors, the
compiled direction numbers, the entry points' argument checks (before any HIP call: there is no GPU here), the replicate
arithmetic of utility.importanceReplicatesSummary and evidence(qmc=)'s refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sobol_ref as sr  # noqa: E402
from test_evidence_arguments_host import _params  # noqa: E402

from approxposterior_amd import _lib  # noqa: E402
from approxposterior_amd import utility as ut  # noqa: E402


def _hex(v):
    return " ".join("%08x" % int(x) for x in np.ravel(v))


def test_compiled_direction_numbers_are_torchs():
    lib = _lib.load()
    V = sr.directions()
    got = np.array([[lib.apgp_sobol_direction(d, b) for b in range(sr.BITS)] for d in range(sr.DIMS)], dtype=np.int64)
    assert np.array_equal(got, V)
    assert _hex(V[1, :4] << 2) == "80000000 c0000000 a0000000 f0000000"
    assert _hex(V[32, :4] << 2) == "80000000 c0000000 20000000 30000000"
    for d, b in ((-1, 0), (33, 0), (0, -1), (0, 30), (1 << 20, 1 << 20)):
        assert lib.apgp_sobol_direction(d, b) == -1


@pytest.mark.parametrize("D", [1, 3, 8, 33])
def test_unscrambled_points_are_sobolengines(D):
    import torch
    ref = torch.quasirandom.SobolEngine(D, scramble=False).draw(5000, dtype=torch.float64).numpy() * 2.0 ** 32
    x = sr.scrambled(5000, D, seed=7, replicate=3, scramble=False)          # (seed and replicate change nothing)
    assert np.array_equal(x.astype(np.float64), ref)
    assert np.all(x[0] == 0)
    # any row range is computable alone
    assert np.array_equal(sr.points(300, D, offset=4700), x[4700:])
    u = sr.uniforms(5000, D, 0, scramble=False)
    assert u.min() == 2.0 ** -33 and u.max() < 1.0


def test_scramble_anchors():
    h = 0x9E3779B9
    for v, want in ((0x00000000, 0xBAC6D875), (0x80000000, 0x4B228BE7), (0x40000000, 0xF6CC311C), (0xC0000000, 0x350F5CCE),
                    (0x12345678, 0xA61C7925)):
        assert int(sr.rev32(sr.lk(sr.rev32(v), h))) == want, "%08x" % v
    assert _hex(sr.hash_seeds(3, 12345, 2)) == "0c7b167f 65fa25b7 33fa6917"
    x = sr.scrambled(9, 3, seed=12345, replicate=2)
    assert _hex(x[5]) == "74b791d2 6cf78768 f2c3ebfa"
    assert _hex(x[8]) == "f822f7aa a564961d 7070437b"
    assert np.array_equal(sr.scrambled(1, 3, seed=12345, replicate=2, offset=8)[0], x[8])
    # another replicate, another seed: other points
    assert not np.array_equal(sr.scrambled(9, 3, seed=12345, replicate=1), x)
    assert not np.array_equal(sr.scrambled(9, 3, seed=12346, replicate=2), x)
    u = sr.uniforms(4096, 3, 12345, 2)
    assert 0.0 < u.min() and u.max() < 1.0


@pytest.mark.parametrize("seed", [0, 1, 20261020, 2 ** 40 + 5])
def test_scrambled_points_keep_the_net_properties(seed):
    K = 10
    x = sr.scrambled(1 << K, 4, seed, replicate=seed % 3)
    for k in range(1, K + 1):
        n = 1 << k
        cells = (x[:n] >> np.uint64(32 - k)).astype(np.int64)
        # one point in each of the 2^k intervals of every dimension
        for d in range(x.shape[1]):
            assert np.array_equal(np.sort(cells[:, d]), np.arange(n)), (k, d)
        # one point in each k1 + k2 = k cell of dimensions (0, 1)
        for k1 in range(k + 1):
            a = (x[:n, 0] >> np.uint64(32 - k1)).astype(np.int64) if k1 else np.zeros(n, dtype=np.int64)
            b = (x[:n, 1] >> np.uint64(32 - (k - k1))).astype(np.int64) if k1 < k else np.zeros(n, dtype=np.int64)
            assert len(np.unique(a * n + b)) == n, (k, k1)
    # aligned blocks [j 2^k, (j + 1) 2^k) are stratified in one dimension too
    for k in (3, 6):
        n = 1 << k
        for j in (1, 5, (1 << (K - k)) - 1):
            blk = (x[j * n:(j + 1) * n] >> np.uint64(32 - k)).astype(np.int64)
            for d in range(x.shape[1]):
                assert np.array_equal(np.sort(blk[:, d]), np.arange(n)), (k, j, d)


def _box_call(lib, T, m=4, D=2, off=0, rep=0, scr=1, lo=None, hi=None):
    arr = ctypes.c_double * _lib.MAX_DIM
    lo = arr() if lo is None else lo
    hi = arr(*([1.0] * _lib.MAX_DIM)) if hi is None else hi
    return lib.apgp_sobol_box_candidates(T, m, D, lo, hi, 1, rep, scr, off, None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    T = ctypes.addressof(buf)
    full = 1 << 30
    # box
    assert _box_call(lib, T, m=0) == 0                                      # nothing to draw: no launch
    assert _box_call(lib, None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert b"apgp_sobol_box_candidates" in lib.apgp_last_error()
    assert _box_call(lib, T, D=0) == -1 and _box_call(lib, T, D=_lib.MAX_DIM + 1) == -1
    assert _box_call(lib, T, m=-1) == -1 and _box_call(lib, T, off=-1) == -1
    assert _box_call(lib, T, m=2, off=full - 1) == -1 and b"2^30" in lib.apgp_last_error()
    assert _box_call(lib, T, m=full + 1, off=0) == -1 and _box_call(lib, T, m=1, off=full) == -1
    assert _box_call(lib, T, m=0, off=full) == 0
    assert _box_call(lib, T, rep=-1) == -1 and b"replicate" in lib.apgp_last_error()
    assert _box_call(lib, T, scr=2) == -1 and _box_call(lib, T, scr=-1) == -1 and b"scramble" in lib.apgp_last_error()
    arr = ctypes.c_double * _lib.MAX_DIM
    assert _box_call(lib, T, lo=arr(*([2.0] * _lib.MAX_DIM))) == -1          # lo > hi
    assert _box_call(lib, T, hi=arr(*([float("inf")] * _lib.MAX_DIM))) == -1
    # prior
    kind = np.array([0, 1], dtype=np.int32)
    p0, p1 = np.array([0.0, 0.5]), np.array([1.0, 2.0])

    def prior_call(t=T, m=4, D=2, off=0, rep=0, scr=1, k=kind, a=p0, b=p1):
        ptr = lambda v: None if v is None else v.ctypes.data      # noqa: E731
        return lib.apgp_sobol_prior_candidates(t, m, D, ptr(k), ptr(a), ptr(b), 1, rep, scr, off, None)
    assert prior_call(m=0) == 0
    assert prior_call(t=None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert prior_call(k=None) == -1 and prior_call(a=None) == -1 and prior_call(b=None) == -1
    assert prior_call(D=0) == -1 and prior_call(D=_lib.MAX_DIM + 1) == -1
    assert prior_call(m=-1) == -1 and prior_call(off=-1) == -1
    assert prior_call(m=2, off=full - 1) == -1 and prior_call(rep=-1) == -1 and prior_call(scr=2) == -1
    assert prior_call(k=np.array([0, 2], dtype=np.int32)) == -1
    assert prior_call(b=np.array([1.0, 0.0])) == -1 and prior_call(b=np.array([0.0, 1.0])) == -1     # sigma = 0; low = high
    assert b"apgp_sobol_prior_candidates" in lib.apgp_last_error()
    # mixture
    good = _params(2, 2)

    def mix_call(rec=good, t=T, m=4, D=2, K=2, off=0, rep=0, scr=1):
        return lib.apgp_sobol_mix_candidates(t, None, m, D, K, rec.ctypes.data if rec is not None else None, 1, rep, scr,
                                             off, None)
    assert mix_call(m=0) == 0
    assert mix_call(t=None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert mix_call(rec=None) == -1
    assert mix_call(D=0) == -1 and mix_call(D=_lib.MAX_DIM + 1) == -1 and mix_call(K=0) == -1 and mix_call(K=17) == -1
    assert mix_call(m=-1) == -1 and mix_call(off=-1) == -1
    assert mix_call(m=2, off=full - 1) == -1 and mix_call(rep=-1) == -1 and mix_call(scr=2) == -1
    bad = good.copy()
    bad[1, 0] = 0.999                                                       # the last cumulative weight is not 1.0
    assert mix_call(rec=bad) == -1 and b"apgp_sobol_mix_candidates" in lib.apgp_last_error()
    bad = good.copy()
    bad[1, 8] = 0.0                                                         # A[0][0] = 0
    assert mix_call(rec=bad) == -1
    assert mix_call(_params(_lib.MAX_DIM, 1), D=_lib.MAX_DIM, K=1, m=0) == 0   # D = 32 (table row 32) passes the checks


def _record(lmax, S0, S2, s1, S, cnt, centre):
    return {"lmax": lmax, "S0": S0, "S2": S2, "cnt": cnt, "s1": np.array(s1, dtype=float), "S": np.array(S, dtype=float),
            "centre": np.array(centre, dtype=float)}


def test_replicates_summary_against_a_hand_computation():
    c = [1.0, -1.0]
    recs = [_record(-2.0, 3.0, 2.5, [0.3, 0.6], [[1.0, 0.1], [0.1, 2.0]], 4, c),
            _record(-1.5, 2.0, 1.5, [-0.2, 0.4], [[0.8, 0.0], [0.0, 1.0]], 4, c),
            _record(-2.5, 3.5, 3.25, [0.7, -0.35], [[1.5, -0.2], [-0.2, 0.9]], 3, c)]
    n, logV = 4, 0.75
    out = ut.importanceReplicatesSummary(recs, n, logVolume=logV)
    # by hand: Z_r = exp(lmax_r) S0_r / n (times the volume)
    Zr = np.array([np.exp(r["lmax"]) * r["S0"] / n for r in recs])
    assert np.allclose(out["logZReplicates"], np.log(Zr) + logV, rtol=0, atol=1e-14)
    assert abs(out["logZ"] - (np.log(Zr.mean()) + logV)) <= 1e-14           # equal sizes: the pooled mean weight
    assert abs(out["logZErr"] - np.std(Zr, ddof=1) / np.sqrt(3) / Zr.mean()) <= 1e-15
    means = np.array([np.array(c) + r["s1"] / r["S0"] for r in recs])
    assert np.allclose(out["meanReplicates"], means, rtol=0, atol=1e-15)
    assert np.allclose(out["meanErr"], np.std(means, axis=0, ddof=1) / np.sqrt(3), rtol=0, atol=1e-15)
    e, m = sr.replicates_summary(out["logZReplicates"], out["meanReplicates"])
    assert abs(e - out["logZErr"]) <= 1e-15 and np.allclose(m, out["meanErr"], rtol=0, atol=1e-15)
    # the pooled keys are importanceSummary of the merged record over R n rows; logZErrIID is its delta-method figure
    pooled = ut.importanceSummary(ut.mergeImportance(ut.mergeImportance(recs[0], recs[1]), recs[2]), 3 * n, logVolume=logV)
    assert out["logZ"] == pooled["logZ"] and out["ess"] == pooled["ess"] and out["nInside"] == 11
    assert np.array_equal(out["mean"], pooled["mean"]) and np.array_equal(out["cov"], pooled["cov"])
    assert out["logZErrIID"] == pooled["logZErr"] and out["qmc"] == 3
    w = np.exp([r["lmax"] for r in recs]) * np.array([r["S0"] for r in recs])
    assert np.allclose(out["mean"], np.array(c) + (w[:, None] * (means - c)).sum(axis=0) / w.sum(), rtol=0, atol=1e-14)
    # replicates far apart in lmax do not overflow; an empty replicate counts as Z_r = 0
    far = ut.importanceReplicatesSummary([_record(-900.0, 1.0, 1.0, [0, 0], np.zeros((2, 2)), 1, c),
                                          _record(800.0, 1.0, 1.0, [0, 0], np.zeros((2, 2)), 1, c)], 1)
    assert np.isfinite(far["logZ"]) and abs(far["logZErr"] - 1.0) <= 1e-15
    empty = _record(-np.inf, 0.0, 0.0, [0, 0], np.zeros((2, 2)), 0, c)
    half = ut.importanceReplicatesSummary([recs[0], empty], n)
    assert abs(half["logZErr"] - 1.0) <= 1e-15 and half["logZReplicates"][1] == -np.inf and np.all(np.isnan(half["meanErr"]))
    none = ut.importanceReplicatesSummary([empty, empty], n)
    assert none["logZ"] == -np.inf and np.isnan(none["logZErr"])
    with pytest.raises(ValueError):
        ut.importanceReplicatesSummary([recs[0]], n)


def test_evidence_refuses_a_bad_qmc_and_the_names_are_public():
    import approxposterior_amd as ap
    X = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.2]])
    a = ap.ApproxPosterior(theta=X, y=np.array([0.0, -1.0, -0.5]), lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                           priorSample=lambda n=1: np.zeros((n, 2)), bounds=[(0.0, 1.0), (0.0, 1.0)], gp=object())
    with pytest.raises(ValueError, match="qmc"):
        a.evidence(nSamples=1024, proposal="box", qmc=1)
    with pytest.raises(ValueError, match="qmc"):
        a.evidence(nSamples=8, proposal="box", qmc=16)
    with pytest.raises(ValueError, match="qmc"):
        a.evidence(nSamples=1024, proposal="box", qmc=0)
    assert ap.importanceReplicatesSummary is ut.importanceReplicatesSummary
    assert ap.sobolSample is ap.gp.sobolSample
    with pytest.raises(ValueError):
        ap.sobolSample(8)
    with pytest.raises(ValueError):
        ap.sobolSample(8, bounds=[(0, 1)], prior=object())
    # deviceCandidates learns its third value; anything else spelled out is refused
    assert a._candidatesMode("sobol") == "sobol" and a._candidatesMode(True) is True and a._candidatesMode(0) is False
    with pytest.raises(ValueError):
        a._candidatesMode("halton")
    a.deviceCandidates = "sobol"
    with pytest.raises(ValueError, match="2\\^30"):
        a._candidateDraw((1 << 30) + 1, None)
