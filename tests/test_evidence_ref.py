# -*- coding: utf-8 -*-
"""CPU: the evidence estimate's host side (utility.mergeImportance, utility.importanceSummary) against the restatement of
tests/evidence_ref.py and closed forms, and the statistical check -- made here with the reference arithmetic alone --
that the seed and size the GPU test uses put the box-proposal estimate within 4 logZErr of a quadrature of exp(mu)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import kvalue_ref as kr  # noqa: E402
from philox_ref import philox_box_numpy  # noqa: E402

from approxposterior_amd import utility as ut  # noqa: E402


def _rows(m, D, seed, shift=0.0, spread=3.0):
    rs = np.random.RandomState(seed)
    T = rs.normal(size=(m, D))
    lw = shift + spread * rs.normal(size=m)
    lw[rs.uniform(size=m) < 0.1] = -np.inf
    return T, lw


def _close(a, b, rtol):
    for key in ("lmax", "S0", "S2", "cnt"):
        assert abs(a[key] - b[key]) <= rtol * abs(b[key]), key
    for key in ("s1", "S"):
        scale = np.abs(b[key]).max() + 1e-300
        assert np.abs(np.asarray(a[key]) - b[key]).max() <= rtol * max(scale, b["S0"]), key


@pytest.mark.parametrize("gap", [0.0, 30.0, 800.0])
def test_merge_is_associative_and_matches_the_restatement(gap):
    c = np.array([0.2, -0.4, 1.0])
    recs = []
    for i, shift in enumerate((0.0, gap, -gap)):
        T, lw = _rows(300 + 17 * i, 3, 5 + i, shift=shift)
        recs.append(er.record(lw, T, c))
    a, b, d = recs
    left = ut.mergeImportance(ut.mergeImportance(a, b), d)
    right = ut.mergeImportance(a, ut.mergeImportance(b, d))
    _close(left, right, 1e-14)
    _close(left, er.merge(er.merge(a, b), d), 1e-14)
    # the two orders of one pair agree too, and lmax is the larger one
    ab, ba = ut.mergeImportance(a, b), ut.mergeImportance(b, a)
    _close(ab, ba, 1e-14)
    assert ab["lmax"] == max(a["lmax"], b["lmax"]) and ab["cnt"] == a["cnt"] + b["cnt"]


def test_merge_handles_the_empty_record_and_refuses_two_centres():
    c = np.zeros(2)
    T, lw = _rows(50, 2, 1)
    full = er.record(lw, T, c)
    empty = er.record(np.full(7, -np.inf), np.zeros((7, 2)), c)
    assert empty["lmax"] == -np.inf and empty["S0"] == 0.0 and empty["cnt"] == 0.0
    for m in (ut.mergeImportance(full, empty), ut.mergeImportance(empty, full)):
        for key in ("lmax", "S0", "S2", "cnt"):
            assert m[key] == full[key]
        assert np.array_equal(m["s1"], full["s1"]) and np.array_equal(m["S"], full["S"])
    both = ut.mergeImportance(empty, empty)
    assert both["lmax"] == -np.inf and both["S0"] == 0.0 and not np.any(both["S"])
    s = ut.importanceSummary(both, 14)
    assert s["logZ"] == -np.inf and s["ess"] == 0.0 and s["nInside"] == 0 and np.all(np.isnan(s["mean"]))
    other = er.record(lw, T, np.ones(2))
    with pytest.raises(ValueError):
        ut.mergeImportance(full, other)


def test_summary_of_a_hand_built_record_matches_closed_forms():
    # four rows with weights e = (1, 1/2, 1/4, 0) times exp(3), about c = (1, -1)
    c = np.array([1.0, -1.0])
    T = np.array([[1.0, -1.0], [2.0, -1.0], [1.0, 1.0], [9.0, 9.0]])
    lw = np.array([3.0, 3.0 + np.log(0.5), 3.0 + np.log(0.25), -np.inf])
    rec = er.record(lw, T, c)
    s = ut.importanceSummary(rec, 4, logVolume=np.log(2.0))
    S0, S2 = 1.75, 1.0 + 0.25 + 0.0625
    assert abs(s["logZ"] - (3.0 + np.log(S0) - np.log(4.0) + np.log(2.0))) <= 4e-16 * 4
    assert abs(s["ess"] - S0 ** 2 / S2) <= 1e-15 * 4
    assert abs(s["logZErr"] - np.sqrt((4 * S2 / S0 ** 2 - 1) / 4)) <= 1e-15
    mean = (1.0 * T[0] + 0.5 * T[1] + 0.25 * T[2]) / S0
    assert np.allclose(s["mean"], mean, rtol=0, atol=1e-15)
    d = T[:3] - mean
    cov = np.einsum("m,mi,mj->ij", np.array([1.0, 0.5, 0.25]) / S0, d, d)
    assert np.allclose(s["cov"], cov, rtol=0, atol=2e-15) and s["nInside"] == 3
    ref = er.summary(rec, 4, logVolume=np.log(2.0))
    assert s["logZ"] == ref["logZ"] and s["ess"] == ref["ess"] and np.array_equal(s["cov"], ref["cov"])
    # equal weights: no scatter, the error is 0 and every row is effective
    flat = ut.importanceSummary(er.record(np.full(5, -2.0), np.zeros((5, 2)), c), 5)
    assert flat["logZErr"] == 0.0 and flat["ess"] == 5.0 and flat["logZ"] == -2.0


@pytest.mark.parametrize("gap", [0.0, 800.0])
def test_a_record_split_at_any_point_merges_to_the_unsplit_one(gap):
    c = np.array([0.5, 0.0, -0.5])
    T, lw = _rows(64, 3, 11)
    lw[40:] += gap                       # the second part may tower over the first
    whole = er.record(lw, T, c)
    for cut in range(0, 65):
        parts = [er.record(lw[:cut], T[:cut], c), er.record(lw[cut:], T[cut:], c)]
        _close(ut.mergeImportance(parts[0], parts[1]), whole, 1e-13)


@functools.lru_cache(maxsize=None)
def box_estimate(seed=er.EVIDENCE_SEED, m=er.EVIDENCE_M):
    """The restatement's box-proposal record of the quadratic case -- rows from philox_box_numpy, mu in long double --
    with the log of the box volume and the largest per-row budget of a device logw."""
    case = er.quadratic_case()
    X, y, metric, mean, _ = case
    _, alpha = er.oracle_gp(case)
    k = kr.kern(1.0 / metric)
    b = np.asarray(er.QUAD_BOUNDS)
    T = philox_box_numpy(m, 2, b[:, 0], b[:, 1], seed, 0)
    lw, bud = er.logw_truth(T, X, alpha, k, mean, lnq=None, bounds=er.QUAD_BOUNDS)
    centre = X[int(np.argmax(y))]
    rec = er.record(lw, T, centre)
    return rec, float(np.sum(np.log(b[:, 1] - b[:, 0]))), float(bud.max())


def test_box_estimate_of_the_quadratic_case_lies_within_four_errors_of_the_quadrature():
    """The seed (evidence_ref.EVIDENCE_SEED, the first one tried) and M = 2^16 of the GPU test satisfy the statistical
    condition with the reference arithmetic alone."""
    rec, logV, _ = box_estimate()
    s = ut.importanceSummary(rec, er.EVIDENCE_M, logVolume=logV)
    logZ, mean, cov = er.quadrature(er.quadratic_case())
    print("logZ %.6f +- %.6f (quadrature %.6f, %.2f errors), ess %.0f" %
          (s["logZ"], s["logZErr"], logZ, abs(s["logZ"] - logZ) / s["logZErr"], s["ess"]))
    assert s["nInside"] == er.EVIDENCE_M
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    # the moments: within 5 importance-sampling standard errors, sqrt(var / ess)
    se = np.sqrt(np.diag(cov) / s["ess"])
    assert np.all(np.abs(s["mean"] - mean) <= 5.0 * se)


def test_mixture_component_boundaries_are_rare_for_the_seeds_of_the_gpu_test():
    """The GPU test skips component uniforms within 1 ulp of a cumulative weight and allows 2 per 1e5 rows: the
    restatement alone stays within that cap for every seed and mixture the GPU test uses."""
    for K, D, seed in er.MIX_CASES:
        w, means, covs = er.mixture(K, D, seed)
        _, _, _, near, _ = er.mix_candidates_numpy(100000, w, means, covs, seed)
        assert near.sum() <= 2, (K, D, seed, int(near.sum()))
