# -*- coding: utf-8 -*-
"""CPU: the reference of the evidence over posterior function draws (tests/pathevidence_ref.py) -- the identity the
feature rests on, the per-draw merge over row ranges, and utility.importanceDrawsSummary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import pathdraw_ref as pr  # noqa: E402
import pathevidence_ref as per  # noqa: E402

from approxposterior_amd import utility as ut  # noqa: E402


@pytest.mark.parametrize("seed", [0, 1])
def test_mean_of_the_draws_evidences_is_the_evidence_of_the_expected_posterior(seed):
    """mean_s Z_s -> mean_i exp(mu_i + v_i / 2): 256 draws in 8 groups of 32, threshold 5 standard errors as in the
    path-draw moment tests (the reference alone gives |z| = 0.12 and 0.13 at seeds 0 and 1); the plug-in value
    mean_i exp(mu_i) fails the same check, so the test sees the variance."""
    fx, _, F = per.moment_draws(seed)
    assert F.shape == (256, 256)
    recs = per.records(per.logw(F, fx["T"]), fx["T"], np.zeros(fx["k"].ndim))
    Zs = per.evidences(recs, F.shape[1])
    assert np.allclose(Zs, np.exp(F).mean(axis=1), rtol=1e-12)
    z, zplug = per.identity_scores(Zs, fx)
    print("seed %d: |z| = %.2f against exp(mu + v / 2), %.2f against exp(mu)" % (seed, z, zplug))
    assert z <= 5.0
    assert zplug > 5.0
    # the same number through the summary of the draws
    summ = ut.importanceDrawsSummary(recs, F.shape[1])
    assert np.isclose(np.exp(summ["logZExpected"]), Zs.mean(), rtol=1e-12) and summ["nEmptyDraws"] == 0


def _small_case():
    c = pr.case(20, 64, 16, 3, 2, seed=5)
    rs = np.random.RandomState(6)
    lnq = rs.uniform(-2.0, 2.0, size=64)
    centre = np.array([0.1, -0.2])
    lw, recs = per.reference(c["T"], c["X"], c["V"], c["Z"], c["b"], c["W"], c["Wl"], c["k"], c["mean"], lnq=lnq,
                             bounds=[(-2.1, 2.1)] * 2, centre=centre)
    return c, lw, recs, centre


def test_reference_gate_and_records():
    c, lw, recs, centre = _small_case()
    T = c["T"]
    out = np.any(np.abs(T) > 2.1, axis=1)
    assert out.any() and not out.all()
    assert np.all(np.isneginf(lw[:, out])) and np.all(np.isfinite(lw[:, ~out]))
    for s, r in enumerate(recs):
        assert r["lmax"] == lw[s].max() and r["cnt"] == float((~out).sum())
        assert 1.0 <= r["S0"] <= r["cnt"] and np.array_equal(r["centre"], centre)
    # NaN / inf coordinates and non-finite ln q are gated; a non-finite draw value gates its own draw only
    T2 = T.copy()
    T2[0, 0], T2[1, 1] = np.nan, np.inf
    lnq = np.zeros(len(T))
    lnq[2], lnq[3], lnq[4] = np.nan, np.inf, -np.inf
    F = np.zeros((2, len(T)))
    F[1, 5] = np.inf
    g = per.logw(F, T2, lnq)
    assert np.all(np.isneginf(g[:, :5])) and g[0, 5] == 0.0 and np.isneginf(g[1, 5]) and np.all(g[:, 6:] == 0.0)
    empty = per.records(np.full((1, len(T)), -np.inf), T, centre)[0]
    assert empty["lmax"] == -np.inf and empty["S0"] == empty["S2"] == empty["cnt"] == 0.0
    assert not empty["s1"].any() and not empty["S"].any()


@pytest.mark.parametrize("quarter", [1, 2, 3])
def test_per_draw_records_merge_over_row_ranges(quarter):
    """Records of two row ranges merged by utility.mergeImportance equal the record of all rows within
    evidence_ref.record_budget -- with the second range 800 below the first, and the other way round, so that one side's
    weights vanish against the other's maximum."""
    c, lw, _, centre = _small_case()
    T = c["T"]
    cut = quarter * len(T) // 4
    for gap in (None, -800.0, 800.0):
        lws = lw.copy()
        if gap is not None:          # the second range's maximum `gap` above the first's
            lws[:, cut:] += (gap + lw[:, :cut].max(axis=1) - lw[:, cut:].max(axis=1))[:, None]
        for s in range(len(lws)):
            a = er.record(lws[s, :cut], T[:cut], centre)
            b = er.record(lws[s, cut:], T[cut:], centre)
            if gap is not None:
                assert abs(abs(a["lmax"] - b["lmax"]) - 800.0) < 1e-9
            got = ut.mergeImportance(a, b)
            want = er.record(lws[s], T, centre)
            b0, b2, b1, bS = er.record_budget(lws[s], T, centre)
            assert got["lmax"] == want["lmax"] and got["cnt"] == want["cnt"]
            assert abs(got["S0"] - want["S0"]) <= b0 * want["S0"]
            assert abs(got["S2"] - want["S2"]) <= b2 * want["S2"]
            assert np.all(np.abs(got["s1"] - want["s1"]) <= b1)
            assert np.all(np.abs(got["S"] - want["S"]) <= bS)


def _rec(lmax, S0, D=2, cnt=10.0):
    return {"lmax": lmax, "S0": S0, "S2": S0 * S0 / 5.0 if S0 else 0.0, "cnt": cnt if S0 else 0.0,
            "s1": np.full(D, 0.1 * S0), "S": np.eye(D) * S0, "centre": np.zeros(D)}


def test_importance_draws_summary():
    recs = [_rec(-3.0, 4.0), _rec(-2.5, 2.0), _rec(-4.0, 7.0)]
    m, lv = 50, 0.7
    out = ut.importanceDrawsSummary(recs, m, logVolume=lv)
    one = [ut.importanceSummary(r, m, logVolume=lv) for r in recs]
    assert out["logZDraws"].shape == (3,) and out["essDraws"].shape == (3,)
    assert out["meanDraws"].shape == (3, 2) and out["covDraws"].shape == (3, 2, 2)
    for s in range(3):
        assert out["logZDraws"][s] == one[s]["logZ"] and out["essDraws"][s] == one[s]["ess"]
        assert np.array_equal(out["meanDraws"][s], one[s]["mean"]) and np.array_equal(out["covDraws"][s], one[s]["cov"])
    Z = np.array([np.exp(r["lmax"]) * r["S0"] / m * np.exp(lv) for r in recs])
    assert np.isclose(out["logZExpected"], np.log(Z.mean()), rtol=0, atol=1e-14)
    assert np.isclose(out["logZSurrogateErr"], np.std(np.log(Z), ddof=1), rtol=1e-13)
    assert out["meanSurrogateErr"].shape == (2,)
    assert np.allclose(out["meanSurrogateErr"], np.std(out["meanDraws"], axis=0, ddof=1), rtol=1e-13)
    assert out["nEmptyDraws"] == 0
    # log-evidences hundreds apart do not overflow
    far = ut.importanceDrawsSummary([_rec(-3.0, 4.0), _rec(900.0, 1.0)], m)
    assert np.isclose(far["logZExpected"], 900.0 - np.log(m) - np.log(2.0), atol=1e-12)


def test_importance_draws_summary_of_one_draw_and_of_empty_draws():
    one = ut.importanceDrawsSummary([_rec(-3.0, 4.0)], 50)
    assert np.isnan(one["logZSurrogateErr"]) and np.all(np.isnan(one["meanSurrogateErr"]))
    assert one["logZExpected"] == one["logZDraws"][0] and one["nEmptyDraws"] == 0
    recs = [_rec(-3.0, 4.0), _rec(-np.inf, 0.0), _rec(-2.0, 1.0)]
    out = ut.importanceDrawsSummary(recs, 50)
    both = ut.importanceDrawsSummary([recs[0], recs[2]], 50)
    assert out["nEmptyDraws"] == 1 and out["logZDraws"][1] == -np.inf and out["essDraws"][1] == 0.0
    assert np.all(np.isnan(out["meanDraws"][1]))
    for key in ("logZSurrogateErr", "logZExpected"):
        assert out[key] == both[key]
    assert np.array_equal(out["meanSurrogateErr"], both["meanSurrogateErr"])
    none = ut.importanceDrawsSummary([_rec(-np.inf, 0.0)], 50)
    assert none["nEmptyDraws"] == 1 and none["logZExpected"] == -np.inf and np.isnan(none["logZSurrogateErr"])
    with pytest.raises(ValueError):
        ut.importanceDrawsSummary([], 50)


def test_work_len_formula():
    per_wg = 3 + 32 + 528
    assert per.work_len(1, 1) == 1 + 1 + 1 + per_wg
    assert per.work_len(257, 32) == 32 * (2 + 257 + 1 + 2 * per_wg)
    assert per.work_len(per.ROW_CAP + 1, 1) == 2049 + per.ROW_CAP + 1 + 1 + 2048 * per_wg
    assert per.work_len(0, 1) == 0 and per.work_len(1, 0) == 0
    assert per.work_len((1 << 40) + 1, 1) == -1 and per.work_len(1, 33) == -1


def test_public_name():
    import approxposterior_amd as ap
    assert ap.importanceDrawsSummary is ut.importanceDrawsSummary
