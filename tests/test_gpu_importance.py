# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): apgp_importance_pass through GP.importance_pass on given rows (DESIGN.md "Evidence by importance
sampling").  logw against the long-double truth of tests/evidence_ref.py within the issue's bound

    (N + 2) u sum_n |k_n alpha_n| + sum_n budget_n |alpha_n| + u (|mu| + |lnq|)

(kvalue_ref.budget per kernel value), the record against the restatement applied to the device's own logw within
evidence_ref.record_budget (m u on the sums plus the exp's E_EXP ulps per row), the gate, determinism, agreement with
apgp_predict_mean, linear-term kernels and weights spanning 1500 in the exponent."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import kvalue_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 8, 32)
NS = (5, 512, 513)            # padding only, exactly one row block, two row blocks
MS = (1, 63, 64, 65, 257)
MMAX = max(MS)


def _gp(D, N, lin_order=None, seed=0):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(1000 * D + N + seed)
    X = rs.uniform(-2.0, 2.0, size=(N, D))
    y = -0.5 * np.sum((X - 0.3) ** 2, axis=1) / D + 0.1 * np.sin(3.0 * X[:, 0])
    kernel = agp.ExpSquaredKernel(rs.uniform(2.0, 5.0, size=D) * D, ndim=D)
    if lin_order is not None:
        kernel = kernel + 0.3 * agp.LinearKernel(log_gamma2=0.4, order=lin_order, ndim=D)
    g = agp.GP(kernel=kernel, fit_mean=True, mean=float(np.median(y)), white_noise=-7.0, fit_white_noise=False)
    g.compute(X)
    return g, X, y


def _kern(g):
    ks = g._kernel_struct()
    return kr.kern(np.array(ks.inv_metric[:ks.ndim]), amp=ks.amp, diag_add=ks.diag_add, lin_coef=ks.lin_coef,
                   lin_order=ks.lin_order)


def _alpha(g, y):
    g._ensure_xs(np.asarray(y, dtype=np.float64))
    return g._alpha.cpu().numpy().copy()


def _rows(D, m, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-2.5, 2.5, size=(m, D)), rs.normal(size=m) - 1.0


@functools.lru_cache(maxsize=None)
def _case(D, N, lin_order=None):
    g, X, y = _gp(D, N, lin_order)
    T, lnq = _rows(D, MMAX, 7 * D + N)
    alpha = _alpha(g, y)
    bounds = [(-2.4, 2.4)] * D
    lw, bud = er.logw_truth(T, X, alpha, _kern(g), float(g.mean.value), lnq=lnq, bounds=bounds)
    for a in (lw, bud):                  # (T and lnq go to torch.from_numpy, which wants writable arrays: nobody writes them)
        a.setflags(write=False)
    return g, X, y, T, lnq, bounds, lw, bud


def _check_logw(dev, lw, bud):
    fin = lw > -np.inf
    assert np.array_equal(np.isneginf(dev), ~fin)
    err = np.abs(dev[fin].astype(np.longdouble) - lw[fin]).astype(np.float64)
    ratio = float((err / bud[fin]).max()) if fin.any() else 0.0
    assert ratio <= 1.0, "logw off by %.3f budgets" % ratio
    return ratio


def _check_record(rec, logw_dev, T, c):
    want = er.record(logw_dev, T, c)
    b0, b2, b1, bS = er.record_budget(logw_dev, T, c)
    assert rec["lmax"] == want["lmax"] and rec["cnt"] == want["cnt"]
    if want["S0"] == 0.0:
        assert rec["S0"] == 0.0 and rec["S2"] == 0.0 and not np.any(rec["s1"]) and not np.any(rec["S"])
        return 0.0
    r = [abs(rec["S0"] - want["S0"]) / (b0 * want["S0"]), abs(rec["S2"] - want["S2"]) / (b2 * want["S2"]),
         float((np.abs(rec["s1"] - want["s1"]) / b1).max()), float((np.abs(rec["S"] - want["S"]) / bS).max())]
    assert max(r) <= 1.0, "record off by %s budgets (S0, S2, s1, S)" % (r,)
    assert np.array_equal(rec["S"], rec["S"].T)
    return max(r)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DIMS)
def test_logw_and_record_over_the_shape_grid(D, N):
    g, X, y, T, lnq, bounds, lw, bud = _case(D, N)
    c = X[int(np.argmax(y))]
    worst_w = worst_r = 0.0
    for m in MS:
        rec, logw = g.importance_pass(y, T[:m], lnq=lnq[:m], bounds=bounds, return_logw=True)
        dev = logw.cpu().numpy()
        assert np.array_equal(rec["centre"], c)
        worst_w = max(worst_w, _check_logw(dev, lw[:m], bud[:m]))
        worst_r = max(worst_r, _check_record(rec, dev, T[:m], c))
    print("D=%d N=%d: largest |logw - truth| / budget = %.3f, largest record error / budget = %.3f" % (D, N, worst_w, worst_r))


def test_a_workgroup_takes_a_second_tile():
    """At most APGP_IMP_MAX_BLOCKS = 2048 workgroups of APGP_IMP_BLOCK = 256 candidates run: with M = 256 * 2048 + 1 =
    524289 rows workgroup 0 takes a second tile (row 524288).  logw is checked against the truth on the first, the last
    and a seeded sample of rows (the truth of all of them costs minutes), against a small call bit for bit on the first
    rows (a row's result does not depend on the other rows), and the record against the restatement on ALL rows."""
    from approxposterior_amd import _lib
    D, N = 3, 64
    M = _lib.IMP_BLOCK * _lib.IMP_MAX_BLOCKS + 1
    assert M == 524289
    g, X, y = _gp(D, N)
    T, lnq = _rows(D, M, 99)
    bounds = [(-2.4, 2.4)] * D
    c = X[int(np.argmax(y))]
    rec, logw = g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True)
    dev = logw.cpu().numpy()
    pick = np.unique(np.concatenate([np.arange(300), np.arange(M - 300, M), np.random.RandomState(3).randint(0, M, 600)]))
    lw, bud = er.logw_truth(T[pick], X, _alpha(g, y), _kern(g), float(g.mean.value), lnq=lnq[pick], bounds=bounds)
    print("second tile: largest |logw - truth| / budget = %.3f" % _check_logw(dev[pick], lw, bud))
    _, small = g.importance_pass(y, T[:257], lnq=lnq[:257], bounds=bounds, return_logw=True)
    assert np.array_equal(small.cpu().numpy(), dev[:257])
    print("second tile: largest record error / budget = %.3f" % _check_record(rec, dev, T, c))


def test_gate_cases():
    g, X, y, T, lnq, bounds, lw, bud = _case(3, 512)
    T, lnq = T[:65].copy(), lnq[:65].copy()
    inside = np.all((T >= -2.4) & (T <= 2.4), axis=1)
    T[5] = [2.41, 0.0, 0.0]            # outside the box
    T[6, 1] = np.nan                   # a NaN coordinate
    T[7] = [0.1, 0.2, 0.3]
    lnq[7] = np.inf                    # ln q = +inf
    T[8] = [0.3, 0.2, 0.1]
    lnq[8] = -np.inf
    T[9, 2] = np.inf
    gated = [5, 6, 7, 8, 9]
    inside[gated] = False
    rec, logw = g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True)
    dev = logw.cpu().numpy()
    assert np.all(np.isneginf(dev[gated])) and np.array_equal(np.isfinite(dev), inside)
    assert rec["cnt"] == inside.sum() and len(dev) == 65
    _check_record(rec, dev, T, rec["centre"])
    assert np.all(np.isfinite(rec["s1"])) and np.all(np.isfinite(rec["S"]))
    # without a box the row outside counts again
    rec2 = g.importance_pass(y, T, lnq=lnq, bounds=None)
    assert rec2["cnt"] == 65 - 4
    # all rows gated: the empty record
    rec3, lw3 = g.importance_pass(y, T, lnq=np.full(65, np.inf), bounds=bounds, return_logw=True)
    assert rec3["lmax"] == -np.inf and rec3["S0"] == 0.0 and rec3["S2"] == 0.0 and rec3["cnt"] == 0.0
    assert not np.any(rec3["s1"]) and not np.any(rec3["S"]) and np.all(np.isneginf(lw3.cpu().numpy()))


def _bits(rec, logw):
    return (np.array([rec["lmax"], rec["S0"], rec["S2"], rec["cnt"]]).tobytes(), rec["s1"].tobytes(), rec["S"].tobytes(),
            logw.cpu().numpy().tobytes())


def test_lnq_none_is_lnq_of_zeros_and_two_calls_give_the_same_bits():
    g, X, y, T, lnq, bounds, lw, bud = _case(8, 513)
    a = _bits(*g.importance_pass(y, T, lnq=None, bounds=bounds, return_logw=True))
    b = _bits(*g.importance_pass(y, T, lnq=np.zeros(len(T)), bounds=bounds, return_logw=True))
    assert a == b
    c1 = _bits(*g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True))
    c2 = _bits(*g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True))
    assert c1 == c2 and c1 != a
    # the record does not depend on whether logw is asked for
    rec = g.importance_pass(y, T, lnq=lnq, bounds=bounds)
    assert _bits(rec, g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True)[1])[:3] == c1[:3]


@pytest.mark.parametrize("D,N", [(3, 513), (32, 512)])
def test_mu_agrees_with_predict_mean(D, N):
    """apgp_predict_mean sums the training rows in another order: the two agree to the budget, not to the bit."""
    import torch
    g, X, y, T, lnq, bounds, lw, bud = _case(D, N)
    _, logw = g.importance_pass(y, T, lnq=None, bounds=None, return_logw=True)
    mu = g._mean_device(np.asarray(y), torch.from_numpy(np.ascontiguousarray(T)).to("cuda:0")).cpu().numpy()
    mine = logw.cpu().numpy()
    assert np.all(np.isfinite(mine))
    assert np.all(np.abs(mine - mu) <= 2.0 * bud)


@pytest.mark.parametrize("order", [1, 2])
def test_linear_term_kernel(order):
    g, X, y, T, lnq, bounds, lw, bud = _case(3, 512, order)
    assert g._kernel_struct().lin_coef > 0.0 and g._kernel_struct().lin_order == order
    rec, logw = g.importance_pass(y, T, lnq=lnq, bounds=bounds, return_logw=True)
    dev = logw.cpu().numpy()
    print("lin_order %d: largest |logw - truth| / budget = %.3f" % (order, _check_logw(dev, lw, bud)))
    _check_record(rec, dev, T, rec["centre"])


def test_weights_spanning_1500_need_the_shift():
    """ln q from +750 to -750: exp(logw) itself would overflow at one end and underflow at the other."""
    g, X, y, T, lnq, bounds, lw, bud = _case(3, 5)
    wide = np.linspace(-750.0, 750.0, len(T))
    rec, logw = g.importance_pass(y, T, lnq=wide, bounds=None, return_logw=True)
    dev = logw.cpu().numpy()
    assert dev.max() - dev.min() > 1490.0 and np.all(np.isfinite(dev))
    assert np.isfinite(rec["S0"]) and 1.0 <= rec["S0"] < len(T) and rec["cnt"] == len(T)
    _check_record(rec, dev, T, rec["centre"])
    from approxposterior_amd import utility as ut
    s = ut.importanceSummary(rec, len(T))
    assert np.isfinite(s["logZ"]) and s["logZ"] > 700.0
