# -*- coding: utf-8 -*-
"""CPU: the NumPy restatement of the device point search (tests/nm_ref.py) is SciPy's adaptive Nelder-Mead, bit for
bit, on objectives without ties -- the pin that lets the GPU replay (tests/test_gpu_nm_search.py) stand for SciPy."""
import os
import sys

import numpy as np
import pytest
from scipy.optimize import minimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nm_ref  # noqa: E402


def quadratic(x):
    w = np.arange(1, len(x) + 1, dtype=float)
    return float(np.sum(w * (x - 0.3 * w) ** 2)) + 0.125


def rosenbrock(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)) + 1e-3 * float(x[0])


CASES = [(D, f, seed) for D in (1, 2, 5, 8) for f in (quadratic, rosenbrock) for seed in (0, 1)]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _check(fn, x0, options):
    sp = minimize(fn, x0, method="nelder-mead", options=dict(options))
    mine = nm_ref.neldermead(fn, x0, **{k: v for k, v in options.items() if k != "adaptive"},
                             adaptive=options.get("adaptive", False))
    assert np.array_equal(_bits(mine["x"]), _bits(sp.x)), (mine["x"], sp.x)
    assert np.array_equal(_bits(mine["fun"]), _bits(sp.fun)), (mine["fun"], sp.fun)
    assert mine["nfev"] == sp.nfev and mine["nit"] == sp.nit and mine["status"] == sp.status
    assert len(mine["points"]) == mine["nfev"]
    return mine


@pytest.mark.parametrize("D,fn,seed", CASES, ids=["D%d-%s-%d" % (D, f.__name__, s) for D, f, s in CASES])
def test_matches_scipy_adaptive(D, fn, seed):
    x0 = np.random.RandomState(seed).uniform(-2.0, 2.0, size=D)
    rec = _check(fn, x0, {"adaptive": True})
    assert len(rec["steps"]) in (rec["nit"] - 1, rec["nit"])


@pytest.mark.parametrize("D", [1, 2, 5, 8])
def test_zero_coordinate_start(D):
    x0 = np.random.RandomState(7).uniform(-1.5, 1.5, size=D)
    x0[0] = 0.0
    rec = _check(quadratic, x0, {"adaptive": True})
    assert rec["points"][1][0] == 0.00025


@pytest.mark.parametrize("D,maxfev", [(2, 17), (5, 40), (8, 23), (8, 9)])
def test_maxfev_stops_mid_iteration(D, maxfev):
    x0 = np.random.RandomState(3).uniform(-2.0, 2.0, size=D)
    rec = _check(rosenbrock, x0, {"adaptive": True, "maxfev": maxfev})
    assert rec["nfev"] == maxfev and rec["status"] == 1


def test_maxiter_and_tolerances():
    x0 = np.array([1.3, -0.7, 0.2])
    rec = _check(rosenbrock, x0, {"adaptive": True, "maxiter": 25})
    assert rec["status"] == 2 and rec["nit"] == 25
    _check(quadratic, x0, {"adaptive": True, "xatol": 1e-8, "fatol": 1e-10})
    _check(quadratic, x0, {"adaptive": False})


def test_every_step_kind_is_recorded():
    seen = set()
    for D, fn, seed in CASES:
        x0 = np.random.RandomState(seed).uniform(-2.0, 2.0, size=D)
        seen.update(nm_ref.neldermead(fn, x0)["steps"])
    assert {nm_ref.REFLECT, nm_ref.EXPAND, nm_ref.CONTRACT_IN} <= seen


def test_xbar_is_summed_in_row_order():
    # the device sums the simplex rows one after another: np.add.reduce over axis 0 does the same
    rs = np.random.RandomState(11)
    for D in (2, 5, 8, 17, 32):
        sim = rs.standard_normal((D, D)) * 10.0 ** rs.randint(-8, 8, size=(D, D))
        acc = sim[0].copy()
        for j in range(1, D):
            acc = acc + sim[j]
        assert np.array_equal(_bits(np.add.reduce(sim, 0)), _bits(acc))


def test_replay_refuses_a_different_point():
    x0 = np.array([0.4, -1.1])
    rec = nm_ref.neldermead(quadratic, x0)
    xs = np.array(rec["points"])
    again = nm_ref.replay(xs, rec["values"], x0)
    assert again["nfev"] == rec["nfev"] and again["steps"] == rec["steps"]
    xs[5, 1] = np.nextafter(xs[5, 1], np.inf)
    with pytest.raises(AssertionError):
        nm_ref.replay(xs, rec["values"], x0)
