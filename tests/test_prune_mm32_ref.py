# -*- coding: utf-8 -*-
"""The error budget of the matrix-core coarse bound (csrc/prune_mm32.h, "Error of mu32"), on the CPU: a NumPy replay
of the kernel's exponent chain and partial sums (tests/prune_mm32_ref.py) against the exact values.  For every
candidate |mu32 - mu| <= e32, and for every kernel value |exponent error| <= eta0.

Inputs on bench.synthetic_c3 with n <= 300: y scaled by 1 and 1e-4; training set and candidates shifted by +1e4; one
dimension with metric 1e-3 (the gate must fail, and the replay must say so); a candidate exactly on a training point
(k^ may exceed 1 by at most e^eta); candidates at the box corners; D = 1, 2, 3, 8."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import prune_mm32_ref as mm                      # noqa: E402

CASES = [("y*1", 1.0, 0.0, 8.0), ("y*1e-4", 1e-4, 0.0, 8.0), ("shift+1e4", 1.0, 1e4, 8.0), ("metric1e-3", 1.0, 0.0, 1e-3)]


def _inputs(n, D, scale, shift, metric0, m=200):
    import bench
    X, y = bench.synthetic_c3(n, D)
    y = y * scale
    metric = np.full(D, 8.0)
    metric[0] = metric0
    rs = np.random.RandomState(1)
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    T[m // 2] = X[min(7, n - 1)]                                      # on a training point
    corners = np.array(list(itertools.islice(itertools.product((-5.0, 5.0), repeat=D), 16)))
    T[:len(corners)] = corners                                        # box corners
    X = X + shift
    T = T + shift
    gpo, _ = bench.oracle_gp(X, y, metric, D)
    alpha = np.asarray(gpo._alpha if hasattr(gpo, "_alpha") else gpo.alpha, dtype=np.float64).ravel()
    return X, alpha, T, np.sqrt(0.5 / metric)


@pytest.mark.parametrize("name,scale,shift,metric0", CASES)
@pytest.mark.parametrize("n,D", [(1, 2), (33, 1), (130, 2), (300, 3), (300, 8)])
def test_budget(n, D, name, scale, shift, metric0):
    X, alpha, T, sc = _inputs(n, D, scale, shift, metric0)
    r = mm.replay(X, alpha, T, sc)
    tag = "n=%d D=%d %s" % (n, D, name)
    ok = r["gate"]
    with np.errstate(invalid="ignore", divide="ignore"):              # (n = 1: alpha = 0, the printed ratios are 0 / 0)
        ratios = ((r["exp_err"] / r["eta0"]).max(), (r["S32"] / r["sa"]).min(), (r["S32"] / r["sa"]).max())
    print("[%s] A <= %.3g, B = %.3g, eta <= %.3g, gate passes for %d of %d; exponent error / eta0 <= %.3g; "
          "|mu32 - mu| / e32 <= %.3g; S32 / sum|alpha| in [%.3g, %.3g]"
          % (tag, r["A"].max(), r["B"], r["eta"].max(), int(ok.sum()), len(ok),
             ratios[0], (np.abs(r["mu32"] - r["mu"])[ok] / r["e32"][ok]).max() if ok.any() else 0.0, ratios[1], ratios[2]))
    if name == "metric1e-3":
        # far wider than the length scale: the gate fails (n = 1: B = 0, it passes for the candidates next to the row)
        assert not ok.all() and (n == 1 or not ok.any()), tag
    else:
        assert ok.all(), tag
    # the exponent's bound holds whether or not the gate passes
    assert np.all(r["exp_err"] <= r["eta0"]), tag
    assert np.all(np.abs(r["mu32"] - r["mu"])[ok] <= r["e32"][ok]), tag
    # S32 bounds the exact sum of |alpha| k from above within the same relative budget, and k^ <= e^eta
    assert np.all(r["S"][ok] <= r["S32"][ok] * np.exp(r["eta"][ok])), tag
    assert np.all(r["khat_max"][ok] <= np.exp(r["eta"][ok]) * (1.0 + 4.0 * mm.U32)), tag


def test_chain_order_and_layout():
    """The order of the entries for the widths that are built, and that it is a permutation."""
    assert mm.entries(8) == [0, 5, 1, 6, 2, 7, 3, 8, 4, 9]
    assert mm.entries(2) == [0, 2, 1, 3]
    for dpad in (2, 4, 8):
        assert sorted(mm.entries(dpad)) == list(range(dpad + 2))


def test_slack_is_tighter_than_sum_alpha():
    """What the per-candidate sum buys: with sum|alpha| in the place of S32 the fp32 part would be far larger."""
    X, alpha, T, sc = _inputs(300, 8, 1.0, 0.0, 8.0)
    r = mm.replay(X, alpha, T, sc)
    assert np.median(r["S32"]) < 0.2 * r["sa"]
