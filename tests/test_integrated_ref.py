# -*- coding: utf-8 -*-
"""tests/integrated_ref.py's reference of the integrated acquisition pass against itself, NumPy and its mutants (no GPU),
on the inputs tests/test_gpu_integrated.py runs on the device:

  * a plain float64 NumPy evaluation and the restatement of the device order are within ``budget`` of ``truth`` on the
    shared case table;
  * every mutant of the restated order exceeds the budget on the cases named for it: the budget is not vacuous;
  * the identity tau_j^2(t) = var(r_j) - var'(r_j) holds in long double, to the bar that NumPy's float64 re-conditioning
    itself achieves against long double on the same fixture (printed with -s; docs/experiments.md)."""
import numpy as np
import pytest

import integrated_ref as ir
import kvalue_ref as kr


def test_case_table_is_the_issues():
    assert ir.PASS_N == (1, 63, 64, 65, 511, 513)
    assert ir.PASS_M == (1, 255, 256, 257)
    assert ir.PASS_D == (1, 2, 3, 4, 8, 9, 16)
    assert {kr.dpad(D) for D in ir.PASS_D} == {2, 4, 8, 16}
    assert {P for P, _ in ir.PASS_LIN} == {1, 2}
    for w in ir.COLUMN_TILES:
        assert {w - 1, w, w + 1} <= set(ir.PASS_J)
    assert 1 in ir.PASS_J and max(ir.PASS_J) > 2 * max(ir.COLUMN_TILES)
    assert {15, 16, 17} <= set(ir.PASS_J_VECTOR) and max(ir.PASS_J_VECTOR) > 32
    assert ir.MAX_CASE.J == ir.MAX_REFS == 4096 and ir.MAX_CASE.m == ir.MAX_CASE.n == 64
    assert {mu for mu, _ in ir.MUTANT_CASES} == set(ir.MUTANTS)


def test_work_len():
    assert ir.work_len(0, 1) == 0
    assert ir.work_len(1, 1) == 2 and ir.work_len(256, 7) == 2 and ir.work_len(257, 4096) == 4
    assert ir.work_len(-1, 1) == -1 and ir.work_len((1 << 40) + 1, 1) == -1
    assert ir.work_len(5, 0) == -1 and ir.work_len(5, 4097) == -1


@pytest.mark.parametrize("case", ir.ALL_CASES, ids=lambda c: c.name)
def test_inputs_are_valid_and_not_hollow(case):
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    assert np.all(inp["B"] != 0.0) and inp["B"].shape == (case.n, case.J)
    assert np.all(inp["var"] + inp["k"].diag_add > 0.0)
    t2 = tau2.astype(np.float64).max(axis=1)
    if case.m >= 131:
        assert t2.max() >= 700.0 and t2.min() < 10.0            # the naive exp overflows on some rows
    if case.J > 1 and case.spread >= 1e3:
        assert inp["a"].max() - inp["a"].min() > 500.0
    assert np.all(bc > 0.0) and np.all(bu > 0.0) and np.all(np.isfinite(bu))
    # the bar is tight: relative 1e-10 of the column's own scale, and 1e-9 of |u| + 1 at the very most
    scale = np.abs(c).astype(np.float64).max() + (P.akh @ np.abs(inp["B"])).max()
    assert bc.max() <= 1e-10 * scale
    assert np.all(bu <= 1e-9 * (np.abs(u).astype(np.float64) + 1.0))


@pytest.mark.parametrize("case", ir.ALL_CASES, ids=lambda c: c.name)
def test_numpy_float64_is_within_budget(case):
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    gc, gu = ir.numpy_pass(*ir.args(inp))
    # NumPy's dot sums pairwise / blocked: no more roundings per summand than the chain the budget counts
    rc, ru = ir.ratio(gc, c, bc), ir.ratio(gu, u, bu)
    print("%s numpy c %.3f u %.3f" % (case.name, rc, ru))
    assert rc <= 1.0 and ru <= 1.0


@pytest.mark.parametrize("name", ir.RESTATE_CASES)
def test_restated_order_is_within_budget(name):
    case = ir.CASE_BY_NAME[name]
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    rows = ir.restate_rows(case)
    gc, gu = ir.restate(*ir.args(inp), rows=rows)
    rc, ru = ir.ratio(gc, c[rows], bc[rows]), ir.ratio(gu, u[rows], bu[rows])
    print("%s restate c %.3f u %.3f" % (name, rc, ru))
    assert rc <= 1.0 and ru <= 1.0


@pytest.mark.parametrize("mutant,name", ir.MUTANT_CASES)
def test_budget_catches_mutants(mutant, name):
    case = ir.CASE_BY_NAME[name]
    inp, P, (c, tau2, u), (bc, bu) = ir.context(case)
    rows = ir.restate_rows(case)
    gc, gu = ir.restate(*ir.args(inp), rows=rows, mutant=mutant)
    rc, ru = ir.ratio(gc, c[rows], bc[rows]), ir.ratio(gu, u[rows], bu[rows])
    print("%s %s c %.3g u %.3g" % (mutant, name, rc, ru))
    if mutant in ("no_diag_add", "no_a"):
        assert rc <= 1.0 and ru > 1.0                 # c does not see s or a
    else:
        assert rc > 1.0 and ru > 1.0


def test_minus_infinity_column_changes_no_bit():
    case = ir.CASE_BY_NAME["J17"]
    inp = ir.inputs(case)
    rows = [0, 7]
    a = np.array(inp["a"])
    a[5] = -np.inf
    _, u0 = ir.restate(inp["T"], inp["X"], inp["R"], inp["B"], a, inp["var"], inp["k"], rows=rows)
    keep = np.arange(case.J) != 5
    _, u1 = ir.restate(inp["T"], inp["X"], inp["R"][keep], inp["B"][:, keep], a[keep], inp["var"], inp["k"], rows=rows)
    assert u0.tobytes() == u1.tobytes()
    assert ir.ratio(u0, ir.Pass(inp["T"], inp["X"], inp["R"], inp["k"]).truth(inp["B"], a, inp["var"])[2][rows],
                    ir.Pass(inp["T"], inp["X"], inp["R"], inp["k"]).budget(inp["B"], a, inp["var"])[1][rows]) <= 1.0


def recondition_fixture():
    """A well-conditioned 2-D fixture: 30 training points, 12 reference points, 6 candidate points, noise 1e-2."""
    rs = np.random.RandomState(77)
    X = rs.uniform(-2.0, 2.0, size=(30, 2))
    R = rs.uniform(-2.0, 2.0, size=(12, 2))
    Ts = rs.uniform(-2.0, 2.0, size=(6, 2))
    return X, R, Ts, kr.kern([1.3, 0.7], amp=1.7, diag_add=1e-2)


def test_tau2_is_the_drop_of_the_reconditioned_variance():
    X, R, Ts, k = recondition_fixture()
    worst_ld = worst_64 = scale = 0.0
    for t in Ts:
        tau2, drop_ld, drop_64 = ir.recondition(X, R, t, k)
        worst_ld = max(worst_ld, float(np.abs(tau2 - drop_ld).max()))
        worst_64 = max(worst_64, float(np.abs(drop_64 - drop_ld.astype(np.float64)).max()))
        scale = max(scale, float(np.abs(tau2).max()))
    print("tau^2 identity: long double %.3g, float64 re-conditioning %.3g, largest tau^2 %.3g" % (worst_ld, worst_64, scale))
    assert scale > 1e-2 and worst_64 > 0.0
    assert worst_ld <= worst_64
