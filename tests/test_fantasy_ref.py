# -*- coding: utf-8 -*-
"""tests/fantasy_ref.py's one-call reference of the fantasy pass against itself, NumPy, mpmath and its mutants (no GPU),
on the inputs tests/test_gpu_fantasy_budget.py runs on the device:

  * a plain float64 NumPy evaluation and both restatements of the device order (the candidate's scaling contracted into
    the subtraction or not) are within ``pass_budget`` of ``pass_truth`` on every case of the tables;
  * every mutant of the restated order exceeds the budget on the cases named for it (fantasy_ref.MUTANT_CASES): the
    budget is not vacuous;
  * ``pass_truth`` agrees with an evaluation at kvalue_ref.DPS digits to within its own stated error;
  * the recursion of ``fantasy_batch`` (``fantasy_step``), fed the same beta, follows ``pass_truth`` step by step."""
import mpmath as mp
import numpy as np
import pytest

import fantasy_ref as fr
import kvalue_ref as kr

_CTX = {}


def ctx(case):
    if case.name not in _CTX:
        inp = fr.pass_inputs(case)
        P = fr.Pass(inp["T"], inp["X"], inp["k"])
        args = fr.pass_args(inp)
        _CTX[case.name] = (inp, P, fr.pass_truth(*args, ctx=P), fr.pass_budget(*args, ctx=P))
    return _CTX[case.name]


def test_case_tables_are_the_issues():
    assert fr.PASS_N == (1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 512, 513)
    assert fr.PASS_M == (1, 255, 256, 257, 1000)
    assert fr.PASS_D == (1, 3, 5, 8, 9, 16, 17, 32)
    assert fr.PASS_J == (1, 2, 31)
    assert set(fr.PASS_LIN) == {(P, D) for P in (0, 1, 2) for D in (3, 8, 32)}
    assert {kr.dpad(D) for D in fr.PASS_D} == {2, 4, 8, 16, 32}
    assert set(m for m, _ in fr.MUTANT_CASES) == set(fr.PASS_MUTANTS)


@pytest.mark.parametrize("case", fr.ALL_CASES, ids=lambda c: c.name)
def test_inputs_are_valid_and_not_hollow(case):
    inp, P, (tC, tv), (bC, bv) = ctx(case)
    k = inp["k"]
    assert inp["var_in"][case.pick] + k.diag_add > 0.0
    assert inp["Cprev"].shape == (case.j - 1, case.m)
    assert np.all(inp["beta"] != 0.0) and len(inp["beta"]) == case.n
    assert len(P.Tu) == min(case.m, 131)
    if case.j > 1 and case.m > 1:
        assert (inp["Cprev"] > 0).any() and (inp["Cprev"] < 0).any()
    if case.kind == "planted" and case.n >= 16:
        a = np.abs(inp["beta"])
        assert a.max() / a.min() >= 1e2
    # the bar is tight: a relative 1e-11 of the column's own scale at the very most
    scale = np.abs(tC).astype(np.float64).max()
    assert np.all(bC > 0.0) and np.all(bv > 0.0)
    assert bC.max() <= 1e-11 * max(scale, (P.akh @ np.abs(inp["beta"])).max() / np.sqrt(inp["var_in"][case.pick] + k.diag_add))
    if case.m >= 131 and case.kind == "planted":
        v = tv.astype(np.float64)
        assert (v > 0).any() and (v < 0).any()


@pytest.mark.parametrize("case", fr.ALL_CASES, ids=lambda c: c.name)
def test_numpy_is_within_the_budget(case):
    inp, P, (tC, tv), (bC, bv) = ctx(case)
    C, v = fr.pass_numpy(*fr.pass_args(inp))
    rC, rv = fr.ratio(C, tC, bC), fr.ratio(v, tv, bv)
    print("numpy %-12s worst |C - truth| / budget %.3f, |v - truth| / budget %.3f" % (case.name, rC, rv))
    assert rC <= 1.0 and rv <= 1.0


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", fr.ALL_CASES, ids=lambda c: c.name)
def test_restated_device_order_is_within_the_budget(case, fused):
    inp, P, (tC, tv), (bC, bv) = ctx(case)
    rows = fr.restate_rows(case)
    C, v = fr.pass_restate(*fr.pass_args(inp), rows=rows, fused=fused)
    rC, rv = fr.ratio(C, tC[rows], bC[rows]), fr.ratio(v, tv[rows], bv[rows])
    print("restate %-12s fused=%d %d rows: worst |C - truth| / budget %.3f, |v - truth| / budget %.3f"
          % (case.name, fused, len(rows), rC, rv))
    assert rC <= 1.0 and rv <= 1.0


@pytest.mark.parametrize("mutant,name", fr.MUTANT_CASES)
def test_mutant_exceeds_the_budget(mutant, name):
    case = fr.CASE_BY_NAME[name]
    inp, P, (tC, tv), (bC, bv) = ctx(case)
    rows = fr.restate_rows(case)
    C, v = fr.pass_restate(*fr.pass_args(inp), rows=rows, mutant=mutant, var_out0=inp["var_out0"])
    rC, rv = fr.ratio(C, tC[rows], bC[rows]), fr.ratio(v, tv[rows], bv[rows])
    over = int((np.abs(C.astype(fr.LD) - tC[rows]).astype(np.float64) > bC[rows]).sum())
    print("mutant %-17s on %-12s worst |C - truth| / budget %.3g (%d of %d rows over), |v - truth| / budget %.3g"
          % (mutant, name, rC, over, len(rows), rv))
    assert rC > 1.0, (mutant, name, "the budget does not catch this defect")
    assert rv > 1.0, (mutant, name, "the variance budget does not catch this defect")


def mp_pass(inp, row):
    k = inp["k"]
    T, X, beta, pick = inp["T"], inp["X"], inp["beta"], inp["pick"]
    with mp.workdps(kr.DPS):
        c = kr.truth1(T[row], T[pick], k)
        for r in range(len(X)):
            c -= kr.truth1(T[row], X[r], k) * mp.mpf(float(beta[r]))
        for i in range(len(inp["Cprev"])):
            c -= mp.mpf(float(inp["Cprev"][i, row])) * mp.mpf(float(inp["Cprev"][i, pick]))
        ch = c / mp.sqrt(mp.mpf(float(inp["var_in"][pick])) + mp.mpf(k.diag_add))
        return ch, mp.mpf(float(inp["var_in"][row])) - ch * ch


@pytest.mark.parametrize("name", ["n129-D8", "P2-D3", "j31", "realistic"])
def test_truth_agrees_with_mpmath(name):
    case = fr.CASE_BY_NAME[name]
    inp, P, (tC, tv), _ = ctx(case)
    eC, ev = P.truth_error(inp["beta"], inp["pick"], inp["Cprev"], inp["var_in"])
    for row in (0, case.pick, case.m - 1):
        ch, v = mp_pass(inp, row)
        with mp.workdps(kr.DPS):
            dC = float(abs(mp.mpf(tC[row].astype(np.float64).item()) + mp.mpf(float(tC[row] - tC[row].astype(np.float64))) - ch))
            dv = float(abs(mp.mpf(tv[row].astype(np.float64).item()) + mp.mpf(float(tv[row] - tv[row].astype(np.float64))) - v))
        print("truth %-10s row %-3d |ld - mp| %.3g (stated %.3g), v %.3g (stated %.3g)" % (name, row, dC, eC[row], dv, ev[row]))
        assert dC <= eC[row] and dv <= ev[row]


def test_fantasy_step_follows_the_truth_step_by_step():
    """Three steps of fantasy_batch's recursion in float64 with a planted beta per step: each step is judged against
    pass_truth computed from the recursion's own earlier columns and variance."""
    case = fr.CASE_BY_NAME["n129-D8"]
    inp = fr.pass_inputs(case)
    T, X, k = inp["T"], inp["X"], inp["k"]
    gp = {"amp": k.amp, "inv_metric": k.inv_metric, "lin_coef": k.lin_coef, "lin_order": k.lin_order, "diag_add": k.diag_add}
    P = fr.Pass(T, X, k)
    rs = np.random.RandomState(77)
    v = np.full(case.m, 4e4) * rs.uniform(1.0, 2.0, size=case.m)
    cols = []
    for step, b in enumerate((case.pick, 3, case.m - 1)):
        beta = fr.planted_beta(rs, case.n) / 100.0
        ch, vn = fr.fantasy_step(X, T, b, beta, cols, v, gp)
        Cprev = np.array(cols).reshape(len(cols), case.m)
        tC, tv = P.truth(beta, b, Cprev, v)
        bC, bv = P.budget(beta, b, Cprev, v)
        rC, rv = fr.ratio(ch, tC, bC), fr.ratio(vn, tv, bv)
        print("fantasy_step %d: worst |C - truth| / budget %.3f, |v - truth| / budget %.3f" % (step + 1, rC, rv))
        assert rC <= 1.0 and rv <= 1.0
        assert v[b] + k.diag_add > 0.0
        cols.append(ch)
        v = vn
