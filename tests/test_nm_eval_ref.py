# -*- coding: utf-8 -*-
"""tests/nm_eval_ref.py against itself, against NumPy / SciPy and against its mutants (no GPU), on the cases of
tests/test_gpu_nm_eval_budget.py: the restated device order of FORM 1 and FORM 2 of apgp_nm_search and plain float64
evaluations of the same operations stay within the budgets; every mutant of the restated order exceeds a budget on at
least one case; and the conditions on the inputs that keep the budgets tight enough to mean something hold on every
case (the reference alone decides them)."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import kvalue_ref as kr
import nm_eval_ref as ne

FORMS = ("inverse", "solve")
ALL = [(form,) + c for form in FORMS for c in ne.cases(form)]
IDS = ["%s-n%d-D%d-P%s-%s" % c for c in ALL]


@pytest.mark.parametrize("form,n,D,order,family", ALL, ids=IDS)
def test_input_conditions(form, n, D, order, family):
    """Worst dq / q below 1e-9, k^ over at least six decades, cancellation in mu (sum |alpha||k^| >= 10 |mu|) on at
    least a tenth of the candidates."""
    _, _, tr = ne.truth(form, n, D, order, family)
    rel, decades, cancel = tr.guards()
    print("%s n=%d D=%d P=%s %s guards: worst dq / q %.3g, k^ spans %.1f decades, %d rows with sum|alpha||k^| >= 10 |mu|"
          % (form, n, D, order, family, rel, decades, cancel))
    assert rel < 1e-9
    assert decades >= 6.0
    assert 10 * cancel >= ne.BASE


@pytest.mark.parametrize("form,n,D,order,family", ALL, ids=IDS)
def test_restatement_and_numpy_within_budget(form, n, D, order, family):
    (X, alpha, T, k, mean), A, tr = ne.truth(form, n, D, order, family)
    kf = ne.kstar(T, X, k)
    rm, rv = tr.ratios(*ne.restate(A, X, alpha, T, k, mean, form, kf=kf))
    v = (np.tril(A) @ kf.T).T if form == "inverse" else solve_triangular(A, kf.T, lower=True).T
    nm, nv = tr.ratios(kf @ alpha + mean, tr.ktt.astype(np.float64) - (v * v).sum(1))
    print("%s n=%d D=%d P=%s %s: restated %.3f / %.3f, NumPy %.3f / %.3f of the mu / var budget"
          % (form, n, D, order, family, rm, rv, nm, nv))
    assert rm <= 1.0 and rv <= 1.0
    assert nm <= 1.0 and nv <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_every_mutant_exceeds_a_budget_somewhere(form):
    """Every mutant on every case of its form: the worst of its two ratios is above 1.0 on at least one, and a case on
    which it cannot act (no ragged block, no padded coordinate, one block) stays within budget."""
    worst = dict.fromkeys(ne.MUTANTS[form], 0.0)
    for (n, D, order, family) in ne.cases(form):
        (X, alpha, T, k, mean), A, tr = ne.truth(form, n, D, order, family)
        kf = ne.kstar(T, X, k)
        for name in ne.MUTANTS[form]:
            r = max(tr.ratios(*ne.restate(A, X, alpha, T, k, mean, form, mutant=name, kf=kf)))
            worst[name] = max(worst[name], r)
    print(form, {name: "%.3g" % r for name, r in worst.items()})
    for name, r in worst.items():
        assert r > 1.0, (form, name, r)


def test_a_mutant_of_the_other_form_changes_nothing():
    (X, alpha, T, k, mean), A, _ = ne.truth("inverse", 257, ne.D_N)
    base = ne.restate(A, X, alpha, T, k, mean, "inverse")
    for name in ("lost_part", "lb_col_shift", "q_skips_block", "stale_tail"):
        got = ne.restate(A, X, alpha, T, k, mean, "inverse", mutant=name)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


def test_counts():
    c = ne.counts(321)
    assert c["mu"] == 2 + 6 + 2 and c["q"] == 81 + 3 and c["q_solve"] == 6 + 6
    assert c["v"][0] == 1 + 6 and c["v"][63] == 1 + 6 and c["v"][64] == 2 + 6 and c["v"][320] == 6 + 6
    assert c["c"][0] == 5 and c["c"][63] == 68 and c["c"][64] == 16 + 5 and c["c"][320] == 80 + 5
    assert ne.ldw_of(257) == (258, 320) and ne.ldw_of(320) == (320,) and ne.ldw_of(513) == (514, 576)


def test_box_and_stale_state_cases():
    """The box leaves about a third of the candidates outside; the vertices of the stale-state simplex have the bits
    SciPy's first simplex has, differ from each other in k* by at least 1 % of the largest entry, and their restatement
    is within budget."""
    for form in FORMS:
        (X, alpha, T, k, mean), _, _ = ne.truth(form, ne.BOX_N[form], ne.D_N)
        lo, hi = ne.box_of(T)
        out = int(((T < lo) | (T > hi)).any(1).sum())
        assert ne.BASE // 4 <= out <= ne.BASE // 2
    X, alpha, V, k, mean, start = ne.stale_case()
    D = len(start)
    assert V.shape == (D + 1, D) and np.all(start != 0.0)
    for j in range(D):
        want = start.copy()
        want[j] = 1.05 * start[j]
        assert np.array_equal(V[j + 1], want)
    assert ne.vertex_spread(V, X, k) >= 0.01
    L, _ = ne.operand("solve", len(X))
    tr = ne.Truth(L, X, alpha, V, k, mean, form="solve")
    rm, rv = tr.ratios(*ne.restate(L, X, alpha, V, k, mean, "solve"))
    assert rm <= 1.0 and rv <= 1.0
    assert kr.dpad(D) == D                                       # (no padded coordinate in this case)
