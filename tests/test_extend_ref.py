# -*- coding: utf-8 -*-
"""CPU tests of tests/extend_ref.py: on the inputs tests/test_gpu_factor_extend.py uses, the float64 restatement of the
appended-row chain (and SciPy's substitution) sits inside every bar -- without that the bars mean nothing -- and each
of its mutants breaks at least one.  Worst ratios are printed (pytest -s) and recorded in docs/experiments.md,
round 28."""
import math

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import extend_ref as er
import factor_ref as fr
import sweep_ref as sr


def chain_inputs(name):
    """(K, L0, Krows, kdiag, diag_add, n0) of a chain in float64 NumPy: the Gram of all n1 points, NumPy's factor of
    the first n0, the cross rows and the restated diagonals."""
    n0, n1, D, wn, P = er.CHAINS[name]
    X, _, metric, wn, P = er.chain_case(name)
    diag_add = math.exp(wn)
    K = er.host_kernel(X, X, metric, P)
    K = np.tril(K) + np.tril(K, -1).T
    kdiag = np.array([K[j, j] + diag_add for j in range(n0, n1)])
    L0 = np.linalg.cholesky(K[:n0, :n0] + diag_add * np.eye(n0))
    return K + diag_add * np.eye(n1), L0, [K[j, :j] for j in range(n0, n1)], kdiag, diag_add, n0


@pytest.fixture(scope="module")
def chains():
    return {name: chain_inputs(name) for name in er.CHAINS}


@pytest.mark.parametrize("name", sorted(er.CHAINS))
def test_restated_append_inside_every_bar(chains, name):
    A, L0, Krows, kdiag, diag_add, n0 = chains[name]
    L, info, _ = er.restate_append(L0, Krows, kdiag, diag_add)
    assert info == 0
    assert np.array_equal(L[:n0, :n0], L0) and np.all(np.triu(L, 1) == 0.0)
    wr, wp = er.judge_append(L, n0, Krows, kdiag)
    wc = fr.chol_ratio(A, L).max()
    # the same rows by LAPACK's substitution
    Ls = L.copy()
    for r, j in enumerate(range(n0, len(L))):
        Ls[j, :j] = solve_triangular(Ls[:j, :j], Krows[r], lower=True)
        Ls[j, j] = math.sqrt(kdiag[r] - Ls[j, :j] @ Ls[j, :j])
    sr_, sp = er.judge_append(Ls, n0, Krows, kdiag)
    sc = fr.chol_ratio(A, Ls).max()
    print("append %-8s restated: row %.3f pivot %.3f chol %.3f; scipy: row %.3f pivot %.3f chol %.3f"
          % (name, wr, wp, wc, sr_, sp, sc))
    assert max(wr, wp, wc) <= 1.0
    assert max(sr_, sp, sc) <= 1.0


@pytest.mark.parametrize("mutant", [m for m in er.MUTANTS if m != "info_last"])
@pytest.mark.parametrize("name", sorted(er.CHAINS))
def test_every_arithmetic_mutant_breaks_a_bar(chains, name, mutant):
    """Each mutant on each chain breaks a bar (the pivot bar is judged against the mutant's own row, as the GPU test
    judges the device's).  On the FIRST appended row, where no earlier wrong pivot has spread yet, the row bar catches
    the short solve and the pivot bar the missing diag_add and the stale sum; a dropped last term shows on whichever
    row's last entry is large enough (the last training point may be far from the new one)."""
    A, L0, Krows, kdiag, diag_add, n0 = chains[name]
    with np.errstate(all="ignore"):
        L, info, _ = er.restate_append(L0, Krows, kdiag, diag_add, mutant=mutant)
        wr, wp = er.judge_append(L, n0, Krows, kdiag)
        fr_, fp = er.judge_append(L[:n0 + 1, :n0 + 1], n0, Krows, kdiag)
    print("append %-8s mutant %-14s row %.3g pivot %.3g (first row: %.3g, %.3g)" % (name, mutant, wr, wp, fr_, fp))
    assert max(wr, wp) > 1.0
    if mutant == "cols_minus_1":
        assert fr_ > 1.0
    elif mutant != "drop_last_term":
        assert fr_ <= 1.0 and fp > 1.0


def test_failure_case_fails_exactly_and_info_keeps_the_first():
    """The store test's failure inputs: both copies of X[0] give an exactly zero pivot difference, the restatement
    reports the first (order n0 + 2), the "info_last" mutant the second (n0 + 4); the other rows stay inside the bars."""
    X, _ = er.failure_case()
    n0 = er.STORE_N + 1
    K = er.host_kernel(X, X, np.full(3, er.FAIL_METRIC))
    K = np.tril(K) + np.tril(K, -1).T
    L0 = np.linalg.cholesky(K[:n0, :n0])
    assert L0[0, 0] == 1.0 and np.array_equal(L0[:, 0], K[:n0, 0])
    Krows = [K[j, :j] for j in range(n0, n0 + 4)]
    kdiag = np.array([K[j, j] for j in range(n0, n0 + 4)])
    L, info, sums = er.restate_append(L0, Krows, kdiag)
    assert info == n0 + 2
    for r in (1, 3):
        row = L[n0 + r, :n0 + r]
        assert row[0] == 1.0 and not row[1:].any() and sums[r] == 1.0 and L[n0 + r, n0 + r] == 1.0
    for r in (0, 2):
        j = n0 + r
        assert er.row_ratio(L, L[j, :j], Krows[r]).max() <= 1.0
        assert er.pivot_ratio(L[j, j], kdiag[r], L[j, :j]) <= 1.0
    assert er.restate_append(L0, Krows, kdiag, mutant="info_last")[1] == n0 + 4


def test_append_diag_table_in_float64():
    """The table of apgp_append_diag alone, restated: successes inside the pivot bar, failures as the kernel's test
    ``d2 > 0 && d2 < inf`` decides them; the subnormal difference is exact and its root normal."""
    for name, kdiag, ss, info0, order, ok in er.APPEND_DIAG:
        d2 = kdiag - ss
        assert (d2 > 0.0 and d2 < np.inf) == ok, name
        if ok:
            r = er.pivot_ratio(math.sqrt(d2), kdiag, None, ss=ss)
            print("append_diag %-22s ratio %.3f" % (name, r))
            assert r <= 1.0
            # a pivot one part in 2^-50 off is outside
            assert er.pivot_ratio(math.sqrt(d2) * (1.0 + 2.0 ** -50), kdiag, None, ss=ss) > 1.0
    name, kdiag, ss = er.APPEND_DIAG[5][:3]
    assert 0.0 < kdiag - ss < er.TINY and math.sqrt(kdiag - ss) > er.TINY


@pytest.mark.parametrize("n", er.SUMMARY_N)
def test_summary_in_float64_inside_the_bounds(n):
    """NumPy's own sums of log L_ii and z.z (pairwise, float64) inside ``summary_bounds``; a dropped last diagonal entry,
    a log-determinant without its factor 2 and a z.z without its last term outside."""
    L, z = er.summary_case(n)
    b = er.summary_bounds(L, z, info=37)
    dg = np.diag(L)
    out = np.array([2.0 * np.log(dg).sum(), dg.min(), dg.max(), float(z @ z), 37.0])
    r = er.summary_ratios(out, b)
    print("summary n=%-4d numpy: logdet %.3f zz %.3f" % (n, r["logdet"], r["zz"]))
    assert r["logdet"] <= 1.0 and r["zz"] <= 1.0 and r["exact"]
    bad = out.copy(); bad[0] = 2.0 * np.log(dg[:-1]).sum()
    assert er.summary_ratios(bad, b)["logdet"] > 1.0
    bad = out.copy(); bad[0] = np.log(dg).sum()
    assert er.summary_ratios(bad, b)["logdet"] > 1.0
    bad = out.copy(); bad[3] = float(z[:-1] @ z[:-1])
    assert er.summary_ratios(bad, b)["zz"] > 1.0
    bad = out.copy(); bad[1] = np.nextafter(out[1], 0.0)
    assert not er.summary_ratios(bad, b)["exact"]
    assert er.summary_bounds(L)["zz"] == (0, 0.0)


@pytest.mark.parametrize("n0", er.W_N0)
def test_w_route_row_by_restated_product_inside_the_bar(n0):
    """The W route on a float64 inverse of NumPy's factor: sweep_ref.winv_restate's row inside ``winv_row_ratio``, its
    "drop_last_row" mutant outside."""
    X = er.points(n0 + 2, 3, 6000 + n0)
    K = er.host_kernel(X, X, np.full(3, 3.0)) + 1e-6 * np.eye(n0 + 2)
    L0 = np.linalg.cholesky(K[:n0, :n0])
    W = np.tril(solve_triangular(L0, np.eye(n0), lower=True))
    k = K[n0, :n0]
    l = sr.winv_restate(W, k, 0.0, 0)
    r = er.winv_row_ratio(sr.winv_panel(W), l, k).max()
    print("W route n0=%-3d restated product / bar %.3f" % (n0, r))
    assert r <= 1.0
    assert er.winv_row_ratio(sr.winv_panel(W), sr.winv_restate(W, k, 0.0, 0, mutant="drop_last_row"), k).max() > 1.0
