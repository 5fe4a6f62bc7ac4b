# -*- coding: utf-8 -*-
"""CPU tests of tests/factor_ref.py: the truth against mpmath, the reference implementations (LAPACK and the float64
restatements of the device order) inside every bar on every matrix family and size the GPU tests use -- without that
the bars mean nothing -- and every mutant outside one.  Worst ratios are printed (pytest -s) and recorded in
docs/experiments.md, round 11."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import factor_ref as fr


@pytest.mark.parametrize("decades", [12.0, 13.0])
def test_kinv_truth_against_mpmath(decades):
    """Two ragged tiles (n = 70), cond(K) = 1e12 and 1e13 (the family the GPU tests use): ``kinv_truth`` against a
    50-digit inverse of L L^T formed from the bits of L; <= 2^-9 ulp of a double relative to max |truth|."""
    bar = 2.0 ** -9
    import mpmath as mp
    n = 70
    K, _ = fr.ill_gram(n, decades)
    assert np.linalg.cond(K) >= 0.99 * 10.0 ** decades
    L = np.linalg.cholesky(K)
    T = fr.kinv_truth(L)
    with mp.workdps(50):
        Lm = mp.matrix(np.tril(L).tolist())
        Ki = mp.inverse(Lm * Lm.T)
        top = max(abs(Ki[i, j]) for i in range(n) for j in range(n))
        # (a long double converts to mpf exactly through its two double halves)
        worst = mp.mpf(0)
        for i in range(n):
            for j in range(n):
                hi = float(T[i, j])
                lo = float(T[i, j] - np.longdouble(hi))
                worst = max(worst, abs(mp.mpf(hi) + mp.mpf(lo) - Ki[i, j]))
        rel = float(worst / top)
    print("kinv_truth vs mpmath, n = 70, cond 1e%d: %.3g of max|truth| = %.3g ulp" % (decades, rel, rel / 2.0 ** -52))
    assert rel <= bar * 2.0 ** -52


@pytest.mark.parametrize("n", fr.POTRF_N)
def test_ill_family_is_ill_and_lapack_factors_it(n):
    K, _ = fr.ill_gram(n)
    L = np.linalg.cholesky(K)
    assert np.all(np.isfinite(L))
    if n >= 2:
        assert 1e12 <= np.linalg.cond(K) <= 1e14


@pytest.mark.parametrize("n", fr.POTRF_N)
@pytest.mark.parametrize("family", ["se", "ill"])
def test_cholesky_references_inside_the_bar(family, n):
    K, y = fr.gram(family, n)
    for name, L in (("lapack", np.linalg.cholesky(K)), ("restate", fr.chol_restate(K))):
        r = fr.chol_ratio(K, L).max()
        z = solve_triangular(L, y - 0.25, lower=True) if name == "lapack" else fr.trsv_restate(L, y, 0.25, 0)
        rz = fr.trsv_ratio(L, z, y, 0.25, 0).max()
        print("potrf %-3s n=%-3d %-7s chol ratio %.3f, rhs ratio %.3f" % (family, n, name, r, rz))
        assert r <= 1.0 and rz <= 1.0


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", fr.TRSV_N)
@pytest.mark.parametrize("family", ["planted", "ill"])
def test_substitution_references_inside_the_bar(family, n, trans):
    L, b = fr.factor(family, n)
    for name, x in (("lapack", solve_triangular(L, b - 0.125, lower=True, trans=trans)),
                    ("restate", fr.trsv_restate(L, b, 0.125, trans))):
        r = fr.trsv_ratio(L, x, b, 0.125, trans).max()
        t, bound = fr.sumsq_bound(x)
        es = abs(float(np.longdouble(float(x @ x)) - t))
        print("trsv %-7s n=%-3d trans=%d %-7s ratio %.3f, x.x err / bound %.3f" % (family, n, trans, name, r, es / bound))
        assert r <= 1.0 and es <= bound


@pytest.mark.parametrize("n", fr.KINV_N)
@pytest.mark.parametrize("family", ["planted", "ill"])
def test_kinv_restatement_inside_the_bar_and_the_contract(family, n):
    L, _ = fr.factor(family, n)
    sentinel = -1.25e300
    Y = fr.kinv_restate(L, sentinel=sentinel)
    low = fr.lower_tile_mask(n)
    assert np.all(Y[~low] == sentinel) and np.all(np.isfinite(Y[low]))
    r = fr.kinv_bar_ratio(Y, L)
    print("kinv %-7s n=%-3d restate: worst tile err / bar %.3f" % (family, n, r))
    assert r <= 1.0
    # a finite value left in the rows of X past n meets zeros of L only: not a bit changes
    assert np.array_equal(Y, fr.kinv_restate(L, sentinel=sentinel, stale=7.0))


@pytest.mark.parametrize("n", fr.KINV_N)
def test_syrk_reference_inside_the_bound(n):
    L, _ = fr.factor("planted", n)
    W = solve_triangular(L, np.eye(n), lower=True)
    T, B = fr.syrk_bound(W)
    low = fr.lower_tile_mask(n)
    err = np.abs((np.tril(W).T @ np.tril(W)).astype(np.longdouble) - T).astype(np.float64)
    assert np.all((B > 0) | (err == 0))
    r = (err[low] / B[low]).max()
    print("syrk n=%-3d numpy W^T W: worst err / bound %.3f" % (n, r))
    assert r <= 1.0


GRAD_GRID = [(n, D, None) for n in fr.GRAD_N for D in fr.GRAD_D] + [(n, D, P) for P, n, D in fr.GRAD_LIN]


@pytest.mark.parametrize("n,D,order", GRAD_GRID)
def test_gradient_restatement_inside_the_budget(n, D, order):
    X, alpha, Kinv, k = fr.grad_case(n, D, order)
    val, bud = fr.grad_record(X, alpha, Kinv, k)
    out = fr.grad_restate(X, alpha, Kinv, k)
    r = fr.grad_ratios(out, val, bud, D, order is not None)
    print("grad n=%-3d D=%-2d P=%-4s restate: %s" % (n, D, order, "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
    assert max(r.values()) <= 1.0


def test_gradient_record_counts_only_the_lower_tiles():
    """The record of a poisoned buffer (NaN above the block diagonal) is finite, and equals the plain full-matrix sum
    of the symmetrised Kinv."""
    n, D = 130, 3
    X, alpha, Kinv, k = fr.grad_case(n, D)
    val, _ = fr.grad_record(X, alpha, Kinv, k)
    S = np.where(fr.lower_tile_mask(n), Kinv, Kinv.T)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 * k.inv_metric)
    Kse = k.amp * np.exp(-0.5 * d2.sum(-1))
    A = np.outer(alpha, alpha) - S
    assert np.isclose(float(val["amp"]), 0.5 * (A * Kse).sum(), rtol=1e-9)
    for d in range(D):
        assert np.isclose(float(val["metric"][d]), 0.5 * (A * Kse * 0.5 * d2[:, :, d]).sum(), rtol=1e-9)
    assert np.isclose(float(val["trace"]), 0.5 * np.trace(A), rtol=1e-12)


# ----------------------------------------------------------------------------------------------------------------------
# mutants: each caught on a named family
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 193])
@pytest.mark.parametrize("mutant", fr.CHOL_MUTANTS)
def test_cholesky_mutants_are_caught(mutant, n):
    """Family "se" (the ill-conditioned family loses positive definiteness under most of them, which is caught as a
    NaN but says less).  n = 129: a ragged last block of one row; 193: two trailing block columns."""
    K, _ = fr.se_gram(n)
    assert fr.chol_ratio(K, fr.chol_restate(K)).max() <= 1.0
    r = fr.chol_ratio(K, fr.chol_restate(K, mutant)).max()
    print("cholesky mutant %-16s n=%d: worst ratio %.3g" % (mutant, n, r))
    assert r > 1.0


@pytest.mark.parametrize("family", ["planted", "ill"])
def test_kinv_mutants_are_caught(family):
    """n = 200 (four block rows, the last of eight rows).  pass 1 starting one block late is an error of order one;
    a row of X past n that pass 0 leaves non-zero reaches the result only if it is not finite (0 * NaN): the finite
    case is asserted harmless in test_kinv_restatement_inside_the_bar_and_the_contract."""
    L, _ = fr.factor(family, 200)
    for mutant in fr.KINV_MUTANTS:
        r = fr.kinv_bar_ratio(fr.kinv_restate(L, mutant), L)
        print("kinv mutant %-16s %-7s n=200: worst tile err / bar %.3g" % (mutant, family, r))
        assert r > 1.0


@pytest.mark.parametrize("mutant", fr.GRAD_MUTANTS)
def test_gradient_mutants_are_caught(mutant):
    """n = 130 (three tiles, the last of two rows), D = 3 (odd: the padded lane carries the last coordinate), a linear
    term of order 1; upper tiles NaN."""
    X, alpha, Kinv, k = fr.grad_case(130, 3, 1)
    val, bud = fr.grad_record(X, alpha, Kinv, k)
    assert max(fr.grad_ratios(fr.grad_restate(X, alpha, Kinv, k), val, bud, 3, True).values()) <= 1.0
    r = fr.grad_ratios(fr.grad_restate(X, alpha, Kinv, k, mutant), val, bud, 3, True)
    print("gradient mutant %-16s: %s" % (mutant, "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
    hit = {"weight1": ("amp", "metric", "lin"), "diag_twice": ("amp", "metric", "lin"), "skip_last_odd": ("amp", "metric"),
           "lin_sign": ("lin",), "transposed_read": ("amp", "metric", "lin")}[mutant]
    for name in hit:
        assert r[name] > 1.0, name
    # what the defect does not touch stays inside its budget
    for name in set(r) - set(hit):
        assert r[name] <= 1.0, name
