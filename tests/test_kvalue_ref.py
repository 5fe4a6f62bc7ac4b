# -*- coding: utf-8 -*-
"""CPU: the kernel-value reference (tests/kvalue_ref.py) against itself before a device is judged by it.

  * the exactly rounded fma agrees with mpmath's exact product and sum;
  * ``restate`` of apgp_exp alone is within E_EXP ulp of exp over the reduction boundaries, the clamp and random
    arguments (the worst value is printed and recorded in docs/experiments.md);
  * ``restate`` is within ``budget`` of the mpmath ``truth`` on every family;
  * the long-double truth agrees with the mpmath truth to 2^-9 ulp;
  * on the lattice the budget is at most 2.1 ulp: a loosened budget cannot hide;
  * every mutant of ``restate`` exceeds the budget on the family meant to catch it (the whole mutant x family table is
    printed, pytest -s, and recorded in docs/experiments.md).
"""
import math

import mpmath as mp
import numpy as np
import pytest

import kvalue_ref as kr


def _sub(n, gram, cap, seed=0, m=None):
    """At most ``cap`` seeded entries of an m x n (or lower-triangular n x n) index set, always with the corners."""
    if gram:
        idx = [(i, j) for i in range(n) for j in range(i + 1)]
    else:
        idx = [(i, j) for i in range(m) for j in range(n)]
    if len(idx) <= cap:
        return idx
    rs = np.random.RandomState(seed)
    keep = set(rs.choice(len(idx), size=cap, replace=False).tolist()) | {0, len(idx) - 1}
    return [idx[t] for t in sorted(keep)]


def _families():
    """name -> (X1, X2, kern, site, pairs): what the CPU test walks (every family of the module, tiny)."""
    fam = {}
    X, k = kr.lattice_1d()
    fam["lattice-1d"] = (X, None, k, "gram", _sub(len(X), True, 5000, 1))
    X, k = kr.lattice_1d(n=65, seed=3, log4=-2, amp=4.0, diag_add=2.0 ** -20)
    fam["lattice-1d-amp4"] = (X, None, k, "gram", None)
    E = kr.lattice_edges_points()
    fam["lattice-edges"] = (E, np.zeros((1, 1)), kr.kern([2.0]), "cross", None)
    fam["lattice-edges-pairs"] = (E[::7], None, kr.kern([2.0], amp=0.125), "gram", None)
    for D in (3, 5, 17):
        X, k = kr.lattice_nd(40 if D < 17 else 24, D, seed=D, amp=2.0, diag_add=0.5)
        fam["lattice-%dd" % D] = (X, None, k, "gram", None)
    for D, n in ((1, 65), (2, 65), (3, 65), (5, 40), (9, 40), (17, 30), (32, 24)):
        X, k = kr.general(n, D, seed=D)
        fam["general-%dd" % D] = (X, None, k, "gram", None)
    X, k = kr.general(20, 4, seed=77)
    fam["general-cross-4d"] = (X[:7], X[7:], k, "cross", None)
    X, k = kr.coincident(41, 3)
    fam["coincident-3d"] = (X, None, k, "gram", None)
    for P in kr.LIN_ORDERS:
        X, k = kr.linear(30, 3, P)
        fam["linear-P%d" % P] = (X, None, k, "gram", None)
    X, k = kr.linear(12, 17, 2, seed=9)
    fam["linear-P2-17d"] = (X[:4], X[4:], k, "cross", None)
    return fam


FAMILIES = _families()
LATTICE = [f for f in FAMILIES if f.startswith("lattice")]
# the family meant to catch each mutant
CATCHES = {"no_720": "lattice-1d", "no_ln2lo": "lattice-edges", "tab4": "lattice-1d", "skip_last_odd": "general-3d",
           "pad_nonzero": "general-5d", "transpose": "general-2d"}


def test_fma_is_exact():
    rs = np.random.RandomState(5)
    for _ in range(3000):
        a, b, c = (rs.uniform(-1, 1, 3) * 10.0 ** rs.uniform(-30, 30, 3)).tolist()
        assert kr.fma(a, b, c) == kr.fma_mp(a, b, c)
    # a product that cancels against the addend down to its last bits, and a tie
    a = 1.0 + 2.0 ** -30
    assert kr.fma(a, a, -1.0) == kr.fma_mp(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60
    assert kr.fma(2.0 ** -53, 1.0, 1.0) == 1.0 and kr.fma(3 * 2.0 ** -53, 1.0, 1.0) == 1.0 + 2.0 ** -51


def test_exp_restatement_within_e_exp():
    rs = np.random.RandomState(6)
    args = kr.exp_edge_arguments() + (-rs.uniform(0.0, 700.0, 4000)).tolist() + (-10.0 ** rs.uniform(-12, 0, 1000)).tolist()
    assert len(args) >= 10000
    worst, at = 0.0, None
    with mp.workdps(kr.DPS):
        for x in args:
            v = kr.exp_restate(x)
            t = mp.exp(mp.mpf(x))
            if x < -700.0:                                # the clamp: ~1e-304 for a smaller true value
                assert v == kr.exp_restate(-700.0) and 0.0 < v < 1e-304 and t < v
                continue
            e = float(abs(mp.mpf(v) - t)) / float(kr.ulp(float(t)))
            if e > worst:
                worst, at = e, x
    print("apgp_exp restated: worst %.4f ulp at x = %r over %d arguments" % (worst, at, len(args)))
    assert worst <= kr.E_EXP
    assert kr.exp_restate(0.0) == 1.0 and kr.exp_restate(-0.0) == 1.0
    assert kr.exp_restate(float("nan")) == kr.exp_restate(-700.0)        # the clamp swallows NaN


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_restate_within_budget_of_truth(name):
    X1, X2, k, site, pairs = FAMILIES[name]
    R = kr.restate(X1, X2, k, site=site, pairs=pairs)
    ratio, ulps = kr.err_over_budget(R, X1, X2, k, pairs=pairs, mp_truth=True)
    print("%-22s worst |err| / budget %.3f   worst |err| %.3f ulp" % (name, ratio, ulps))
    assert ratio <= 1.0
    if name in LATTICE:
        assert ulps <= 2.1


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_longdouble_truth_agrees_with_mpmath(name):
    X1, X2, k, site, pairs = FAMILIES[name]
    gram = X2 is None
    n = len(X1) if gram else len(X2)
    pairs = _sub(n, gram, 1500, 2, m=len(X1)) if pairs is None or len(pairs) > 1500 else pairs
    T = kr.truth_ld(X1, X2, k)
    t = kr.truth(X1, X2, k, pairs)
    worst = 0.0
    with mp.workdps(kr.DPS):
        for (i, j), v in t.items():
            mant, ex = np.frexp(T[i, j])                # (long double -> mpf exactly, below the doubles' range too)
            hi = float(mant)
            d = abs(mp.ldexp(mp.mpf(hi) + mp.mpf(float(mant - np.longdouble(hi))), int(ex)) - v)
            worst = max(worst, float(d) / float(kr.ulp(float(v))))
    print("%-22s long double against mpmath: %.2e ulp" % (name, worst))
    assert worst <= 2.0 ** -9


@pytest.mark.parametrize("name", LATTICE)
def test_lattice_budget_is_sharp(name):
    X1, X2, k, site, pairs = FAMILIES[name]
    B = kr.budget(X1, X2, k)
    T = kr.truth_ld(X1, X2, k).astype(np.float64)
    live = T > k.amp * 1e-304                            # (below: the clamp's floor, where an ulp means nothing)
    r = B[live] / kr.ulp(T[live])
    assert r.max() <= 2.1
    off = live & ~np.eye(*B.shape, dtype=bool) if X2 is None else live
    assert abs((B[off] / kr.ulp(T[off])).max() - (kr.E_EXP + 0.5)) < 0.05      # (E_EXP + 1/2) ulp, nothing else
    if X2 is None:
        i = np.arange(len(X1))
        assert (B[i, i] / kr.ulp(T[i, i])).max() <= 0.5 + 1e-9          # amp + diag_add: one rounding


def test_every_mutant_is_caught():
    table = {}
    for mut in kr.MUTANTS:
        for name in sorted(FAMILIES):
            X1, X2, k, site, pairs = FAMILIES[name]
            if pairs is not None and len(pairs) > 1200:
                pairs = pairs[::5]
            R = kr.restate(X1, X2, k, site=site, mutant=mut, pairs=pairs)
            table[mut, name] = kr.err_over_budget(R, X1, X2, k, pairs=pairs)[0]
    print("mutant x family: worst |err| / budget (caught where > 1)")
    for mut in kr.MUTANTS:
        print("  %-14s %s" % (mut, "  ".join("%s=%.3g" % (n, table[mut, n]) for n in sorted(FAMILIES) if table[mut, n] > 1.0)))
    for mut, name in CATCHES.items():
        assert table[mut, name] > 1.0, (mut, name, table[mut, name])
    # and the unmutated restatement is caught nowhere (test_restate_within_budget_of_truth), so the table is not noise
    assert set(CATCHES) == set(kr.MUTANTS)


def test_budget_has_the_cancellation_term():
    """Two points 1e6 length scales from the origin and a fraction of one apart: their xs round to 1e6 u each, which the
    budget must carry (a budget of rounding counts alone would not)."""
    k = kr.kern([0.7])
    X = np.array([[1.0e6 / math.sqrt(0.35)], [(1.0e6 + 1.5) / math.sqrt(0.35)]])
    B = kr.budget(X, None, k)
    T = kr.truth_ld(X, None, k).astype(np.float64)
    assert B[1, 0] > 1e5 * kr.ulp(T[1, 0])
    R = kr.restate(X, None, k)
    assert kr.err_over_budget(R, X, None, k, mp_truth=True)[0] <= 1.0
