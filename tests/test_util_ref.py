# -*- coding: utf-8 -*-
"""Pins tests/util_ref.py -- the reference and bound the GPU utility tests judge the device with -- on the CPU.

1. The NumPy / SciPy evaluation of the formulas as util_value.h writes them lies within ``bound`` of ``truth`` on a seeded
   grid (sigma^2 1e-14 .. 1e3, |mu| 1e-3 / 1 / 1e3, Jones z in [-30, 8]; 700 points per utility): the bound holds for a
   library well inside the budgets, and is not vacuous -- the worst ratios are 0.24 (AGP), 0.22 (BAPE), 0.14 (Jones).
2. Planted defects of the kind the GPU test is there to find land OUTSIDE the bound (or in the wrong class) on a stated
   share of the same grid -- the evidence that the comparison has teeth, without mutating the library.
3. The class rules."""
import numpy as np
import pytest
from scipy.special import erfc

import util_ref as ur

YBEST, ZETA = 0.3, 0.01


def _grids():
    """700 (mu, var) per utility: 35 sigma^2 levels x 20 draws, one seeded stream through the three utilities."""
    rs = np.random.RandomState(0)
    out = {}
    for kind in ur.KINDS:
        pts = []
        for lv in np.linspace(-14, 3, 35):
            for _ in range(20):
                var = 10.0 ** (lv + rs.uniform(-0.2, 0.2))
                mu = rs.choice([1e-3, 1.0, 1e3]) * rs.normal()
                if kind == "jones":
                    mu = YBEST + ZETA + rs.uniform(-30, 8) * np.sqrt(var)
                pts.append((mu, var))
        out[kind] = np.array(pts)
    return out


GRIDS = _grids()


def grid(kind):
    return GRIDS[kind]


# var at and below the point where exp(-var) rounds to 1.0, <= 0, NaN rows: compared in class
CLASS_POINTS = np.array([(0.5, 1e-17), (0.5, 2e-17), (0.5, 5e-17), (-2.0, 1e-20), (1.0, 1e-300), (0.5, 0.0), (0.5, -0.0), (0.5, -1e-13),
                         (np.nan, np.nan), (3.0, -5.0)])


def ratios(kind, fn, pts):
    with np.errstate(all="ignore"):
        u = np.array([float(fn(np.float64(m), np.float64(v))) for m, v in pts])
    return ur.judge_all(kind, u, pts[:, 0], pts[:, 1], ZETA, YBEST)


@pytest.mark.parametrize("kind,expected", [("agp", 0.24), ("bape", 0.22), ("jones", 0.14)])
def test_numpy_evaluation_is_within_the_bound(kind, expected):
    pts = grid(kind)
    classes, r = ratios(kind, lambda m, v: ur.f64(kind, m, v, ZETA, YBEST), pts)
    assert set(classes) == {"value"}
    print("%s: worst NumPy err / bound = %.3f over %d points" % (kind, r.max(), len(r)))
    assert r.max() <= 1.0
    assert r.max() >= 0.02, "the bound is vacuous on this grid"
    # class points: NumPy produces the classes truth names
    classes, r = ratios(kind, lambda m, v: ur.f64(kind, m, v, ZETA, YBEST), CLASS_POINTS)
    assert np.all(r <= 1.0), list(zip(classes, r))


def _jones(m, v, const=ur.PDF_CONST, cdf_scale=1.0):
    sd = np.sqrt(v)
    if not sd > 0.0:
        return 0.0
    imp = m - YBEST - ZETA
    z = imp / sd
    cdf = 0.5 * erfc(-z * np.sqrt(0.5)) * cdf_scale
    return -(imp * cdf + sd * np.exp(-0.5 * z * z) * const)


DEFECTS = [
    # (utility, name, defective formula, least share of the grid + class points that must be judged wrong)
    ("jones", "1/sqrt(2 pi) truncated to 8 digits", lambda m, v: _jones(m, v, const=0.39894228), 0.85),
    ("jones", "erfc off by 1e-9", lambda m, v: _jones(m, v, cdf_scale=1.0 + 1e-9), 0.90),
    ("jones", "NaN / non-positive sigma^2 not sent to 0.0",
     lambda m, v: -((m - YBEST - ZETA) * 0.5 + np.sqrt(v) * ur.PDF_CONST) if not np.sqrt(v) > 0 else _jones(m, v), 0.005),
    ("agp", "log off by 1e-9 (relaxed math)",
     lambda m, v: -(m + 0.5 * np.log(2.0 * np.pi * np.e * v) * (1.0 + 1e-9)), 0.80),
    ("agp", "2 pi e truncated to 8 digits", lambda m, v: -(m + 0.5 * np.log(17.079468 * v)), 0.60),
    ("agp", "sigma^2 == 0 sent to NaN", lambda m, v: np.nan if v == 0 else -(m + 0.5 * np.log(2.0 * np.pi * np.e * v)), 0.002),
    ("bape", "exp off by 1e-9 (relaxed math)",
     lambda m, v: -((2.0 * m + v) + (v + np.log(1.0 - np.exp(-v) * (1.0 + 1e-9)))) if v > 0 else np.inf, 0.60),
    ("bape", "a wrong branch for small sigma^2: 2 log(sigma) below 1e-6",
     lambda m, v: (-((2.0 * m + v) + (v + (2.0 * np.log(np.sqrt(v)) if v < 1e-6 else np.log(1.0 - np.exp(-v)))))
                   if v > 0 else np.inf), 0.004),
    # log(-expm1(-v)) / log1p(-exp(-v)) in place of log(1 - exp(-v)): a BETTER formula.  On the value grid it cannot be
    # told from the formula as written -- the bound carries the 1 / sigma^2 amplification of exp's rounding, which is the
    # whole difference -- but it changes the class where exp(-sigma^2) rounds to 1.0: the device must give the
    # reference's +inf there, and a finite value is judged wrong (the four class points at or below 2^-55).
    ("bape", "log(-expm1(-v)) instead of log(1 - exp(-v))",
     lambda m, v: -((2.0 * m + v) + (v + np.log(-np.expm1(-v)))) if v > 0 else np.inf, 0.004),
]


@pytest.mark.parametrize("kind,name,fn,share", DEFECTS, ids=[d[1] for d in DEFECTS])
def test_planted_defect_lands_outside_the_bound(kind, name, fn, share):
    pts = np.concatenate([grid(kind), CLASS_POINTS])
    classes, r = ratios(kind, fn, pts)
    wrong = float(np.mean(r > 1.0))
    print("%s / %s: judged wrong on %.1f %% of %d points" % (kind, name, 100.0 * wrong, len(pts)))
    assert wrong >= share


def test_class_rules():
    assert ur.truth("agp", 1.0, -1e-9)[1] == "nan" and ur.truth("agp", 1.0, 0.0)[1] == "+inf"
    assert ur.truth("agp", np.nan, np.nan)[1] == "nan"
    assert ur.truth("bape", 1.0, 0.0)[1] == "+inf" and ur.truth("bape", 1.0, -3.0)[1] == "+inf"
    assert ur.truth("bape", 1.0, 2.0 ** -54)[1] == "+inf" and ur.truth("bape", 1.0, 2.0 ** -54 * (1 + 2.0 ** -52))[1] == "value"
    assert ur.truth("bape", np.nan, np.nan)[1] == "nan"
    for v in (0.0, -1.0, np.nan):
        assert ur.truth("jones", 1.0, v)[1] == "zero" and ur.truth("jones", np.nan, v)[1] == "zero"
    assert ur.truth("jones", np.nan, 1.0)[1] == "nan"
    # outside the edge zone NumPy's exp agrees with the class
    for v in (2.0 ** -55, 1e-17, 1e-300, 1e-15, 2.0 ** -50):
        assert not ur.bape_edge(v) and (np.exp(-v) == 1.0) == (ur.truth("bape", 0.0, v)[1] == "+inf")
    # BAPE's edge: either class is the formula's own for 2^-55 < var <= 3.5 ulp, nowhere else
    assert ur.judge("bape", ur.f64("bape", 0.5, 2.0 ** -54), 0.5, 2.0 ** -54)[1] <= 1.0
    assert ur.judge("bape", np.inf, 0.5, 2.0 ** -53)[1] == 0.0
    assert ur.judge("bape", np.inf, 0.5, 1e-15)[1] == np.inf
    assert ur.judge("bape", ur.f64("bape", 0.5, 2.0 ** -53), 0.5, 2.0 ** -53) == ("value", pytest.approx(0.0, abs=1.0))
    assert ur.judge("bape", 36.0, 0.5, 1e-17) == ("+inf", np.inf)     # finite at or below 2^-55: the wrong class
    # a wrong class is never accepted
    assert ur.judge("agp", 1.0, 0.5, -1.0)[1] == np.inf and ur.judge("jones", -1e-300, 0.5, -1.0)[1] == np.inf
    assert ur.judge("jones", -0.0, 0.5, -1.0)[1] == 0.0


def test_underflowed_jones_tail_is_zero_class():
    """zeta = 1e6: Phi and phi underflow; the fp64 result is +-0.0 and the bound there admits nothing above the
    subnormal range."""
    for var in (1e-12, 1.0, 900.0):
        u = float(ur.f64("jones", 0.3, var, 1e6, YBEST))
        assert u == 0.0
        assert ur.judge("jones", u, 0.3, var, 1e6, YBEST) == ("value", pytest.approx(0.0, abs=1e-9))
        assert ur.judge("jones", -1e-300, 0.3, var, 1e6, YBEST)[1] > 1.0
