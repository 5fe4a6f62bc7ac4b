# -*- coding: utf-8 -*-
"""High-precision reference of the three acquisition utilities and the forward-error bound of evaluating them in fp64
the way csrc/util_value.h writes them.  Plain Python (mpmath, NumPy, SciPy): no GPU, no library import.

The formulas are the reference's (utility.py:136 AGP; :183 BAPE with logsubexp :85-88; :229-244 Jones):

    AGP    u = -(mu + 1/2 log(2 pi e var))
    BAPE   u = -((2 mu + var) + var + log(1 - exp(-var)))
    Jones  u = -(imp Phi(z) + sd phi(z)),  sd = sqrt(var), imp = mu - ybest - zeta, z = imp / sd

``truth`` evaluates them with 60 digits and names the CLASS of the result as the reference's fp64 code produces it:

    AGP    var < 0 (or a NaN input) -> "nan";  var == 0 -> "+inf"
    BAPE   var <= 0, or exp(-var) rounding to 1.0 in fp64 -> "+inf";  a NaN input -> "nan"
    Jones  ``sqrt(var) > 0`` false (var <= 0 or NaN) -> "zero";  NaN mu with sd > 0 -> "nan"
    anything else -> "value"

``bound`` is a first-order bound of |fp64 result - truth| for the operation sequence of util_value.h, from per-function
budgets: exp and log 3 ulp, erfc 16 ulp (the OpenCL full-profile fp64 limits, which ROCm's device math library is built
to; SciPy/NumPy on the host are well inside them), sqrt / div / mul / add correctly rounded.  u = 2^-53, one ulp = 2u.
It is a formula of (mu, var, zeta, ybest) and those budgets only.  Term by term (everything in units of 2u):

  AGP    w = 2 pi e var carries three roundings (1.5), which log turns into an absolute 1.5; L = log(w) adds E_LOG |L|;
         halving is exact; the sum mu + L/2 and nothing else rounds once more: |mu| + |L|/2, and the starting form keeps
         a second |mu| + (1/2)|L| for slack  ->  2|mu| + (0.5 (E_LOG + 1) + 0.5)|L| + 1.5.
  BAPE   e = exp(-var) is off by E_EXP ulp, om = 1 - e by one more rounding: relative (2 E_EXP + 1) e / om in om -- the
         known 1 / var amplification of a one-ulp exp for small var -- which log passes on as an absolute error; lg =
         log(om) adds (E_LOG + 1)|lg|; the three sums 2 mu + var, var + lg and their total are each bounded by
         2|mu| + 2 var + |lg|  ->  3 (2|mu| + 2 var + |lg|) + (E_LOG + 1)|lg| + (2 E_EXP + 1) e / om + 1.
  Jones  z carries three roundings (imp twice, the division); d Phi / Phi = z' |z| phi / Phi and d phi / phi = z' z^2
         amplify them inside the Gaussian tail.  Phi: E_ERFC + the product by M_SQRT1_2, the halving (exact), the
         product with imp and the final sum  ->  |imp Phi| (E_ERFC + 4 + 3 |z| phi / Phi).  phi: E_EXP + squaring,
         the two constant products, the product with sd (whose sqrt rounds too) and the final sum, with the z^2
         amplification of z's three roundings and of the rounding of z z / 2  ->  sd phi (E_EXP + 5 + 4 z^2).
         imp = (mu - ybest) - zeta may cancel: its first difference rounds relative to |mu - ybest|, not to |imp|, an
         absolute u |mu - ybest| that the rest of the formula sees as a shifted input, and d u / d imp = -Phi exactly
         (the phi terms of the derivative cancel)  ->  + u Phi |mu - ybest|.  (Found on the device: a fantasy pick had
         raised ybest until mu - ybest ~ zeta; the starting form, without this term, was exceeded 6.5 times there.)
         Below the normal range the relative model ends: a subnormal result is rounded to a multiple of 2^-1074 and the
         budgets count in that spacing, so 2^-1074 ((E_ERFC + 1)|imp| + (E_EXP + 2) sd + 1) is added; and a function
         value below the smallest normal, 2^-1022, may come back flushed to zero (SciPy's erfc does that), so a term
         whose Phi or phi is below 2^-1022 is allowed to be missing altogether: |imp| Phi, sd phi are added for those.
         That is the class rule of an underflowed tail: the fp64 result is -0.0 or 0.0 or, at the edge of the
         underflow, something below 2^-1022 (|imp| + sd).

BAPE's class has an edge the budget decides: for 2^-55 < var <= (E_EXP + 1/2) ulp an exp inside its budget may or may
not return 1.0 (NumPy's returns 1 - 2^-53 at var = 2^-54, where the correctly rounded value is 1.0), so there
(``bape_edge``) +inf is accepted next to a value inside the bound.  At and below 2^-55 the result must be +inf: the
device has to reproduce the reference's formula, not a better one (log(-expm1(-var)) would be finite there)."""
import mpmath as mp
import numpy as np
from scipy.special import erfc

DPS = 60
U = 2.0 ** -53
E_EXP, E_LOG, E_ERFC = 3, 3, 16
KINDS = ("agp", "bape", "jones")
PDF_CONST = 0.3989422804014326779399461      # 1 / sqrt(2 pi) as util_value.h spells it


def f64(kind, mu, var, zeta=0.01, ybest=0.0):
    """The formulas in NumPy / SciPy fp64, operation by operation as util_value.h has them (element-wise)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "agp":
            return -(mu + 0.5 * np.log(2.0 * np.pi * np.e * var))
        if kind == "bape":
            lse = np.where(var <= 0.0, -np.inf, var + np.log(1.0 - np.exp(0.0 - var)))
            return -((2.0 * mu + var) + lse)
        sd = np.sqrt(var)
        imp = mu - ybest - zeta
        z = imp / sd
        cdf = 0.5 * erfc(-z * np.sqrt(0.5))
        pdf = np.exp(-0.5 * z * z) * PDF_CONST
        return np.where(sd > 0.0, -(imp * cdf + sd * pdf), 0.0)


def classify(kind, mu, var):
    """The class of one (mu, var) (Python floats): "value", "nan", "+inf" or "zero"."""
    mu, var = float(mu), float(var)
    if kind == "agp":
        if mu != mu or var != var or var < 0.0:
            return "nan"
        return "+inf" if var == 0.0 else "value"
    if kind == "bape":
        if var != var:
            return "nan"
        if var <= 0.0:
            return "+inf"
        if mu != mu:
            return "nan"
        # exp(-var) correctly rounded is 1.0 exactly when var <= 2^-54 (1 - var rounds to even at the midpoint)
        return "+inf" if var <= 2.0 ** -54 else "value"
    if not (var > 0.0):                 # sqrt(var) > 0 is false for var <= 0 and for NaN
        return "zero"
    return "nan" if mu != mu else "value"


def bape_edge(var):
    """True where exp(-var) may or may not come back as 1.0 from an exp inside its budget: both classes are the
    formula's own there.  Above: 1 - var is (E_EXP + 1/2) ulp from 1.0.  Below: an exp ends in a rounded addition
    1 + p, p ~ -var, which gives 1.0 for every p > -2^-54; at var <= 2^-55 no rounding of p reaches that, the result IS
    1.0 and +inf is required, as the reference gives it."""
    return 2.0 ** -55 < var <= (E_EXP + 0.5) * 2.0 * U


def _eval(kind, mu, var, zeta, ybest, cls=None):
    """(truth as mpf or None, bound as float or None, class); ``cls`` = "value" forces the value form."""
    cls = cls or classify(kind, mu, var)
    if cls != "value":
        return None, None, cls
    if not (np.isfinite(mu) and np.isfinite(var)):
        raise ValueError("truth/bound are defined for finite or NaN inputs")
    with mp.workdps(DPS):
        m, v = mp.mpf(float(mu)), mp.mpf(float(var))
        if kind == "agp":
            L = mp.log(2 * mp.pi * mp.e * v)
            t = -(m + L / 2)
            b = 2 * U * (2 * abs(m) + (0.5 * (E_LOG + 1) + 0.5) * abs(L) + 1.5)
        elif kind == "bape":
            e = mp.exp(-v)
            om = -mp.expm1(-v)
            lg = mp.log(om)
            t = -((2 * m + v) + v + lg)
            b = 2 * U * (3 * (2 * abs(m) + 2 * v + abs(lg)) + (E_LOG + 1) * abs(lg) + (2 * E_EXP + 1) * e / om + 1)
        else:
            sd = mp.sqrt(v)
            imp = m - mp.mpf(float(ybest)) - mp.mpf(float(zeta))
            z = imp / sd
            Phi, phi = mp.ncdf(z), mp.npdf(z)
            t = -(imp * Phi + sd * phi)
            b = 2 * U * (abs(imp * Phi) * (E_ERFC + 4 + 3 * abs(z) * phi / Phi) + sd * phi * (E_EXP + 5 + 4 * z * z))
            b += U * Phi * abs(m - mp.mpf(float(ybest)))
            b += mp.ldexp(1, -1074) * ((E_ERFC + 1) * abs(imp) + (E_EXP + 2) * sd + 1)
            tiny = mp.ldexp(1, -1022)
            if Phi < tiny:
                b += abs(imp) * Phi
            if phi < tiny:
                b += sd * phi
        return t, float(b), cls


def truth(kind, mu, var, zeta=0.01, ybest=0.0):
    """(value, class): value is an mpmath number with DPS digits for class "value", else None."""
    t, _, cls = _eval(kind, mu, var, zeta, ybest)
    return t, cls


def bound(kind, mu, var, zeta=0.01, ybest=0.0):
    """The forward-error bound (float) for class "value", else None."""
    return _eval(kind, mu, var, zeta, ybest)[1]


def jones_z(mu, var, zeta, ybest):
    """z of Jones in fp64 (for binning only)."""
    with np.errstate(all="ignore"):
        return (np.asarray(mu, dtype=np.float64) - ybest - zeta) / np.sqrt(np.asarray(var, dtype=np.float64))


def same_class(cls, u):
    """Does the fp64 result ``u`` have the non-value class ``cls``?"""
    u = float(u)
    if cls == "nan":
        return u != u
    if cls == "+inf":
        return u == np.inf
    if cls == "zero":
        return u == 0.0
    raise ValueError(cls)


def judge(kind, u, mu, var, zeta=0.01, ybest=0.0):
    """One result against the reference: ("value", err / bound) or (class, 0.0 if the class matches else inf).
    In BAPE's edge zone +inf is accepted next to a value inside the bound."""
    t, b, cls = _eval(kind, mu, var, zeta, ybest)
    u = float(u)
    if kind == "bape" and cls == "+inf" and bape_edge(float(var)) and np.isfinite(u):
        t, b, cls = _eval(kind, mu, var, zeta, ybest, cls="value")
    if cls != "value":
        return cls, (0.0 if same_class(cls, u) else np.inf)
    if kind == "bape" and u == np.inf and bape_edge(float(var)):
        return "+inf", 0.0
    if not np.isfinite(u):
        return "value", np.inf
    with mp.workdps(DPS):
        return "value", float(abs(mp.mpf(u) - t) / b)


def judge_all(kind, u, mu, var, zeta=0.01, ybest=0.0):
    """``judge`` over arrays: (classes as a list, ratios as an array).  Rows with the same (u, mu, var) bits are
    evaluated once."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    memo = {}
    classes, ratios = [], np.empty(len(u))
    keys = np.stack([u.view(np.int64), mu.view(np.int64), var.view(np.int64)], axis=1)
    for i in range(len(u)):
        k = keys[i].tobytes()
        r = memo.get(k)
        if r is None:
            r = memo[k] = judge(kind, u[i], mu[i], var[i], zeta, ybest)
        classes.append(r[0])
        ratios[i] = r[1]
    return classes, ratios
