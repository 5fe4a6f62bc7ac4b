# -*- coding: utf-8 -*-
"""
:py:mod:`utility.py` - acquisition functions, scalar and batched
----------------------------------------------------------------

Mirror of the reference's ``approxposterior/utility.py`` (``logsubexp`` :69-89,
``AGPUtility`` :99-142, ``BAPEUtility`` :145-189, ``JonesUtility`` :192-250,
``minimizeObjective`` :253-372, ``klNumerical`` :26-65) with identical names, argument order and
sentinel values, plus the batched counterpart the reference lacks:
:func:`sweepObjective` evaluates a utility over a whole candidate matrix in one
fused HIP sweep (predict + variance + utility + arg-min) instead of one
``cho_solve`` per Nelder-Mead step.

The scalar functions call ``gp.predict`` on a single point -- with the
HIP-backed GP that is ``apgp_predict1_host`` (three small launches, 28-52 us per
call up to N = 4096); they keep the reference's default Nelder-Mead point search
(``minimizeObjective``) and polish a sweep winner.
"""

import numpy as np
from scipy.optimize import minimize
from scipy.stats import norm

__all__ = ["logsubexp", "AGPUtility", "BAPEUtility", "JonesUtility", "EIVUtility",
           "minimizeObjective", "sweepObjective", "utilityKind", "searchKind", "klNumerical",
           "mergeImportance", "importanceSummary", "importanceDrawsSummary",
           "importanceReplicatesSummary"]


def klNumerical(x, p, q):
    """Monte Carlo estimate of KL(p || q) from samples ``x`` drawn from p: the mean of
    log(p(x) / q(x)) over the samples (Hershey & Olsen 2007); ``p`` and ``q`` are density
    callables.  The estimate may come out negative for few samples."""
    try:
        res = np.sum(np.log(p(x) / q(x))) / len(x)
    except ValueError:
        raise ValueError("ERROR: inf/NaN encountered.  q(x) = 0 likely occured.")
    return res


def logsubexp(x1, x2):
    """log(exp(x1) - exp(x2)); -inf when x1 <= x2 (utility.py:69-89)."""
    if x1 <= x2:
        return -np.inf
    return x1 + np.log(1.0 - np.exp(x2 - x1))


def _predict_one(theta, y, gp):
    if not gp.computed:
        raise RuntimeError("ERROR: Need to compute GP before using it!")
    return gp.predict(y, np.asarray(theta, dtype=float).reshape(1, -1), return_var=True)


def AGPUtility(theta, y, gp, priorFn):
    """Negative AGP utility -(mu + 0.5 log(2 pi e var)) (Wang & Li 2017);
    +inf where the prior is not finite (utility.py:99-142)."""
    if not np.isfinite(priorFn(theta)):
        return np.inf
    mu, var = _predict_one(theta, y, gp)
    return -(mu + 0.5 * np.log(2.0 * np.pi * np.e * var))


def BAPEUtility(theta, y, gp, priorFn):
    """Negative log BAPE utility -((2 mu + var) + log(exp(var) - 1))
    (Kandasamy et al. 2015); +inf outside the prior (utility.py:145-189)."""
    if not np.isfinite(priorFn(theta)):
        return np.inf
    mu, var = _predict_one(theta, y, gp)
    return -((2.0 * mu + var) + logsubexp(var, 0.0))


def JonesUtility(theta, y, gp, priorFn, zeta=0.01):
    """Negative expected improvement (Jones et al. 1998) with exploration
    ``zeta``; 0.0 when the predictive std is not positive (utility.py:192-250)."""
    if not np.isfinite(priorFn(theta)):
        return np.inf
    mu, var = _predict_one(theta, y, gp)
    std = np.sqrt(var)
    yBest = np.max(y)
    if not (std > 0):
        return 0.0
    z = (mu - yBest - zeta) / std
    return -((mu - yBest - zeta) * norm.cdf(z) + std * norm.pdf(z))


def EIVUtility(theta, y, gp, priorFn, refs, logWeights):
    """The expected integrated variance of the posterior estimate exp(f) after one more evaluation at ``theta``
    (Jarvenpaa et al. 2021), reduced to what depends on theta: -log sum_j exp(a_j + cov(theta, r_j)^2 / (var(theta) +
    noise)) over the reference points ``refs`` (J, D) with log-weights ``logWeights`` (``GP.integration_weights``);
    +inf where the prior is not finite.  The scalar host form of ``GP.acquire_integrated``, from one
    ``gp.predict(..., return_cov=True)`` over [theta; refs]; hand ``refs`` and ``logWeights`` to
    :func:`minimizeObjective` through ``args``.  An integrated rule, not a pointwise one: it has no sweep kind."""
    if not np.isfinite(priorFn(theta)):
        return np.inf
    if not gp.computed:
        raise RuntimeError("ERROR: Need to compute GP before using it!")
    pts = np.vstack([np.asarray(theta, dtype=float).reshape(1, -1), np.asarray(refs, dtype=float)])
    _, cov = gp.predict(y, pts, return_cov=True)
    s = cov[0, 0] + gp._kernel_struct().diag_add
    if not (s > 0.0 and np.isfinite(s)):
        return np.inf
    e = np.asarray(logWeights, dtype=float) + cov[0, 1:] ** 2 / s
    mx = np.max(e)
    if not np.isfinite(mx):
        return -mx
    return -(mx + np.log(np.sum(np.exp(e - mx))))


_KINDS = {AGPUtility: "agp", BAPEUtility: "bape", JonesUtility: "jones"}
# minimizeObjective(jac=True): the objective kinds GP.predict_grad differentiates, the SciPy methods that take no gradient
_GRADIENT_KINDS = ("agp", "bape", "jones", "negmean")
_NO_GRADIENT_METHODS = ("nelder-mead", "powell", "cobyla", "cobyqa")


def utilityKind(fn):
    """'agp' | 'bape' | 'jones' for one of the utility functions (or its name)."""
    if isinstance(fn, str):
        k = fn.lower()
        if k not in ("agp", "bape", "jones"):
            raise ValueError("unknown utility %r" % fn)
        return k
    try:
        return _KINDS[fn]
    except KeyError:
        raise ValueError("the batched sweep supports AGPUtility, BAPEUtility and JonesUtility")


def searchKind(fn):
    """The objective kind of the device point search (:meth:`GP.nelder_mead_search`) for ``fn``: the
    utility's (:func:`utilityKind`), or the kind a function declares in its ``searchKind`` attribute
    (``ApproxPosterior.findMAP``'s minus-mean objective declares "negmean")."""
    declared = getattr(fn, "searchKind", None)
    if declared is not None:
        return str(declared).lower()
    return utilityKind(fn)


def minimizeObjective(fn, y, gp, sampleFn, priorFn, nRestarts=5,
                      method="nelder-mead", options=None, bounds=None,
                      theta0=None, args=None, maxIters=100, onDevice=False, jac=False):
    """Restarted scalar minimisation of a utility (utility.py:253-372).

    Same control flow as the reference: ``nRestarts`` SciPy runs from prior
    draws (or perturbed ``theta0``), each repeated from a fresh draw until the
    solution is finite and allowed by ``priorFn`` (at most ``maxIters`` times),
    and the best of them returned as ``(theta, value)``.  Differences forced by
    current SciPy (quirks Q1/Q2): the start point is flattened and the objective
    is cast to float.

    ``onDevice=True`` (Nelder-Mead only) runs the restarts on the device
    (:meth:`GP.nelder_mead_search`, the same simplex arithmetic as SciPy) over
    the objective :func:`searchKind` names, gated by ``bounds`` -- the box (or
    the support) the prior is assumed to be: the device evaluates the utility
    there and +inf outside, it does not call ``priorFn``.  The solutions are
    checked on the host with ``priorFn`` as above and ``value`` is ``fn`` at the
    best one.  All ``nRestarts`` starts are drawn first, in restart order, and
    searched in one launch; the restarts whose solution is refused are then
    redrawn in restart order and searched together, again until ``maxIters``
    redraws of one restart raise the same ``RuntimeError``.  Without a redraw
    NumPy's random stream is consumed exactly as by the host path; with
    redraws the draws come in another order than the host path's (which
    redraws a restart before it starts the next one).

    ``jac=True`` (gradient methods: "l-bfgs-b", "tnc", "bfgs", ...) hands SciPy
    the objective with its exact gradient, ``(u, du)`` of one
    ``gp.predict_grad(y, x, kind=searchKind(fn))`` call per evaluation, instead
    of letting it difference D + 1 ``predict`` calls; +inf with a zero gradient
    where ``priorFn`` is not finite.  Restarts, redraws, the bounds rule and
    the return value (``fn`` at the best solution) are those of ``jac=False``.
    Jones takes ``zeta`` from ``args[3]`` when given.  ``ValueError`` with a
    method that takes no gradient, with ``onDevice=True`` or for a ``fn``
    :func:`searchKind` cannot name.
    """
    if jac:
        if str(method).strip().lower() in _NO_GRADIENT_METHODS:
            raise ValueError("jac=True needs a gradient method (l-bfgs-b, tnc, bfgs, ...), not %r" % (method,))
        if onDevice:
            raise ValueError("jac=True is the host search with exact gradients: not with onDevice=True")
        kind = searchKind(fn)
        if kind not in _GRADIENT_KINDS:
            raise ValueError("jac=True: no predictive gradient for the objective kind %r" % (kind,))
    if str(method).lower() == "nelder-mead" and options is None:
        options = {"adaptive": True}
    if onDevice:
        if str(method).lower() != "nelder-mead":
            raise ValueError("onDevice=True runs Nelder-Mead only, not %r" % (method,))
        return _minimizeOnDevice(fn, y, gp, sampleFn, priorFn, nRestarts, options, bounds, theta0,
                                 () if args is None else args, maxIters)
    # bounds are only forwarded for the two methods the reference allows
    # (its l-bfgs-b test carries a leading space, utility.py:311; kept)
    if str(method).lower() not in [" l-bfgs-b", "tnc"]:
        bounds = None
    if args is None:
        args = ()
    if theta0 is not None:
        theta0 = np.asarray(theta0).squeeze()
        ndim = max(theta0.ndim, 1)

    if jac:
        zeta = float(args[3]) if len(args) > 3 else 0.01

        def objective(x, *a):     # (u, du) from one device call
            x = np.ascontiguousarray(x, dtype=np.float64)
            if not np.isfinite(priorFn(x)):
                return np.inf, np.zeros_like(x)
            u, du = gp.predict_grad(y, x, kind=kind, zeta=zeta)[:2]
            return float(u[0]), np.array(du[0], dtype=np.float64)
    else:
        def objective(x, *a):
            return float(np.asarray(fn(x, *a), dtype=float).ravel()[0])

    res, vals = [], []
    for _ in range(nRestarts):
        if theta0 is None:
            t0 = np.asarray(sampleFn(1)).reshape(1, -1)
        else:
            t0 = theta0 + np.min(theta0) * 1.0e-3 * np.random.randn(ndim)
        tries = 0
        while True:
            if tries >= maxIters:
                raise RuntimeError("ERROR: Cannot find a valid solution. Current iterations: %d\n"
                                   "Maximum iterations: %d\n" % (tries, maxIters))
            sol = minimize(objective, np.asarray(t0, dtype=float).ravel(), args=args,
                           bounds=bounds, method=method, options=options, **({"jac": True} if jac else {}))["x"]
            if np.all(np.isfinite(sol)) and np.isfinite(priorFn(sol)):
                res.append(sol)
                vals.append(fn(sol, *args))
                break
            t0 = np.array(sampleFn(1)).reshape(1, -1)
            tries += 1
    best = int(np.argmin([float(np.asarray(v, dtype=float).ravel()[0]) for v in vals]))
    return np.array(res)[best], vals[best]


def _minimizeOnDevice(fn, y, gp, sampleFn, priorFn, nRestarts, options, gate, theta0, args, maxIters):
    """The ``onDevice`` branch of :func:`minimizeObjective`."""
    kind = searchKind(fn)
    if theta0 is not None:
        theta0 = np.asarray(theta0).squeeze()
        ndim = max(theta0.ndim, 1)
    starts = []
    for _ in range(nRestarts):
        if theta0 is None:
            t0 = np.asarray(sampleFn(1)).reshape(1, -1)
        else:
            t0 = theta0 + np.min(theta0) * 1.0e-3 * np.random.randn(ndim)
        starts.append(np.asarray(t0, dtype=float).ravel())
    starts = np.array(starts)
    res = [None] * nRestarts
    tries = [0] * nRestarts
    pending = list(range(nRestarts))
    while pending:
        sols = gp.nelder_mead_search(y, starts[pending], kind, bounds=gate, options=options)[0]
        refused = []
        for i, sol in zip(pending, sols):
            if np.all(np.isfinite(sol)) and np.isfinite(priorFn(sol)):
                res[i] = sol
            else:
                refused.append(i)
        for i in refused:
            starts[i] = np.array(sampleFn(1), dtype=float).ravel()
            tries[i] += 1
            if tries[i] >= maxIters:
                raise RuntimeError("ERROR: Cannot find a valid solution. Current iterations: %d\n"
                                   "Maximum iterations: %d\n" % (tries[i], maxIters))
        pending = refused
    vals = [fn(sol, *args) for sol in res]
    best = int(np.argmin([float(np.asarray(v, dtype=float).ravel()[0]) for v in vals]))
    return np.array(res)[best], vals[best]


def sweepObjective(fn, y, gp, candidates, bounds=None, mask=None, zeta=0.01,
                   returnAll=False):
    """Batched counterpart of :func:`minimizeObjective`: evaluate utility ``fn``
    (AGP / BAPE / Jones) at every row of ``candidates`` (M, D) with one fused
    HIP sweep and return ``(thetaBest, uBest)`` -- or, with ``returnAll``,
    ``(thetaBest, uBest, u, mu, var)``.

    ``bounds`` is the box prior evaluated on the device; ``mask`` (M,) marks
    candidates an arbitrary host-side prior allows.  Pointwise the values equal
    the scalar utilities (same theta => same mu, var, u); ties resolve to the
    lowest candidate index and NaN utilities never win.
    """
    kind = utilityKind(fn)
    cands = gp.parse_samples(candidates) if not hasattr(candidates, "data_ptr") else candidates
    out = gp.acquire(y, cands, kind, bounds=bounds, mask=mask, zeta=zeta, return_all=returnAll)
    bi, bu = out[0], out[1]
    if bi < 0:
        raise RuntimeError("ERROR: Cannot find a valid solution: no candidate is allowed by the prior")
    if hasattr(cands, "data_ptr"):
        best = cands[bi].cpu().numpy()
    else:
        best = np.array(cands[bi])
    if returnAll:
        return best, bu, out[2], out[3], out[4]
    return best, bu


# ---------------------------------------------------------------------------------------------------------------------
# importance-sampling records (GP.importance_pass, ApproxPosterior.evidence)
# ---------------------------------------------------------------------------------------------------------------------
def mergeImportance(a, b):
    """The record of the rows of ``a`` and ``b`` together.  A record (``GP.importance_pass``) is a dict with ``lmax``
    (the largest log-weight, -inf for no admissible row), ``S0 = sum e``, ``S2 = sum e^2``, ``cnt``, ``s1 = sum e (t - c)``
    (D,), ``S = sum e (t - c)(t - c)^T`` (D, D) and the centre ``centre`` (D,), with ``e = exp(logw - lmax)``.  The merge
    works in log space: with ``l = max`` of the two ``lmax``, the zeroth and first moments and ``S`` of each side are
    rescaled by ``exp(lmax - l)`` and ``S2`` by ``exp(2 (lmax - l))`` -- one of the two factors is exactly 1 -- so records
    whose ``lmax`` lie hundreds apart merge without overflow.  Associative up to rounding; an empty record is the neutral
    element.  Both records must be taken about the same centre (``ValueError`` otherwise)."""
    ca, cb = np.asarray(a["centre"], dtype=float), np.asarray(b["centre"], dtype=float)
    if ca.shape != cb.shape or not np.array_equal(ca, cb):
        raise ValueError("mergeImportance: the two records are taken about different centres")
    la, lb = float(a["lmax"]), float(b["lmax"])
    l = max(la, lb)
    out = {"lmax": l, "centre": ca.copy(), "cnt": float(a["cnt"]) + float(b["cnt"])}
    fa = np.exp(la - l) if la > -np.inf else 0.0
    fb = np.exp(lb - l) if lb > -np.inf else 0.0
    out["S0"] = fa * float(a["S0"]) + fb * float(b["S0"])
    out["S2"] = (fa * fa) * float(a["S2"]) + (fb * fb) * float(b["S2"])
    out["s1"] = fa * np.asarray(a["s1"], dtype=float) + fb * np.asarray(b["s1"], dtype=float)
    out["S"] = fa * np.asarray(a["S"], dtype=float) + fb * np.asarray(b["S"], dtype=float)
    return out


def importanceSummary(record, m, logVolume=0.0):
    """What an importance-sampling record over ``m`` proposal draws says, as a dict:

    ``logZ``     ``lmax + log S0 - log m + logVolume``: the log of the mean weight.  ``logVolume`` is for weights taken
                 without a constant proposal density (``lnq=None`` under a uniform proposal: pass the log of the box volume)
    ``logZErr``  ``sqrt(max(m S2 / S0^2 - 1, 0) / m)``, the delta-method standard error of ``logZ``
    ``ess``      ``S0^2 / S2``, the effective sample size
    ``mean``     ``c + s1 / S0``
    ``cov``      ``S / S0 - (s1 / S0)(s1 / S0)^T``
    ``nInside``  ``cnt``, the rows with a finite weight

    A record with no admissible row gives ``logZ = -inf``, ``ess = 0`` and NaN for the rest.  ``logZErr`` is the sampling
    error GIVEN the draws' weight variance: a proposal with lighter tails than exp(mu) under-samples the rows that carry
    the weight, and ``logZErr`` comes out misleadingly small -- watch ``ess`` and widen the proposal."""
    m = float(m)
    c = np.asarray(record["centre"], dtype=float)
    S0, S2 = float(record["S0"]), float(record["S2"])
    if not S0 > 0.0:
        nan = np.full(c.shape, np.nan)
        return {"logZ": -np.inf, "logZErr": np.nan, "ess": 0.0, "mean": nan, "cov": np.full(c.shape * 2, np.nan),
                "nInside": int(record["cnt"])}
    d = np.asarray(record["s1"], dtype=float) / S0
    return {"logZ": float(record["lmax"]) + np.log(S0) - np.log(m) + float(logVolume),
            "logZErr": float(np.sqrt(max(m * S2 / (S0 * S0) - 1.0, 0.0) / m)),
            "ess": S0 * S0 / S2,
            "mean": c + d,
            "cov": np.asarray(record["S"], dtype=float) / S0 - np.outer(d, d),
            "nInside": int(record["cnt"])}


def importanceReplicatesSummary(records, n, logVolume=0.0):
    """What R >= 2 importance records say together when each is taken over the ``n`` rows of another independently
    scrambled replicate of a quasi-random sequence (``ApproxPosterior.evidence(qmc=R)``).  The pooled estimates are
    :func:`importanceSummary` of the records merged in order (:func:`mergeImportance`) over ``R n`` rows: ``logZ``,
    ``ess``, ``mean``, ``cov``, ``nInside``.  The rows of a replicate are not independent, so the error comes from the
    scatter of the replicates, which are:

    ``logZErr``         ``std(Z_r, ddof=1) / sqrt(R) / mean(Z_r)`` with ``Z_r = exp(logZ_r - max_r logZ_r)``: the relative
                        standard error of the mean of the replicates' evidences, i.e. the standard error of ``logZ``
    ``meanErr``         ``std(mean_r, ddof=1) / sqrt(R)`` per dimension, (D,)
    ``logZReplicates``  (R,), ``meanReplicates`` (R, D): :func:`importanceSummary` of every replicate
    ``logZErrIID``      the pooled record's delta-method figure, which takes the rows for independent draws and
                        over-states the error of a quasi-random estimate
    ``qmc``             R

    A replicate with no admissible row has ``logZ_r = -inf`` (``Z_r = 0``) and a NaN mean: it counts in ``logZErr`` and
    makes ``meanErr`` NaN.  With no admissible row at all ``logZErr`` is NaN.  The error bar is the scatter of R numbers:
    itself uncertain by about ``1 / sqrt(2 (R - 1))`` of its value, and blind -- like every importance estimate -- to
    mass the proposal never reaches."""
    records = list(records)
    R = len(records)
    if R < 2:
        raise ValueError("importanceReplicatesSummary needs at least two replicates: the error is their scatter")
    pooled = records[0]
    for r in records[1:]:
        pooled = mergeImportance(pooled, r)
    out = importanceSummary(pooled, R * float(n), logVolume=logVolume)
    per = [importanceSummary(r, n, logVolume=logVolume) for r in records]
    logZ = np.array([p["logZ"] for p in per], dtype=float)
    mean = np.array([p["mean"] for p in per], dtype=float)
    out["logZErrIID"] = out["logZErr"]
    top = logZ.max()
    if top > -np.inf:
        Z = np.exp(logZ - top)
        out["logZErr"] = float(np.std(Z, ddof=1) / np.sqrt(R) / np.mean(Z))
    else:
        out["logZErr"] = np.nan
    out["meanErr"] = np.std(mean, axis=0, ddof=1) / np.sqrt(R)
    out["logZReplicates"], out["meanReplicates"], out["qmc"] = logZ, mean, R
    return out


def importanceDrawsSummary(records, m, logVolume=0.0):
    """What the importance records of S posterior function draws (``GP.importance_paths``; one record per draw, all over
    the same ``m`` proposal rows) say about the surrogate's own uncertainty, as a dict:

    ``logZDraws``, ``essDraws``, ``meanDraws``, ``covDraws``  :func:`importanceSummary` of every draw: (S,), (S,), (S, D),
                          (S, D, D)
    ``logZSurrogateErr``  the standard deviation (ddof = 1) of ``logZDraws``: how far the evidence moves when the GP is
                          redrawn from its posterior; NaN for fewer than two draws
    ``meanSurrogateErr``  the same per dimension for ``meanDraws``, (D,)
    ``logZExpected``      ``logsumexp(logZDraws) - log S``: the log of the mean of the draws' evidences, i.e. the
                          evidence of the expected posterior ``exp(mu + sigma^2 / 2)``
    ``nEmptyDraws``       draws with ``S0 = 0`` (no admissible row): left out of the three aggregates

    The draws share the proposal rows, so the scatter is the surrogate's alone: the sampling error of the proposal is
    ``logZErr`` of the plug-in record.  A draw's ``ess`` collapses where the predictive variance is large under a
    narrow proposal; watch ``essDraws``."""
    records = list(records)
    if not records:
        raise ValueError("importanceDrawsSummary needs at least one record")
    per = [importanceSummary(r, m, logVolume=logVolume) for r in records]
    logZ = np.array([p["logZ"] for p in per], dtype=float)
    mean = np.array([p["mean"] for p in per], dtype=float)
    keep = np.array([float(r["S0"]) > 0.0 for r in records])
    lz, mk = logZ[keep], mean[keep]
    nan_d = np.full(mean.shape[1:], np.nan)
    if len(lz):
        top = lz.max()
        expected = float(top + np.log(np.sum(np.exp(lz - top))) - np.log(len(lz)))
    else:
        expected = -np.inf
    return {"logZDraws": logZ, "essDraws": np.array([p["ess"] for p in per], dtype=float), "meanDraws": mean,
            "covDraws": np.array([p["cov"] for p in per], dtype=float),
            "logZSurrogateErr": float(np.std(lz, ddof=1)) if len(lz) > 1 else np.nan,
            "meanSurrogateErr": np.std(mk, axis=0, ddof=1) if len(lz) > 1 else nan_d,
            "logZExpected": expected, "nEmptyDraws": int(np.sum(~keep))}
