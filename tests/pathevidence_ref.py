# -*- coding: utf-8 -*-
"""Reference of the evidence over posterior function draws (csrc/pathdraw.hip: apgp_path_importance; DESIGN.md "Evidence
over path draws").  Plain Python: no GPU, no library import.  It composes what exists:

    f_s(t)        tests/pathdraw_ref.py ``draws`` (every sum exactly rounded)
    logw_s(row)   f_s(t_row) - lnq[row] where every coordinate is finite and inside the box and f_s and lnq are finite,
                  -inf elsewhere (``gate`` / ``logw``)
    record s      tests/evidence_ref.py ``record`` of draw s's log-weights about the centre (``records``)

and restates the scratch formula of include/apgp.h (``work_len``).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import pathdraw_ref as pr  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble
PD_THREADS = 256           # candidates per workgroup of the first stage
IMP_BLOCK = 256            # APGP_IMP_BLOCK
IMP_MAX_BLOCKS = 2048      # APGP_IMP_MAX_BLOCKS: beyond IMP_BLOCK * IMP_MAX_BLOCKS rows the moments' workgroups loop
MAX_DIM = 32
ROW_CAP = IMP_BLOCK * IMP_MAX_BLOCKS


def work_len(m, ndraws):
    """apgp_path_importance_work_len: per draw the first stage's maxima, the log-weights, the draw's maximum and the
    moments' partial sums (sized for the largest record, 3 + 32 + 528 outputs per workgroup)."""
    if m < 1 or ndraws < 1:
        return 0
    if m > 1 << 40 or ndraws > pr.MAX_DRAWS:
        return -1
    nblk = (m + PD_THREADS - 1) // PD_THREADS
    nb = min((m + IMP_BLOCK - 1) // IMP_BLOCK, IMP_MAX_BLOCKS)
    return ndraws * (nblk + m + 1 + nb * (3 + MAX_DIM + MAX_DIM * (MAX_DIM + 1) // 2))


def gate(T, lnq=None, bounds=None):
    """(m,) bool: the rows whose coordinates are all finite and inside the box and whose ln q is finite."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    ok = np.all(np.isfinite(T), axis=1)
    if lnq is not None:
        ok &= np.isfinite(np.asarray(lnq, dtype=np.float64))
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        with np.errstate(invalid="ignore"):
            ok &= np.all((T >= b[:, 0]) & (T <= b[:, 1]), axis=1)
    return ok


def logw(F, T, lnq=None, bounds=None):
    """(S, m) log-weights of the draw values F (S, m; any float type) in F's precision: F - lnq where the row passes the
    gate and F is finite, -inf elsewhere."""
    F = np.asarray(F)
    ok = gate(T, lnq, bounds)[None, :] & np.isfinite(F.astype(np.float64))
    lq = np.zeros(F.shape[1]) if lnq is None else np.where(np.isfinite(lnq), lnq, 0.0)
    with np.errstate(invalid="ignore"):
        return np.where(ok, np.where(ok, F, 0.0) - lq.astype(F.dtype)[None, :], F.dtype.type(-np.inf))


def records(lw, T, centre):
    """One evidence_ref.record per draw."""
    return [er.record(row, T, centre) for row in lw]


def reference(T, X, V, Z, b, W, Wl, k, mean, lnq=None, bounds=None, centre=None):
    """(logw (S, m) float64 from the exactly rounded draws, records) of the whole pass."""
    F = pr.draws(T, X, V, Z, b, W, Wl, k, mean)
    lw = logw(F, T, lnq, bounds)
    c = np.zeros(k.ndim) if centre is None else np.asarray(centre, dtype=np.float64)
    return lw, records(lw, T, c)


def evidences(recs, m):
    """(S,) Z_s = mean_i exp(logw_s(i)) = exp(lmax) S0 / m of every record."""
    return np.array([np.exp(r["lmax"]) * r["S0"] / float(m) if r["S0"] > 0.0 else 0.0 for r in recs])


def moment_draws(seed, groups=8, size=32, m=256):
    """The identity test's draws: pathdraw_ref.moment_fixture(seed, m=m) and ``groups`` x ``size`` functions by
    pathdraw_ref.fast_draws.  Per group, from RandomState(100 + seed) in this order: the weights, size x (R + D); eps =
    sqrt(diag_add) x normals, size x n.  Returns (fixture, [(W, eps), ...], F (groups size, m))."""
    fx = pr.moment_fixture(seed, m=m)
    rs = np.random.RandomState(100 + seed)
    numbers, F = [], []
    for _ in range(groups):
        W = rs.standard_normal((size, fx["phiT"].shape[1]))
        eps = np.sqrt(fx["k"].diag_add) * rs.standard_normal((size, len(fx["y"])))
        numbers.append((W, eps))
        F.append(pr.fast_draws(fx["phiT"], fx["phiX"], fx["Kxt"], fx["solve"], fx["y"], fx["mean"], W, eps)[0])
    return fx, numbers, np.vstack(F)


def expected_evidence(fx):
    """(mean_i exp(mu_i + v_i / 2), mean_i exp(mu_i)) of the fixture: the evidence of the expected posterior under the
    surrogate with its features fixed, and the plug-in value."""
    mu = fx["mean"] + fx["Kxt"].T @ fx["solve"](fx["y"] - fx["mean"])
    v = pr.surrogate_variance(fx["phiT"], fx["phiX"], fx["Kxt"], fx["solve"], fx["k"].diag_add)
    return float(np.mean(np.exp(mu + 0.5 * v))), float(np.mean(np.exp(mu)))


def identity_scores(Zs, fx):
    """(|mean_s Z_s - expected| / se, |mean_s Z_s - plug-in| / se), se = std_s(Z_s) / sqrt(S)."""
    want, plug = expected_evidence(fx)
    se = np.std(Zs, ddof=1) / np.sqrt(len(Zs))
    return abs(np.mean(Zs) - want) / se, abs(np.mean(Zs) - plug) / se
