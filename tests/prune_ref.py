# -*- coding: utf-8 -*-
"""NumPy restatement of the pruned arg-min of the sweep (csrc/sweep.hip, "Pruned arg-min"):

  1. bound      b_i = util(mu_i, k(t_i, t_i)) - slack_i for every admissible row (+inf otherwise; -inf if it is NaN),
                bmin[blk] = min over the 64 rows of candidate block blk
  2. seed       the SEED blocks with the smallest bmin (ties: lowest block number) are evaluated in full;
                tau = their smallest utility below +inf (+inf if there is none)
  3. select     survivors = blocks with bmin < +inf and bmin <= tau that are no seeds, ascending

and the arg-min over the seeds' and the survivors' rows, which must be the arg-min over all rows (lowest index among
equal utilities).  It rests on var_i <= k(t_i, t_i) and on the utilities not increasing with var at fixed mu.

``python tests/prune_ref.py`` prints the share of surviving blocks at the benchmark's shapes from the NumPy oracle
(mu for every candidate, the variance for the seed blocks only: minutes on a CPU)."""
import numpy as np

import util_ref

BLOCK = 64          # SW_CAND
SEED = 16           # PR_SEED
EPS = 2.0 ** -53


def slack(kind, b, mu, ktt, S, n, dpad, zeta=0.01, ybest=0.0):
    """prune_bound_kernel's slack, term by term (the derivation stands beside it in csrc/sweep.hip)."""
    mu = np.asarray(mu, dtype=np.float64)
    s = 2.0 * (4.0 * (n + 16) + 8.0 * dpad + 32.0) * EPS * np.asarray(S, dtype=np.float64) + \
        64.0 * EPS * (1.0 + np.abs(mu) + abs(ybest) + abs(zeta) + ktt + np.abs(b))
    if kind == "bape":
        with np.errstate(all="ignore"):
            s = s + 16.0 * EPS / (1.0 - np.exp(0.0 - np.asarray(ktt, dtype=np.float64)))
    return s


def row_bounds(kind, mu, ktt, S, adm, n, dpad, zeta=0.01, ybest=0.0):
    ktt = np.broadcast_to(np.asarray(ktt, dtype=np.float64), np.shape(mu))
    b = util_ref.f64(kind, mu, ktt, zeta, ybest)
    with np.errstate(all="ignore"):
        b = b - slack(kind, b, mu, ktt, S, n, dpad, zeta, ybest)
    b = np.where(np.isnan(b), -np.inf, b)
    return np.where(adm, b, np.inf)


def block_min(b):
    nblk = (len(b) + BLOCK - 1) // BLOCK
    pad = np.full(nblk * BLOCK, np.inf)
    pad[:len(b)] = b
    return pad.reshape(nblk, BLOCK).min(axis=1)


def seeds(bmin, k=SEED):
    order = np.lexsort((np.arange(len(bmin)), bmin))            # by value, then by block number
    order = order[bmin[order] < np.inf]
    return order[:k]


def select(bmin, tau, seed_blocks):
    keep = (bmin < np.inf) & (bmin <= tau)
    keep[np.asarray(seed_blocks, dtype=np.int64)] = False
    return np.nonzero(keep)[0]


def block_rows(blocks, m):
    rows = (np.asarray(blocks, dtype=np.int64)[:, None] * BLOCK + np.arange(BLOCK)[None, :]).ravel()
    return rows[rows < m]


def argmin(u):
    """The sweep's contract: NaN and +inf never win, ties go to the lowest index, -1 if nothing is admissible."""
    u = np.asarray(u, dtype=np.float64)
    ok = u < np.inf
    if not ok.any():
        return -1
    return int(np.nonzero(ok & (u == u[ok].min()))[0][0])


def pruned_argmin(kind, mu, var, ktt, S, adm, n, dpad, zeta=0.01, ybest=0.0, k=SEED):
    """Steps 1-3 on given per-row (mu, var): returns (index, u, seed blocks, surviving blocks, tau, bmin)."""
    m = len(mu)
    u = np.where(adm, util_ref.f64(kind, mu, var, zeta, ybest), np.inf)
    bmin = block_min(row_bounds(kind, mu, ktt, S, adm, n, dpad, zeta, ybest))
    sd = seeds(bmin, k)
    rows = block_rows(sd, m)
    us = u[rows]
    fin = us[us < np.inf]
    tau = fin.min() if len(fin) else np.inf
    sv = select(bmin, tau, sd)
    rows = np.sort(np.concatenate([rows, block_rows(sv, m)]))
    i = argmin(u[rows])
    best = (-1, np.inf) if i < 0 else (int(rows[i]), float(u[rows[i]]))
    return best[0], best[1], sd, sv, tau, bmin


def survivor_share(n, d, m, kind, metric=8.0, chunk=20000):
    """Seed and surviving blocks at one of the benchmark's shapes (bench.py's training set and candidates), from the
    NumPy oracle: mu and S for every row, the full prediction for the seed blocks only."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "oracle"))
    import bench
    X, y = bench.synthetic_c3(n, d)
    gpo, _ = bench.oracle_gp(X, y, metric, d)
    T = np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, d))
    alpha = np.asarray(gpo._alpha if hasattr(gpo, "_alpha") else gpo.alpha).ravel()
    mean = float(np.median(y))
    mu = np.empty(m)
    S = np.empty(m)
    x2 = (X * X).sum(1)
    for i in range(0, m, chunk):
        t = T[i:i + chunk]
        d2 = (t * t).sum(1)[:, None] + x2[None, :] - 2.0 * t @ X.T
        K = np.exp(-0.5 * np.maximum(d2, 0.0) / metric)
        mu[i:i + chunk] = K @ alpha + mean
        S[i:i + chunk] = K @ np.abs(alpha)
    adm = np.all(np.abs(T) <= 5.0, axis=1)
    dpad = 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32
    ybest = float(np.max(y))
    bmin = block_min(row_bounds(kind, mu, 1.0, S, adm, n, dpad, 0.01, ybest))
    sd = seeds(bmin)
    rows = block_rows(sd, m)
    mo, vo = gpo.predict(y, T[rows], return_var=True)
    us = np.where(adm[rows], util_ref.f64(kind, mo, vo, 0.01, ybest), np.inf)
    fin = us[us < np.inf]
    tau = fin.min() if len(fin) else np.inf
    sv = select(bmin, tau, sd)
    i = argmin(us)
    return {"n": n, "d": d, "m": m, "kind": kind, "blocks": len(bmin), "seeds": len(sd), "survivors": len(sv),
            "share": (len(sd) + len(sv)) / float(len(bmin)), "tau": float(tau),
            "seed_winner": int(rows[i]) if i >= 0 else -1, "mu_min": float(mu.min()), "mu_max": float(mu.max())}


if __name__ == "__main__":
    import json
    import sys
    shapes = {"C2": (1024, 2, 100000, "bape"), "C5": (1152, 8, 1000000, "agp"), "C3": (4096, 8, 1000000, "agp")}
    for name in (sys.argv[1:] or ["C2", "C5"]):
        print(name, json.dumps(survivor_share(*shapes[name])), flush=True)
