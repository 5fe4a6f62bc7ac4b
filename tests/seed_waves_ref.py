# -*- coding: utf-8 -*-
"""NumPy restatement of the pruned arg-min with TWO seed waves (csrc/sweep.hip, launch_sweep_list).

tests/prune_ref.py sweeps all SEED seed blocks and takes tau from them.  Here the selection is the same SEED blocks in
the same order, but only the first K are swept at once:

  2a. first wave   the seeds at list positions [0, K); tau_1 = their smallest utility below +inf (+inf if none)
  2b. second wave  a seed at position >= K is swept if bmin <= tau_1 -- it could still win or tie; otherwise it is pruned
                   like any other block and its partial stays (+inf, -1)
  2c. tau          the minimum over the partials of all SEED seeds, that is over the swept ones
  3.  select       as before: bmin < +inf, bmin <= tau, not one of the SEED seeds

A skipped seed has bmin > tau_1 >= tau, so every one of its rows has u >= bmin > tau: it can neither win nor tie, and the
winner is argmin(u) for every K."""
import numpy as np

import prune_ref
import util_ref

SEED = prune_ref.SEED
FIRST = 4           # S2_SEED_FIRST: the rule's K


def _tau(u, rows):
    us = u[rows]
    fin = us[us < np.inf]
    return fin.min() if len(fin) else np.inf


def pruned_argmin(kind, mu, var, ktt, S, adm, n, dpad, zeta=0.01, ybest=0.0, k_first=FIRST, k=SEED):
    """Returns (index, u, seed blocks, surviving blocks, tau, bmin, second-wave seeds swept)."""
    m = len(mu)
    u = np.where(adm, util_ref.f64(kind, mu, var, zeta, ybest), np.inf)
    bmin = prune_ref.block_min(prune_ref.row_bounds(kind, mu, ktt, S, adm, n, dpad, zeta, ybest))
    sd = prune_ref.seeds(bmin, k)
    first, rest = sd[:k_first], sd[k_first:]
    tau1 = _tau(u, prune_ref.block_rows(first, m)) if len(first) else np.inf
    passed = np.asarray([b for b in rest if bmin[b] <= tau1], dtype=np.int64)
    swept = np.concatenate([first, passed]).astype(np.int64)
    rows = prune_ref.block_rows(swept, m)
    tau = _tau(u, rows)
    sv = prune_ref.select(bmin, tau, sd)
    rows = np.sort(np.concatenate([rows, prune_ref.block_rows(sv, m)]))
    i = prune_ref.argmin(u[rows])
    best = (-1, np.inf) if i < 0 else (int(rows[i]), float(u[rows[i]]))
    return best[0], best[1], sd, sv, tau, bmin, len(passed)
