# -*- coding: utf-8 -*-
"""CPU: the pruned arg-min with two seed waves (tests/seed_waves_ref.py) finds the arg-min over all rows whatever the
size K of the first wave, and with K = 16 it is the one-wave restatement (tests/prune_ref.py) count for count.

Inputs as in tests/test_prune_ref.py: random mu, any var <= k(t,t) (zero, negative and NaN included), random gates and
exact duplicates across blocks.  Over K = 1, 4, 16 the test demands

  * the winner is argmin(u), lowest index among ties, with u's bits;
  * with K = 16 the seeds, the survivors and tau are those of prune_ref.pruned_argmin and no second wave runs;
  * for every K the seed blocks are the same 16 in the same order (the selection does not know about the waves), a
    skipped seed holds no row at or below tau, and tau is the same number for every K whenever the row that sets it lies
    in a block that is swept -- which it must, as that row's block has bmin <= tau <= tau_1."""
import zlib

import numpy as np
import pytest

import prune_ref as pr
import seed_waves_ref as sw
import test_prune_ref as tp
import util_ref

KINDS = tp.KINDS
FIRSTS = (1, 4, 16)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spread,ktt", [(300.0, 1.0), (1.0, 1.0), (1e-3, 1.0), (5.0, 40.0), (0.0, 2.5)])
def test_the_winner_does_not_depend_on_the_first_wave(kind, spread, ktt):
    rs = np.random.RandomState(zlib.crc32(repr(("waves", kind, spread, ktt)).encode()))
    for rep in range(6):
        m = int(rs.choice([63, 64 * 3 + 1, 64 * 40 + 1, 64 * 700 + 17]))
        mu, var, S, adm = tp._case(rs, m, spread, ktt, ties=20)
        ybest = float(rs.normal(0.0, max(spread, 1e-3)))
        zeta = float(rs.choice([0.01, 1.0, 1e6]))
        u = np.where(adm, util_ref.f64(kind, mu, var, zeta, ybest), np.inf)
        ok = adm & (u < np.inf)
        want = pr.argmin(u)
        one = pr.pruned_argmin(kind, mu, var, ktt, S, adm, 1000, 8, zeta, ybest)
        taus = []
        for k_first in FIRSTS:
            bi, bu, sd, sv, tau, bmin, nsecond = sw.pruned_argmin(kind, mu, var, ktt, S, adm, 1000, 8, zeta, ybest, k_first)
            assert bi == want and (want < 0 or np.float64(bu).view(np.uint64) == u[want].view(np.uint64)), (k_first, bi, want)
            assert list(sd) == list(one[2])
            assert 0 <= nsecond <= max(0, len(sd) - k_first)
            # a seed the second wave skipped holds no row at or below tau, ties included
            swept = np.zeros(len(bmin), dtype=bool)
            swept[sd[:k_first]] = True
            tau1 = sw._tau(u, pr.block_rows(sd[:k_first], m)) if k_first else np.inf
            for b in sd[k_first:]:
                swept[b] = bmin[b] <= tau1
            swept[sv] = True
            low = np.nonzero(ok & (u <= tau))[0]
            assert np.all(swept[low // pr.BLOCK])
            taus.append(tau)
            if k_first == 16:
                assert nsecond == 0 and list(sv) == list(one[3])
                assert np.float64(tau).view(np.uint64) == np.float64(one[4]).view(np.uint64)
        assert all(np.float64(t).view(np.uint64) == np.float64(taus[0]).view(np.uint64) for t in taus), taus


def test_a_second_wave_seed_wins():
    """The smallest bound sits on a row whose utility is poor (var = 0 at a large mu: the bound is far below u), so the
    first seed's tau_1 prunes nothing, and the winner lies in a seed of rank >= K: the second wave has to sweep it."""
    m = 64 * 40
    rs = np.random.RandomState(11)
    mu = rs.normal(0.0, 1.0, size=m)
    var = np.full(m, 0.9)
    S = np.abs(mu) * 2.0
    adm = np.ones(m, dtype=bool)
    for kind in KINDS:
        u = np.where(adm, util_ref.f64(kind, mu, var, 0.01, 0.0), np.inf)
        want = pr.argmin(u)
        for k_first in (1, 4):
            bi, bu, sd, sv, tau, bmin, nsecond = sw.pruned_argmin(kind, mu, var, 1.0, S, adm, 500, 4, 0.01, 0.0, k_first)
            assert bi == want
            rank = list(sd).index(want // pr.BLOCK) if want // pr.BLOCK in sd else -1
            if rank >= k_first:
                assert nsecond > 0


def test_nothing_admissible_and_infinite_tau_1():
    m = 64 * 20 + 5
    rs = np.random.RandomState(3)
    mu = rs.normal(size=m)
    S = np.abs(mu) * 3
    var = np.full(m, 0.5)
    none = np.zeros(m, dtype=bool)
    for k_first in FIRSTS:
        bi, bu, sd, sv, tau, bmin, nsecond = sw.pruned_argmin("agp", mu, var, 1.0, S, none, 300, 2, k_first=k_first)
        assert (bi, bu) == (-1, np.inf) and len(sd) == 0 and len(sv) == 0 and np.isposinf(tau) and nsecond == 0
    # the first wave finds nothing finite (AGP at var < 0 is NaN in its blocks): tau_1 = +inf, every other seed is swept
    bmin = pr.block_min(pr.row_bounds("agp", mu, 1.0, S, np.ones(m, dtype=bool), 300, 2))
    first = pr.seeds(bmin)[:4]
    var2 = var.copy()
    var2[pr.block_rows(first, m)] = -1.0
    adm = np.ones(m, dtype=bool)
    bi, bu, sd, sv, tau, bmin, nsecond = sw.pruned_argmin("agp", mu, var2, 1.0, S, adm, 300, 2, k_first=4)
    u = util_ref.f64("agp", mu, var2, 0.01, 0.0)
    assert list(sd[:4]) == list(first) and nsecond == len(sd) - 4 == 12 and bi == pr.argmin(u)
