# -*- coding: utf-8 -*-
"""CPU: the pruned arg-min (tests/prune_ref.py, the NumPy restatement of csrc/sweep.hip's bound / seed / select steps)
never prunes a row that wins or ties the winner.

Inputs are oracle-side values: random mu, any var <= k(t,t) (down to 0, negative and NaN included), random gates; the
utilities come from tests/util_ref.py.  For the three utilities the test demands, row by row,

    b_i - slack_i <= u_i            (the monotonicity claim and the slack: every admissible row with a finite utility)

and, block by block, that no row with u_i <= tau lies in a pruned block and that the pruned arg-min IS the arg-min
over all rows, lowest index among ties."""
import zlib

import numpy as np
import pytest

import prune_ref as pr
import util_ref

KINDS = ("agp", "bape", "jones")


def _case(rs, m, spread, ktt, ties=0):
    mu = rs.normal(0.0, spread, size=m)
    # var <= k(t,t): mostly a fraction of it, some tiny, some zero / negative / NaN (a cancelled or failed contraction)
    frac = rs.uniform(0.0, 1.0, size=m) ** rs.choice([1.0, 4.0, 16.0], size=m)
    var = ktt * frac
    var[rs.uniform(size=m) < 0.02] = 0.0
    var[rs.uniform(size=m) < 0.01] = -1e-12
    var[rs.uniform(size=m) < 0.01] = np.nan
    var[rs.uniform(size=m) < 0.05] = ktt            # nothing subtracted: u_i == b_i up to the slack
    adm = rs.uniform(size=m) < 0.9
    S = np.abs(mu) * rs.uniform(1.0, 50.0, size=m)  # sum |k alpha| >= |sum k alpha|
    for _ in range(ties):                           # exact duplicates in other blocks, before and after
        i, j = rs.randint(0, m, size=2)
        mu[j], var[j], S[j], adm[j] = mu[i], var[i], S[i], adm[i]
    return mu, var, S, adm


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spread,ktt", [(300.0, 1.0), (1.0, 1.0), (1e-3, 1.0), (5.0, 1e-6), (5.0, 40.0), (0.0, 2.5)])
def test_no_winner_is_pruned(kind, spread, ktt):
    rs = np.random.RandomState(zlib.crc32(repr((kind, spread, ktt)).encode()))
    for rep in range(6):
        m = int(rs.choice([63, 64 * 40 + 1, 64 * 700 + 17]))
        mu, var, S, adm = _case(rs, m, spread, ktt, ties=20)
        ybest = float(rs.normal(0.0, max(spread, 1e-3)))
        zeta = float(rs.choice([0.01, 1.0, 1e6]))
        u = np.where(adm, util_ref.f64(kind, mu, var, zeta, ybest), np.inf)
        b = pr.row_bounds(kind, mu, ktt, S, adm, 1000, 8, zeta, ybest)
        ok = adm & (u < np.inf)                                  # rows that can enter the arg-min (NaN < inf is False)
        assert np.all(b[ok] <= u[ok]), (kind, np.max(b[ok] - u[ok]))
        assert np.all(np.isposinf(b[~adm]))
        bi, bu, sd, sv, tau, bmin = pr.pruned_argmin(kind, mu, var, ktt, S, adm, 1000, 8, zeta, ybest)
        want = pr.argmin(u)
        assert bi == want and (want < 0 or np.float64(bu).view(np.uint64) == u[want].view(np.uint64))
        # no row at or below tau in a pruned block, ties included
        kept = np.zeros(len(bmin), dtype=bool)
        kept[sd] = True
        kept[sv] = True
        low = np.nonzero(ok & (u <= tau))[0]
        assert np.all(kept[low // pr.BLOCK])
        assert np.all(np.diff(sv) > 0) and not np.intersect1d(sd, sv).size


def test_everything_ties_nothing_is_pruned():
    m = 64 * 50
    mu = np.full(m, -3.25)
    var = np.full(m, 0.4)
    S = np.full(m, 10.0)
    adm = np.ones(m, dtype=bool)
    for kind in KINDS:
        bi, bu, sd, sv, tau, bmin = pr.pruned_argmin(kind, mu, var, 1.0, S, adm, 500, 4)
        assert bi == 0 and len(sd) == pr.SEED and len(sd) + len(sv) == 50
        assert list(sd) == list(range(pr.SEED))                 # equal bounds: the lowest block numbers


def test_nothing_admissible_and_infinite_tau():
    m = 64 * 20 + 5
    rs = np.random.RandomState(3)
    mu = rs.normal(size=m)
    S = np.abs(mu) * 3
    var = np.full(m, 0.5)
    none = np.zeros(m, dtype=bool)
    bi, bu, sd, sv, tau, bmin = pr.pruned_argmin("agp", mu, var, 1.0, S, none, 300, 2)
    assert (bi, bu) == (-1, np.inf) and len(sd) == 0 and len(sv) == 0 and np.isposinf(tau)
    # every evaluated utility NaN (AGP at var < 0): tau = +inf and every block with an admissible row survives
    adm = np.ones(m, dtype=bool)
    adm[64:128] = False
    bi, bu, sd, sv, tau, bmin = pr.pruned_argmin("agp", mu, np.full(m, -1.0), 1.0, S, adm, 300, 2)
    assert (bi, bu) == (-1, np.inf) and np.isposinf(tau) and len(sd) + len(sv) == 20 and 1 not in sv and 1 not in sd


def test_select_with_a_planted_tau():
    bmin = np.array([3.0, np.inf, -np.inf, 1.0, 1.0, 2.0, np.inf, 0.5])
    assert list(pr.seeds(bmin, 3)) == [2, 7, 3]
    assert list(pr.select(bmin, 1.0, [2, 7, 3])) == [4]
    assert list(pr.select(bmin, np.inf, [2])) == [0, 3, 4, 5, 7]
    assert list(pr.select(bmin, -np.inf, [])) == [2]
