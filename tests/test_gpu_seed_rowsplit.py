# -*- coding: utf-8 -*-
"""MI355X: the row-half items of the pruned arg-min's seed launch (csrc/sweep.hip "row-half items", sweep_fold_kernel;
``GP.seed_rowsplit`` / apgp_set_seed_rowsplit) change no bit.

A 256-row block of W at or above J0 that has rows in its lower half goes as two workgroups of 128 rows, and the fold
continues the upper half's chain of squares through the lower half's accumulators in the whole item's order.  Every case
runs with ``sweep_prune = 2`` (pruned from two candidates on) at J0 = 0 (every such row block), J0 = nrb / 2 and
J0 >= nrb (no halves: the launch as it was), and compares index, utility bits, seed count, survivor count and the bits
of tau across the three, with ``sweep_prune = 0`` (the full sweep) and with ``argmin(u)`` of a ``return_all`` call.

n gives two to five row blocks and a last block of 1, 44, 128 (no lower half: never halved), 129 (a lower half of one
row), 192, 193 and 256 rows; D both feeder forms (8: the single loop; 1, 2, 3, 16: the structured one) and, with 16, a
fit without the coarse bound's pre-split rows; m fewer seeds than the cap of 16 blocks (65: two blocks), exactly the
cap, and survivors beyond it."""
import numpy as np
import pytest

import fantasy_ref
import test_gpu_argmin_contract as ac
import test_gpu_sweep_prune as sp
import test_gpu_utility_epilogue as ep

pytestmark = pytest.mark.gpu

KINDS = ac.KINDS
SIZES = (257, 300, 384, 385, 448, 449, 512, 513, 640, 1100)
DIMS = (1, 2, 3, 8, 16)
MS = (65, 64 * 16, 64 * 17 + 5)


def _nrb(n):
    return (n + 255) // 256


def _switch_values(n):
    return (0, _nrb(n) // 2, _nrb(n))


def _one(gp, y, T, kind, rowsplit, **kw):
    """(index, bits of u, seed count, survivor count, bits of tau) of one pruned call at one switch value."""
    gp.sweep_prune, gp.sweep_prune_stats, gp.seed_rowsplit = 2, True, rowsplit
    try:
        bi, bu = gp.acquire(y, T, kind, **kw)
        ns, nv, tau = sp._counts(gp)
    finally:
        gp.sweep_prune, gp.sweep_prune_stats, gp.seed_rowsplit = None, False, None
    return bi, int(sp._bits(bu)), ns, nv, int(sp._bits(tau))


def _across_the_switch(gp, y, T, kind, n, **kw):
    """The same record at the three switch values, the full sweep's winner and argmin(u) of a return_all call."""
    recs = [_one(gp, y, T, kind, v, **kw) for v in _switch_values(n)]
    assert recs[0] == recs[1] == recs[2], (kind, n, _switch_values(n), recs)
    gp.sweep_prune = 0
    try:
        fi, fu = gp.acquire(y, T, kind, **kw)
    finally:
        gp.sweep_prune = None
    assert (fi, int(sp._bits(fu))) == recs[0][:2], (kind, n, fi, fu, recs[0])
    ri, ru, u, _, _ = gp.acquire(y, T, kind, return_all=True, **kw)
    want = fantasy_ref.argmin(u)
    assert recs[0][0] == want == ri, (kind, n, recs[0], want, ri)
    if want >= 0:
        assert recs[0][1] == int(sp._bits(u[want])) == int(sp._bits(ru))
    return recs[0]


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_bits_across_the_switch(n, D):
    for m in MS:
        gp, y, T = ac._setup(n, D, m, "inverse")
        assert gp.seed_rowsplit is None
        mask = np.ones(m, dtype=np.uint8)
        mask[np.random.RandomState(5).uniform(size=m) < 0.3] = 0
        Tb = T.copy()
        Tb[::7, 0] = 2.5                            # outside the box
        Tn = T.copy()
        Tn[3, D - 1] = np.nan                       # a NaN row in the first seed block
        for kind in KINDS:
            bi, _, ns, nv, _ = _across_the_switch(gp, y, T, kind, n)
            assert ns == min(16, (m + 63) // 64) and 0 <= nv <= (m + 63) // 64 - ns
            _across_the_switch(gp, y, Tb, kind, n, bounds=ac.BOX * D)
            _across_the_switch(gp, y, T, kind, n, mask=mask)
            assert _across_the_switch(gp, y, Tn, kind, n)[0] != 3


def test_linear_kernel_term():
    """With a LinearKernel term the coarse stage falls away and the LIN instantiation of the kernel runs."""
    from approxposterior_amd import gp as agp
    n, D, m = 640, 3, 64 * 17 + 5
    case = ep.C(n, D, m, "inverse", 1.0, -20, 1.0, lin=1, seed=51)
    c = ep.build_case(case)
    T = c["T"]
    T[~np.isfinite(T).all(axis=1)] = 0.25
    gp = ep.make_gp(agp, case, c["ell"])
    gp.variance_mode = "inverse"
    gp.compute(c["X"])
    for kind in KINDS:
        _across_the_switch(gp, c["y"], T, kind, n)


def test_solve_form_ignores_the_switch():
    n, D, m = 640, 3, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "solve")
    for kind in KINDS:
        _across_the_switch(gp, y, T, kind, n)


def test_winner_in_the_lower_half():
    """A candidate on a training point of the last full row block's LOWER half: its variance is amp less a sum of
    squares that those rows dominate (W is lower triangular: row i of V carries what the points before i left
    unexplained), so a dropped or doubled half changes its utility by orders of magnitude -- and with the mask down to
    that one row it is the winner, whose bits must be those of the return_all call.  The same for a point of the upper
    half and of a partial last block's lower half."""
    n, D, m = 1100, 3, 64 * 17 + 5                  # row blocks of 256, 256, 256, 256, 76 rows
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    for point in (3 * 256 + 200, 3 * 256 + 130, 3 * 256 + 17, 2 * 256 + 255, 1 * 256 + 128, 4 * 256 + 70):
        for row in (70, 64 * 16 + 9):               # alone under the mask (one seed block) and among all rows
            T = T0.copy()
            T[row] = X[point]
            mask = np.zeros(m, dtype=np.uint8)
            mask[row] = 1
            for kind in KINDS:
                assert _across_the_switch(gp, y, T, kind, n, mask=mask)[0] == row
                _across_the_switch(gp, y, T, kind, n)
    # and n = 449: the last block's lower half is 65 rows
    n = 449
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    for point in (256 + 192, 256 + 129, 256 + 100):
        T = T0.copy()
        T[70] = X[point]
        mask = np.zeros(m, dtype=np.uint8)
        mask[70] = 1
        for kind in KINDS:
            assert _across_the_switch(gp, y, T, kind, n, mask=mask)[0] == 70
