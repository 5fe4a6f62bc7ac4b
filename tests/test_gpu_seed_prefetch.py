# -*- coding: utf-8 -*-
"""MI355X: the stage ring of the parked seed launch's row-part workgroups (csrc/sweep.hip ``sweep2_kernel<.., DEEP>``;
``GP.seed_prefetch`` / apgp_set_seed_prefetch) changes no bit.

With the switch on, a row-part workgroup keeps its tiles in a ring of stages in LDS and its feeder wavefronts request the
re-read tiles several tiles ahead, with counted waits in front of the tile barriers.  Every case runs with
``sweep_prune = 2`` (pruned from two candidates on).

1. index, bits of u and all five ``last_prune_counts`` (seed count, survivor count, bits of tau, blocks the coarse bound
   left, second-wave seeds swept) are equal with the switch on and off, and the winner is the full sweep's and
   ``argmin(u)`` of a ``return_all`` call.  n: two to five row blocks, last blocks of 1, 129, 1, 129 and 76 rows; forced
   ``seed_parts`` 1, 2, 4, 8 (pairs per item: 8, 4, 2 parts of a row block and whole items); distances 6, 3 and 0;
   ``seed_rowsplit`` 0 and nrb / 2; ``seed_first`` 1, 4, 16; D 3, 8, 16 (Dpad 4, 8, 16: both of the
   parent's feeder forms); m: fewer seeds than the cap, the cap, survivors beyond it.  Once each: a box, a mask, a NaN
   row in the first seed block.
2. every seed candidate's row-block shares of sum V^2 and of mu are bit-equal on and off (C ABI, apgp_acquire_rows2
   over the row stream GP.acquire hands it, sign-sorted where the fit has one, caller-owned scratch);
   a difference is reported with its row block.
3. stale stages: the same call three times in a row and then one on other candidates; a candidate on a training point,
   alone under the mask, whose variance a wrong or stale B stage moves by orders of magnitude.
4. a LinearKernel term, the substitution form and one row block give equal bits at both values.

Tolerance: none, every comparison is of bits."""
import ctypes

import numpy as np
import pytest

import fantasy_ref
import test_gpu_argmin_contract as ac
import test_gpu_seed_park as pk
import test_gpu_seed_waves as sw
import test_gpu_sweep_prune as sp
import test_gpu_utility_epilogue as ep

pytestmark = pytest.mark.gpu

SIZES = (257, 385, 513, 641, 1100)
DIMS = (3, 8, 16)
MS = (65, 64 * 16, 64 * 17 + 5)
PARTS = (1, 2, 4, 8)               # sub-block pairs per item: rings of 8, 6 and 4 stages, and whole items
DISTANCES = (6, 3, 0)               # as far as the ring holds, a shorter distance (other wait counts), the launch as it was
FIRSTS = (1, 4, 16)
SW_CAND = pk.SW_CAND


def _one(gp, y, T, kind, prefetch, parts=None, rowsplit=None, first=None, **kw):
    """(index, bits of u, the five counts) of one pruned call at one set of switch values."""
    gp.sweep_prune, gp.sweep_prune_stats = 2, True
    gp.seed_prefetch, gp.seed_parts, gp.seed_rowsplit, gp.seed_first = prefetch, parts, rowsplit, first
    try:
        bi, bu = gp.acquire(y, T, kind, **kw)
        counts = tuple(int(v) for v in gp.last_prune_counts.cpu().numpy())
    finally:
        gp.sweep_prune, gp.sweep_prune_stats = None, False
        gp.seed_prefetch, gp.seed_parts, gp.seed_rowsplit, gp.seed_first = None, None, None, None
    assert len(counts) == 5
    return (bi, int(sp._bits(bu))) + counts


def _reference(gp, y, T, kind, **kw):
    """(index, bits of u) of the full sweep, which must be argmin(u) of a return_all call."""
    gp.sweep_prune = 0
    try:
        fi, fu = gp.acquire(y, T, kind, **kw)
    finally:
        gp.sweep_prune = None
    ri, ru, u, _, _ = gp.acquire(y, T, kind, return_all=True, **kw)
    want = fantasy_ref.argmin(u)
    assert fi == want == ri and want >= 0
    assert int(sp._bits(fu)) == int(sp._bits(u[want])) == int(sp._bits(ru))
    return want, int(sp._bits(u[want]))


def _across_the_switch(gp, y, T, kind, ref, **sel):
    recs = [_one(gp, y, T, kind, v, **sel) for v in DISTANCES]
    assert all(r == recs[-1] for r in recs), (kind, sel, recs)
    assert recs[0][:2] == ref, (kind, sel, recs[0], ref)
    return recs[0]


# ---- 1. bits across the switch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_bits_across_the_switch(n, D):
    nrb = pk._nrb(n)
    for m in MS:
        gp, y, T = ac._setup(n, D, m, "inverse")
        assert gp.seed_prefetch is None
        ref = _reference(gp, y, T, "agp")
        for parts in PARTS:
            for rowsplit in (0, nrb // 2):
                for first in FIRSTS:
                    rec = _across_the_switch(gp, y, T, "agp", ref, parts=parts, rowsplit=rowsplit, first=first)
                    assert rec[2] == min(16, (m + 63) // 64)


@pytest.mark.parametrize("what", ("box", "mask", "nan"))
def test_box_mask_and_nan_row_across_the_switch(what):
    n, D, m = 641, 8, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "inverse")
    T = T.copy()
    kw = {}
    if what == "box":
        T[::7, 0] = 2.5                             # outside the box
        kw = dict(bounds=ac.BOX * D)
    elif what == "mask":
        mask = np.ones(m, dtype=np.uint8)
        mask[np.random.RandomState(5).uniform(size=m) < 0.3] = 0
        kw = dict(mask=mask)
    else:
        T[3, D - 1] = np.nan                        # a NaN row in the first seed block
    ref = _reference(gp, y, T, "agp", **kw)
    assert ref[0] != 3 or what != "nan"
    for parts in PARTS:
        _across_the_switch(gp, y, T, "agp", ref, parts=parts, rowsplit=0, first=4, **kw)


# ---- 2. the shares -----------------------------------------------------------------------------------------------------
def _acquire(gp, y, T, prefetch, first, parts, rowsplit):
    """One pruned apgp_acquire_rows2 call for the winner alone, over the row stream GP.acquire hands the coarse bound:
    (index, bits of u), the whole work area as a host array."""
    torch, _lib, lib = pk._rt()
    from approxposterior_amd import gp as agp
    ks = gp._kernel_struct()
    n, m = len(gp._x), T.shape[0]
    gp._ensure_linv()
    gp._ensure_xs(y)
    rows, rows_kind = gp._prune_stream()            # (sign-sorted where the fit has such a stream: Dpad <= 8)
    T_d = torch.from_numpy(np.ascontiguousarray(T)).cuda()
    part = torch.zeros(int(lib.apgp_acquire_work_len(m, n)), dtype=torch.float64, device="cuda")
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    was = (lib.apgp_set_sweep_prune(2), lib.apgp_set_seed_park(1), lib.apgp_set_seed_rowsplit(rowsplit),
           lib.apgp_set_seed_first(first), lib.apgp_set_seed_parts(parts), lib.apgp_set_seed_prefetch(prefetch))
    try:
        _lib.check(lib.apgp_acquire_rows2(T_d.data_ptr(), m, 0, gp._packed.data_ptr(), gp._xs.data_ptr(), n, ctypes.byref(ks),
                                          float(gp.mean.value), agp.UTILITY_KINDS["agp"], None, None, None, 0.01,
                                          float(np.max(y)), None, None, None, part.data_ptr(), best.data_ptr(), rows,
                                          rows_kind, None), "apgp_acquire_rows2")
    finally:
        lib.apgp_set_sweep_prune(was[0])
        lib.apgp_set_seed_park(was[1])
        lib.apgp_set_seed_rowsplit(was[2])
        lib.apgp_set_seed_first(was[3])
        lib.apgp_set_seed_parts(was[4])
        lib.apgp_set_seed_prefetch(was[5])
    torch.cuda.synchronize()
    b = best.cpu().numpy().view(np.int64)
    return (int(b[1]), int(b[0])), part.cpu().numpy()


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", (385, 641, 1100))
def test_row_block_shares_are_bit_equal(n, D):
    """m = 64 * 16: every block is a seed and nothing survives beyond them, so the survivors' launches leave the seed
    launch's shares where they are."""
    nrb, m = pk._nrb(n), 64 * 16
    gp, y, T = ac._setup(n, D, m, "inverse")
    T = T.copy()
    T[3, D - 1] = np.nan
    lay = pk._layout(m, n)
    ne = lay["ncb"] * SW_CAND * nrb
    for parts in PARTS:
        for rowsplit in (0, nrb // 2):
            out = {}
            for prefetch in DISTANCES:
                best, part = _acquire(gp, y, T, prefetch, first=16, parts=parts, rowsplit=rowsplit)
                cnt = sw._counts(part, lay)
                assert cnt[0] == lay["ncb"] and cnt[1] == 0, (n, D, parts, cnt)
                out[prefetch] = (best, part[lay["q"]:lay["q"] + ne].view(np.int64), part[lay["mu"]:lay["mu"] + ne].view(np.int64),
                                 part[lay["seeds"]:lay["seeds"] + lay["ncb"]].view(np.int64))
            for v in DISTANCES[:-1]:
                assert out[v][0] == out[0][0]
                for name, a, b in zip(("sum V^2", "mu"), out[v][1:3], out[0][1:3]):
                    bad = np.flatnonzero(a != b)
                    # share e = (position * 64 + candidate) * nrb + row block
                    assert bad.size == 0, (n, D, parts, rowsplit, v, name, "row blocks", sorted(set(bad % nrb)),
                                           "positions", sorted(set(bad // (SW_CAND * nrb)))[:4])
                assert np.array_equal(out[v][3], out[0][3])
            assert np.any(out[6][1] != 0) and np.any(out[6][2] != 0)


# ---- 3. stale stages -----------------------------------------------------------------------------------------------------
def test_repeated_calls_and_then_other_candidates():
    n, D, m = 1100, 8, 64 * 16
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    Ta, Tb = T0.copy(), T0[::-1].copy()
    for parts in PARTS:
        sel = dict(parts=parts, rowsplit=0, first=4)
        runs = [_one(gp, y, Ta, "agp", 6, **sel) for _ in range(3)]
        assert runs[0] == runs[1] == runs[2], (parts, runs)
        other = _one(gp, y, Tb, "agp", 6, **sel)
        assert other == _one(gp, y, Tb, "agp", 0, **sel), parts
        assert runs[0] == _one(gp, y, Ta, "agp", 0, **sel), parts


def test_a_parked_stage_decides_the_winner():
    n, D, m = 769, 3, 64 * 17 + 5                   # row blocks of 256, 256, 256 and 1 rows
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    for point in (256 + 100, 256 + 17, 512 + 100, 512 + 255, 40):
        for row in (70, 64 * 16 + 9):               # alone under the mask (one seed block) and among all rows
            T = T0.copy()
            T[row] = X[point]
            mask = np.zeros(m, dtype=np.uint8)
            mask[row] = 1
            for kind in ac.KINDS:
                ref = _reference(gp, y, T, kind, mask=mask)
                assert ref[0] == row
                for parts in PARTS:
                    _across_the_switch(gp, y, T, kind, ref, parts=parts, rowsplit=0, first=4, mask=mask)
                _across_the_switch(gp, y, T, kind, _reference(gp, y, T, kind), parts=2, rowsplit=0, first=4)


# ---- 4. routes that must ignore the switch -----------------------------------------------------------------------------------
def test_linear_kernel_term_ignores_the_switch():
    from approxposterior_amd import gp as agp
    n, D, m = 640, 3, 64 * 17 + 5
    case = ep.C(n, D, m, "inverse", 1.0, -20, 1.0, lin=1, seed=51)
    c = ep.build_case(case)
    T = c["T"]
    T[~np.isfinite(T).all(axis=1)] = 0.25
    gp = ep.make_gp(agp, case, c["ell"])
    gp.variance_mode = "inverse"
    gp.compute(c["X"])
    for kind in ac.KINDS:
        _across_the_switch(gp, c["y"], T, kind, _reference(gp, c["y"], T, kind))


def test_solve_form_ignores_the_switch():
    n, D, m = 640, 3, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "solve")
    for kind in ac.KINDS:
        _across_the_switch(gp, y, T, kind, _reference(gp, y, T, kind))


def test_one_row_block_ignores_the_switch():
    n, D, m = 200, 3, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "inverse")
    for kind in ac.KINDS:
        _across_the_switch(gp, y, T, kind, _reference(gp, y, T, kind))
