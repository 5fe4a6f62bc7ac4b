# -*- coding: utf-8 -*-
"""MI355X: the parked stream of the seed blocks (csrc/sweep.hip seed_park_kernel; ``GP.seed_park`` /
apgp_set_seed_park) changes no bit.

With the switch on, the k*(t, x) operands of the pruned arg-min's seed blocks are generated once per call into slot
`position` of the parked-operand region of the caller's scratch, and the seed launch's items read the chunks left of
their diagonal from there instead of generating them.  Every case runs with ``sweep_prune = 2`` (pruned from two
candidates on).

1. index, bits of u, seed count, survivor count and bits of tau are equal with the switch on and off, at
   ``seed_rowsplit`` 0, nrb / 2 and nrb, and equal to the full sweep's winner and to ``argmin(u)`` of a ``return_all``
   call.  n: two to five row blocks, a last block of 1, 129, 193 and 76 rows; D: the structured feeder (3), the plain
   one (8), Dpad 16 and Dpad 32 with its second x piece (17); m: fewer seeds than the cap, the cap, survivors beyond it.
2. every seed candidate's row-block shares of sum V^2 and of mu are bit-equal on and off (C ABI, caller-owned scratch).
3. the stream itself against tests/kvalue_ref.py, site "sweep": chunk 0 in the fused form, every other chunk in the
   plain one; rows past m enter as t = 0; a row with a NaN coordinate holds what the feeder's clamp makes of it.
4. a candidate on a training point, alone under the mask, whose chunk is read as a parked operand one and two row blocks
   later: a wrong or stale chunk moves its variance by orders of magnitude; and two pruned calls in a row on different
   candidates, where the second must not see the first one's slots.
5. a LinearKernel term, the substitution form and one row block keep the launch as it was at both values.

Tolerance: none, every comparison is of bits."""
import ctypes

import numpy as np
import pytest

import fantasy_ref
import kvalue_ref as kr
import test_gpu_argmin_contract as ac
import test_gpu_sweep_prune as sp
import test_gpu_utility_epilogue as ep

pytestmark = pytest.mark.gpu

KINDS = ac.KINDS
SIZES = (257, 385, 449, 513, 641, 769, 1100)
DIMS = (3, 8, 16, 17)
MS = (65, 64 * 16, 64 * 17 + 5)
SW_BCH, SW_CAND, S2_SPLIT_MAX, SW_GRID, PR_SEED = 1024, 64, 184, 256, 16


def _nrb(n):
    return (n + 255) // 256


def _one(gp, y, T, kind, rowsplit, park, **kw):
    """(index, bits of u, seed count, survivor count, bits of tau) of one pruned call at one pair of switch values."""
    gp.sweep_prune, gp.sweep_prune_stats, gp.seed_rowsplit, gp.seed_park = 2, True, rowsplit, park
    try:
        bi, bu = gp.acquire(y, T, kind, **kw)
        ns, nv, tau = sp._counts(gp)
    finally:
        gp.sweep_prune, gp.sweep_prune_stats, gp.seed_rowsplit, gp.seed_park = None, False, None, None
    return bi, int(sp._bits(bu)), ns, nv, int(sp._bits(tau))


def _across_the_switch(gp, y, T, kind, n, rowsplits=None, **kw):
    """The same record with the stream on and off at every ``seed_rowsplit``, the full sweep's winner and argmin(u) of a
    return_all call."""
    if rowsplits is None:
        rowsplits = (0, _nrb(n) // 2, _nrb(n))
    recs = [_one(gp, y, T, kind, v, park, **kw) for v in rowsplits for park in (1, 0)]
    assert all(r == recs[0] for r in recs), (kind, n, rowsplits, recs)
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


# ---- 1. bits across the switch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_bits_across_the_switch(n, D):
    for m in MS:
        gp, y, T = ac._setup(n, D, m, "inverse")
        assert gp.seed_park is None
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


# ---- the C ABI with a caller-owned work area ---------------------------------------------------------------------------
def _rt():
    import torch
    from approxposterior_amd import _lib
    return torch, _lib, _lib.load()


def _acquire(gp, y, T, kind, park, rowsplit=-1, mask=None):
    """One pruned apgp_acquire_rows call for the winner alone; the whole work area comes back as a host array."""
    torch, _lib, lib = _rt()
    from approxposterior_amd import gp as agp
    ks = gp._kernel_struct()
    n, m = len(gp._x), T.shape[0]
    gp._ensure_linv()
    gp._ensure_xs(y)
    T_d = torch.from_numpy(np.ascontiguousarray(T)).cuda()
    mask_d = None if mask is None else torch.from_numpy(mask).cuda()
    part = torch.zeros(int(lib.apgp_acquire_work_len(m, n)), dtype=torch.float64, device="cuda")
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    was = (lib.apgp_set_sweep_prune(2), lib.apgp_set_seed_park(park), lib.apgp_set_seed_rowsplit(rowsplit))
    try:
        _lib.check(lib.apgp_acquire_rows(T_d.data_ptr(), m, 0, gp._packed.data_ptr(), gp._xs.data_ptr(), n, ctypes.byref(ks),
                                         float(gp.mean.value), agp.UTILITY_KINDS[kind], None, None, agp._ptr(mask_d), 0.01,
                                         float(np.max(y)), None, None, None, part.data_ptr(), best.data_ptr(),
                                         agp._ptr(gp._prune_rows), None), "apgp_acquire_rows")
    finally:
        lib.apgp_set_sweep_prune(was[0])
        lib.apgp_set_seed_park(was[1])
        lib.apgp_set_seed_rowsplit(was[2])
    torch.cuda.synchronize()
    return best.cpu().numpy().view(np.int64), part.cpu().numpy()


def _layout(m, n):
    """Offsets (doubles) into the work area, from the layout comment above pr_work_len: the parked operands, the
    row-block shares of sum V^2 and of mu, the seed block numbers, the counts."""
    _, _, lib = _rt()
    ncb = (m + SW_CAND - 1) // SW_CAND
    slots = min(ncb, SW_GRID)
    ncache = 16 * (_nrb(n) - 1)
    k0 = 2 * ncb
    q0 = k0 + slots * ncache * SW_BCH
    mu0 = q0 + S2_SPLIT_MAX * SW_CAND * _nrb(n)
    c0 = int(lib.apgp_sweep_prune_counts_offset(m, n))
    assert mu0 + S2_SPLIT_MAX * SW_CAND * _nrb(n) + 2 * ncb + PR_SEED == c0        # the two descriptions agree
    return dict(ncb=ncb, ncache=ncache, k=k0, q=q0, mu=mu0, seeds=c0 - PR_SEED, counts=c0)


# ---- 2. the shares -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 8))
@pytest.mark.parametrize("n", (449, 769, 1100))
def test_row_block_shares_are_bit_equal(n, D):
    """m = 65 and 64 * 16: every block is a seed and nothing survives beyond them, so the survivors' launches leave the
    seed launch's shares where they are."""
    nrb = _nrb(n)
    for m in (65, 64 * 16):
        gp, y, T = ac._setup(n, D, m, "inverse")
        T[3, D - 1] = np.nan
        lay = _layout(m, n)
        for rowsplit in (0, nrb // 2, nrb):
            out = {}
            for park in (1, 0):
                best, part = _acquire(gp, y, T, "agp", park, rowsplit)
                cnt = part[lay["counts"]:lay["counts"] + 2].view(np.int64)
                assert cnt[0] == lay["ncb"] and cnt[1] == 0, (n, D, m, cnt)
                ne = lay["ncb"] * SW_CAND * nrb
                out[park] = (best, part[lay["q"]:lay["q"] + ne].view(np.int64), part[lay["mu"]:lay["mu"] + ne].view(np.int64),
                             part[lay["seeds"]:lay["seeds"] + lay["ncb"]].view(np.int64))
            for a, b in zip(out[1], out[0]):
                assert np.array_equal(a, b), (n, D, m, rowsplit, np.argwhere(a != b)[:4])
            assert np.any(out[1][1] != 0) and np.any(out[1][2] != 0)


# ---- 3. the stream itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 8))
def test_stream_has_the_restated_bits(D):
    """n = 769 (48 parked chunks per slot), m = 130: three seed blocks, the last with two rows -- its other lanes are rows
    past m.  Four lanes per block against the restatement, one of them the NaN row; every chunk, every training point."""
    n, m = 769, 130
    gp, y, T = ac._setup(n, D, m, "inverse")
    T[3, D - 1] = np.nan
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    ks = gp._kernel_struct()
    k = kr.kern([float(ks.inv_metric[d]) for d in range(D)], amp=float(ks.amp))
    lay = _layout(m, n)
    _, part = _acquire(gp, y, T, "agp", 1)
    assert part[lay["counts"]:lay["counts"] + 1].view(np.int64)[0] == 3
    seeds = part[lay["seeds"]:lay["seeds"] + 3].view(np.int64)
    assert sorted(seeds) == [0, 1, 2]
    nan_value = k.amp * kr.exp_restate(float("nan"))             # (fmax(NaN, -700) = -700: the clamp swallows NaN)
    checked = 0
    for p, blk in enumerate(seeds):
        slot = part[lay["k"] + p * lay["ncache"] * SW_BCH:lay["k"] + (p + 1) * lay["ncache"] * SW_BCH]
        # [chunk][half][feeder thread][2]: thread ht = 64 hw + 16 kq + cl holds k = 4 kk + kq, kk = 2 half + {0, 1}
        got = slot.reshape(lay["ncache"], 2, 4, 4, 16, 2)          # chunk, half, hw, kq, cl, pair
        for cand in (0, 1, 3, 63):
            row = blk * SW_CAND + cand
            t = T[row] if row < m else np.zeros(D)
            hw, cl = cand // 16, cand % 16
            for kc in range(lay["ncache"]):
                dev = np.empty(16)
                for kk in range(4):
                    for kq in range(4):
                        dev[4 * kk + kq] = got[kc, kk // 2, hw, kq, cl, kk % 2]
                if np.isnan(t).any():
                    want = np.full(16, nan_value)
                else:
                    want = kr.restate(t[None, :], X[16 * kc:16 * kc + 16], k, site="sweep", fused=(kc == 0))[0]
                assert np.array_equal(dev.view(np.int64), want.view(np.int64)), (D, p, blk, cand, kc, dev, want)
                checked += 16
    assert checked == 3 * 4 * lay["ncache"] * 16
    # the slots beyond the seed count are untouched
    rest = part[lay["k"] + 3 * lay["ncache"] * SW_BCH:lay["q"]]
    assert not rest.any()


# ---- 4. a wrong or stale chunk must show ---------------------------------------------------------------------------------
def test_a_parked_chunk_decides_the_winner():
    n, D, m = 769, 3, 64 * 17 + 5                   # row blocks of 256, 256, 256 and 1 rows
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    for point in (256 + 100, 256 + 17, 512 + 100, 512 + 255, 40):
        for row in (70, 64 * 16 + 9):               # alone under the mask (one seed block) and among all rows
            T = T0.copy()
            T[row] = X[point]
            mask = np.zeros(m, dtype=np.uint8)
            mask[row] = 1
            for kind in KINDS:
                assert _across_the_switch(gp, y, T, kind, n, mask=mask)[0] == row
                _across_the_switch(gp, y, T, kind, n)


def test_the_second_call_does_not_see_the_first_calls_slots():
    n, D, m = 769, 3, 64 * 16
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    Ta, Tb = T0.copy(), T0[::-1].copy()
    Ta[70] = X[256 + 100]
    Tb[70] = X[512 + 100]
    mask = np.zeros(m, dtype=np.uint8)
    mask[70] = 1
    for kind in KINDS:
        first = _one(gp, y, Ta, kind, -1, 1, mask=mask)
        second = _one(gp, y, Tb, kind, -1, 1, mask=mask)
        again = _one(gp, y, Ta, kind, -1, 1, mask=mask)
        assert first == again and first[0] == second[0] == 70, (kind, first, second, again)
        # (Jones gives -0.0 at either training point: sd -> 0 with imp < 0; the other two tell the calls apart)
        assert kind == "jones" or first[1] != second[1], (kind, first, second)
        for T, rec in ((Ta, first), (Tb, second)):
            ri, ru, u, _, _ = gp.acquire(y, T, kind, return_all=True, mask=mask)
            assert (ri, int(sp._bits(ru))) == rec[:2] and rec[1] == int(sp._bits(u[70])), (kind, rec, ri, ru)
            assert rec == _one(gp, y, T, kind, -1, 0, mask=mask)


# ---- 5. routes that keep the launch as it was ------------------------------------------------------------------------------
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
    for kind in KINDS:
        _across_the_switch(gp, c["y"], T, kind, n)


def test_solve_form_ignores_the_switch():
    n, D, m = 640, 3, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "solve")
    for kind in KINDS:
        _across_the_switch(gp, y, T, kind, n)


def test_one_row_block_ignores_the_switch():
    n, D, m = 200, 3, 64 * 17 + 5
    gp, y, T = ac._setup(n, D, m, "inverse")
    for kind in KINDS:
        _across_the_switch(gp, y, T, kind, n)
    # nothing is parked at n <= 256: the work area has no parked-operand region to write
    lay = _layout(m, n)
    assert lay["ncache"] == 0 and lay["k"] == lay["q"]
    on, off = _acquire(gp, y, T, "agp", 1), _acquire(gp, y, T, "agp", 0)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1].view(np.int64), off[1].view(np.int64))
