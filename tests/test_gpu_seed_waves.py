# -*- coding: utf-8 -*-
"""MI355X: the pruned arg-min's seeds in two waves and in row items finer than halves (csrc/sweep.hip
launch_sweep_list; ``GP.seed_first`` / apgp_set_seed_first, ``GP.seed_parts`` / apgp_set_seed_parts) change no bit.

The 16 seed blocks are selected as ever.  The first wave sweeps the first K of them; a workgroup of the second wave
forms tau_1 from the first wave's partials and leaves if its seed's bound lies above it.  A row block of either wave may
go as 1, 2, 4 or 8 items of 8, 4, 2 or 1 sub-block pairs whose sums sweep_fold_kernel puts together in the whole item's
order.  Every call goes through the C ABI with a caller-owned work area, pruned from two candidates on.

1. shares: with K = 16 and m = 64 * 16 every block is a seed; the row-block shares of sum V^2 and of mu of every position,
   the seeds and the winner are bit-equal across parts 8 / 4 / 2 / 1 and the parked stream on / off.
2. winner: K = 1, 4, 16 x parts x three utilities: index and bits of u equal the full sweep's and ``argmin`` of a
   ``return_all`` call, also with an index offset far above 2^32.  n: a last row block of 1, 193, 1 (three full blocks
   before it) and 76 rows; D: the structured feeder (3) and the plain one (8); m: fewer seeds than K = 4 allows a second
   wave for (65), exactly the seeds (64 * 16), survivors beyond them (64 * 17 + 5); one NaN row.
3. the second wave decides / skips / ties / tau_1 = +inf / nothing admissible / stale scratch: see the tests.

Tolerance: none, every comparison is of bits or of counts."""
import ctypes

import numpy as np
import pytest

import fantasy_ref
import test_gpu_argmin_contract as ac
import test_gpu_seed_park as pk
import test_gpu_sweep_prune as sp
import test_gpu_utility_epilogue as ep

pytestmark = pytest.mark.gpu

KINDS = ac.KINDS
SIZES = (257, 449, 769, 1100)
DIMS = (3, 8)
MS = (65, 64 * 16, 64 * 17 + 5)
PARTS = (8, 4, 2, 1)
FIRSTS = (1, 4, 16)
BIG = (1 << 40) + 12345
SW_CAND, PR_SEED = pk.SW_CAND, pk.PR_SEED


def _acquire(gp, y, T, kind, first=-1, parts=-1, park=1, rowsplit=0, mask=None, idx_offset=0, prune=2, part=None,
             want_part=True):
    """One apgp_acquire_rows call for the winner alone: (index, bits of u), the work area as a host array (or None)."""
    torch, _lib, lib = pk._rt()
    from approxposterior_amd import gp as agp
    ks = gp._kernel_struct()
    n, m = len(gp._x), T.shape[0]
    gp._ensure_linv()
    gp._ensure_xs(y)
    T_d = torch.from_numpy(np.ascontiguousarray(T)).cuda()
    mask_d = None if mask is None else torch.from_numpy(mask).cuda()
    if part is None:
        part = torch.zeros(int(lib.apgp_acquire_work_len(m, n)), dtype=torch.float64, device="cuda")
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    was = (lib.apgp_set_sweep_prune(prune), lib.apgp_set_seed_park(park), lib.apgp_set_seed_rowsplit(rowsplit),
           lib.apgp_set_seed_first(first), lib.apgp_set_seed_parts(parts))
    try:
        _lib.check(lib.apgp_acquire_rows(T_d.data_ptr(), m, idx_offset, gp._packed.data_ptr(), gp._xs.data_ptr(), n,
                                         ctypes.byref(ks), float(gp.mean.value), agp.UTILITY_KINDS[kind], None, None,
                                         agp._ptr(mask_d), 0.01, float(np.max(y)), None, None, None, part.data_ptr(),
                                         best.data_ptr(), agp._ptr(gp._prune_rows), None), "apgp_acquire_rows")
    finally:
        lib.apgp_set_sweep_prune(was[0])
        lib.apgp_set_seed_park(was[1])
        lib.apgp_set_seed_rowsplit(was[2])
        lib.apgp_set_seed_first(was[3])
        lib.apgp_set_seed_parts(was[4])
    torch.cuda.synchronize()
    b = best.cpu().numpy().view(np.int64)
    return (int(b[1]), int(b[0])), (part.cpu().numpy() if want_part else None)


def _counts(part, lay):
    return part[lay["counts"]:lay["counts"] + 5].view(np.int64)


def _reference(gp, y, T, kind, mask=None):
    """(index, bits of u) of the full sweep and of argmin(u) of a return_all call; they must agree."""
    gp.sweep_prune = 0
    try:
        fi, fu = gp.acquire(y, T, kind, mask=mask)
    finally:
        gp.sweep_prune = None
    ri, ru, u, _, _ = gp.acquire(y, T, kind, return_all=True, mask=mask)
    want = fantasy_ref.argmin(u)
    assert fi == want == ri
    if want >= 0:
        assert int(sp._bits(fu)) == int(sp._bits(u[want])) == int(sp._bits(ru))
    return want, (int(sp._bits(u[want])) if want >= 0 else None), u


def _same(got, want_i, want_bits, off=0):
    if want_i < 0:
        return got[0] == -1
    return got[0] == want_i + off and int(np.array(got[1], dtype=np.int64).view(np.uint64)) == want_bits


def _far(m, D):
    """Candidates far from every training point: k* underflows to zero, mu is the mean, var is k(t, t), and the bound of
    such a row is its utility.  All of them tie."""
    return 40.0 + np.random.RandomState(7).uniform(0.0, 1.0, size=(m, D))


# ---- 1. the shares -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_row_block_shares_do_not_depend_on_the_parts(n, D):
    nrb = pk._nrb(n)
    m = 64 * 16
    gp, y, T = ac._setup(n, D, m, "inverse")
    T = T.copy()
    T[3, D - 1] = np.nan
    lay = pk._layout(m, n)
    ne = lay["ncb"] * SW_CAND * nrb
    ref = None
    for parts in PARTS:
        for park in (1, 0):
            best, part = _acquire(gp, y, T, "agp", first=16, parts=parts, park=park, rowsplit=0)
            cnt = _counts(part, lay)
            assert cnt[0] == lay["ncb"] and cnt[1] == 0 and cnt[4] == 0, (n, D, parts, park, cnt)
            rec = (np.asarray(best), part[lay["q"]:lay["q"] + ne].view(np.int64), part[lay["mu"]:lay["mu"] + ne].view(np.int64),
                   part[lay["seeds"]:lay["seeds"] + lay["ncb"]].view(np.int64))
            if ref is None:
                ref = rec
                assert np.any(rec[1] != 0) and np.any(rec[2] != 0)
            for a, b in zip(rec, ref):
                assert np.array_equal(a, b), (n, D, parts, park, np.argwhere(a != b)[:4])


# ---- 2. the winner -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_winner_across_waves_and_parts(n, D):
    for m in MS:
        gp, y, T = ac._setup(n, D, m, "inverse")
        T = T.copy()
        T[3, D - 1] = np.nan
        lay = pk._layout(m, n)
        for kind in KINDS:
            want_i, want_bits, _ = _reference(gp, y, T, kind)
            assert want_i >= 0 and want_i != 3
            off_rec = _acquire(gp, y, T, kind, prune=0, want_part=False)[0]
            assert _same(off_rec, want_i, want_bits), (n, D, m, kind, off_rec, want_i)
            for first in FIRSTS:
                for parts in PARTS:
                    got, part = _acquire(gp, y, T, kind, first=first, parts=parts)
                    assert _same(got, want_i, want_bits), (n, D, m, kind, first, parts, got, want_i, want_bits)
                    cnt = _counts(part, lay)
                    assert cnt[0] == min(PR_SEED, lay["ncb"]) and 0 <= cnt[4] <= max(0, cnt[0] - first), (first, parts, cnt)
                got = _acquire(gp, y, T, kind, first=first, parts=-1, rowsplit=-1, idx_offset=BIG, want_part=False)[0]
                assert _same(got, want_i, want_bits, BIG), (n, D, m, kind, first, got)


# ---- 3. the second wave ----------------------------------------------------------------------------------------------------
def _planted(n, D, m, nplant):
    """Candidates with `nplant` blocks masked down to one row each, that row ON one of the training points with the
    largest y: mu = y there and the bound takes var = k(t, t), while var ~ 0 makes the utility poor.  Eight more blocks
    stay admissible -- fewer than PR_SEED in all, so every one of them is a seed -- without the rows whose mean comes
    within 0.05 of a planted one's (AGP's bound falls with mu at the bound's fixed variance): the planted blocks have
    the smallest bounds, the first wave's tau_1 is a poor utility, and the winner sits in a later seed."""
    gp, y, T = ac._setup(n, D, m, "inverse")
    T = T.copy()
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    mask = np.zeros(m, dtype=np.uint8)
    top = np.argsort(-np.asarray(y))[:nplant]
    rows = []
    for j, p in enumerate(top):
        row = (5 + 3 * j) * SW_CAND + 9
        T[row] = X[p]
        rows.append(row)
    mu = gp.acquire(y, T, "agp", return_all=True)[3]
    for blk in (1, 2, 3, 10, 12, 20, 30, (m - 1) // SW_CAND):
        sl = slice(blk * SW_CAND, min((blk + 1) * SW_CAND, m))
        mask[sl] = mu[sl] < mu[rows].min() - 0.05
        assert mask[sl].any()
    mask[rows] = 1
    return gp, y, T, mask, rows


@pytest.mark.parametrize("first", (1, 4))
def test_the_second_wave_decides(first):
    n, D, m = 769, 3, 64 * 40 + 5
    gp, y, T, mask, rows = _planted(n, D, m, first)
    lay = pk._layout(m, n)
    kind = "agp"
    want_i, want_bits, u = _reference(gp, y, T, kind, mask=mask)
    one, part16 = _acquire(gp, y, T, kind, first=16, mask=mask)
    c16 = _counts(part16, lay)
    assert c16[0] == first + 8
    seeds = list(part16[lay["seeds"]:lay["seeds"] + c16[0]].view(np.int64))
    # the planted blocks are the first seeds, and the winner sits in a seed of rank >= K
    assert sorted(seeds[:first]) == sorted(r // SW_CAND for r in rows), (seeds, rows)
    assert want_i // SW_CAND in seeds[first:], (want_i, seeds)
    for parts in PARTS:
        for park in (1, 0):
            got, part = _acquire(gp, y, T, kind, first=first, parts=parts, park=park, mask=mask)
            c = _counts(part, lay)
            assert _same(got, want_i, want_bits) and got == one, (first, parts, park, got, want_i)
            assert c[4] > 0 and (c[0], c[1], c[3]) == (c16[0], c16[1], c16[3]) and c[2] == c16[2], (first, parts, c, c16)


def test_the_second_wave_skips():
    """A wide gap between the first bound and the second: one candidate far from the data (mu is the mean, var is
    k(t, t), its utility is its bound) and every other one next to a training point of the lowest quarter of y, whose
    bound -- AGP's falls with mu -- lies above that.  tau_1 of a first wave of one seed prunes the 15 others."""
    n, D, m = 769, 3, 64 * 20
    gp, y, _ = ac._setup(n, D, m, "inverse")
    lay = pk._layout(m, n)
    kind = "agp"
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    low = np.argsort(np.asarray(y))[:n // 4]
    T = X[low[np.arange(m) % len(low)]] + 1e-3 * np.random.RandomState(9).uniform(-1.0, 1.0, size=(m, D))
    row = 7 * SW_CAND + 9
    T[row] = _far(1, D)[0]
    want_i, want_bits, u = _reference(gp, y, T, kind)
    assert want_i == row
    got, part = _acquire(gp, y, T, kind, first=1)
    c = _counts(part, lay)
    seeds = part[lay["seeds"]:lay["seeds"] + PR_SEED].view(np.int64)
    assert _same(got, want_i, want_bits) and c[0] == PR_SEED and seeds[0] == row // SW_CAND, (got, c, seeds)
    bmin = part[lay["counts"] - PR_SEED - 2 * lay["ncb"]:lay["counts"] - PR_SEED - lay["ncb"]]
    tau = c[2:3].view(np.float64)[0]
    assert np.all(bmin[seeds[1:]] > tau), (bmin[seeds], tau)       # the case is what it claims to be
    assert c[4] == 0 and c[1] == 0, c
    part_u, part_i = part[:lay["ncb"]], part[lay["ncb"]:2 * lay["ncb"]].view(np.int64)
    assert np.all(np.isposinf(part_u[seeds[1:]])) and np.all(part_i[seeds[1:]] == -1)
    assert part_u[seeds[0]] == tau and part_i[seeds[0]] == row
    # a first wave of four: seeds 1 .. 3 are swept with it, the other twelve are not
    got, part = _acquire(gp, y, T, kind, first=4, parts=-1, rowsplit=-1)
    c = _counts(part, lay)
    part_u = part[:lay["ncb"]]
    assert _same(got, want_i, want_bits) and c[4] == 0 and np.all(np.isposinf(part_u[seeds[4:]])) and \
        np.all(np.isfinite(part_u[seeds[:4]]))


def test_a_tie_in_a_second_wave_seed_goes_to_the_lowest_index():
    n, D, m = 769, 3, 64 * 40 + 5
    gp, y, T, mask, rows = _planted(n, D, m, 1)
    lay = pk._layout(m, n)
    for kind in KINDS:
        want_i, _, _ = _reference(gp, y, T, kind, mask=mask)
        _, part = _acquire(gp, y, T, kind, first=16, mask=mask)
        seeds = list(part[lay["seeds"]:lay["seeds"] + 9].view(np.int64))
        # a duplicate of the winning row at a lower global index, in another seed of rank >= 1
        cand = [b for b in seeds[1:] if b != want_i // SW_CAND and b * SW_CAND + 9 not in rows]
        lower = [b for b in cand if b * SW_CAND < want_i]
        if not lower:                                # the winner sits in the lowest such seed: put the duplicate ABOVE
            blk = cand[0]                            # and demand that the original still wins
        else:
            blk = lower[0]
        T2 = T.copy()
        dup = blk * SW_CAND + 1
        T2[dup] = T[want_i]
        mask2 = mask.copy()
        mask2[dup] = 1
        want2, bits2, _ = _reference(gp, y, T2, kind, mask=mask2)
        assert want2 == min(dup, want_i)
        for parts in (4, 2):
            got, part = _acquire(gp, y, T2, kind, first=1, parts=parts, mask=mask2)
            assert _same(got, want2, bits2), (kind, parts, got, want2)


def test_nothing_admissible_and_an_empty_first_wave():
    n, D, m = 449, 3, 64 * 20
    gp, y, T0 = ac._setup(n, D, m, "inverse")
    lay = pk._layout(m, n)
    kind = "agp"
    none = np.zeros(m, dtype=np.uint8)
    got, part = _acquire(gp, y, T0, kind, first=4, mask=none)
    c = _counts(part, lay)
    assert got[0] == -1 and c[0] == 0 and c[1] == 0 and c[4] == 0, (got, c)
    # tau_1 = +inf: every admissible row of the first wave's seeds has a NaN utility.  AGP is NaN where the variance
    # comes out negative, which it does by rounding ON some training points once the white noise (e^-36) lies below the
    # contraction's rounding; such points with y above the mean, each alone under the mask in a block of its own, have
    # the smallest bounds among candidates far from the data.
    from approxposterior_amd import gp as agp
    case = ep.C(n, D, m, "inverse", 1.0, -36, 1.0, seed=50)
    cc = ep.build_case(case)
    gp = ep.make_gp(agp, case, cc["ell"])
    gp.variance_mode = "inverse"
    gp.compute(cc["X"])
    y = cc["y"]
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    _, _, ux = _reference(gp, y, X.copy(), kind)
    bad = [p for p in np.argsort(-np.asarray(y)) if np.isnan(ux[p]) and y[p] > float(gp.mean.value) + 0.05][:4]
    assert bad, "no training point with a negative computed variance: the case cannot be built"
    first = len(bad)
    T = _far(m, D)
    mask = np.ones(m, dtype=np.uint8)
    blocks = [2, 6, 7, 11][:first]
    for blk, p in zip(blocks, bad):
        mask[blk * SW_CAND:(blk + 1) * SW_CAND] = 0
        mask[blk * SW_CAND + 5] = 1
        T[blk * SW_CAND + 5] = X[p]
    want_i, want_bits, u = _reference(gp, y, T, kind, mask=mask)
    assert want_i == 0 and all(np.isnan(u[b * SW_CAND + 5]) for b in blocks)
    for parts in (4, 2):
        got, part = _acquire(gp, y, T, kind, first=first, parts=parts, mask=mask)
        c = _counts(part, lay)
        seeds = list(part[lay["seeds"]:lay["seeds"] + PR_SEED].view(np.int64))
        assert sorted(seeds[:first]) == blocks, seeds
        assert _same(got, want_i, want_bits) and c[0] == PR_SEED and c[4] == PR_SEED - first, (got, want_i, c)


def test_the_second_call_does_not_see_the_first_calls_scratch():
    n, D, m = 769, 3, 64 * 40 + 5
    gp, y, Ta, mask, rows = _planted(n, D, m, 1)
    torch, _lib, lib = pk._rt()
    Tb = Ta[::-1].copy()
    Tb[rows[0]] = Ta[rows[0]]
    part = torch.zeros(int(lib.apgp_acquire_work_len(m, n)), dtype=torch.float64, device="cuda")
    for kind in KINDS:
        wa = _reference(gp, y, Ta, kind, mask=mask)
        wb = _reference(gp, y, Tb, kind, mask=mask)
        for parts in (4, 2, 1):
            first = _acquire(gp, y, Ta, kind, first=1, parts=parts, mask=mask, part=part, want_part=False)[0]
            second = _acquire(gp, y, Tb, kind, first=1, parts=parts, mask=mask, part=part, want_part=False)[0]
            again = _acquire(gp, y, Ta, kind, first=4, parts=parts, mask=mask, part=part, want_part=False)[0]
            assert _same(first, wa[0], wa[1]) and _same(second, wb[0], wb[1]) and again == first, (kind, parts, first, second, again)
