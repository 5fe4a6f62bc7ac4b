# -*- coding: utf-8 -*-
"""MI355X: the arg-min contract of the sweep (include/apgp.h: ties go to the lowest GLOBAL index, NaN and +inf never
win, -1 / +inf when nothing is admissible) on the device -- best_merge in every reduction stage (lane, wavefront,
workgroup partial, split last round, argmin_final_kernel's strided loop over > 1024 partials) and the 64-bit index.

Every assertion is exact and is taken against the u array the same call returned; the index-only forms
(``return_all=False``, ``device_record=True``, ``idx_offset``) against a ``return_all`` call on the same inputs.

Shapes (launch_sweep: 256 persistent workgroups x 64 candidates per round, 256-row blocks; a last round of <= 184
candidate blocks is split by row block when n > 256):  n = 1100, m = 5000: split launch only;  n = 1100, m = 40000: two
persistent rounds (rows 0 .. 32767) + 113 split blocks;  n = 200, m = 70000: 1094 partials."""
import numpy as np
import pytest

import fantasy_ref
import test_gpu_utility_epilogue as ep

pytestmark = pytest.mark.gpu

ROUND = 64 * 256                # candidates per persistent round: same lane, same workgroup slot one round later
BIG = 2 ** 33 + 5
KINDS = ("agp", "bape", "jones")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


_CACHE = {}


def _setup(n, D, m, form, seed=50):
    """A computed GP and finite, pairwise different candidates (no NaN rows, everything inside the box [-2, 2]^D)."""
    from approxposterior_amd import gp as agp
    key = (n, D, m, form, seed)
    if key not in _CACHE:
        _CACHE.clear()
        case = ep.C(n, D, m, form, 1.0, -20, 1.0, seed=seed)
        c = ep.build_case(case)
        T = c["T"]
        bad = ~np.isfinite(T).all(axis=1)
        T[bad] = 0.25
        T += 1e-6 * np.random.RandomState(seed).uniform(-1.0, 1.0, size=T.shape)      # no two rows alike
        gp = ep.make_gp(agp, case, c["ell"])
        gp.variance_mode = form
        gp.compute(c["X"])
        _CACHE[key] = (gp, c["y"], T)
    gp, y, T = _CACHE[key]
    return gp, y, T.copy()


def _record(rec):
    """(index, u) of a device apgp_best_t record (int64[2]: bit pattern of u, index)."""
    r = rec.cpu().numpy()
    return int(r[1]), float(r[0:1].view(np.float64)[0])


def _all_forms(gp, y, T, kind, want_row, want_u, **kw):
    """The winner through the tuple and the device record, without and with a 64-bit index offset."""
    for off in (0, BIG):
        want = (want_row + off if want_row >= 0 else -1, want_u)
        bi, bu = gp.acquire(y, T, kind, idx_offset=off, **kw)
        assert (bi, bu) == want, (off, bi, bu, want)
        assert _record(gp.acquire(y, T, kind, idx_offset=off, device_record=True, **kw)) == want, off
        r = gp.acquire(y, T, kind, idx_offset=off, return_all=True, **kw)
        assert (r[0], r[1]) == want


BOX = [(-2.0, 2.0)]


@pytest.mark.parametrize("n,D,m,form", [(1100, 3, 5000, "inverse"), (1100, 3, 40000, "inverse"), (200, 2, 70000, "inverse"),
                                        (1100, 3, 40000, "solve"), (200, 2, 5000, "solve")])
def test_mass_ties_go_to_the_lowest_admissible_index(n, D, m, form):
    """Jones with zeta = 1e6: every admissible utility is +-0.0.  Rows 0-2 are outside the box, rows 3-6 masked: row 7
    wins, whatever block, round or reduction stage the other m - 8 equal values sit in."""
    gp, y, T = _setup(n, D, m, form)
    T[:3, 0] = 2.5
    mask = np.ones(m, dtype=np.uint8)
    mask[3:7] = 0
    kw = dict(bounds=BOX * D, mask=mask, zeta=1e6)
    bi, bu, u, mu, var = gp.acquire(y, T, "jones", return_all=True, **kw)
    assert np.all(np.isposinf(u[:7])) and np.all(u[7:] == 0.0)
    assert (bi, bu) == (7, 0.0) and bi == fantasy_ref.argmin(u)
    _all_forms(gp, y, T, "jones", 7, 0.0, **kw)
    # and with the ties starting in the last block / the split part only
    mask[:] = 0
    first = (m - 1) // 64 * 64 - 64 * 3 + 17
    mask[first:] = 1
    kw["mask"] = mask
    bi, bu, u, _, _ = gp.acquire(y, T, "jones", return_all=True, **kw)
    assert np.all(u[first:] == 0.0) and (bi, bu) == (first, 0.0)
    _all_forms(gp, y, T, "jones", first, 0.0, **kw)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_mass_ties_in_the_fantasy_pass(form):
    gp, y, T = _setup(200, 2, 5000, form)
    m = len(T)
    T[:3, 0] = 2.5
    mask = np.ones(m, dtype=np.uint8)
    mask[3:7] = 0
    for off in (0, BIG):
        idx, ub, u, mu, var = gp.acquire_batch(y, T, "jones", 2, bounds=BOX * 2, mask=mask, zeta=1e6, idx_offset=off,
                                               return_all=True)
        assert np.all(np.isposinf(u[:7])) and np.all(u[7:] == 0.0)
        assert list(idx) == [7 + off, 7 + off] and list(ub) == [0.0, 0.0]


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_pairwise_exact_ties(form):
    """The best row duplicated at i and i + 64 * 256 k (same lane, same workgroup slot): straddling two persistent
    rounds, then the persistent / split boundary.  Where the two utilities are bit-equal (printed; DESIGN.md records
    it per form) the lower index must win with a finite, non-zero utility; in any case a pair of Jones zeros alone
    behind a mask must give the lower index."""
    n, D, m = 1100, 3, 40000
    gp, y, T0 = _setup(n, D, m, form)
    pairs = [(100, 100 + ROUND), (ROUND + 4321, 2 * ROUND + 4321), (2 * ROUND - 1, 2 * ROUND + 64 * 50 + 63)]
    for kind in ("agp", "bape"):
        r0 = gp.acquire(y, T0, kind, bounds=BOX * D)[0]
        for a, b in pairs:
            T = T0.copy()
            if r0 not in (a, b):
                T[r0] = T0[(r0 + 1) % m] if (r0 + 1) % m not in (a, b) else T0[(r0 + 3) % m]
            T[a] = T[b] = T0[r0]
            bi, bu, u, mu, var = gp.acquire(y, T, kind, bounds=BOX * D, return_all=True)
            equal = _bits(u[a]) == _bits(u[b])
            print("[%s %s] duplicated rows %d / %d: u bit-equal: %s" % (form, kind, a, b, bool(equal)))
            assert bi == fantasy_ref.argmin(u) and _bits(bu) == _bits(u[bi])
            if equal:
                assert np.isfinite(u[a]) and u[a] != 0.0 and bi == a, (kind, a, b, bi)
                _all_forms(gp, y, T, kind, a, float(u[a]), bounds=BOX * D)
    for a, b in pairs:
        mask = np.zeros(m, dtype=np.uint8)
        mask[[a, b]] = 1
        bi, bu, u, _, _ = gp.acquire(y, T0, "jones", mask=mask, zeta=1e6, return_all=True)
        assert u[a] == 0.0 and u[b] == 0.0 and (bi, bu) == (a, 0.0)
        _all_forms(gp, y, T0, "jones", a, 0.0, mask=mask, zeta=1e6)


def test_tie_across_shards():
    """Two shards merged by dist.combine_best: the lower global index lies in the split part of shard 0's call, its
    equal in the persistent part of shard 1's."""
    from approxposterior_amd import dist
    n, D = 1100, 3
    m0, m1 = ROUND + 5000, ROUND + 3000           # shard 0: one persistent round + 79 split blocks
    gp, y, T = _setup(n, D, m0 + m1, "inverse")
    a, b = ROUND + 1234, m0 + 777                 # a: split part of shard 0; b: persistent part of shard 1
    for kind, kw in (("jones", dict(zeta=1e6)), ("agp", {})):
        mask = np.zeros(m0 + m1, dtype=np.uint8)
        mask[[a, b]] = 1
        Tk = T.copy()
        Tk[b] = Tk[a]
        for off in (0, BIG):
            p0 = gp.acquire(y, Tk[:m0], kind, mask=mask[:m0], idx_offset=off, **kw)
            p1 = gp.acquire(y, Tk[m0:], kind, mask=mask[m0:], idx_offset=off + m0, **kw)
            assert p0[0] == off + a and p1[0] == off + b
            if _bits(p0[1]) != _bits(p1[1]):
                print("[shards %s] equal rows differ in the last bits between the split and the persistent part" % kind)
                continue
            for order in ((p0, p1), (p1, p0)):
                assert dist.combine_best([(u, i) for i, u in order]) == (off + a, p0[1])


PLANT_SHAPES = [(200, 2, 65 + 64 * 3, "inverse"), (1100, 3, ROUND + 64 * 79 - 63, "inverse"), (1100, 3, ROUND + 64 * 79 - 63, "solve"),
                (200, 2, 65 + 64 * 3, "solve")]


@pytest.mark.parametrize("n,D,m,form", PLANT_SHAPES)
def test_planted_winner(n, D, m, form):
    """A mask that admits exactly one row: that row wins and best_u is its u -- rows 0, 15, 16, 63, 64, m - 1 of a
    ragged last block (m % 64 == 1), the last row of the persistent part, the first and the last row of the split part
    (the inverse form at n = 1100; the solve form never splits) -- for the three utilities."""
    assert m % 64 == 1
    gp, y, T = _setup(n, D, m, form)
    rows = [0, 15, 16, 63, 64, m - 1]
    if m > ROUND:
        rows += [ROUND - 1, ROUND, m - 1]
    for kind in KINDS:
        ref = gp.acquire(y, T, kind, return_all=True)[2]
        for row in sorted(set(rows)):
            mask = np.zeros(m, dtype=np.uint8)
            mask[row] = 1
            bi, bu, u, _, _ = gp.acquire(y, T, kind, mask=mask, return_all=True)
            assert np.all(np.isposinf(np.delete(u, row))) and np.isfinite(u[row])
            assert _bits(u[row]) == _bits(ref[row])
            assert bi == row and _bits(bu) == _bits(u[row]), (kind, row, bi)
            assert gp.acquire(y, T, kind, mask=mask, idx_offset=BIG) == (BIG + row, float(u[row]))


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,m", [(200, 2, 300), (1100, 3, 5000), (1100, 3, ROUND + 700)])
def test_nothing_admissible(n, D, m, form):
    """All masked, all outside the box, all rows NaN without a box (inadmissible whatever the utility): (-1, +inf), below and above
    one round, through the record and the index offset; and through acquire_batch for that step and every later one."""
    gp, y, T = _setup(n, D, m, form)
    Tn = np.full_like(T, np.nan)
    calls = [(T, "bape", dict(mask=np.zeros(m, dtype=np.uint8))),
             (T + 10.0, "jones", dict(bounds=BOX * D)),
             (Tn, "agp", {}), (Tn, "bape", {}), (Tn, "jones", {})]
    for cand, kind, kw in calls:
        bi, bu, u, _, _ = gp.acquire(y, cand, kind, return_all=True, **kw)
        assert (bi, bu) == (-1, np.inf)
        assert not np.any(u < np.inf)
        _all_forms(gp, y, cand, kind, -1, np.inf, **kw)
        idx, ub = gp.acquire_batch(y, cand, kind, 3, **kw)
        assert list(idx) == [-1, -1, -1] and np.all(np.isposinf(ub))
    # one admissible row: step 0 takes it; it stays admissible (its fantasy variance is ~0, not a refusal), so the
    # documented -1 tail is reached through a mask that admits nothing after an empty first step only
    mask = np.zeros(m, dtype=np.uint8)
    idx, ub = gp.acquire_batch(y, T, "agp", 2, mask=mask, idx_offset=BIG)
    assert list(idx) == [-1, -1] and np.all(np.isposinf(ub))


def test_gate_edges():
    """lo and hi themselves are admissible; lo == hi admits only that value; +-inf bounds admit every finite value;
    -0.0 against a 0.0 bound is admissible; a uint8 mask admits wherever it is not 0 (2 and 255 included)."""
    n, D, m = 200, 2, 300
    gp, y, T = _setup(n, D, m, "inverse")
    T[:, :] = np.clip(T, -0.9, 0.9)
    T[10] = (-1.0, 1.0)                            # on lo / on hi
    T[11] = (np.nextafter(-1.0, -2.0), 0.0)        # one ulp outside
    T[12] = (0.0, np.nextafter(1.0, 2.0))
    box = [(-1.0, 1.0)] * D
    bi, bu, u, _, _ = gp.acquire(y, T, "agp", bounds=box, return_all=True)
    assert np.isfinite(u[10]) and np.isposinf(u[11]) and np.isposinf(u[12])
    assert np.array_equal(np.isfinite(u), fantasy_ref.admissible(T, box)) and bi == fantasy_ref.argmin(u)
    # lo == hi
    T2 = T.copy()
    T2[:, 1] = 0.3
    T2[20, 1] = np.nextafter(0.3, 1.0)
    box2 = [(-1.0, 1.0), (0.3, 0.3)]
    u = gp.acquire(y, T2, "agp", bounds=box2, return_all=True)[2]
    assert np.array_equal(np.isfinite(u), fantasy_ref.admissible(T2, box2)) and np.isposinf(u[20]) and np.isfinite(u[21])
    # infinite bounds admit every finite value
    T3 = T.copy()
    T3[30] = (1e300, -1e300)
    box3 = [(-np.inf, np.inf)] * D
    bi, bu, u, _, _ = gp.acquire(y, T3, "agp", bounds=box3, return_all=True)
    assert np.all(np.isfinite(u)) and bi == fantasy_ref.argmin(u)
    # -0.0 against a 0.0 bound
    T4 = T.copy()
    T4[40] = (-0.0, 0.5)
    T4[41] = (0.5, -0.0)
    T4[42] = (np.nextafter(0.0, -1.0), 0.5)
    box4 = [(0.0, 1.0)] * D
    u = gp.acquire(y, T4, "agp", bounds=box4, return_all=True)[2]
    assert np.isfinite(u[40]) and np.isfinite(u[41]) and np.isposinf(u[42])
    assert np.array_equal(np.isfinite(u), fantasy_ref.admissible(T4, box4))
    # mask values
    mask = np.zeros(m, dtype=np.uint8)
    mask[50], mask[51], mask[52] = 2, 255, 1
    bi, bu, u, _, _ = gp.acquire(y, T, "agp", mask=mask, return_all=True)
    assert np.array_equal(np.nonzero(np.isfinite(u))[0], [50, 51, 52]) and bi == fantasy_ref.argmin(u) and bi in (50, 51, 52)
    idx, ub, u2, _, _ = gp.acquire_batch(y, T, "agp", 2, mask=mask, return_all=True)
    assert np.array_equal(np.nonzero(np.isfinite(u2))[0], [50, 51, 52]) and idx[0] == bi and idx[1] == fantasy_ref.argmin(u2)
