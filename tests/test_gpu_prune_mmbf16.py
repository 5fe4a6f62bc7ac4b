# -*- coding: utf-8 -*-
"""MI355X: the coarse bound with its exponents on the bf16 matrix cores (csrc/prune_mm32.h) against the NumPy replay of
tests/prune_mmbf16_ref.py, which forms every exponent under the measured model of v_mfma_f32_32x32x16_bf16 and the slack
term by term.

* shapes, the smallest at which the tiling can go wrong: n = 1, 31, 33 (below and above one 32-row matrix tile), 130 (one
  LDS tile and a partial one), 513 (past the packed stream's 512-row padding); D = 1, 2, 3, 8 (Dpad 2, 4, 8: two, three
  and four instructions per tile); m = 1, 33, 64, 70, 513 (a second and third workgroup with one live row).
* two-sided: every row of a block masked but one, the kept row on lanes 0, 31, 32 and 63: b - 2 slack <= bmin <= b with b
  the fp64 bound of that row from the exact mu.  Blocks without an admissible row give +inf exactly.
* k slots: training sets and candidates that differ from c in exactly ONE coordinate, every coordinate in turn, with
  mantissas chosen so that even the products of the low parts exceed the slack (prune_mmbf16_ref.one_coordinate_case):
  a product that is lost, or stands in a wrong slot, on either side, leaves the two-sided window --
  tests/test_prune_mmbf16_ref.py shows it for each of them on these very inputs.
* gate failure (metric 1e-3 in dimension 0): the bounds of admissible blocks are finite -- the vector-ALU kernel ran for
  them -- and valid, and the winner is the full sweep's.
* the pruned winner is the full sweep's, bit for bit (test_gpu_sweep_prune._against_return_all), all three utilities.

Tolerance: none of its own -- the slack is the kernel's documented error budget."""
import numpy as np
import pytest

import prune_mmbf16_ref as bf
import prune_ref as pr
import test_gpu_prune_coarse as pc
import test_gpu_prune_mm32 as base
import test_gpu_sweep_prune as sp
import util_ref

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
NS = [1, 31, 33, 130, 513]
DS = [1, 2, 3, 8]
MS = [1, 33, 64, 70, 513]
LANES = [0, 31, 32, 63]


def _check_rows(tag, gp, y, T, rows, mask, box, n, D, sc):
    """b - 2 slack <= bmin <= b for the one live row of each block in rows; +inf for the other blocks.  Returns the
    number of rows checked."""
    m = len(T)
    ncb = (m + 63) // 64
    dpad = bf.dpad_of(D)
    ybest = float(np.max(y))
    mean = float(gp.mean.value)
    r = None
    for kind in KINDS:
        bmin = gp.prune_bounds(y, T, kind, coarse=True, bounds=box, mask=mask)
        assert len(bmin) == ncb
        dead = np.ones(ncb, dtype=bool)
        dead[rows // 64] = False
        assert np.all(bmin[dead] == np.inf), (tag, kind, bmin)
        if len(rows) == 0:
            continue
        if r is None:                                    # the packed stream as the device holds it: scaled rows | alpha | 0
            xs = gp._xs.cpu().numpy().reshape(-1, dpad + 2)
            r = bf.replay(xs[:n, :D], xs[:n, dpad].copy(), T[rows], sc, amp=1.0, xs=xs[:n, :D])
            assert r["gate"].all(), tag
        mu = r["mu"] + mean
        b = pr.row_bounds(kind, mu, 1.0, r["S"], np.ones(len(rows), dtype=bool), n, dpad, 0.01, ybest)
        b0 = util_ref.f64(kind, mu, np.ones(len(rows)), 0.01, ybest)
        sl = bf.slack(kind, b0, mu, 1.0, r, 0.01, ybest)
        got = bmin[rows // 64]
        print("[%s %s] (b - bmin) / slack in [%.3g, %.3g]" % (tag, kind, ((b - got) / sl).min(), ((b - got) / sl).max()))
        assert np.all(got <= b) and np.all(b - 2.0 * sl <= got), (tag, kind, got, b, sl)
    return len(rows)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_one_live_row_per_block(D, n):
    gp, y, T_all, box, _, _, metric = base._case(n, D, max(MS), "inverse", plain=True)
    sc = np.sqrt(0.5 / metric)
    checked = 0
    for m in MS:
        T = np.ascontiguousarray(T_all[:m])
        for kept in LANES:
            rows = np.arange((m + 63) // 64) * 64 + kept
            rows = rows[rows < m]
            mask = np.zeros(m, dtype=np.uint8)
            mask[rows] = 1
            checked += _check_rows("n=%d D=%d m=%d lane %d" % (n, D, m, kept), gp, y, T, rows, mask, box, n, D, sc)
    assert checked > 0


@pytest.mark.parametrize("D", DS)
def test_one_coordinate_sets(D):
    from approxposterior_amd import gp as agp
    metric = np.full(D, bf.ONE_METRIC)
    sc = np.sqrt(0.5 / metric)
    box = [(-5.0, 5.0)] * D
    for d in range(D):
        X, y, Tc = bf.one_coordinate_case(D, d)
        gp = agp.GP(kernel=agp.ExpSquaredKernel(metric, ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                    fit_white_noise=False)
        gp.variance_mode = "inverse"
        gp.compute(X)
        # candidate i is the one live row of block i, on the lanes in turn; the other rows are copies of c, masked
        m = 64 * len(Tc)
        T = np.tile(X[0], (m, 1))
        rows = np.arange(len(Tc)) * 64 + np.array([LANES[i % 4] for i in range(len(Tc))])
        T[rows] = Tc
        mask = np.zeros(m, dtype=np.uint8)
        mask[rows] = 1
        assert _check_rows("one coordinate D=%d d=%d" % (D, d), gp, y, T, rows, mask, box, len(X), D, sc) == len(Tc)


def test_gate_failure_ends_in_finite_valid_bounds():
    n, D, m = 130, 2, 5000
    gp, y, T, box, mask, adm, _ = base._case(n, D, m, "inverse", metric0=1e-3)
    kw = dict(bounds=box, mask=mask)
    for kind in KINDS:
        tag = "gate %s" % kind
        sp._against_return_all(gp, y, T, kind, **kw)
        _, _, u, _, var = gp.acquire(y, T, kind, return_all=True, **kw)
        bmin = gp.prune_bounds(y, T, kind, coarse=True, **kw)
        pc._check_bounds(tag, bmin, u, var, adm)
        has = np.zeros(len(bmin) * 64, dtype=bool)
        has[:m] = adm
        assert np.all(np.isfinite(bmin[has.reshape(-1, 64).any(axis=1)])), tag


@pytest.mark.parametrize("n", [33, 513])
@pytest.mark.parametrize("D", DS)
def test_the_pruned_winner_is_the_full_sweeps(D, n):
    for m in (70, 513):
        gp, y, T, box, mask, adm, _ = base._case(n, D, m, "inverse")
        kw = dict(bounds=box, mask=mask)
        for kind in KINDS:
            _, _, u = sp._against_return_all(gp, y, T, kind, **kw)
            _, _, _, _, var = gp.acquire(y, T, kind, return_all=True, **kw)
            pc._check_bounds("n=%d D=%d m=%d %s" % (n, D, m, kind), gp.prune_bounds(y, T, kind, coarse=True, **kw), u, var, adm)
