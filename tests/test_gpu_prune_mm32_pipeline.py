# -*- coding: utf-8 -*-
"""MI355X: the matrix-core coarse bound (csrc/prune_mm32.h) at the shapes where its loop structure can go wrong -- the
two-sided check of test_gpu_prune_mm32.test_row_mapping, b - 2 slack <= bmin <= b against prune_mm32_ref.replay, with one
live row per block so that every bmin IS one row's bound:

* n = 1, 32, 33, 96, 128, 129, 160, 257: one 32-row matrix tile, the tile boundary, three of the four tiles of an LDS
  tile, exactly one LDS tile, one and two LDS tiles plus a partial one.  A row tile that is dropped, taken twice or read
  from the wrong LDS tile moves mu by that tile's share, far outside two slacks.  The sum of |alpha| in the slack is
  gathered by the staging lanes, once per row and workgroup: rows it misses make the slack too small, and bmin rises
  above b as soon as the fp32 error exceeds what is left; rows counted per tile or per wavefront again make it too large
  by a factor that the lower side, b - 2 slack <= bmin, does not allow.
* D = 1 and 8 (Dpad 2 and 8: KH = 2 and 5 product steps, with and without a remainder behind the 16-byte reads).
* m = 1, 64, 65, 257, 513: one row, one block, a block with one row, a partial last block in the second and third
  wavefront, a second workgroup with one live row.
* the live row on lanes 0, 31, 32, 63: both 32-candidate groups of a block, both ends.

Tolerance: none of its own -- the slack is the kernel's documented error budget, replayed term by term."""
import numpy as np
import pytest

import prune_mm32_ref as mm
import prune_ref as pr
import test_gpu_prune_mm32 as base
import util_ref

pytestmark = pytest.mark.gpu

NS = [1, 32, 33, 96, 128, 129, 160, 257]
DS = [1, 8]
MS = [1, 64, 65, 257, 513]
LANES = [0, 31, 32, 63]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_one_live_row_per_block(D, n):
    gp, y, T_all, box, _, _, metric = base._case(n, D, max(MS), "inverse", plain=True)
    sc = np.sqrt(0.5 / metric)
    ybest = float(np.max(y))
    mean = float(gp.mean.value)
    dpad = mm.dpad_of(D)
    checked = 0
    for m in MS:
        T = np.ascontiguousarray(T_all[:m])
        ncb = (m + 63) // 64
        for kept in LANES:
            rows = np.arange(ncb) * 64 + kept
            rows = rows[rows < m]
            mask = np.zeros(m, dtype=np.uint8)
            mask[rows] = 1
            r = None
            for kind in base.KINDS:
                bmin = gp.prune_bounds(y, T, kind, coarse=True, bounds=box, mask=mask)
                assert len(bmin) == ncb
                dead = np.ones(ncb, dtype=bool)
                dead[rows // 64] = False
                assert np.all(bmin[dead] == np.inf), (n, D, m, kept, kind, bmin)
                if len(rows) == 0:
                    continue
                if r is None:                            # the packed stream as the device holds it: scaled rows | alpha | 0
                    xs = gp._xs.cpu().numpy().reshape(-1, dpad + 2)
                    r = mm.replay(xs[:n, :D], xs[:n, dpad].copy(), T[rows], sc, amp=1.0, xs=xs[:n, :D])
                    assert r["gate"].all()
                mu = r["mu"] + mean
                one = np.ones(len(rows))
                b = pr.row_bounds(kind, mu, 1.0, r["S"], np.ones(len(rows), dtype=bool), n, dpad, 0.01, ybest)
                b0 = util_ref.f64(kind, mu, one, 0.01, ybest)
                sl = mm.slack(kind, b0, mu, 1.0, r, 0.01, ybest)
                got = bmin[rows // 64]
                print("[n=%d D=%d m=%d lane %d %s] (b - bmin) / slack in [%.3g, %.3g]"
                      % (n, D, m, kept, kind, ((b - got) / sl).min(), ((b - got) / sl).max()))
                assert np.all(got <= b) and np.all(b - 2.0 * sl <= got), (n, D, m, kept, kind, got, b, sl)
                checked += len(rows)
    assert checked > 0
