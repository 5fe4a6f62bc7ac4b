# -*- coding: utf-8 -*-
"""MI355X: the coarse bound with its exponents on the fp32 matrix cores (csrc/prune_mm32.h) and the vector-ALU kernel
launched behind it for the blocks whose gate failed.

* shapes, the smallest at which the tiling can go wrong: n below and above one 32-row matrix tile (1, 31, 33), one LDS
  tile (130) and the packed stream's 512-row padding (513); D = 1, 2, 3, 8 (Dpad 16 keeps the vector-ALU kernel);
  m = 1, 33, 64, 70 and B + 1 with B = 512 candidate rows per workgroup -- a second workgroup with one live row.
* row mapping: every row of a block masked but one, the kept row on lanes 0, 31, 32 and 63: b - 2 slack <= bmin <= b with
  b the fp64 NumPy bound of that row (prune_ref.row_bounds) and slack from prune_mm32_ref -- two-sided, so a kernel
  that drops rows 32..63 or swaps the halves fails where ``bound <= u`` alone would pass.
* validity and end to end: test_gpu_prune_coarse._check_bounds and test_gpu_sweep_prune._against_return_all over the
  shapes, all three utilities, both variance forms; blocks without an admissible row give +inf exactly.
* gate failure (metric 1e-3 in dimension 0): the coarse bounds of admissible blocks are finite -- the vector-ALU kernel
  ran for them --, valid, and the winner is the full sweep's.
* prune quality: "coarse kept" (counts[3]) per configuration of test_gpu_prune_coarse.SHAPES[1] is not above what the
  parent commit's vector-ALU kernel kept, measured once on the parent (PARENT_KEPT)."""
import numpy as np
import pytest

import prune_mm32_ref as mm
import prune_ref as pr
import test_gpu_prune_coarse as pc
import test_gpu_sweep_prune as sp
import util_ref

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
WG_ROWS = 512                                       # candidate rows per workgroup: 4 wavefronts x PMM_G / 2 blocks x 64
NS = [1, 31, 33, 130, 513]
DS = [1, 2, 3, 8]
MS = [1, 33, 64, 70, WG_ROWS + 1]

# "coarse kept" of the parent commit (prune_bound32_kernel alone) on SHAPES[1] = (1100, 3, 40000), variance form
# "inverse", test_gpu_prune_coarse.INPUTS[:5] x (agp, bape, jones): profiles/r13_parent_coarse_kept.txt.  606 is every
# block that is neither a seed nor without an admissible row: on this ill-conditioned fit the parent's coarse stage
# prunes nothing, so the table can only catch a count that is wrong, not a bound that is looser.
PARENT_KEPT = {
    ("y*1", "agp"): 606,
    ("y*1", "bape"): 606,
    ("y*1", "jones"): 606,
    ("y*1e-2", "agp"): 606,
    ("y*1e-2", "bape"): 606,
    ("y*1e-2", "jones"): 606,
    ("y*1e-4", "agp"): 606,
    ("y*1e-4", "bape"): 606,
    ("y*1e-4", "jones"): 606,
    ("shift+1e4", "agp"): 606,
    ("shift+1e4", "bape"): 606,
    ("shift+1e4", "jones"): 606,
    ("shift+1e4,y*1e-2", "agp"): 606,
    ("shift+1e4,y*1e-2", "bape"): 606,
    ("shift+1e4,y*1e-2", "jones"): 606,
}


def _case(n, D, m, form, metric0=8.0, plain=False):
    """test_gpu_prune_coarse._case for any n and m >= 1 (its rows 7 and m // 2 need n >= 8); plain: every row admissible."""
    import bench
    from approxposterior_amd import gp as agp
    X, y = bench.synthetic_c3(n, D)
    rs = np.random.RandomState(1)
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    T[m // 2] = X[min(7, n - 1)]                    # on a training point
    mask = np.ones(m, dtype=np.uint8)
    if not plain:
        T[5::7, 0] = 5.5                            # outside the box
        T[3::11, D - 1] = np.nan
        mask[rs.uniform(size=m) < 0.3] = 0
    metric = np.full(D, 8.0)
    metric[0] = metric0
    gp = agp.GP(kernel=agp.ExpSquaredKernel(metric, ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                fit_white_noise=False)
    gp.variance_mode = form
    gp.compute(X)
    box = [(-5.0, 5.0)] * D
    adm = np.all((T >= -5.0) & (T <= 5.0), axis=1) & (mask != 0)
    return gp, y, T, box, mask, adm, metric


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_bounds_are_valid_and_the_pruned_call_is_the_full_sweep(D, n, form):
    for m in MS:
        gp, y, T, box, mask, adm, _ = _case(n, D, m, form)
        kw = dict(bounds=box, mask=mask)
        for kind in KINDS:
            tag = "%s n=%d D=%d m=%d %s" % (form, n, D, m, kind)
            bi, bu, u = sp._against_return_all(gp, y, T, kind, **kw)
            _, _, _, _, var = gp.acquire(y, T, kind, return_all=True, **kw)
            pc._check_bounds(tag + " coarse", gp.prune_bounds(y, T, kind, coarse=True, **kw), u, var, adm)


@pytest.mark.parametrize("n,D", [(33, 2), (130, 2), (513, 3), (130, 8)])
def test_row_mapping(n, D):
    """One live row per block, on lanes 0, 31, 32, 63 of its block, in blocks 0 .. 8 (both 32-candidate groups of a
    block, every block of a wavefront, a second workgroup)."""
    nblk = 9
    m = 64 * nblk
    gp, y, T, box, _, _, metric = _case(n, D, m, "inverse", plain=True)
    sc = np.sqrt(0.5 / metric)
    ybest = float(np.max(y))
    for kept in (0, 31, 32, 63):
        mask = np.zeros(m, dtype=np.uint8)
        rows = np.arange(nblk) * 64 + (kept + np.arange(nblk) * 0)
        mask[rows] = 1
        for kind in KINDS:
            bmin = gp.prune_bounds(y, T, kind, coarse=True, bounds=box, mask=mask)
            # the packed stream as the device holds it: scaled rows | alpha | 0
            dpad = mm.dpad_of(D)
            xs = gp._xs.cpu().numpy().reshape(-1, dpad + 2)
            r = mm.replay(xs[:n, :D], xs[:n, dpad].copy(), T[rows], sc, amp=1.0, xs=xs[:n, :D])
            assert r["gate"].all()
            mean = float(gp.mean.value)
            mu = r["mu"] + mean
            b = pr.row_bounds(kind, mu, 1.0, r["S"], np.ones(nblk, dtype=bool), n, dpad, 0.01, ybest)
            b0 = util_ref.f64(kind, mu, np.ones(nblk), 0.01, ybest)
            sl = mm.slack(kind, b0, mu, 1.0, r, 0.01, ybest)
            print("[n=%d D=%d lane %d %s] (b - bmin) / slack in [%.3g, %.3g]"
                  % (n, D, kept, kind, ((b - bmin) / sl).min(), ((b - bmin) / sl).max()))
            assert np.all(bmin <= b) and np.all(b - 2.0 * sl <= bmin), (n, D, kept, kind, bmin, b, sl)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_gate_failure_goes_to_the_vector_kernel(form):
    n, D, m = 130, 2, 5000
    gp, y, T, box, mask, adm, _ = _case(n, D, m, form, metric0=1e-3)
    kw = dict(bounds=box, mask=mask)
    for kind in KINDS:
        tag = "gate %s %s" % (form, kind)
        bi, bu, u = sp._against_return_all(gp, y, T, kind, **kw)
        _, _, _, _, var = gp.acquire(y, T, kind, return_all=True, **kw)
        bmin = gp.prune_bounds(y, T, kind, coarse=True, **kw)
        pc._check_bounds(tag, bmin, u, var, adm)
        has = np.zeros(len(bmin) * 64, dtype=bool)
        has[:m] = adm
        assert np.all(np.isfinite(bmin[has.reshape(-1, 64).any(axis=1)])), tag


def test_prune_quality_against_the_parent():
    n, D, m = pc.SHAPES[1]
    worse = []
    for name, scale, shift, metric0 in pc.INPUTS[:5]:
        gp, y, T, box, mask, adm = pc._case(n, D, m, scale, shift, metric0, "inverse")
        for kind in KINDS:
            sp._against_return_all(gp, y, T, kind, bounds=box, mask=mask)
            c = gp.last_prune_counts.cpu().numpy()
            print("[%s %s] coarse kept %d (parent %d), survivors %d" % (name, kind, c[3], PARENT_KEPT[(name, kind)], c[1]))
            if c[3] > PARENT_KEPT[(name, kind)]:
                worse.append((name, kind, int(c[3]), PARENT_KEPT[(name, kind)]))
    assert not worse, worse
