# -*- coding: utf-8 -*-
"""MI355X: the two-stage bound of the pruned arg-min (csrc/sweep.hip, "Coarse bound in single precision"): a bound pass
whose kernel values are fp32 over all blocks, the fp64 bound on the blocks it left at or below tau, the sweep on what
is left then.

* validity -- the property everything rests on: for every candidate row, the bound of its block (``apgp_prune_bounds``,
  coarse and fp64) lies at or below the utility a ``return_all`` sweep gives the row, as floats; +inf exactly for the
  blocks without an admissible row.  No row is left out.  The ONLY exemption from ``bound <= u``: a row whose utility
  is NaN (AGP at a variance that came out <= 0) never wins the arg-min and orders with nothing; such a row is counted,
  and must have var <= 0 -- a NaN utility at a positive variance fails the test.
* end to end: index and utility of the pruned call equal the full sweep's and ``return_all``'s as bit patterns
  (test_gpu_sweep_prune's helpers), and the four counters are consistent.  These inputs hold blocks without an
  admissible row, which cannot be seeds: counts[0] == min(16, blocks with an admissible row) there, and
  counts[0] == min(16, nblk) on the same shapes with every row admissible (test_counts_without_inadmissible_blocks).
* the refine stage removes blocks the coarse stage kept in at least one configuration.
* with a LinearKernel term the coarse stage is not used.
* the one-pass seed kernel against tests/prune_ref.py.
* C3 at full size.

Inputs: ``bench.synthetic_c3`` with y scaled by 1, 1e-2, 1e-4 (the last leaves almost no gap between bound and
utility); training set and candidates shifted by +1e4 in every coordinate (fp32 coordinates without centring would be
useless); one metric of 1e-3 (far kernel values underflow in fp32); a candidate on a training point; rows outside the
box, masked rows, NaN rows.  Shapes: one block of rows per tile and several, D = 2, 3, 8, a ragged last block."""
import ctypes

import numpy as np
import pytest

import prune_ref as pr
import test_gpu_sweep_prune as sp

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
SHAPES = [(130, 2, 5000), (1100, 3, 40000), (1100, 8, 20000), (300, 8, 70)]
# (name, y scale, shift of every coordinate, metric of dimension 0)
INPUTS = [("y*1", 1.0, 0.0, 8.0), ("y*1e-2", 1e-2, 0.0, 8.0), ("y*1e-4", 1e-4, 0.0, 8.0), ("shift+1e4", 1.0, 1e4, 8.0),
          ("shift+1e4,y*1e-2", 1e-2, 1e4, 8.0), ("metric1e-3", 1.0, 0.0, 1e-3)]


def _case(n, D, m, scale, shift, metric0, form, lin=False):
    """A computed GP on bench.synthetic_c3's data, candidates with every kind of inadmissible row, the box and a mask."""
    import bench
    from approxposterior_amd import gp as agp
    X, y = bench.synthetic_c3(n, D)
    y = y * scale
    rs = np.random.RandomState(1)
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    T[m // 2] = X[7]                                # on a training point
    T[5::7, 0] = 5.5                                # outside the box
    T[3::11, D - 1] = np.nan
    mask = np.ones(m, dtype=np.uint8)
    mask[rs.uniform(size=m) < 0.3] = 0
    if m > 64 * 9:
        T[64 * 3:64 * 4, 0] = -5.5                  # whole blocks without an admissible row: box, mask, NaN
        mask[64 * 5:64 * 6] = 0
        T[64 * 8:64 * 9, 1] = np.nan
    X = X + shift
    T = T + shift
    metric = np.full(D, 8.0)
    metric[0] = metric0
    k = agp.ExpSquaredKernel(metric, ndim=D)
    if lin:
        k = k + 0.3 * agp.kernels.LinearKernel(log_gamma2=0.4, order=2, bounds=None, ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
    gp.variance_mode = form
    gp.compute(X)
    box = [(-5.0 + shift, 5.0 + shift)] * D
    adm = np.all((T >= -5.0 + shift) & (T <= 5.0 + shift), axis=1) & (mask != 0)       # (a NaN compares false)
    return gp, y, T, box, mask, adm


def _check_bounds(tag, bmin, u, var, adm):
    m = len(u)
    nblk = (m + 63) // 64
    assert bmin.shape == (nblk,) and not np.isnan(bmin).any(), tag
    has = np.zeros(nblk * 64, dtype=bool)
    has[:m] = adm
    assert np.array_equal(np.isposinf(bmin), ~has.reshape(nblk, 64).any(axis=1)), tag
    assert np.all(np.isposinf(u[~adm])), tag
    per_row = np.repeat(bmin, 64)[:m]
    nan = np.isnan(u)
    assert not np.any(nan & ~(var <= 0.0)), tag     # the only NaN utilities: a variance that came out <= 0
    bad = ~nan & ~(per_row <= u)
    fin = adm & ~nan & np.isfinite(u)
    gap = np.min((u - per_row)[fin]) if np.any(fin) else np.inf
    print("[%s] %d blocks, %d rows, %d NaN utilities, smallest u - bound %.3g" % (tag, nblk, m, int(nan.sum()), gap))
    assert not bad.any(), (tag, np.nonzero(bad)[0][:5], per_row[bad][:5], u[bad][:5])


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,m", SHAPES)
def test_bounds_are_valid_and_the_pruned_call_is_the_full_sweep(n, D, m, form):
    nblk = (m + 63) // 64
    for name, scale, shift, metric0 in INPUTS:
        gp, y, T, box, mask, adm = _case(n, D, m, scale, shift, metric0, form)
        for kind in KINDS:
            tag = "%s n=%d D=%d m=%d %s %s" % (form, n, D, m, name, kind)
            kw = dict(bounds=box, mask=mask)
            bi, bu, u = sp._against_return_all(gp, y, T, kind, **kw)
            c = gp.last_prune_counts.cpu().numpy()
            print("[%s] seeds %d, coarse kept %d, survivors %d, winner %d" % (tag, c[0], c[3], c[1], bi))
            nadm = int(np.isfinite(gp.prune_bounds(y, T, kind, coarse=False, **kw)).sum())
            assert c[0] == min(16, nadm) and 0 <= c[1] <= c[3] <= nblk - c[0], (tag, c)
            _, _, _, _, var = gp.acquire(y, T, kind, return_all=True, **kw)
            for coarse in (True, False):
                bmin = gp.prune_bounds(y, T, kind, coarse=coarse, **kw)
                _check_bounds(tag + (" coarse" if coarse else " fp64"), bmin, u, var, adm)


def test_counts_without_inadmissible_blocks():
    """counts[0] == min(16, nblk) when every block has an admissible row, the ragged one included."""
    for n, D, m in SHAPES:
        gp, y, T, box, mask, adm = _case(n, D, m, 1.0, 0.0, 8.0, "inverse")
        T = np.clip(np.nan_to_num(T, nan=0.5), -5.0, 5.0)
        nblk = (m + 63) // 64
        for kind in KINDS:
            sp._against_return_all(gp, y, T, kind, bounds=box)
            c = gp.last_prune_counts.cpu().numpy()
            assert c[0] == min(16, nblk) and 0 <= c[1] <= c[3] <= nblk - c[0], (n, D, m, kind, c)


def test_refine_stage_does_work():
    """Some configuration must show counts[1] < counts[3]: the fp64 bound removed blocks the coarse one kept."""
    refined = []                                    # its own calls: the shifted and scaled cases of one shape
    n, D, m = SHAPES[1]
    for name, scale, shift, metric0 in INPUTS[:5]:                     # y scaled by 1, 1e-2, 1e-4; shifted
        gp, y, T, box, mask, adm = _case(n, D, m, scale, shift, metric0, "inverse")
        for kind in KINDS:
            sp._against_return_all(gp, y, T, kind, bounds=box, mask=mask)
            c = gp.last_prune_counts.cpu().numpy()
            refined.append(("inverse n=%d D=%d m=%d %s %s" % (n, D, m, name, kind), int(c[1]), int(c[3])))
    hits = [r for r in refined if r[1] < r[2]]
    for tag, nv, na in refined:
        print("[%s] coarse kept %d, survivors %d" % (tag, na, nv))
    assert hits, "no configuration in which the refine stage removed a block"


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_linear_term_takes_the_fp64_bound_alone(form):
    n, D, m = 1100, 3, 40000
    gp, y, T, box, mask, adm = _case(n, D, m, 1.0, 0.0, 8.0, form, lin=True)
    for kind in KINDS:
        bi, bu, u = sp._against_return_all(gp, y, T, kind, bounds=box, mask=mask)
        c = gp.last_prune_counts.cpu().numpy()
        print("[lin %s %s] seeds %d, survivors %d (list A %d), winner %d" % (form, kind, c[0], c[1], c[3], bi))
        assert c[3] == c[1]
        _, _, _, _, var = gp.acquire(y, T, kind, return_all=True, bounds=box, mask=mask)
        _check_bounds("lin %s %s fp64" % (form, kind), gp.prune_bounds(y, T, kind, coarse=False, bounds=box, mask=mask),
                      u, var, adm)
    from approxposterior_amd import _lib
    with pytest.raises(_lib.ApgpError):
        gp.prune_bounds(y, T, "agp", coarse=True, bounds=box, mask=mask)


def test_seed_kernel():
    """apgp_sweep_prune_seeds alone: planted ties, +-inf, fewer than 16 finite entries; against prune_ref.seeds."""
    import torch
    from approxposterior_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(3)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ncb in (1, 5, 1023, 1025, 15625):
        arrays = []
        b = rs.normal(size=ncb)
        b[rs.uniform(size=ncb) < 0.2] = np.inf
        b[rs.uniform(size=ncb) < 0.01] = -np.inf
        arrays.append(b)
        b = np.round(rs.normal(size=ncb), 1)                          # ties everywhere, the smallest values included
        b[rs.uniform(size=ncb) < 0.3] = b.min()
        arrays.append(b)
        arrays.append(np.full(ncb, -np.inf))                          # all equal: the first 16 block numbers
        arrays.append(np.full(ncb, np.inf))                           # nothing admissible
        b = np.full(ncb, np.inf)                                      # fewer than 16 below +inf, at the far end too
        b[rs.choice(ncb, size=min(ncb, 7), replace=False)] = rs.normal(size=min(ncb, 7))
        b[ncb - 1] = 0.5
        arrays.append(b)
        b = rs.normal(size=ncb)                                       # the 16 smallest in ONE thread's strided share
        b[::1024] = -10.0 - np.arange(len(b[::1024]))
        arrays.append(b)
        for k, bmin in enumerate(arrays):
            want = pr.seeds(bmin)
            b_d = torch.from_numpy(bmin).to(dev)
            s_d = torch.full((16,), -5, dtype=torch.int64, device=dev)
            c_d = torch.full((4,), -7, dtype=torch.int64, device=dev)
            _lib.check(lib.apgp_sweep_prune_seeds(b_d.data_ptr(), ncb, s_d.data_ptr(), c_d.data_ptr(), st),
                       "apgp_sweep_prune_seeds")
            torch.cuda.synchronize()
            c = c_d.cpu().numpy()
            assert c[0] == len(want) and c[1] == 0 and c[3] == 0, (ncb, k, c, want)
            assert np.array_equal(s_d.cpu().numpy()[:len(want)], want), (ncb, k, s_d.cpu().numpy(), want)


def test_c3_at_full_size():
    import torch
    import bench
    from approxposterior_amd import gp as agp
    n, D, m = 4096, 8, 1000000
    X, y = bench.synthetic_c3(n, D)
    T = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, D))).cuda()
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                fit_white_noise=False)
    gp.compute(X)
    gp.sweep_prune = 1
    gp.sweep_prune_stats = True
    bi, bu = gp.acquire(y, T, "agp", bounds=[(-5.0, 5.0)] * D)
    c = gp.last_prune_counts.cpu().numpy()
    print("[C3] seeds %d, coarse kept %d, survivors %d, tau %.17g, winner %d %.17g"
          % (c[0], c[3], c[1], float(c[2:3].view(np.float64)[0]), bi, bu))
    assert c[0] == 16 and c[3] < 100 and c[1] <= c[3]
    assert (bi, bu) == (31730, -223.33178758089198)
