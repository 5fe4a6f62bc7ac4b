# -*- coding: utf-8 -*-
"""MI355X: the pruned arg-min (csrc/sweep.hip "Pruned arg-min": bound pass, seed blocks, selection, surviving blocks
through the sweep's own kernel) returns what the full sweep returns -- index and utility as bit patterns -- and what
``argmin(u)`` of a ``return_all`` call on the same inputs gives.

``GP.sweep_prune = 2`` prunes from two candidates on (the library's own threshold would send the small shapes to the
full sweep), ``0`` is the full sweep.  Shapes: those of test_gpu_argmin_contract.py (split launch only, persistent
rounds + split blocks, > 1024 partials, ragged last block, one block) in both variance forms, and the benchmark's C3
and C2 at full size."""
import ctypes

import numpy as np
import pytest

import fantasy_ref
import test_gpu_argmin_contract as ac

pytestmark = pytest.mark.gpu

ROUND = ac.ROUND
BIG = ac.BIG
KINDS = ac.KINDS
SHAPES = [(1100, 3, 5000), (1100, 3, 40000), (200, 2, 70000), (200, 2, 5000), (200, 2, 300), (1100, 3, ROUND + 700),
          (200, 2, 65 + 64 * 3), (1100, 3, ROUND + 64 * 79 - 63)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _counts(gp):
    """(seed blocks, surviving blocks beyond the seeds, tau) of the last pruned call."""
    c = gp.last_prune_counts.cpu().numpy()
    return int(c[0]), int(c[1]), float(c[2:3].view(np.float64)[0])


def _both(gp, y, T, kind, **kw):
    """(index, u) with the switch off and on; they must agree bit for bit, through every form of the call."""
    out = {}
    for sw in (0, 2):
        gp.sweep_prune = sw
        gp.sweep_prune_stats = sw == 2
        try:
            bi, bu = gp.acquire(y, T, kind, **kw)
            ri, ru = ac._record(gp.acquire(y, T, kind, device_record=True, **kw))
            oi, ou = gp.acquire(y, T, kind, idx_offset=BIG, **kw)
        finally:
            gp.sweep_prune = None
            gp.sweep_prune_stats = False
        assert (ri, _bits(ru)) == (bi, _bits(bu))
        assert (oi, _bits(ou)) == (bi + BIG if bi >= 0 else -1, _bits(bu))
        out[sw] = (bi, bu)
    assert out[0][0] == out[2][0] and _bits(out[0][1]) == _bits(out[2][1]), (kind, out)
    return out[2]


def _against_return_all(gp, y, T, kind, **kw):
    bi, bu = _both(gp, y, T, kind, **kw)
    ri, ru, u, _, _ = gp.acquire(y, T, kind, return_all=True, **kw)
    want = fantasy_ref.argmin(u)
    assert bi == want == ri, (kind, bi, want, ri)
    if want >= 0:
        assert _bits(bu) == _bits(u[want]) == _bits(ru)
    else:
        assert np.isposinf(bu)
    return bi, bu, u


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,m", SHAPES)
def test_pruned_equals_full(n, D, m, form):
    gp, y, T = ac._setup(n, D, m, form)
    mask = np.ones(m, dtype=np.uint8)
    mask[np.random.RandomState(5).uniform(size=m) < 0.3] = 0
    Tb = T.copy()
    Tb[::7, 0] = 2.5                                # outside the box
    nblk = (m + 63) // 64
    for kind in KINDS:
        bi, bu, u = _against_return_all(gp, y, T, kind)
        ns, nv, tau = _counts(gp)
        print("[%s n=%d m=%d %s] blocks %d: %d seeds + %d survivors, tau %.17g, winner %d" % (form, n, m, kind, nblk, ns, nv, tau, bi))
        assert ns == min(16, nblk) and 0 <= nv <= nblk - ns and tau >= bu
        _against_return_all(gp, y, Tb, kind, bounds=ac.BOX * D, mask=mask)
        # the winner masked out: the runner-up, which the first call's tau may have pruned
        mask2 = np.ones(m, dtype=np.uint8)
        mask2[bi] = 0
        _against_return_all(gp, y, T, kind, mask=mask2)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_adversarial_inputs(form):
    n, D, m = 1100, 3, 40000
    gp, y, T0 = ac._setup(n, D, m, form)
    nblk = (m + 63) // 64
    X = np.asarray(gp._x, dtype=np.float64).reshape(n, D)
    for kind in KINDS:
        # all rows identical: everything ties, nothing may be pruned, row 0 wins
        T = np.repeat(T0[17:18], m, axis=0)
        bi, bu, u = _against_return_all(gp, y, T, kind)
        ns, nv, _ = _counts(gp)
        assert bi == 0 and ns + nv == nblk, (kind, bi, ns, nv)
        # the winner duplicated at a lower and at a higher index, in other blocks: the lowest wins
        r0 = gp.acquire(y, T0, kind)[0]
        lo_row, hi_row = (r0 + 64 * 37 + 5) % m, (r0 + 64 * 300 + 11) % m
        T = T0.copy()
        T[lo_row] = T[hi_row] = T0[r0]
        bi, bu, u = _against_return_all(gp, y, T, kind)
        same = [r for r in (r0, lo_row, hi_row) if _bits(u[r]) == _bits(u[r0])]
        assert bi == min(same), (kind, bi, same)
        # a candidate on a training point (var ~ 0, its bound far below its utility), alone and among the rest
        T = T0.copy()
        T[12345] = X[7]
        T[64 * 200] = X[500]
        _against_return_all(gp, y, T, kind)
        mask = np.zeros(m, dtype=np.uint8)
        mask[[12345, 64 * 200]] = 1
        _against_return_all(gp, y, T, kind, mask=mask)
        # nothing admissible
        bi, bu = _both(gp, y, T0, kind, mask=np.zeros(m, dtype=np.uint8))
        assert (bi, bu) == (-1, np.inf)
        assert _counts(gp)[:2] == (0, 0)
        bi, bu = _both(gp, y, T0 + 10.0, kind, bounds=ac.BOX * D)
        assert (bi, bu) == (-1, np.inf)
        bi, bu = _both(gp, y, np.full_like(T0, np.nan), kind)
        assert (bi, bu) == (-1, np.inf)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_flat_mean(form):
    """Constant y: alpha = 0, every mean equals the prior mean, the bound separates nothing -- every block with an
    admissible row survives and the answer is the full sweep's."""
    from approxposterior_amd import gp as agp
    n, D, m = 700, 3, 30000
    rs = np.random.RandomState(11)
    X = rs.uniform(-2, 2, size=(n, D))
    y = np.full(n, 1.5)
    T = rs.uniform(-2, 2, size=(m, D))
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 1.0), ndim=D), fit_mean=True, mean=1.5, white_noise=-12,
                fit_white_noise=False)
    gp.variance_mode = form
    gp.compute(X)
    for kind in ("agp", "bape"):
        _against_return_all(gp, y, T, kind)
        ns, nv, _ = _counts(gp)
        assert ns + nv == (m + 63) // 64


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_partial_pruning(form):
    """Between "nothing pruned" (a mean flatter than half a log of the variance) and "everything but the seeds" lies the
    case the list is for: some blocks survive.  The observations are scaled down by half decades -- the spread of the
    mean against the variance term shrinks with them -- and at least one scale must leave a surviving list that is
    neither empty nor complete; every scale must return the full sweep's winner."""
    import bench
    from approxposterior_amd import gp as agp
    n, D, m = 1100, 3, 40000
    X, y0 = bench.synthetic_c3(n, D)
    T = np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, D))
    nblk = (m + 63) // 64
    partial = 0
    for scale in (1.0, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003):
        y = y0 * scale
        gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=np.median(y),
                    white_noise=-12, fit_white_noise=False)
        gp.variance_mode = form
        gp.compute(X)
        for kind in KINDS:
            bi, bu, u = _against_return_all(gp, y, T, kind, bounds=[(-5.0, 5.0)] * D)
            ns, nv, tau = _counts(gp)
            print("[%s scale %g %s] %d blocks: %d seeds + %d survivors" % (form, scale, kind, nblk, ns, nv))
            partial += 0 < nv < nblk - ns
    assert partial >= 3


def test_select_with_a_planted_tau():
    """apgp_sweep_prune_select alone: tau = +inf keeps every block with an admissible row, tau = -inf only the blocks
    whose bound is -inf, seeds are left out, the list is ascending; against tests/prune_ref.py."""
    import torch
    import prune_ref as pr
    from approxposterior_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(9)
    for ncb in (1, 5, 1023, 1024, 1025, 15625, 70001):
        bmin = rs.normal(size=ncb)
        bmin[rs.uniform(size=ncb) < 0.2] = np.inf
        bmin[rs.uniform(size=ncb) < 0.05] = -np.inf
        bmin[rs.uniform(size=ncb) < 0.1] = 0.25                       # ties with a planted tau
        sd = pr.seeds(bmin)
        seeds = np.full(16, -1, dtype=np.int64)
        seeds[:len(sd)] = sd
        b_d = torch.from_numpy(bmin).to(dev)
        s_d = torch.from_numpy(seeds).to(dev)
        for tau in (np.inf, -np.inf, 0.25, np.nextafter(0.25, -1.0), -0.5):
            c_d = torch.tensor([len(sd), -7, 0], dtype=torch.int64, device=dev)
            l_d = torch.full((ncb,), -1, dtype=torch.int64, device=dev)
            _lib.check(lib.apgp_sweep_prune_select(b_d.data_ptr(), ncb, s_d.data_ptr(), c_d.data_ptr(), float(tau),
                                                   l_d.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "apgp_sweep_prune_select")
            torch.cuda.synchronize()
            want = pr.select(bmin, tau, sd)
            c = c_d.cpu().numpy()
            assert c[1] == len(want) and _bits(c[2:3].view(np.float64)) == _bits(tau)
            assert np.array_equal(l_d.cpu().numpy()[:len(want)], want), (ncb, tau)


@pytest.mark.parametrize("name,n,D,m,kind,form", [("C3", 4096, 8, 1000000, "agp", "inverse"),
                                                  ("C3", 4096, 8, 1000000, "agp", "solve"),
                                                  ("C2", 1024, 2, 100000, "bape", "inverse"),
                                                  ("C2", 1024, 2, 100000, "bape", "solve")])
def test_benchmark_shapes_at_full_size(name, n, D, m, kind, form):
    import torch
    import bench
    from approxposterior_amd import gp as agp
    X, y = bench.synthetic_c3(n, D)
    T = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, D))).cuda()
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                fit_white_noise=False)
    gp.variance_mode = form
    gp.compute(X)
    box = [(-5.0, 5.0)] * D
    res = {}
    for sw in (0, 1):                               # 1: the library's own threshold -- both shapes lie above it
        gp.sweep_prune = sw
        gp.sweep_prune_stats = sw == 1
        res[sw] = gp.acquire(y, T, kind, bounds=box)
        oi, ou = gp.acquire(y, T, kind, bounds=box, idx_offset=BIG)
        assert (oi - BIG, _bits(ou)) == (res[sw][0], _bits(res[sw][1]))
    ns, nv, tau = _counts(gp)
    gp.sweep_prune = None
    gp.sweep_prune_stats = False
    ri, ru, u, _, _ = gp.acquire(y, T, kind, bounds=box, return_all=True)
    print("[%s %s] %d blocks: %d seeds + %d survivors, tau %.17g, winner %d %.17g" % (name, form, (m + 63) // 64, ns, nv, tau, ri, ru))
    want = fantasy_ref.argmin(u)
    for sw in (0, 1):
        assert res[sw][0] == want == ri and _bits(res[sw][1]) == _bits(u[want]) == _bits(ru), (sw, res[sw], want)
    assert ns == 16
    if name == "C3":                                # (C2: every block holds a row whose bound is below tau, prune_ref.py)
        assert nv < 100
        if form == "inverse":
            assert (ri, ru) == (31730, -223.33178758089198)
