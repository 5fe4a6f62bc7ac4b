# -*- coding: utf-8 -*-
"""MI355X: the coarse prune bound with its training rows split into bf16 parts once per fit (apgp_pack_prune_rows and the
entry points that take the stream; csrc/prune_mm32.h; DESIGN.md sections 3 and 4).

* stream image: apgp_pack_prune_rows against the NumPy restatement tests/prune_rows_ref.py (built from
  prune_mmbf16_ref.split / slots), every bf16 value and every fp32 alpha bit for bit, the rows of the padding and the
  position of the pad columns included (the pad's content is free); n = 1, 31, 33, 127, 128, 129, 513 (below, at and
  past one 32-row matrix tile, one 128-row tile, the packed stream's 512-row padding), D = 1, 2, 3, 4, 8 (Dpad 2, 4, 8).
  Header: sum |alpha| within n 2^-53 relative of math.fsum (n fp64 additions of positive terms), bm2 within 4 ulp of
  NumPy's (the kernel's fma chain and NumPy's sum of rounded squares differ by at most Dpad / 2 + 1 roundings each).
* route equality: apgp_prune_bounds_rows(coarse = 1) with the stream equals apgp_prune_bounds(coarse = 1), which splits
  the rows in every workgroup, in every block, bit for bit: n = 1, 33, 128, 129, 257, 513, 641 (one, two, three and five
  tiles, both buffer parities, the last tile full or partial), m = 1, 64, 70, 513, 1025 (one workgroup and several, a
  ragged last block), D = 1, 3, 8, all three utilities, with a box, a mask and NaN candidates; and one case whose gate
  fails (data far wider than the length scale), which reaches the -inf mark and the kernel behind it.
* the pruned apgp_acquire_rows (switch value 2) leaves the best record and the four counts of apgp_acquire, bit for bit,
  and its winner is the full sweep's.
* refit: on one GP, a new y and then a new kernel vector; the pruned winner is the full sweep's each time, and the stream
  the GP holds is the one a fresh pack of its current rows gives.

Tolerance: none beyond the two header bounds above."""
import ctypes
import math

import numpy as np
import pytest

import prune_mmbf16_ref as bf
import prune_rows_ref as rr
import test_gpu_prune_mm32 as base
import test_gpu_sweep_prune as sp

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
IMAGE_NS = [1, 31, 33, 127, 128, 129, 513]
IMAGE_DS = [1, 2, 3, 4, 8]
NS = [1, 33, 128, 129, 257, 513, 641]
MS = [1, 64, 70, 513, 1025]
DS = [1, 3, 8]


def _rt():
    import torch
    from approxposterior_amd import _lib
    return torch, _lib, _lib.load()


def _kernel_struct(_lib, D, metric=8.0):
    ks = _lib.KernelStruct()
    ks.ndim = D
    ks.amp = 1.0
    for d in range(D):
        ks.inv_metric[d] = 1.0 / metric
    return ks


def _pack(torch, _lib, lib, xs_d, n, ks):
    rows = torch.full((int(lib.apgp_prune_rows_len(n, ks.ndim)),), np.nan, dtype=torch.float64, device="cuda")
    _lib.check(lib.apgp_pack_prune_rows(xs_d.data_ptr(), n, ctypes.byref(ks), rows.data_ptr(), None),
               "apgp_pack_prune_rows")
    torch.cuda.synchronize()
    return rows


@pytest.mark.parametrize("n", IMAGE_NS)
@pytest.mark.parametrize("D", IMAGE_DS)
def test_stream_image(D, n):
    torch, _lib, lib = _rt()
    rs = np.random.RandomState(100 * D + n)
    X = rs.uniform(-5.0, 5.0, size=(n, D))
    alpha = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 6, size=n)
    ks = _kernel_struct(_lib, D)
    dpad = bf.dpad_of(D)
    xs_d = torch.empty(int(lib.apgp_packed_train_len(n, D)), dtype=torch.float64, device="cuda")
    _lib.check(lib.apgp_pack_train(torch.from_numpy(X).cuda().data_ptr(), torch.from_numpy(alpha).cuda().data_ptr(), n,
                                   ctypes.byref(ks), xs_d.data_ptr(), None), "apgp_pack_train")
    rows = _pack(torch, _lib, lib, xs_d, n, ks)
    xs = xs_d.cpu().numpy().reshape(-1, dpad + 2)
    assert len(rows) == rr.length(n, dpad)
    bm2, sal, image, alphas = rr.parse(rows.cpu().numpy(), n, dpad)
    want_image, want_alphas, checked = rr.layout(xs, n, dpad)
    assert image.shape == want_image.shape and alphas.shape == want_alphas.shape
    bad = np.argwhere(image[:, :, checked] != want_image[:, :, checked])
    assert len(bad) == 0, ("first differing (tile, row, slot)", bad[:4], n, D)
    assert np.array_equal(alphas.view(np.uint32), want_alphas.view(np.uint32))
    want_bm2, want_sal = rr.header(xs, n, dpad)
    print("[n=%d D=%d] sal rel %.3g of n eps, bm2 %.3g ulp" % (
        n, D, abs(sal - want_sal) / max(want_sal, 1e-300) / (n * 2.0 ** -53),
        abs(bm2 - want_bm2) / max(np.spacing(want_bm2), 5e-324)))
    assert abs(sal - want_sal) <= n * 2.0 ** -53 * want_sal
    assert abs(bm2 - want_bm2) <= 4.0 * np.spacing(want_bm2)


def _bounds(gp, y, T_d, m, kind, box, mask_d, rows):
    """One coarse bound pass over T_d[:m] through apgp_prune_bounds (rows None) or apgp_prune_bounds_rows; int64 bits."""
    torch, _lib, lib = _rt()
    from approxposterior_amd import gp as agp
    lo, hi = agp._box(box, gp.kernel.ndim)
    ks = gp._kernel_struct()
    bmin = torch.full(((m + 63) // 64,), np.nan, dtype=torch.float64, device="cuda")
    head = (T_d.data_ptr(), m, gp._xs.data_ptr(), len(gp._x), ctypes.byref(ks), float(gp.mean.value),
            agp.UTILITY_KINDS[kind], lo, hi, None if mask_d is None else mask_d.data_ptr(), 0.01, float(np.max(y)), 1,
            bmin.data_ptr())
    if rows is None:
        _lib.check(lib.apgp_prune_bounds(*head, None), "apgp_prune_bounds")
    else:
        _lib.check(lib.apgp_prune_bounds_rows(*head, rows.data_ptr(), None), "apgp_prune_bounds_rows")
    torch.cuda.synchronize()
    return bmin.cpu().numpy().view(np.int64)


def _routes_agree(tag, gp, y, T, box, mask, ms):
    torch, _, _ = _rt()
    gp._ensure_xs(y)
    assert gp._prune_rows is not None
    T_d = torch.from_numpy(np.ascontiguousarray(T)).cuda()
    mask_d = torch.from_numpy(mask).cuda()
    finite = 0
    for m in ms:
        for kind in KINDS:
            a = _bounds(gp, y, T_d, m, kind, box, mask_d, None)
            b = _bounds(gp, y, T_d, m, kind, box, mask_d, gp._prune_rows)
            assert np.array_equal(a, b), (tag, m, kind, np.argwhere(a != b)[:4])
            finite += int(np.isfinite(a.view(np.float64)).sum())
    assert finite > 0, tag
    return finite


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_both_routes_give_the_same_bits(D, n):
    # base._case: a box with rows outside it, a mask, NaN candidates, a candidate on a training point
    gp, y, T, box, mask, _, _ = base._case(n, D, max(MS), "inverse")
    _routes_agree("n=%d D=%d" % (n, D), gp, y, T, box, mask, MS)


def test_both_routes_give_the_same_bits_when_the_gate_fails():
    n, D, m = 129, 2, 1025
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse", metric0=1e-3)
    # the gate: eta > 2^-8 for every candidate, from B alone (test_gpu_prune_mmbf16's gate case)
    gp._ensure_xs(y)
    xs = gp._xs.cpu().numpy().reshape(-1, bf.dpad_of(D) + 2)[:n, :D]
    B = np.sqrt(((xs - xs[0]) ** 2).sum(axis=1).max())
    assert bf.eta_of(0.0, B, 0.0, bf.dpad_of(D))[1] > 2.0 ** -8
    _routes_agree("gate", gp, y, T, box, mask, [m])


def _acquire(gp, y, T_d, kind, box, mask_d, rows, switch):
    """apgp_acquire (rows None) or apgp_acquire_rows for the winner alone: (best record as int64[2], the four counts)."""
    torch, _lib, lib = _rt()
    from approxposterior_amd import gp as agp
    lo, hi = agp._box(box, gp.kernel.ndim)
    ks = gp._kernel_struct()
    n, m = len(gp._x), T_d.shape[0]
    gp._ensure_linv()
    gp._ensure_xs(y)
    part = torch.zeros(int(lib.apgp_acquire_work_len(m, n)), dtype=torch.float64, device="cuda")
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    head = (T_d.data_ptr(), m, 0, gp._packed.data_ptr(), gp._xs.data_ptr(), n, ctypes.byref(ks), float(gp.mean.value),
            agp.UTILITY_KINDS[kind], lo, hi, mask_d.data_ptr(), 0.01, float(np.max(y)), None, None, None, part.data_ptr(),
            best.data_ptr())
    was = lib.apgp_set_sweep_prune(switch)
    try:
        if rows is None:
            _lib.check(lib.apgp_acquire(*head, None), "apgp_acquire")
        else:
            _lib.check(lib.apgp_acquire_rows(*head, rows.data_ptr(), None), "apgp_acquire_rows")
    finally:
        lib.apgp_set_sweep_prune(was)
    torch.cuda.synchronize()
    off = int(lib.apgp_sweep_prune_counts_offset(m, n))
    return best.cpu().numpy().view(np.int64), part[off:off + 4].cpu().numpy().view(np.int64)


@pytest.mark.parametrize("n", [33, 513])
def test_pruned_acquire_rows_is_apgp_acquire(n):
    torch, _, _ = _rt()
    D, m = 8, 1025
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")
    T_d = torch.from_numpy(T).cuda()
    mask_d = torch.from_numpy(mask).cuda()
    for kind in KINDS:
        gp._ensure_xs(y)
        old_best, old_counts = _acquire(gp, y, T_d, kind, box, mask_d, None, 2)
        new_best, new_counts = _acquire(gp, y, T_d, kind, box, mask_d, gp._prune_rows, 2)
        full_best, _ = _acquire(gp, y, T_d, kind, box, mask_d, gp._prune_rows, 0)
        assert np.array_equal(old_best, new_best) and np.array_equal(old_counts, new_counts), (kind, old_counts, new_counts)
        assert old_counts[0] >= 1                        # the pruned route ran: it left its seed count
        assert np.array_equal(new_best, full_best), (kind, new_best, full_best)


def test_a_refit_rebuilds_the_stream():
    torch, _lib, lib = _rt()
    n, D, m = 257, 3, 1025
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")
    X = np.array(gp._x, copy=True)

    def check(tag, y):
        out = {}
        for sw in (0, 2):
            gp.sweep_prune = sw
            try:
                out[sw] = gp.acquire(y, T, "agp", bounds=box, mask=mask)
            finally:
                gp.sweep_prune = None
        assert out[0][0] == out[2][0] and sp._bits(out[0][1]) == sp._bits(out[2][1]), (tag, out)
        # the stream the GP holds belongs to the rows it holds now
        fresh = _pack(torch, _lib, lib, gp._xs, n, gp._kernel_struct())
        assert torch.equal(fresh.view(torch.int64), gp._prune_rows.view(torch.int64)), tag
        return gp._prune_rows.clone()

    s0 = check("first", y)
    s1 = check("new y", np.cos(3.0 * y) + 0.1 * y)
    assert not torch.equal(s0.view(torch.int64), s1.view(torch.int64))   # alpha changed: other alphas in the stream
    gp.set_parameter_vector(gp.get_parameter_vector() + 0.3)
    gp.compute(X)
    s2 = check("new kernel vector", y)
    assert not torch.equal(s0.view(torch.int64), s2.view(torch.int64))
