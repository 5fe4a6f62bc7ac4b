# -*- coding: utf-8 -*-
"""CPU: the NumPy restatement of the coarse bound's pre-split rows (tests/prune_rows_ref.py) against the operands
tests/prune_mmbf16_ref.replay forms -- the same parts in the same k slots --, the stream's length, and the refusals of
the entry points that take the stream (argument checks run before any HIP call)."""
import ctypes

import numpy as np
import pytest

import prune_mm32_ref as mm
import prune_mmbf16_ref as bf
import prune_rows_ref as rr
from approxposterior_amd import _lib

F = np.float32


def _xs(n, D, seed=0):
    """A packed stream as apgp_pack_train leaves it: (npad, dpad + 2), scaled rows | alpha | 0, zero past n."""
    rs = np.random.RandomState(seed)
    dpad = bf.dpad_of(D)
    npad = (n + 511) // 512 * 512
    xs = np.zeros((npad, dpad + 2))
    xs[:n, :D] = rs.uniform(-5.0, 5.0, size=(n, D)) * np.sqrt(0.5 / 8.0)
    xs[:n, dpad] = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 6, size=n)
    return xs, dpad


@pytest.mark.parametrize("n,D", [(1, 1), (31, 2), (129, 3), (200, 4), (513, 8)])
def test_layout_holds_the_replays_operands(n, D):
    xs, dpad = _xs(n, D)
    ni, pitch, xp, ap = rr.shape(dpad)
    assert pitch % 8 == 0 and (pitch // 8) % 2 == 1 and xp * 8 == 128 * pitch      # an odd number of 16-byte units
    image, alphas, checked = rr.layout(xs, n, dpad)
    nt = (n + 127) // 128
    assert image.shape == (nt, 128, pitch) and alphas.shape == (nt, 128) and checked.sum() == 16 * ni
    # P as prune_mmbf16_ref.replay forms it, its parts, and the part each k slot takes on the training rows' side
    cb = xs[:n, :D] - xs[0, :D]
    bfl, nb = mm.operands(cb, dpad)
    P = np.concatenate([-nb[:, None], np.ones((n, 1), dtype=F), F(2.0) * bfl], axis=1)
    parts = bf.parts_of(P)
    flat = image.reshape(-1, pitch)
    sl = bf.slots(dpad)
    assert len(sl) == 16 * ni
    for i, (e, pp, _) in enumerate(sl):
        got = (flat[:, i].astype(np.uint32) << 16).view(F)
        want = parts[:, e, pp] if e >= 0 else np.zeros(n, dtype=F)
        assert np.array_equal(got[:n].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (i, e, pp)
        # the padding: coordinates and norm 0 in all three parts, the entry "1" one
        assert np.all(got[n:] == (1.0 if (e, pp) == (1, 0) else 0.0)), (i, e, pp)
    assert np.array_equal(alphas.reshape(-1)[:n], xs[:n, dpad].astype(F)) and np.all(alphas.reshape(-1)[n:] == 0.0)
    # the three parts of every entry add up to the entry
    P2, _ = rr.entries(xs, n, dpad)
    h, m, l = bf.split(P2)
    assert np.array_equal((h.astype(np.float64) + m + l), P2.astype(np.float64))


def test_stream_length():
    lib = _lib.load()
    # Dpad 8: four instructions, pitch 72: 128 * 72 * 2 + 128 * 4 = 18,944 bytes per tile, 32 tiles, a 16-byte header
    assert lib.apgp_prune_rows_len(4096, 8) == 2 + 32 * 18944 // 8 == rr.length(4096, 8)
    # Dpad 4: three instructions, pitch 56, one tile
    assert lib.apgp_prune_rows_len(100, 3) == 2 + (128 * 56 * 2 + 512) // 8 == rr.length(100, 4)
    assert lib.apgp_prune_rows_len(129, 2) == rr.length(129, 2) == 2 + 2 * (128 * 40 * 2 + 512) // 8
    # Dpad 16 and 32: the coarse bound keeps the vector-ALU kernel, no stream
    assert lib.apgp_prune_rows_len(4096, 9) == 0 and lib.apgp_prune_rows_len(100, 32) == 0 == rr.length(100, 16)
    assert lib.apgp_prune_rows_len(100, 0) == -1 and lib.apgp_prune_rows_len(100, _lib.MAX_DIM + 1) == -1


def test_null_pointers_are_refused_without_a_gpu():
    lib = _lib.load()
    ks = _lib.KernelStruct()
    ks.ndim = 2
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 0.125
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    for args in ((None, 4, ctypes.byref(ks), p, None), (p, 4, None, p, None), (p, 4, ctypes.byref(ks), None, None)):
        assert lib.apgp_pack_prune_rows(*args) == -1
        assert b"apgp_pack_prune_rows" in lib.apgp_last_error() and b"null pointer" in lib.apgp_last_error()
    assert lib.apgp_pack_prune_rows(p, 0, ctypes.byref(ks), p, None) == -1
    ks.ndim = 9
    assert lib.apgp_pack_prune_rows(p, 4, ctypes.byref(ks), p, None) == -1       # no stream beyond Dpad 8
    ks.ndim = 2
    assert lib.apgp_acquire_rows(None, 1, 0, None, None, 4, ctypes.byref(ks), 0.0, 0, None, None, None,
                                 0.01, 0.0, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in lib.apgp_last_error()
    assert lib.apgp_acquire_solve_rows(None, 1, 0, None, None, 4, ctypes.byref(ks), 0.0, 0, None, None, None,
                                       0.01, 0.0, None, None, None, None, None, None, None) == -1
    assert lib.apgp_prune_bounds_rows(None, 1, None, 4, ctypes.byref(ks), 0.0, 0, None, None, None, 0.0, 0.0, 1, None,
                                      None, None) == -1
    assert b"apgp_prune_bounds_rows" in lib.apgp_last_error() and b"null pointer" in lib.apgp_last_error()
