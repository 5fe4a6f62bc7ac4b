# -*- coding: utf-8 -*-
"""NumPy restatement of the pre-split training rows of the coarse prune bound (apgp_pack_prune_rows; csrc/prune_mm32.h,
pmm_pack_rows_kernel): per 128-row tile the LDS image of prune_bound_mm32_kernel -- 128 rows of
PITCH bf16 values, of which the first 16 NI are the k slots of prune_mmbf16_ref.slots in order and the last 8 a pad --
then the tile's 128 fp32 alphas; in front a 16-byte header: max |x - c|^2 over the rows < n and sum |alpha|, both fp64.

Built from prune_mmbf16_ref.split / slots, so that the slot order is stated once."""
import math

import numpy as np

import prune_mmbf16_ref as bf

F = np.float32
ROWS = 128                                             # PMM_ROWS


def shape(dpad):
    """(instructions NI, row pitch in bf16 values, 16-byte pieces per tile: rows, alphas)."""
    ni = bf.counts(dpad)[1]
    pitch = 16 * ni + 8
    return ni, pitch, ROWS * pitch // 8, ROWS // 4


def length(n, dpad):
    """apgp_prune_rows_len in doubles."""
    if dpad > 8:
        return 0
    _, _, xp, ap = shape(dpad)
    return 2 + (n + ROWS - 1) // ROWS * 2 * (xp + ap)


def entries(xs, n, dpad):
    """P's fp32 entries (-|b|^2, 1, 2 b_1 .. 2 b_dpad) of every row of the tiles as the staging lanes form them: the
    norm summed in fp64 from the converted coordinates in the order of the dimensions; rows >= n: coordinates and norm 0
    (the norm is -0.0: the kernel negates it).  xs: the packed stream, (npad, dpad + 2)."""
    nt = (n + ROWS - 1) // ROWS
    x = np.asarray(xs, dtype=np.float64)[:nt * ROWS]
    cb = x[:, :dpad] - x[0, :dpad]
    b = (cb * bf.KAPPA).astype(F)
    b[n:] = 0.0
    n2 = np.zeros(len(b))
    for d in range(dpad):
        n2 = n2 + b[:, d].astype(np.float64) ** 2        # the square is exact in fp64: one rounding per step, as fma
    P = np.concatenate([-(n2.astype(F))[:, None], np.ones((len(b), 1), dtype=F), F(2.0) * b], axis=1)
    return P, cb


def layout(xs, n, dpad):
    """The stream without its header: (image, alphas, checked) -- image (tiles, 128, PITCH) uint16, the bf16 bit
    patterns; alphas (tiles, 128) fp32; checked (PITCH,) bool: False on the pad columns, whose content is free."""
    ni, pitch, _, _ = shape(dpad)
    P, _ = entries(xs, n, dpad)
    parts = np.stack(bf.split(P), axis=2)                # (rows, K, 3)
    rows = np.zeros((len(P), pitch), dtype=np.uint16)
    for i, (e, pp, _) in enumerate(bf.slots(dpad)):
        if e >= 0:
            v = np.ascontiguousarray(parts[:, e, pp])
            assert np.all((v.view(np.uint32) & 0xffff) == 0)             # every part is a bf16 number
            rows[:, i] = (v.view(np.uint32) >> 16).astype(np.uint16)
    al = np.asarray(xs, dtype=np.float64)[:len(P), dpad].astype(F)
    al[n:] = 0.0
    checked = np.zeros(pitch, dtype=bool)
    checked[:16 * ni] = True
    return rows.reshape(-1, ROWS, pitch), al.reshape(-1, ROWS), checked


def header(xs, n, dpad):
    """(bm2, sal): NumPy's max |x - c|^2 over the rows < n and math.fsum of |alpha|."""
    x = np.asarray(xs, dtype=np.float64)
    cb = x[:n, :dpad] - x[0, :dpad]
    return float((cb * cb).sum(axis=1).max()), math.fsum(np.abs(x[:n, dpad]).tolist())


def parse(stream, n, dpad):
    """A device stream (float64 array of length(n, dpad)) -> (bm2, sal, image, alphas) in layout's shapes."""
    _, pitch, xp, ap = shape(dpad)
    nt = (n + ROWS - 1) // ROWS
    s = np.ascontiguousarray(stream, dtype=np.float64)
    assert len(s) == length(n, dpad)
    raw = s[2:].view(np.uint8).reshape(nt, 16 * (xp + ap))
    image = np.ascontiguousarray(raw[:, :16 * xp]).view(np.uint16).reshape(nt, ROWS, pitch)
    alphas = np.ascontiguousarray(raw[:, 16 * xp:]).view(F).reshape(nt, ROWS)
    return float(s[0]), float(s[1]), image, alphas
