# -*- coding: utf-8 -*-
"""NumPy restatement of the coarse bound's training rows sorted by alpha's sign (apgp_pack_prune_srows; csrc/prune_mm32.h,
pmm_pack_srows_kernel) and of the bound kernel's one-chain route over them.

The stream: a 32-byte header -- bm2, sal (fp64), nrt (int64), 0 -- then tiles of prune_rows_ref's image and alphas.
Class P: the rows < n whose alpha is not below 0, in their order; class N: those with alpha < 0, in theirs.
gP = ceil(|P| / 16) groups of P, then gN = ceil(|N| / 16) of N; group q is half q & 1 of 32-row matrix tile q >> 1, its
slot s the tile's row (s & 3) + 8 (s >> 2) + 4 (q & 1); nrt = ceil((gP + gN) / 2).  A slot without a row is a padding row
of the pre-split stream.  The stream has room for stiles(n) 128-row tiles, whatever the split into classes.

Built on prune_rows_ref (the image of a row) and prune_mmbf16_ref (the exponents, the error terms) by import."""
import numpy as np

import prune_mm32_ref as mm
import prune_mmbf16_ref as bf
import prune_rows_ref as rr

F = np.float32
ROWS = rr.ROWS
HDR = 4                                                # doubles in the header


def stiles(n):
    """128-row tiles of the stream: ceil(n / 16) + 1 groups at most, two per matrix tile, four matrix tiles per tile."""
    nrt_max = ((n + 15) // 16 + 2) // 2
    return (nrt_max + 3) // 4


def length(n, dpad):
    """apgp_prune_srows_len in doubles."""
    if dpad > 8:
        return 0
    _, _, xp, ap = rr.shape(dpad)
    return HDR + stiles(n) * 2 * (xp + ap)


def slot_row(q, s):
    """Row of the stream at which slot s of group q stands."""
    return 32 * (q >> 1) + (s & 3) + 8 * (s >> 2) + 4 * (q & 1)


def groups(alpha, n):
    """(rows of class P, rows of class N, gP, gN, nrt)."""
    a = np.asarray(alpha, dtype=np.float64)[:n]
    neg = a < 0.0
    P, N = np.flatnonzero(~neg), np.flatnonzero(neg)
    gP, gN = (len(P) + 15) // 16, (len(N) + 15) // 16
    return P, N, gP, gN, (gP + gN + 1) // 2


def perm(alpha, n):
    """src (stiles(n) * 128,): the original row that stands at each row of the stream, -1 for a slot without a row."""
    P, N, gP, gN, _ = groups(alpha, n)
    src = np.full(stiles(n) * ROWS, -1, dtype=np.int64)
    for rows, g0 in ((P, 0), (N, gP)):
        for k, i in enumerate(rows):
            src[slot_row(g0 + k // 16, k % 16)] = i
    return src


def layout(xs, n, dpad):
    """The stream without its header, in prune_rows_ref.layout's shapes: (image, alphas, checked)."""
    image, al, checked = rr.layout(xs, n, dpad)
    pitch = image.shape[2]
    image, al = image.reshape(-1, pitch), al.reshape(-1)
    pad_image = rr.layout(np.zeros((ROWS, dpad + 2)), 1, dpad)[0][0, 1]          # a row past n of the pre-split stream
    src = perm(np.asarray(xs, dtype=np.float64)[:, dpad], n)
    out = np.where((src >= 0)[:, None], image[np.maximum(src, 0)], pad_image[None, :])
    oal = np.where(src >= 0, al[np.maximum(src, 0)], F(0.0)).astype(F)
    return out.reshape(-1, ROWS, pitch), oal.reshape(-1, ROWS), checked


def parse(stream, n, dpad):
    """A device stream (float64 array of length(n, dpad)) -> (bm2, sal, nrt, zero word, image, alphas)."""
    _, pitch, xp, ap = rr.shape(dpad)
    nt = stiles(n)
    s = np.ascontiguousarray(stream, dtype=np.float64)
    assert len(s) == length(n, dpad)
    raw = s[HDR:].view(np.uint8).reshape(nt, 16 * (xp + ap))
    image = np.ascontiguousarray(raw[:, :16 * xp]).view(np.uint16).reshape(nt, ROWS, pitch)
    alphas = np.ascontiguousarray(raw[:, 16 * xp:]).view(F).reshape(nt, ROWS)
    words = s[2:4].view(np.int64)
    return float(s[0]), float(s[1]), int(words[0]), int(words[1]), image, alphas


def chain(k, al, absolute=False):
    """One fp32 partial sum: ps = fma(k_r, al_r, ps) over the slots r in order, from 0.  k (m, slots), al (slots,)."""
    ps = np.zeros(k.shape[0], dtype=F)
    for r in range(k.shape[1]):
        a = np.abs(al[r]) if absolute else al[r]
        ps = mm._fma32(k[:, r], np.broadcast_to(F(a), ps.shape), ps)
    return ps


def kernel_values(X, T, sc, xs=None):
    """The fp32 kernel values k^ (m, n) as prune_mmbf16_ref.replay forms them (its statements; the centre is row 0)."""
    X = np.asarray(X, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    n, d = X.shape
    dpad = bf.dpad_of(d)
    xs = X * sc if xs is None else np.asarray(xs, dtype=np.float64)
    c = xs[0].copy()
    ca, cb = T * sc - c, xs - c
    af, na = mm.operands(ca, dpad, use=(ca * ca).sum(axis=1) <= 2.0 ** 100)
    bfl, nb = mm.operands(cb, dpad)
    P = np.concatenate([-nb[:, None], np.ones((n, 1), dtype=F), F(2.0) * bfl], axis=1)
    Q = np.concatenate([np.ones((len(T), 1), dtype=F), -na[:, None], af], axis=1)
    e = bf.exponents(bf.parts_of(P), bf.parts_of(Q), dpad)
    with np.errstate(under="ignore"):
        k = np.exp2(e.astype(np.float64)).astype(F)
    k[np.abs(k) < 2.0 ** -126] = 0.0
    return k


def replay(X, alpha, T, sc, amp=1.0, xs=None, src=None):
    """prune_mmbf16_ref.replay with the partial sums taken over the rows in the stream's order (src: perm's, or a
    planted one) and S32 as the one-chain route forms it, the sum of |ps| over the groups.  Everything that does not
    depend on the order (the exact values, eta, the gate, sum |alpha|) is the existing replay's.  Adds "S32_two": what
    the two-chain route gives on the same order, and "S_hat": sum |fl32(alpha)| k^ in long double."""
    r = bf.replay(X, alpha, T, sc, amp=amp, xs=xs)
    n = len(alpha)
    k = kernel_values(X, T, sc, xs=xs)
    al32 = np.asarray(alpha, dtype=np.float64).astype(F)
    src = perm(alpha, n) if src is None else src
    m = len(T)
    acc_m, acc_s, acc_two = np.zeros(m), np.zeros(m), np.zeros(m)
    for g0 in range(0, len(src), 32):
        for h in (0, 1):
            rows = src[[g0 + (s & 3) + 8 * (s >> 2) + 4 * h for s in range(16)]]
            rows = rows[rows >= 0]                       # a slot without a row adds k * 0: exactly nothing
            if len(rows) == 0:
                continue
            ps = chain(k[:, rows], al32[rows])
            acc_m += ps.astype(np.float64)
            acc_s += np.abs(ps).astype(np.float64)
            acc_two += chain(k[:, rows], al32[rows], absolute=True).astype(np.float64)
    r = dict(r)
    r["mu32"] = amp * acc_m
    r["S32"] = acc_s * (1.0 + 2.0 ** -16)
    r["S32_two"] = acc_two * (1.0 + 2.0 ** -16)
    r["S_hat"] = (k.astype(np.longdouble) * np.abs(al32).astype(np.longdouble)[None, :]).sum(axis=1).astype(np.float64)
    r["e32"] = np.where(r["gate"], amp * (np.expm1(r["eta"]) * (1.0 + 2.0 ** -20) * r["S32"]
                                          + 2.0 ** -120 * (r["sa"] + n)), np.inf)
    return r


# ---- inputs that tests/test_prune_srows_ref.py and tests/test_gpu_prune_srows.py share ----
NS = [1, 15, 16, 17, 31, 32, 33, 130, 513]
PATTERNS = ["nonneg", "neg", "alternating", "16k", "one_negative", "zeros"]


def alphas(pattern, n, seed=0):
    """alpha (n,) of a sign pattern: all >= 0; all < 0; alternating signs; exactly 16 k positives (k = n // 32, the
    rest negative; scattered); a single negative; +0 and -0 among ordinary values of both signs."""
    rs = np.random.RandomState(1000 * seed + n)
    mag = np.abs(rs.standard_normal(n)) * 10.0 ** rs.uniform(-2, 3, size=n) + 1e-3
    if pattern == "nonneg":
        return mag
    if pattern == "neg":
        return -mag
    if pattern == "alternating":
        return mag * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    if pattern == "16k":
        sign = -np.ones(n)
        sign[rs.permutation(n)[:16 * (n // 32)]] = 1.0
        return mag * sign
    if pattern == "one_negative":
        a = mag.copy()
        a[n // 2] = -a[n // 2]
        return a
    if pattern == "zeros":
        a = mag * np.where(rs.uniform(size=n) < 0.5, 1.0, -1.0)
        a[::3] = 0.0
        a[1::6] = -0.0
        return a
    raise ValueError(pattern)
