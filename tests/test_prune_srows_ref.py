# -*- coding: utf-8 -*-
"""CPU: the NumPy restatement of the coarse bound's sign-sorted rows (tests/prune_srows_ref.py): every row once, one
sign per (matrix tile, half) group, the classes' order kept, nrt and the stream's length; the property the one-chain
route rests on -- an fp32 fma chain over terms of one sign is the mirror image of the chain over their absolute values,
and a planted group of mixed signs breaks it --; and the refusals of the entry points that take the stream (argument
checks run before any HIP call)."""
import ctypes

import numpy as np
import pytest

import prune_mmbf16_ref as bf
import prune_rows_ref as rr
import prune_srows_ref as sr
from approxposterior_amd import _lib

F = np.float32


def _xs(n, D, pattern, seed=0):
    """A packed stream as apgp_pack_train leaves it: (npad, dpad + 2), scaled rows | alpha | 0, zero past n."""
    rs = np.random.RandomState(seed + 7 * n)
    dpad = bf.dpad_of(D)
    npad = (n + 511) // 512 * 512
    xs = np.zeros((npad, dpad + 2))
    xs[:n, :D] = rs.uniform(-5.0, 5.0, size=(n, D)) * np.sqrt(0.5 / 8.0)
    xs[:n, dpad] = sr.alphas(pattern, n)
    return xs, dpad


@pytest.mark.parametrize("pattern", sr.PATTERNS)
@pytest.mark.parametrize("n", sr.NS)
def test_every_row_once_and_one_sign_per_group(n, pattern):
    alpha = sr.alphas(pattern, n)
    P, N, gP, gN, nrt = sr.groups(alpha, n)
    src = sr.perm(alpha, n)
    assert len(src) == sr.stiles(n) * 128 and len(src) >= 32 * nrt
    assert sorted(src[src >= 0].tolist()) == list(range(n))              # every row < n exactly once
    assert np.all(src[32 * nrt:] == -1)                                  # nothing past the matrix tiles that count
    assert nrt == (gP + gN + 1) // 2 and gP == -(-len(P) // 16) and gN == -(-len(N) // 16)
    assert np.all(src[32 * (nrt - 1):32 * nrt] >= -1) and np.any(src[32 * (nrt - 1):32 * nrt] >= 0)    # nrt is tight
    seq = {0: [], 1: []}
    for q in range(2 * nrt):
        rows = src[[sr.slot_row(q, s) for s in range(16)]]
        live = rows[rows >= 0]
        assert np.all(rows[:len(live)] >= 0) and np.all(rows[len(live):] == -1)      # a group fills from slot 0
        neg = alpha[live] < 0.0
        assert np.all(neg) or not np.any(neg), (q, alpha[live])                      # one sign per group
        assert np.all(neg) == (q >= gP) or len(live) == 0
        seq[int(q >= gP)] += live.tolist()
    assert seq[0] == P.tolist() and seq[1] == N.tolist()                 # the order within a class is the rows' own
    if pattern == "16k":
        assert len(P) == 16 * (n // 32)
    if pattern == "one_negative":
        assert len(N) == 1
    if pattern == "zeros":
        assert np.all(alpha[N] != 0.0) and np.any(np.signbit(alpha[P])) == (n > 1)   # -0 stands with the rows >= 0


@pytest.mark.parametrize("n,D,pattern", [(1, 1, "neg"), (17, 2, "alternating"), (33, 3, "16k"), (130, 8, "zeros"),
                                         (513, 8, "one_negative")])
def test_layout_is_the_presplit_rows_in_another_order(n, D, pattern):
    xs, dpad = _xs(n, D, pattern)
    image, alphas, checked = sr.layout(xs, n, dpad)
    old_image, old_alphas, _ = rr.layout(xs, n, dpad)
    pitch = image.shape[2]
    assert image.shape == (sr.stiles(n), 128, pitch) and alphas.shape == (sr.stiles(n), 128)
    src = sr.perm(xs[:, dpad], n)
    flat, oflat = image.reshape(-1, pitch), old_image.reshape(-1, pitch)
    live = src >= 0
    assert np.array_equal(flat[live], oflat[src[live]])
    assert np.array_equal(alphas.reshape(-1)[live].view(np.uint32), old_alphas.reshape(-1)[src[live]].view(np.uint32))
    # a slot without a row: coordinates and norm 0 in all three parts (the h part of the norm is -0), the entry "1"
    # one, alpha +0
    sl = bf.slots(dpad)
    for i, (e, pp, _) in enumerate(sl):
        got = (flat[~live][:, i].astype(np.uint32) << 16).view(F)
        assert np.all(got == (1.0 if (e, pp) == (1, 0) else 0.0)), (i, e, pp)
    assert np.all(alphas.reshape(-1)[~live].view(np.uint32) == 0)


def test_stream_length():
    lib = _lib.load()
    # n = 4096: 256 groups if the classes end on group borders, 257 if not: 129 matrix tiles, 33 staged tiles
    assert sr.stiles(4096) == 33 and sr.stiles(1) == 1 and sr.stiles(112) == 1 and sr.stiles(113) == 2
    assert lib.apgp_prune_srows_len(4096, 8) == 4 + 33 * 18944 // 8 == sr.length(4096, 8)
    for n in sr.NS:
        for D in (1, 3, 8):
            assert lib.apgp_prune_srows_len(n, D) == sr.length(n, bf.dpad_of(D)), (n, D)
        for pattern in sr.PATTERNS:                                      # room for every split
            assert sr.groups(sr.alphas(pattern, n), n)[4] <= 4 * sr.stiles(n)
    assert lib.apgp_prune_srows_len(4096, 9) == 0 == sr.length(100, 16)
    assert lib.apgp_prune_srows_len(100, 0) == -1 and lib.apgp_prune_srows_len(100, _lib.MAX_DIM + 1) == -1


def test_a_chain_over_one_sign_is_the_mirror_of_the_chain_over_absolute_values():
    rs = np.random.RandomState(3)
    m = 4096
    for trial in range(8):
        # kernel values in (0, 1], some tiny, some zero (a flushed value), some equal to one
        k = np.exp2(-rs.uniform(0.0, 40.0, size=(m, 16)) * rs.randint(0, 2, size=(m, 16))).astype(F)
        k[rs.uniform(size=k.shape) < 0.05] = 0.0
        mag = (np.abs(rs.standard_normal(16)) * 10.0 ** rs.uniform(-6, 6, size=16)).astype(F)
        mag[rs.randint(16)] = 0.0
        for sign in (1.0, -1.0):
            al = (sign * mag).astype(F)
            if trial % 2:
                al[al == 0] = -0.0 * sign                # a zero of either sign among them
            ps, pS = sr.chain(k, al), sr.chain(k, al, absolute=True)
            assert np.array_equal(np.abs(ps).view(np.uint32), pS.view(np.uint32)), (trial, sign)
        # a planted mixed group: one alpha of the other sign, and |ps| falls below pS where that term counts
        al = mag.copy()
        j = int(np.argmax(mag))
        al[j] = -al[j]
        ps, pS = sr.chain(k, al), sr.chain(k, al, absolute=True)
        assert np.all(np.abs(ps) <= pS)
        others = (np.delete(k, j, axis=1) * np.delete(mag, j)[None, :]).max(axis=1)
        counts = (others > 0) & (k[:, j] * mag[j] >= 2.0 ** -10 * others) & (others >= 2.0 ** -10 * k[:, j] * mag[j])
        assert counts.sum() > m // 16 and np.all(np.abs(ps)[counts] < pS[counts]), trial


@pytest.mark.parametrize("n,pattern", [(33, "alternating"), (130, "16k"), (130, "zeros")])
def test_replay_one_chain_equals_two_chains_on_the_sorted_rows_only(n, pattern):
    rs = np.random.RandomState(n)
    D = 3
    X = rs.uniform(-5.0, 5.0, size=(n, D))
    T = rs.uniform(-5.0, 5.0, size=(40, D))
    alpha = sr.alphas(pattern, n)
    sc = np.sqrt(0.5 / np.full(D, 8.0))
    r = sr.replay(X, alpha, T, sc)
    assert np.array_equal(r["S32"].view(np.int64), r["S32_two"].view(np.int64))
    u = 2.0 ** -24
    assert np.all(r["S32"] >= (1.0 - 17.0 * u) * r["S_hat"]) and np.all(r["S32"] <= (1.0 + 2.0 ** -15) * r["S_hat"])
    # the rows in their own order, 16 to a group (the pre-split stream's order), taken as if they were sorted: mixed
    # groups, and the one-chain sum falls below (1 - 17 u) of sum |alpha| k^
    own = np.full(sr.stiles(n) * 128, -1, dtype=np.int64)
    for i in range(n):
        own[sr.slot_row(i // 16, i % 16)] = i
    bad = sr.replay(X, alpha, T, sc, src=own)
    assert np.any(bad["S32"] < (1.0 - 17.0 * u) * bad["S_hat"])
    assert np.all(bad["S32_two"] >= (1.0 - 17.0 * u) * bad["S_hat"])


def test_bad_arguments_are_refused_without_a_gpu():
    lib = _lib.load()
    ks = _lib.KernelStruct()
    ks.ndim = 2
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 0.125
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    for args in ((None, 4, ctypes.byref(ks), p, None), (p, 4, None, p, None), (p, 4, ctypes.byref(ks), None, None)):
        assert lib.apgp_pack_prune_srows(*args) == -1
        assert b"apgp_pack_prune_srows" in lib.apgp_last_error() and b"null pointer" in lib.apgp_last_error()
    assert lib.apgp_pack_prune_srows(p, 0, ctypes.byref(ks), p, None) == -1
    ks.ndim = 9
    assert lib.apgp_pack_prune_srows(p, 4, ctypes.byref(ks), p, None) == -1      # no stream beyond Dpad 8
    ks.ndim = 2
    for kind, rows in ((_lib.PRUNE_ROWS_SIGNED, None), (2, p), (-1, p)):         # SIGNED needs its stream; unknown kinds
        assert lib.apgp_acquire_rows2(p, 1, 0, p, p, 4, ctypes.byref(ks), 0.0, 0, None, None, None,
                                      0.01, 0.0, None, None, None, None, p, rows, kind, None) == -1
        assert b"rows_kind" in lib.apgp_last_error()
        assert lib.apgp_acquire_solve_rows2(p, 1, 0, p, p, 4, ctypes.byref(ks), 0.0, 0, None, None, None,
                                            0.01, 0.0, None, None, None, None, p, rows, kind, None) == -1
        assert b"rows_kind" in lib.apgp_last_error()
        assert lib.apgp_prune_bounds_rows2(p, 1, p, 4, ctypes.byref(ks), 0.0, 0, None, None, None, 0.0, 0.0, 1, p,
                                           rows, kind, None, None) == -1
        assert b"apgp_prune_bounds_rows2" in lib.apgp_last_error() and b"rows_kind" in lib.apgp_last_error()
    assert lib.apgp_prune_bounds_rows2(None, 1, None, 4, ctypes.byref(ks), 0.0, 0, None, None, None, 0.0, 0.0, 1, None,
                                       None, 0, None, None) == -1
    assert b"null pointer" in lib.apgp_last_error()
