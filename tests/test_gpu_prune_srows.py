# -*- coding: utf-8 -*-
"""MI355X: the coarse prune bound over the training rows sorted by alpha's sign (apgp_pack_prune_srows and the entry
points that take the stream's kind; csrc/prune_mm32.h; DESIGN.md sections 3 and 4).

Training sets n = 1, 15, 16, 17, 31, 32, 33, 130, 513 (below, at and past one group of 16, one 32-row matrix tile, one
128-row tile; 130 and 513 leave a ragged last staged tile, nrt not a multiple of 4) with alpha of six sign patterns
(tests/prune_srows_ref.alphas), D = 1, 3, 8 (Dpad 2, 4, 8), m = 1, 33, 64, 70, 513.

* stream image against the restatement tests/prune_srows_ref.py, every bf16 value and fp32 alpha bit for bit, the slots
  without a row included; nrt exact, the header's last word 0; sal within n 2^-53 relative of math.fsum and bm2 within
  4 ulp of NumPy's (test_gpu_prune_rows's two bounds; bm2's maximum is exact, the 4 ulp are the two ways to sum a
  row's squares, so "within 1 ulp" of the pre-split stream's header is asked for as well: the same fma chain).
* contract: every row of a block masked but one, on lanes 0, 31, 32, 63: b - 2 slack <= bmin <= b, b from the exact mu,
  the slack from the replay with the rows in the stream's order (prune_srows_ref.replay).
* S32: est - bmin is the kernel's slack of that row; taking prune_bound_kernel's part and e32's absolute term off and
  dividing by 2 amp expm1(eta) (1 + 2^-20) gives the kernel's S32, which must not lie below (1 - 17 u) of
  sum |fl32(alpha)| k^ (the replay's kernel values).  bmin = fl(est - slack) carries one rounding of size
  2^-53 |est|, est another: the recovered S32 is allowed 2^-51 (|est| + |bmin|) / (2 amp expm1(eta)) for them.  A group
  of mixed signs would put |ps| below the chain on |alpha| and fail here, silently everywhere else.
* the gate-failure route: the bounds are the pre-split route's, bit for bit (the vector-ALU kernel behind both).
* the pruned GP.acquire through the new stream, through the old one and the full sweep: one winner, bit for bit.
* a refit rebuilds the stream; GP.prune_signed = False selects the old route.

Tolerance: none beyond those stated."""
import ctypes
import math

import numpy as np
import pytest

import prune_mmbf16_ref as bf
import prune_ref as pr
import prune_rows_ref as rr
import prune_srows_ref as sr
import test_gpu_prune_mm32 as base
import test_gpu_sweep_prune as sp
import util_ref

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
DS = [1, 3, 8]
MS = [1, 33, 64, 70, 513]
LANES = [0, 31, 32, 63]
MEAN, ZETA, YBEST = 0.3, 0.01, 1.5
U = 2.0 ** -24


def _rt():
    import torch
    from approxposterior_amd import _lib
    return torch, _lib, _lib.load()


def _kernel_struct(_lib, D, metric0=8.0):
    ks = _lib.KernelStruct()
    ks.ndim = D
    ks.amp = 1.0
    for d in range(D):
        ks.inv_metric[d] = 1.0 / 8.0
    ks.inv_metric[0] = 1.0 / metric0
    return ks


class _Fit:
    """A training set with a chosen alpha on the device: the packed stream and both row streams."""

    def __init__(self, n, D, pattern, metric0=8.0):
        torch, _lib, lib = _rt()
        rs = np.random.RandomState(31 * n + D)
        self.n, self.D, self.dpad = n, D, bf.dpad_of(D)
        self.X = rs.uniform(-5.0, 5.0, size=(n, D))
        self.alpha = sr.alphas(pattern, n)
        self.ks = _kernel_struct(_lib, D, metric0)
        metric = np.full(D, 8.0)
        metric[0] = metric0
        self.sc = np.sqrt(0.5 / metric)
        self.xs_d = torch.empty(int(lib.apgp_packed_train_len(n, D)), dtype=torch.float64, device="cuda")
        X_d, alpha_d = torch.from_numpy(self.X).cuda(), torch.from_numpy(self.alpha).cuda()    # (both alive in the call)
        _lib.check(lib.apgp_pack_train(X_d.data_ptr(), alpha_d.data_ptr(), n, ctypes.byref(self.ks),
                                       self.xs_d.data_ptr(), None), "apgp_pack_train")
        self.srows = torch.full((int(lib.apgp_prune_srows_len(n, D)),), np.nan, dtype=torch.float64, device="cuda")
        _lib.check(lib.apgp_pack_prune_srows(self.xs_d.data_ptr(), n, ctypes.byref(self.ks), self.srows.data_ptr(), None),
                   "apgp_pack_prune_srows")
        self.rows = torch.full((int(lib.apgp_prune_rows_len(n, D)),), np.nan, dtype=torch.float64, device="cuda")
        _lib.check(lib.apgp_pack_prune_rows(self.xs_d.data_ptr(), n, ctypes.byref(self.ks), self.rows.data_ptr(), None),
                   "apgp_pack_prune_rows")
        torch.cuda.synchronize()
        self.xs = self.xs_d.cpu().numpy().reshape(-1, self.dpad + 2)

    def bounds(self, T_d, m, kind, mask_d, signed=True, box=None):
        """(bmin, est) of one coarse pass over T_d[:m] through apgp_prune_bounds_rows2."""
        torch, _lib, lib = _rt()
        from approxposterior_amd import gp as agp
        lo, hi = agp._box(box, self.D)
        ncb = (m + 63) // 64
        out = torch.full((2, ncb), np.nan, dtype=torch.float64, device="cuda")
        stream, kind_of = (self.srows, _lib.PRUNE_ROWS_SIGNED) if signed else (self.rows, _lib.PRUNE_ROWS_SPLIT)
        _lib.check(lib.apgp_prune_bounds_rows2(T_d.data_ptr(), m, self.xs_d.data_ptr(), self.n, ctypes.byref(self.ks), MEAN,
                                               agp.UTILITY_KINDS[kind], lo, hi, mask_d.data_ptr(), ZETA, YBEST, 1,
                                               out[0].data_ptr(), stream.data_ptr(), kind_of, out[1].data_ptr(), None),
                   "apgp_prune_bounds_rows2")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        return o[0], o[1]


def _check_image(f):
    n, dpad = f.n, f.dpad
    assert len(f.srows) == sr.length(n, dpad)
    bm2, sal, nrt, zero, image, alphas = sr.parse(f.srows.cpu().numpy(), n, dpad)
    want_image, want_alphas, checked = sr.layout(f.xs, n, dpad)
    assert image.shape == want_image.shape and alphas.shape == want_alphas.shape
    bad = np.argwhere(image[:, :, checked] != want_image[:, :, checked])
    assert len(bad) == 0, ("first differing (tile, row, slot)", bad[:4], n, f.D)
    assert np.array_equal(alphas.view(np.uint32), want_alphas.view(np.uint32))
    assert nrt == sr.groups(f.alpha, n)[4] and zero == 0
    want_bm2, want_sal = rr.header(f.xs, n, dpad)
    assert abs(sal - want_sal) <= n * 2.0 ** -53 * want_sal
    assert abs(bm2 - want_bm2) <= 4.0 * np.spacing(want_bm2)
    old_bm2 = float(f.rows[:1].cpu().numpy()[0])                        # the pre-split stream's: the same chain per row
    assert abs(bm2 - old_bm2) <= np.spacing(old_bm2)
    return sal


@pytest.mark.parametrize("pattern", sr.PATTERNS)
@pytest.mark.parametrize("n", sr.NS)
@pytest.mark.parametrize("D", DS)
def test_image_contract_and_s32(D, n, pattern):
    torch, _, _ = _rt()
    f = _Fit(n, D, pattern)
    sal = _check_image(f)
    sa = sal * (1.0 + 2.0 ** -16)
    rs = np.random.RandomState(5 * n + D)
    mmax = max(MS)
    T = rs.uniform(-5.0, 5.0, size=(mmax, D))
    T[LANES[1]] = f.X[n // 2]                            # a candidate on a training point
    T_d = torch.from_numpy(T).cuda()
    live = np.array(sorted(b * 64 + l for b in range((mmax + 63) // 64) for l in LANES if b * 64 + l < mmax))
    r = sr.replay(f.xs[:n, :D], f.alpha, T[live], f.sc, amp=1.0, xs=f.xs[:n, :D])
    assert r["gate"].all()
    assert np.array_equal(r["S32"].view(np.int64), r["S32_two"].view(np.int64))          # the sorted order: one chain is two
    mu = r["mu"] + MEAN
    sharp = 0
    for m in MS:
        for kept in LANES:
            rows = np.arange((m + 63) // 64) * 64 + kept
            rows = rows[rows < m]
            mask = np.zeros(m, dtype=np.uint8)
            mask[rows] = 1
            mask_d = torch.from_numpy(mask).cuda()
            at = np.searchsorted(live, rows)
            sub = {"e32": r["e32"][at], "sa": r["sa"], "n": n, "dpad": f.dpad}
            for kind in KINDS:
                tag = "n=%d D=%d %s m=%d lane %d %s" % (n, D, pattern, m, kept, kind)
                bmin, est = f.bounds(T_d, m, kind, mask_d)
                dead = np.ones(len(bmin), dtype=bool)
                dead[rows // 64] = False
                assert np.all(bmin[dead] == np.inf) and np.all(est[dead] == np.inf), tag
                if len(rows) == 0:
                    continue
                b = pr.row_bounds(kind, mu[at], 1.0, r["S"][at], np.ones(len(rows), dtype=bool), n, f.dpad, ZETA, YBEST)
                b0 = util_ref.f64(kind, mu[at], np.ones(len(rows)), ZETA, YBEST)
                sl = bf.slack(kind, b0, mu[at], 1.0, sub, ZETA, YBEST)
                got, ge = bmin[rows // 64], est[rows // 64]
                assert np.all(got <= b) and np.all(b - 2.0 * sl <= got), (tag, got, b, sl)
                # the kernel's S32 out of its slack
                rest = pr.slack(kind, ge, mu[at], 1.0, sa, n, f.dpad, ZETA, YBEST)
                scale = 2.0 * np.expm1(r["eta"][at]) * (1.0 + 2.0 ** -20)
                s32 = ((ge - got - rest) - 2.0 * 2.0 ** -120 * (sa + n)) / scale / (1.0 + 2.0 ** -16)
                room = 2.0 ** -51 * (np.abs(ge) + np.abs(got)) / scale
                assert np.all(s32 >= (1.0 - 17.0 * U) * r["S_hat"][at] - room), (tag, s32, r["S_hat"][at], room)
                sharp += int((room < U * r["S_hat"][at]).sum())
    if pattern != "zeros" or n > 1:
        assert sharp > 0                                 # rows where the recovery resolves 17 u were among them


def test_gate_failure_takes_the_kernel_behind_both_routes():
    torch, _, _ = _rt()
    n, D, m = 130, 2, 1025
    f = _Fit(n, D, "alternating", metric0=1e-3)
    B = np.sqrt(((f.xs[:n, :D] - f.xs[0, :D]) ** 2).sum(axis=1).max())
    assert bf.eta_of(0.0, B, 0.0, f.dpad)[1] > 2.0 ** -8
    rs = np.random.RandomState(2)
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    T[3::11, D - 1] = np.nan
    mask = (rs.uniform(size=m) < 0.7).astype(np.uint8)
    T_d, mask_d = torch.from_numpy(T).cuda(), torch.from_numpy(mask).cuda()
    box = [(-4.0, 5.0)] * D
    for kind in KINDS:
        new, new_est = f.bounds(T_d, m, kind, mask_d, signed=True, box=box)
        old, old_est = f.bounds(T_d, m, kind, mask_d, signed=False, box=box)
        assert np.array_equal(new.view(np.int64), old.view(np.int64)), kind
        assert np.array_equal(new_est.view(np.int64), old_est.view(np.int64)), kind
        adm = np.all((T >= -4.0) & (T <= 5.0), axis=1) & (mask != 0)
        has = np.zeros(len(new) * 64, dtype=bool)
        has[:m] = adm
        has = has.reshape(-1, 64).any(axis=1)
        assert np.all(np.isfinite(new[has])) and np.all(new[~has] == np.inf), kind


@pytest.mark.parametrize("n", [130, 513])
def test_pruned_acquire_is_the_full_sweep_through_either_stream(n):
    D, m = 8, 1025
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")          # a box, a mask, NaN candidates
    kw = dict(bounds=box, mask=mask)
    for kind in KINDS:
        out = {}
        for name, sw, signed in (("full", 0, True), ("signed", 2, True), ("split", 2, False)):
            gp.sweep_prune, gp.prune_signed, gp.sweep_prune_stats = sw, signed, True
            gp.last_prune_counts = None
            try:
                out[name] = gp.acquire(y, T, kind, **kw)
            finally:
                gp.sweep_prune, gp.prune_signed, gp.sweep_prune_stats = None, True, False
            if sw:
                assert int(gp.last_prune_counts.cpu().numpy()[0]) >= 1   # the pruned route ran: it left its seed count
        for name in ("signed", "split"):
            assert out[name][0] == out["full"][0] and sp._bits(out[name][1]) == sp._bits(out["full"][1]), (kind, out)
        sp._against_return_all(gp, y, T, kind, **kw)


def test_a_refit_rebuilds_the_stream_and_the_switch_selects_the_old_route():
    torch, _lib, lib = _rt()
    from approxposterior_amd import gp as agp
    n, D, m = 130, 3, 513
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")

    def fresh():
        s = torch.full((int(lib.apgp_prune_srows_len(n, D)),), np.nan, dtype=torch.float64, device="cuda")
        _lib.check(lib.apgp_pack_prune_srows(gp._xs.data_ptr(), n, ctypes.byref(gp._kernel_struct()), s.data_ptr(), None),
                   "apgp_pack_prune_srows")
        torch.cuda.synchronize()
        return s

    def raw(y, kind, stream, kind_of):
        lo, hi = agp._box(box, D)
        ks = gp._kernel_struct()
        bmin = torch.full(((m + 63) // 64,), np.nan, dtype=torch.float64, device="cuda")
        T_d, mask_d = torch.from_numpy(T).cuda(), torch.from_numpy(mask).cuda()
        _lib.check(lib.apgp_prune_bounds_rows2(T_d.data_ptr(), m, gp._xs.data_ptr(), n, ctypes.byref(ks),
                                               float(gp.mean.value), agp.UTILITY_KINDS[kind], lo, hi, mask_d.data_ptr(), 0.01,
                                               float(np.max(y)), 1, bmin.data_ptr(), stream.data_ptr(), kind_of, None, None),
                   "apgp_prune_bounds_rows2")
        torch.cuda.synchronize()
        return bmin.cpu().numpy().view(np.int64)

    streams = []
    for tag, yy in (("first", y), ("new y", np.cos(3.0 * y) + 0.1 * y)):
        got = gp.prune_bounds(yy, T, "agp", bounds=box, mask=mask).view(np.int64)
        assert gp._prune_srows is not None and gp._prune_rows is not None
        assert torch.equal(fresh().view(torch.int64), gp._prune_srows.view(torch.int64)), tag
        assert np.array_equal(got, raw(yy, "agp", gp._prune_srows, _lib.PRUNE_ROWS_SIGNED)), tag
        gp.prune_signed = False
        try:
            old = gp.prune_bounds(yy, T, "agp", bounds=box, mask=mask).view(np.int64)
        finally:
            gp.prune_signed = True
        assert np.array_equal(old, raw(yy, "agp", gp._prune_rows, _lib.PRUNE_ROWS_SPLIT)), tag
        streams.append(gp._prune_srows.clone())
    assert not torch.equal(streams[0].view(torch.int64), streams[1].view(torch.int64))   # alpha changed
