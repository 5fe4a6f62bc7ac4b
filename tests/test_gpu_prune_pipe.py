# -*- coding: utf-8 -*-
"""MI355X: the pipelined row loop of the coarse prune bound over the sign-sorted rows (csrc/prune_mm32.h, PIPE;
``apgp_set_prune_pipe`` / ``GP.prune_pipe``) changes no bit.  The pipeline only reorders the issue of the same
statements, so every comparison here is between bit patterns, switch on against switch off.

Shapes, chosen for the places a carried pipeline and a prefetch can go wrong (nrt: 32-row matrix tiles that hold a row;
a staged tile holds four):

* n = 1, 16, 17, 33, 130, 513 with the six sign patterns of tests/prune_srows_ref.alphas: nrt = 1 (the prologue is the
  epilogue), nrt not a multiple of 4 (matrix tiles alone behind a barrier, taken one at a time and drained), a class
  that ends inside a group, and at 513 four full staged tiles whose last group is carried across the barrier;
  n = 128 and 256 in addition: nrt = 4 and 8, where the LAST staged tile is full and drains in the straight-line path.
* D = 1, 3, 8: 2, 3 and 4 matrix instructions per chain, so slices of 8, 5-5-6 and 4 exponentials.
* m = 1, 33, 64, 70, 513: partial groups, partial blocks, more than one workgroup.

Bound outputs: ``apgp_prune_bounds_rows2`` on every combination and three utilities: bmin and est_out; again with a
box, with a mask, with a NaN coordinate in one candidate, and on the gate-failure route.  (That entry point passes no
arg-min partials to the kernel, so the kernel's (+inf, -1) pre-fill of part_u / part_i is covered by the winner test:
the pruned arg-min reads them for every block it does not sweep.)
Winner: pruned ``GP.acquire`` at n = 130 and 513 with ``prune_pipe`` on and off against the full sweep: one winner, the
index equal and u equal as bits, ``last_prune_counts`` (seeds, survivors, tau's bits, coarse kept, second-wave seeds)
equal.  Plumbing: ``GP.prune_pipe = False`` reaches the library and is put back; a refit keeps the setting.

Tolerance: none."""
import numpy as np
import pytest

import prune_srows_ref as sr
import test_gpu_prune_mm32 as base
import test_gpu_prune_srows as ps
import test_gpu_sweep_prune as sp

pytestmark = pytest.mark.gpu

KINDS = sp.KINDS
NS = [1, 16, 17, 33, 130, 513]
NS_FULL_LAST = [128, 256]
DS = [1, 3, 8]
MS = [1, 33, 64, 70, 513]


def _on_off(f, T_d, m, kind, mask_d, box=None, signed=True):
    """((bmin, est) with the switch on, the same with it off) as int64 bit patterns."""
    _, _, lib = ps._rt()
    out = []
    for v in (1, 0):
        was = lib.apgp_set_prune_pipe(v)
        try:
            assert lib.apgp_get_prune_pipe() == v
            bmin, est = f.bounds(T_d, m, kind, mask_d, signed=signed, box=box)
        finally:
            lib.apgp_set_prune_pipe(was)
        out.append((bmin.view(np.int64), est.view(np.int64)))
    return out


def _same(f, T_d, m, kind, mask_d, tag, box=None):
    (b1, e1), (b0, e0) = _on_off(f, T_d, m, kind, mask_d, box=box)
    assert np.array_equal(b1, b0), ("bmin", tag, np.flatnonzero(b1 != b0)[:4])
    assert np.array_equal(e1, e0), ("est", tag, np.flatnonzero(e1 != e0)[:4])
    return b1.view(np.float64)


def _bounds_across_the_switch(D, n, patterns):
    torch, _, _ = ps._rt()
    mmax = max(MS)
    rs = np.random.RandomState(7 * n + D)
    T = rs.uniform(-5.0, 5.0, size=(mmax, D))
    Tn = T.copy()
    Tn[min(37, mmax - 1), D - 1] = np.nan                # a NaN coordinate in one candidate
    Tn[0, 0] = np.nan                                    # (and in the only candidate of m = 1)
    T_d, Tn_d = torch.from_numpy(T).cuda(), torch.from_numpy(Tn).cuda()
    ones_d = torch.ones(mmax, dtype=torch.uint8, device="cuda")
    mask = (rs.uniform(size=mmax) < 0.6).astype(np.uint8)
    mask_d = torch.from_numpy(mask).cuda()
    box = [(-4.0, 4.5)] * D
    for pattern in patterns:
        f = ps._Fit(n, D, pattern)
        for m in MS:
            for kind in KINDS:
                tag = "n=%d D=%d %s m=%d %s" % (n, D, pattern, m, kind)
                b = _same(f, T_d, m, kind, ones_d, tag)
                assert np.all(np.isfinite(b)), tag       # every block has an admissible row
                _same(f, T_d, m, kind, ones_d, tag + " box", box=box)
                _same(f, T_d, m, kind, mask_d, tag + " mask")
                _same(f, Tn_d, m, kind, ones_d, tag + " nan")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_bounds_across_the_switch(D, n):
    _bounds_across_the_switch(D, n, sr.PATTERNS)


@pytest.mark.parametrize("n", NS_FULL_LAST)
@pytest.mark.parametrize("D", DS)
def test_bounds_across_the_switch_last_staged_tile_full(D, n):
    for pattern in ("nonneg", "alternating"):
        assert sr.groups(sr.alphas(pattern, n), n)[4] == n // 32        # nrt: a multiple of four
    _bounds_across_the_switch(D, n, ("nonneg", "alternating"))


def test_gate_failure_route_across_the_switch():
    torch, _, _ = ps._rt()
    n, D, m = 130, 2, 1025                               # the inputs of test_gpu_prune_srows's gate-failure test
    f = ps._Fit(n, D, "alternating", metric0=1e-3)
    B = np.sqrt(((f.xs[:n, :D] - f.xs[0, :D]) ** 2).sum(axis=1).max())
    assert ps.bf.eta_of(0.0, B, 0.0, f.dpad)[1] > 2.0 ** -8
    rs = np.random.RandomState(2)
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    T[3::11, D - 1] = np.nan
    mask = (rs.uniform(size=m) < 0.7).astype(np.uint8)
    T_d, mask_d = torch.from_numpy(T).cuda(), torch.from_numpy(mask).cuda()
    for kind in KINDS:
        _same(f, T_d, m, kind, mask_d, "gate failure " + kind, box=[(-4.0, 5.0)] * D)
        (b1, e1), _ = _on_off(f, T_d, m, kind, mask_d, box=[(-4.0, 5.0)] * D)
        (bs, es), _ = _on_off(f, T_d, m, kind, mask_d, box=[(-4.0, 5.0)] * D, signed=False)
        assert np.array_equal(b1, bs) and np.array_equal(e1, es), kind   # the vector-ALU kernel behind both streams


@pytest.mark.parametrize("n", [130, 513])
def test_pruned_acquire_across_the_switch(n):
    D, m = 8, 1025
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")          # a box, a mask, NaN candidates
    assert gp.prune_pipe is None and gp.prune_signed
    kw = dict(bounds=box, mask=mask)
    for kind in KINDS:
        out = {}
        for name, sw, pipe in (("full", 0, None), ("pipe", 2, True), ("plain", 2, False)):
            gp.sweep_prune, gp.prune_pipe, gp.sweep_prune_stats = sw, pipe, True
            gp.last_prune_counts = None
            try:
                bi, bu = gp.acquire(y, T, kind, **kw)
            finally:
                gp.sweep_prune, gp.prune_pipe, gp.sweep_prune_stats = None, None, False
            counts = None
            if sw:
                counts = tuple(int(c) for c in gp.last_prune_counts.cpu().numpy())
                assert len(counts) == 5 and counts[0] >= 1           # the pruned route ran: it left its seed count
            out[name] = (bi, int(sp._bits(bu)), counts)
        assert out["pipe"] == out["plain"], (kind, out)
        assert out["pipe"][:2] == out["full"][:2], (kind, out)
        sp._against_return_all(gp, y, T, kind, **kw)


def test_the_switch_reaches_the_library_and_a_refit_keeps_it(monkeypatch):
    _, _, lib = ps._rt()
    n, D, m = 130, 3, 513
    gp, y, T, box, mask, _, _ = base._case(n, D, m, "inverse")
    assert lib.apgp_get_prune_pipe() == 1                # the library's default: on
    real, seen = lib.apgp_set_prune_pipe, []

    def spy(v):
        was = real(v)
        seen.append((int(v), int(was)))
        return was

    monkeypatch.setattr(lib, "apgp_set_prune_pipe", spy)
    gp.sweep_prune = 2
    try:
        want = gp.acquire(y, T, "agp", bounds=box, mask=mask)
        assert seen == []                                # None: the process-wide setting is left alone
        gp.prune_pipe = False
        got = gp.acquire(y, T, "agp", bounds=box, mask=mask)
        assert seen == [(0, 1), (1, 0)]                  # off for the call, and put back
        assert got[0] == want[0] and sp._bits(got[1]) == sp._bits(want[1])
        b_off = gp.prune_bounds(y, T, "agp", bounds=box, mask=mask).view(np.int64)
        assert seen[2:] == [(0, 1), (1, 0)]
        # a refit: new y, then the training set computed again
        y2 = np.cos(3.0 * y) + 0.1 * y
        del seen[:]
        got2 = gp.acquire(y2, T, "agp", bounds=box, mask=mask)
        gp.compute(gp._x)
        got3 = gp.acquire(y2, T, "agp", bounds=box, mask=mask)
        assert gp.prune_pipe is False and seen == [(0, 1), (1, 0)] * 2
        assert got2[0] == got3[0] and sp._bits(got2[1]) == sp._bits(got3[1])
        gp.prune_pipe = True
        b_on = gp.prune_bounds(y, T, "agp", bounds=box, mask=mask).view(np.int64)
        assert seen[-2:] == [(1, 1), (1, 1)]
    finally:
        gp.sweep_prune, gp.prune_pipe = None, None
    assert lib.apgp_get_prune_pipe() == 1
    assert np.array_equal(b_on, b_off)
