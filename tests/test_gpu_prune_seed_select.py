# -*- coding: utf-8 -*-
"""MI355X: prune_seed_kernel alone (the apgp_sweep_prune_seeds hook) against np.lexsort: the 16 smallest (value, block)
pairs below +inf, ascending by value and then by block number, fewer if fewer exist, counts = (ns, 0, ., 0).

The kernel's 1024 threads take the blocks in chunks of 16 x 1024: thread t holds blocks base + t + 1024 j (j < 16) of a
chunk.  The largest of the 16 wavefronts' smallest pairs bounds the 16th smallest of all; the pairs at or below it go to
a list of 256 and are ranked by counting.  A list that overflows is dropped, and every wavefront selects the 16 smallest
of what its lanes hold, chunk after chunk (from the second on only values below its 16th so far enter).

Sizes: ncb = 1, 15, 16, 17 (around the number of seeds), 64 (one wavefront's lanes), 256 and 257 (the list's length),
1025 (a second value in thread 0 alone), 15625 (C3: almost one chunk), 16384 and 16385 (exactly one chunk; one block
into the second), 50000 (four chunks).
Inputs: random with +inf and -inf entries; ties everywhere, across threads, wavefronts and chunks; all equal; all +inf;
NaN entries (not below +inf: never a seed); fewer than 16 finite entries, the last block among them; the 16 smallest
all in ONE thread's strided share; the smallest values all in the last chunk, and all in the first (later chunks then
add nothing).  Made to overflow the list: one wavefront's whole share at +inf, so that nothing bounds the 16th
smallest; the same with ties; values ascending with the block number, so that the wavefronts' minima are a chunk's
first blocks and 961 pairs lie at or below the largest of them; descending.  (By a host model of the filter these,
"ties" and "all -inf" overflow at every size from 257 on, where both routes are therefore taken; up to 256 blocks
everything is listed and ranked.)"""
import ctypes

import numpy as np
import pytest

import prune_ref as pr

pytestmark = pytest.mark.gpu

NCB = [1, 15, 16, 17, 64, 256, 257, 1025, 15625, 16384, 16385, 50000]
THREADS = 1024


def _inputs(ncb, rs):
    out = {}
    b = rs.normal(size=ncb)
    b[rs.uniform(size=ncb) < 0.2] = np.inf
    b[rs.uniform(size=ncb) < 0.01] = -np.inf
    out["random, +-inf"] = b
    b = np.round(rs.normal(size=ncb), 1)                              # ties everywhere, the smallest values included
    b[rs.uniform(size=ncb) < 0.3] = b.min()
    out["ties"] = b
    b = rs.normal(size=ncb)                                           # one tie per thread slice, wavefront and chunk
    b[::37] = -7.0
    out["ties across slices"] = b
    out["all -inf"] = np.full(ncb, -np.inf)                           # all equal: the first 16 block numbers
    out["all +inf"] = np.full(ncb, np.inf)                            # nothing admissible
    b = rs.normal(size=ncb)
    b[rs.uniform(size=ncb) < 0.5] = np.nan
    b[0] = np.nan
    out["NaN"] = b
    b = np.full(ncb, np.inf)                                          # fewer than 16 below +inf, at the far end too
    b[rs.choice(ncb, size=min(ncb, 7), replace=False)] = rs.normal(size=min(ncb, 7))
    b[ncb - 1] = 0.5
    out["7 finite"] = b
    for t in (0, 700):                                                # the 16 smallest in ONE thread's strided share
        if t < ncb:
            b = rs.normal(size=ncb)
            k = len(b[t::THREADS])
            b[t::THREADS] = -10.0 - rs.permutation(k)
            out["one thread %d" % t] = b
    b = rs.normal(size=ncb)                                           # the smallest at the far end: the last chunk
    b[-min(ncb, 40):] -= 20.0
    out["far end"] = b
    b = rs.normal(size=ncb)                                           # ... and at the near end: later chunks add nothing
    b[:min(ncb, 40)] -= 20.0
    out["near end"] = b
    hole = (np.arange(ncb) % THREADS) // 64 == 5                      # wavefront 5 sees +inf only: no bound, long list
    b = rs.normal(size=ncb)
    b[hole] = np.inf
    out["wavefront 5 empty"] = b
    b = np.round(rs.normal(size=ncb), 1)
    b[hole] = np.inf
    out["wavefront 5 empty, ties"] = b
    b = np.sort(rs.normal(size=ncb))
    out["ascending"] = b
    out["descending"] = b[::-1].copy()
    return out


@pytest.mark.parametrize("ncb", NCB)
def test_seeds_against_lexsort(ncb):
    import torch
    from approxposterior_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, bmin in _inputs(ncb, np.random.RandomState(ncb)).items():
        want = pr.seeds(bmin)
        assert np.array_equal(want, [i for i in np.lexsort((np.arange(ncb), bmin)) if bmin[i] < np.inf][:16])
        b_d = torch.from_numpy(bmin).to(dev)
        s_d = torch.full((16,), -5, dtype=torch.int64, device=dev)
        c_d = torch.full((4,), -7, dtype=torch.int64, device=dev)
        _lib.check(lib.apgp_sweep_prune_seeds(b_d.data_ptr(), ncb, s_d.data_ptr(), c_d.data_ptr(), st),
                   "apgp_sweep_prune_seeds")
        torch.cuda.synchronize()
        c = c_d.cpu().numpy()
        s = s_d.cpu().numpy()
        assert c[0] == len(want) and c[1] == 0 and c[2] == -7 and c[3] == 0, (ncb, name, c, want)
        assert np.array_equal(s[:len(want)], want), (ncb, name, s, want)
        assert np.all(s[len(want):] == -5), (ncb, name, s)            # nothing written past the count
