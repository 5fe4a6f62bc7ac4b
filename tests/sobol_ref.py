# -*- coding: utf-8 -*-
"""NumPy restatement of the quasi-random draws (csrc/sobol.hip, DESIGN.md "Quasi-random draws") -- test infrastructure
like philox_ref.py, prior_ref.py and evidence_ref.py: the checker the device is held to, never the thing shipped.  No GPU,
no library import.

Direction numbers: torch.quasirandom.SobolEngine(33).sobolstate, V[d][b] (30-bit); V32 = V << 2.
Point g (0 <= g < 2^30): gray = g ^ (g >> 1); x[d] = XOR over the set bits b of gray of V32[d][b]; x / 2^32 is row g of
SobolEngine(D).draw().
Scramble (nested uniform, hash-based; Laine-Karras as in Burley 2020), per dimension: x <- rev32(lk(rev32(x), h_d)),
  lk(v, h): v += h; v ^= v * 0x6c50b47c; v ^= v * 0xb82f1e52; v ^= v * 0xc7afe638; v ^= v * 0x8d22f6e6  (uint32),
  h_d = word 0 of Philox4x32-10 with counter (d, replicate, 0, 0x534f424c "SOBL"), key = seed.
Uniform: u = (x + 0.5) 2^-32.
Transforms: box / Uniform factor fma(span, u, lo) (prior_ref.fma_exact); Gaussian factor prior_ref.gaussian; mixture:
Sobol dimensions 0 .. D - 1 give z_d = gaussian(0, 1, u_d), dimension D picks the first k with u < cumw[k], t = c_k + A_k z."""
import functools

import numpy as np

from evidence_ref import cumulative
from philox_ref import philox4x32_10
from prior_ref import fma_exact, gaussian

DIMS, BITS = 33, 30
MAX_ROWS = 1 << BITS
SOBOL_TAG = 0x534F424C
_M32 = np.uint64(0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def directions():
    """V[d][b] as torch holds it: (33, 30) int64 of 30-bit values."""
    import torch
    v = torch.quasirandom.SobolEngine(DIMS).sobolstate.numpy().astype(np.int64)
    assert v.shape == (DIMS, BITS)
    return v


def points(m, D, offset=0):
    """x (m, D) uint64 of 32-bit values: rows offset .. offset + m - 1 of the unscrambled sequence."""
    assert 1 <= D <= DIMS and 0 <= offset and offset + m <= MAX_ROWS
    v32 = (directions()[:D].astype(np.uint64) << np.uint64(2))
    g = np.arange(m, dtype=np.uint64) + np.uint64(offset)
    gray = g ^ (g >> np.uint64(1))
    x = np.zeros((m, D), dtype=np.uint64)
    for b in range(BITS):
        bit = ((gray >> np.uint64(b)) & np.uint64(1)).astype(bool)
        x[bit] ^= v32[None, :, b]
    return x


def rev32(v):
    v = np.asarray(v, dtype=np.uint64) & _M32
    out = np.zeros_like(v)
    for b in range(32):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return out


def lk(v, h):
    """The Laine-Karras hash in uint32 arithmetic (values held in uint64)."""
    v = (np.asarray(v, dtype=np.uint64) + np.asarray(h, dtype=np.uint64)) & _M32
    for c in (0x6C50B47C, 0xB82F1E52, 0xC7AFE638, 0x8D22F6E6):
        v = v ^ ((v * np.uint64(c)) & _M32)
    return v


def hash_seeds(D, seed, replicate):
    """h_d, d = 0 .. D - 1 (uint64 array of 32-bit values)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10(np.arange(D, dtype=np.uint64), int(replicate), 0, SOBOL_TAG, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
    return c[0]


def scrambled(m, D, seed, replicate=0, offset=0, scramble=True):
    """x (m, D) uint64 of 32-bit values after the scramble (``scramble=False``: the plain points)."""
    x = points(m, D, offset)
    if not scramble:
        return x
    return rev32(lk(rev32(x), hash_seeds(D, seed, replicate)[None, :]))


def uniforms(m, D, seed, replicate=0, offset=0, scramble=True):
    """u = (x + 0.5) 2^-32, exact in float64."""
    return (scrambled(m, D, seed, replicate, offset, scramble).astype(np.float64) + 0.5) * 2.0 ** -32


def box(m, lo, hi, seed, replicate=0, offset=0, scramble=True):
    """fma(hi - lo, u, lo), correctly rounded."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    u = uniforms(m, len(lo), seed, replicate, offset, scramble)
    return fma_exact((hi - lo)[None, :], u, lo[None, :])


def prior(m, kind, p0, p1, seed, replicate=0, offset=0, scramble=True):
    """(T (m, D), u (m, D)): a Uniform factor (kind 0, p0 = low, p1 = high) as ``box``, a Gaussian one (kind 1, p0 = mu,
    p1 = sigma) prior_ref.gaussian."""
    kind = np.asarray(kind)
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    u = uniforms(m, len(kind), seed, replicate, offset, scramble)
    out = np.empty_like(u)
    for d in range(len(kind)):
        if kind[d] == 0:
            out[:, d] = fma_exact(p1[d] - p0[d], u[:, d], p0[d])
        else:
            out[:, d] = gaussian(p0[d], p1[d], u[:, d])
    return out, u


def mixture(m, weights, means, covs, seed, replicate=0, offset=0, scramble=True, covScale=1.0):
    """(T, component, z, near, A) as evidence_ref.mix_candidates_numpy returns them, from the Sobol uniforms: dimensions
    0 .. D - 1 the normals, dimension D the component."""
    means = np.atleast_2d(np.asarray(means, dtype=np.float64))
    covs = np.asarray(covs, dtype=np.float64)
    K, D = means.shape
    _, cum = cumulative(weights)
    u = uniforms(m, D + 1, seed, replicate, offset, scramble)
    uc = u[:, D]
    comp = np.minimum(np.searchsorted(cum, uc, side="right"), K - 1)          # the first k with u < cum[k]
    near = np.zeros(m, dtype=bool)
    for k in range(K - 1):
        near |= np.abs(uc - cum[k]) <= np.spacing(cum[k])
    z = gaussian(0.0, 1.0, u[:, :D])
    A = np.array([np.linalg.cholesky(covScale * covs[k]) for k in range(K)])
    T = means[comp] + np.einsum("mij,mj->mi", A[comp], z)
    return T, comp, z, near, A


def replicates_summary(logZ, means):
    """(logZErr, meanErr) of utility.importanceReplicatesSummary from the replicates' logZ (R,) and means (R, D)."""
    logZ, means = np.asarray(logZ, dtype=float), np.asarray(means, dtype=float)
    R = len(logZ)
    Z = np.exp(logZ - logZ.max())
    return np.std(Z, ddof=1) / np.sqrt(R) / np.mean(Z), np.std(means, axis=0, ddof=1) / np.sqrt(R)
