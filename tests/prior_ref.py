"""NumPy restatement of csrc/ensemble.hip prior_candidates_kernel (candidates drawn from a priors.JointPrior) -- test
infrastructure like philox_ref.py: the checker the device is held to, never the thing shipped.

The stream is box_candidates_kernel's: Philox4x32-10, counter = (row low, row high, d / 2, 0x43414e44), key = seed, words
0, 1 give dimension d and words 2, 3 dimension d + 1; u = the 53-bit uniform of philox_ref.u01.
* Uniform (kind 0, p0 = low, p1 = high): the kernel computes fma(high - low, u, low).  ``fused=True`` restates that fused
  multiply-add exactly (rational arithmetic, correctly rounded), ``fused=False`` is philox_box_numpy's low + (high - low) u.
* Gaussian (kind 1, p0 = mu, p1 = sigma): mu + (sigma * sqrt(2)) * erfcinv(2 * (1 - u)), each operation rounded in this
  order -- GaussianPrior.transform_uniform's expression, with scipy's erfcinv in place of the device's."""
from fractions import Fraction

import numpy as np
from scipy.special import erfcinv

from philox_ref import philox4x32_10, u01

_MASK = np.uint64(0xFFFFFFFF)


def uniforms(m, D, seed, offset):
    """(m, D) uniforms of rows offset .. offset + m - 1 of the candidate stream keyed by ``seed``."""
    rows = np.arange(m, dtype=np.uint64) + np.uint64(offset)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF
    out = np.empty((m, D))
    for d in range(0, D, 2):
        c = philox4x32_10(rows & _MASK, rows >> np.uint64(32), d >> 1, 0x43414E44, k0, k1)
        out[:, d] = u01(c[0], c[1])
        if d + 1 < D:
            out[:, d + 1] = u01(c[2], c[3])
    return out


def fma_exact(a, b, c):
    """Correctly rounded a * b + c elementwise (what the device's fma returns), by exact rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                  np.asarray(c, dtype=np.float64))
    flat = [float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]
    return np.array(flat, dtype=np.float64).reshape(a.shape)


def gaussian(mu, sigma, u, erfcinv_fn=erfcinv):
    """mu + (sigma * sqrt(2)) * erfcinv(2 * (1 - u)), in that order."""
    return mu + sigma * np.sqrt(2.0) * erfcinv_fn(2.0 * (1.0 - u))


def prior_candidates_numpy(m, kind, p0, p1, seed, offset, fused=True):
    """Rows offset .. offset + m - 1 of the candidate matrix the device draws from the per-dimension records
    (kind, p0, p1) of a JointPrior (JointPrior.records())."""
    kind = np.asarray(kind)
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    D = len(kind)
    u = uniforms(m, D, seed, offset)
    out = np.empty((m, D))
    for d in range(D):
        if kind[d] == 0:
            span = p1[d] - p0[d]
            out[:, d] = fma_exact(span, u[:, d], p0[d]) if fused else p0[d] + span * u[:, d]
        else:
            out[:, d] = gaussian(p0[d], p1[d], u[:, d])
    return out
