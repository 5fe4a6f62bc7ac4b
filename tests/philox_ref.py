"""NumPy restatement of the device's counter-based RNG (csrc/ensemble.hip: philox4x32, u01) and of the candidate generator
box_candidates_kernel -- test infrastructure: the GPU tests pin the kernels to it, the gloo test's stub GP draws its
candidates with it, ensemble_ref.py replays the ensemble sampler's stretch moves with it."""
import numpy as np

_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def _u32(v):
    return np.asarray(v, dtype=np.uint64) & _MASK


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011), as csrc/ensemble.hip philox4x32: counter (c0, c1, c2, c3), key (k0, k1).
    Arguments are 32-bit values held in ``uint64`` arrays or Python ints, broadcast against each other; returns the four
    output words as ``uint64`` arrays of 32-bit values."""
    c = list(np.broadcast_arrays(_u32(c0), _u32(c1), _u32(c2), _u32(c3), _u32(k0), _u32(k1)))
    c = [np.array(v, copy=True) for v in c]
    k0, k1 = c[4], c[5]
    c = c[:4]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _MASK, p0 & _MASK]
        k0 = (k0 + _W0) & _MASK
        k1 = (k1 + _W1) & _MASK
    return c


def u01(a, b):
    """csrc/ensemble.hip u01: the 53-bit uniform in (0, 1) from two 32-bit words (27 high bits of a, 26 of b, + 1/2)."""
    a, b = _u32(a), _u32(b)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64) + 0.5) \
        / 9007199254740992.0


def philox_box_numpy(m, D, lo, hi, seed, offset):
    """NumPy restatement of csrc/ensemble.hip box_candidates_kernel: Philox4x32-10, counter = (row low, row high, d / 2,
    0x43414e44), key = seed; u = 53-bit uniform in (0, 1); value = fma(span, u, lo) (the product span * u is exact enough to
    compare to 1 ulp: the kernel fuses it)."""
    rows = (np.arange(m, dtype=np.uint64) + np.uint64(offset))
    out = np.empty((m, D))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for d in range(0, D, 2):
        c = philox4x32_10(rows & _MASK, rows >> np.uint64(32), d >> 1, 0x43414E44, k0, k1)
        out[:, d] = lo[d] + (hi[d] - lo[d]) * u01(c[0], c[1])
        if d + 1 < D:
            out[:, d + 1] = lo[d + 1] + (hi[d + 1] - lo[d + 1]) * u01(c[2], c[3])
    return out
