# -*- coding: utf-8 -*-
"""NumPy replay of the matrix-core coarse bound of the pruned arg-min (csrc/prune_mm32.h; DESIGN.md section 4, "The
bound in two stages"): the exponent of every kernel value as the fp32 fma chain v_mfma_f32_32x32x2_f32 runs, in the
shipped order of the entries, the fp32 partial sums over a lane's 16 rows, and the slack term by term.

The fma is emulated by the fp64 product of two fp32 numbers (exact) added to the fp32 accumulator in fp64 and rounded to
fp32; the second rounding can differ from a true fma in the last bit in rare halfway cases, which the bound on the
exponent's error covers either way (it charges a full rounding to every step)."""
import numpy as np

import prune_ref

U32 = 2.0 ** -24
EPS = 2.0 ** -53
KAPPA = float.fromhex("0x1.337cc2183b050p+0")          # sqrt(log2(e)), PR32_KAPPA
LN2 = float(np.log(2.0))
F = np.float32


def dpad_of(d):
    return 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def entries(dpad):
    """The chain's order: step s adds entry s (lane half 0), then entry KH + s (lane half 1).  Entry 0: -|b|^2 * 1,
    entry 1: 1 * -|a|^2, entry 2 + d: 2 b_d * a_d."""
    kh = (dpad + 2) // 2
    order = []
    for s in range(kh):
        order += [s, kh + s]
    return order


def operands(ce, dpad, use=None):
    """fp64 centred coordinates (rows, D) -> fp32 coordinates padded to dpad and the fp32 norm, as the kernel forms them."""
    n, d = ce.shape
    f = np.zeros((n, dpad), dtype=F)
    f[:, :d] = (ce * KAPPA).astype(F)
    if use is not None:
        f[~use] = 0.0
    nrm = (f.astype(np.float64) ** 2).sum(axis=1).astype(F)
    return f, nrm


def replay(X, alpha, T, sc, amp=1.0, xs=None):
    """Everything the kernel computes for candidates T (m, D) against the training set X (n, D) with weights alpha,
    per-dimension scale sc (k = amp exp(-|sc (t - x)|^2)); dict of per-candidate arrays.  Also the exact values.
    xs: the scaled training rows where the caller has them (the device's packed stream) in the place of X * sc."""
    X = np.asarray(X, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    n, d = X.shape
    m = T.shape[0]
    dpad = dpad_of(d)
    xs = X * sc if xs is None else np.asarray(xs, dtype=np.float64)
    ts = T * sc
    c = xs[0].copy()
    cn = np.sqrt((c * c).sum())
    ca = ts - c
    cb = xs - c
    an = np.sqrt((ca * ca).sum(axis=1))
    bn = np.sqrt((cb * cb).sum(axis=1).max())
    af, na = operands(ca, dpad, use=(ca * ca).sum(axis=1) <= 2.0 ** 100)
    bf, nb = operands(cb, dpad)
    # P (training rows) and Q (candidates), entry by entry
    P = np.concatenate([-nb[:, None], np.ones((n, 1), dtype=F), F(2.0) * bf], axis=1)
    Q = np.concatenate([np.ones((m, 1), dtype=F), -na[:, None], af], axis=1)
    order = entries(dpad)
    # exact exponent (natural units) from the fp64 inputs t sc and x
    ld = np.longdouble
    ex = -((ts.astype(ld)[:, None, :] - xs.astype(ld)[None, :, :]) ** 2).sum(axis=2)          # (m, n)
    k_true = np.exp(ex)
    mu_true = amp * (k_true * alpha.astype(ld)[None, :]).sum(axis=1)
    S_true = amp * (k_true * np.abs(alpha).astype(ld)[None, :]).sum(axis=1)
    al32 = alpha.astype(F)
    acc_m = np.zeros(m)
    acc_s = np.zeros(m)
    sal = 0.0
    exp_err = np.zeros(m)
    khat_max = np.zeros(m)
    for t0 in range(0, n, 32):
        for h in (0, 1):
            rows = [(r & 3) + 8 * (r >> 2) + 4 * h + t0 for r in range(16)]
            ps = np.zeros(m, dtype=F)
            pS = np.zeros(m, dtype=F)
            pa = F(0.0)
            for i in rows:
                if i >= n:                               # a padding row: operands 0, alpha 0 -- adds exactly 0
                    continue
                e = np.zeros(m, dtype=F)
                for j in order:
                    e = _fma32(np.broadcast_to(P[i, j], (m,)), Q[:, j], e)
                exp_err = np.maximum(exp_err, np.abs(e.astype(ld) * ld(LN2) - ex[:, i]).astype(np.float64))
                with np.errstate(under="ignore"):
                    k = np.exp2(e).astype(F)
                k[np.abs(k) < 2.0 ** -126] = 0.0         # v_exp_f32 flushes
                khat_max = np.maximum(khat_max, k)
                ps = _fma32(k, np.broadcast_to(al32[i], (m,)), ps)
                pS = _fma32(k, np.broadcast_to(np.abs(al32[i]), (m,)), pS)
                pa = F(pa + np.abs(al32[i]))
            acc_m += ps.astype(np.float64)
            acc_s += pS.astype(np.float64)
            sal += float(pa)
    sa = sal * (1.0 + 2.0 ** -16)
    s32 = acc_s * (1.0 + 2.0 ** -16)
    eta0, eta = eta_of(an, bn, cn, dpad)
    gate = eta <= 2.0 ** -8
    e32 = np.where(gate, amp * (np.expm1(eta) * (1.0 + 2.0 ** -20) * s32 + 2.0 ** -120 * (sa + n)), np.inf)
    return {"mu32": amp * acc_m, "mu": mu_true.astype(np.float64), "S": S_true.astype(np.float64), "S32": s32, "sa": sa,
            "eta0": eta0, "eta": eta, "gate": gate, "e32": e32, "exp_err": exp_err, "khat_max": khat_max, "A": an,
            "B": bn, "c": cn, "dpad": dpad, "n": n}


def eta_of(A, B, cn, dpad):
    """The exponent's error bound eta0 and the relative error bound eta of one product alpha k^, term by term."""
    K = dpad + 2
    ab = A + B
    conv = 2.01 * U32 * ab * ab                          # a, b -> fp32
    norms = 1.0 * U32 * ab * ab                          # |a^|^2, |b^|^2 rounded once each, no low parts
    chain = K * U32 * ab * ab                            # one rounding per entry, partial sums <= (A + B)^2
    room = 0.99 * U32 * ab * ab                          # fp64 roundings of a, b, kappa, the norms; (1 + u)^K
    centre = 2.5 * EPS * ab * (cn + A)                   # t sc - c contracted to one fma
    eta0 = conv + norms + chain + room + centre          # = (K + 4) u (A + B)^2 + centre
    eta = eta0 + 24.0 * U32                              # v_exp_f32 4.1 u, alpha 1.01 u, 16 fma 16.1 u, room
    return eta0, eta


def slack(kind, b, mu, ktt, r, zeta=0.01, ybest=0.0):
    """prune_bound_mm32_kernel's slack for the rows of a replay r: twice e32 (|du/dmu| <= 2) on top of
    prune_bound_kernel's with S <= amp sum|alpha|."""
    return 2.0 * r["e32"] + prune_ref.slack(kind, b, mu, ktt, ktt * r["sa"], r["n"], r["dpad"], zeta, ybest)
