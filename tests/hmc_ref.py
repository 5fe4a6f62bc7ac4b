"""NumPy restatement of the on-device Hamiltonian Monte Carlo sampler (csrc/hmc.hip) -- the checker the device is held to,
never the thing shipped.  Everything is in the kernel's scaled coordinates q = theta * sc, sc = sqrt(inv_metric / 2).

The recipe (chain c, global iteration i = iteration0 + it; Philox4x32-10 under ``ensemble_ref.stream_keys(seed, c)``):

* momentum   p_d = sqrt(-2 log u) cospi(2 u') sqrt(m_d), (u, u') = u01 of words (0, 1), (2, 3) of counter (i, i >> 32, d, 8)
* step       eps_i = eps (1 + jitter (2 u - 1)), u = u01 of words 0, 1 of counter (i, i >> 32, 0xffffffff, 9) under the keys
             of chain 0: the same for every chain
* L steps    p += (eps_i / 2) g(q);  q += (eps_i / m) p;  reflect;  p += (eps_i / 2) g(q)            (g = d mu / d q)
* canonical  the end point of the LAST drift, after reflection, is replaced by q = th sc with th = clamp(q / sc) to the box
             in the caller's coordinates, before its gradient is taken: what is stored (th) is exactly what a
             following call starts from.  It moves q by at most 2 u |q|
* reflect    while q_d is outside a finite face: q_d = 2 face - q_d, p_d = -p_d, at most MAX_REFLECT times; still outside
             then, or q or p not finite: a divergence
* accept     dH = (K(p_L) - mu(q_L)) - (K(p_0) - mu(q_0)), K = sum_d p_d^2 (0.5 / m_d); accept iff log u < -dH, u = u01 of
             words 0, 1 of counter (i, i >> 32, 0xfffffffe, 10); dH not finite or > 1000: rejected, a divergence; a start
             outside the box has mu = -inf and never moves.

The target's mean and gradient, from the oracle's alpha (``Model``), with x_n the scaled training rows:
    mu(q)  = mean + sum_n alpha_n [ amp exp(-|q - x_n|^2) + lin_coef sum_d (q_d x_nd lw_d)^P ]
    g_d(q) = sum_n alpha_n [ -2 amp exp(-|q - x_n|^2) (q_d - x_nd) + lin_coef P (q_d x_nd lw_d)^(P - 1) x_nd lw_d ]
``Model.mg`` evaluates them in numpy.longdouble (64-bit significand: its own error is 2^-11 of a double's and is not
charged) and returns, beside them, the ROUNDING BUDGETS of the device's fp64 evaluation.

Budgets (u = 2^-53, first order; nothing is fitted to a device's output and nothing depends on cond(K) -- alpha is an
input).  One term of the sums is alpha_n J_nd with J = J_se + J_lin.
  k_se     the kernel-value budget of tests/kvalue_ref.py in scaled coordinates: the argument S = |q - x_n|^2 carries
           2 u per df_d^2 (the subtraction), 2 |df_d| |x_nd| u (x_n = x sc was rounded once; q is the device's own
           number and exact), and ceil(DPAD / 2) + 1 <= D + 1 roundings of the two-accumulator sum, u S each:
           dS <= u [(D + 3) S + 2 sum_d |df_d| |x_nd|]; exp: E_EXP = 1.5 ulp <= 3 u; amp *: u.  rel(k_se) <= dS + 4 u.
  J_se     (-2 k) df: df rounds once, the product once (-2 k is exact): rel <= rel(k_se) + 2 u.
  J_lin    xl = x lw: lw 1 rounding, x 1, product 1 = 3 u; p = q xl: 4 u; p^(P - 1): (P - 1) 4 u + (P - 2) u; the
           coefficient lin_coef P p^(P-1): 2 u; times xl: 3 u, the fma 1 u: rel <= (5 P + 8) u.
  k_lin    sum_d p^(P - 1) p by fma: per term (P - 1) 4 u + P u + 4 u <= (5 P + 4) u, D roundings of the sum, the closing
           fma 1: rel <= (5 P + D + 5) u of sum_d |p_d|^P.
  sums     a lane adds its rows in order with one rounded fma each: R = ceil(Npad / (64 G)) roundings; the butterfly adds
           6, the group's partials G - 1, the mean 1 (mu only): (R + 6 + G) u sum_n |alpha_n J_nd|.
  B_g[d] = u sum_n |alpha_n| [ |J_se| (dS / u + 6) + |J_lin| (5 P + 8) ] + (R + 6 + G) u sum_n |alpha_n J_nd|
  B_mu   = u sum_n |alpha_n| [ k_se (dS / u + 4) + |k_lin| (5 P + D + 5) ] + (R + 7 + G) u sum_n |alpha_n k_n| + u |mu|
A step from the device's own (q, p) (``forced``):
  eps_i    1 + jitter (2 u - 1) may or may not be contracted into an fma: eps_i within 2 u; eps_i / 2 exact; eps_i / m: u.
           The device rounds an fma once; this file rounds the product and the sum: both are charged.
  half kick p1 = fma(he, g, p):  B_p1 = B_p + he B_g + 5 u |he g| + 2 u |p1|
  drift    q1 = fma(em, p1, q):  B_q = em B_p1 + 6 u |em p1| + 2 u |q1|, plus u (2 |face| + |q|) per reflection, plus
           3 u |q1| on the last step (the device's canonical end point; ``forced`` does not round its own)
  kick     p2 = fma(he, g(q1), +-p1), g at the DEVICE's q1:  B_p2 = B_p1 + he B_g(q1) + 5 u |he g(q1)| + 2 u |p2|
  p_0      the Box-Muller normal: log, sqrt, cospi of the device's libm within 4 ulp together with the products, doubled
           for the reference's own: B_p0 = 16 u |p_0|.
  K        terms p^2 (0.5 / m): 2 roundings, the butterfly 6, 0.5 / m 1: 9 u K; K(p_0) adds 32 u K (B_p0).
  B_dH   = B_mu(q_0) + B_mu(q_L) + 9 u (K_0 + K_L) + 32 u K_0 + u (|H_0| + |H_L| + |dH|)
A decision is a NEAR-TIE when |log u + dH| <= B_dH + 4 u |log u|; a drift is NEAR A FACE when, before or between
reflections, q_d lies within 1e-12 of the span (of max(1, |face|) where the span is infinite) of a face.  Those are not
compared; the GPU test caps their share."""
import numpy as np

from ensemble_moves_ref import cospi
from ensemble_ref import stream_keys
from philox_ref import philox4x32_10, u01

U = 2.0 ** -53
MAX_REFLECT = 8
NEAR_FACE = 1e-12
NEAR_CAP = 0.02           # share of near-tie decisions / near-face drifts a replay case may have
_MASK = np.uint64(0xFFFFFFFF)
LD = np.longdouble


def dpad(d):
    return 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def npad(n):
    return (n + 63) // 64 * 64


class Model(object):
    """The surrogate in scaled coordinates: xs (n, D) = x * sc, alpha (n,), and the kernel's constants."""

    def __init__(self, xs, alpha, mean, amp=1.0, lin_coef=0.0, lin_order=0, lw=None, sc=None):
        self.xs = np.ascontiguousarray(xs, dtype=np.float64)
        self.alpha = np.asarray(alpha, dtype=np.float64)
        self.n, self.D = self.xs.shape
        self.mean, self.amp, self.lin_coef, self.P = float(mean), float(amp), float(lin_coef), int(lin_order)
        self.lw = np.ones(self.D) if lw is None else np.asarray(lw, dtype=np.float64)
        self.sc = np.ones(self.D) if sc is None else np.asarray(sc, dtype=np.float64)

    @classmethod
    def from_gps(cls, gp, gpo, y):
        """From the package's GP (the kernel's constants, host arithmetic only) and the oracle GP (alpha, in float64 SciPy)."""
        ks = gp._kernel_struct()
        D = ks.ndim
        im = np.array(ks.inv_metric[:D], dtype=np.float64)
        sc = np.sqrt(0.5 * im)
        return cls(np.asarray(gpo._x, dtype=np.float64) * sc, gpo._compute_alpha(np.asarray(y, dtype=np.float64), False),
                   float(gpo.mean.value), ks.amp, ks.lin_coef, ks.lin_order, 2.0 / im, sc)

    def mg(self, q, G=1, budgets=False):
        """mu (M,), g (M, D) at the scaled points q (M, D) as float64 [, B_mu (M,), B_g (M, D)] (module docstring)."""
        q = np.asarray(q, dtype=np.float64).reshape(-1, self.D)
        M, D, P = len(q), self.D, self.P
        mu, g = np.empty(M), np.empty((M, D))
        Bmu, Bg = np.zeros(M), np.zeros((M, D))
        xs, al, lw = self.xs.astype(LD), self.alpha.astype(LD), self.lw.astype(LD)
        aal = np.abs(al)
        R = -(-npad(self.n) // (64 * G))
        step = max(1, int(2e6 // (self.n * D)))
        for i in range(0, M, step):
            qq = q[i:i + step].astype(LD)
            df = qq[:, None, :] - xs[None]                                  # (m, n, D)
            S = np.sum(df * df, axis=2)
            kse = LD(self.amp) * np.exp(-S)
            Jse = -2.0 * kse[:, :, None] * df
            k, J = kse, Jse
            if self.lin_coef != 0.0:
                xl = xs * lw
                p = qq[:, None, :] * xl[None]
                if P == 0:
                    klin = np.full(S.shape, LD(self.lin_coef) * D)
                    kabs = np.abs(klin)
                    Jlin = np.zeros_like(df)
                else:
                    pw = p ** (P - 1)
                    klin = LD(self.lin_coef) * np.sum(pw * p, axis=2)
                    kabs = LD(self.lin_coef) * np.sum(np.abs(pw * p), axis=2)
                    Jlin = LD(self.lin_coef) * P * pw * xl[None]
                k, J = kse + klin, Jse + Jlin
            m_ = np.sum(al[None] * k, axis=1) + LD(self.mean)
            mu[i:i + step] = m_.astype(np.float64)
            g[i:i + step] = np.sum(al[None, :, None] * J, axis=1).astype(np.float64)
            if budgets:
                dS = (D + 3) * S + 2.0 * np.sum(np.abs(df) * np.abs(xs)[None], axis=2)         # in units of u
                bm = np.sum(aal[None] * kse * (dS + 4.0), axis=1) + (R + 7 + G) * np.sum(aal[None] * np.abs(k), axis=1) \
                    + np.abs(m_)
                bg = np.sum(aal[None, :, None] * np.abs(Jse) * (dS[:, :, None] + 6.0), axis=1) \
                    + (R + 6 + G) * np.sum(aal[None, :, None] * np.abs(J), axis=1)
                if self.lin_coef != 0.0:
                    bm = bm + np.sum(aal[None] * kabs, axis=1) * (5 * P + D + 5)
                    bg = bg + np.sum(aal[None, :, None] * np.abs(Jlin), axis=1) * (5 * P + 8)
                Bmu[i:i + step] = (U * bm).astype(np.float64)
                Bg[i:i + step] = (U * bg).astype(np.float64)
        return (mu, g, Bmu, Bg) if budgets else (mu, g)


class Gaussian(object):
    """An analytic Gaussian 'surrogate': mu(q) = -1/2 (q - c)' A (q - c), for the free-run statistics."""

    def __init__(self, centre, cov):
        self.c, self.A = np.asarray(centre, dtype=np.float64), np.linalg.inv(np.asarray(cov, dtype=np.float64))
        self.D = len(self.c)

    def mg(self, q, G=1, budgets=False):
        r = np.asarray(q, dtype=np.float64).reshape(-1, self.D) - self.c
        Ar = r @ self.A
        return -0.5 * np.sum(r * Ar, axis=1), -Ar


def draws(its, chains, D, seed):
    """Random numbers of global iterations ``its`` (T,) for the chains ``chains`` (C,): the unit normals ``z`` (T, C, D),
    the jitter uniforms ``uj`` (T,) and the acceptance uniforms ``ua`` (T, C)."""
    its = np.asarray(its, dtype=np.uint64).reshape(-1)
    chains = np.asarray(chains, dtype=np.int64).reshape(-1)
    keys = [stream_keys(seed, int(c)) for c in chains]
    k0 = np.array([k[0] for k in keys], dtype=np.uint64)
    k1 = np.array([k[1] for k in keys], dtype=np.uint64)
    lo, hi = (its & _MASK)[:, None, None], (its >> np.uint64(32))[:, None, None]
    c8 = philox4x32_10(lo, hi, np.arange(D, dtype=np.uint64)[None, None, :], 8, k0[None, :, None], k1[None, :, None])
    z = np.sqrt(-2.0 * np.log(u01(c8[0], c8[1]))) * cospi(2.0 * u01(c8[2], c8[3]))
    j0, j1 = stream_keys(seed, 0)
    c9 = philox4x32_10(lo[:, 0, 0], hi[:, 0, 0], 0xFFFFFFFF, 9, j0, j1)
    ca = philox4x32_10(lo[:, :, 0], hi[:, :, 0], 0xFFFFFFFE, 10, k0[None, :], k1[None, :])
    return z, u01(c9[0], c9[1]), u01(ca[0], ca[1])


def step_sizes(uj, eps, jitter):
    return eps * (1.0 + jitter * (2.0 * uj - 1.0))


def face_tol(lo, hi):
    span = hi - lo
    with np.errstate(invalid="ignore"):
        tl = np.where(np.isfinite(span), NEAR_FACE * span, NEAR_FACE * np.maximum(1.0, np.abs(lo)))
        th = np.where(np.isfinite(span), NEAR_FACE * span, NEAR_FACE * np.maximum(1.0, np.abs(hi)))
    # (an infinite face has nobody near it)
    return np.where(np.isfinite(lo), tl, -1.0), np.where(np.isfinite(hi), th, -1.0)


def reflect(q, p, lo, hi):
    """The reflection loop on (M, D) arrays: (q, p, count (M, D), near (M, D), out (M, D))."""
    q, p = q.copy(), p.copy()
    cnt = np.zeros(q.shape, dtype=np.int64)
    near = np.zeros(q.shape, dtype=bool)
    tl, th = face_tol(lo, hi)
    live = np.ones(q.shape, dtype=bool)
    for _ in range(MAX_REFLECT):
        with np.errstate(invalid="ignore"):
            near |= live & ((np.abs(q - lo) <= tl) | (np.abs(q - hi) <= th))
            above = live & (q > hi)
            below = live & ~above & (q < lo)
        q = np.where(above, 2.0 * hi - q, np.where(below, 2.0 * lo - q, q))
        flip = above | below
        p = np.where(flip, -p, p)
        cnt += flip
        live = flip
    with np.errstate(invalid="ignore"):
        near |= live & ((np.abs(q - lo) <= tl) | (np.abs(q - hi) <= th))
        out = ~((q >= lo) & (q <= hi)) | ~np.isfinite(p)
    return q, p, cnt, near, out


def leapfrog(target, q, p, g, eps, minv, lo, hi, canon=None):
    """One step on (M, D) arrays from (q, p) with g = g(q): (q1, p2, mu1, g1, info).  ``canon`` = (sc, lo_user, hi_user)
    makes the drift's end point canonical (the last step of a trajectory)."""
    he = 0.5 * eps
    p1 = p + he * g
    q1, p1r, cnt, near, out = reflect(q + (eps * minv) * p1, p1, lo, hi)
    if canon is not None:
        with np.errstate(invalid="ignore"):
            q1 = np.where(out, q1, np.minimum(np.maximum(q1 / canon[0], canon[1]), canon[2]) * canon[0])
    mu1, g1 = target.mg(q1)
    return q1, p1r + he * g1, mu1, g1, {"count": cnt, "near": near, "out": out}


def kinetic(p, minv):
    return np.sum((p * p) * (0.5 * minv), axis=-1)


def inside(q, lo, hi):
    return np.all((q >= lo) & (q <= hi), axis=-1)


def run(target, q0, iterations, lo, hi, eps, L, jitter=0.0, mass=None, seed=0, iteration0=0, chains=None, canon=None):
    """Free run from the scaled starts q0 (C, D) in the scaled box [lo, hi].  Returns ``chain`` (T, C, D, scaled),
    ``log_prob``, ``accept`` (T, C), ``dH``, ``margin`` (|log u + dH|), ``reflected`` (T, C: the trajectory reflected),
    ``near`` (T, C, L: a drift near a face), ``trace`` (T, C, L, 2, D: q, p after every step), ``diverge`` (T, C), ``coords``, ``final_log_prob``."""
    q = np.array(q0, dtype=np.float64)
    C, D = q.shape
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    m = np.ones(D) if mass is None else np.asarray(mass, dtype=np.float64)
    minv, sqm = 1.0 / m, np.sqrt(m)
    chains = np.arange(C) if chains is None else np.asarray(chains)
    z, uj, ua = draws(iteration0 + np.arange(iterations), chains, D, seed)
    es = step_sizes(uj, eps, jitter)
    mu, g = target.mg(q)
    mu = np.where(inside(q, lo, hi), mu, -np.inf)
    out = {k: np.zeros((iterations, C)) for k in ("log_prob", "dH", "margin")}
    out.update({k: np.zeros((iterations, C), dtype=bool) for k in ("accept", "reflected", "diverge")})
    out["chain"] = np.zeros((iterations, C, D))
    out["near"] = np.zeros((iterations, C, L), dtype=bool)
    out["trace"] = np.zeros((iterations, C, L, 2, D))
    for it in range(iterations):
        p = z[it] * sqm
        H0 = kinetic(p, minv) - mu
        qc, gc, muc = q, g, mu
        bad = np.zeros(C, dtype=bool)
        for l in range(L):
            qc, p, muc, gc, info = leapfrog(target, qc, p, gc, es[it], minv, lo, hi, canon if l == L - 1 else None)
            bad |= info["out"].any(axis=1)
            out["reflected"][it] |= info["count"].any(axis=1)
            out["near"][it, :, l] = info["near"].any(axis=1)
            out["trace"][it, :, l, 0], out["trace"][it, :, l, 1] = qc, p
        with np.errstate(invalid="ignore"):
            dH = (kinetic(p, minv) - muc) - H0
        gated = np.isneginf(mu)
        with np.errstate(invalid="ignore"):
            div = ~gated & (bad | ~np.isfinite(dH) | (dH > 1000.0))
            acc = ~gated & ~div & (np.log(ua[it]) < -dH)
            out["margin"][it] = np.abs(np.log(ua[it]) + dH)
        q = np.where(acc[:, None], qc, q)
        g = np.where(acc[:, None], gc, g)
        mu = np.where(acc, muc, mu)
        out["chain"][it], out["log_prob"][it], out["accept"][it], out["dH"][it], out["diverge"][it] = q, mu, acc, dH, div
    out["coords"], out["final_log_prob"] = q, mu
    return out


def forced(model, q0, trace, accepted, lo, hi, eps, L, jitter=0.0, mass=None, seed=0, iteration0=0, G=1):
    """Teacher-forced replay.  ``trace`` (T, C, L, 2, D) is the device's (q, p) after every step (scaled), ``accepted``
    (T, C) its decisions, q0 (C, D) the scaled starts.  Every step is recomputed from the device's own (q, p) before it
    (the momentum draw before the first), the kick's gradient at the device's drifted q.  Returns per step the
    reference ``q``, ``p`` (T, C, L, D) with the budgets ``Bq``, ``Bp``, ``near`` (T, C, L) and ``count`` (reflections, T, C,
    L), and per iteration ``dH`` with ``BdH``, ``logu``, ``accept``, ``margin``, ``gated`` (T, C)."""
    T, C, _, _, D = trace.shape
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    m = np.ones(D) if mass is None else np.asarray(mass, dtype=np.float64)
    minv, sqm = 1.0 / m, np.sqrt(m)
    z, uj, ua = draws(iteration0 + np.arange(T), np.arange(C), D, seed)
    es = step_sizes(uj, eps, jitter)
    # the state before every iteration, from the device's decisions
    state = np.empty((T + 1, C, D))
    state[0] = q0
    for it in range(T):
        state[it + 1] = np.where(accepted[it][:, None], trace[it, :, L - 1, 0], state[it])
    p0 = z * sqm                                                            # (T, C, D)
    qb = np.concatenate([state[:T, :, None], trace[:, :, :-1, 0]], axis=2)  # (T, C, L, D): q before each step
    pb = np.concatenate([p0[:, :, None], trace[:, :, :-1, 1]], axis=2)
    Bpb = np.concatenate([16.0 * U * np.abs(p0)[:, :, None], np.zeros((T, C, L - 1, D))], axis=2)
    qa = trace[:, :, :, 0]
    mua, ga, Bmua, Bga = [v.reshape((T, C, L) + v.shape[1:]) for v in model.mg(qa.reshape(-1, D), G, True)]
    # (the point before step l > 0 is the point after step l - 1: only the states are new)
    ms, gs, Bms, Bgs = [v.reshape((T, C, 1) + v.shape[1:]) for v in model.mg(state[:T].reshape(-1, D), G, True)]
    mub, gb, Bmub, Bgb = [np.concatenate([a, b[:, :, :-1]], axis=2) for a, b in
                          ((ms, mua), (gs, ga), (Bms, Bmua), (Bgs, Bga))]
    e = es[:, None, None, None]
    he, em = 0.5 * e, e * minv
    p1 = pb + he * gb
    Bp1 = Bpb + he * Bgb + 5.0 * U * np.abs(he * gb) + 2.0 * U * np.abs(p1)
    qpre = qb + em * p1
    q1, p1r, cnt, near, _ = reflect(qpre.reshape(-1, D), p1.reshape(-1, D), lo, hi)
    q1, p1r, cnt, near = [v.reshape(T, C, L, D) for v in (q1, p1r, cnt, near)]
    face = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    Bq = em * Bp1 + 6.0 * U * np.abs(em * p1) + 2.0 * U * np.abs(q1) \
        + cnt * U * (2.0 * face + np.abs(qpre))
    Bq[:, :, L - 1] += 3.0 * U * np.abs(q1[:, :, L - 1])
    p2 = p1r + he * ga
    Bp = Bp1 + he * Bga + 5.0 * U * np.abs(he * ga) + 2.0 * U * np.abs(p2)
    out = {"q": q1, "p": p2, "Bq": Bq, "Bp": Bp, "near": near.any(axis=3), "count": cnt.sum(axis=3)}
    mu0 = np.where(inside(state[:T], lo, hi), mub[:, :, 0], -np.inf)
    K0, KL = kinetic(p0, minv), kinetic(trace[:, :, L - 1, 1], minv)
    H0, HL = K0 - mu0, KL - mua[:, :, L - 1]
    with np.errstate(invalid="ignore"):
        dH = HL - H0
        out["BdH"] = Bmub[:, :, 0] + Bmua[:, :, L - 1] + 9.0 * U * (K0 + KL) + 32.0 * U * K0 \
            + U * (np.abs(H0) + np.abs(HL) + np.abs(dH))
        logu = np.log(ua)
        out["gated"] = np.isneginf(mu0)
        out["accept"] = ~out["gated"] & np.isfinite(dH) & (dH <= 1000.0) & (logu < -dH)
        out["margin"] = np.abs(logu + dH)
    out["dH"], out["logu"], out["eps"] = dH, logu, es
    out["mu_after"], out["Bmu_after"] = mua[:, :, L - 1], Bmua[:, :, L - 1]
    return out


# ---- the replay cases of tests/test_gpu_hmc.py (tests/test_hmc_ref.py runs the reference alone on the same inputs) ----
# (D, C, n, kernel, L, eps, G, jitter, box): box "wide" is the ensemble replay's, "tight" a small box around the bulk in
# which trajectories reflect, "inf" the wide one with its first lower and last upper edge infinite.
REPLAY_CASES = [
    (1, 5, 40, "se", 7, 0.15, 1, 0.0, "wide"),
    (2, 17, 90, "amp", 7, 0.1, 4, 0.3, "tight"),
    (2, 1, 90, "se", 1, 0.2, 1, 0.3, "inf"),
    (8, 5, 200, "selin1", 7, 0.08, 4, 0.0, "wide"),
    (8, 17, 200, "se", 7, 0.08, 1, 0.3, "tight"),
    (8, 5, 1536, "se", 7, 0.08, 1, 0.3, "wide"),
    (8, 5, 1536, "se", 1, 0.1, 4, 0.0, "tight"),
    (12, 5, 200, "amplin2", 7, 0.05, 1, 0.3, "inf"),
    (12, 17, 90, "se", 1, 0.05, 4, 0.0, "tight"),
    (32, 5, 200, "se", 7, 0.03, 4, 0.3, "wide"),
    (32, 17, 40, "selin1", 7, 0.03, 1, 0.0, "tight"),
    (32, 1, 200, "amp", 1, 0.05, 4, 0.0, "inf"),
]
REPLAY_ITERATIONS = 40
REPLAY_SEED = 20260


def case_id(c):
    return "D%d-C%d-n%d-%s-L%d-G%d-j%g-%s" % (c[0], c[1], c[2], c[3], c[4], c[6], c[7], c[8])


def case_box(D, box):
    import test_gpu_ensemble_replay as rp
    b = rp._bounds(D).astype(np.float64)
    if box == "tight":
        b = np.array([(-0.35 - 0.01 * d, 0.4 + 0.005 * d) for d in range(D)])
    elif box == "inf":
        b[0, 0], b[D - 1, 1] = -np.inf, np.inf
    return b


def case_start(C, D, b, seed):
    """Chains inside the box; with five or more, chain 0 starts outside it and chain 1 on a lower face."""
    rs = np.random.RandomState(seed)
    fin = np.where(np.isfinite(b), b, np.sign(b) * 2.0)
    mid, half = 0.5 * (fin[:, 0] + fin[:, 1]), 0.5 * (fin[:, 1] - fin[:, 0])
    p0 = mid + 0.8 * half * rs.uniform(-1, 1, size=(C, D))
    if C >= 5:
        p0[0, D - 1] = fin[D - 1, 0] - 0.5
        p0[1, D - 1] = b[D - 1, 0]
    return p0


_INPUTS = {}


def problem(D, n, kern):
    """The training set and kernels of test_gpu_ensemble_replay._problem (the same random stream, the same recipe), with
    the oracle GP factored and the package's GP only constructed: its kernel constants are host arithmetic, and a test
    on a GPU calls ``gp.compute(X)`` itself."""
    import george_oracle as go
    import test_gpu_ensemble_replay as rp
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(1000 + 37 * D + n)
    b = rp._bounds(D)
    X = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(size=(n, D))
    c = rs.uniform(-0.5, 0.5, D)
    y = -0.5 * np.sum((X - c) ** 2 / (0.3 + 0.1 * np.arange(D)), axis=1) + 0.2 * np.sin(2.0 * X[:, 0])
    metric = np.linspace(0.6, 1.6, D) * max(1.0, D / 2.0)

    def make(mod):
        k = mod.ExpSquaredKernel(metric, ndim=D)
        if kern.startswith("amp"):
            k = 2.5 * k
        if "lin" in kern:
            k = k + 0.3 * mod.kernels.LinearKernel(log_gamma2=0.4, order=int(kern[-1]), bounds=None, ndim=D)
        return mod.GP(kernel=k, fit_mean=True, mean=float(np.median(y)), white_noise=-4.0, fit_white_noise=False)
    gp, gpo = make(agp), make(go)
    gpo.compute(X)
    return X, y, gp, gpo


def case_inputs(c):
    """(X, y, gp, gpo, model, bounds, p0) of a replay case; built once per (D, n, kernel) and shared."""
    D, C, n, kern = c[:4]
    key = (D, n, kern)
    if key not in _INPUTS:
        X, y, gp, gpo = problem(D, n, kern)
        _INPUTS[key] = (X, y, gp, gpo, Model.from_gps(gp, gpo, y))
    X, y, gp, gpo, model = _INPUTS[key]
    b = case_box(D, c[8])
    return X, y, gp, gpo, model, b, case_start(C, D, b, REPLAY_SEED + C)
