"""NumPy restatement of the on-device nested sampler (csrc/nested.hip; the recipe is include/apgp.h's apgp_nested_sample)
and of its accounting (mcmc.nested_weights) -- the checker the device is held to, never the thing shipped.

Positions are kept in the caller's coordinates th; the target is evaluated at q = th * sc.  Run r draws from
Philox4x32-10 under ``ensemble_ref.stream_keys(seed, r)``:

* start    th[w, d] = min(lo + (hi - lo) u, hi), u = u01 of words (0, 1) for even d, (2, 3) for odd d, of counter (w, d // 2, 0, 11)
* batch b  order the live points by (logL, slot); the first ``batch`` die, L* = the last one's logL; the survivors in
           the same order are S = nlive - batch points, frozen for the batch; walker i refills the slot of dead point i
* walker   starts at survivor word 0 % S of counter (b, 0xffffffff, i, 12)
* step s   a = word 0 % S, k = word 1 % (S - 1), k += (k >= a) of counter (b, s, i, 13); n = sqrt(-2 log u) cospi(2 u'),
           (u, u') = u01 of words (0, 1), (2, 3) of counter (b, s, i, 14); gamma = gamma0 (1 + sigma n);
           q' = q + gamma (th_a sc - th_k sc); th' = q' / sc; q'' = th' sc; accepted iff th' is finite, inside
           [lo, hi] and mu(q'') > L*
* sums     per dead point i of a batch, n = nlive - i: logZ = logaddexp(logZ, logL + logX + log(1 - exp(-1 / n))),
           logX -= 1 / n
* stop     before batch b >= 1 if dlogz > 0 and logaddexp(logZ, Lmax + logX) - logZ < dlogz; at maxBatches.

A target is anything with ``mg(q)`` returning ``(mu, gradient)`` at scaled points (hmc_ref.Model, or the analytic
targets below): only mu is used.

Budgets of the replay (``forced``; u = 2^-53, first order, nothing fitted to a device's output):
  proposal  ca = th_a sc, cb = th_k sc: u |ca|, u |cb|; their difference u |ca - cb|; gamma: the Box-Muller normal within
            16 u |n| (hmc_ref's B_p0), sigma n and 1 + . and gamma0 . one rounding each: d gamma <= 16 u gamma0 sigma |n| +
            2 u |gamma|; the fma u |q'|; the division u |th'|.  The reference rounds the same operations: all doubled.
            B_th = 2 u [ |gamma| (|ca| + |cb| + |ca - cb|) + (16 gamma0 sigma |n| + 2 |gamma|) |ca - cb| + |q'| ] / sc + 2 u |th'|
  mean      hmc_ref.Model.mg's B_mu with G = 1 (one wavefront strides the rows): the budget of the existing mean tests.
A decision whose |mu(q'') - L*| <= B_mu is a NEAR-TIE and is not compared; the GPU test caps their share at 1 %."""
import numpy as np

from ensemble_moves_ref import cospi
from ensemble_ref import stream_keys
from philox_ref import philox4x32_10, u01

U = 2.0 ** -53
NEAR_CAP = 0.01
TAG_START, TAG_WALKER, TAG_PAIR, TAG_NORMAL = 11, 12, 13, 14


def default_gamma0(D):
    return 2.38 / np.sqrt(2.0 * D)


def start_points(seed, run, nlive, lo, hi):
    """The start of run ``run``: (nlive, D) in the caller's coordinates (the device fuses span * u + lo: 1 ulp)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    D = len(lo)
    k0, k1 = stream_keys(seed, run)
    w = np.arange(nlive, dtype=np.uint64)
    th = np.empty((nlive, D))
    for d in range(0, D, 2):
        c = philox4x32_10(w, d >> 1, 0, TAG_START, k0, k1)
        th[:, d] = np.minimum(lo[d] + (hi[d] - lo[d]) * u01(c[0], c[1]), hi[d])
        if d + 1 < D:
            th[:, d + 1] = np.minimum(lo[d + 1] + (hi[d + 1] - lo[d + 1]) * u01(c[2], c[3]), hi[d + 1])
    return th


def walker_starts(seed, run, b, batch, S):
    k0, k1 = stream_keys(seed, run)
    c = philox4x32_10(b, 0xFFFFFFFF, np.arange(batch, dtype=np.uint64), TAG_WALKER, k0, k1)
    return (c[0] % np.uint64(S)).astype(np.int64)


def step_draws(seed, run, b, batch, nsteps, S):
    """(a, k, n), each (batch, nsteps): the survivor pair and the unit normal of every step of batch ``b``."""
    k0, k1 = stream_keys(seed, run)
    i = np.arange(batch, dtype=np.uint64)[:, None]
    s = np.arange(nsteps, dtype=np.uint64)[None, :]
    c = philox4x32_10(b, s, i, TAG_PAIR, k0, k1)
    a = (c[0] % np.uint64(S)).astype(np.int64)
    k = (c[1] % np.uint64(S - 1)).astype(np.int64)
    k = k + (k >= a)
    c = philox4x32_10(b, s, i, TAG_NORMAL, k0, k1)
    n = np.sqrt(-2.0 * np.log(u01(c[0], c[1]))) * cospi(2.0 * u01(c[2], c[3]))
    return a, k, n


def order_of(logl):
    """Slots ascending by (logL, slot)."""
    return np.lexsort((np.arange(len(logl)), logl))


def logaddexp(a, b):
    m = max(a, b)
    if m == -np.inf:
        return m
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def run_sums(dead_logl, nlive, batch):
    """(logZ, logX) a run keeps over its dead points: dead point i of a batch has n = nlive - i.  (mcmc.nested_weights
    counts the same n from the births except at an exact tie that a batch boundary splits: a point born AT a threshold
    is not counted live at a later point of exactly that logL.)"""
    logZ, logX = -np.inf, 0.0
    for k, l in enumerate(np.asarray(dead_logl, dtype=np.float64)):
        inv = 1.0 / (nlive - k % batch)
        logZ = logaddexp(logZ, l + (logX + np.log(-np.expm1(-inv))))
        logX -= inv
    return logZ, logX


def propose(th, tha, thb, gam, sc):
    qv = th * sc + gam * (tha * sc - thb * sc)
    thp = qv / sc
    return thp, thp * sc


def inside(thp, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(thp) & (thp >= lo) & (thp <= hi), axis=-1)


def run_one(target, lo, hi, sc, nlive, batch, nsteps, maxBatches, dlogz, seed, run, sigma=1.0e-5, gamma0=None):
    """A free run.  Returns a dict: ``points``, ``logL``, ``birth``, ``rec`` (rows in the device's order: the dead of
    batch 0, 1, ..., then the final live points, rec -1), ``nbatch``, ``ncall``, ``naccept``, ``nstuck``, ``logZ`` and
    ``logX`` (over the dead points), ``margin`` (the smallest |mu - L*| of any decision)."""
    lo, hi, sc = (np.asarray(v, dtype=np.float64) for v in (lo, hi, sc))
    D = len(lo)
    g0 = default_gamma0(D) if not gamma0 else float(gamma0)
    th = start_points(seed, run, nlive, lo, hi)
    ll = np.asarray(target.mg(th * sc)[0], dtype=np.float64).copy()
    ll[np.isnan(ll)] = -np.inf
    birth = np.full(nlive, -np.inf)
    S = nlive - batch
    out = {k: [] for k in ("points", "logL", "birth", "rec")}
    logZ, logX, nb, ncall, nacc, nstuck, margin = -np.inf, 0.0, 0, nlive, 0, 0, np.inf
    while True:
        order = order_of(ll)
        if nb >= maxBatches:
            break
        if nb > 0 and dlogz > 0.0 and logaddexp(logZ, ll[order[-1]] + logX) - logZ < dlogz:
            break
        dead, surv = order[:batch], order[batch:]
        Lstar = ll[dead[-1]]
        out["points"].append(th[dead].copy()); out["logL"].append(ll[dead].copy())
        out["birth"].append(birth[dead].copy()); out["rec"].append(np.full(batch, nb))
        for i in range(batch):
            inv = 1.0 / (nlive - i)
            logZ = logaddexp(logZ, ll[dead[i]] + (logX + np.log(-np.expm1(-inv))))
            logX -= inv
        s0 = surv[walker_starts(seed, run, nb, batch, S)]
        ja, jk, nrm = step_draws(seed, run, nb, batch, nsteps, S)
        cur, curl, acc = th[s0].copy(), ll[s0].copy(), np.zeros(batch, dtype=np.int64)
        frozen = th.copy()
        for s in range(nsteps):
            gam = g0 * (1.0 + sigma * nrm[:, s])
            thp, qn = propose(cur, frozen[surv[ja[:, s]]], frozen[surv[jk[:, s]]], gam[:, None], sc)
            ok = inside(thp, lo, hi)
            if np.any(ok):
                mu = np.asarray(target.mg(qn[ok])[0], dtype=np.float64)
                ncall += int(ok.sum())
                margin = min(margin, float(np.min(np.abs(mu - Lstar))))
                take = np.zeros(batch, dtype=bool)
                take[ok] = mu > Lstar
                full = np.zeros(batch)
                full[ok] = mu
                cur[take], curl[take] = thp[take], full[take]
                acc += take
        th[dead], ll[dead], birth[dead] = cur, curl, Lstar
        nacc += int(acc.sum())
        nstuck += int(np.sum(acc == 0))
        nb += 1
    out = {k: np.concatenate(v + [w]) for (k, v), w in zip(out.items(), (th[order], ll[order], birth[order],
                                                                          np.full(nlive, -1)))}
    out.update(nbatch=nb, ncall=ncall, naccept=nacc, nstuck=nstuck, logZ=logZ, logX=logX, margin=margin)
    return out


def run(target, lo, hi, sc, nlive, batch, nsteps, maxBatches, dlogz, seed, nruns, sigma=1.0e-5, gamma0=None):
    """``nruns`` free runs, a list of ``run_one``'s dicts."""
    return [run_one(target, lo, hi, sc, nlive, batch, nsteps, maxBatches, dlogz, seed, r, sigma, gamma0) for r in range(nruns)]


def merged(runs):
    """(points, logL, birth, run) of several runs' dicts, concatenated: all that a merge is."""
    return (np.concatenate([r["points"] for r in runs]), np.concatenate([r["logL"] for r in runs]),
            np.concatenate([r["birth"] for r in runs]), np.concatenate([np.full(len(r["logL"]), k) for k, r in enumerate(runs)]))


def weights(logL, birth, run=None):
    """The accounting by its definition, point by point (mcmc.nested_weights vectorises it): returns ``order``,
    ``nlive``, ``logX``, ``logWt`` (in the sorted order), ``logZ``, ``H`` and ``logZErr = sqrt(sum dH_k / n_k)``."""
    logL, birth = np.asarray(logL, dtype=np.float64), np.asarray(birth, dtype=np.float64)
    M = len(logL)
    run = np.zeros(M, dtype=np.int64) if run is None else np.asarray(run)
    order = np.lexsort((np.arange(M), run, logL))
    n, lx, lw = np.empty(M), np.empty(M), np.empty(M)
    x = 0.0
    for k in range(M):
        n[k] = max(1, int(np.sum(birth[order[k:]] < logL[order[k]])))
        lw[k] = logL[order[k]] + x + np.log(-np.expm1(-1.0 / n[k]))
        x -= 1.0 / n[k]
        lx[k] = x
    logZ, H, var = -np.inf, 0.0, 0.0
    for k in range(M):
        new = logaddexp(logZ, lw[k])
        if new > -np.inf:
            # Skilling's update of the information
            Hn = np.exp(lw[k] - new) * logL[order[k]] + (np.exp(logZ - new) * (H + logZ) if logZ > -np.inf else 0.0) - new
            var += (Hn - H) / n[k]
            H = Hn
        logZ = new
    return {"order": order, "nlive": n, "logX": lx, "logWt": lw, "logZ": logZ, "H": H, "logZErr": np.sqrt(max(var, 0.0))}


# ---- analytic targets (scaled coordinates = the caller's: sc = 1) ----
class IsoGaussian(object):
    """L = exp(-|q - c|^2 / (2 s^2)); ``truth(lo, hi)`` is log int_box L / V by the closed form of erf terms."""

    def __init__(self, centre, s):
        self.c, self.s = np.asarray(centre, dtype=np.float64), float(s)
        self.D = len(self.c)

    def mg(self, q, G=1, budgets=False):
        r = np.asarray(q, dtype=np.float64).reshape(-1, self.D) - self.c
        return -0.5 * np.sum(r * r, axis=1) / self.s ** 2, -r / self.s ** 2

    def truth(self, lo, hi):
        from math import erf, sqrt, pi, log
        t = 0.0
        for d in range(self.D):
            a, b = (lo[d] - self.c[d]) / (self.s * sqrt(2.0)), (hi[d] - self.c[d]) / (self.s * sqrt(2.0))
            t += log(self.s * sqrt(pi / 2.0) * (erf(b) - erf(a)) / (hi[d] - lo[d]))
        return t


class TwoWell(object):
    """L = w0 N-shaped bump at c0 + w1 bump at c1 (isotropic, widths s0, s1): two separated modes of unequal mass."""

    def __init__(self, c0, c1, s0, s1, w1):
        self.a, self.b = IsoGaussian(c0, s0), IsoGaussian(c1, s1)
        self.lw1, self.D = float(np.log(w1)), len(c0)

    def mg(self, q, G=1, budgets=False):
        return np.logaddexp(self.a.mg(q)[0], self.b.mg(q)[0] + self.lw1), None

    def truth(self, lo, hi):
        return float(np.logaddexp(self.a.truth(lo, hi), self.b.truth(lo, hi) + self.lw1))

    def mass1(self, lo, hi):
        """The share of the evidence in the second well."""
        return float(np.exp(self.b.truth(lo, hi) + self.lw1 - self.truth(lo, hi)))


def exact_run(rs, D, s, R, nlive, batch, nbatches):
    """Exact nested sampling of IsoGaussian(0, s) in the box [-R, R]^D with s << R, so that every threshold after the
    first few lies inside the box: a constrained draw is uniform in the ball |q| < r*.  Returns (logL, birth) in the
    device's row order.  No MCMC: this tests the accounting alone.  (While the ball still sticks out of the box the
    draw is by rejection from the box.)"""
    def draw(rmax, m):
        out = np.empty((0, D))
        while len(out) < m:
            if rmax >= R:
                c = rs.uniform(-R, R, size=(4 * m + 16, D))
                c = c[np.sum(c * c, axis=1) < rmax * rmax]
            else:
                g = rs.normal(size=(m, D))
                c = g / np.linalg.norm(g, axis=1)[:, None] * (rmax * rs.uniform(size=(m, 1)) ** (1.0 / D))
            out = np.concatenate([out, c])
        return out[:m]
    r2 = np.sum(rs.uniform(-R, R, size=(nlive, D)) ** 2, axis=1)
    ll, birth = -0.5 * r2 / s ** 2, np.full(nlive, -np.inf)
    L, Bt = [], []
    for b in range(nbatches):
        order = order_of(ll)
        dead = order[:batch]
        Lstar = ll[dead[-1]]
        L.append(ll[dead].copy()); Bt.append(birth[dead].copy())
        new = draw(np.sqrt(-2.0 * Lstar) * s, batch)
        ll[dead], birth[dead] = -0.5 * np.sum(new * new, axis=1) / s ** 2, Lstar
    order = order_of(ll)
    return np.concatenate(L + [ll[order]]), np.concatenate(Bt + [birth[order]])


def forced(model, lo, hi, sc, nlive, batch, nsteps, seed, run, points, logL, birth, rec, nbatch, trace, sigma=1.0e-5,
           gamma0=None):
    """Teacher-forced replay of one device run, batch by batch.  ``points``, ``logL``, ``birth``, ``rec`` are the run's
    rows, ``trace`` (maxBatches, batch, nsteps, D + 2) its steps.  The live set is tracked in the device's own numbers:
    a walker's end point is its last accepted proposal of the trace (or its start survivor).  Returns a dict of
    checks: ``start_err`` (max |start - reference| in ulps of the span), ``dead_ok`` (every batch's dead rows are
    exactly the lowest (logL, slot) of the tracked live set, in order, with their births), ``final_ok``, ``prop_err``
    (max |th' - reference| / B_th), ``box_ok`` (every evaluated / not-evaluated flag is the reference's), ``mu_err``
    (max |mu - reference| / B_mu), ``ndecisions``, ``nnear``, ``nwrong`` (decisions outside the near-tie band that
    differ), ``stuck``, ``naccept``, ``ncall``."""
    lo, hi, sc = (np.asarray(v, dtype=np.float64) for v in (lo, hi, sc))
    D = len(lo)
    g0 = default_gamma0(D) if not gamma0 else float(gamma0)
    S = nlive - batch
    ref0 = start_points(seed, run, nlive, lo, hi)
    first = np.where(np.isneginf(birth))[0]
    out = {"dead_ok": True, "final_ok": True, "box_ok": True, "prop_err": 0.0, "mu_err": 0.0, "ndecisions": 0, "nnear": 0,
           "nwrong": 0, "stuck": 0, "naccept": 0, "ncall": nlive}
    # the start points carry birth -inf; slot w is the row nearest to the reference's start point w
    th = np.empty((nlive, D)); ll = np.empty(nlive)
    assert len(first) == nlive
    used = np.zeros(len(first), dtype=bool)
    err = 0.0
    for w in range(nlive):
        d = np.max(np.abs(points[first] - ref0[w]) / (hi - lo), axis=1)
        d[used] = np.inf
        j = int(np.argmin(d))
        used[j] = True
        err = max(err, d[j])
        th[w], ll[w] = points[first[j]], logL[first[j]]
    out["start_err"] = err / U
    out["start_th"], out["start_logL"] = th.copy(), ll.copy()
    bt = np.full(nlive, -np.inf)
    for b in range(nbatch):
        order = order_of(ll)
        dead, surv = order[:batch], order[batch:]
        rows = slice(b * batch, (b + 1) * batch)
        if not (np.array_equal(points[rows], th[dead]) and np.array_equal(logL[rows], ll[dead])
                and np.array_equal(birth[rows], bt[dead]) and np.all(rec[rows] == b)):
            out["dead_ok"] = False
            return out
        Lstar = ll[dead[-1]]
        s0 = surv[walker_starts(seed, run, b, batch, S)]
        ja, jk, nrm = step_draws(seed, run, b, batch, nsteps, S)
        cur, curl, acc = th[s0].copy(), ll[s0].copy(), np.zeros(batch, dtype=np.int64)
        for s in range(nsteps):
            gam = (g0 * (1.0 + sigma * nrm[:, s]))[:, None]
            tha, thb = th[surv[ja[:, s]]], th[surv[jk[:, s]]]
            thp, _ = propose(cur, tha, thb, gam, sc)
            ca, cb = np.abs(tha * sc), np.abs(thb * sc)
            df = np.abs(tha * sc - thb * sc)
            Bth = 2.0 * U * (np.abs(gam) * (ca + cb + df) + (16.0 * g0 * sigma * np.abs(nrm[:, s])[:, None] + 2.0 * np.abs(gam)) * df
                             + np.abs(thp * sc)) / sc + 2.0 * U * np.abs(thp)
            dev = trace[b, :, s, :D]
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.where(Bth > 0.0, np.abs(dev - thp) / Bth, np.where(dev == thp, 0.0, np.inf))
            out["prop_err"] = max(out["prop_err"], float(np.max(r)))
            ok = inside(dev, lo, hi)                                      # the device's own th': the same comparison
            if not np.array_equal(ok, ~np.isnan(trace[b, :, s, D])):
                out["box_ok"] = False
            take = trace[b, :, s, D + 1] == 1.0
            if np.any(take & ~ok):
                out["box_ok"] = False
            if np.any(ok):
                mu, _, Bmu, _ = model.mg(dev[ok] * sc, 1, True)
                dmu = trace[b, ok, s, D]
                out["mu_err"] = max(out["mu_err"], float(np.max(np.abs(dmu - mu) / Bmu)))
                near = np.abs(mu - Lstar) <= Bmu
                out["ndecisions"] += int(ok.sum())
                out["nnear"] += int(near.sum())
                out["nwrong"] += int(np.sum(~near & ((mu > Lstar) != take[ok])))
                out["ncall"] += int(ok.sum())
            cur[take], curl[take] = dev[take], trace[b, take, s, D]
            acc += take
        th[dead], ll[dead], bt[dead] = cur, curl, Lstar
        out["naccept"] += int(acc.sum())
        out["stuck"] += int(np.sum(acc == 0))
    order = order_of(ll)
    rows = slice(nbatch * batch, nbatch * batch + nlive)
    out["final_ok"] = bool(np.array_equal(points[rows], th[order]) and np.array_equal(logL[rows], ll[order])
                           and np.array_equal(birth[rows], bt[order]) and np.all(rec[rows] == -1))
    return out
