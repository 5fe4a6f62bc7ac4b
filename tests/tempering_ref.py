"""NumPy restatement of the tempered ensemble sampler (csrc/tempering.hip: tempered_kernel, include/apgp.h:
apgp_tempered_sample) -- the checker the device is held to, never the thing shipped.  It is built on
ensemble_moves_ref.py (the moves, their draws and the box gate) and philox_ref.py.

The recipe.  A ladder is T ensembles ("rungs"); rung k of ladder l is ensemble e = l T + k of ensemble_moves_ref: keys
``stream_keys(seed, e)``, counters with the global iteration number, the same proposals.  Rung k keeps mu per walker and
accepts on the tempered value t(mu) = beta_k mu, -inf wherever mu is not finite (at every beta, 0 included):
accept iff the proposal is finite and inside the box and log u_acc < factor + t(mu(q)) - t(mu(s)).
After every ``swap_every`` iterations except the last comes exchange round r = 0, 1, ...: it pairs rungs (k, k + 1) with
k = r (mod 2); walker i of rung k and walker i of rung k + 1 trade places (coordinates and mu) iff both mu are finite and
log u < (beta_k - beta_{k+1}) (mu_{k+1,i} - mu_{k,i}), u = u01(words 0, 1) of Philox counter (r, r >> 32, i, 7) under the
keys of ensemble l T + k.  Logged per (round, ladder, pair, walker): 0 = not proposed (inactive pair or a mu that is not
finite), 1 = rejected, 2 = accepted.  Accept counters stay with the rung."""
import numpy as np

import ensemble_moves_ref as emr
from ensemble_ref import _box, _face, _inside, _lp, halves, stream_keys
from philox_ref import philox4x32_10, u01

_MASK = np.uint64(0xFFFFFFFF)


def temper(beta, mu):
    """beta mu, -inf wherever mu is not finite."""
    mu = np.asarray(mu, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(mu), beta * np.where(np.isfinite(mu), mu, 0.0), -np.inf)


def as4(p0, L, T):
    p0 = np.asarray(p0, dtype=np.float64)
    return np.array(np.broadcast_to(p0, (L, T) + p0.shape[-2:]))


def rounds_of(iterations, swap_every):
    return max(0, -(-int(iterations) // int(swap_every)) - 1)


def exchange_uniforms(seed, L, T, r, W):
    """u of exchange round r per (ladder, pair, walker): (L, T - 1, W)."""
    out = np.empty((L, max(T - 1, 0), W))
    for l in range(L):
        for k in range(T - 1):
            k0, k1 = stream_keys(seed, l * T + k)
            c = philox4x32_10(int(r) & 0xFFFFFFFF, int(r) >> 32, np.arange(W, dtype=np.uint64), 7, k0, k1)
            out[l, k] = u01(c[0], c[1])
    return out


def exchange(mu, betas, u, r):
    """Decisions of round r from mu (L, T, W) and the uniforms u (L, T - 1, W): (log, margin), each (L, T - 1, W); the
    margin |log u - rhs| is inf where nothing was proposed."""
    L, T, W = mu.shape
    log = np.zeros((L, max(T - 1, 0), W), dtype=np.uint8)
    margin = np.full(log.shape, np.inf)
    for k in range(int(r) % 2, T - 1, 2):
        lo_, hi_ = mu[:, k], mu[:, k + 1]
        both = np.isfinite(lo_) & np.isfinite(hi_)
        with np.errstate(invalid="ignore"):
            rhs = (betas[k] - betas[k + 1]) * (hi_ - lo_)
            logu = np.log(u[:, k])
            acc = both & (logu < rhs)
            margin[:, k] = np.where(both, np.abs(logu - rhs), np.inf)
        log[:, k] = np.where(both, np.where(acc, 2, 1), 0)
    return log, margin


def apply_exchange(log, arrays):
    """Swap rows [l, k, i] and [l, k + 1, i] of every array in ``arrays`` ((L, T, W, ...)) where log[l, k, i] == 2."""
    for l, k, i in np.argwhere(log == 2):
        for a in arrays:
            a[l, k, i], a[l, k + 1, i] = a[l, k + 1, i].copy(), a[l, k, i].copy()


def run(lp_fn, p0, iterations, bounds, tab, betas, swap_every, seed=0, sc=None, ladders=1):
    """Free-running ladders from ``p0`` ((W, D), (T, W, D) or (L, T, W, D)).  Returns ``chain`` (N, L, T, W, D),
    ``log_prob`` (N, L, T, W: mu), ``naccept`` (L, T, W), ``coords``, ``final_log_prob``, ``swap_log`` (rounds, L, T - 1,
    W), ``swap_prop`` / ``swap_acc`` (L, T - 1), ``move`` (L T, N) and under ``decisions`` the moves' ``margin`` and
    ``face`` (L T, N, 2, H) and the exchanges' ``swap_margin`` (rounds, L, T - 1, W)."""
    betas = np.asarray(betas, dtype=np.float64)
    L, T, N, se = int(ladders), len(betas), int(iterations), int(swap_every)
    p0 = as4(p0, L, T)
    W, D = p0.shape[-2:]
    H = W // 2
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    R = rounds_of(N, se)
    chain, logp = np.empty((N, L, T, W, D)), np.empty((N, L, T, W))
    nacc = np.zeros((L, T, W), dtype=np.int64)
    margin, face = np.full((L * T, N, 2, H), np.inf), np.full((L * T, N, 2, H), np.inf)
    swap_log = np.zeros((R, L, max(T - 1, 0), W), dtype=np.uint8)
    swap_margin = np.full(swap_log.shape, np.inf)
    moves = np.zeros((L * T, N), dtype=np.int64)
    cs = p0 * sc
    mu = np.empty((L, T, W))
    dr, kinds, idx, parts = {}, {}, {}, {}
    for l in range(L):
        for k in range(T):
            e = l * T + k
            k0, k1 = stream_keys(seed, e)
            dr[e] = emr.draws(np.arange(N), W, k0, k1, tab)
            moves[e] = dr[e]["move"]
            kinds[e] = emr._per_iteration(tab, dr[e]["move"])
            idx[e] = halves(dr[e]["rot"], W)
            parts[e] = emr._partners(dr[e], kinds[e][0])
            mu[l, k] = _lp(lp_fn, cs[l, k] / sc, _inside(cs[l, k], lo_sc, hi_sc))
    for it in range(N):
        if it > 0 and it % se == 0:
            r = it // se - 1
            swap_log[r], swap_margin[r] = exchange(mu, betas, exchange_uniforms(seed, L, T, r, W), r)
            apply_exchange(swap_log[r], (cs, mu))
        one = slice(it, it + 1)
        for l in range(L):
            for k in range(T):
                e = l * T + k
                d, (kind, par), (sidx, cidx), (js, ks, ls) = dr[e], kinds[e], idx[e], parts[e]
                c_, m_ = cs[l, k], mu[l, k]
                for split in range(2):
                    s, c = sidx[it, split], cidx[it, split]
                    q, fac, _ = emr._propose(tab, kind[one], (par[0][one], par[1][one]), c_[s][None],
                                             c_[c[js[it, split]]][None], c_[c[ks[it, split]]][None],
                                             c_[c[ls[it, split]]][None], d["u"][one, split], d["de_n"][one, split], D)
                    q, fac = q[0], fac[0]
                    ok = emr._ok(q, lo_sc, hi_sc)
                    lpq = _lp(lp_fn, q / sc, ok)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ltq = temper(betas[k], lpq)
                        diff = fac + ltq - temper(betas[k], m_[s])
                        logu = np.log(d["uacc"][it, split])
                        acc = ok & ~np.isnan(ltq) & (logu < diff)
                        margin[e, it, split] = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
                        face[e, it, split] = np.where(np.all(np.isfinite(q), axis=-1), _face(q / sc, lo, hi), np.inf)
                    c_[s[acc]] = q[acc]
                    m_[s[acc]] = lpq[acc]
                    nacc[l, k, s[acc]] += 1
        chain[it] = cs / sc
        logp[it] = mu
    return {"chain": chain, "log_prob": logp, "naccept": nacc, "coords": cs / sc, "final_log_prob": mu.copy(),
            "swap_log": swap_log, "swap_prop": (swap_log >= 1).sum(axis=(0, 3)), "swap_acc": (swap_log == 2).sum(axis=(0, 3)),
            "move": moves, "decisions": {"margin": margin, "face": face, "swap_margin": swap_margin}}


def forced(lp_fn, p0, chain, swap_log, bounds, tab, betas, swap_every, seed=0, sc=None):
    """Teacher-forced replay of a stored all-rung chain ``chain`` (N, L, T, W, D) that started from ``p0``: every half-step
    and every exchange is replayed from the state the chain itself records, with the DEVICE'S RECORDED exchange
    (``swap_log``, (rounds, L, T - 1, W)) applied at each boundary, so one near-tie cannot cascade.  The state before
    iteration it is chain[it - 1] (``p0`` at it = 0), after the recorded exchange where it opens a segment.
    Returns ``moves``: arrays over (L T, N, 2, H) -- ``walker`` (index in the rung), ``accept``, ``margin``, ``face``,
    ``q`` (.., D), ``lpq`` (mu of the proposal), ``before`` (.., D), ``kind`` -- and ``prev`` (N, L, T, W, D), the state
    before each iteration; and ``swaps``: ``log`` (the reference's decision from the reference's mu at the stored
    positions, 0 / 1 / 2) and ``margin``, each (rounds, L, T - 1, W)."""
    betas = np.asarray(betas, dtype=np.float64)
    chain = np.asarray(chain, dtype=np.float64)
    N, L, T, W, D = chain.shape
    H, se = W // 2, int(swap_every)
    p0 = as4(p0, L, T)
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    R = rounds_of(N, se)
    swap_log = np.asarray(swap_log).reshape(R, L, max(T - 1, 0), W)
    mu_rows = _lp(lp_fn, chain, _inside(chain * sc, lo_sc, hi_sc))                       # (N, L, T, W)
    mu_p0 = _lp(lp_fn, p0, _inside(p0 * sc, lo_sc, hi_sc))
    prev = np.concatenate([p0[None], chain[:-1]], axis=0)
    mu_prev = np.concatenate([mu_p0[None], mu_rows[:-1]], axis=0)
    ref_log = np.zeros(swap_log.shape, dtype=np.uint8)
    ref_margin = np.full(swap_log.shape, np.inf)
    for r in range(R):
        it = (r + 1) * se
        ref_log[r], ref_margin[r] = exchange(mu_prev[it], betas, exchange_uniforms(seed, L, T, r, W), r)
        apply_exchange(swap_log[r], (prev[it], mu_prev[it]))
    keys = ("walker", "accept", "margin", "face", "q", "lpq", "before", "kind")
    out = {k: [] for k in keys}
    tt = np.arange(N)[:, None]
    t3, sp3 = np.arange(N)[:, None, None], np.arange(2)[None, :, None]
    for l in range(L):
        for k in range(T):
            e = l * T + k
            k0, k1 = stream_keys(seed, e)
            dr = emr.draws(np.arange(N), W, k0, k1, tab)
            kind, par = emr._per_iteration(tab, dr["move"])
            sidx, cidx = halves(dr["rot"], W)
            st = np.stack([prev[:, l, k], prev[:, l, k]], axis=1)                       # (N, 2, W, D)
            lst = np.stack([mu_prev[:, l, k], mu_prev[:, l, k]], axis=1)
            s0 = sidx[:, 0]
            st[tt, 1, s0] = chain[tt, l, k, s0]
            lst[tt, 1, s0] = mu_rows[tt, l, k, s0]
            js, ks, ls = emr._partners(dr, kind)
            pick = lambda slots: st[t3, sp3, np.take_along_axis(cidx, slots, axis=2)]
            xs, xj, xk, xl = st[t3, sp3, sidx], pick(js), pick(ks), pick(ls)
            q, fac, _ = emr._propose(tab, kind, par, xs * sc, xj * sc, xk * sc, xl * sc, dr["u"], dr["de_n"], D)
            ok = emr._ok(q, lo_sc, hi_sc)
            with np.errstate(invalid="ignore", divide="ignore"):
                lpq = _lp(lp_fn, q / sc, ok)
                ltq = temper(betas[k], lpq)
                diff = fac + ltq - temper(betas[k], lst[t3, sp3, sidx])
                logu = np.log(dr["uacc"])
                acc = ok & ~np.isnan(ltq) & (logu < diff)
                margin = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
                fc = np.where(np.all(np.isfinite(q), axis=-1), _face(q / sc, lo, hi), np.inf)
            k3 = kind[:, None, None] + np.zeros((N, 2, H), dtype=np.int64)
            for name, v in (("walker", sidx), ("accept", acc), ("margin", margin), ("face", fc), ("q", q / sc),
                            ("lpq", lpq), ("before", xs), ("kind", k3)):
                out[name].append(v)
    return {"moves": {k: np.stack(v) for k, v in out.items()}, "prev": prev, "mu_prev": mu_prev,
            "swaps": {"log": ref_log, "margin": ref_margin}}
