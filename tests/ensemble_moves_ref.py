"""NumPy restatement of the on-device ensemble sampler's moves (csrc/ens_moves.h: ens_pick_move and ens_propose, called by
both ensemble kernels) -- the checker the device is held to, never the thing shipped.  ensemble_ref.py is the stretch-only
restatement; this file adds differential evolution, the snooker update and weighted mixtures, and shares its key schedule,
partition, box gate and stretch arithmetic.  It states what the kernel implements, not emcee's moves.

The recipe (H = W / 2, D = ndim; all 32-bit words come from Philox4x32-10 with the keys of ``ensemble_ref.stream_keys``):

* per iteration ``it``: counter (it, it >> 32, 0xffffffff, 5) gives four words.  Word 0 % W is the partition offset, as in
  ensemble_ref.  With ONE move in the table that move is taken and no other word is read.  With more, u = u01(word 1,
  word 2) picks the move for the whole iteration (both half-steps): cum[m] = (w_0 + ... + w_m) / (w_0 + ... + w_last), the
  sums accumulated left to right in float64; the move is the first m < last with u < cum[m], else the last.
* per slot t of half-step ``split``: counter (it, it >> 32, split * 256 + t, tag).
    tag 1  stretch: u = u01(words 0, 1), partner slot word 2 % H              (ensemble_ref, unchanged)
    tag 2  the acceptance uniform u01(words 0, 1), every move                 (ensemble_ref, unchanged)
    tag 3  DE partners: j = word 0 % H, k = word 1 % (H - 1), k += 1 if k >= j        (ordered pair, j != k)
    tag 4  DE normal: n = sqrt(-2 log u01(words 0, 1)) * cospi(2 * u01(words 2, 3))   (Box-Muller; cospi(x) = cos(pi x)
           with the argument reduced exactly, see ``cospi``)
    tag 6  snooker partners: j, k as under tag 3 from words 0, 1; l = word 2 % (H - 2), l += 1 if l >= min(j, k),
           then l += 1 if l >= max(j, k)                                       (ordered triple, all distinct)
  A stretch iteration of a mixture therefore draws exactly what the stretch-only chain draws in that iteration.
* the moves, on the scaled positions x * sc at the start of the half-step (s: the walker, c_i: complement slot i):
    stretch(a):       z = (a - 1) u + 1, zz = z z / a, q = c_j - (c_j - s) zz, factor (D - 1) log zz
    DE(sigma, g0):    gamma = g0 (1 + sigma n), q = s + gamma (c_j - c_k), factor 0;  g0 defaults to 2.38 / sqrt(2 D)
    snooker(gammas):  v = s - c_j, n2 = sum v_d^2, dot = sum v_d (c_k - c_l)_d  (d ascending), coef = gammas * dot / n2,
                      q = s + coef v, nq2 = sum (q - c_j)_d^2, factor (0.5 * (D - 1)) * log(nq2 / n2)
                      -- ter Braak & Vrugt's q = s + gammas (e . (z1 - z2)) e, e = v / |v|, z = c_j, z1 = c_k, z2 = c_l,
                      factor (D - 1) (log|q - z| - log|s - z|).  s = c_j gives 0 / 0: q is NaN.
* accept iff q is finite and inside the box in every dimension, lp(q) is not NaN and log u_acc < factor + lp(q) - lp(s).

A move table is a list of records ``(kind, weight, p0, p1)`` as ``apgp_ens_move_t``: (STRETCH, w, a, 0), (DE, w, sigma,
g0), (SNOOKER, w, gammas, 0); ``table`` builds one from ("stretch", a) / ("de", sigma, gamma0 or None) / ("snooker",
gammas) entries, each optionally wrapped as (entry, weight).  The device fuses q = s + gamma (c_j - c_k) and the snooker's
sums into multiply-adds; this file does not."""
import numpy as np

from ensemble_ref import ENS_MAXW, _as3, _box, _face, _inside, _lp, _move as _stretch, halves, stream_keys
from philox_ref import philox4x32_10, u01

STRETCH, DE, SNOOKER = 0, 1, 2
MAX_MOVES = 8
_MASK = np.uint64(0xFFFFFFFF)
_KINDS = {"stretch": STRETCH, "de": DE, "snooker": SNOOKER}


def table(moves, D):
    """Records (kind, weight, p0, p1) from entries ("stretch", a), ("de", sigma, gamma0 | None), ("snooker", gammas) or
    (entry, weight) pairs; equal weights where none are given."""
    if isinstance(moves[0], str):
        moves = [moves]
    out = []
    for m in moves:
        m, w = (m[0], float(m[1])) if not isinstance(m[0], str) else (m, 1.0)
        kind = _KINDS[m[0]]
        if kind == DE:
            g0 = m[2] if len(m) > 2 and m[2] is not None else 2.38 / np.sqrt(2.0 * D)
            out.append((DE, w, float(m[1]), float(g0)))
        else:
            out.append((kind, w, float(m[1]), 0.0))
    assert 1 <= len(out) <= MAX_MOVES
    return out


def cum_weights(tab):
    total = 0.0
    for r in tab:
        total = total + r[1]
    acc, cum = 0.0, []
    for r in tab:
        acc = acc + r[1]
        cum.append(acc / total)
    return np.array(cum)


def cospi(x):
    """cos(pi x) for x in [0, 2] with every reduction step exact: x -> 2 - x above 1, x -> 1 - x (sign flipped) above
    1/2, then cos(pi x) on [0, 1/4] and sin(pi (1/2 - x)) on (1/4, 1/2].  The one rounding of pi x there moves the result
    by at most an ulp or two (|x cot x|, |x tan x| <= 1 on [0, pi / 4]), so this agrees with a correctly reduced device
    cospi to a few ulps of the RESULT even next to a zero of the cosine, which cos(fl(2 pi u)) would not."""
    x = np.asarray(x, dtype=np.float64)
    r = np.where(x > 1.0, 2.0 - x, x)
    sign = np.where(r > 0.5, -1.0, 1.0)
    r = np.where(r > 0.5, 1.0 - r, r)
    return sign * np.where(r > 0.25, np.sin(np.pi * (0.5 - r)), np.cos(np.pi * r))


def draws(its, W, k0, k1, tab):
    """Random numbers of iterations ``its`` for the table ``tab``: ``rot`` and ``move`` (T,), and per (iteration, split,
    slot), each (T, 2, H): ``u`` and ``jslot`` (stretch), ``uacc``, ``de_j``, ``de_k``, ``de_n``, ``sn_j``, ``sn_k``,
    ``sn_l`` (zeros where H is too small for the move to exist)."""
    its = np.asarray(its, dtype=np.uint64).reshape(-1)
    T, H = len(its), W // 2
    cr = philox4x32_10(its & _MASK, its >> np.uint64(32), 0xFFFFFFFF, 5, k0, k1)
    out = {"rot": (cr[0] % np.uint64(W)).astype(np.int64)}
    if len(tab) == 1:
        out["move"] = np.zeros(T, dtype=np.int64)
    else:
        um, cum = u01(cr[1], cr[2]), cum_weights(tab)
        out["move"] = np.sum(~(um[:, None] < cum[None, :-1]), axis=1).astype(np.int64)      # (cum is non-decreasing)
    it3 = its[:, None, None]
    ctr = np.uint64(ENS_MAXW) * np.arange(2, dtype=np.uint64)[None, :, None] + np.arange(H, dtype=np.uint64)[None, None, :]
    ph = lambda tag: philox4x32_10(it3 & _MASK, it3 >> np.uint64(32), ctr, tag, k0, k1)
    c1, c2 = ph(1), ph(2)
    out["u"], out["jslot"], out["uacc"] = u01(c1[0], c1[1]), (c1[2] % np.uint64(H)).astype(np.int64), u01(c2[0], c2[1])
    zero = np.zeros((T, 2, H), dtype=np.int64)

    def pair(c):
        j = (c[0] % np.uint64(H)).astype(np.int64)
        k = (c[1] % np.uint64(H - 1)).astype(np.int64)
        return j, k + (k >= j)
    if H >= 2:
        c3, c4 = ph(3), ph(4)
        out["de_j"], out["de_k"] = pair(c3)
        out["de_n"] = np.sqrt(-2.0 * np.log(u01(c4[0], c4[1]))) * cospi(2.0 * u01(c4[2], c4[3]))
    else:
        out["de_j"], out["de_k"], out["de_n"] = zero, zero, np.zeros((T, 2, H))
    if H >= 3:
        c6 = ph(6)
        j, k = pair(c6)
        l = (c6[2] % np.uint64(H - 2)).astype(np.int64)
        l = l + (l >= np.minimum(j, k))
        l = l + (l >= np.maximum(j, k))
        out["sn_j"], out["sn_k"], out["sn_l"] = j, k, l
    else:
        out["sn_j"], out["sn_k"], out["sn_l"] = zero, zero, zero
    return out


def _de(cs_s, cs_j, cs_k, n, sigma, g0):
    gamma = g0 * (1.0 + sigma * n)
    return cs_s + gamma[..., None] * (cs_j - cs_k), np.zeros(np.shape(n)), gamma


def _snooker(cs_s, cs_j, cs_k, cs_l, gammas, D):
    v, dz = cs_s - cs_j, cs_k - cs_l
    n2, dot = np.zeros(v.shape[:-1]), np.zeros(v.shape[:-1])
    for d in range(v.shape[-1]):
        n2 = n2 + v[..., d] * v[..., d]
        dot = dot + v[..., d] * dz[..., d]
    with np.errstate(all="ignore"):
        coef = gammas * dot / n2
        q = cs_s + coef[..., None] * v
        r = q - cs_j
        nq2 = np.zeros(v.shape[:-1])
        for d in range(v.shape[-1]):
            nq2 = nq2 + r[..., d] * r[..., d]
        fac = (0.5 * (D - 1.0)) * np.log(nq2 / n2)
    return q, fac, coef


def _partners(dr, kind):
    """Complement slots (j, k, l) of every (iteration, split, slot) for the iteration's move kind (T,)."""
    kd = kind[:, None, None]
    j = np.where(kd == STRETCH, dr["jslot"], np.where(kd == DE, dr["de_j"], dr["sn_j"]))
    k = np.where(kd == DE, dr["de_k"], dr["sn_k"])
    return j, k, dr["sn_l"]


def _propose(tab, kind, par, cs_s, cs_j, cs_k, cs_l, u, n, D):
    """Proposals (..., D), log factors and the scalar multiplying the partner difference (zz | gamma | coef) for arrays of
    slots whose leading axis runs over iterations with move kinds ``kind`` and parameters ``par`` = (p0, p1) per
    iteration."""
    p0 = par[0].reshape((-1,) + (1,) * (u.ndim - 1))
    p1 = par[1].reshape(p0.shape)
    kd = kind.reshape(p0.shape)
    with np.errstate(all="ignore"):
        a = np.where(kd == STRETCH, p0, 2.0)
        z = (a - 1.0) * u + 1.0
        zz = z * z / a
        qs_, fs_ = _stretch(cs_j, cs_s, u, a, D)
        qd, fd, gam = _de(cs_s, cs_j, cs_k, n, p0 + 0.0 * u, p1 + 0.0 * u)
        qn, fn, coef = _snooker(cs_s, cs_j, cs_k, cs_l, p0 + 0.0 * u, D)
    k3 = kd + 0 * np.zeros(u.shape, dtype=np.int64)
    q = np.where((k3 == STRETCH)[..., None], qs_, np.where((k3 == DE)[..., None], qd, qn))
    fac = np.where(k3 == STRETCH, fs_, np.where(k3 == DE, fd, fn))
    mult = np.where(k3 == STRETCH, zz, np.where(k3 == DE, gam, coef))
    return q, fac, mult


def _ok(q, lo_sc, hi_sc):
    with np.errstate(invalid="ignore"):
        return _inside(q, lo_sc, hi_sc) & np.all(np.isfinite(q), axis=-1)


def _per_iteration(tab, move):
    kind = np.array([tab[m][0] for m in move], dtype=np.int64)
    par = (np.array([tab[m][2] for m in move]), np.array([tab[m][3] for m in move]))
    return kind, par


def run(lp_fn, p0, iterations, bounds, tab, seed=0, sc=None):
    """Free-running chain from ``p0`` ((W, D) or (E, W, D)) under the move table ``tab``; the result of
    ``ensemble_ref.run`` plus ``move`` (E, T), the table index each iteration took."""
    p0 = _as3(p0)
    E, W, D = p0.shape
    H = W // 2
    T = int(iterations)
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    chain, logp = np.empty((T, E, W, D)), np.empty((T, E, W))
    nacc = np.zeros((E, W), dtype=np.int64)
    coords, final = np.empty((E, W, D)), np.empty((E, W))
    margin, face = np.full((E, T, 2, H), np.inf), np.full((E, T, 2, H), np.inf)
    moves = np.zeros((E, T), dtype=np.int64)
    for e in range(E):
        k0, k1 = stream_keys(seed, e)
        dr = draws(np.arange(T), W, k0, k1, tab)
        moves[e] = dr["move"]
        kind, par = _per_iteration(tab, dr["move"])
        sidx, cidx = halves(dr["rot"], W)
        js, ks, ls = _partners(dr, kind)
        cs = p0[e] * sc
        lp = _lp(lp_fn, cs / sc, _inside(cs, lo_sc, hi_sc))
        for it in range(T):
            one = slice(it, it + 1)
            for split in range(2):
                s, c = sidx[it, split], cidx[it, split]
                q, fac, _ = _propose(tab, kind[one], (par[0][one], par[1][one]), cs[s][None], cs[c[js[it, split]]][None],
                                     cs[c[ks[it, split]]][None], cs[c[ls[it, split]]][None], dr["u"][one, split],
                                     dr["de_n"][one, split], D)
                q, fac = q[0], fac[0]
                ok = _ok(q, lo_sc, hi_sc)
                lpq = _lp(lp_fn, q / sc, ok)
                with np.errstate(invalid="ignore", divide="ignore"):
                    diff = fac + lpq - lp[s]
                    logu = np.log(dr["uacc"][it, split])
                    acc = ok & ~np.isnan(lpq) & (logu < diff)
                    margin[e, it, split] = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
                    face[e, it, split] = np.where(np.all(np.isfinite(q), axis=-1), _face(q / sc, lo, hi), np.inf)
                cs[s[acc]] = q[acc]
                lp[s[acc]] = lpq[acc]
                nacc[e, s[acc]] += 1
            chain[it, e] = cs / sc
            logp[it, e] = lp
        coords[e] = cs / sc
        final[e] = lp
    return {"chain": chain.reshape(T, E * W, D), "log_prob": logp.reshape(T, E * W), "naccept": nacc.reshape(E * W),
            "coords": coords.reshape(E * W, D), "final_log_prob": final.reshape(E * W), "move": moves,
            "decisions": {"margin": margin, "face": face}}


def forced(lp_fn, p0, chain, bounds, tab, seed=0, sc=None):
    """Teacher-forced replay of a stored chain under the move table ``tab``, as ``ensemble_ref.forced``: arrays over
    (E, T, 2, H) -- ``walker``, ``q`` (.., D), ``inside`` (in the box and finite), ``lpq``, ``lps``, ``diff``, ``logu``,
    ``accept``, ``margin``, ``face``, ``before`` (.., D) -- and, for the position bound of an accepted move, ``kind``, the
    plain-coordinate positions ``xs``, ``xj``, ``xk``, ``xl`` (.., D) of the walker and its partners, ``mult`` (zz, gamma
    or coef), ``normal`` (the DE draw n) and ``par`` (.., 2), the move's (p0, p1); ``move`` is (E, T)."""
    p0 = _as3(p0)
    E, W, D = p0.shape
    H = W // 2
    chain = np.asarray(chain, dtype=np.float64)
    T = chain.shape[0]
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    ch = chain.reshape(T, E, W, D)
    keys = ("walker", "q", "inside", "lpq", "lps", "diff", "logu", "accept", "margin", "face", "before", "kind", "xs", "xj",
            "xk", "xl", "mult", "normal", "par", "move")
    out = {k: [] for k in keys}
    tt = np.arange(T)[:, None]
    for e in range(E):
        k0, k1 = stream_keys(seed, e)
        dr = draws(np.arange(T), W, k0, k1, tab)
        kind, par = _per_iteration(tab, dr["move"])
        sidx, cidx = halves(dr["rot"], W)
        prev = np.concatenate([p0[e][None], ch[:-1, e]], axis=0)
        lp_rows = _lp(lp_fn, ch[:, e], _inside(ch[:, e] * sc, lo_sc, hi_sc))
        lp_p0 = _lp(lp_fn, p0[e], _inside(p0[e] * sc, lo_sc, hi_sc))
        lp_prev = np.concatenate([lp_p0[None], lp_rows[:-1]], axis=0)
        st = np.stack([prev, prev], axis=1)
        lst = np.stack([lp_prev, lp_prev], axis=1)
        s0 = sidx[:, 0]
        st[tt, 1, s0] = ch[tt, e, s0]
        lst[tt, 1, s0] = lp_rows[tt, s0]
        t3, sp3 = np.arange(T)[:, None, None], np.arange(2)[None, :, None]
        js, ks, ls = _partners(dr, kind)
        pick = lambda slots: st[t3, sp3, np.take_along_axis(cidx, slots, axis=2)]
        xs, xj, xk, xl = st[t3, sp3, sidx], pick(js), pick(ks), pick(ls)
        q, fac, mult = _propose(tab, kind, par, xs * sc, xj * sc, xk * sc, xl * sc, dr["u"], dr["de_n"], D)
        ok = _ok(q, lo_sc, hi_sc)
        with np.errstate(invalid="ignore", divide="ignore"):
            lpq = _lp(lp_fn, q / sc, ok)
            lps = lst[t3, sp3, sidx]
            diff = fac + lpq - lps
            logu = np.log(dr["uacc"])
            acc = ok & ~np.isnan(lpq) & (logu < diff)
            margin = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
            fc = np.where(np.all(np.isfinite(q), axis=-1), _face(q / sc, lo, hi), np.inf)
        k3 = kind[:, None, None] + np.zeros((T, 2, H), dtype=np.int64)
        pr = np.stack([par[0][:, None, None] + np.zeros((T, 2, H)), par[1][:, None, None] + np.zeros((T, 2, H))], axis=-1)
        for k, v in (("walker", sidx + e * W), ("q", q / sc), ("inside", ok), ("lpq", lpq), ("lps", lps), ("diff", diff),
                     ("logu", logu), ("accept", acc), ("margin", margin), ("face", fc), ("before", xs), ("kind", k3),
                     ("xs", xs), ("xj", xj), ("xk", xk), ("xl", xl), ("mult", mult), ("normal", dr["de_n"]), ("par", pr),
                     ("move", dr["move"])):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}
