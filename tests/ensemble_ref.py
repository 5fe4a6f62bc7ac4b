"""NumPy restatement of the on-device ensemble sampler's stretch move (csrc/ensemble.hip: ensemble_kernel and
ensemble_mw_kernel; both draw the same proposals) -- test infrastructure like gmm_ref.py: the checker the device is held
to, never the thing shipped.  It restates what the kernel implements, not emcee's move:

* keys: k0 = seed & 0xffffffff, k1 = (seed >> 32) ^ (ens * 0x9E3779B9 mod 2^32), seed taken mod 2^64 as gp.py does;
* partition offset of iteration it: rot = philox((it, it >> 32, 0xffffffff, 5))[0] % W; slot i of the active half is
  walker (i + split * H + rot) % W, slot i of the complement (i + (1 - split) * H + rot) % W;
* slot t of a half-step: counter (it, it >> 32, split * 256 + t, 1) gives u (words 0, 1) and the partner's complement slot
  (word 2 % H); z = (a - 1) u + 1, zz = z^2 / a, q = x_j - (x_j - x_s) zz, factor = (D - 1) log zz; counter word 3 = 2
  gives the acceptance uniform;
* accept iff q lies in the box in every dimension, lp(q) is not NaN and log u_acc < factor + lp(q) - lp(s); the slots of a
  half-step are decided in parallel against the state at its start.

The kernel holds the walkers in scaled coordinates x * sc (sc = sqrt(inv_metric / 2), the kernel's own scaling), forms
the proposal and gates the box there, and stores x = (x * sc) / sc; with ``sc`` given the restatement does the same, so
it differs from the device only by the kernel's fused multiply-add in q and the GP mean's rounding.
``lp_fn(points) -> values`` is the log-probability inside the box (the oracle's GP mean); outside it is -inf."""
import numpy as np

from philox_ref import philox4x32_10, u01

ENS_MAXW = 256
_MASK = np.uint64(0xFFFFFFFF)


def stream_keys(seed, ens=0):
    """Philox key (k0, k1) of ensemble ``ens`` for the Python ``seed`` handed to ``GP.sample_ensemble``."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, (s >> 32) ^ ((int(ens) * 0x9E3779B9) & 0xFFFFFFFF)


def draws(its, W, k0, k1):
    """Random numbers of iterations ``its``: ``rot`` (T,), and per (iteration, split, slot) the stretch uniform ``u``,
    the partner's complement slot ``jslot`` and the acceptance uniform ``uacc`` (T, 2, H)."""
    its = np.asarray(its, dtype=np.uint64).reshape(-1)
    H = W // 2
    cr = philox4x32_10(its & _MASK, its >> np.uint64(32), 0xFFFFFFFF, 5, k0, k1)
    rot = (cr[0] % np.uint64(W)).astype(np.int64)
    it3 = its[:, None, None]
    ctr = np.uint64(ENS_MAXW) * np.arange(2, dtype=np.uint64)[None, :, None] + np.arange(H, dtype=np.uint64)[None, None, :]
    c1 = philox4x32_10(it3 & _MASK, it3 >> np.uint64(32), ctr, 1, k0, k1)
    c2 = philox4x32_10(it3 & _MASK, it3 >> np.uint64(32), ctr, 2, k0, k1)
    return rot, u01(c1[0], c1[1]), (c1[2] % np.uint64(H)).astype(np.int64), u01(c2[0], c2[1])


def halves(rot, W):
    """Walker indices of the active half (T, 2, H) and of the complement for each split, given the offsets ``rot``."""
    H = W // 2
    slot = np.arange(H)[None, None, :]
    split = np.arange(2)[None, :, None]
    r = np.asarray(rot)[:, None, None]
    return (slot + split * H + r) % W, (slot + (1 - split) * H + r) % W


def _box(bounds, sc):
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    return b[:, 0] * sc, b[:, 1] * sc, b[:, 0], b[:, 1]


def _inside(pts_sc, lo_sc, hi_sc):
    return np.all((pts_sc >= lo_sc) & (pts_sc <= hi_sc), axis=-1)


def _lp(lp_fn, pts, ok):
    """lp_fn at the rows of ``pts`` (..., D) where ``ok``, -inf elsewhere."""
    out = np.full(pts.shape[:-1], -np.inf)
    if np.any(ok):
        out[ok] = np.asarray(lp_fn(pts[ok]), dtype=np.float64).reshape(-1)
    return out


def _move(cs_j, cs_s, u, a, D):
    z = (a - 1.0) * u + 1.0
    zz = z * z / a
    return cs_j - (cs_j - cs_s) * zz[..., None], (D - 1.0) * np.log(zz)


def _face(q, lo, hi):
    """Distance of q from the nearest face of the box, in units of the span, over all dimensions (>= 0 inside or out)."""
    span = hi - lo
    return np.min(np.minimum(np.abs(q - lo), np.abs(hi - q)) / span, axis=-1)


def _as3(p0):
    p0 = np.asarray(p0, dtype=np.float64)
    return p0[None] if p0.ndim == 2 else p0


def run(lp_fn, p0, iterations, bounds, a=2.0, seed=0, sc=None):
    """Free-running chain from ``p0`` ((W, D) or (E, W, D); ensemble e keyed by (seed, e) as the device keys block e).
    Returns ``chain`` (T, E W, D), ``log_prob`` (T, E W), ``naccept`` (E W), ``coords``, ``final_log_prob`` and the
    per-proposal record (``margin`` = |log u - diff|, ``face``) under ``decisions``, each (E, T, 2, H)."""
    p0 = _as3(p0)
    E, W, D = p0.shape
    H = W // 2
    T = int(iterations)
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    chain = np.empty((T, E, W, D))
    logp = np.empty((T, E, W))
    nacc = np.zeros((E, W), dtype=np.int64)
    coords = np.empty((E, W, D))
    final = np.empty((E, W))
    margin = np.full((E, T, 2, H), np.inf)
    face = np.full((E, T, 2, H), np.inf)
    for e in range(E):
        k0, k1 = stream_keys(seed, e)
        rot, u, jslot, uacc = draws(np.arange(T), W, k0, k1)
        sidx, cidx = halves(rot, W)
        cs = p0[e] * sc
        lp = _lp(lp_fn, cs / sc, _inside(cs, lo_sc, hi_sc))
        for it in range(T):
            for split in range(2):
                s = sidx[it, split]
                j = cidx[it, split][jslot[it, split]]
                q, fac = _move(cs[j], cs[s], u[it, split], a, D)
                ok = _inside(q, lo_sc, hi_sc)
                lpq = _lp(lp_fn, q / sc, ok)
                with np.errstate(invalid="ignore"):
                    diff = fac + lpq - lp[s]
                    logu = np.log(uacc[it, split])
                    acc = ok & ~np.isnan(lpq) & (logu < diff)
                    margin[e, it, split] = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
                face[e, it, split] = _face(q / sc, lo, hi)
                cs[s[acc]] = q[acc]
                lp[s[acc]] = lpq[acc]
                nacc[e, s[acc]] += 1
            chain[it, e] = cs / sc
            logp[it, e] = lp
        coords[e] = cs / sc
        final[e] = lp
    return {"chain": chain.reshape(T, E * W, D), "log_prob": logp.reshape(T, E * W), "naccept": nacc.reshape(E * W),
            "coords": coords.reshape(E * W, D), "final_log_prob": final.reshape(E * W),
            "decisions": {"margin": margin, "face": face}}


def forced(lp_fn, p0, chain, bounds, a=2.0, seed=0, sc=None):
    """Teacher-forced replay of a stored chain ``chain`` (T, E W, D) that started from ``p0``: every half-step is replayed
    from the state the chain itself records, so one near-tie cannot cascade.  Between the two halves of iteration it,
    the walkers of the first half hold ``chain[it]``, the others ``chain[it - 1]`` (``p0`` at it = 0).
    Returns arrays over (E, T, 2, H): ``walker`` (global index), ``partner``, ``q`` (.., D), ``inside``, ``lpq``, ``lps``,
    ``diff``, ``logu``, ``accept``, ``margin`` = |log u - diff| (inf where the decision does not hinge on it), ``face``,
    ``scale`` = max(|x_j|, |x_s|) per dimension (.., D); and ``before`` (.., D), the walker's coordinates at the start
    of the half-step as the chain records them."""
    p0 = _as3(p0)
    E, W, D = p0.shape
    H = W // 2
    chain = np.asarray(chain, dtype=np.float64)
    T = chain.shape[0]
    sc = np.ones(D) if sc is None else np.asarray(sc, dtype=np.float64)
    lo_sc, hi_sc, lo, hi = _box(bounds, sc)
    ch = chain.reshape(T, E, W, D)
    out = {k: [] for k in ("walker", "partner", "q", "inside", "lpq", "lps", "diff", "logu", "accept", "margin", "face",
                           "scale", "before")}
    tt = np.arange(T)[:, None]
    for e in range(E):
        k0, k1 = stream_keys(seed, e)
        rot, u, jslot, uacc = draws(np.arange(T), W, k0, k1)
        sidx, cidx = halves(rot, W)
        prev = np.concatenate([p0[e][None], ch[:-1, e]], axis=0)                    # (T, W, D) state before iteration it
        lp_rows = _lp(lp_fn, ch[:, e], _inside(ch[:, e] * sc, lo_sc, hi_sc))       # (T, W)
        lp_p0 = _lp(lp_fn, p0[e], _inside(p0[e] * sc, lo_sc, hi_sc))
        lp_prev = np.concatenate([lp_p0[None], lp_rows[:-1]], axis=0)
        st = np.stack([prev, prev], axis=1)                                       # (T, 2, W, D)
        lst = np.stack([lp_prev, lp_prev], axis=1)
        s0 = sidx[:, 0]
        st[tt, 1, s0] = ch[tt, e, s0]
        lst[tt, 1, s0] = lp_rows[tt, s0]
        t3, sp3 = np.arange(T)[:, None, None], np.arange(2)[None, :, None]
        j = np.take_along_axis(cidx, jslot, axis=2)
        xs, xj = st[t3, sp3, sidx], st[t3, sp3, j]                                # (T, 2, H, D)
        q, fac = _move(xj * sc, xs * sc, u, a, D)
        ok = _inside(q, lo_sc, hi_sc)
        lpq = _lp(lp_fn, q / sc, ok)
        lps = lst[t3, sp3, sidx]
        with np.errstate(invalid="ignore"):
            diff = fac + lpq - lps
            logu = np.log(uacc)
            acc = ok & ~np.isnan(lpq) & (logu < diff)
            margin = np.where(ok & np.isfinite(diff), np.abs(logu - diff), np.inf)
        for k, v in (("walker", sidx + e * W), ("partner", j + e * W), ("q", q / sc), ("inside", ok), ("lpq", lpq),
                     ("lps", lps), ("diff", diff), ("logu", logu), ("accept", acc), ("margin", margin),
                     ("face", _face(q / sc, lo, hi)), ("scale", np.maximum(np.abs(xj), np.abs(xs))), ("before", xs)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}
