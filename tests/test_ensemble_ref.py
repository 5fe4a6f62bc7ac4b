"""CPU: the NumPy restatements the on-device ensemble sampler is replayed against (philox_ref.py, ensemble_ref.py), and the
plumbing of the stretch scale ``a`` into ``runMCMC(onDevice=True)``.  The GPU side is tests/test_gpu_ensemble_replay.py."""
import os
import sys

import numpy as np
import pytest

import ensemble_ref as er
from philox_ref import philox4x32_10, u01

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """The published Random123 known-answer vectors of philox4x32-10 (kat_vectors), scalar and broadcast over an array."""
    assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want
    many = philox4x32_10(np.full(5, ctr[0], dtype=np.uint64), ctr[1], ctr[2], ctr[3], *key)
    assert all(np.array_equal(m, np.full(5, w, dtype=np.uint64)) for m, w in zip(many, want))


def test_u01_is_the_open_unit_interval_53_bit_uniform():
    """u01 as ensemble.hip: (a >> 5) 2^26 + (b >> 6) + 1/2 over 2^53 -- never 0, never 1, a 2^-53 grid."""
    lo, hi = u01(0, 0), u01(0xFFFFFFFF, 0xFFFFFFFF)
    assert lo == 2.0 ** -54 and hi == 1.0 - 2.0 ** -54
    assert u01(1 << 5, 0) - lo == 2.0 ** -27 and u01(0, 1 << 6) - lo == 2.0 ** -53


def test_stream_keys_follow_the_device_key_schedule():
    """k0 = seed mod 2^32, k1 = (seed >> 32) ^ (ens * 0x9E3779B9 mod 2^32), the seed taken mod 2^64 as gp.py masks it."""
    assert er.stream_keys(7, 0) == (7, 0)
    assert er.stream_keys(7, 1) == (7, 0x9E3779B9)
    assert er.stream_keys(3 * 2 ** 32 + 5, 2) == (5, 3 ^ ((2 * 0x9E3779B9) & 0xFFFFFFFF))
    assert er.stream_keys(-1, 0) == (0xFFFFFFFF, 0xFFFFFFFF) == er.stream_keys(2 ** 64 - 1, 0)
    rot, u, jslot, uacc = er.draws(np.arange(50), 6, *er.stream_keys(11, 0))
    assert rot.shape == (50,) and u.shape == jslot.shape == uacc.shape == (50, 2, 3)
    assert rot.min() >= 0 and rot.max() < 6 and jslot.min() >= 0 and jslot.max() < 3
    assert len(set(rot.tolist())) == 6                       # every offset turns up
    s, c = er.halves(rot, 6)
    for it in range(50):                                     # the two halves partition the walkers, complement = other half
        assert sorted(s[it, 0].tolist() + s[it, 1].tolist()) == list(range(6))
        assert np.array_equal(c[it, 0], s[it, 1]) and np.array_equal(c[it, 1], s[it, 0])


def _gauss(D, seed):
    rs = np.random.RandomState(seed)
    A = rs.normal(size=(D, D))
    C = A @ A.T / D + 0.5 * np.eye(D)
    mu = rs.uniform(-1.0, 1.0, D)
    P = np.linalg.inv(C)
    return mu, C, lambda x: -0.5 * np.einsum("...i,ij,...j->...", x - mu, P, x - mu)


@pytest.mark.parametrize("D,W,E,T,a", [(3, 16, 2, 4000, 2.0), (8, 32, 2, 4000, 1.7)])
def test_restated_move_samples_a_correlated_gaussian(D, W, E, T, a):
    """The restated move is a valid stretch move, independently of any kernel: on an analytic correlated Gaussian (box far
    out) the chain's mean is within 5 batch-means standard errors and its covariance within 12 % of each entry's scale
    sqrt(C_ii C_jj), and the scaled-coordinate form (sc) samples the same target."""
    mu, C, lp = _gauss(D, D)
    rs = np.random.RandomState(100 + D)
    p0 = mu + 0.5 * rs.normal(size=(E, W, D))
    bounds = [(-40.0, 40.0)] * D
    sc = rs.uniform(0.3, 3.0, D)
    r = er.run(lp, p0, T, bounds, a=a, seed=2 ** 33 + D, sc=sc)
    x = r["chain"][T // 5:]                                  # (T', E W, D)
    walk = x.mean(axis=1)                                    # ensemble means per iteration
    nb = 20
    bm = walk[: len(walk) // nb * nb].reshape(nb, -1, D).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / np.sqrt(nb)
    m = x.reshape(-1, D).mean(axis=0)
    assert np.all(np.abs(m - mu) <= 5 * se + 1e-12), (m - mu, se)
    cov = np.cov(x.reshape(-1, D).T)
    scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
    assert np.abs(cov - C).max() <= 0.12 * scale.max() and np.all(np.abs(cov - C) <= 0.12 * scale), np.abs(cov - C) / scale
    acc = r["naccept"].sum() / (T * E * W)
    assert 0.2 < acc < 0.8
    assert np.all(np.isfinite(r["log_prob"])) and np.allclose(r["log_prob"], lp(r["chain"]), rtol=0, atol=1e-9)


def test_restated_chain_is_a_pure_function_of_seed_and_ensemble():
    """Same (seed, ensemble, start): the same chain bit for bit, whatever else runs beside it; another ensemble index or
    another seed: another stream; the forced replay of a free-running chain takes every one of its decisions."""
    mu, C, lp = _gauss(3, 5)
    rs = np.random.RandomState(9)
    p0 = mu + rs.normal(size=(3, 8, 3))
    b = [(-4.0, 4.0)] * 3
    r3 = er.run(lp, p0, 60, b, a=2.5, seed=-12345)
    again = er.run(lp, p0, 60, b, a=2.5, seed=-12345)
    assert np.array_equal(r3["chain"], again["chain"]) and np.array_equal(r3["naccept"], again["naccept"])
    r2 = er.run(lp, p0[:2], 60, b, a=2.5, seed=-12345)      # ensembles 0 and 1 alone
    assert np.array_equal(r2["chain"], r3["chain"][:, :16])
    same = er.run(lp, np.stack([p0[0]] * 3), 60, b, a=2.5, seed=-12345)      # one start, three ensemble indices
    ch = same["chain"].reshape(60, 3, 8, 3)
    assert not np.array_equal(ch[:, 0], ch[:, 1]) and not np.array_equal(ch[:, 1], ch[:, 2])
    assert np.array_equal(ch[:, 0], r3["chain"].reshape(60, 3, 8, 3)[:, 0])
    other = er.run(lp, p0, 60, b, a=2.5, seed=-12345 + 2 ** 32)             # differs in k1 only
    assert not np.array_equal(other["chain"], r3["chain"])
    f = er.forced(lp, p0, r3["chain"], b, a=2.5, seed=-12345)
    assert np.array_equal(np.bincount(f["walker"][f["accept"]], minlength=24), r3["naccept"])


def test_walkers_outside_the_box_and_on_its_faces():
    """A walker that starts outside the box has -inf until it takes a proposal (any proposal inside is taken); walkers on a
    face are inside; no accepted proposal leaves the box; the forced replay's accept counts are the free run's."""
    rs = np.random.RandomState(3)
    D, W = 2, 6
    p0 = rs.uniform(-1, 1, size=(W, D))
    p0[0] = [1.5, 0.0]                       # outside
    p0[1] = [-1.0, 0.3]                      # on the lower face of dimension 0
    p0[2] = [0.2, 1.0]                       # on the upper face of dimension 1
    b = [(-1.0, 1.0)] * D
    lp = lambda x: -np.sum(x ** 2, axis=-1)
    r = er.run(lp, p0, 40, b, a=2.0, seed=4)
    f = er.forced(lp, p0, r["chain"], b, a=2.0, seed=4)
    moved = np.any(r["chain"][:, 0] != p0[0], axis=1)
    first = int(np.argmax(moved))
    assert moved.any() and np.all(np.isneginf(r["log_prob"][:first, 0])) and np.all(np.isfinite(r["log_prob"][first:, 0]))
    own0 = (f["walker"] == 0) & f["inside"]
    assert np.all(f["accept"][own0 & np.isneginf(f["lps"])])                 # from -inf, every proposal inside is taken
    for w in (1, 2):
        assert np.all(np.isfinite(f["lps"][0, 0][f["walker"][0, 0] == w]))   # on a face: inside
    acc = f["accept"]
    assert np.all(f["inside"][acc]) and np.all(np.abs(f["q"][acc]) <= 1.0) and np.all(np.abs(r["chain"][:, 1:]) <= 1.0)
    assert np.bincount(f["walker"][acc], minlength=W).tolist() == r["naccept"].tolist()


class _RecordingGP(object):
    """Stands in for the HIP GP: records what reaches ``sample_ensemble`` and returns a fixed-shape result."""

    def __init__(self):
        self.calls = []

    def sample_ensemble(self, y, initial_state, iterations, bounds, a=2.0, seed=0, store=True):
        self.calls.append({"a": a, "seed": seed, "W": len(np.asarray(initial_state).reshape(-1, 2))})
        p0 = np.asarray(initial_state, dtype=float).reshape(-1, 2)
        T = int(iterations)
        chain = np.repeat(p0[None], T, axis=0)
        logp = np.zeros((T, len(p0)))
        return {"chain": chain, "log_prob": logp, "naccept": np.zeros(len(p0)), "coords": p0,
                "final_log_prob": logp[-1]}


def test_run_mcmc_on_device_passes_the_stretch_scale():
    """runMCMC(onDevice=True) hands samplerKwargs["a"] to GP.sample_ensemble (default 2.0, as the host sampler) and the
    returned chain records it; an initial_state whose rows disagree with nwalkers is refused as on the host."""
    sys.path.insert(0, ROOT)
    from approxposterior_amd import approx, likelihood as lh
    gp = _RecordingGP()
    ap = approx.ApproxPosterior(theta=np.zeros((3, 2)), y=np.zeros(3), gp=gp, lnprior=lh.rosenbrockLnprior,
                                lnlike=lh.rosenbrockLnlike, priorSample=lh.rosenbrockSample, bounds=((-5, 5),) * 2,
                                distributed=False)
    p0 = np.random.RandomState(0).uniform(-1, 1, size=(8, 2))
    kw = dict(cache=False, estBurnin=False, thinChains=False, onDevice=True)
    s, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": 8, "a": 3.0}, mcmcKwargs={"iterations": 5, "initial_state": p0}, **kw)
    assert gp.calls[-1]["a"] == 3.0 and s.a == 3.0 and gp.calls[-1]["W"] == 8
    s, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": 8}, mcmcKwargs={"iterations": 5, "initial_state": p0}, **kw)
    assert gp.calls[-1]["a"] == 2.0 and s.a == 2.0
    n = len(gp.calls)
    for bad in (p0[:6], p0.reshape(-1)[:12]):
        with pytest.raises(ValueError):
            ap.runMCMC(samplerKwargs={"nwalkers": 8}, mcmcKwargs={"iterations": 5, "initial_state": bad}, **kw)
    assert len(gp.calls) == n                                # refused before the device is touched
    s, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": 8, "a": 1.5},
                         mcmcKwargs={"iterations": 5, "initial_state": p0.reshape(-1)}, **kw)
    assert gp.calls[-1]["a"] == 1.5 and gp.calls[-1]["W"] == 8
