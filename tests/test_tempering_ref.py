# -*- coding: utf-8 -*-
"""CPU: parallel tempering's host side -- the NumPy restatement of the tempered sampler (tests/tempering_ref.py) on its
own, ``mcmc.tempering_ladder``, the arithmetic of ``mcmc.TemperedChain`` on synthetic results, and the ``tempering``
keyword's guard.  No device code runs here."""
import math

import numpy as np
import pytest

import ensemble_moves_ref as emr
import george_oracle as go
import tempering_ref as tr
from approxposterior_amd import approx, likelihood as lh, mcmc, mcmcUtils


def _quadratic(pts):
    return -0.5 * np.sum(np.asarray(pts) ** 2, axis=-1)


def _truncated_mean_lp(beta, D, edge):
    """E[-|x|^2 / 2] under exp(-beta |x|^2 / 2) on [-edge, edge]^D: -(D / 2) E[x^2] of a normal of variance 1 / beta
    truncated at a = edge sqrt(beta) standard deviations, E[x^2] = (1 - 2 a phi(a) / (2 Phi(a) - 1)) / beta."""
    a = edge * math.sqrt(beta)
    phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    mass = math.erf(a / math.sqrt(2.0))
    return -0.5 * D * (1.0 - 2.0 * a * phi / mass) / beta


def test_reference_ladder_is_stationary():
    """lp = -|x|^2 / 2 on [-10, 10]^2, betas (1, 0.5, 0.2, 0.05), 8 ladders of 8 walkers, 1200 iterations with an exchange
    round every 5, the first 200 discarded (about 25 s): every rung's mean lp lies within 5 standard errors (between
    ladders) of its expectation.  That expectation is -D / (2 beta) of the untruncated normal for the three colder
    rungs to better than 1e-3; at beta = 0.05 the box cuts the normal at 2.24 standard deviations and the expectation
    is -17.0, not -20: the test uses the truncated normal's exact value at every beta."""
    D, W, L, N, discard = 2, 8, 8, 1200, 200
    betas = np.array([1.0, 0.5, 0.2, 0.05])
    rs = np.random.RandomState(11)
    p0 = rs.uniform(-1.0, 1.0, size=(L, len(betas), W, D))
    out = tr.run(_quadratic, p0, N, [(-10.0, 10.0)] * D, emr.table(("stretch", 2.0), D), betas, 5, seed=5, ladders=L)
    per = out["log_prob"][discard:].mean(axis=(0, 3))                      # (L, T)
    mean, se = per.mean(axis=0), per.std(axis=0, ddof=1) / np.sqrt(L)
    want = np.array([_truncated_mean_lp(b, D, 10.0) for b in betas])
    assert abs(want[0] + D / 2.0) < 1e-12 and abs(want[2] + D / (2 * 0.2)) < 1e-3 and abs(want[3] + 17.0) < 0.05
    print("rung means", mean, "expected", want, "standard errors", se, "z", (mean - want) / se)
    print("exchange acceptance", out["swap_acc"].sum(axis=0) / out["swap_prop"].sum(axis=0))
    assert np.all(np.abs(mean - want) <= 5.0 * se)
    assert np.all(out["swap_acc"] > 0) and np.all(out["swap_acc"] < out["swap_prop"])


def test_one_rung_is_the_ensemble_reference():
    D, W, L, N = 2, 8, 3, 23
    tab = emr.table([(("stretch", 2.0), .4), (("de", 1e-5, None), .4), (("snooker", 1.7), .2)], D)
    rs = np.random.RandomState(3)
    p0 = rs.uniform(-1.5, 1.5, size=(L, W, D))
    p0[0, 0, 0] = 4.0                                               # outside the box: -inf until it takes a proposal
    b = [(-2.0, 2.0)] * D
    sc = np.array([0.7, 1.3])
    want = emr.run(_quadratic, p0, N, b, tab, seed=2 ** 33 + 5, sc=sc)
    got = tr.run(_quadratic, p0[:, None], N, b, tab, [1.0], 4, seed=2 ** 33 + 5, sc=sc, ladders=L)
    assert np.array_equal(got["chain"].reshape(N, L * W, D), want["chain"])
    assert np.array_equal(got["log_prob"].reshape(N, L * W), want["log_prob"])
    assert np.array_equal(got["naccept"].reshape(L * W), want["naccept"])
    assert np.array_equal(got["coords"].reshape(L * W, D), want["coords"])
    assert np.array_equal(got["final_log_prob"].reshape(L * W), want["final_log_prob"])
    assert np.array_equal(got["decisions"]["margin"], want["decisions"]["margin"])
    assert got["swap_log"].shape == (5, L, 0, W)


@pytest.mark.parametrize("T,se,spec", [(2, 1, ("stretch", 2.0)), (3, 3, [(("de", 1e-5, None), .5), (("snooker", 1.7), .5)]),
                                       (5, 2, ("stretch", 2.0))])
def test_forced_replay_reproduces_the_free_run(T, se, spec):
    """The teacher-forced replay of the free run's own chain and exchange log gives the free run's decisions back."""
    D, W, L, N, seed = 2, 8, 2, 21, 6
    tab = emr.table(spec, D)
    betas = mcmc.tempering_ladder(T, 0.05)
    rs = np.random.RandomState(T)
    p0 = rs.uniform(-1.5, 1.5, size=(L, T, W, D))
    p0[0, 0, 0, 0] = 5.0
    b, sc = [(-2.0, 2.0)] * D, np.array([0.8, 1.2])
    free = tr.run(_quadratic, p0, N, b, tab, betas, se, seed=seed, sc=sc, ladders=L)
    f = tr.forced(_quadratic, p0, free["chain"], free["swap_log"], b, tab, betas, se, seed=seed, sc=sc)
    assert np.array_equal(f["swaps"]["log"], free["swap_log"]) and (free["swap_log"] == 2).sum() > 0
    m = f["moves"]
    w = m["walker"].reshape(L, T, N, 2, W // 2)
    t = np.arange(N)[None, None, :, None, None]
    li, ki = np.arange(L)[:, None, None, None, None], np.arange(T)[None, :, None, None, None]
    before, after = f["prev"][t, li, ki, w], free["chain"][t, li, ki, w]
    moved = np.any(np.abs(after - before) > 4 * np.spacing(np.abs(before)), axis=-1)      # ((x sc) / sc is not x to the bit)
    acc = m["accept"].reshape(moved.shape)
    assert np.array_equal(moved, acc) and acc.sum() > 0 and (~acc).sum() > 0
    count = np.zeros((L, T, W), dtype=np.int64)
    np.add.at(count, (np.broadcast_to(li, w.shape)[acc], np.broadcast_to(ki, w.shape)[acc], w[acc]), 1)
    assert np.array_equal(count, free["naccept"])
    assert np.allclose(m["margin"], free["decisions"]["margin"], rtol=1e-6, atol=1e-9)


def test_equal_betas_accept_every_proposed_exchange():
    D, W, N = 2, 6, 12
    rs = np.random.RandomState(4)
    p0 = rs.uniform(-1.5, 1.5, size=(3, W, D))
    p0[1, 2, 1] = 9.0                                               # a walker that starts outside: not proposed while -inf
    out = tr.run(_quadratic, p0, N, [(-2.0, 2.0)] * D, emr.table(("stretch", 2.0), D), [1.0, 1.0, 1.0], 1, seed=9)
    log = out["swap_log"]
    assert log.shape == (N - 1, 1, 2, W)
    for r in range(N - 1):
        assert np.all(log[r, :, 1 - r % 2] == 0)                    # the pair that sits round r out
    assert np.all((log == 0) | (log == 2)) and (log == 2).sum() > 0
    assert np.array_equal(out["swap_acc"], out["swap_prop"]) and np.all(out["swap_prop"] > 0)
    assert (log[0, 0, 0] == 0).sum() <= 1                           # only the -inf walker can go unproposed


def test_tempering_ladder():
    assert np.array_equal(mcmc.tempering_ladder(1, 0.1), [1.0])
    assert np.array_equal(mcmc.tempering_ladder(2, 0.1), [1.0, 0.0])
    assert np.allclose(mcmc.tempering_ladder(4, 0.01), [1.0, 0.1, 0.01, 0.0], rtol=1e-15)
    assert np.allclose(mcmc.tempering_ladder(4, 0.001, zero=False), [1.0, 0.1, 0.01, 0.001], rtol=1e-14)
    b = mcmc.tempering_ladder(8, 1e-3)
    assert b[0] == 1.0 and b[-1] == 0.0 and b[-2] == 1e-3 and np.all(np.diff(b) < 0)
    assert np.allclose(b[1:-1] / b[:-2], b[1] / b[0])               # geometric
    for bad in (dict(ntemps=0, betaMin=.1), dict(ntemps=65, betaMin=.1), dict(ntemps=4, betaMin=0.0),
                dict(ntemps=4, betaMin=1.0)):
        with pytest.raises(ValueError):
            mcmc.tempering_ladder(**bad)


def _synthetic(L, betas, N=40, W=4, D=2, noise=0.0, seed=0):
    rs = np.random.RandomState(seed)
    T = len(betas)
    level = -3.0 / (0.2 + np.asarray(betas))                        # a smooth E_beta[mu]
    rung = level[None, None, :] + noise * rs.standard_normal((N, L, T))
    return {"chain": rs.uniform(size=(N, L * W, D)), "log_prob": rs.uniform(size=(N, L * W)),
            "coords": rs.uniform(size=(L * W, D)), "final_log_prob": rs.uniform(size=L * W),
            "naccept": np.full(L * W, N // 2), "betas": np.asarray(betas, dtype=float),
            "rung_naccept": np.arange(L * T * W).reshape(L, T, W) % (N + 1),
            "swap_proposed": np.full((L, T - 1), 10), "swap_accepted": np.arange(L * (T - 1)).reshape(L, T - 1) % 11,
            "rung_mean_log_prob": rung, "log_volume": 1.25, "swap_every": 5}, level


def test_log_evidence_arithmetic():
    betas = [1.0, 0.5, 0.25, 0.1, 0.0]
    res, level = _synthetic(3, betas, noise=0.3, seed=2)
    ch = mcmc.TemperedChain(res)
    logz, disc, mc = ch.log_evidence(discard=10)
    per = res["rung_mean_log_prob"][10:].mean(axis=0)               # (L, T)
    trap = lambda b, f: sum((b[i] - b[i + 1]) * 0.5 * (f[i] + f[i + 1]) for i in range(len(b) - 1))
    each = np.array([trap(betas, per[l]) for l in range(3)])
    assert abs(logz - (1.25 + each.mean())) < 1e-12
    assert abs(disc - abs(trap(betas, per.mean(axis=0)) - trap(betas[::2], per.mean(axis=0)[::2]))) < 1e-12
    assert abs(mc - each.std(ddof=1) / np.sqrt(3.0)) < 1e-12
    assert abs(ch.log_evidence(discard=10, logVolume=0.0)[0] - each.mean()) < 1e-12
    # an even number of rungs: "every other rung" keeps the last one
    b4 = [1.0, 0.4, 0.1, 0.0]
    res4, _ = _synthetic(2, b4)
    m = res4["rung_mean_log_prob"][0, 0]
    _, disc4, mc4 = mcmc.TemperedChain(res4).log_evidence()
    assert abs(disc4 - abs(trap(b4, m) - trap([1.0, 0.1, 0.0], m[[0, 2, 3]]))) < 1e-12 and mc4 < 1e-12
    # one ladder: the rungs' batch-means errors under the trapezoid weights
    res1, _ = _synthetic(1, betas, N=400, noise=0.5, seed=3)
    _, _, mc1 = mcmc.TemperedChain(res1).log_evidence(discard=0)
    w = np.array([0.25, 0.375, 0.2, 0.125, 0.05])
    se = mcmcUtils.batchMeansMCSE(res1["rung_mean_log_prob"][:, 0, :])
    assert abs(mc1 - np.sqrt(np.sum((w * se) ** 2))) < 1e-12 and mc1 > 0
    # no beta = 0 rung: no integral from 0
    resn, _ = _synthetic(2, [1.0, 0.5, 0.1])
    with pytest.raises(ValueError, match="end at 0"):
        mcmc.TemperedChain(resn).log_evidence()
    res.pop("log_volume")
    with pytest.raises(ValueError, match="logVolume"):
        mcmc.TemperedChain(res).log_evidence()


def test_tempered_chain_accessors():
    betas = [1.0, 0.3, 0.0]
    L, N, W, D = 2, 40, 4, 2
    res, _ = _synthetic(L, betas, N=N, W=W, D=D)
    ch = mcmc.TemperedChain(res, moves=mcmc.DEMove())
    assert isinstance(ch, mcmc.DeviceChain) and ch.nwalkers == L * W and ch.ndim == D and ch.iteration == N
    assert ch.ntemps == 3 and ch.nladders == L and np.array_equal(ch.betas, betas) and ch.swap_every == 5
    assert np.array_equal(ch.get_chain(discard=5, thin=2), res["chain"][6::2])
    assert ch.get_chain(flat=True).shape == (N * L * W, D) and ch.get_log_prob().shape == (N, L * W)
    assert np.allclose(ch.acceptance_fraction, 0.5)
    assert np.allclose(ch.swap_acceptance_fraction, res["swap_accepted"].sum(axis=0) / 20.0)
    assert np.allclose(ch.rung_acceptance_fraction, res["rung_naccept"].mean(axis=(0, 2)) / N)
    assert ch.rung_means(discard=3).shape == (L, 3)
    assert isinstance(ch.moves[0][0], mcmc.DEMove)
    with pytest.raises(NotImplementedError):
        ch.sample(None)
    res["swap_proposed"] = np.zeros((L, 2))
    assert np.all(np.isnan(mcmc.TemperedChain(res).swap_acceptance_fraction))


def test_tempering_needs_the_device_sampler():
    np.random.seed(57)
    theta = np.array(list(lh.rosenbrockSample(20)) + [[-5, 5], [5, 5]])
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = go.GP(kernel=go.ExpSquaredKernel(metric=[1.0, 1.0], ndim=2), fit_mean=True, mean=np.median(y), white_noise=-12,
               fit_white_noise=False)
    gp.compute(theta)
    ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                priorSample=lh.rosenbrockSample, bounds=((-5, 5), (-5, 5)), algorithm="bape")
    with pytest.raises(ValueError, match="onDevice=True"):
        ap.runMCMC(samplerKwargs={"nwalkers": 4}, mcmcKwargs={"iterations": 5}, cache=False, onDevice=False, tempering=4)
    with pytest.raises(ValueError, match="onDevice=True"):
        ap.run(m=1, nmax=1, cache=False, verbose=False, onDevice=False, tempering={"ntemps": 3})
