# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): the integrated acquisition end to end (GP.acquire_integrated, utility.EIVUtility,
findNextPoint(integrated=...); DESIGN.md "Integrated acquisition") on the 2-D Rosenbrock fixture of tests/golden
(N = 50) with M = 2000 candidates.

  * GP.acquire_integrated agrees with the scalar host form utility.EIVUtility (one predict(return_cov=True) over
    [theta; refs]) at the winner and at a sample of rows, for J = 1, 40, 300.  The bar: what NumPy's float64
    re-conditioning of the same fixture achieves against long double for tau^2 = var(r) - var'(r)
    (integrated_ref.recondition; the log-sum-exp moves by at most the largest error of an exponent), times 4 -- the
    device solves B in another order.  The ratio is printed (-s) and recorded in docs/experiments.md.
  * the pick's integrated expected variance, by the host form, is no larger than that of the BAPE pick from the same
    candidates;
  * findNextPoint(nCandidates=2000, integrated=64) returns a point inside the bounds, before and after
    runMCMC(onDevice=True); integrated=None draws and returns what the plain sweep does for the same seed."""
import os

import numpy as np
import pytest

import integrated_ref as ir
import kvalue_ref as kr

pytestmark = pytest.mark.gpu

M = 2000
SAMPLE = (0, 17, 503, 1999)


@pytest.fixture(scope="module")
def rosen(golden_dir):
    from approxposterior_amd import gp as agp
    g = np.load(os.path.join(golden_dir, "rosen2d_n50_amp.npz"))
    D = g["theta"].shape[1]
    p = g["p"]
    k = agp.Product(agp.ConstantKernel(p[1], ndim=D), agp.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]), fit_white_noise=False)
    gp.compute(g["theta"])
    rs = np.random.RandomState(5)
    lo, hi = np.asarray(g["lo"], dtype=float), np.asarray(g["hi"], dtype=float)
    T = rs.uniform(lo, hi, size=(M, D))
    refs = rs.uniform(lo, hi, size=(300, D))
    ks = gp._kernel_struct()
    kern = kr.kern([ks.inv_metric[d] for d in range(D)], amp=ks.amp, diag_add=ks.diag_add)
    return dict(gp=gp, X=np.array(g["theta"]), y=np.array(g["y"]), T=T, refs=refs, kern=kern,
                bounds=list(zip(lo, hi)))


def _bar(rosen, refs, rows):
    """4 x the worst error of the float64 re-conditioned tau^2 against long double over ``rows`` of the candidates."""
    worst = 0.0
    for r in rows:
        _, drop_ld, drop_64 = ir.recondition(rosen["X"], refs, rosen["T"][r], rosen["kern"])
        worst = max(worst, float(np.abs(drop_64 - drop_ld.astype(np.float64)).max()))
    return 4.0 * worst


@pytest.mark.parametrize("J", (1, 40, 300))
def test_acquire_integrated_agrees_with_the_host_utility(rosen, J):
    from approxposterior_amd import utility as ut
    gp, y, T, refs = rosen["gp"], rosen["y"], rosen["T"], rosen["refs"][:J]
    w = gp.integration_weights(y, refs, "posterior")
    mu_r, var_r = gp.predict(y, refs, return_cov=False, return_var=True)
    assert np.allclose(w, mu_r + var_r, rtol=1e-12, atol=1e-12)
    assert np.allclose(gp.integration_weights(y, refs, "uniform"), w + mu_r, rtol=1e-12, atol=1e-12)
    before = gp.get_parameter_vector().copy()
    bi, bu, u, mu, var = gp.acquire_integrated(y, T, refs, logWeights=w, bounds=rosen["bounds"], return_all=True)
    assert np.array_equal(gp.get_parameter_vector(), before)
    assert (bi, bu) == gp.acquire_integrated(y, T, refs, logWeights=w, bounds=rosen["bounds"])
    assert (bi, bu) == ir.argmin(u) and 0 <= bi < M
    rows = sorted(set(SAMPLE) | {bi})
    bar = _bar(rosen, refs, rows)
    prior = lambda t: 0.0                                           # noqa: E731
    worst = 0.0
    for r in rows:
        host = float(ut.EIVUtility(T[r], y, gp, prior, refs, w))
        worst = max(worst, abs(host - u[r]))
    print("J %d: |device u - host EIVUtility| %.3g, bar %.3g, ratio %.3g" % (J, worst, bar, worst / bar))
    assert worst <= bar
    if J == 300:
        # logWeights=None is integration_weights(..., "posterior")
        assert gp.acquire_integrated(y, T, refs, bounds=rosen["bounds"]) == (bi, bu)


def test_the_pick_beats_the_bape_pick_in_integrated_variance(rosen):
    from approxposterior_amd import utility as ut
    gp, y, T, refs = rosen["gp"], rosen["y"], rosen["T"], rosen["refs"][:40]
    w = gp.integration_weights(y, refs, "posterior")
    bi, _ = gp.acquire_integrated(y, T, refs, logWeights=w, bounds=rosen["bounds"])
    bb, _ = gp.acquire(y, T, "bape", bounds=rosen["bounds"])
    prior = lambda t: 0.0                                           # noqa: E731
    ui = float(ut.EIVUtility(T[bi], y, gp, prior, refs, w))
    ub = float(ut.EIVUtility(T[bb], y, gp, prior, refs, w))
    print("EIV pick %d u %.6g, BAPE pick %d u %.6g" % (bi, ui, bb, ub))
    # u is minus the log of the variance REMOVED from the integral: the smaller, the smaller what is left
    assert ui <= ub + _bar(rosen, refs, [bi, bb])


def _ap(rosen):
    from approxposterior_amd import approx, likelihood as lh
    from approxposterior_amd import gp as agp
    g0 = rosen["gp"]
    gp = agp.GP(kernel=g0.kernel, fit_mean=True, mean=g0.mean, white_noise=g0.white_noise, fit_white_noise=False)
    gp.compute(rosen["X"])
    return approx.ApproxPosterior(theta=rosen["X"].copy(), y=rosen["y"].copy(), gp=gp, lnprior=lh.rosenbrockLnprior,
                                  lnlike=lh.rosenbrockLnlike, priorSample=lh.rosenbrockSample,
                                  bounds=[(-5, 5), (-5, 5)], algorithm="bape")


def test_find_next_point_integrated(rosen, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap(rosen)
    np.random.seed(11)
    with np.errstate(all="ignore"):
        first = ap.findNextPoint(computeLnLike=False, nCandidates=2000, integrated=64, verbose=False)
        assert first.shape == (2,) and np.all(np.abs(first) <= 5.0) and len(ap.y) == 50
        p0 = np.array(ap.priorSample(20))
        ap.runMCMC(samplerKwargs={"nwalkers": 20}, mcmcKwargs={"iterations": 400, "initial_state": p0}, cache=False, estBurnin=True,
                   thinChains=True, onDevice=True, verbose=False)
        refs, density = ap._integrationRefs(64)
        assert refs.shape == (64, 2) and density == "posterior" and np.all(np.abs(refs) <= 5.0)
        second = ap.findNextPoint(computeLnLike=False, nCandidates=2000, integrated=64, verbose=False)
        assert second.shape == (2,) and np.all(np.abs(second) <= 5.0)
        third = ap.findNextPoint(computeLnLike=False, nCandidates=2000, integrated=refs[:7], deviceCandidates=True,
                                 verbose=False)
        assert third.shape == (2,) and np.all(np.abs(third) <= 5.0)


def test_integrated_none_is_the_plain_sweep(rosen, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap(rosen)
    with np.errstate(all="ignore"):
        np.random.seed(23)
        plain = ap.findNextPoint(computeLnLike=False, nCandidates=2000, verbose=False)
        np.random.seed(23)
        none = ap.findNextPoint(computeLnLike=False, nCandidates=2000, integrated=None, verbose=False)
        np.random.seed(23)
        draws = np.asarray(ap.priorSample(2000), dtype=float).reshape(2000, -1)
        bi, _ = ap.gp.acquire(ap.y, draws, "bape", bounds=ap.bounds)
    assert plain.tobytes() == none.tobytes() == draws[bi].tobytes()
