# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): apgp_mix_candidates through GP.mixture_candidates against the NumPy restatement of
tests/evidence_ref.py: the draws within the Gaussian-draw bound of tests/test_gpu_priors.py (its GAUSS_K form, carried
through |A_k|), the chosen component exactly, ln q against NumPy's mixture log-density of the returned rows, sharding by
idx_offset, and the sample moments of 2e5 draws."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

GAUSS_K = 4.0          # tests/test_gpu_priors.py: |device - replay| <= GAUSS_K eps (sigma (1 + |z|) + |x|)
M = 100000


@functools.lru_cache(maxsize=None)
def _gp(D):
    from approxposterior_amd import gp as agp
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 2.0), ndim=D), mean=0.0, white_noise=-8.0)
    g.compute(np.random.RandomState(D).uniform(-1, 1, size=(8, D)))
    return g


@functools.lru_cache(maxsize=None)
def _drawn(K, D, seed):
    w, means, covs = er.mixture(K, D, seed)
    T, lnq = _gp(D).mixture_candidates(M, w, means, covs, seed)
    return (w, means, covs), T.cpu().numpy(), lnq.cpu().numpy()


@pytest.mark.parametrize("K,D,seed", er.MIX_CASES)
def test_draws_components_and_density_against_the_restatement(K, D, seed):
    (w, means, covs), T, lnq = _drawn(K, D, seed)
    rep, comp, z, near, A = er.mix_candidates_numpy(M, w, means, covs, seed)
    skipped = int(near.sum())
    print("K=%d D=%d: %d component uniforms within 1 ulp of a boundary skipped" % (K, D, skipped))
    assert skipped <= 2 * M // 100000
    keep = ~near
    assert T.shape == (M, D) and np.all(np.isfinite(T)) and np.all(np.isfinite(lnq))
    bound = er.mix_draw_bound(rep, comp, z, A, GAUSS_K)
    ratio = np.abs(T - rep)[keep] / bound[keep]
    print("K=%d D=%d: largest |device - replay| / bound = %.3f" % (K, D, ratio.max()))
    assert ratio.max() <= 1.0
    # the component is exact: a row drawn from another component would sit |c_k - c_k'| away, far outside the bound
    if K > 1:
        for k in range(K):
            other = means[k] + np.einsum("ij,mj->mi", A[k], z)
            wrong = keep & (comp != k) & np.all(np.abs(T - other) <= bound, axis=1)
            assert not wrong.any()
    # ln q at the STORED rows
    want, bud = er.mix_logpdf(T, w, means, covs)
    r = np.abs(lnq.astype(np.longdouble) - want).astype(np.float64) / bud
    print("K=%d D=%d: largest |lnq - numpy| / budget = %.3f" % (K, D, r.max()))
    assert r.max() <= 1.0


def test_cov_scale_scales_the_factor_and_the_density():
    w, means, covs = er.mixture(3, 3, 102)
    g = _gp(3)
    T, lnq = g.mixture_candidates(4096, w, means, covs, 5, covScale=2.25)
    T, lnq = T.cpu().numpy(), lnq.cpu().numpy()
    rep, comp, z, near, A = er.mix_candidates_numpy(4096, w, means, covs, 5, covScale=2.25)
    assert np.all(np.abs(T - rep)[~near] <= er.mix_draw_bound(rep, comp, z, A, GAUSS_K)[~near])
    want, bud = er.mix_logpdf(T, w, means, covs, covScale=2.25)
    assert np.all(np.abs(lnq.astype(np.longdouble) - want).astype(np.float64) <= bud)


@pytest.mark.parametrize("K,D,seed", [(3, 3, 102), (16, 8, 103)])
def test_two_chunks_concatenate_to_one_call(K, D, seed):
    (w, means, covs), T, lnq = _drawn(K, D, seed)
    g = _gp(D)
    cut = 33333
    a = g.mixture_candidates(cut, w, means, covs, seed, idx_offset=0)
    b = g.mixture_candidates(M - cut, w, means, covs, seed, idx_offset=cut)
    assert np.array_equal(np.concatenate([a[0].cpu().numpy(), b[0].cpu().numpy()]).view(np.int64), T.view(np.int64))
    assert np.array_equal(np.concatenate([a[1].cpu().numpy(), b[1].cpu().numpy()]).view(np.int64), lnq.view(np.int64))
    # a row far along the stream, alone, twice
    far = 2 ** 33 + 12345
    r1 = g.mixture_candidates(1, w, means, covs, seed, idx_offset=far)
    r2 = g.mixture_candidates(3, w, means, covs, seed, idx_offset=far - 2)
    assert np.array_equal(r1[0].cpu().numpy()[0], r2[0].cpu().numpy()[2]) and r1[1].cpu().numpy()[0] == r2[1].cpu().numpy()[2]
    rep = er.mix_candidates_numpy(1, w, means, covs, seed, offset=far)
    assert np.all(np.abs(r1[0].cpu().numpy() - rep[0]) <= er.mix_draw_bound(rep[0], rep[1], rep[2], rep[4], GAUSS_K))
    assert g.mixture_candidates(0, w, means, covs, seed)[0].shape == (0, D)


@pytest.mark.parametrize("K,D,seed", [(3, 3, 202), (16, 8, 203), (1, 1, 201)])
def test_sample_moments(K, D, seed):
    """Mean and covariance of 2e5 draws within 5 standard errors of the mixture's: se(mean_d) = sqrt(C_dd / m),
    se(C_de) = sqrt((E[x_d^2 x_e^2] - C_de^2) / m) with the fourth moment taken from the sample itself."""
    m = 200000
    w, means, covs = er.mixture(K, D, seed)
    T = _gp(D).mixture_candidates(m, w, means, covs, seed)[0].cpu().numpy()
    mean = w @ means
    d = means - mean
    C = np.einsum("k,kij->ij", w, covs) + np.einsum("k,ki,kj->ij", w, d, d)
    assert np.all(np.abs(T.mean(axis=0) - mean) <= 5.0 * np.sqrt(np.diag(C) / m))
    x = T - mean
    prod = np.einsum("mi,mj->mij", x, x)
    se = np.sqrt(np.maximum(prod.var(axis=0), 1e-300) / m)
    assert np.all(np.abs(prod.mean(axis=0) - C) <= 5.0 * se)


def test_the_python_layer_refuses_bad_mixtures():
    g = _gp(3)
    w, means, covs = er.mixture(3, 3, 102)
    bad = covs.copy()
    bad[1] = -np.eye(3)
    with pytest.raises(ValueError):
        g.mixture_candidates(10, w, means, bad, 1)
    with pytest.raises(ValueError):
        g.mixture_candidates(10, w, means[:, :2], covs[:, :2, :2], 1)       # not the GP's dimension
    with pytest.raises(ValueError):
        g.mixture_candidates(10, w, means, covs, 1, covScale=0.0)
