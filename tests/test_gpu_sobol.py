# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): the quasi-random draws (csrc/sobol.hip) through GP.sobol_candidates against the NumPy restatement
of tests/sobol_ref.py -- the sequence to the bit, the box and Uniform factors to the bit, Gaussian factors and the mixture
within the budgets of tests/test_gpu_priors.py and tests/evidence_ref.py -- and what is built on them:
ApproxPosterior.evidence(qmc=) on the D = 2 quadratic case of tests/evidence_ref.py against a quadrature and against the
pseudo-random estimate, findNextPoint(deviceCandidates="sobol"), sobolSample.

Shapes: m = 1000 (no multiple of the 256 rows of a workgroup, four workgroups) from idx_offset = 2^16 - 300, so that the
carry into Gray bit 16 falls inside the call; row 0 alone (no bit set) and the last rows of the sequence (all 30)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
import sobol_ref as sr  # noqa: E402
from test_gpu_evidence import _ap, _quad  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GAUSS_K = 4.0          # tests/test_gpu_priors.py: |device - replay| <= GAUSS_K eps (sigma (1 + |z|) + |x|)
M = 1000
OFF = 2 ** 16 - 300
DIMS = (1, 2, 8, 32)
SEED = er.EVIDENCE_SEED
N_EVID = 2 ** 16
QMC = 16


@functools.lru_cache(maxsize=None)
def _gp(D):
    """A computed GP of dimension D (the draws only need its dimension, device and stream)."""
    from approxposterior_amd import gp as agp
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 2.0), ndim=D), mean=0.0, white_noise=-8.0)
    g.compute(np.random.RandomState(D).uniform(-1, 1, size=(8, D)))
    return g


def _bounds(D):
    lo = -1.0 - 0.37 * np.arange(D)
    hi = 2.0 + 0.21 * np.arange(D)
    return lo, hi, np.stack([lo, hi], axis=1)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("D", DIMS)
def test_unscrambled_box_is_the_sequence(D):
    unit = [(0.0, 1.0)] * D
    T = _gp(D).sobol_candidates(M, bounds=unit, seed=9, replicate=4, scramble=False, idx_offset=OFF).cpu().numpy()
    assert T.shape == (M, D) and np.all((T > 0.0) & (T < 1.0))
    assert np.array_equal(np.floor(T * 2.0 ** 32).astype(np.uint64), sr.points(M, D, offset=OFF))
    assert _same_bits(T, sr.uniforms(M, D, 0, offset=OFF, scramble=False))


@pytest.mark.parametrize("D", DIMS)
def test_scrambled_box_is_the_restatement_to_the_bit(D):
    lo, hi, b = _bounds(D)
    seed = 2 ** 40 + 77 + D
    T = _gp(D).sobol_candidates(M, bounds=b, seed=seed, replicate=3, idx_offset=OFF).cpu().numpy()
    assert _same_bits(T, sr.box(M, lo, hi, seed, replicate=3, offset=OFF))
    assert np.all((T >= lo) & (T <= hi))


def test_replicates_chunks_single_rows_and_the_ends_of_the_sequence():
    D = 8
    g = _gp(D)
    lo, hi, b = _bounds(D)
    draw = lambda m, off, rep=0, seed=11: g.sobol_candidates(m, bounds=b, seed=seed, replicate=rep,      # noqa: E731
                                                             idx_offset=off).cpu().numpy()
    whole = draw(M, OFF)
    assert not np.array_equal(whole, draw(M, OFF, rep=1)) and not np.array_equal(whole, draw(M, OFF, seed=12))
    # every replicate fills the box on its own: the first 256 rows put one point in each of 256 slabs of every dimension
    for rep in (0, 1):
        first = draw(256, 0, rep=rep)
        cells = np.floor((first - lo) / (hi - lo) * 256).astype(np.int64)
        assert all(np.array_equal(np.sort(cells[:, d]), np.arange(256)) for d in range(D))
    cut = 333
    assert _same_bits(np.concatenate([draw(cut, OFF), draw(M - cut, OFF + cut)]), whole)
    for i in (0, 299, 300, M - 1):              # (rows 2^16 - 1 and 2^16: either side of the carry)
        assert _same_bits(draw(1, OFF + i), whole[i:i + 1])
    # row 0 alone sets no bit of the Gray code, the last rows set all 30
    assert _same_bits(draw(1, 0), sr.box(1, lo, hi, 11))
    last = sr.MAX_ROWS - 5
    assert _same_bits(draw(5, last), sr.box(5, lo, hi, 11, offset=last))
    assert draw(0, 0).shape == (0, D)
    from approxposterior_amd import _lib
    with pytest.raises(_lib.ApgpError):
        draw(6, last)
    with pytest.raises(ValueError):
        g.sobol_candidates(4)
    with pytest.raises(ValueError):
        g.sobol_candidates(4, bounds=b, prior=object())


def test_prior_with_alternating_uniform_and_gaussian_factors():
    from approxposterior_amd import priors as P
    D = 5
    J = P.JointPrior([P.UniformPrior(-3.0, 4.5), P.GaussianPrior(0.5, 2.0), P.UniformPrior(10.0, 10.25),
                      P.GaussianPrior(-40.0, 0.03), P.UniformPrior(-1e3, 1e3)])
    kind, p0, p1 = J.records()
    dev = _gp(D).sobol_candidates(M, prior=J, seed=31, replicate=2, idx_offset=OFF).cpu().numpy()
    rep, u = sr.prior(M, kind, p0, p1, 31, replicate=2, offset=OFF)
    uni = np.asarray(kind) == 0
    assert _same_bits(dev[:, uni], rep[:, uni])
    gs = ~uni
    z = (rep[:, gs] - p0[gs]) / p1[gs]
    ratio = np.abs(dev[:, gs] - rep[:, gs]) / (EPS * (p1[gs] * (1.0 + np.abs(z)) + np.abs(rep[:, gs])))
    print("Gaussian factors: largest |device - replay| / (eps (sigma (1 + |z|) + |x|)) = %.3f" % ratio.max())
    assert np.all(np.isfinite(dev)) and ratio.max() <= GAUSS_K
    # chunks and single rows as for the box
    g = _gp(D)
    two = [g.sobol_candidates(m, prior=J, seed=31, replicate=2, idx_offset=o).cpu().numpy() for m, o in ((300, OFF), (700, OFF + 300))]
    assert _same_bits(np.concatenate(two), dev)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("D", [2, 8, 32])
def test_mixture_components_draws_and_density(K, D):
    seed = 500 + 10 * K + D
    w, means, covs = er.mixture(K, D, seed)
    g = _gp(D)
    T, lnq = g.sobol_candidates(M, mixture=(w, means, covs), seed=seed, replicate=1, idx_offset=OFF)
    T, lnq = T.cpu().numpy(), lnq.cpu().numpy()
    rep, comp, z, near, A = sr.mixture(M, w, means, covs, seed, replicate=1, offset=OFF)
    assert int(near.sum()) <= 2 * max(M // 100000, 0)          # (2 per 100 000 rows: none at this size)
    assert T.shape == (M, D) and lnq.shape == (M,) and np.all(np.isfinite(T)) and np.all(np.isfinite(lnq))
    bound = er.mix_draw_bound(rep, comp, z, A, GAUSS_K)
    ratio = np.abs(T - rep) / bound
    print("K=%d D=%d: largest |device - replay| / bound = %.3f" % (K, D, ratio.max()))
    assert ratio.max() <= 1.0
    # the component is exact: a row drawn from another component would sit |c_k - c_k'| away, far outside the bound
    if K > 1:
        assert len(np.unique(comp)) == K
        for k in range(K):
            other = means[k] + np.einsum("ij,mj->mi", A[k], z)
            assert not ((comp != k) & np.all(np.abs(T - other) <= bound, axis=1)).any()
    want, bud = er.mix_logpdf(T, w, means, covs)
    r = np.abs(lnq.astype(np.longdouble) - want).astype(np.float64) / bud
    print("K=%d D=%d: largest |lnq - numpy| / budget = %.3f" % (K, D, r.max()))
    assert r.max() <= 1.0
    # two chunks, one call
    a = g.sobol_candidates(300, mixture=(w, means, covs), seed=seed, replicate=1, idx_offset=OFF)
    b = g.sobol_candidates(700, mixture=(w, means, covs), seed=seed, replicate=1, idx_offset=OFF + 300)
    assert _same_bits(np.concatenate([a[0].cpu().numpy(), b[0].cpu().numpy()]), T)
    assert _same_bits(np.concatenate([a[1].cpu().numpy(), b[1].cpu().numpy()]), lnq)


# ----------------------------------------------------------------------------------------------------------------------
# evidence(qmc=)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quad1200():
    return er.quadrature(er.quadratic_case(), n=1200)


@functools.lru_cache(maxsize=None)
def _box_estimates():
    """(the evidence object, the qmc estimate, the pseudo-random one at the same nSamples and seed)."""
    a = _ap()
    return a, a.evidence(nSamples=N_EVID, proposal="box", seed=SEED, qmc=QMC), \
        a.evidence(nSamples=N_EVID, proposal="box", seed=SEED)


def test_evidence_box_proposal_against_the_quadrature_and_the_pseudo_random_error():
    a, s, p = _box_estimates()
    logZ, mean, cov = _quad1200()
    print("box qmc=%d: logZ %.9f +- %.3e (iid figure %.3e; quadrature %.9f, off by %.2f errors), ess %.0f; Philox +- %.3e: "
          "ratio %.0f" % (QMC, s["logZ"], s["logZErr"], s["logZErrIID"], logZ, abs(s["logZ"] - logZ) / s["logZErr"],
                          s["ess"], p["logZErr"], p["logZErr"] / s["logZErr"]))
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    assert s["logZErr"] <= p["logZErr"] / 20.0
    assert s["qmc"] == QMC and s["nInside"] == N_EVID and s["logZReplicates"].shape == (QMC,)
    assert s["meanReplicates"].shape == (QMC, 2) and s["meanErr"].shape == (2,)
    e, m = sr.replicates_summary(s["logZReplicates"], s["meanReplicates"])
    assert abs(s["logZErr"] - e) <= 1e-12 * e and np.allclose(s["meanErr"], m, rtol=1e-12, atol=0)
    assert np.all(np.abs(s["mean"] - mean) <= 4.0 * s["meanErr"] + 1e-7)      # (1e-7: the quadrature's own error)
    # the iid figure is the pseudo-random one's size: the rows' weights have the same variance
    assert 0.5 * p["logZErr"] <= s["logZErrIID"] <= 2.0 * p["logZErr"]


def test_evidence_qmc_does_not_depend_on_the_chunk_and_none_is_the_parent():
    a, s, p = _box_estimates()
    for chunk in (2 ** 10, 1234):
        t = a.evidence(nSamples=N_EVID, proposal="box", seed=SEED, qmc=QMC, chunk=chunk)
        assert abs(t["logZ"] - s["logZ"]) <= 1e-12 * abs(s["logZ"]), chunk
        assert np.all(np.abs(t["logZReplicates"] - s["logZReplicates"]) <= 1e-12), chunk
        assert abs(t["ess"] - s["ess"]) <= 1e-10 * s["ess"] and t["nInside"] == N_EVID
        assert np.allclose(t["mean"], s["mean"], rtol=0, atol=1e-11) and np.allclose(t["cov"], s["cov"], rtol=0, atol=1e-11)
        assert abs(t["logZErr"] - s["logZErr"]) <= 1e-6 * s["logZErr"]
    # qmc=None is the call that never mentions qmc
    n = a.evidence(nSamples=N_EVID, proposal="box", seed=SEED, qmc=None)
    assert sorted(n) == sorted(p) and "qmc" not in n
    for key in p:
        assert np.array_equal(np.asarray(n[key]), np.asarray(p[key])), key
    # nSamples that R does not divide: R (nSamples // R) rows are used
    odd = a.evidence(nSamples=4096 + 3, proposal="box", seed=SEED, qmc=4)
    assert odd["nInside"] == 4096 and odd["logZ"] == a.evidence(nSamples=4096, proposal="box", seed=SEED, qmc=4)["logZ"]


def test_evidence_prior_and_mixture_proposals_against_the_quadrature():
    from approxposterior_amd import priors as P
    b = er.QUAD_BOUNDS
    J = P.JointPrior([P.UniformPrior(b[0][0], b[0][1]), P.GaussianPrior(0.5, 1.0)])
    s = _ap(prior=J).evidence(nSamples=N_EVID, proposal="prior", seed=SEED + 1, qmc=QMC)
    logZ = _quad(wide=True)[0]
    print("prior qmc: logZ %.7f +- %.2e (quadrature %.7f, off by %.2f errors), ess %.0f" %
          (s["logZ"], s["logZErr"], logZ, abs(s["logZ"] - logZ) / s["logZErr"], s["ess"]))
    assert s["nInside"] == N_EVID and abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    logZ, mean, cov = _quad1200()
    mix = ([0.6, 0.4], [mean + [0.4, 0.0], mean - [0.5, 0.2]], [1.5 * cov, 2.5 * cov])
    a = _ap()
    s = a.evidence(nSamples=N_EVID, proposal=mix, seed=SEED + 2, qmc=QMC, chunk=2 ** 11)
    print("mixture qmc: logZ %.7f +- %.2e (quadrature %.7f, off by %.2f errors), ess %.0f" %
          (s["logZ"], s["logZErr"], logZ, abs(s["logZ"] - logZ) / s["logZErr"], s["ess"]))
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"] and s["ess"] > 0.2 * N_EVID
    # surrogateDraws rides along on the same rows: the plug-in keys keep their bits
    d = a.evidence(nSamples=4096, proposal=mix, seed=SEED + 2, qmc=4, surrogateDraws=3, nFeatures=256)
    e = a.evidence(nSamples=4096, proposal=mix, seed=SEED + 2, qmc=4)
    assert d["logZ"] == e["logZ"] and d["logZErr"] == e["logZErr"] and d["logZDraws"].shape == (3,)
    assert np.all(np.isfinite(d["logZDraws"]))


# ----------------------------------------------------------------------------------------------------------------------
# candidates of the acquisition sweep, initial designs
# ----------------------------------------------------------------------------------------------------------------------
def test_find_next_point_over_sobol_candidates():
    from approxposterior_amd import utility as ut
    a = _ap()
    m = 4096
    np.random.seed(42)
    point = a.findNextPoint(computeLnLike=False, nCandidates=m, deviceCandidates="sobol", verbose=False, cache=False)
    assert a.deviceCandidates == "sobol"
    np.random.seed(42)
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    T = a.gp.sobol_candidates(m, bounds=a.bounds, seed=seed)
    best = a.gp.acquire(a.y, T, ut.utilityKind(a.utility), bounds=a.bounds)[0]
    assert 0 <= best < m
    assert _same_bits(np.asarray(point), T[best].cpu().numpy())          # the winning row, regenerated alone
    assert _same_bits(np.asarray(point), sr.box(1, *np.asarray(a.bounds).T, seed, offset=best)[0])
    # True still means the Philox stream
    np.random.seed(42)
    philox = a.findNextPoint(computeLnLike=False, nCandidates=m, deviceCandidates=True, verbose=False, cache=False)
    assert a.deviceCandidates is True
    want, _ = ut.sweepObjective(a.utility, a.y, a.gp, a.gp.box_candidates(m, a.bounds, seed).cpu().numpy(), bounds=a.bounds)
    assert np.array_equal(philox, want) and not np.array_equal(philox, point)
    # under a JointPrior the rows come from the prior
    from approxposterior_amd import priors as P
    b = er.QUAD_BOUNDS
    J = P.JointPrior([P.UniformPrior(b[0][0], b[0][1]), P.GaussianPrior(0.5, 1.0)])
    aj = _ap(prior=J)
    np.random.seed(43)
    pj = aj.findNextPoint(computeLnLike=False, nCandidates=m, deviceCandidates="sobol", verbose=False, cache=False)
    np.random.seed(43)
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    Tj = aj.gp.sobol_candidates(m, prior=J, seed=seed).cpu().numpy()
    wj, _ = ut.sweepObjective(aj.utility, aj.y, aj.gp, Tj, bounds=[tuple(r) for r in J.support()])
    assert np.array_equal(pj, wj)


def test_sobol_sample_is_a_seeded_space_filling_design():
    import approxposterior_amd as ap
    from approxposterior_amd import priors as P
    lo, hi, b = _bounds(3)
    X = ap.sobolSample(64, bounds=b, seed=5)
    assert isinstance(X, np.ndarray) and _same_bits(X, sr.box(64, lo, hi, 5))
    np.random.seed(8)
    Y = ap.sobolSample(64, bounds=b)
    np.random.seed(8)
    assert _same_bits(Y, sr.box(64, lo, hi, int(np.random.randint(0, 2 ** 31 - 1))))
    J = P.JointPrior([P.UniformPrior(0.0, 2.0), P.GaussianPrior(1.0, 3.0)])
    Z = ap.sobolSample(128, prior=J, seed=6)
    assert Z.shape == (128, 2) and _same_bits(Z[:, 0], sr.box(128, [0.0, 0.0], [2.0, 1.0], 6)[:, 0])
    # 128 stratified normals: the sample mean is far closer to mu than sigma / sqrt(128) = 0.27
    assert abs(Z[:, 1].mean() - 1.0) < 0.05
