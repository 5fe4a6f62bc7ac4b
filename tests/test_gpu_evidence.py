# -*- coding: utf-8 -*-
"""GPU (``-m gpu``): ApproxPosterior.evidence end to end on the D = 2, N = 60 quadratic case of tests/evidence_ref.py,
against the CPU restatement's number and a 400 x 400 quadrature of exp(mu)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_ref as er  # noqa: E402
from test_evidence_ref import box_estimate  # noqa: E402

pytestmark = pytest.mark.gpu

M = er.EVIDENCE_M
SEED = er.EVIDENCE_SEED


def _ap(prior=None):
    import approxposterior_amd as ap
    from approxposterior_amd import gp as agp
    X, y, metric, mean, wn = er.quadratic_case()
    g = agp.GP(kernel=agp.ExpSquaredKernel(metric, ndim=2), fit_mean=True, mean=mean, white_noise=wn,
               fit_white_noise=False)
    g.compute(X)
    b = np.asarray(er.QUAD_BOUNDS)
    inside = lambda t: bool(np.all((np.asarray(t) >= b[:, 0]) & (np.asarray(t) <= b[:, 1])))      # noqa: E731
    lnprior = prior if prior is not None else (lambda t: 0.0 if inside(t) else -np.inf)
    sample = lambda n=1: b[:, 0] + (b[:, 1] - b[:, 0]) * np.random.uniform(size=(n, 2))         # noqa: E731
    return ap.ApproxPosterior(theta=X, y=y, lnprior=lnprior, lnlike=lambda t: 0.0, priorSample=sample,
                              bounds=er.QUAD_BOUNDS, gp=g)


@functools.lru_cache(maxsize=None)
def _quad(wide=False):
    """The quadrature over the box; ``wide``: the second dimension out to 5 sigma of the Gaussian prior factor N(0.5, 1),
    all a proposal of 2^16 draws from it can reach (6e-7 of its mass lies beyond)."""
    return er.quadrature(er.quadratic_case(), bounds=[er.QUAD_BOUNDS[0], (-4.5, 5.5)] if wide else None)


def _moments_ok(s, mean, cov):
    """mean and cov within 5 importance-sampling standard errors: se(mean_d) = sqrt(C_dd / ess), se(C_de) =
    sqrt((C_dd C_ee + C_de^2) / ess) (the Gaussian fourth moment; the posterior here is close to one)."""
    se_m = np.sqrt(np.diag(cov) / s["ess"])
    se_c = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / s["ess"])
    assert np.all(np.abs(s["mean"] - mean) <= 5.0 * se_m), (s["mean"], mean, se_m)
    assert np.all(np.abs(s["cov"] - cov) <= 5.0 * se_c), (s["cov"], cov, se_c)


def test_box_proposal_reproduces_the_cpu_number_and_does_not_depend_on_the_chunk():
    from approxposterior_amd import utility as ut
    a = _ap()
    s = a.evidence(nSamples=M, proposal="box", seed=SEED, chunk=M)
    rec, logV, row_budget = box_estimate()
    ref = ut.importanceSummary(rec, M, logVolume=logV)
    # the record budget on S0 (m u relative on the sum plus the exp's ulps per row: together below 2 m u) and the rows'
    # own logw error, which moves log S0 by at most its largest value (the per-row budget of test_gpu_importance.py)
    tol = 2.0 * M * 2.0 ** -53 + row_budget
    print("box: logZ %.12f (cpu %.12f, diff %.2e, tol %.2e) +- %.6f ess %.0f" %
          (s["logZ"], ref["logZ"], abs(s["logZ"] - ref["logZ"]), tol, s["logZErr"], s["ess"]))
    assert abs(s["logZ"] - ref["logZ"]) <= tol
    assert abs(s["ess"] - ref["ess"]) <= 1e-9 * ref["ess"] and s["nInside"] == M
    logZ, mean, cov = _quad()
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    _moments_ok(s, mean, cov)
    for chunk in (2 ** 13, 12345):
        t = a.evidence(nSamples=M, proposal="box", seed=SEED, chunk=chunk)
        assert abs(t["logZ"] - s["logZ"]) <= 1e-12 * abs(s["logZ"]), chunk
        assert abs(t["ess"] - s["ess"]) <= 1e-10 * s["ess"] and t["nInside"] == M
        assert np.allclose(t["mean"], s["mean"], rtol=0, atol=1e-11) and np.allclose(t["cov"], s["cov"], rtol=0, atol=1e-11)
    # seed=None draws one from NumPy's global stream: the same stream state, the same estimate
    np.random.seed(4)
    u1 = a.evidence(nSamples=4096, proposal="box")
    np.random.seed(4)
    u2 = a.evidence(nSamples=4096, proposal="box")
    assert u1["logZ"] == u2["logZ"] and u1["logZ"] != s["logZ"]


def test_prior_proposal_under_a_joint_prior_with_a_gaussian_factor():
    from approxposterior_amd import priors as P
    b = er.QUAD_BOUNDS
    J = P.JointPrior([P.UniformPrior(b[0][0], b[0][1]), P.GaussianPrior(0.5, 1.0)])
    a = _ap(prior=J)
    s = a.evidence(nSamples=M, proposal="prior", seed=SEED + 1)
    # the gate is the prior's support: the Gaussian dimension is unbounded, and the estimate sees what the draws reach
    logZ, mean, cov = _quad(wide=True)
    print("prior: logZ %.6f +- %.6f (quadrature %.6f), ess %.0f, inside %d" % (s["logZ"], s["logZErr"], logZ, s["ess"], s["nInside"]))
    assert s["nInside"] == M and s["ess"] > 1000
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    _moments_ok(s, mean, cov)


def test_mixture_proposal():
    a = _ap()
    logZ, mean, cov = _quad()
    mix = ([0.6, 0.4], [mean + [0.4, 0.0], mean - [0.5, 0.2]], [1.5 * cov, 2.5 * cov])
    s = a.evidence(nSamples=M, proposal=mix, seed=SEED + 2, chunk=2 ** 14)
    print("mixture: logZ %.6f +- %.6f (quadrature %.6f), ess %.0f, inside %d" % (s["logZ"], s["logZErr"], logZ, s["ess"], s["nInside"]))
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"] and s["ess"] > 0.2 * M
    _moments_ok(s, mean, cov)

    class Fitted(object):
        weights_, means_, covariances_, covariance_type = np.array(mix[0]), np.array(mix[1]), np.array(mix[2]), "full"
    t = a.evidence(nSamples=M, proposal=Fitted(), seed=SEED + 2, chunk=2 ** 14)
    assert t["logZ"] == s["logZ"] and np.array_equal(t["cov"], s["cov"])
    wide = a.evidence(nSamples=M, proposal=mix, seed=SEED + 2, covScale=2.0)
    assert abs(wide["logZ"] - logZ) <= 4.0 * wide["logZErr"] and wide["ess"] < s["ess"]


def test_error_paths():
    a = _ap()
    with pytest.raises(ValueError, match="JointPrior"):
        a.evidence(nSamples=64, proposal="prior")
    with pytest.raises(ValueError, match="runMCMC"):
        a.evidence(nSamples=64, proposal="gmm")

    class Diag(object):
        weights_, means_, covariances_, covariance_type = np.ones(1), np.zeros((1, 2)), np.ones((1, 2)), "diag"
    with pytest.raises(ValueError, match="full"):
        a.evidence(nSamples=64, proposal=Diag())
    with pytest.raises(ValueError):
        a.evidence(nSamples=64, proposal="nested")
    with pytest.raises(ValueError):
        a.evidence(nSamples=0, proposal="box")


def test_gmm_proposal_fitted_to_samples():
    pytest.importorskip("sklearn")
    a = _ap()
    logZ, mean, cov = _quad()
    samples = np.random.RandomState(8).multivariate_normal(mean, cov, size=4000)
    s = a.evidence(nSamples=M, proposal="gmm", samples=samples, seed=SEED + 3, maxComp=2, covScale=1.5)
    print("gmm: logZ %.6f +- %.6f (quadrature %.6f), ess %.0f" % (s["logZ"], s["logZErr"], logZ, s["ess"]))
    assert abs(s["logZ"] - logZ) <= 4.0 * s["logZErr"]
    _moments_ok(s, mean, cov)
