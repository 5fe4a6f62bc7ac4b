"""CPU: approxposterior_amd.priors against scipy.stats and the reference's definitions, JointPrior's closed form, the NumPy
replay of the device's prior candidates (tests/prior_ref.py), the C entries' argument checks with no GPU, klNumerical and
the package's top-level names."""
import numpy as np
import pytest
import scipy.stats as ss
from scipy.special import erfcinv

import prior_ref
from philox_ref import philox_box_numpy


def _priors():
    from approxposterior_amd import priors
    return priors


def _mixed():
    P = _priors()
    return [P.UniformPrior(-2.0, 3.0, theta_name="a"), P.GaussianPrior(1.5, 0.25, theta_name="b"),
            P.GaussianPrior(-40.0, 7.0), P.UniformPrior(10.0, 10.5, theta_name="d"), P.GaussianPrior(0.0, 1.0)]


def test_uniform_prior_values():
    P = _priors()
    u = P.UniformPrior(0.0, 100.0, theta_name="x")
    assert u.lnprior(50.0) == pytest.approx(-np.log(100.0), rel=1e-15)
    assert u(0.0) == u.lnprior(100.0) == pytest.approx(-np.log(100.0), rel=1e-15)
    assert np.isneginf(u.lnprior(-1e-9)) and np.isneginf(u.lnprior(100.0 + 1e-9))
    assert u.transform_uniform(0.25) == 25.0 and u.transform_uniform(0.0) == 0.0 and u.transform_uniform(1.0) == 100.0
    assert u.get_bounds() == (0.0, 100.0)
    assert np.allclose(u.dist.pdf([10.0, 200.0]), [0.01, 0.0])
    assert u.theta_name == "x" and repr(u) == "UniformPrior(low=0.000, high=100.000)"


def test_gaussian_prior_values():
    P = _priors()
    g = P.GaussianPrior(50.0, 10.0)
    assert g.lnprior(50.0) == pytest.approx(-np.log(10.0) - 0.5 * np.log(2 * np.pi), rel=1e-15)
    assert g(70.0) == pytest.approx(-2.0 - np.log(10.0) - 0.5 * np.log(2 * np.pi), rel=1e-15)
    assert g.transform_uniform(0.5) == 50.0
    assert g.transform_uniform(0.975) == pytest.approx(50.0 + 10.0 * ss.norm.ppf(0.975), rel=1e-13)
    r = np.linspace(0.01, 0.99, 17)
    assert np.array_equal(g.transform_uniform(r), 50.0 + 10.0 * np.sqrt(2.0) * erfcinv(2.0 * (1.0 - r)))
    assert g.get_bounds() == pytest.approx((0.0, 100.0), abs=1e-12)
    assert g.get_bounds(Nstd=2.0) == pytest.approx((30.0, 70.0), abs=1e-12)
    assert g.theta_name is None and repr(g) == "GaussianPrior(mu=50.000, sigma=10.000)"


def test_list_utilities():
    P = _priors()
    pri = _mixed()
    theta = [0.5, 1.7, -38.0, 10.2, 0.3]
    want = ss.uniform(-2.0, 5.0).logpdf(0.5) + ss.norm(1.5, 0.25).logpdf(1.7) \
        + ss.norm(-40.0, 7.0).logpdf(-38.0) + ss.uniform(10.0, 0.5).logpdf(10.2) + ss.norm(0, 1).logpdf(0.3)
    assert P.get_lnprior(theta, pri) == pytest.approx(want, rel=1e-14)
    with pytest.raises(AssertionError):
        P.get_lnprior(theta[:4], pri)
    cube = np.array([0.5, 0.5, 0.5, 0.2, 0.8413447460685429])
    out = P.get_prior_unit_cube(cube, pri)
    assert out is cube
    assert np.allclose(out, [0.5, 1.5, -40.0, 10.1, 1.0], rtol=1e-12, atol=1e-12)
    b = P.get_theta_bounds(pri)
    assert b[0] == (-2.0, 3.0) and b[3] == (10.0, 10.5)
    assert b[1] == pytest.approx((1.5 - 1.25, 1.5 + 1.25)) and b[2] == pytest.approx((-75.0, -5.0))
    assert P.get_theta_names(pri) == ["a", "b", None, "d", None]


def test_random_sample_uses_the_global_random_state():
    P = _priors()
    u, g = P.UniformPrior(-1.0, 4.0), P.GaussianPrior(2.0, 3.0)
    np.random.seed(11)
    a, b, c = u.random_sample(1000), g.random_sample(1000), g.random_sample()
    np.random.seed(11)
    assert np.array_equal(a, ss.uniform(-1.0, 5.0).rvs(size=1000))
    assert np.array_equal(b, ss.norm(2.0, 3.0).rvs(size=1000))
    assert c == ss.norm(2.0, 3.0).rvs() and np.ndim(c) == 0
    np.random.seed(11)
    assert np.array_equal(a, -1.0 + 5.0 * np.random.uniform(size=1000))


def test_base_prior_raises():
    P = _priors()
    p = P.Prior(theta_name="t")
    assert p.theta_name == "t"
    for call in (lambda: p.lnprior(0.0), lambda: p(0.0), lambda: p.random_sample(3), lambda: p.transform_uniform(0.5),
                 p.get_bounds):
        with pytest.raises(NotImplementedError):
            call()


def test_joint_prior_batch_matches_get_lnprior():
    P = _priors()
    pri = _mixed()
    J = P.JointPrior(pri)
    rs = np.random.RandomState(3)
    lo = np.array([-2.0, 0.0, -70.0, 10.0, -4.0])
    hi = np.array([3.0, 3.0, -10.0, 10.5, 4.0])
    pts = lo - 0.3 * (hi - lo) + 1.6 * (hi - lo) * rs.uniform(size=(4000, 5))      # about half outside the Uniform faces
    faces = np.tile([0.5, 1.5, -40.0, 10.25, 0.0], (8, 1))
    faces[0, 0], faces[1, 0], faces[2, 3], faces[3, 3] = -2.0, 3.0, 10.0, 10.5    # exactly on the faces: inside
    faces[4, 0], faces[5, 3] = np.nextafter(-2.0, -3.0), 10.5 + 1e-9               # just outside
    faces[6, 0], faces[7, 3] = -2.0, 10.0
    faces[6, 3], faces[7, 0] = 10.5, 3.0
    bad = np.tile([0.5, 1.5, -40.0, 10.25, 0.0], (6, 1))
    bad[0, 1], bad[1, 2], bad[2, 0], bad[3, 4], bad[4, 3], bad[5, 1] = np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan
    allp = np.vstack([pts, faces, bad])
    got = J.batch(allp)
    with np.errstate(invalid="ignore"):
        want = np.array([P.get_lnprior(p, pri) for p in allp])
    assert got.shape == (len(allp),)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    assert not np.any(np.isnan(got)) and np.all(np.isneginf(got[~np.isfinite(want)]))
    f = np.isfinite(want)
    assert np.all(np.abs(got[f] - want[f]) <= 1e-12 * (1.0 + np.abs(want[f])))
    assert 1000 < f[:4000].sum() < 3000
    assert np.all(np.isfinite(got[4000:4004])) and np.all(np.isfinite(got[4006:4008]))
    assert np.all(np.isneginf(got[4004:4006])) and np.all(np.isneginf(got[-6:]))
    assert J(allp[0]) == P.get_lnprior(allp[0], pri)


def test_joint_prior_sample_support_bounds():
    P = _priors()
    pri = _mixed()
    J = P.JointPrior(pri)
    np.random.seed(5)
    s = J.sample(2000)
    np.random.seed(5)
    want = np.vstack([p.random_sample(2000) for p in pri]).T
    assert s.shape == (2000, 5) and np.array_equal(s, want)
    sup = J.support()
    assert sup.shape == (5, 2)
    assert np.array_equal(sup, [[-2.0, 3.0], [-np.inf, np.inf], [-np.inf, np.inf], [10.0, 10.5], [-np.inf, np.inf]])
    assert J.bounds() == P.get_theta_bounds(pri)
    kind, p0, p1 = J.records()
    assert kind.dtype == np.int32 and list(kind) == [0, 1, 1, 0, 1]
    assert list(p0) == [-2.0, 1.5, -40.0, 10.0, 0.0] and list(p1) == [3.0, 0.25, 7.0, 10.5, 1.0]


def test_joint_prior_refusals():
    P = _priors()
    with pytest.raises(TypeError):
        P.JointPrior([P.UniformPrior(0, 1), P.Prior()])
    with pytest.raises(TypeError):
        P.JointPrior([lambda x: 0.0])
    for bad in ([P.UniformPrior(1.0, 1.0)], [P.UniformPrior(2.0, 1.0)], [P.UniformPrior(-np.inf, 1.0)],
                [P.UniformPrior(0.0, np.nan)], [P.GaussianPrior(0.0, 0.0)], [P.GaussianPrior(0.0, -1.0)],
                [P.GaussianPrior(0.0, np.inf)], [P.GaussianPrior(np.nan, 1.0)], [P.GaussianPrior(np.inf, 1.0)], []):
        with pytest.raises(ValueError):
            P.JointPrior(bad)


def test_replay_of_uniform_only_priors_is_the_box_stream():
    P = _priors()
    for D in (1, 2, 3, 7, 8, 32):
        lo = -1.0 - 0.5 * np.arange(D)
        hi = 2.0 + 0.25 * np.arange(D)
        J = P.JointPrior([P.UniformPrior(a, b) for a, b in zip(lo, hi)])
        for seed, off in ((7, 0), (2 ** 40 + 3, 2 ** 33 + 11)):
            rep = prior_ref.prior_candidates_numpy(300, *J.records(), seed, off, fused=False)
            assert np.array_equal(rep, philox_box_numpy(300, D, lo, hi, seed, off))
            fused = prior_ref.prior_candidates_numpy(300, *J.records(), seed, off)
            assert np.all(np.abs(fused - rep) <= np.spacing(np.abs(lo) + np.abs(hi)))      # (one rounding fewer)


def test_replay_gaussian_columns_are_transform_uniform():
    P = _priors()
    pri = _mixed()
    J = P.JointPrior(pri)
    rep = prior_ref.prior_candidates_numpy(500, *J.records(), 99, 1000)
    u = prior_ref.uniforms(500, 5, 99, 1000)
    for d in (1, 2, 4):
        assert np.array_equal(rep[:, d], pri[d].transform_uniform(u[:, d]))
    assert np.all((rep[:, 0] >= -2.0) & (rep[:, 0] <= 3.0)) and np.all((rep[:, 3] >= 10.0) & (rep[:, 3] <= 10.5))
    # rows do not depend on the shard they are drawn in
    assert np.array_equal(rep[100:], prior_ref.prior_candidates_numpy(400, *J.records(), 99, 1100))


def test_prior_entries_refuse_bad_arguments_without_a_gpu():
    """Every call below fails an argument check before anything reaches the device (m is 0 or negative throughout)."""
    from approxposterior_amd import _lib
    lib = _lib.load()
    D = 3
    T = np.zeros((4, D))
    out = np.zeros(4)

    def recs(kind=(0, 1, 0), p0=(0.0, 1.0, -1.0), p1=(1.0, 2.0, 5.0)):
        return (np.array(kind, dtype=np.int32), np.array(p0, dtype=np.float64), np.array(p1, dtype=np.float64))

    def cand(m=0, ndim=D, r=None, null=None, off=0):
        k, a, b = recs() if r is None else r
        ptrs = [T.ctypes.data, k.ctypes.data, a.ctypes.data, b.ctypes.data]
        if null is not None:
            ptrs[null] = None
        return lib.apgp_prior_candidates(ptrs[0], m, ndim, ptrs[1], ptrs[2], ptrs[3], 5, off, None)

    def lnp(m=0, ndim=D, r=None, null=None):
        k, a, b = recs() if r is None else r
        ptrs = [T.ctypes.data, k.ctypes.data, a.ctypes.data, b.ctypes.data, out.ctypes.data]
        if null is not None:
            ptrs[null] = None
        return lib.apgp_prior_lnprior(ptrs[0], m, ndim, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)

    assert cand() == 0 and lnp() == 0                    # the baseline is valid (and m = 0 launches nothing)
    for i in range(4):
        assert cand(null=i) == -1 and b"null pointer" in lib.apgp_last_error()
    for i in range(5):
        assert lnp(null=i) == -1 and b"null pointer" in lib.apgp_last_error()
    bad_records = [
        (dict(kind=(0, 2, 0)), b"kind"), (dict(kind=(-1, 1, 0)), b"kind"),
        (dict(p1=(1.0, 0.0, 5.0)), b"sigma"), (dict(p1=(1.0, -2.0, 5.0)), b"sigma"),
        (dict(p1=(1.0, np.nan, 5.0)), b"sigma"), (dict(p1=(1.0, np.inf, 5.0)), b"sigma"),
        (dict(p0=(0.0, np.inf, -1.0)), b"sigma"), (dict(p0=(0.0, np.nan, -1.0)), b"sigma"),
        (dict(p0=(1.0, 1.0, -1.0)), b"low < high"), (dict(p0=(2.0, 1.0, -1.0)), b"low < high"),
        (dict(p0=(0.0, 1.0, -np.inf)), b"low < high"), (dict(p1=(np.inf, 2.0, 5.0)), b"low < high"),
        (dict(p0=(np.nan, 1.0, -1.0)), b"low < high"), (dict(p0=(-1e308, 1.0, -1.0), p1=(1e308, 2.0, 5.0)), b"low < high"),
    ]
    for kw, msg in bad_records:
        r = recs(**kw)
        assert cand(r=r) == -1 and msg in lib.apgp_last_error(), kw
        assert lnp(r=r) == -1 and msg in lib.apgp_last_error(), kw
    for nd in (0, -1, 33):
        assert cand(ndim=nd) == -1 and b"ndim" in lib.apgp_last_error()
        assert lnp(ndim=nd) == -1 and b"ndim" in lib.apgp_last_error()
    assert cand(m=-1) == -1 and cand(off=-1) == -1 and lnp(m=-1) == -1
    # the records are only read for the first ndim dimensions
    assert cand(ndim=2, r=recs(kind=(0, 1, 7))) == 0 and lnp(ndim=2, r=recs(kind=(0, 1, 7))) == 0


def test_kl_numerical_known_answer():
    """The reference's test_KL restated: seed 57, two unit normals 2.4 apart, 1e4 samples from p; the Monte Carlo
    estimate is within 0.5 % of scipy.stats.entropy on a grid."""
    from approxposterior_amd import utility as ut
    np.random.seed(57)
    x = np.linspace(-5, 5, 1000)
    exact = ss.entropy(ss.norm.pdf(x, loc=1.2, scale=1), ss.norm.pdf(x, loc=-1.2, scale=1))
    samples = ss.norm.rvs(loc=1.2, scale=1, size=10000)
    est = ut.klNumerical(samples, lambda v: ss.norm.pdf(v, loc=1.2, scale=1), lambda v: ss.norm.pdf(v, loc=-1.2, scale=1))
    assert 100 * abs((exact - est) / exact) < 0.5

    def boom(v):
        raise ValueError("math domain error")
    with pytest.raises(ValueError, match=r"ERROR: inf/NaN encountered\.  q\(x\) = 0 likely occured\."):
        ut.klNumerical(samples, boom, boom)


REFERENCE_NAMES = [
    "ApproxPosterior",
    "logsubexp", "AGPUtility", "BAPEUtility", "JonesUtility", "minimizeObjective", "klNumerical",
    "rosenbrockLnlike", "rosenbrockLnprior", "rosenbrockSample", "rosenbrockLnprob", "testBOFn", "testBOFnSample",
    "testBOFnLnPrior", "sphereLnlike", "sphereSample", "sphereLnprior",
    "defaultHyperPrior", "defaultGP", "optimizeGP",
    "validateMCMCKwargs", "batchMeansMCSE", "estimateBurnin",
    "fitGMM",
    "Prior", "UniformPrior", "GaussianPrior", "get_lnprior", "get_prior_unit_cube", "get_theta_bounds", "get_theta_names",
]


def test_every_reference_name_is_importable_from_the_package():
    import approxposterior_amd
    ns = {}
    exec("from approxposterior_amd import *", ns)
    missing = [n for n in REFERENCE_NAMES if n not in ns]
    assert not missing, missing
    from approxposterior_amd import priors, utility, likelihood
    assert approxposterior_amd.JointPrior is priors.JointPrior and "JointPrior" in ns
    assert approxposterior_amd.klNumerical is utility.klNumerical
    assert approxposterior_amd.rosenbrockLnlike is likelihood.rosenbrockLnlike
    from approxposterior_amd.priors import (Prior, UniformPrior, GaussianPrior, get_lnprior,  # noqa: F401
                                            get_prior_unit_cube, get_theta_bounds, get_theta_names)
