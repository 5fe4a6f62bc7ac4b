"""GPU parity tests (run with ``-m gpu`` on an MI355X): the HIP path, called
through the C ABI (libapgp.so via ctypes, approxposterior_amd.gp.GP), against

  * the committed golden fixtures (tests/golden/*.npz) that the REFERENCE's own
    utility.py / gpUtils.py produced one candidate at a time (oracle/make_golden.py);
  * the NumPy oracle (oracle/george_oracle.py) on seeded inputs at sizes it
    finishes in seconds;
  * size-independent properties at the BASELINE.json sizes (exact-interpolation
    at training points, invariance of the arg-min to sharding/permutation).

Tolerances (all arithmetic is IEEE fp64): the achievable
agreement between two correct fp64 implementations scales with cond(K):
    mu  : |d| <= 200 * cond * eps * (|mu - mean| + sum|k*_n alpha_n| bound)
    var : |d| <= 200 * cond * eps * amp        (absolute, amp = k(t,t))
    u   : follows from mu / var through the utility's own conditioning
with eps = 2.2e-16.  For the well-conditioned BASELINE synthetic configs
(cond ~ 1e1..1e3) that is ~1e-12 relative; the fixtures' worst case
(c2small, cond 4.7e6) gives ~2e-7 * amp.
"""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
FIXTURES = ["rosen2d_n50_noamp", "rosen2d_n50_amp", "rosen2d_n50_noamp_opt",
            "c2small_d2_n200", "c3small_d8_n300", "d5_n130_amp", "bo1d_n12_amp"]


def _mods():
    import george_oracle as go
    from approxposterior_amd import gp as agp
    return go, agp


def build(mod, g):
    D = g["theta"].shape[1]
    p = g["p"]
    if int(g["fit_amp"]):
        k = mod.Product(mod.ConstantKernel(p[1], ndim=D), mod.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    else:
        k = mod.ExpSquaredKernel(np.exp(p[1:]), ndim=D)
    gp = mod.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]),
                fit_white_noise=False)
    gp.compute(g["theta"])
    return gp


def amp_of(g):
    D = g["theta"].shape[1]
    return D * np.exp(g["p"][1]) if int(g["fit_amp"]) else 1.0


def same_nonfinite(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and
            np.array_equal(np.isposinf(a), np.isposinf(b)) and
            np.array_equal(np.isneginf(a), np.isneginf(b)))


@pytest.fixture(scope="module")
def lib_loaded():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_abi_version() == _lib.ABI_VERSION
    return lib


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fit_quantities(golden_dir, name, lib_loaded):
    """K1 gram + potrf + K2 logdet + K3 solves vs the reference fixtures."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gp = build(agp, g)
    tol = 200 * g["cond"] * EPS
    assert gp.computed
    assert np.isclose(gp.log_determinant, g["logdet"], rtol=1e-11, atol=1e-9)
    ll = gp.log_likelihood(g["y"], quiet=True)
    assert np.isclose(ll, g["ll"], rtol=max(1e-11, tol))
    gp._solve(g["y"], need_alpha=True)
    alpha = gp._alpha.cpu().numpy()
    assert np.abs(alpha - g["alpha"]).max() <= max(1e-12, tol) * np.abs(g["alpha"]).max()
    # condition estimate from the Cholesky diagonal is a lower bound within ~N of cond
    assert gp.cond_estimate <= g["cond"] * 1.01


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_predict_and_utilities(golden_dir, name, lib_loaded):
    """K5 sweep (mu, var, AGP/BAPE/Jones) + K6 arg-min vs the per-candidate
    outputs of the reference's utility.py (test_GPUtil.py style, rtol there 1e-4)."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gp = build(agp, g)
    y, cands = g["y"], g["cands"]
    amp = amp_of(g)
    tol = 200 * g["cond"] * EPS
    mu, var = gp.predict(y, cands, return_var=True)
    mu_only = gp.predict(y, cands, return_cov=False, return_var=False)
    scale = np.abs(g["alpha"]).sum() * amp
    assert np.abs(mu - g["mu"]).max() <= max(1e-13, tol) * scale
    assert np.abs(mu_only - g["mu"]).max() <= max(1e-13, tol) * scale
    assert np.abs(var - g["var"]).max() <= max(1e-14, tol) * amp
    bounds = list(zip(g["lo"], g["hi"]))
    for kind, key in (("agp", "u_agp"), ("bape", "u_bape"), ("jones", "u_jones")):
        bi, bu, u, m2, v2 = gp.acquire(y, cands, kind, bounds=bounds, return_all=True)
        ref = g[key]
        assert same_nonfinite(u, ref), kind
        fin = np.isfinite(ref)
        # propagate the mu / var tolerances through each utility's own derivative:
        #   AGP   |du| <= |dmu| + 0.5 |dvar| / var
        #   BAPE  |du| <= 2 |dmu| + |dvar| (1 + 1/(e^var - 1))
        #   Jones |du| <= Phi |dmu| + phi |dvar| / (2 sqrt(var)) <= |dmu| + 0.2 |dvar| / sqrt(var)
        tmu = max(1e-13, tol) * scale
        tvar = max(1e-14, tol) * amp
        vr = np.maximum(g["var"][fin], 1e-300)
        if kind == "agp":
            tu = tmu + 0.5 * tvar / vr
        elif kind == "bape":
            tu = 2 * tmu + tvar * (1.0 + 1.0 / np.expm1(vr))
        else:
            tu = tmu + 0.2 * tvar / np.sqrt(vr)
        err = np.abs(u[fin] - ref[fin])
        assert (err <= 4 * tu + 1e-11 * np.abs(ref[fin])).all(), (kind, float((err / tu).max()))
        # reference-test tolerance (test_GPUtil.py: rtol 1e-4) holds with a wide margin
        refm = np.where(np.isnan(ref), np.inf, ref)
        assert np.allclose(u[fin], ref[fin], rtol=1e-4, atol=1e-9 * amp)
        # arg-min: same winner, or a tie within tolerance
        if np.isfinite(refm).any():
            ri = int(np.argmin(refm))
            assert bi == ri or abs(refm[bi] - refm[ri]) <= 1e-9 * max(1.0, abs(refm[ri]))
            assert np.isclose(bu, u[bi])
        else:
            assert bi == -1


@pytest.mark.parametrize("name", ["rosen2d_n50_noamp", "rosen2d_n50_amp", "d5_n130_amp", "c3small_d8_n300"])
def test_fixture_gradient(golden_dir, name, lib_loaded):
    """K4 gradient vs the oracle's grad_log_likelihood (itself FD-checked; the
    reference has no known-answer test for the gradient: 'parity unpinned')."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gp = build(agp, g)
    grad = gp.grad_log_likelihood(g["y"], quiet=True)
    tol = max(1e-11, 500 * g["cond"] * EPS)
    assert np.allclose(grad, g["grad"], rtol=tol, atol=tol * np.abs(g["grad"]).max())


def test_fit_white_noise_protocol_and_gradient(lib_loaded):
    """george's fit_white_noise=True (the reference's defaultGP fixes it to False,
    gpUtils.py:176-177, but the GP boundary accepts such an object): the white-noise
    parameter sits between the mean and the kernel parameters, likelihood and gradient
    follow the oracle (whose white-noise derivative is finite-difference checked in the
    CPU suite)."""
    go, agp = _mods()
    rs = np.random.RandomState(11)
    X = rs.uniform(-3, 3, size=(150, 3))
    y = np.sin(X).sum(axis=1) + 0.05 * rs.normal(size=150)
    def make(mod):
        k = 2.0 * mod.ExpSquaredKernel(np.array([1.5, 0.7, 2.0]), ndim=3)
        return mod.GP(kernel=k, fit_mean=True, mean=0.1, white_noise=np.log(2.5e-3), fit_white_noise=True)
    gpo, gp = make(go), make(agp)
    assert gp.get_parameter_names() == gpo.get_parameter_names()
    assert gp.get_parameter_names()[1] == "white_noise:value" and len(gp) == 6
    gpo.compute(X); gp.compute(X)
    assert abs(gp.log_likelihood(y) - gpo.log_likelihood(y)) <= 1e-10 * abs(gpo.log_likelihood(y))
    g, go_ = gp.grad_log_likelihood(y), gpo.grad_log_likelihood(y)
    assert np.allclose(g, go_, rtol=1e-9, atol=1e-9 * np.abs(go_).max())
    p = gp.get_parameter_vector(); p[1] += 0.7
    gp.set_parameter_vector(p); gpo.set_parameter_vector(p)
    assert not gp.computed
    assert abs(gp.log_likelihood(y) - gpo.log_likelihood(y)) <= 1e-10 * abs(gpo.log_likelihood(y))
    assert np.allclose(gp.grad_log_likelihood(y), gpo.grad_log_likelihood(y), rtol=1e-9, atol=1e-9 * np.abs(go_).max())


@pytest.mark.parametrize("order,fit_amp,n,d", [(1, False, 150, 3), (2, True, 150, 3), (1, True, 700, 8), (0, False, 60, 2)])
def test_linear_kernel_term_parity(order, fit_amp, n, d, lib_loaded):
    """defaultGP(order=...): ExpSquared [x amplitude] + c * LinearKernel (gpUtils.py:167-173)
    through every device kernel that evaluates k(x,x') -- Gram/Cholesky (ll), K4 (gradient incl.
    the two linear-term parameters), the sweep (mu, sigma^2 with the candidate-dependent k(t,t),
    utilities, arg-min), the solve-based sweep, the mean-only kernel and the cross kernel of the
    incremental factor extension -- against the oracle (the reference has no test with order !=
    None: 'parity unpinned', see oracle LinearKernel)."""
    go, agp = _mods()
    rs = np.random.RandomState(20 + order)
    X = rs.uniform(-2, 2, size=(n, d))
    y = X[:, 0] - 0.5 * X[:, 1] + np.sin(X).sum(axis=1) + 0.01 * rs.normal(size=n)
    def make(mod):
        k = mod.ExpSquaredKernel(np.linspace(0.8, 2.0, d), ndim=d)
        if fit_amp:
            k = 2.0 * k
        k = k + 0.3 * mod.kernels.LinearKernel(log_gamma2=0.4, order=order, bounds=None, ndim=d)
        return mod.GP(kernel=k, fit_mean=True, mean=0.1, white_noise=-8.0, fit_white_noise=False)
    gpo, gp = make(go), make(agp)
    gpo.compute(X); gp.compute(X)
    llo = gpo.log_likelihood(y)
    cond = np.linalg.cond(gpo.kernel.get_value(X) + np.exp(-8.0) * np.eye(n))
    tol = max(1e-11, 500 * cond * EPS)
    assert abs(gp.log_likelihood(y) - llo) <= tol * abs(llo)
    g0 = gpo.grad_log_likelihood(y)
    for mode in (None, "solve"):            # ("solve": K^-1 by apgp_kinv_solve, the route above the conditioning gate)
        gp.variance_mode = mode
        try:
            g = gp.grad_log_likelihood(y)
        finally:
            gp.variance_mode = None
        assert np.allclose(g, g0, rtol=tol, atol=tol * np.abs(g0).max())
    T = rs.uniform(-2.2, 2.2, size=(333, d))
    mo, vo = gpo.predict(y, T, return_var=True)
    scale = np.abs(gpo.kernel.get_value(T, diag=True)).max()
    for mode in ("inverse", "solve"):
        gp.variance_mode = mode
        try:
            mu, var = gp.predict(y, T, return_var=True)
        finally:
            gp.variance_mode = None
        assert np.abs(mu - mo).max() <= tol * max(1.0, np.abs(mo).max()) * 10
        assert np.abs(var - vo).max() <= tol * scale * 10
    assert np.abs(gp.predict(y, T, return_cov=False) - mo).max() <= tol * max(1.0, np.abs(mo).max()) * 10
    bi, bu, u, _, _ = gp.acquire(y, T, "agp", bounds=[(-2, 2)] * d, return_all=True)
    uo = -(mo + 0.5 * np.log(2 * np.pi * np.e * vo))
    uo[np.any(np.abs(T) > 2, axis=1)] = np.inf
    fin = np.isfinite(uo)
    assert np.array_equal(np.isfinite(u), fin) and np.abs(u[fin] - uo[fin]).max() <= 1e-6 * np.abs(uo[fin]).max()
    assert bi == int(np.argmin(np.where(np.isfinite(u), u, np.inf)))
    # the on-device ensemble sampler evaluates the same mean (log-probability of its final state)
    res = gp.sample_ensemble(y, rs.uniform(-1, 1, size=(4 * d, d)), 40, [(-2, 2)] * d, seed=9)
    assert np.abs(res["final_log_prob"] - gpo.predict(y, res["coords"], return_cov=False)).max() \
        <= tol * max(1.0, np.abs(mo).max()) * 10
    # incremental extension (kernel_cross) with the linear term
    Xn = np.vstack([X, rs.uniform(-2, 2, size=(3, d))])
    yn = np.concatenate([y, [0.3, -0.2, 0.9]])
    gp2, gpo2 = make(agp), make(go)
    gp2.compute(Xn, previous=gp); gpo2.compute(Xn)
    assert abs(gp2.log_likelihood(yn) - gpo2.log_likelihood(yn)) <= 10 * tol * abs(gpo2.log_likelihood(yn))


def test_reference_known_answers(golden_dir, lib_loaded):
    """The reference's own known-answer constants (test_InitGP.py:43,76;
    test_GPUtil.py:50-62,101-113) through the HIP-backed defaultGP + utilities."""
    from approxposterior_amd import gpUtils, utility as ut, likelihood as lh
    pins = json.load(open(os.path.join(golden_dir, "pins.json")))
    c = pins["reference_test_constants"]
    tt = np.array(c["theta_test"])
    for amp, k_init, keys in ((True, "test_InitGP.py:43", ("test_GPUtil.py:50", "test_GPUtil.py:56", "test_GPUtil.py:62")),
                              (False, "test_InitGP.py:76", ("test_GPUtil.py:101", "test_GPUtil.py:107", "test_GPUtil.py:113"))):
        np.random.seed(57)
        theta = np.array(lh.rosenbrockSample(50))
        y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
        gp = gpUtils.defaultGP(theta, y, fitAmp=amp)
        assert np.allclose(c[k_init], gp.get_parameter_vector())
        np.random.seed(57)
        theta = np.array(lh.rosenbrockSample(20))
        y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
        gp = gpUtils.defaultGP(theta, y, fitAmp=amp)
        got = (ut.AGPUtility(tt, y, gp, lh.rosenbrockLnprior),
               ut.BAPEUtility(tt, y, gp, lh.rosenbrockLnprior),
               ut.JonesUtility(tt, y, gp, lh.rosenbrockLnprior))
        for gv, k in zip(got, keys):
            assert np.allclose(gv, c[k], rtol=1.0e-4), (amp, k, gv, c[k])


def test_gpll_guards(golden_dir, lib_loaded):
    """ApproxPosterior._gpll guard cases (approx.py:148-189) vs the harness replay."""
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    pins = json.load(open(os.path.join(golden_dir, "pins.json")))
    for tag, amp in (("amp", True), ("noamp", False)):
        np.random.seed(57)
        theta = np.array(list(lh.rosenbrockSample(50)) + [[-5, 5], [5, 5]])
        y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
        gp = gpUtils.defaultGP(theta, y, fitAmp=amp)
        ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior,
                                    lnlike=lh.rosenbrockLnlike, priorSample=lh.rosenbrockSample,
                                    bounds=((-5, 5), (-5, 5)), algorithm="bape")
        for case in pins["harness_replay"]["gpll_" + tag]:
            t = np.array([float(v) for v in case["theta_repr"]])
            want = [float(v) for v in case["out"]]
            with np.errstate(all="ignore"):
                got = ap._gpll(t)
            got = [float(np.ravel(v)[0]) for v in got]
            for a_, b_ in zip(got, want):
                if np.isnan(b_):
                    assert np.isnan(a_)
                elif np.isinf(b_):
                    assert a_ == b_
                else:
                    assert np.isclose(a_, b_, rtol=1e-8, atol=1e-8)


def test_hip_against_mpmath_truth_d8(golden_dir, lib_loaded):
    """HIP path vs the 50-digit mpmath truth of the D = 8, N = 300 fixture (mu, sigma^2,
    log-likelihood, alpha; oracle/make_golden.py d8_truth): a comparison at D > 2 that does
    not go through the oracle.  Bound: the fp64 conditioning limit 200 cond eps."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, "c3small_d8_n300.npz"))
    gp = build(agp, g)
    idx = g["truth_idx"]
    tol = 200 * float(g["cond"]) * EPS
    asum = np.abs(g["alpha_truth"]).sum()
    mu, var = gp.predict(g["y"], g["cands"][idx], return_var=True)
    assert np.abs(mu - g["mu_truth"]).max() <= tol * asum
    assert np.abs(var - g["var_truth"]).max() <= tol
    assert np.abs(gp.predict(g["y"], g["cands"][idx], return_cov=False) - g["mu_truth"]).max() <= tol * asum
    assert abs(gp.log_likelihood(g["y"]) - float(g["ll_truth"])) <= tol * abs(float(g["ll_truth"]))
    gp._solve(g["y"], need_alpha=True)
    assert np.abs(gp._alpha.cpu().numpy() - g["alpha_truth"]).max() <= tol * np.abs(g["alpha_truth"]).max()
    # the utilities at the truth's (mu, sigma^2): AGP through the HIP epilogue
    bi, bu, u, _, _ = gp.acquire(g["y"], g["cands"][idx], "agp", return_all=True)
    ut = -(g["mu_truth"] + 0.5 * np.log(2 * np.pi * np.e * g["var_truth"]))
    assert np.abs(u - ut).max() <= tol * asum + 0.5 * tol / g["var_truth"].min() + 1e-13 * np.abs(ut).max()
    assert bi == int(np.argmin(ut))


def _synthetic(n, d, seed=0):
    from scipy.optimize import rosen
    rs = np.random.RandomState(seed)
    X = rs.uniform(-5, 5, size=(n, d))
    y = np.array([-rosen(x) / 100.0 for x in X])
    return X, y


@pytest.mark.parametrize("n,d,m,metric", [(1024, 2, 3000, 2.0), (700, 8, 1500, 8.0), (513, 3, 777, 1.0),
                                           (64, 16, 200, 30.0), (1, 1, 5, 1.0), (17, 4, 1, 4.0),
                                           (90, 2, 300, 2.0), (128, 16, 100, 30.0), (65, 5, 64, 6.0),
                                           (1100, 8, 2000, 8.0), (500, 4, 900, 4.0), (448, 2, 700, 2.0)])
def test_oracle_parity_seeded(n, d, m, metric, lib_loaded):
    """HIP vs oracle on seeded synthetic sets: ragged sizes (N, M not multiples
    of any tile), D from 1 to the 16-dim maximum, single candidate / single point.  The last
    256-row block of the factor is partial in most of them: 1 / 76 rows (four-pair tile body),
    188 / 192 rows (six-pair body), 244 rows (predicated body)."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    cands = np.random.RandomState(1).uniform(-5.2, 5.2, size=(m, d))
    ko = go.ExpSquaredKernel(np.full(d, metric), ndim=d)
    gpo = go.GP(kernel=ko, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
    gpo.compute(X)
    k = agp.ExpSquaredKernel(np.full(d, metric), ndim=d)
    gp = agp.GP(kernel=k, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
    gp.compute(X)
    x = gpo._x
    K = gpo.kernel.get_value(x)
    K[np.diag_indices_from(K)] += np.exp(-12.0)
    cond = np.linalg.cond(K)
    tol = max(1e-13, 200 * cond * EPS)
    mo, vo = gpo.predict(y, cands, return_var=True)
    mu, var = gp.predict(y, cands, return_var=True)
    alpha = gpo._compute_alpha(y, False)
    assert np.isclose(gp.log_likelihood(y), gpo.log_likelihood(y), rtol=max(1e-11, tol))
    assert np.abs(mu - mo).max() <= tol * max(np.abs(alpha).sum(), 1e-300)
    assert np.abs(var - vo).max() <= tol
    with np.errstate(all="ignore"):
        uo = -(mo + 0.5 * np.log(2 * np.pi * np.e * vo))
    inside = np.all(np.abs(cands) <= 5, axis=1)
    uo = np.where(inside, uo, np.inf)
    bi, bu = gp.acquire(y, cands, "agp", bounds=[(-5, 5)] * d)
    if np.isfinite(uo).any():
        ri = int(np.nanargmin(uo))
        assert bi == ri or abs(uo[bi] - uo[ri]) <= 1e-9 * max(1.0, abs(uo[ri]))
    else:
        assert bi == -1


@pytest.mark.gpu
def test_george_surface_off_the_path(lib_loaded):
    """george.GP methods approxposterior never calls but a george user may: apply_inverse (vector and
    matrix right-hand sides), get_matrix, nll / grad_nll and the lnlikelihood aliases -- against the oracle."""
    go, agp = _mods()
    n, d = 200, 3
    X, y = _synthetic(n, d)
    def make(mod):
        gp_ = mod.GP(kernel=4.0 * mod.ExpSquaredKernel(np.full(d, 3.0), ndim=d), fit_mean=True, mean=np.median(y),
                     white_noise=-10, fit_white_noise=False)
        gp_.compute(X)
        return gp_
    gpo, gp = make(go), make(agp)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-10.0)
    tol = max(1e-11, 200 * np.linalg.cond(K) * EPS)
    B = np.random.RandomState(5).normal(size=(n, 3))
    for b in (B[:, 0].copy(), B):
        want = gpo.apply_inverse(b)
        got = gp.apply_inverse(b)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= tol * np.abs(want).max()
    T = np.random.RandomState(6).uniform(-5, 5, size=(17, d))
    assert np.abs(gp.get_matrix(T) - gpo.kernel.get_value(T)).max() <= 1e-13 * 4.0
    assert np.abs(gp.get_matrix(T, X) - gpo.kernel.get_value(T, X)).max() <= 1e-13 * 4.0
    p = np.array(gpo.get_parameter_vector()) + 0.05
    gpo.set_parameter_vector(p)
    llo = gpo.log_likelihood(y)
    glo = gpo.grad_log_likelihood(y)
    assert np.isclose(gp.nll(p, y), -llo, rtol=max(1e-11, tol))
    assert np.abs(gp.grad_nll(p, y) + glo).max() <= max(1e-9, tol) * max(1.0, np.abs(glo).max())
    assert gp.lnlikelihood(y) == gp.log_likelihood(y)
    assert np.array_equal(gp.grad_lnlikelihood(y), gp.grad_log_likelihood(y))
    # N <= 64: the factor of the fused one-launch evaluation lives in an uninitialised buffer above its diagonal
    Xs, ys = X[:40], y[:40]
    gps = agp.GP(kernel=4.0 * agp.ExpSquaredKernel(np.full(d, 3.0), ndim=d), fit_mean=True, mean=np.median(ys),
                 white_noise=-10, fit_white_noise=False)
    gos = go.GP(kernel=4.0 * go.ExpSquaredKernel(np.full(d, 3.0), ndim=d), fit_mean=True, mean=np.median(ys),
                white_noise=-10, fit_white_noise=False)
    gps.compute(Xs); gos.compute(Xs)
    assert np.isclose(gps.log_likelihood(ys), gos.log_likelihood(ys), rtol=1e-10)
    bs = B[:40, 0].copy()
    assert np.abs(gps.apply_inverse(bs) - gos.apply_inverse(bs)).max() <= 1e-8 * np.abs(gos.apply_inverse(bs)).max()
    ms_, cs_ = gps.predict(ys, T)
    mo_, co_ = gos.predict(ys, T)
    assert np.abs(cs_ - co_).max() <= 1e-8 * max(1.0, np.abs(co_).max())


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m,metric,order", [(130, 5, 40, 6.0, None), (700, 8, 257, 8.0, None), (50, 2, 1, 2.0, None),
                                                (150, 3, 33, 3.0, 1)])
def test_predict_full_covariance(n, d, m, metric, order, lib_loaded):
    """george's GP.predict DEFAULT (return_cov=True): (mu, cov) with cov = k(t,t) - k(t,X) K^-1 k(X,t).
    The reference never asks for it (approx.py:178 and utility.py:131,178,224 pass return_cov=False /
    return_var=True) -- served for callers of the george default, against the oracle's restatement
    (Appendix A.7): the whole matrix, its symmetry, and its diagonal against return_var=True."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    T = np.random.RandomState(3).uniform(-5, 5, size=(m, d))
    def make(mod):
        k = mod.ExpSquaredKernel(np.full(d, metric), ndim=d)
        if order is not None:
            k = 7.0 * k + 0.3 * mod.kernels.LinearKernel(log_gamma2=0.5, order=order, bounds=None, ndim=d)
        gp_ = mod.GP(kernel=k, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
        gp_.compute(X)
        return gp_
    gpo, gp = make(go), make(agp)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-12.0)
    tol = max(1e-12, 200 * np.linalg.cond(K) * EPS)
    mo, co = gpo.predict(y, T)
    mu, cov = gp.predict(y, T)
    assert cov.shape == (m, m) and mu.shape == (m,)
    scale = max(1.0, np.abs(co).max())
    assert np.abs(mu - mo).max() <= tol * max(np.abs(gpo._compute_alpha(y, False)).sum(), 1e-300)
    assert np.abs(cov - co).max() <= tol * scale
    assert np.abs(cov - cov.T).max() <= 1e-10 * scale
    _, var = gp.predict(y, T, return_var=True)
    assert np.abs(np.diag(cov) - var).max() <= tol * scale


@pytest.mark.parametrize("n,d,m,metric", [(1024, 2, 3000, 2.0), (700, 8, 1500, 8.0), (513, 3, 777, 1.0),
                                           (64, 16, 200, 30.0), (1, 1, 5, 1.0), (17, 4, 1, 4.0),
                                           (1300, 8, 20000, 8.0), (255, 2, 333, 2.0), (271, 5, 16500, 6.0)])
def test_substitution_sweep_oracle_parity(n, d, m, metric, lib_loaded):
    """The substitution form of the sweep (apgp_pack_lsolve + apgp_acquire_solve: blocked
    forward substitution against L on the matrix cores, what george's cho_solve computes --
    utility.py:131,178,224) vs the oracle at the same ragged sizes as the inverse form: one
    and several 256-row blocks, partial last block / last 16-row and 4-row group, D = 1 .. 16,
    more candidate blocks than CUs (several rounds of the persistent grid, parked V re-used),
    the three utilities' arg-min.  Same tolerances as the inverse form."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    cands = np.random.RandomState(1).uniform(-5.2, 5.2, size=(m, d))
    gpo = go.GP(kernel=go.ExpSquaredKernel(np.full(d, metric), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gpo.compute(X)
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, metric), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gp.variance_mode = "solve"
    gp.compute(X)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-12.0)
    tol = max(1e-13, 200 * np.linalg.cond(K) * EPS)
    mo, vo = gpo.predict(y, cands, return_var=True)
    mu, var = gp.predict(y, cands, return_var=True)
    assert gp._packed is None                                       # no inverse was formed
    assert (gp._packed_solve is not None) == (m > 1)                # (one candidate: apgp_predict1_host solves against L itself)
    alpha = gpo._compute_alpha(y, False)
    assert np.abs(mu - mo).max() <= tol * max(np.abs(alpha).sum(), 1e-300)
    assert np.abs(var - vo).max() <= tol
    inside = np.all(np.abs(cands) <= 5, axis=1)
    with np.errstate(all="ignore"):
        uo = {"agp": -(mo + 0.5 * np.log(2 * np.pi * np.e * vo)),
              "bape": -((2 * mo + vo) + (vo + np.log(1.0 - np.exp(-vo))))}
    for kind in ("agp", "bape"):
        want = np.where(inside, uo[kind], np.inf)
        bi, bu, u, mu2, var2 = gp.acquire(y, cands, kind, bounds=[(-5, 5)] * d, return_all=True)
        if m > 1:
            assert np.array_equal(mu2, mu) and np.array_equal(var2, var)     # same kernel, same bits
        else:                                                            # (predict took the single-candidate path)
            assert np.abs(mu2 - mu).max() <= tol * max(np.abs(alpha).sum(), 1e-300) and np.abs(var2 - var).max() <= tol
        if np.isfinite(want).any():
            ri = int(np.nanargmin(want))
            assert bi == ri or abs(want[bi] - want[ri]) <= 1e-9 * max(1.0, abs(want[ri]))
            fin = np.where(np.isfinite(u), u, np.inf)
            assert bu == u[bi] and bi == int(np.argmin(fin))
        else:
            assert bi == -1


@pytest.mark.parametrize("n,d,m", [(1152, 8, 30000), (2100, 5, 9000), (4096, 8, 40000)])
def test_substitution_sweep_deterministic_and_matches_inverse(n, d, m, lib_loaded):
    """The substitution form parks the solved blocks V from the MATRIX wavefronts and reads them
    back through the feeders' LDS-DMA a row block later: a missing wait / stale line would show
    as run-to-run differences.  Six launches bit-identical; and against the inverse form on
    the same well-conditioned factor the two formulations agree to the conditioning bound."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    def make(mode):
        g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y),
                   white_noise=-12, fit_white_noise=False)
        g.variance_mode = mode
        g.compute(X)
        return g
    gs, gi = make("solve"), make("inverse")
    T = np.random.RandomState(8).uniform(-5, 5, size=(m, d))
    ref = gs.acquire(y, T, "bape", bounds=[(-5, 5)] * d, return_all=True)
    for _ in range(5):
        out = gs.acquire(y, T, "bape", bounds=[(-5, 5)] * d, return_all=True)
        assert out[0] == ref[0] and out[1] == ref[1]
        for a, b in zip(out[2:], ref[2:]):
            assert np.array_equal(a, b, equal_nan=True)
    inv = gi.acquire(y, T, "bape", bounds=[(-5, 5)] * d, return_all=True)
    tol = max(1e-13, 200 * gs.cond_estimate * 100 * EPS)
    assert np.abs(ref[4] - inv[4]).max() <= tol                     # sigma^2
    assert np.abs(ref[3] - inv[3]).max() <= 1e-9 * np.abs(inv[3]).max()   # mu (alpha by trsv vs W)
    assert ref[0] == inv[0] or abs(ref[1] - inv[1]) <= 1e-9 * abs(inv[1])


@pytest.mark.parametrize("n,d", [(50, 2), (300, 5), (700, 16), (1300, 8)])
@pytest.mark.parametrize("mode", ["inverse", "solve"])
def test_single_candidate_path(n, d, mode, lib_loaded):
    """ONE candidate per call (apgp_predict1_host: k* kernel -> one matrix-vector product with the dense
    L^-1 or one triangular solve -> single-workgroup epilogue -> mailbox) is what the reference's scalar
    utilities evaluate once per Nelder-Mead step (utility.py:131,178,224).  Against the oracle and against
    the fused sweep over the same candidates (different summation order: to the conditioning bound), NaN
    coordinates, and the three scalar utilities of utility.py on top of it."""
    go, agp = _mods()
    from approxposterior_amd import utility as ut
    X, y = _synthetic(n, d)
    gpo = go.GP(kernel=go.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gpo.compute(X)
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gp.variance_mode = mode
    gp.compute(X)
    T = np.random.RandomState(9).uniform(-5, 5, size=(40, d))
    T[:4] = X[:4] + 1e-3                                     # near training points: tiny variance
    mo, vo = gpo.predict(y, T, return_var=True)
    mb, vb = gp.predict(y, T, return_var=True)               # fused sweep
    one = np.array([gp.predict(y, T[i:i + 1], return_var=True) for i in range(len(T))]).reshape(len(T), 2)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-12.0)
    tol = max(1e-13, 200 * np.linalg.cond(K) * EPS)
    asum = np.abs(gpo._compute_alpha(y, False)).sum()
    assert np.abs(one[:, 0] - mo).max() <= tol * asum and np.abs(one[:, 1] - vo).max() <= tol
    assert np.abs(one[:, 0] - mb).max() <= tol * asum and np.abs(one[:, 1] - vb).max() <= tol
    again = np.array(gp.predict(y, T[7:8], return_var=True)).ravel()
    assert np.array_equal(again, one[7])                     # run-to-run identical
    bad = T[5:6].copy(); bad[0, d - 1] = np.nan
    mn, vn = gp.predict(y, bad, return_var=True)
    assert np.isnan(mn[0]) and np.isnan(vn[0])
    prior = lambda t: 0.0                                    # noqa: E731
    with np.errstate(all="ignore"):
        for i in (0, 9, 21):
            assert np.isclose(float(np.ravel(ut.AGPUtility(T[i], y, gp, prior))[0]),
                              -(mo[i] + 0.5 * np.log(2 * np.pi * np.e * vo[i])), rtol=1e-8, atol=1e-8) or vo[i] < 1e-5
            if vo[i] > 1e-5:
                assert np.isclose(float(np.ravel(ut.BAPEUtility(T[i], y, gp, prior))[0]),
                                  -((2 * mo[i] + vo[i]) + (vo[i] + np.log(1.0 - np.exp(-vo[i])))), rtol=1e-7)


@pytest.mark.parametrize("n,d", [(700, 8), (1100, 3), (50, 2), (129, 5)])
def test_alpha_through_resident_inverse(n, d, lib_loaded):
    """K3 both ways: z = L^-1 r, alpha = L^-T z by the triangular solves (apgp_trsv) and, once
    the sweep's dense W = L^-1 is resident, by the two matrix-vector products of
    apgp_winv_apply -- both against the oracle's cho_solve (george GP._compute_alpha), and
    z.z (the quadratic form of GP.log_likelihood) against r^T K^-1 r."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    ko = go.ExpSquaredKernel(np.full(d, float(d)), ndim=d)
    gpo = go.GP(kernel=ko, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
    gpo.compute(X)
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, float(d)), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gp.compute(X)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-12.0)
    tol = max(1e-12, 200 * np.linalg.cond(K) * EPS)
    want = gpo._compute_alpha(y, False)
    quad = float((y - np.median(y)) @ want)
    gp.variance_mode = "solve"                             # the triangular solves at every size (from N = 512
    ztz_t = gp._solve(y, need_alpha=True)                  # on gp._solve would form L^-1 first, see W_FIRST_MIN_N)
    a_t = gp._alpha.cpu().numpy()
    assert gp._work is None
    gp.variance_mode = None
    gp._ensure_linv()
    gp._z = gp._alpha = gp._alpha_y = None
    ztz_w = gp._solve(y, need_alpha=True)                  # W resident: matrix-vector products
    a_w = gp._alpha.cpu().numpy()
    for a_, q_ in ((a_t, ztz_t), (a_w, ztz_w)):
        assert np.abs(a_ - want).max() <= tol * np.abs(want).max()
        assert abs(q_ - quad) <= tol * abs(quad)
    # the sweep set-up takes the second path and predicts the same mean
    T = np.random.RandomState(4).uniform(-5, 5, size=(300, d))
    mu, var = gp.predict(y, T, return_var=True)
    mo, vo = gpo.predict(y, T, return_var=True)
    assert np.abs(mu - mo).max() <= tol * np.abs(want).sum() and np.abs(var - vo).max() <= tol


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 193, 257, 700, 1100])
def test_cholesky_c_abi_against_lapack(n, lib_loaded):
    """apgp_potrf through the C ABI at ragged sizes (one block, block boundaries +-1, the fused
    update + panel launches with a partial last block): L against numpy's Cholesky of the same
    matrix, the forward solve riding along against a triangular solve, and the bytes above the
    diagonal untouched ("only the lower triangle of A is read and written")."""
    import torch
    from scipy.linalg import solve_triangular
    rs = np.random.RandomState(100 + n)
    X = rs.uniform(-3, 3, size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-0.5 * d2) + 1e-6 * np.eye(n)
    y = rs.randn(n)
    Lref = np.linalg.cholesky(K)
    zref = solve_triangular(Lref, y - 0.25, lower=True)
    A = np.tril(K) + np.triu(np.full((n, n), 7.5), 1)      # a sentinel above the diagonal
    Ad = torch.from_numpy(A).cuda()
    yd = torch.from_numpy(y).cuda()
    zd = torch.empty(n, dtype=torch.float64, device="cuda")
    info = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):                                     # (second call: the cached scratch)
        Ad.copy_(torch.from_numpy(A))
        rc = lib_loaded.apgp_potrf(Ad.data_ptr(), n, n, yd.data_ptr(), 0.25, zd.data_ptr(), info.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        L = Ad.cpu().numpy()
        tol = 50 * np.linalg.cond(K) * EPS
        assert np.abs(np.tril(L) - Lref).max() <= tol * np.abs(Lref).max()
        assert np.array_equal(np.triu(L, 1), np.triu(A, 1))
        assert np.abs(zd.cpu().numpy() - zref).max() <= tol * max(1.0, np.abs(zref).max())
    # not positive definite: LAPACK's info (first failing leading minor)
    B = np.tril(K)
    kbad = n // 2
    B[kbad, kbad] = -1.0
    Ad.copy_(torch.from_numpy(B))
    assert lib_loaded.apgp_potrf(Ad.data_ptr(), n, n, None, 0.0, None, info.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(info.item()) == kbad + 1


@pytest.mark.parametrize("n", [1, 63, 65, 130, 700, 2100])
def test_triangular_inverse_c_abi_against_lapack(n, lib_loaded):
    """apgp_trtri_pack through the C ABI: the dense W = L^-1 it leaves behind against a triangular
    solve with the identity -- one block, block boundaries +-1, several merge levels, and N = 2100
    (33 blocks: the top merge level takes the paired-tile path with a ragged last block)."""
    import torch
    from scipy.linalg import solve_triangular
    rs = np.random.RandomState(300 + n)
    X = rs.uniform(-3, 3, size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-0.5 * d2) + 1e-4 * np.eye(n)
    L = np.linalg.cholesky(K)
    Wref = solve_triangular(L, np.eye(n), lower=True)
    Ld = torch.from_numpy(L).cuda()
    work = torch.empty(int(lib_loaded.apgp_trtri_work_len(n)), dtype=torch.float64, device="cuda")
    packed = torch.empty(int(lib_loaded.apgp_packed_linv_len(n)), dtype=torch.float64, device="cuda")
    Wd = torch.empty((n, n), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib_loaded.apgp_trtri_pack(Ld.data_ptr(), n, n, work.data_ptr(), packed.data_ptr(), Wd.data_ptr(), st) == 0
    torch.cuda.synchronize()
    W = Wd.cpu().numpy()
    assert np.array_equal(np.triu(W, 1), np.zeros((n, n)))
    # forward error of a triangular inverse: ~ cond(L) eps relative to |W|
    tol = 50 * np.linalg.cond(L) * EPS
    assert np.abs(W - Wref).max() <= tol * np.abs(Wref).max()


@pytest.mark.parametrize("n,d", [(1300, 5), (257, 2)])
def test_gradient_many_tiles(n, d, lib_loaded):
    """K4 beyond the fixtures' sizes: K^-1 on the lower-triangle tiles only, gradient tiles
    counted twice off the diagonal (21 x 22 / 2 tiles at N = 1300) -- against the oracle's
    gradient (full matrices, NumPy)."""
    go, agp = _mods()
    X, y = _synthetic(n, d, seed=3)
    def make(mod):
        k = mod.Product(mod.ConstantKernel(np.log(2.0), ndim=d), mod.ExpSquaredKernel(np.full(d, 3.0 * d), ndim=d))
        g = mod.GP(kernel=k, fit_mean=True, mean=float(np.median(y)), white_noise=-9.0, fit_white_noise=False)
        g.compute(X)
        return g
    gpo, gp = make(go), make(agp)
    want = gpo.grad_log_likelihood(y, quiet=True)
    K = gpo.kernel.get_value(gpo._x)
    K[np.diag_indices_from(K)] += np.exp(-9.0)
    tol = max(1e-11, 500 * np.linalg.cond(K) * EPS)
    for mode in (None, "solve"):            # (None: the explicit inverse for this K; "solve": apgp_kinv_solve, 21 block rows)
        gp.variance_mode = mode
        got = gp.grad_log_likelihood(y, quiet=True)
        assert np.allclose(got, want, rtol=tol, atol=tol * np.abs(want).max())


@pytest.mark.parametrize("m", [5000, 40000])
def test_multi_row_block_utilities_mask_nan(m, lib_loaded):
    """N > 512 (several row blocks: parked operands, persistent + split launches) with everything
    the epilogue handles: the three utilities against the reference's formulas (utility.py:136,
    183 with logsubexp :85-88, 229-244) on the oracle's mu / sigma^2, the host mask, the box
    prior, NaN coordinates (george propagates NaN; a NaN utility never wins)."""
    from scipy.stats import norm
    go, agp = _mods()
    n, d = 1100, 3
    X, y = _synthetic(n, d)
    def make(mod):
        return mod.GP(kernel=mod.ExpSquaredKernel(np.full(d, 3.0), ndim=d), fit_mean=True, mean=np.median(y),
                      white_noise=-12, fit_white_noise=False)
    gpo, gp = make(go), make(agp)
    gpo.compute(X); gp.compute(X)
    rs = np.random.RandomState(2)
    T = rs.uniform(-5.3, 5.3, size=(m, d))
    T[7, 1] = np.nan
    T[m - 3, 0] = np.nan
    mask = rs.uniform(size=m) > 0.1
    ok = ~np.isnan(T).any(axis=1)
    mo = np.full(m, np.nan); vo = np.full(m, np.nan)
    mo[ok], vo[ok] = gpo.predict(y, T[ok], return_var=True)
    inside = np.all(np.abs(np.nan_to_num(T)) <= 5, axis=1)
    adm = inside & mask & ok
    ybest = y.max()
    with np.errstate(all="ignore"):
        sd = np.sqrt(vo)
        imp = mo - ybest - 0.01
        want = {"agp": -(mo + 0.5 * np.log(2 * np.pi * np.e * vo)),
                "bape": -((2 * mo + vo) + np.where(vo <= 0, -np.inf, vo + np.log(1 - np.exp(-vo)))),
                "jones": np.where(sd > 0, -(imp * norm.cdf(imp / sd) + sd * norm.pdf(imp / sd)), 0.0)}
    for kind, uo in want.items():
        bi, bu, u, mu, var = gp.acquire(y, T, kind, bounds=[(-5, 5)] * d, mask=mask, return_all=True)
        assert np.isnan(mu[~ok]).all() and np.isnan(var[~ok]).all()
        assert np.abs(mu[ok] - mo[ok]).max() <= 1e-9 * np.abs(mo[ok]).max() and np.abs(var[ok] - vo[ok]).max() <= 1e-9
        assert np.all(np.isposinf(u[~inside | ~mask]))
        # the utilities amplify the sigma^2 rounding where sigma^2 is tiny: compare where it is not
        sel = adm & (vo > 1e-6)
        assert np.allclose(u[sel], uo[sel], rtol=1e-6, atol=1e-6 * np.abs(uo[sel]).max())
        fin = np.where(np.isfinite(u) & adm, u, np.inf)
        assert adm[bi] and bu == u[bi] and bi == int(np.argmin(fin))


def test_full_size_properties(lib_loaded):
    """BASELINE.json C3 shape (N=4096, D=8): size-independent properties.
    (a) at a training point the posterior mean reproduces y and the variance
        collapses to the white-noise level: mu(x_i) = y_i - e^wn * alpha_i,
        var(x_i) = e^wn * (1 - e^wn * Kinv_ii) in (0, e^wn];
    (b) the arg-min over a candidate set is invariant under permutation and under
        sharding with global index offsets (what the multi-GPU path relies on);
    (c) candidates outside the box prior never win and get u = +inf."""
    go, agp = _mods()
    import torch
    N, D = 4096, 8
    X, y = _synthetic(N, D)
    k = agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=np.median(y), white_noise=-12, fit_white_noise=False)
    gp.compute(X)
    wn = np.exp(-12.0)
    idx = np.arange(0, N, 37)
    mu, var = gp.predict(y, X[idx], return_var=True)
    gp._solve(y, need_alpha=True)
    alpha = gp._alpha.cpu().numpy()
    assert np.abs(mu - (y[idx] - wn * alpha[idx])).max() <= 1e-9 * np.abs(y).max()
    assert (var > 0).all() and (var <= wn * (1 + 1e-6)).all()
    rs = np.random.RandomState(3)
    M = 20000
    cands = rs.uniform(-5.5, 5.5, size=(M, D))
    bi, bu, u, mu, var = gp.acquire(y, cands, "agp", bounds=[(-5, 5)] * D, return_all=True)
    outside = np.any(np.abs(cands) > 5, axis=1)
    assert np.all(np.isposinf(u[outside])) and not outside[bi]
    assert bi == int(np.nanargmin(np.where(np.isnan(u), np.inf, u)))
    perm = rs.permutation(M)
    pbi, pbu = gp.acquire(y, cands[perm], "agp", bounds=[(-5, 5)] * D)
    assert perm[pbi] == bi and pbu == bu
    # sharded with offsets
    from approxposterior_amd.dist import shard_bounds, combine_best
    pairs = []
    for r in range(3):
        lo, hi = shard_bounds(M, 3, r)
        sbi, sbu = gp.acquire(y, cands[lo:hi], "agp", bounds=[(-5, 5)] * D, idx_offset=lo)
        pairs.append((sbu, sbi))
    assert combine_best(pairs) == (bi, bu)
    # device-resident candidates give the same answer as host candidates
    T = torch.from_numpy(cands).cuda()
    assert gp.acquire(y, T, "agp", bounds=[(-5, 5)] * D) == (bi, bu)
    # (d) BASELINE.json's full candidate count (1e6: 62 rounds of the persistent grid, every
    #     workgroup slot's parked-operand stream re-used): the result for a candidate does not
    #     depend on which block / round / slot evaluated it (to rounding: the order in which
    #     the four row-group partial sums of sigma^2 are added depends on the candidate's lane)
    M1 = 1000000
    big = rs.uniform(-5.0, 5.0, size=(M1, D))
    Tb = torch.from_numpy(big).cuda()
    fbi, fbu, fu, fmu, fvar = gp.acquire(y, Tb, "agp", bounds=[(-5, 5)] * D, return_all=True)
    assert fbi == int(np.argmin(fu)) and fbu == fu[fbi] and np.isfinite(fu).all()
    pick = np.sort(rs.choice(M1, size=5000, replace=False))
    sbi, sbu, su, smu, svar = gp.acquire(y, big[pick], "agp", bounds=[(-5, 5)] * D, return_all=True)
    assert np.array_equal(smu, fmu[pick])
    assert np.abs(svar - fvar[pick]).max() <= 1e-13 and np.abs(su - fu[pick]).max() <= 1e-11 * np.abs(fu).max()
    # (e) an empty candidate set: nothing admissible
    assert gp.acquire(y, np.empty((0, D)), "agp") == (-1, np.inf)
    emu, ecov = gp.predict(y, np.empty((0, D)))
    assert emu.shape == (0,) and ecov.shape == (0, 0)
    emu, evar = gp.predict(y, np.empty((0, D)), return_var=True)
    assert emu.shape == (0,) and evar.shape == (0,)


@pytest.mark.parametrize("n,d,m", [(1152, 8, 30000), (2100, 5, 9000), (4096, 8, 20000)])
def test_sweep_is_deterministic(n, d, m, lib_loaded):
    """The sweep's LDS ring / parked-operand stream / split last round are hand-synchronised:
    a missing barrier or a stale slot would show up as run-to-run differences.  Same inputs,
    six launches (persistent + split paths), bit-identical mu, sigma^2, u and arg-min."""
    go, agp = _mods()
    X, y = _synthetic(n, d)
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y),
                white_noise=-12, fit_white_noise=False)
    gp.compute(X)
    T = np.random.RandomState(8).uniform(-5, 5, size=(m, d))
    ref = gp.acquire(y, T, "bape", bounds=[(-5, 5)] * d, return_all=True)
    for _ in range(5):
        out = gp.acquire(y, T, "bape", bounds=[(-5, 5)] * d, return_all=True)
        assert out[0] == ref[0] and out[1] == ref[1]
        for a, b in zip(out[2:], ref[2:]):
            assert np.array_equal(a, b, equal_nan=True)


def test_error_behaviour(lib_loaded):
    """Failure conventions the boundary must keep:
    non-PD -> LinAlgError from compute, -inf from log_likelihood(quiet=True);
    dimension mismatch -> ValueError; uncomputed GP -> RuntimeError in utilities;
    bad C-ABI arguments -> negative status + message, never a crash."""
    go, agp = _mods()
    from approxposterior_amd import _lib, utility as ut
    X = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]])   # duplicate point
    y = np.array([1.0, 2.0, 3.0])
    k = agp.ExpSquaredKernel([1.0, 1.0], ndim=2)
    gp = agp.GP(kernel=k, fit_mean=True, mean=0.0, white_noise=-800.0, fit_white_noise=False)
    with pytest.raises(np.linalg.LinAlgError):
        gp.compute(X)
    assert gp.log_likelihood(y, quiet=True) == -np.inf
    assert np.all(gp.grad_log_likelihood(y, quiet=True) == 0)
    gp2 = agp.GP(kernel=agp.ExpSquaredKernel([1.0, 1.0], ndim=2), fit_mean=True, mean=0.0,
                 white_noise=-12, fit_white_noise=False)
    gp2.compute(X[1:])
    with pytest.raises(ValueError):
        gp2.predict(y[1:], np.zeros((4, 3)), return_var=True)
    with pytest.raises(ValueError):
        gp2.log_likelihood(y)           # wrong length, not quiet
    gp2.set_parameter_vector(gp2.get_parameter_vector() + 0.1)
    assert not gp2.computed
    with pytest.raises(RuntimeError):
        ut.AGPUtility(np.zeros(2), y[1:], gp2, lambda t: 0.0)
    lib = _lib.load()
    assert lib.apgp_gram(None, 4, None, None, 4, None) == -1
    assert b"null pointer" in lib.apgp_last_error()
    ks = _lib.KernelStruct()
    ks.ndim = 99
    import torch
    buf = torch.zeros(16, dtype=torch.float64, device="cuda")
    assert lib.apgp_gram(buf.data_ptr(), 4, ctypes.byref(ks), buf.data_ptr(), 4, None) == -1


def test_illconditioned_uses_solve_path(golden_dir, lib_loaded):
    """cond(K) ~ 1e16 (fitAmp=True at the reference's own optimum, SURVEY.md
    section 7).  No fp64 formulation agrees with another here -- george's cho_solve
    is itself up to 28 % off exact arithmetic -- so the HIP path is judged against
    the 60-digit mpmath truth stored in the fixture: it must select the solve-based
    sweep automatically and be no worse than the oracle's error class (the explicit
    inverse is off by factors of 10-1000 here and must NOT be what runs)."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, "rosen2d_n50_amp_opt_illcond.npz"))
    gp = build(agp, g)
    assert gp.cond_estimate > 1e10 and g["cond"] > 1e15
    mu, var = gp.predict(g["y"], g["cands"], return_var=True)
    vt, mt = g["var_truth"], g["mu_truth"]
    mine = np.abs(var - vt) / np.abs(vt)
    ref = np.abs(g["var"] - vt) / np.abs(vt)
    assert mine.max() <= 2.0 * ref.max() and np.median(mine) <= 5.0 * np.median(ref), (mine.max(), ref.max())
    assert (np.abs(mu - mt) / np.abs(mt)).max() <= 1e-2
    # the arg-min it selects is a candidate whose TRUE utility is within the noise of the best
    bounds = list(zip(g["lo"], g["hi"]))
    bi, bu = gp.acquire(g["y"], g["cands"], "bape", bounds=bounds)
    u_true = -((2 * mt + vt) + (vt + np.log(-np.expm1(-vt))))
    assert u_true[bi] <= u_true.min() + 0.3 * abs(u_true.min())


LADDER = ["rosen2d_n50_amp_cond1e8", "rosen2d_n50_amp_cond1e11", "rosen2d_n50_amp_cond1e13"]


@pytest.mark.parametrize("mode", ["inverse", "solve", None])
@pytest.mark.parametrize("name", LADDER)
def test_conditioning_ladder(golden_dir, name, mode, lib_loaded):
    """Between the well-conditioned fixtures (cond <= 4.7e6) and the reference's fitAmp=True
    optimum (8.5e15): the reference's own N = 50 Rosenbrock set at true cond(K) = 1e8 / 1e11 /
    1e13 (oracle/make_golden.py cond_ladder), each with a 60-digit mpmath truth.  BOTH variance
    formulations -- the explicit L^-1 contraction and the blocked substitution -- and the
    automatic choice must stay in george's own error class against exact arithmetic: median
    relative error of sigma^2 <= 3x the oracle's (cho_solve), largest absolute error <= 2x the
    oracle's; alpha (through apgp_winv_apply resp. apgp_trsv) and mu likewise.  This is what
    pins COND_SOLVE: the Cholesky-diagonal estimate under-reads the true condition number by
    2-3 orders here (4e5 / 3e8 / 2.9e10 for 1e8 / 1e11 / 1e13), so the gate at 1e10 *estimated*
    hands over between the 1e11 and 1e13 rungs, and the inverse is asserted good on both sides
    of it (at 8.5e15 it is 200x off: test_illconditioned_uses_solve_path)."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gp = build(agp, g)
    gp.variance_mode = mode
    est = gp.cond_estimate
    assert est < g["cond"]                                   # the estimate is a lower bound
    if mode is None:
        assert gp._trust_inverse() == (est <= agp.COND_SOLVE)
    mu, var = gp.predict(g["y"], g["cands"], return_var=True)
    vt, mt, at = g["var_truth"], g["mu_truth"], g["alpha_truth"]
    mine, ref = np.abs(var - vt), np.abs(g["var"] - vt)
    assert np.median(mine / np.abs(vt)) <= 3.0 * np.median(ref / np.abs(vt)), (np.median(mine / np.abs(vt)), np.median(ref / np.abs(vt)))
    assert mine.max() <= 2.0 * ref.max(), (mine.max(), ref.max())
    alpha = gp._alpha.cpu().numpy()
    assert np.abs(alpha - at).max() <= 3.0 * np.abs(g["alpha"] - at).max(), (np.abs(alpha - at).max(), np.abs(g["alpha"] - at).max())
    assert np.abs(mu - mt).max() <= 3.0 * np.abs(g["mu"] - mt).max() + 1e-13 * np.abs(mt).max()
    # the acquisition picks a candidate whose TRUE utility is the best one's (to the noise level)
    bounds = list(zip(g["lo"], g["hi"]))
    for kind, u_true in (("bape", -((2 * mt + vt) + (vt + np.log(-np.expm1(-vt))))),
                         ("agp", -(mt + 0.5 * np.log(2 * np.pi * np.e * vt)))):
        bi, bu = gp.acquire(g["y"], g["cands"], kind, bounds=bounds)
        assert u_true[bi] <= u_true.min() + 1e-3 * abs(u_true.min())


@pytest.mark.parametrize("mode", ["inverse", "solve", None])
@pytest.mark.parametrize("name", LADDER + ["rosen2d_n50_amp_opt_illcond"])
def test_gradient_on_the_conditioning_ladder(golden_dir, name, mode, lib_loaded):
    """K4 (gpUtils._grad_nll -> george GP.grad_log_likelihood, gpUtils.py:83-111) against a 60-digit mpmath gradient
    on every rung of the ladder and at the reference's optimum (true cond 8.5e15): through the explicit inverse
    (K^-1 = W^T W), through the solve route (two blocked triangular solves against the identity: george's
    cho_solve(L, I)), and through the automatic gate, which must hand the gradient to the solve route exactly when it
    hands sigma^2 and alpha to it (round 3: the gradient ignored the gate).
    Bar per component: error <= max(3 x the oracle's, 1e-3 cond eps max|truth|).  The second term is the error CLASS
    (both implementations sit two to three orders below cond eps |g|; within it the oracle's own error varies by 10x
    from component to component -- 1.9e-6 vs 1.4e-4 at cond 1e13 -- so a bare ratio would compare noise).  At 8.5e15
    the explicit inverse is held to the bar only where it is trusted: there the solve route is 15x closer on
    d/d log_constant (9.5e-3 vs 2.3e-1, oracle 1.4e-1: profiles/r04e_grad_ladder.txt)."""
    go, agp = _mods()
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    gp = build(agp, g)
    gp.variance_mode = mode
    truth, ref = g["grad_truth"], g["grad"]
    hip = gp.grad_log_likelihood(g["y"])
    if mode is None:
        assert gp._trust_inverse() == (gp.cond_estimate <= agp.COND_SOLVE)
    if name.endswith("illcond"):
        assert gp.cond_estimate > agp.COND_SOLVE                # auto = solve route here
        if mode == "inverse":
            return                                              # (forced against the gate: not held to the bar)
    floor = 1e-3 * float(g["cond"]) * np.finfo(np.float64).eps * np.abs(truth).max()
    err, err_ref = np.abs(hip - truth), np.abs(ref - truth)
    assert np.all(err <= np.maximum(3.0 * err_ref, floor)), (err, err_ref, floor)
    # and it is a descent direction of the right size: relative to the truth's norm
    assert np.linalg.norm(hip - truth) <= max(3.0 * np.linalg.norm(ref - truth), 2.0 * floor)


# ---- round 4: the Cholesky as ONE persistent launch (csrc/potrf_persist.h) vs the multi-launch path ----------------
def _nll_eval_raw(lib, torch, X_d, y_d, n, ks, mean, mode):
    lib.apgp_potrf_mode(mode)
    try:
        K = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        z = torch.empty(n, dtype=torch.float64, device="cuda")
        info = torch.empty(1, dtype=torch.int32, device="cuda")
        o5 = torch.empty(5, dtype=torch.float64, device="cuda")
        o = np.empty(5)
        rc = lib.apgp_nll_eval(X_d.data_ptr(), n, ctypes.byref(ks), y_d.data_ptr(), mean, K.data_ptr(), z.data_ptr(),
                               info.data_ptr(), o5.data_ptr(), o.ctypes.data, None)
        assert rc == 0, lib.apgp_last_error()
        torch.cuda.synchronize()
        return torch.tril(K).clone(), z.clone(), o.copy(), int(info.item())
    finally:
        lib.apgp_potrf_mode(0)


def _persist_case(n, D, seed, wn=-12.0, dup=None):
    import torch
    go, agp = _mods()
    rs = np.random.RandomState(seed)
    X = rs.uniform(-5, 5, size=(n, D))
    if dup is not None:
        X[dup] = X[dup - 1]; X[dup + 1] = X[dup - 1]
    y = rs.normal(size=n)
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=0.0, white_noise=wn,
               fit_white_noise=False)
    g._x = X; g._yerr2 = 0.0
    return torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), g._kernel_struct()


@pytest.mark.parametrize("n,D", [(65, 2), (100, 8), (128, 2), (129, 8), (192, 3), (300, 8), (700, 2), (1152, 8), (1153, 8),
                                 (2048, 8), (3000, 5), (4095, 8), (4096, 8)])
def test_persistent_cholesky_bit_identical_to_multi_launch(n, D, lib_loaded):
    """One gpUtils._nll evaluation (gpUtils.py:46-80) through the persistent launch (forced, mode 3: up to n = 4096)
    and through the launch-per-step path: factor, z = L^-1 (y - mean), the 5-value record and the LAPACK info word are
    the SAME BITS -- every element sees the same operations in the same order, whatever the hand-offs' timing -- at
    sizes that are not multiples of the 64-column block, of the 16-column chunk or of anything else; and the
    persistent launch did not fall back to produce them."""
    import torch
    lib = lib_loaded
    X_d, y_d, ks = _persist_case(n, D, n + D)
    L1, z1, o1, i1 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 1)
    fb = lib.apgp_potrf_fallbacks()
    L3, z3, o3, i3 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 3)
    assert lib.apgp_potrf_fallbacks() == fb
    assert i1 == i3 == 0 and np.array_equal(o1, o3)
    assert torch.equal(L1, L3) and torch.equal(z1, z3)
    # and the factor is a Cholesky factor: L L^T against the oracle's Gram matrix
    if n <= 1153:
        go, agp = _mods()
        Lh = L3.cpu().numpy()
        Kh = Lh @ Lh.T
        Xh = X_d.cpu().numpy()
        d2 = ((Xh[:, None, :] - Xh[None, :, :]) ** 2).sum(-1) / 8.0
        Ko = np.exp(-0.5 * d2) + np.exp(-12.0) * np.eye(n)
        assert np.abs(Kh - Ko).max() <= 1e-12


@pytest.mark.parametrize("n,dup", [(200, 70), (700, 650), (1152, 64), (1152, 1100)])
def test_persistent_cholesky_reports_the_failing_minor(n, dup, lib_loaded):
    """scipy.linalg.cholesky inside george raises LinAlgError with the order of the first leading minor that is not
    positive definite; apgp_nll_eval reports it in the record's info slot.  Duplicated points with e^-60 of white
    noise: the persistent launch must report the multi-launch path's (LAPACK's) order and, like it, never hang on the
    NaNs that follow the failed pivot."""
    import torch
    lib = lib_loaded
    X_d, y_d, ks = _persist_case(n, 3, 7 * n, wn=-60.0, dup=dup)
    _, _, o1, i1 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.0, 1)
    _, _, o3, i3 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.0, 3)
    assert i1 > 0 and i3 == i1 and o3[4] == o1[4] == i1


def test_persistent_cholesky_gives_up_and_falls_back(lib_loaded):
    """The persistent launch needs all its workgroups resident; when they are not (a foreign kernel holds compute
    units) it gives up after a bounded wait and apgp_nll_eval re-runs the evaluation on the multi-launch path.
    Mode 2 makes workgroup 0 give up at once: the call must return the multi-launch result and count one fallback;
    the next ordinary call runs persistently again (the give-up mark is per call)."""
    import torch
    lib = lib_loaded
    n = 1152
    X_d, y_d, ks = _persist_case(n, 8, 3)
    L1, z1, o1, _ = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.0, 1)
    fb = lib.apgp_potrf_fallbacks()
    L2, z2, o2, _ = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.0, 2)
    assert lib.apgp_potrf_fallbacks() == fb + 1
    assert torch.equal(L2, L1) and torch.equal(z2, z1) and np.array_equal(o2, o1)
    L0, z0, o0, _ = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.0, 0)
    assert lib.apgp_potrf_fallbacks() == fb + 1
    assert torch.equal(L0, L1) and np.array_equal(o0, o1)


def test_persistent_cholesky_repeated_calls_leave_no_state(lib_loaded):
    """Flags and granule tags are call-unique and never zeroed between calls: 120 evaluations in a row -- two
    training sets of different size alternating on one stream -- must reproduce their first results bit for bit."""
    import torch
    lib = lib_loaded
    cases = [(1152, _persist_case(1152, 8, 3)), (700, _persist_case(700, 2, 4))]
    first = [_nll_eval_raw(lib, torch, c[0], c[1], n, c[2], 0.0, 0) for n, c in cases]
    fb = lib.apgp_potrf_fallbacks()
    for it in range(60):
        for (n, c), f in zip(cases, first):
            L, z, o, i = _nll_eval_raw(lib, torch, c[0], c[1], n, c[2], 0.0, 0)
            assert torch.equal(L, f[0]) and torch.equal(z, f[1]) and np.array_equal(o, f[2])
    assert lib.apgp_potrf_fallbacks() == fb


@pytest.mark.parametrize("n,D,dup", [(3264, 8, None), (3800, 8, None), (4096, 8, None), (5000, 5, None), (4096, 3, 3000)])
def test_hybrid_cholesky_bit_identical_to_multi_launch(n, D, dup, lib_loaded):
    """Above 50 block columns the default is the hybrid (round 4): the first block columns a launch per 64-column step --
    while the trailing update bounds a step -- and the last 44 as ONE persistent launch on the trailing
    matrix (shifted base pointers, pivot numbering of the full matrix, the running right-hand side handed over in
    place).  Same bits as the launch-per-step path all the way: factor, z, record, LAPACK info (also on a matrix that
    is not positive definite inside the persistent part's range)."""
    import torch
    lib = lib_loaded
    X_d, y_d, ks = _persist_case(n, D, n + D, wn=-60.0 if dup is not None else -12.0, dup=dup)
    L1, z1, o1, i1 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 1)
    fb = lib.apgp_potrf_fallbacks()
    L0, z0, o0, i0 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 0)
    assert lib.apgp_potrf_fallbacks() == fb
    assert i0 == i1 and o0[4] == o1[4]
    if dup is None:
        assert i0 == 0 and np.array_equal(o0, o1) and torch.equal(L0, L1) and torch.equal(z0, z1)
    else:
        assert i0 > 0


@pytest.mark.parametrize("n,D", [(1700, 3), (1857, 2), (3000, 8), (4096, 8), (5000, 5), (6100, 4)])
def test_paired_trailing_updates_bit_identical(n, D, lib_loaded):
    """Launch-per-step Cholesky with its paired trailing updates (a narrow step applies its block column to the first two
    tile columns, the wide step after it applies both block columns to every other tile in one pass, each product
    accumulated from zero and subtracted in turn) against the same path with every step applying its own column
    (mode + 16): factor, z, record the same bits."""
    import torch
    lib = lib_loaded
    X_d, y_d, ks = _persist_case(n, D, n + D)
    L1, z1, o1, i1 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 1)
    L0, z0, o0, i0 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, 17)
    assert i0 == i1 == 0 and np.array_equal(o0, o1) and torch.equal(L0, L1) and torch.equal(z0, z1)
    # ... and with the pairs but without the deferred tiles (round 5: a wide step leaves half of its far tiles to the
    # narrow step after it, mode + 32 switches that off), launch-per-step and default plan
    for mode in (1 + 32, 0 + 32):
        L2, z2, o2, i2 = _nll_eval_raw(lib, torch, X_d, y_d, n, ks, 0.25, mode)
        assert i2 == 0 and np.array_equal(o2, o1) and torch.equal(L2, L1) and torch.equal(z2, z1)
    assert lib.apgp_potrf_mode(-1) == 0


def test_persistent_cholesky_two_streams_at_once(lib_loaded):
    """Two host threads evaluate on two streams at the same time.  A persistent launch needs all its workgroups
    resident; two of them can hold each other's CUs, in which case the bounded spins give up and the evaluation is
    redone on the launch-per-step path -- slower, never wrong, never hung: every result must be the single-stream one
    bit for bit, whichever path produced it."""
    import threading
    import torch
    lib = lib_loaded
    cases = [(1152, _persist_case(1152, 8, 5)), (900, _persist_case(900, 3, 6))]
    ref = [_nll_eval_raw(lib, torch, c[0], c[1], n, c[2], 0.0, 0) for n, c in cases]
    streams = [torch.cuda.Stream() for _ in cases]
    errors = []

    def worker(k):
        n, c = cases[k]
        try:
            with torch.cuda.stream(streams[k]):
                K = torch.zeros((n, n), dtype=torch.float64, device="cuda")
                z = torch.empty(n, dtype=torch.float64, device="cuda")
                info = torch.empty(1, dtype=torch.int32, device="cuda")
                o5 = torch.empty(5, dtype=torch.float64, device="cuda")
                o = np.empty(5)
                for _ in range(40):
                    rc = lib.apgp_nll_eval(c[0].data_ptr(), n, ctypes.byref(c[2]), c[1].data_ptr(), 0.0, K.data_ptr(), z.data_ptr(),
                                           info.data_ptr(), o5.data_ptr(), o.ctypes.data, ctypes.c_void_p(streams[k].cuda_stream))
                    assert rc == 0, lib.apgp_last_error()
                    streams[k].synchronize()
                    assert torch.equal(torch.tril(K), ref[k][0]) and torch.equal(z, ref[k][1]) and np.array_equal(o, ref[k][2])
        except BaseException as e:      # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    torch.cuda.synchronize()
    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(cases))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "an evaluation hangs"
    assert not errors, errors[0]


@pytest.mark.parametrize("trans", [0, 1])
# (320: a second super-block of one full sub-block; 577 = 9 * 64 + 1: a third super-block of one full and one 1-row
# sub-block -- the tile subtraction inside a super-block meets the ragged substitution)
@pytest.mark.parametrize("n", [256, 300, 320, 577, 1100, 1153, 2048, 4095, 8000])
def test_persistent_trsv_bit_identical_to_multi_launch(n, trans, lib_loaded):
    """K3 (george BasicSolver.apply_inverse on a vector: gpUtils.py:78, utility.py:131): the blocked triangular solve as
    ONE persistent launch (trsv_persist_kernel: a workgroup per 64-row block, solved blocks handed on as tagged granules,
    roles by ticket) against the launch-per-256-rows path -- x and x.x the same bits, forward and transposed, ld > n,
    b aliasing x -- and against LAPACK."""
    import torch
    lib = lib_loaded
    rs = np.random.RandomState(n)
    ld = n + (3 if n % 2 else 0)
    Lh = np.tril(rs.normal(size=(n, n)) * 0.05) + np.diag(1.0 + rs.uniform(size=n))
    Lbuf = np.zeros((n, ld)); Lbuf[:, :n] = Lh
    L = torch.from_numpy(Lbuf).cuda()
    b = torch.from_numpy(rs.normal(size=n)).cuda()

    def run(mode, alias):
        lib.apgp_trsv_mode(mode)
        try:
            x = b.clone() if alias else torch.empty(n, dtype=torch.float64, device="cuda")
            ss = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
            rc = lib.apgp_trsv(L.data_ptr(), n, ld, (x if alias else b).data_ptr(), 0.125, trans, x.data_ptr(), ss.data_ptr(), None)
            assert rc == 0, lib.apgp_last_error()
            torch.cuda.synchronize()
            return x, float(ss.item())
        finally:
            lib.apgp_trsv_mode(0)
    x1, s1 = run(1, False)
    for alias in (False, True):
        for _ in range(3):                                   # (repeated: tickets and tags are call-unique, never reset)
            x0, s0 = run(0, alias)
            assert torch.equal(x0, x1) and s0 == s1
    ref = np.linalg.solve(Lh.T if trans else Lh, b.cpu().numpy() - 0.125)
    assert np.abs(x1.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.isclose(s1, float(ref @ ref), rtol=1e-12)


def make_full_logdet(make, X):
    g = make()
    g.compute(X)
    return g.log_determinant


def test_incremental_factor_extension(lib_loaded):
    """Appending design points (approx.py:693-717): the O(N^2) factor extension
    (compute(x, previous=old_gp)) must agree with a full refactorisation, fall back
    to it when the hyper-parameters differ, and feed the same predictions."""
    go, agp = _mods()
    X, y = _synthetic(700, 8)
    def make():
        return agp.GP(kernel=agp.ExpSquaredKernel(np.full(8, 8.0), ndim=8), fit_mean=True,
                      mean=np.median(y), white_noise=-12, fit_white_noise=False)
    old = make(); old.compute(X[:690])
    ext = make()
    ext.extend_max_rows = 64              # (by cost, ten rows at N = 700 would be refactorised)
    ext.compute(X, previous=old)
    one = make(); one.compute(X[:691], previous=old)      # the default rule appends a single row (triangular solve)
    old._ensure_linv()                                    # with L^-1 resident the row is a matrix-vector product
    onew = make(); onew.compute(X[:691], previous=old)
    assert np.abs(onew._L[690].cpu().numpy() - one._L[690].cpu().numpy()).max() <= 1e-10 * np.abs(one._L[690].cpu().numpy()).max()
    assert one._L.shape == (691, 691) and np.isclose(one.log_determinant, make_full_logdet(make, X[:691]), rtol=1e-12)
    full = make(); full.compute(X)
    assert ext._L.shape == (700, 700)
    assert np.isclose(ext.log_determinant, full.log_determinant, rtol=1e-12)
    assert np.isclose(ext.log_likelihood(y), full.log_likelihood(y), rtol=1e-11)
    Le, Lf = np.tril(ext._L.cpu().numpy()), np.tril(full._L.cpu().numpy())
    assert np.abs(Le - Lf).max() <= 1e-11 * np.abs(Lf).max()
    cands = np.random.RandomState(4).uniform(-5, 5, size=(300, 8))
    me, ve = ext.predict(y, cands, return_var=True)
    mf, vf = full.predict(y, cands, return_var=True)
    assert np.allclose(me, mf, rtol=1e-10, atol=1e-10 * np.abs(mf).max()) and np.allclose(ve, vf, rtol=1e-9, atol=1e-12)
    # different hyper-parameters -> silently refactorises from scratch
    other = agp.GP(kernel=agp.ExpSquaredKernel(np.full(8, 7.0), ndim=8), fit_mean=True,
                   mean=np.median(y), white_noise=-12, fit_white_noise=False)
    other.compute(X, previous=old)
    ref = agp.GP(kernel=agp.ExpSquaredKernel(np.full(8, 7.0), ndim=8), fit_mean=True,
                 mean=np.median(y), white_noise=-12, fit_white_noise=False)
    ref.compute(X)
    assert np.isclose(other.log_determinant, ref.log_determinant, rtol=1e-13)
    # a duplicated point makes the extension fail exactly like a factorisation would
    dup = make()
    with pytest.raises(np.linalg.LinAlgError):
        bad = agp.GP(kernel=agp.ExpSquaredKernel(np.full(8, 8.0), ndim=8), fit_mean=True,
                     mean=0.0, white_noise=-800.0, fit_white_noise=False)
        bad.compute(X[:50])
        dup2 = agp.GP(kernel=agp.ExpSquaredKernel(np.full(8, 8.0), ndim=8), fit_mean=True,
                      mean=0.0, white_noise=-800.0, fit_white_noise=False)
        dup2.compute(np.vstack([X[:50], X[:1]]), previous=bad)
