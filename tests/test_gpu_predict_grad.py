"""GPU tests of ``apgp_predict_grad`` / ``GP.predict_grad`` and of the exact-gradient point search (run with ``-m gpu``).

Bounds.  eps = 2.2e-16, cond the condition number of K, 200 the constant of tests/test_gpu_parity.py's header:
    dmu  : |d| <= 200 cond eps S_mu,   S_mu[d]  = sum_n |alpha_n J_nd|
    dvar : |d| <= 200 cond eps S_var,  S_var[d] = |d k(t,t)/d t_d| + 2 sum_n |w_n J_nd|
per component, against the 60-digit truth of tests/golden/predgrad_truth.npz on the fixtures and against the NumPy
restatement (tests/predgrad_ref.py, which tests/test_predgrad_ref.py holds to the same bound) on seeded shapes.
mu / var: NOT bit-equal to ``predict(return_var=True)`` -- the gradient kernels sum v = W k and k.alpha in their own
fixed order (two rows of W per wavefront, 2 x 64 running sums), not in apgp_predict1_host's -- so they are held to
the mu / var bounds of tests/test_gpu_parity.py: 200 cond eps sum|alpha| amp and 200 cond eps amp.

Tiles of the implementation the shapes straddle (csrc/predgrad.hip): 8 points per workgroup through the inverse (m = 7,
8, 9, 63..65), 4 through the factor (m = 3, 4, 5); 8 rows of W per workgroup of the forward product and two per
wavefront (N = 1, 7, 9, odd N); 64 columns per workgroup of the transposed product and 64-row blocks of the
substitutions (N = 63, 64, 65, 255..257); 512-row chunks of the transposed product (N = 513, 520: two chunks); 8
dimensions per workgroup of the last kernel (D = 8, 9, 17, 32); 4096 points per chunk of the call (m = 4100).
"""
import os

import numpy as np
import pytest

import predgrad_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
WELL = ["rosen2d_n50_noamp", "rosen2d_n50_amp", "c2small_d2_n200", "c3small_d8_n300", "d5_n130_amp"]
LADDER = ["rosen2d_n50_amp_cond1e8", "rosen2d_n50_amp_cond1e11", "rosen2d_n50_amp_cond1e13"]


@pytest.fixture(scope="module")
def truth(golden_dir):
    return np.load(os.path.join(golden_dir, "predgrad_truth.npz"))


def _fixture_gp(golden_dir, name):
    from approxposterior_amd import gp as agp
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    D = g["theta"].shape[1]
    p = g["p"]
    if int(g["fit_amp"]):
        k = agp.Product(agp.ConstantKernel(p[1], ndim=D), agp.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    else:
        k = agp.ExpSquaredKernel(np.exp(p[1:]), ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]), fit_white_noise=False)
    gp.compute(g["theta"])
    return g, gp


# ---- truth parity on the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WELL + LADDER)
def test_truth_parity(golden_dir, truth, name):
    from approxposterior_amd import gp as agp
    g, gp = _fixture_gp(golden_dir, name)
    y, T = g["y"], truth[name + "/T"]
    tol = 200 * float(g["cond"]) * EPS
    amp = ref.fixture_params(g)["amp"]
    scale = np.abs(g["alpha"]).sum() * amp
    by_gate = "inverse" if gp._trust_inverse() else "solve"
    assert gp._trust_inverse() == (gp.cond_estimate <= agp.COND_SOLVE)
    if name == "rosen2d_n50_amp_cond1e13":
        assert by_gate == "solve"                       # (estimate 2.9e10: the one rung above COND_SOLVE)
    modes = [None] + ([{"inverse": "solve", "solve": "inverse"}[by_gate]] if name in WELL else [])
    for mode in modes:
        gp.variance_mode = mode
        mu, var, dmu, dvar = gp.predict_grad(y, T)
        if mode is None and by_gate == "solve":
            assert gp._packed is None and gp._work is None      # no inverse was formed: the factor route ran
        rmu = np.abs(dmu - truth[name + "/dmu"]) / (tol * truth[name + "/S_mu"])
        rvar = np.abs(dvar - truth[name + "/dvar"]) / (tol * truth[name + "/S_var"])
        print(name, mode or by_gate, "dmu %.3g, dvar %.3g of the bound" % (rmu.max(), rvar.max()))
        assert rmu.max() <= 1.0 and rvar.max() <= 1.0, (mode, float(rmu.max()), float(rvar.max()))
        assert np.abs(mu - truth[name + "/mu"]).max() <= max(1e-13, tol) * scale
        assert np.abs(var - truth[name + "/var"]).max() <= max(1e-14, tol) * amp
        # the single-point prediction at the same point, to the same bounds (see the header: not bit-equal)
        m1, v1 = gp.predict(y, T[:1].copy(), return_var=True)
        assert abs(m1[0] - mu[0]) <= 2 * max(1e-13, tol) * scale and abs(v1[0] - var[0]) <= 2 * max(1e-14, tol) * amp


# ---- shapes where the kernels can go wrong ----------------------------------------------------------------------------------
# (N, D, m, fitAmp, order of an added LinearKernel or 0)
SHAPES = [(1, 1, 1, 0, 0), (7, 2, 3, 1, 1), (9, 3, 4, 0, 2), (63, 2, 2, 1, 0), (64, 3, 63, 0, 1), (65, 8, 64, 1, 2),
          (255, 9, 65, 0, 0), (256, 17, 130, 1, 0), (257, 32, 9, 0, 1), (513, 2, 7, 1, 0), (520, 8, 5, 0, 2),
          (65, 3, 4100, 0, 0)]


def _seeded(N, D, fit_amp, lin):
    """A seeded training set with a metric short enough for cond(K) <= 1e6, its GP and the restatement's parameters."""
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(1000 * N + 10 * D + lin)
    X = rs.uniform(-2, 2, size=(N, D))
    y = np.sin(X.sum(axis=1)) + 0.1 * rs.randn(N)
    logM = np.log(np.full(D, 0.05 * D) * rs.uniform(0.8, 1.25, size=D))
    k = agp.ExpSquaredKernel(np.exp(logM), ndim=D)
    lc = lt = None
    if fit_amp:
        lc = np.log(1.7 / D)
        k = agp.ConstantKernel(lc, ndim=D) * k
    if lin:
        lt = (np.log(0.3 / D), 0.2, lin)
        k = k + agp.ConstantKernel(lt[0], ndim=D) * agp.LinearKernel(log_gamma2=lt[1], order=lin, ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=0.1, white_noise=-8.0, fit_white_noise=False)
    gp.compute(X)
    prm = ref.params(D, logM, log_constant=lc, white_noise=-8.0, mean=0.1, lin=lt)
    return gp, X, y, prm, rs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-D%d-m%d-amp%d-lin%d" % s)
def test_shapes_against_the_restatement(shape):
    N, D, m, fit_amp, lin = shape
    gp, X, y, prm, rs = _seeded(N, D, fit_amp, lin)
    cond = np.linalg.cond(ref.gram(X, prm))
    assert cond <= 1e6
    tol = 200 * cond * EPS
    T = rs.uniform(-2, 2, size=(m, D))
    alpha_sum = None
    for mode in ("inverse", "solve"):
        gp.variance_mode = mode
        mu, var, dmu, dvar = gp.predict_grad(y, T)
        rm, rv, rdm, rdv, s_mu, s_var = ref.posterior(T, X, y, prm, route=mode, scales=True)
        if alpha_sum is None:
            alpha_sum = np.abs(gp._alpha.cpu().numpy()).sum()
        ktt = ref.kernel_diag(T, prm)[0]
        e_mu, e_var = np.abs(dmu - rdm) / (tol * s_mu), np.abs(dvar - rdv) / (tol * s_var)
        print(shape, mode, "cond %.3g: dmu %.3g, dvar %.3g of the bound" % (cond, e_mu.max(), e_var.max()))
        assert dmu.shape == (m, D) and dvar.shape == (m, D)
        assert e_mu.max() <= 1.0 and e_var.max() <= 1.0, (mode, float(e_mu.max()), float(e_var.max()))
        assert np.abs(mu - rm).max() <= max(1e-13, tol) * alpha_sum * ktt.max()
        assert (np.abs(var - rv) <= max(1e-14, tol) * ktt).all()


# ---- utilities ----------------------------------------------------------------------------------------------------------------
def _propagated(kind, tmu, tvar, var):
    """tests/test_gpu_parity.py: the mu / var tolerances through each utility's own derivative."""
    vr = np.maximum(var, 1e-300)
    if kind == "agp":
        return tmu + 0.5 * tvar / vr
    if kind == "bape":
        return 2 * tmu + tvar * (1.0 + 1.0 / np.expm1(vr))
    return tmu + 0.2 * tvar / np.sqrt(vr)


@pytest.mark.parametrize("name", ["rosen2d_n50_noamp", "d5_n130_amp", "c3small_d8_n300"])
def test_utilities_against_the_sweep_and_the_restatement(golden_dir, name):
    g, gp = _fixture_gp(golden_dir, name)
    y, T = g["y"], np.ascontiguousarray(g["cands"][:40])
    X, prm = g["theta"], ref.fixture_params(g)
    bounds = list(zip(g["lo"], g["hi"]))
    tol = 200 * float(g["cond"]) * EPS
    tmu = max(1e-13, tol) * np.abs(g["alpha"]).sum() * prm["amp"]
    tvar = max(1e-14, tol) * prm["amp"]
    ybest = float(np.max(y))
    _, _, rdm, rdv, s_mu, s_var = ref.posterior(T, X, y, prm, scales=True)
    for kind in ("agp", "bape", "jones"):
        u, du, mu, var = gp.predict_grad(y, T, kind=kind, bounds=bounds)
        _, _, us, mus, vars_ = gp.acquire(y, T, kind, bounds=bounds, return_all=True)
        fin = np.isfinite(us)
        assert np.array_equal(np.isposinf(u), np.isposinf(us)) and np.array_equal(np.isnan(u), np.isnan(us))
        tu = _propagated(kind, tmu, tvar, vars_[fin])
        assert (np.abs(u[fin] - us[fin]) <= 4 * tu + 1e-11 * np.abs(us[fin])).all(), kind
        # du: the restatement's chain rule with the utility's derivatives taken at the device's own (mu, var) -- so the
        # bound is the gradients' (200 cond eps S, weighted) plus 64 eps (1 + z^2) of each term for the handful of
        # operations and library functions (erfc 16 ulp, exp, expm1) in the two derivative factors
        _, g_mu, g_var, flat = ref.utility(kind, mu, var, ybest=ybest)
        inside = np.isfinite(mu)
        want = np.where((flat | ~inside)[:, None], 0.0, g_mu[:, None] * rdm + g_var[:, None] * rdv)
        z2 = ((mu - ybest - 0.01) ** 2 / np.maximum(var, 1e-300))[:, None] if kind == "jones" else 0.0
        bound = (np.abs(g_mu)[:, None] * (tol * s_mu + 64 * EPS * (1 + z2) * np.abs(rdm))
                 + np.abs(g_var)[:, None] * (tol * s_var + 64 * EPS * (1 + z2) * np.abs(rdv)))
        ok = inside & ~flat
        err = np.abs(du - want)
        print(name, kind, "du: %.3g of the bound" % (err[ok] / bound[ok]).max())
        assert (err[ok] <= bound[ok]).all(), kind
        assert np.all(du[~ok] == 0.0)
    # -mu
    u, du, mu, var = gp.predict_grad(y, T, kind="negmean")
    mu2, var2, dmu, dvar = gp.predict_grad(y, T)
    assert np.array_equal(u, -mu) and np.array_equal(du, -dmu) and np.array_equal(mu, mu2) and np.array_equal(var, var2)


def test_non_finite_table(golden_dir):
    from approxposterior_amd import gp as agp
    g, gp = _fixture_gp(golden_dir, "rosen2d_n50_noamp")
    y = g["y"]
    lo, hi = g["lo"], g["hi"]
    mid = 0.5 * (lo + hi)
    T = np.array([mid, [np.nan, mid[1]], [hi[0] + 1.0, mid[1]], [mid[0], np.inf], mid])
    for kind in ("agp", "bape", "jones", "negmean"):
        u, du, mu, var = gp.predict_grad(y, T, kind=kind, bounds=list(zip(lo, hi)))
        assert np.all(np.isfinite(u[[0, 4]])) and np.all(np.isfinite(du[[0, 4]]))
        assert np.all(np.isposinf(u[1:4])) and np.all(du[1:4] == 0.0)
        assert np.all(np.isnan(mu[1:4])) and np.all(np.isnan(var[1:4]))
    mu, var, dmu, dvar = gp.predict_grad(y, T, bounds=list(zip(lo, hi)))
    assert np.all(np.isnan(dmu[1:4])) and np.all(np.isnan(dvar[1:4])) and np.all(np.isfinite(dmu[[0, 4]]))
    # without a box only the non-finite rows are refused
    mu, var, dmu, dvar = gp.predict_grad(y, T)
    assert np.isnan(mu[[1, 3]]).all() and np.isfinite(mu[2]) and np.isfinite(dvar[2]).all()
    # sigma^2 at the training points of a noise-free model (exp(-40) is lost in K_ii = 1): 1 - |v|^2 is a few units of
    # 2^-53 around zero, of either sign or exactly zero (in NumPy: 13 negative, 24 zero, 27 positive of these 64)
    rs = np.random.RandomState(4)
    X = rs.uniform(-1, 1, size=(64, 2))
    yy = np.sin(X[:, 0]) * X[:, 1]
    gp2 = agp.GP(kernel=agp.ExpSquaredKernel([0.1, 0.1], ndim=2), fit_mean=True, mean=0.0, white_noise=-40.0,
                 fit_white_noise=False)
    gp2.compute(X)
    res = {kind: gp2.predict_grad(yy, X, kind=kind) for kind in ("agp", "bape", "jones")}
    var = res["agp"][3]
    neg, nonpos = var < 0, var <= 0
    assert neg.any() and (~nonpos).any()
    u, du = res["bape"][:2]
    assert np.all(np.isposinf(u[nonpos])) and np.all(du[nonpos] == 0.0) and np.all(np.isfinite(u[~nonpos]))
    u, du = res["jones"][:2]
    assert np.all(u[nonpos] == 0.0) and np.all(du[nonpos] == 0.0)
    u, du = res["agp"][:2]
    assert np.all(np.isnan(u[neg])) and np.all(np.isnan(du[neg])) and np.all(np.isfinite(du[~nonpos]))


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["inverse", "solve"])
def test_same_bits_twice_and_batch_equals_single_calls(mode):
    """A point's arithmetic does not depend on the block of points it travels in (8 and 4 per workgroup, or alone), so a
    batch returns the bits of the single-point calls -- the replayed single-point call included."""
    gp, X, y, prm, rs = _seeded(300, 5, 1, 1)
    gp.variance_mode = mode
    T = rs.uniform(-2, 2, size=(21, 5))
    first = gp.predict_grad(y, T, kind="bape")
    again = gp.predict_grad(y, T, kind="bape")
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for i in range(len(T)):
        one = gp.predict_grad(y, T[i].copy(), kind="bape")          # (from the second on: the kept argument list)
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(one, first)), i
    assert "pgrad" in gp._replays
    dev = gp.predict_grad(y, T, kind="bape", return_device=True)
    assert all(np.array_equal(d.cpu().numpy(), a) for d, a in zip(dev, first))


# ---- the exact-gradient search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rosen2d_n50_noamp", "c3small_d8_n300"])
def test_search_with_exact_gradients(golden_dir, name):
    """BAPE under the fixture's box prior, three restarts.  ``bounds`` are not forwarded for "l-bfgs-b" (the reference's
    rule), so the prior is a wall of +inf, and SciPy's L-BFGS-B ends a run at its last finite iterate as soon as a line
    search steps into it ("relative reduction of f"), with exact and with differenced gradients alike: such a run is
    neither stationary nor on the bound (from draws over the whole box two of three runs on the Rosenbrock fixture end
    that way, in NumPy too).  The starts are therefore drawn from the inner half of the box, where the first, unit-length
    step of a run cannot leave it; the best of the three is then a run that converged inside."""
    from approxposterior_amd import utility as ut
    g, gp = _fixture_gp(golden_dir, name)
    y, lo, hi = g["y"], g["lo"], g["hi"]
    D = len(lo)

    def prior(x):
        x = np.asarray(x).ravel()
        return 0.0 if np.all((x >= lo) & (x <= hi)) else -np.inf

    def sample(n):      # the inner half of the box, see the docstring
        return np.random.uniform(0.75 * lo + 0.25 * hi, 0.25 * lo + 0.75 * hi, size=(n, D))

    out = {}
    for jac in (True, False):
        np.random.seed(21)
        with np.errstate(all="ignore"):
            x, val = ut.minimizeObjective(ut.BAPEUtility, y, gp, sample, prior, nRestarts=3, method="l-bfgs-b",
                                          args=(y, gp, prior), jac=jac)
        out[jac] = (x, float(np.ravel(val)[0]))
    x, val = out[True]
    print(name, "jac=True: u = %.10g at %s; jac=False: u = %.10g" % (val, x, out[False][1]))
    assert np.isfinite(prior(x))
    assert val <= out[False][1] + 1e-6 * abs(out[False][1])
    # stationary to 1e-3 of the scale of the sums the gradient is made of, or on the box
    u, du, mu, var = gp.predict_grad(y, x, kind="bape")
    prm = ref.fixture_params(g)
    _, _, _, _, s_mu, s_var = ref.posterior(x, g["theta"], y, prm, scales=True)
    _, g_mu, g_var, _ = ref.utility("bape", mu, var)
    scale = np.abs(g_mu)[:, None] * s_mu + np.abs(g_var)[:, None] * s_var
    on_box = (np.abs(x - lo) <= 1e-9 * (hi - lo)) | (np.abs(x - hi) <= 1e-9 * (hi - lo))
    print(name, "|du| / scale:", np.abs(du[0]) / scale[0])
    assert np.all((np.abs(du[0]) <= 1e-3 * scale[0]) | on_box)


def test_find_next_point_and_find_map_with_exact_gradients(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    np.random.seed(57)
    theta = np.array(lh.sphereSample(20))
    y = np.array([lh.sphereLnlike(t) + lh.sphereLnprior(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y, fitAmp=True)
    ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.sphereLnprior, lnlike=lh.sphereLnlike,
                                priorSample=lh.sphereSample, bounds=[(-5, 5), (-5, 5)], algorithm="jones")
    with np.errstate(all="ignore"):
        ap.optGP(seed=57, method="powell", nGPRestarts=3)
        ap.findNextPoint(numNewPoints=5, nGPRestarts=3, cache=False, verbose=False, searchJac=True,
                         minObjMethod="l-bfgs-b")
        assert ap.theta.shape == (25, 2) and np.all(np.isfinite(ap.y))
        assert all(np.isfinite(lh.sphereLnprior(t)) for t in ap.theta[20:])
        testMAP, testVal = ap.findMAP(nRestarts=15, method="l-bfgs-b", searchJac=True)
    assert np.allclose([0.0, 0.0], testMAP, atol=1.0e-3)
    assert np.allclose(0.0, testVal, atol=1.0e-3)
    with pytest.raises(ValueError):
        ap.findNextPoint(computeLnLike=False, verbose=False, cache=False, searchJac=True)      # Nelder-Mead takes no gradient
