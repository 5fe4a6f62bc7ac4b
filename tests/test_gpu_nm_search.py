# -*- coding: utf-8 -*-
"""MI355X: the restarted Nelder-Mead point search on the device (csrc/nmsearch.hip, GP.nelder_mead_search,
utility.minimizeObjective(onDevice=True), ApproxPosterior(deviceSearch=True)).

1. Replay: the device trace of every restart is teacher-forced through the NumPy restatement (tests/nm_ref.py, pinned to
   SciPy by tests/test_nm_ref.py): every evaluated point must be the replay's next point bit for bit given the device's
   own values, and every step, nfev, nit, status and the final x must be equal.
2. Evaluation: through the inverse at N <= 256 every traced (mu, sigma^2) is GP.predict's at that point bit for bit;
   elsewhere within a tolerance scaled by the condition estimate, and at N = 300 (FORM 1 / FORM 2 of nmsearch.hip) within
   the derived budgets of tests/nm_eval_ref.py against a long-double truth of the GP's own operand.  Each u is the host formula applied to (mu, sigma^2)
   within a few ulps, and +inf exactly where the point is outside the box.
3. End to end against the host path from the same NumPy seed.
4. The product: run / findMAP / bayesOpt / a JointPrior gate with deviceSearch=True."""
import os

import numpy as np
import pytest
from scipy.optimize import minimize
from scipy.stats import norm

import kvalue_ref as kr
import nm_eval_ref as ne
import nm_ref
import sweep_ref as sr
import util_ref

pytestmark = pytest.mark.gpu

KINDS = ("agp", "bape", "jones", "negmean")


def _bounds(D):
    return np.array([(-2.0 - 0.1 * d, 2.0 + 0.05 * d) for d in range(D)])


def _problem(D, n, fit_amp=True):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(500 + 31 * D + n)
    b = _bounds(D)
    X = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(size=(n, D))
    c = rs.uniform(-0.5, 0.5, D)
    y = -0.5 * np.sum((X - c) ** 2 / (0.3 + 0.1 * np.arange(D)), axis=1) + 0.2 * np.sin(2.0 * X[:, 0])
    metric = np.linspace(0.6, 1.6, D) * max(1.0, D / 2.0)
    k = agp.ExpSquaredKernel(metric, ndim=D)
    if fit_amp:
        k = 2.5 * k
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(np.median(y)), white_noise=-6.0, fit_white_noise=False)
    gp.compute(X)
    return y, gp, b


def _fixture(name):
    from approxposterior_amd import gp as agp
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    D = g["theta"].shape[1]
    p = g["p"]
    if int(g["fit_amp"]):
        k = agp.Product(agp.ConstantKernel(p[1], ndim=D), agp.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    else:
        k = agp.ExpSquaredKernel(np.exp(p[1:]), ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]), fit_white_noise=False)
    gp.compute(g["theta"])
    return g["y"], gp, np.column_stack([g["lo"], g["hi"]])


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _starts(b, R, seed):
    rs = np.random.RandomState(seed)
    return b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(0.1, 0.9, size=(R, len(b)))


def _replay(res, starts, options):
    x, fun, nfev, nit, status, recs = res
    for r, rec in enumerate(recs):
        rep = nm_ref.replay(rec["x"], rec["u"], starts[r], **options)
        assert rep["nfev"] == nfev[r] == len(rec["x"]), (r, rep["nfev"], nfev[r])
        assert rep["nit"] == nit[r] and rep["status"] == status[r], (r, rep["nit"], nit[r], rep["status"], status[r])
        assert rep["steps"] == rec["steps"], r
        assert np.array_equal(_bits(rep["x"]), _bits(x[r])), (r, rep["x"], x[r])
        assert np.array_equal(_bits(rep["fun"]), _bits(fun[r])), (r, rep["fun"], fun[r])


def _host_u(kind, mu, var, ybest, zeta=0.01):
    from approxposterior_amd import utility as ut
    with np.errstate(all="ignore"):
        if kind == "agp":
            return -(mu + 0.5 * np.log(2.0 * np.pi * np.e * var))
        if kind == "bape":
            return np.array([-((2.0 * m + v) + ut.logsubexp(v, 0.0)) for m, v in zip(mu, var)])
        if kind == "jones":
            out = np.zeros_like(mu)
            sd = np.sqrt(var)
            ok = sd > 0
            z = (mu[ok] - ybest - zeta) / sd[ok]
            out[ok] = -((mu[ok] - ybest - zeta) * norm.cdf(z) + sd[ok] * norm.pdf(z))
            return out
        return np.where(np.isfinite(mu), -mu, np.inf)


def _check_evaluations(gp, y, rec, kind, b, exact, budget=None):
    xs = rec["x"]
    inside = np.all(np.isfinite(xs), axis=1) & np.all((xs >= b[:, 0]) & (xs <= b[:, 1]), axis=1)
    assert np.all(np.isposinf(rec["u"][~inside]))
    assert np.all(np.isnan(rec["mu"][~inside]))
    if not inside.any():
        return
    pts = xs[inside]
    mu_d, var_d, u_d = rec["mu"][inside], rec["var"][inside], rec["u"][inside]
    if exact:
        host = np.array([np.concatenate(gp.predict(y, p.reshape(1, -1), return_var=True)) for p in pts])
        assert np.array_equal(_bits(mu_d), _bits(host[:, 0]))
        assert np.array_equal(_bits(var_d), _bits(host[:, 1]))
    else:
        mu_h, var_h = gp.predict(y, pts, return_var=True)
        amp = float(gp._kernel_struct().amp)
        scale = max(1.0, float(np.max(np.abs(y))))
        cond = max(1.0, float(gp.cond_estimate))
        assert np.allclose(mu_d, mu_h, rtol=1e-9, atol=1e-9 * scale * max(1.0, cond * 1e-6))
        assert np.allclose(var_d, var_h, rtol=1e-7, atol=64 * np.finfo(float).eps * amp * cond + 1e-12 * amp)
        if budget is not None:
            _check_budget(gp, pts[:64], mu_d[:64], var_d[:64], budget)
    want = _host_u(kind, mu_d, var_d, float(np.max(y)))
    both = np.isfinite(want) & np.isfinite(u_d)
    assert np.array_equal(np.isfinite(want), np.isfinite(u_d))
    tol = 1e-12 * (1.0 + np.abs(mu_d) + np.abs(var_d) + abs(float(np.max(y))))
    if kind == "bape":
        # log(1 - exp(-var)): a one-ulp difference of exp() is amplified by 1 / var for small var
        tol = tol + 8.0 * np.finfo(float).eps / np.maximum(np.abs(var_d), 1e-300)
    assert np.all(np.abs(u_d[both] - want[both]) <= tol[both]), np.max(np.abs(u_d[both] - want[both]) / tol[both])
    if kind in util_ref.KINDS:
        # against the 60-digit truth of the device's own (mu, sigma^2), within the smaller of the tolerance above and the
        # forward-error bound of the formula (tests/util_ref.py); NaN / +inf / 0.0 by class
        ybest = float(np.max(y))
        for i in range(len(u_d)):
            cls, r = util_ref.judge(kind, u_d[i], mu_d[i], var_d[i], 0.01, ybest)
            assert r <= 1.0, (kind, i, cls, r, u_d[i], mu_d[i], var_d[i])
            b = util_ref.bound(kind, mu_d[i], var_d[i], 0.01, ybest)
            if cls == "value" and b is not None:
                assert r * b <= tol[i], (kind, i, r * b, tol[i], u_d[i], mu_d[i], var_d[i])


def _check_budget(gp, pts, mu_d, var_d, form):
    """(mu, sigma^2) of the evaluations at ``pts`` against the long-double truth built from the bits the kernel was
    handed -- the GP's own operand (the dense inverse or the factor) and its packed training image, both read back --
    within the budgets of tests/nm_eval_ref.py (FORM 1 / FORM 2 of csrc/nmsearch.hip)."""
    n, D = gp._x.shape
    ks = gp._kernel_struct()
    k = kr.Kern(D, float(ks.amp), 0.0, np.array(ks.inv_metric[:D], dtype=np.float64), float(ks.lin_coef), int(ks.lin_order))
    dpad = kr.dpad(D)
    img = gp._xs.cpu().numpy().reshape(-1, dpad + 2)[:n]
    X = np.ascontiguousarray(gp._x, dtype=np.float64)
    assert np.array_equal(_bits(img[:, :D]), _bits(X * np.sqrt(0.5 * k.inv_metric))), "the image is not of these points"
    assert not img[:, D:dpad].any()
    alpha = img[:, dpad].copy()
    if form == "inverse":
        assert n > 256, "FORM 1 runs above 256 points"
        ldw = (n + 63) // 64 * 64
        A = gp._work.cpu().numpy()[:n * ldw].reshape(n, ldw)[:, :n]
        la = None
    else:
        A = gp._L.cpu().numpy()
        A = A[:n, :n] if A.ndim == 2 else A.reshape(-1)[:n * gp._ld].reshape(n, gp._ld)[:, :n]
        la = np.abs(sr.inv_ld(A)).astype(np.float64) * (1.0 + 1e-9)
    truth = ne.Truth(A, X, alpha, pts, k, float(gp.mean.value), form=form, linv_abs=la)
    rm, rv = truth.ratios(mu_d, var_d)
    print("nm %-7s real GP n=%d D=%d: worst |mu - truth| / budget %.3f, |var - truth| / budget %.3f over %d evaluations; "
          "guards %s" % (form, n, D, rm, rv, len(pts), "%.3g %.1f %d" % truth.guards()))
    assert rm <= 1.0 and rv <= 1.0, (form, n, D, rm, rv)


CASES = [(n, form) for n in (50, 90, 256, 300, 1152) for form in ("inverse", "solve")]


@pytest.mark.parametrize("n,form", CASES, ids=["n%d-%s" % c for c in CASES])
def test_replay_and_evaluations(n, form):
    for D in (1, 2, 5, 8):
        y, gp, b = _problem(D, n, fit_amp=(D % 2 == 0))
        gp.variance_mode = form
        for j, kind in enumerate(KINDS):
            starts = _starts(b, 3, 10 * D + j)
            if j == 1:
                starts[2, 0] = 0.0                           # a zero coordinate: 0.00025 in the first simplex
            if j == 2:
                starts[1] = b[:, 1] - 1e-3 * (b[:, 1] - b[:, 0])   # near a face: the simplex leaves the box
            options = {"adaptive": True}
            if j == 3:
                options["maxfev"] = 40 + 3 * D                 # stops mid-iteration
            res = gp.nelder_mead_search(y, starts, kind, bounds=b, options=options, trace=True)
            _replay(res, starts, options)
            for r, rec in enumerate(res[5]):
                # N = 300 is past the single-launch body: the first restart of the first kind is held to the budget too
                _check_evaluations(gp, y, rec, kind, b, exact=(form == "inverse" and n <= 256),
                                   budget=form if (n == 300 and j == 0 and r == 0) else None)


@pytest.mark.parametrize("form", ["inverse", "solve"])
def test_replay_on_the_ill_conditioned_fixture(form):
    y, gp, b = _fixture("rosen2d_n50_amp_cond1e13")
    gp.variance_mode = form
    for kind in KINDS:
        starts = _starts(b, 4, 3)
        res = gp.nelder_mead_search(y, starts, kind, bounds=b, options={"adaptive": True}, trace=True)
        _replay(res, starts, {"adaptive": True})
        for rec in res[5]:
            _check_evaluations(gp, y, rec, kind, b, exact=(form == "inverse"))


def test_default_gate_picks_the_form_of_predict():
    # without variance_mode: the solve form on the fitAmp optimum's conditioning, the inverse on a tame set -- each
    # bit-identical to predict at N <= 256 through the inverse, within tolerance through the factor
    for name in ("rosen2d_n50_amp_cond1e13", "rosen2d_n50_noamp"):
        y, gp, b = _fixture(name)
        res = gp.nelder_mead_search(y, _starts(b, 2, 1), "bape", bounds=b, options={"adaptive": True}, trace=True)
        _replay(res, _starts(b, 2, 1), {"adaptive": True})
        for rec in res[5]:
            _check_evaluations(gp, y, rec, "bape", b, exact=gp._trust_inverse())


def test_linear_kernel_term():
    from approxposterior_amd import gp as agp
    y, _, b = _problem(2, 90)
    rs = np.random.RandomState(500 + 31 * 2 + 90)
    X = b[:, 0] + (b[:, 1] - b[:, 0]) * rs.uniform(size=(90, 2))
    k = 2.5 * agp.ExpSquaredKernel(np.array([0.6, 1.6]), ndim=2) + \
        0.3 * agp.kernels.LinearKernel(log_gamma2=0.4, order=2, bounds=None, ndim=2)
    gp = agp.GP(kernel=k, fit_mean=True, mean=float(np.median(y)), white_noise=-6.0, fit_white_noise=False)
    gp.compute(X)
    for form in ("inverse", "solve"):
        gp.variance_mode = form
        starts = _starts(b, 3, 4)
        res = gp.nelder_mead_search(y, starts, "agp", bounds=b, options={"adaptive": True}, trace=True)
        _replay(res, starts, {"adaptive": True})
        for rec in res[5]:
            _check_evaluations(gp, y, rec, "agp", b, exact=(form == "inverse"))


def _near_tie(values):
    v = np.asarray(values, dtype=float)
    v = v[np.isfinite(v)]
    if len(v) < 2:
        return False
    d = np.diff(np.sort(v))
    return bool(np.any(d <= 1e-9 * np.maximum(1.0, np.abs(np.sort(v)[1:]))))


def test_end_to_end_against_the_host_path():
    """Same NumPy seed -> the same starts; per restart, the host search (SciPy over the host utility) and the device
    search end at the same point to 1e-8 of the box span unless a last-bit comparison flipped (the utility formulas
    differ by a few ulps between NumPy and the device).  Restarts whose device trace has a near-tie are not held to it;
    the others may diverge at most twice in the 16."""
    from approxposterior_amd import utility as ut
    y, gp, b = _problem(2, 90)
    gp.variance_mode = "inverse"

    def prior(x):
        x = np.ravel(x)
        return 0.0 if np.all((x >= b[:, 0]) & (x <= b[:, 1])) else -np.inf

    drawn = []

    def sample(m):
        s = b[:, 0] + (b[:, 1] - b[:, 0]) * np.random.uniform(size=(m, 2))
        drawn.append(np.ravel(s).copy())
        return s

    np.random.seed(21)
    with np.errstate(all="ignore"):
        ph, vh = ut.minimizeObjective(ut.AGPUtility, y, gp, sample, prior, nRestarts=16, args=(y, gp, prior))
    host_starts = np.array(drawn)
    drawn.clear()
    np.random.seed(21)
    with np.errstate(all="ignore"):
        pd, vd = ut.minimizeObjective(ut.AGPUtility, y, gp, sample, prior, nRestarts=16, args=(y, gp, prior),
                                      onDevice=True, bounds=b)
    assert np.array_equal(np.array(drawn), host_starts)
    span = float(np.max(b[:, 1] - b[:, 0]))
    res = gp.nelder_mead_search(y, host_starts, "agp", bounds=b, options={"adaptive": True}, trace=True)
    diverged = []
    for r, x0 in enumerate(host_starts):
        with np.errstate(all="ignore"):
            hx = minimize(lambda x: float(np.ravel(ut.AGPUtility(x, y, gp, prior))[0]), x0, method="nelder-mead",
                          options={"adaptive": True}).x
        if np.max(np.abs(hx - res[0][r])) > 1e-8 * span:
            diverged.append((r, _near_tie(res[5][r]["u"]), hx, res[0][r]))
    print("restarts that diverged (restart, near-tie in the trace, host x, device x):", diverged)
    assert sum(1 for d in diverged if not d[1]) <= 2, diverged
    # the restarts' solutions are found again by the wrapper, which returns the host utility at the best one
    assert np.isfinite(float(np.ravel(vd)[0]))
    if not diverged:
        assert np.allclose(pd, ph, atol=1e-8 * span)


def test_run_c1_shaped_with_device_search(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    np.random.seed(57)
    theta = lh.rosenbrockSample(50)
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y, white_noise=-12)
    ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                priorSample=lh.rosenbrockSample, bounds=[(-5, 5), (-5, 5)], algorithm="bape")
    with np.errstate(all="ignore"):
        ap.run(m=5, nmax=1, estBurnin=True, nGPRestarts=1, mcmcKwargs={"iterations": 2000}, cache=False,
               samplerKwargs={"nwalkers": 20}, verbose=False, thinChains=False, onlyLastMCMC=True, deviceSearch=True)
    assert ap.deviceSearch is True and len(ap.y) == 55
    new = ap.theta[50:]
    assert np.all(np.isfinite(new)) and np.all(np.abs(new) <= 5)


def test_find_map_sphere_matches_host(tmp_path, monkeypatch):
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
        ap.findNextPoint(numNewPoints=5, nGPRestarts=3, cache=False, verbose=False)
        np.random.seed(3)
        hostMAP, hostVal = ap.findMAP(nRestarts=15)
        np.random.seed(3)
        devMAP, devVal = ap.findMAP(nRestarts=15, deviceSearch=True)
    assert ap.deviceSearch is False                  # a findMAP argument does not change the object's setting
    assert np.allclose(devMAP, hostMAP, atol=1e-3) and np.allclose(devMAP, [0.0, 0.0], atol=1e-3)
    assert np.allclose(devVal, hostVal, atol=1e-3)


def test_bayesopt_1d_device_search(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from approxposterior_amd import approx, gpUtils, likelihood as lh

    def setup():
        np.random.seed(57)
        theta = lh.testBOFnSample(3)
        y = np.array([lh.testBOFn(t) + lh.testBOFnLnPrior(t) for t in theta])
        gp = gpUtils.defaultGP(theta, y, fitAmp=True)
        return approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.testBOFnLnPrior, lnlike=lh.testBOFn,
                                      priorSample=lh.testBOFnSample, bounds=[[-1, 2]], algorithm="jones")

    kw = dict(nmax=10, tol=1.0e-3, seed=57, verbose=False, cache=False, gpMethod="powell", optGPEveryN=1,
              nGPRestarts=3, nMinObjRestarts=5, initGPOpt=True, minObjMethod="nelder-mead", findMAP=True)
    with np.errstate(all="ignore"):
        host = setup().bayesOpt(**kw)
        ap = setup()
        dev = ap.bayesOpt(deviceSearch=True, **kw)
    assert np.allclose(dev["thetaBest"], host["thetaBest"], rtol=5.0e-2)
    assert np.allclose(dev["valBest"], host["valBest"], rtol=5.0e-2)
    # (the two runs' surrogates differ once a design point does, so their MAP histories do too: the MAP search itself is
    # compared on the device run's final surrogate, host against device from the same random state)
    with np.errstate(all="ignore"):
        np.random.seed(4)
        hmap, hval = ap.findMAP(nRestarts=5, deviceSearch=False)
        np.random.seed(4)
        dmap, dval = ap.findMAP(nRestarts=5, deviceSearch=True)
    assert np.allclose(dmap, hmap, atol=1e-3) and np.allclose(dval, hval, rtol=1e-6, atol=1e-9)


def test_joint_prior_gates_on_its_support(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from approxposterior_amd import approx, gpUtils, likelihood as lh, priors
    jp = priors.JointPrior([priors.UniformPrior(-1.0, 1.5), priors.GaussianPrior(0.5, 1.0)])
    np.random.seed(8)
    theta = np.array(jp.sample(30))
    y = np.array([lh.sphereLnlike(t) + jp(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y, fitAmp=True)
    ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=jp, lnlike=lh.sphereLnlike, priorSample=jp.sample,
                                bounds=jp.bounds(), algorithm="bape")
    with np.errstate(all="ignore"):
        pts = ap.findNextPoint(computeLnLike=False, numNewPoints=3, deviceSearch=True, verbose=False, cache=False)
    pts = np.atleast_2d(pts)
    assert np.all(np.isfinite(pts)) and np.all((pts[:, 0] >= -1.0) & (pts[:, 0] <= 1.5))
    # the gate itself: points outside the Uniform factor get +inf and no prediction
    gate = [tuple(r) for r in jp.support()]
    res = ap.gp.nelder_mead_search(ap.y, np.array([[1.49, 0.0], [-0.5, 3.0]]), "bape", bounds=gate,
                                   options={"adaptive": True}, trace=True)
    for rec in res[5]:
        out = (rec["x"][:, 0] < -1.0) | (rec["x"][:, 0] > 1.5)
        assert np.all(np.isposinf(rec["u"][out])) and np.all(np.isfinite(rec["mu"][~out]))
    assert np.all((res[0][:, 0] >= -1.0) & (res[0][:, 0] <= 1.5))
