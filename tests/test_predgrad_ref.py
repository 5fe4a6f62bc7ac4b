"""CPU tests of the predictive-gradient restatement (tests/predgrad_ref.py) and of ``utility.minimizeObjective(jac=True)``.

* the float64 restatement against the 60-digit truth of tests/golden/predgrad_truth.npz (tools/make_predgrad_golden.py)
  within the bound the GPU tests hold the device to: per component
      |dmu - truth| <= 200 cond eps S_mu,   |dvar - truth| <= 200 cond eps S_var,
  S the sums of absolute terms stored with the truth, cond the fixture's condition number, 200 the constant of
  tests/test_gpu_parity.py's header.  If the restatement left the bound on a point, the bound would be dishonest.
* its gradients against central differences of the oracle's ``predict`` and of tests/util_ref.py's utilities on the
  well-conditioned fixtures, step h = 1e-5 x the box width.  Derived bound of |cd(h) - g| per component:
      2/3 |cd(2h) - cd(h)|      truncation: cd(h) - g = c h^2 + O(h^4), so cd(2h) - cd(h) = 3 c h^2; a factor 2 for O(h^4)
    + 2 df / (2h)               rounding: both function values carry an error of at most df, the bound
                                tests/test_gpu_parity.py holds mu / var / u to (200 cond eps x its scale, propagated
                                through the utility's own derivatives)
    + 200 cond eps S            the restatement's own error, as above.
* the stage budgets of tests/predgrad_ref.py's docstring, which tests/test_gpu_predict_grad_budget.py holds the device to
  kernel by kernel: the scratch layout and the loop strides the counts rest on are read off csrc/predgrad.hip; the
  float64 restatement of the device order and NumPy / SciPy's own order sit within every budget on every input of the GPU
  test; every mutant of the restatement breaks one; the utility case leaves out at most a tenth of its rows.
* ``minimizeObjective(jac=True)`` on a NumPy stub GP: SciPy gets ``jac=True`` and (u, du), the refusals are raised, and
  ``jac=False`` consumes the random stream and returns what the loop without the keyword did.
"""
import os

import numpy as np
import pytest
import scipy.optimize

import predgrad_ref as ref
import util_ref

EPS = 2.2e-16
WELL = ["rosen2d_n50_noamp", "rosen2d_n50_amp", "c2small_d2_n200", "c3small_d8_n300", "d5_n130_amp"]
LADDER = ["rosen2d_n50_amp_cond1e8", "rosen2d_n50_amp_cond1e11", "rosen2d_n50_amp_cond1e13"]


@pytest.fixture(scope="module")
def truth(golden_dir):
    return np.load(os.path.join(golden_dir, "predgrad_truth.npz"))


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


@pytest.mark.parametrize("name", WELL + LADDER)
def test_restatement_within_the_bound_of_the_truth(golden_dir, truth, name):
    g = _load(golden_dir, name)
    prm = ref.fixture_params(g)
    tol = 200 * float(g["cond"]) * EPS
    T = truth[name + "/T"]
    amp = prm["amp"]
    scale = np.abs(g["alpha"]).sum() * amp
    for route in ("solve", "inverse") if name in WELL else ("solve",):
        mu, var, dmu, dvar = ref.posterior(T, g["theta"], g["y"], prm, route=route)
        rmu = np.abs(dmu - truth[name + "/dmu"]) / (tol * truth[name + "/S_mu"])
        rvar = np.abs(dvar - truth[name + "/dvar"]) / (tol * truth[name + "/S_var"])
        print(name, route, "dmu: %.3g of the bound, dvar: %.3g of the bound" % (rmu.max(), rvar.max()))
        assert rmu.max() <= 1.0 and rvar.max() <= 1.0, (route, rmu.max(), rvar.max())
        # the values, to the bounds tests/test_gpu_parity.py holds mu / var to
        assert np.abs(mu - truth[name + "/mu"]).max() <= max(1e-13, tol) * scale
        assert np.abs(var - truth[name + "/var"]).max() <= max(1e-14, tol) * amp


def _oracle(g):
    import george_oracle as go
    D = g["theta"].shape[1]
    p = g["p"]
    if int(g["fit_amp"]):
        k = go.Product(go.ConstantKernel(p[1], ndim=D), go.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    else:
        k = go.ExpSquaredKernel(np.exp(p[1:]), ndim=D)
    gp = go.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]), fit_white_noise=False)
    gp.compute(g["theta"])
    return gp


def _utility_error(kind, tmu, tvar, var):
    """|du| a (|dmu| <= tmu, |dvar| <= tvar) error of the inputs allows (tests/test_gpu_parity.py's propagation)."""
    vr = np.maximum(var, 1e-300)
    if kind == "agp":
        return tmu + 0.5 * tvar / vr
    if kind == "bape":
        return 2 * tmu + tvar * (1.0 + 1.0 / np.expm1(vr))
    return tmu + 0.2 * tvar / np.sqrt(vr)


@pytest.mark.parametrize("name", WELL)
def test_gradients_against_central_differences_of_the_oracle(golden_dir, truth, name):
    g = _load(golden_dir, name)
    prm = ref.fixture_params(g)
    X, y = g["theta"], g["y"]
    T = truth[name + "/T"][:4]
    M, D = T.shape
    tol = 200 * float(g["cond"]) * EPS
    tmu = max(1e-13, tol) * np.abs(g["alpha"]).sum() * prm["amp"]
    tvar = max(1e-14, tol) * prm["amp"]
    h = 1e-5 * (X.max(axis=0) - X.min(axis=0))
    gp = _oracle(g)
    ybest = float(np.max(y))

    def values(P):
        mu, var = gp.predict(y, P, return_var=True)
        return {"mu": mu, "var": var, **{k: util_ref.f64(k, mu, var, 0.01, ybest) for k in util_ref.KINDS}}

    def central(step):
        out = {}
        for d in range(D):
            e = np.zeros(D)
            e[d] = step * h[d]
            hi, lo = values(T + e), values(T - e)
            for key in hi:
                out.setdefault(key, np.zeros((M, D)))[:, d] = (hi[key] - lo[key]) / (2 * e[d])
        return out

    cd1, cd2 = central(1.0), central(2.0)
    mu, var, dmu, dvar, s_mu, s_var = ref.posterior(T, X, y, prm, scales=True)
    grads = {"mu": dmu, "var": dvar}
    own = {"mu": tol * s_mu, "var": tol * s_var}
    df = {"mu": np.full(M, tmu), "var": np.full(M, tvar)}
    for kind in util_ref.KINDS:
        u, du, _, _ = ref.predict_grad(T, X, y, prm, kind=kind)
        _, g_mu, g_var, _ = ref.utility(kind, mu, var, ybest=ybest)
        grads[kind] = du
        own[kind] = np.abs(g_mu)[:, None] * own["mu"] + np.abs(g_var)[:, None] * own["var"]
        df[kind] = _utility_error(kind, tmu, tvar, var)
    for key, grad in grads.items():
        bound = 2.0 / 3.0 * np.abs(cd2[key] - cd1[key]) + 2.0 * df[key][:, None] / (2 * h[None, :]) + own[key]
        err = np.abs(cd1[key] - grad)
        print(name, key, "largest error / bound: %.3g" % (err / bound).max())
        assert (err <= bound).all(), (key, float((err / bound).max()))
        # and the bound is a test: far below the gradient itself wherever the gradient is not small (mu and var; a
        # utility may be flat to rounding at these points, Jones' underflowed tail is)
        big = np.abs(grad) >= 0.1 * np.abs(grad).max()
        # (not c2small: at cond 4.7e6 the rounding allowance of the differenced mu, 200 cond eps sum|alpha| / h, is
        # itself larger than the gradient -- the finite differences the exact gradient replaces are noise there)
        if key in ("mu", "var") and name != "c2small_d2_n200":
            print(name, key, "largest bound / |gradient|: %.3g" % (bound[big] / np.abs(grad[big])).max())
            assert (bound[big] <= 0.05 * np.abs(grad[big])).all(), key


def test_non_finite_table_of_the_restatement():
    rs = np.random.RandomState(3)
    X = rs.uniform(-1, 1, size=(20, 2))
    y = np.sin(X[:, 0]) + X[:, 1]
    prm = ref.params(2, np.log([0.3, 0.5]), white_noise=-30.0)
    T = np.array([[0.1, 0.2], [np.nan, 0.0], [3.0, 0.0], [np.inf, 0.1]])
    box = [(-1, 1), (-1, 1)]
    for kind in ref.KINDS:
        u, du, mu, var = ref.predict_grad(T, X, y, prm, kind=kind, bounds=box)
        assert np.isfinite(u[0]) and np.all(np.isfinite(du[0]))
        assert np.all(np.isposinf(u[1:])) and np.all(du[1:] == 0.0) and np.all(np.isnan(mu[1:])) and np.all(np.isnan(var[1:]))
    mu, var, dmu, dvar = ref.predict_grad(T, X, y, prm, bounds=box)
    assert np.all(np.isnan(dmu[1:])) and np.all(np.isnan(dvar[1:])) and np.all(np.isfinite(dmu[0]))
    u, g_mu, g_var, flat = ref.utility("bape", np.array([1.0, 1.0]), np.array([0.0, -1e-3]))
    assert np.all(np.isposinf(u)) and np.all(flat)
    u, g_mu, g_var, flat = ref.utility("jones", np.array([1.0, 1.0]), np.array([0.0, -1e-3]))
    assert np.all(u == 0.0) and np.all(flat)
    u, g_mu, g_var, flat = ref.utility("agp", np.array([1.0]), np.array([-1e-3]))
    assert np.isnan(u[0]) and np.isnan(g_mu[0]) and np.isnan(g_var[0]) and not flat[0]


# ---- minimizeObjective(jac=True) on a NumPy stub -----------------------------------------------------------------------
class StubGP(object):
    """The two calls the scalar utilities and the exact-gradient search make, in NumPy."""
    computed = True

    def __init__(self):
        rs = np.random.RandomState(11)
        self.X = rs.uniform(-2, 2, size=(30, 2))
        self.y = -np.sum(self.X ** 2, axis=1)
        self.prm = ref.params(2, np.log([1.5, 1.5]), white_noise=-10.0, mean=float(np.mean(self.y)))
        self.grad_calls = []

    def predict(self, y, t, return_var=True, **kw):
        mu, var, _, _ = ref.posterior(np.atleast_2d(t), self.X, y, self.prm)
        return mu, var

    def predict_grad(self, y, t, kind=None, bounds=None, zeta=0.01, return_device=False):
        self.grad_calls.append((kind, zeta))
        return ref.predict_grad(np.atleast_2d(t), self.X, y, self.prm, kind=kind, bounds=bounds, zeta=zeta)


def _prior(x):
    x = np.asarray(x).ravel()
    return 0.0 if np.all(np.abs(x) <= 2.0) else -np.inf


def _sample(n):
    return np.random.uniform(-2, 2, size=(n, 2))


def test_jac_true_hands_scipy_the_exact_gradient(monkeypatch):
    from approxposterior_amd import utility as ut
    gp = StubGP()
    seen = []
    real = scipy.optimize.minimize

    def spy(fun, x0, **kw):
        seen.append(kw)
        f, gr = fun(np.asarray(x0, dtype=float), *kw.get("args", ()))
        assert isinstance(f, float) and gr.shape == (2,) and gr.dtype == np.float64
        return real(fun, x0, **kw)

    monkeypatch.setattr(ut, "minimize", spy)
    np.random.seed(5)
    x, val = ut.minimizeObjective(ut.BAPEUtility, gp.y, gp, _sample, _prior, nRestarts=3, method="l-bfgs-b",
                                  args=(gp.y, gp, _prior), jac=True)
    assert len(seen) >= 3 and all(kw.get("jac") is True for kw in seen)
    assert all(kw["bounds"] is None for kw in seen)            # the reference's quirk: " l-bfgs-b" and "tnc" only
    assert gp.grad_calls and all(k == ("bape", 0.01) for k in gp.grad_calls)
    assert np.isfinite(_prior(x))
    assert float(val) == float(ut.BAPEUtility(x, gp.y, gp, _prior))
    # a stationary point of the utility, or on the prior's edge
    u, du, _, _ = gp.predict_grad(gp.y, x, kind="bape")
    assert np.abs(du).max() <= 1e-3 * max(1.0, abs(float(u[0]))) or np.any(np.abs(np.abs(x) - 2.0) < 1e-6)
    # Jones reads zeta from args[3]; tnc gets the bounds
    seen.clear(); gp.grad_calls.clear()
    ut.minimizeObjective(ut.JonesUtility, gp.y, gp, _sample, _prior, nRestarts=1, method="tnc", bounds=[(-2, 2)] * 2,
                         args=(gp.y, gp, _prior, 0.05), jac=True)
    assert all(k == ("jones", 0.05) for k in gp.grad_calls) and seen[0]["bounds"] == [(-2, 2)] * 2
    # outside the prior: +inf and a zero gradient, without a device call
    gp.grad_calls.clear()
    fun = None

    def grab(f, x0, **kw):
        nonlocal fun
        fun = f
        return real(f, x0, **kw)

    monkeypatch.setattr(ut, "minimize", grab)
    ut.minimizeObjective(ut.AGPUtility, gp.y, gp, _sample, _prior, nRestarts=1, method="bfgs", args=(gp.y, gp, _prior),
                         jac=True)
    gp.grad_calls.clear()
    f, gr = fun(np.array([5.0, 0.0]))
    assert f == np.inf and np.array_equal(gr, np.zeros(2)) and not gp.grad_calls


def test_jac_true_refusals():
    from approxposterior_amd import utility as ut
    gp = StubGP()
    for method in ("nelder-mead", "Powell", "cobyla"):
        with pytest.raises(ValueError):
            ut.minimizeObjective(ut.AGPUtility, gp.y, gp, _sample, _prior, method=method, args=(gp.y, gp, _prior), jac=True)
    with pytest.raises(ValueError):
        ut.minimizeObjective(ut.AGPUtility, gp.y, gp, _sample, _prior, onDevice=True, args=(gp.y, gp, _prior), jac=True)
    with pytest.raises(ValueError):
        ut.minimizeObjective(lambda x, *a: 0.0, gp.y, gp, _sample, _prior, method="l-bfgs-b", jac=True)

    def declared(x, *a):
        return 0.0
    declared.searchKind = "something"
    with pytest.raises(ValueError):
        ut.minimizeObjective(declared, gp.y, gp, _sample, _prior, method="l-bfgs-b", jac=True)


def _loop_without_the_keyword(fn, y, gp, sampleFn, priorFn, nRestarts, method, args):
    """minimizeObjective's host loop as it stood before ``jac`` existed (theta0=None, no bounds forwarded)."""
    options = {"adaptive": True} if method == "nelder-mead" else None
    res, vals = [], []
    for _ in range(nRestarts):
        t0 = np.asarray(sampleFn(1)).reshape(1, -1)
        while True:
            sol = scipy.optimize.minimize(lambda x, *a: float(np.asarray(fn(x, *a), dtype=float).ravel()[0]),
                                          np.asarray(t0, dtype=float).ravel(), args=args, bounds=None, method=method,
                                          options=options)["x"]
            if np.all(np.isfinite(sol)) and np.isfinite(priorFn(sol)):
                res.append(sol)
                vals.append(fn(sol, *args))
                break
            t0 = np.array(sampleFn(1)).reshape(1, -1)
    best = int(np.argmin([float(np.asarray(v, dtype=float).ravel()[0]) for v in vals]))
    return np.array(res)[best], vals[best]


@pytest.mark.parametrize("method", ["nelder-mead", "l-bfgs-b"])
def test_jac_false_is_the_search_as_it_was(method):
    from approxposterior_amd import utility as ut
    gp = StubGP()
    args = (gp.y, gp, _prior)
    np.random.seed(9)
    want = _loop_without_the_keyword(ut.AGPUtility, gp.y, gp, _sample, _prior, 3, method, args)
    state_want = np.random.get_state()[1].copy()
    for kw in ({}, {"jac": False}):
        np.random.seed(9)
        got = ut.minimizeObjective(ut.AGPUtility, gp.y, gp, _sample, _prior, nRestarts=3, method=method, args=args, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1]), np.asarray(want[1]))
        assert np.array_equal(np.random.get_state()[1], state_want)
    assert not gp.grad_calls


# ---- the stage budgets of apgp_predict_grad (tests/test_gpu_predict_grad_budget.py's bars, held on the CPU) ------------
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "approxposterior_amd", "csrc",
                   "predgrad.hip")


def _define(text, name):
    import re
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, text, re.M)
    assert m, "csrc/predgrad.hip no longer defines %s: tests/predgrad_ref.py's layout has to follow" % name
    return m.group(1).strip()


def test_scratch_layout_is_the_source_s():
    """``work_views`` and the stage depths are read off csrc/predgrad.hip: a change of one of these lines changes what
    the call leaves in ``work`` or how deep a sum is, and predgrad_ref has to follow before the GPU tests mean anything."""
    text = open(SRC).read()
    for name, want in (("PG_T", ref.PG_T), ("PG_PB", ref.PG_PB), ("PG_PBS", ref.PG_PBS), ("PG_FR", ref.PG_FR),
                       ("PG_NRC", ref.PG_NRC), ("PG_B", ref.PG_B)):
        assert int(_define(text, name)) == want, "%s is %s in the source, %d in predgrad_ref" % (name, _define(text, name), want)
    assert _define(text, "PG_PER_POINT") == "(2 + PG_NRC)" and ref.PG_PER_POINT == 2 + ref.PG_NRC
    assert _define(text, "PG_CHUNK_DOUBLES") == "(1ll << 24)" and ref.PG_CHUNK_DOUBLES == 1 << 24
    for line, what in (
            ("int64_t ch = PG_CHUNK_DOUBLES / (PG_PER_POINT * ns) / PG_PB * PG_PB;", "pg_chunk"),
            ("if (ch > 4096) ch = 4096;", "pg_chunk's cap (PG_CHUNK_MAX)"),
            ("if (ch < PG_PB) ch = PG_PB;", "pg_chunk's floor"),
            ("const int64_t mr = apgp_round_up(m, PG_PB);", "pg_chunk's round-up of m"),
            ("a.kbuf = work; a.vbuf = work + ch * ns; a.wbuf = work + 2 * ch * ns;", "the order of kbuf, vbuf, wbuf"),
            ("a.vsrc = inverse ? a.vbuf : a.kbuf;", "v on the solve route"),
            ("a.wstride = ch * ns;", "the stride of the partial planes"),
            ("a.rc = apgp_round_up((n + PG_NRC - 1) / PG_NRC, 64);", "the rc rule"),
            ("if (a.rc < 512) a.rc = 512;", "the rc rule's floor (PG_RC_MIN)"),
            ("a.nrc = (int)((n + a.rc - 1) / a.rc);", "nrc"),
            ("a.rc = ns;", "rc on the solve route"),
            ("for (long long k = 2 * lane; k <= i1; k += 128) {", "the forward product's stride (FWD_STRIDE)"),
            ("for (long long i = ibeg + rs; i < iend; i += 4) {", "the transposed product's four chains"),
            ("for (long long k = t; k < a.n; k += PG_T) {", "the finish kernel's strided chain"),
            ("for (long long r = k / a.rc; r < a.nrc; ++r) wk += wp[r * a.wstride + k];", "the sum of the partial planes"),
            ("for (long long i = j0 + PG_B + w; i < n; i += 4) {", "the backward substitution's four chains")):
        assert line in text, "csrc/predgrad.hip: %s changed; update tests/predgrad_ref.py (layout and counts)" % what
    assert ref.PG_CHUNK_MAX == 4096 and ref.PG_RC_MIN == 512 and ref.FWD_STRIDE == 128
    # what the GPU test's shapes are chosen for
    got = {n: ref.row_chunks(n, "inverse") for n in (512, 513, 1025, 2049, 4096, 4097)}
    assert got == {512: (512, 1), 513: (512, 2), 1025: (512, 3), 2049: (512, 5), 4096: (512, 8), 4097: (576, 8)}
    assert ref.row_chunks(449, "solve") == (512, 1)
    assert ref.chunk(4100, 65) == 4096 and ref.chunk(9, 4097) == 16 and ref.chunk(1, 1) == 8
    assert all(ref.chunk(c[2], c[0]) >= c[2] for cs in ref.budget_cases().values() for c in cs), "one chunk per case"
    # the views
    m, n = 9, 513
    ns, ch = ref.ns_of(n), ref.chunk(m, n)
    work = np.arange(ref.work_len(m, n), dtype=np.float64)
    vw = ref.work_views(work, m, n, "inverse")
    assert vw["k"][2, 5] == 2 * ns + 5 and vw["v"][2, 5] == ch * ns + 2 * ns + 5
    assert vw["w"].shape == (2, m, ns) and vw["w"][1, 3, 7] == (2 + 1) * ch * ns + 3 * ns + 7
    vs = ref.work_views(work, m, n, "solve")
    assert vs["k"] is None and vs["v"][2, 5] == 2 * ns + 5 and vs["w"].shape == (1, m, ns) and vs["w"][0, 1, 0] == 2 * ch * ns + ns
    with pytest.raises(ValueError):
        ref.work_views(work[:-1], 17, n, "inverse")


ALL_CASES = sorted(set(c for cs in ref.budget_cases().values() for c in cs),
                   key=lambda c: (c[3], c[0], c[1], c[2], -1 if c[4] is None else c[4]))


@pytest.mark.parametrize("c", ALL_CASES, ids=ref.case_id)
def test_restatement_and_scipy_within_every_stage_budget(c):
    """The clean restatement of the device order and NumPy / SciPy's own order, on every input of the GPU test."""
    case = ref.Case(*c, util=(c[2] == ref.UTIL_M))
    for name, rec in (("restated", ref.restate(case)), ("scipy", ref.scipy_route(case))):
        r = ref.judge(case, rec)
        print(ref.case_id(c), name, "  ".join("%s %.3f" % kv for kv in sorted(r.items())))
        assert max(r.values()) <= 1.0, (name, r)


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_every_mutant_breaks_a_budget(mutant):
    route, n, D, order = ref.MUTANTS[mutant]
    c = (n, D, ref.M_OF[route], route, order)
    assert c in ALL_CASES, "a mutant is shown on an input of the GPU test"
    case = ref.Case(*c)
    assert max(ref.judge(case, ref.restate(case)).values()) <= 1.0
    r = ref.judge(case, ref.restate(case, mutant))
    broken = {k: v for k, v in r.items() if v > 1.0}
    print(mutant, ref.case_id(c), "breaks", "  ".join("%s %.3g" % kv for kv in sorted(broken.items())))
    assert broken, (mutant, r)


@pytest.mark.parametrize("route", ["inverse", "solve"])
def test_utility_case_leaves_out_at_most_a_tenth_and_the_chain_budget_holds(route):
    """From the truth alone (long double, no device): the rows of the utility case outside the box or with sigma^2 <= 0
    are at most UTIL_CAP of it, both kinds occur, no sigma^2 is so close to zero that a device within its budget could
    land on the other side, and NumPy's chain rule sits within the chain budget while a dropped term does not."""
    case = ref.Case(ref.UTIL_N, ref.UTIL_D, ref.UTIL_M, route, util=True)
    n = case.n
    with np.errstate(all="ignore"):
        kh = ref.kr.truth_ld(case.T, case.X, case.k)
    A = np.tril(case.A)
    v = (kh @ A.astype(ref.LD).T) if route == "inverse" else ref.sr.solve_ld(A, kh.T).T
    var = (ref.sr.ktt_truth(case.T, case.k)[0] - (v * v).sum(1)).astype(np.float64)
    inside, judged = ref.util_rows(case, var)
    out, flat = int((~inside).sum()), int((inside & ~judged).sum())
    print(route, "outside the box: %d, sigma^2 <= 0: %d, of %d; smallest |sigma^2| %.3g" % (out, flat, case.m, np.abs(var).min()))
    assert out == ref.UTIL_OUT and flat >= 1
    assert out + flat <= ref.UTIL_CAP * case.m
    assert np.abs(var[inside]).min() >= 1e-6                       # (the variance budget is below 1e-12 here)
    rec = ref.restate(case)
    assert np.array_equal(ref.util_rows(case, rec["var"])[1], judged)
    mu, vr, dmu, dvar = (rec[key][judged] for key in ("mu", "var", "dmu", "dvar"))
    for kind in ref.UTIL_KINDS:
        _, g_mu, g_var, fl = ref.utility(kind, mu, vr, zeta=ref.UTIL_ZETA, ybest=ref.UTIL_YBEST)
        assert not fl.any()
        du = g_mu[:, None] * dmu + g_var[:, None] * dvar
        r = ref.du_ratio(kind, du, mu, vr, dmu, dvar, ref.UTIL_ZETA, ref.UTIL_YBEST)
        print(route, kind, "NumPy's chain rule / budget %.3f" % r.max())
        assert r.max() <= 1.0
        if kind in ("agp", "bape"):                                # a derivative factor demoted to fp32
            bad = g_mu[:, None] * dmu + g_var.astype(np.float32).astype(np.float64)[:, None] * dvar
            assert ref.du_ratio(kind, bad, mu, vr, dmu, dvar, ref.UTIL_ZETA, ref.UTIL_YBEST).max() > 1.0
        if kind == "jones":                                        # zeta left out of z
            _, b_mu, b_var, _ = ref.utility(kind, mu, vr, zeta=0.0, ybest=ref.UTIL_YBEST)
            bad = b_mu[:, None] * dmu + b_var[:, None] * dvar
            assert ref.du_ratio(kind, bad, mu, vr, dmu, dvar, ref.UTIL_ZETA, ref.UTIL_YBEST).max() > 1.0
