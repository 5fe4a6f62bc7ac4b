"""MI355X: the on-device Hamiltonian Monte Carlo sampler (csrc/hmc.hip, GP.sample_hmc, mcmc.HMCChain, runMCMC(hmc=...))
against its NumPy restatement (tests/hmc_ref.py), whose docstring derives every budget used here.

1. step-by-step replay: from the device's own (q, p) before each leapfrog step (``trace``) the reference recomputes the
   step; every component within the rounding budget, dH within its budget, every decision equal outside near-ties and
   near-face drifts, whose share is capped at 2 % (tests/test_hmc_ref.py shows the reference's own free runs stay below it);
2. the first half kick against GP.predict_grad(kind=None);
3. bits: repeatability, independence of the number of chains, of where a run is cut; different G within the budget;
4. gate and edge cases;  5. stationarity against quadrature and against evidence();  6. the API and its refusals."""
import ctypes

import numpy as np
import pytest

import hmc_ref as hr
import test_gpu_ensemble_replay as rp

pytestmark = pytest.mark.gpu
U = hr.U


def _mcmc():
    from approxposterior_amd import mcmc
    return mcmc


def _run(c, debug=True, **kw):
    D, C, n, kern, L, eps, G, jitter, box = c
    X, y, gp, gpo, model, b, p0 = hr.case_inputs(c)
    if not gp.computed:
        gp.compute(X)
    args = dict(jitter=jitter, seed=hr.REPLAY_SEED, debug=debug, gRows=G)
    args.update(kw)
    p0 = args.pop("p0", p0)
    iters = args.pop("iterations", hr.REPLAY_ITERATIONS)
    return gp.sample_hmc(y, p0, iters, b, eps, L, **args), model, b, p0, y, gp


# ---------------------------------------------------------------------------------------------------------------------
# 1. replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hr.REPLAY_CASES, ids=hr.case_id)
def test_replay_step_by_step(c):
    D, C, n, kern, L, eps, G, jitter, box = c
    res, model, b, p0, y, gp = _run(c)
    sc = model.sc
    lo, hi = b[:, 0] * sc, b[:, 1] * sc
    tr = res["trace"]
    T = tr.shape[0]
    assert tr.shape == (T, C, L, 2, D) and res["g_rows"] == G
    # the device's decisions: the stored state is the trajectory's end point.  (A rejected end point equal to the previous
    # state in every bit would read as accepted; the device's own count, naccept, and the stored log-probabilities are
    # checked against this reading below.)
    moved = np.all(res["chain"] == res["proposals"], axis=2)
    f = hr.forced(model, p0 * sc, tr, moved, lo, hi, eps, L, jitter=jitter, seed=hr.REPLAY_SEED, G=G)
    assert np.all(res["ndiverge"] == 0)
    near = f["near"]
    nnear, ndrift = int(near.sum()), near.size
    eq, ep = np.abs(tr[:, :, :, 0] - f["q"]), np.abs(tr[:, :, :, 1] - f["p"])
    rq = np.where(near[..., None], 0.0, eq / f["Bq"])
    rp_ = np.where(near[..., None], 0.0, ep / f["Bp"])
    print("%s: worst q %.3f, p %.3f of the budget; budgets up to q %.2e, p %.2e; %d of %d drifts near a face, "
          "%d trajectories reflected" % (hr.case_id(c), rq.max(), rp_.max(), f["Bq"].max(), f["Bp"].max(), nnear, ndrift,
                                        int((f["count"].sum(axis=2) > 0).sum())))
    assert rq.max() <= 1.0 and rp_.max() <= 1.0
    # dH from the same endpoints
    live = ~f["gated"]
    rd = np.abs(res["dH"] - f["dH"])[live] / f["BdH"][live]
    print("  dH: worst %.3f of the budget (budget up to %.2e)" % (rd.max(), f["BdH"][live].max()))
    assert rd.max() <= 1.0
    # decisions
    tie = live & (f["margin"] <= f["BdH"] + 4.0 * U * np.abs(f["logu"]))
    skip = tie | near.any(axis=2)
    assert np.array_equal(moved[~skip], f["accept"][~skip])
    assert not moved[f["gated"]].any()
    ntie = int(tie.sum())
    print("  %d near-ties in %d decisions; acceptance %.2f" % (ntie, moved.size, moved.mean()))
    assert ntie <= hr.NEAR_CAP * moved.size and nnear <= hr.NEAR_CAP * ndrift
    if box == "tight":
        refl = (f["count"].sum(axis=2) > 0)[live]
        assert refl.mean() >= 0.1, "only %.3f of the trajectories reflect" % refl.mean()
    # the stored chain: the accepted end point or the previous state, the log-probability within the mean's budget
    prev = np.concatenate([p0[None], res["chain"][:-1]], axis=0)
    assert np.array_equal(res["chain"][~moved], prev[~moved])
    assert np.allclose(res["proposals"], tr[:, :, L - 1, 0] / sc, rtol=4 * U, atol=0)
    lp = res["log_prob"]
    assert np.all(np.abs(lp[moved] - f["mu_after"][moved]) <= f["Bmu_after"][moved])
    assert np.array_equal(res["naccept"], moved.sum(axis=0))
    assert np.array_equal(lp[1:][~moved[1:]], lp[:-1][~moved[1:]])                 # a rejection keeps the log-probability
    inside = np.all((res["chain"] >= b[:, 0]) & (res["chain"] <= b[:, 1]), axis=2)
    assert inside[:, ~f["gated"][0]].all()
    if f["gated"][0].any():
        g = f["gated"][0]
        assert np.all(res["naccept"][g] == 0) and np.all(np.isneginf(res["final_log_prob"][g]))
        assert np.array_equal(res["coords"][g], p0[g])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the gradient against the existing kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [hr.REPLAY_CASES[i] for i in (1, 3, 7, 9)], ids=hr.case_id)
def test_first_half_kick_is_predict_grad(c):
    """L = 1, jitter = 0, the wide box: p after the step minus the drawn momentum is (eps / 2) (g(q_0) + g(q_1)).  With q_1
    from the trace, GP.predict_grad at q_0 / sc and q_1 / sc (dmu / sc is the gradient in scaled coordinates) must give the
    same kick within the sum of the two kernels' budgets: B_g of hmc_ref at both points for this kernel, the same again
    for predict_grad's finish kernel (the same N-term sums over 256 lanes: no more roundings than G = 1 is charged) with
    8 u |g| for its chain rule and the division here, the momentum draw's 16 u |p_0|, 4 u |p_1| for the two kicks'
    roundings, and the move of the reference's own gradient between q and (q / sc) sc, the point predict_grad sees."""
    D, C, n, kern, L, eps, G, jitter, box = c
    res, model, b, p0, y, gp = _run((D, C, n, kern, 1, eps, G, 0.0, "wide"), iterations=1)
    sc = model.sc
    tr = res["trace"]
    z, uj, ua = hr.draws(np.arange(1), np.arange(C), D, hr.REPLAY_SEED)
    live = np.all((p0 >= b[:, 0]) & (p0 <= b[:, 1]), axis=1)
    q0, q1, p1 = p0 * sc, tr[0, :, 0, 0], tr[0, :, 0, 1]
    g0 = np.asarray(gp.predict_grad(y, q0 / sc, kind=None)[2]) / sc
    g1 = np.asarray(gp.predict_grad(y, q1 / sc, kind=None)[2]) / sc
    _, r0, _, B0 = model.mg(q0, 1, True)
    _, r1, _, B1 = model.mg(q1, 1, True)
    kick, want = p1 - z[0], 0.5 * eps * (g0 + g1)
    # a reflected component has its momentum flipped between the two half kicks: the unreflected ones are compared
    flat = np.abs(q1 - (q0 + eps * (z[0] + 0.5 * eps * r0))) <= 1e-9
    tol = 0.5 * eps * (2.0 * (B0 + B1) + 8.0 * U * (np.abs(g0) + np.abs(g1))) + 16.0 * U * np.abs(z[0]) + 4.0 * U * np.abs(p1)
    tol = tol + 0.5 * eps * (np.abs(model.mg((q0 / sc) * sc)[1] - r0) + np.abs(model.mg((q1 / sc) * sc)[1] - r1))
    sel = live[:, None] & flat
    err = np.abs(kick - want)
    print("%s: first kick against predict_grad: worst %.3f of the budget over %d components" % (
        hr.case_id(c), (err / tol)[sel].max(), sel.sum()))
    assert sel.sum() >= sel.size // 2 and np.all(err[sel] <= tol[sel])


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
_KEYS = ("chain", "log_prob", "coords", "final_log_prob", "naccept", "accept_prob", "ndiverge", "proposals", "dH", "trace")


@pytest.mark.parametrize("G", [1, 4])
def test_same_call_same_bits_and_chain_independence(G):
    c = (8, 5, 200, "selin1", 7, 0.08, G, 0.3, "tight")
    X, y, gp, gpo, model, b, p5 = hr.case_inputs(c)
    a, _, _, _, _, _ = _run(c)
    a2, _, _, _, _, _ = _run(c)
    for k in _KEYS:
        assert np.array_equal(a[k], a2[k], equal_nan=True), k
    p37 = hr.case_start(37, 8, b, 5)
    p37[3] = p5[3]
    big, _, _, _, _, _ = _run(c, p0=p37)
    for k in ("chain", "log_prob", "proposals", "dH", "trace"):
        assert np.array_equal(a[k][:, 3], big[k][:, 3]), k
    for k in ("coords", "final_log_prob", "naccept", "accept_prob", "ndiverge"):
        assert np.array_equal(a[k][3], big[k][3]), k


@pytest.mark.parametrize("G", [1, 4])
def test_a_run_cut_into_calls_is_the_uncut_run(G):
    c = (2, 17, 90, "amp", 7, 0.1, G, 0.3, "tight")
    whole, model, b, p0, y, gp = _run(c, iterations=37, debug=False)
    cuts = [5, 5, 5, 5, 5, 5, 5, 2]
    coords, it0, parts, nacc = p0, 0, [], 0
    for m in cuts:
        r = gp.sample_hmc(y, coords, m, b, c[5], c[4], jitter=c[7], seed=hr.REPLAY_SEED, iteration0=it0, gRows=G)
        parts.append(r)
        coords, it0, nacc = r["coords"], it0 + m, nacc + r["naccept"]
    assert np.array_equal(np.concatenate([r["chain"] for r in parts]), whole["chain"])
    assert np.array_equal(np.concatenate([r["log_prob"] for r in parts]), whole["log_prob"])
    assert np.array_equal(nacc, whole["naccept"]) and np.array_equal(coords, whole["coords"])


def test_different_group_widths_agree_within_the_step_budget():
    """One trajectory of every chain from the same start and momentum at G = 1 and G = 4, every step held to the step
    budget.  Step l of width G is within its budget B_G of Ref(its own (q, p) after step l - 1), Ref being the reference's
    step; so the two devices differ after step l by at most B_1 + B_4 plus |Ref(a_{l-1}) - Ref(d_{l-1})|, the difference the
    previous step left, carried through the reference's own step map (hmc_ref.forced evaluates Ref at each device's
    trace; for the first step the inputs are identical and that term is zero).  The same for dH: within B_dH(1) + B_dH(4)
    plus the reference's dH difference between the two pairs of end points; and the two decisions are equal unless either
    margin |log u + dH| lies within that window."""
    c1 = (8, 5, 200, "se", 7, 0.08, 1, 0.0, "wide")
    c4 = c1[:6] + (4,) + c1[7:]
    a, model, b, p0, y, gp = _run(c1, iterations=1)
    d, _, _, _, _, _ = _run(c4, iterations=1)
    sc = model.sc
    fs = []
    for r, G in ((a, 1), (d, 4)):
        moved = np.all(r["chain"] == r["proposals"], axis=2)
        fs.append((moved, hr.forced(model, p0 * sc, r["trace"], moved, b[:, 0] * sc, b[:, 1] * sc, c1[5], c1[4],
                                    seed=hr.REPLAY_SEED, G=G)))
    (m1, f1), (m4, f4) = fs
    assert not (f1["near"].any() or f4["near"].any())
    dq, dp = np.abs(a["trace"][:, :, :, 0] - d["trace"][:, :, :, 0]), np.abs(a["trace"][:, :, :, 1] - d["trace"][:, :, :, 1])
    carry_q, carry_p = np.abs(f1["q"] - f4["q"]), np.abs(f1["p"] - f4["p"])
    assert np.all(carry_q[:, :, 0] == 0.0)                      # the first step has identical inputs
    bq, bp = f1["Bq"] + f4["Bq"] + carry_q, f1["Bp"] + f4["Bp"] + carry_p
    print("G = 1 against G = 4: worst q %.3f, p %.3f of the summed budgets; the carried part up to %.2e, the budgets up to "
          "%.2e" % ((dq / bq).max(), (dp / bp).max(), max(carry_q.max(), carry_p.max()), max(bq.max(), bp.max())))
    assert np.all(dq <= bq) and np.all(dp <= bp)
    live = ~f1["gated"]
    window = f1["BdH"] + f4["BdH"] + np.where(live, np.abs(f1["dH"] - f4["dH"]), 0.0)
    assert np.all(np.abs(a["dH"] - d["dH"])[live] <= window[live])
    tie = live & ((f1["margin"] <= window) | (f4["margin"] <= window))
    assert np.array_equal(m1[~tie], m4[~tie]) and tie.sum() <= hr.NEAR_CAP * tie.size


# ---------------------------------------------------------------------------------------------------------------------
# 4. gate and edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_zero_iterations_store_and_divergence():
    c = (2, 5, 90, "se", 7, 0.1, 1, 0.1, "wide")
    X, y, gp, gpo, model, b, p0 = hr.case_inputs(c)
    res, _, _, _, _, _ = _run(c, iterations=30)
    assert res["naccept"][0] == 0 and np.isneginf(res["final_log_prob"][0]) and np.array_equal(res["coords"][0], p0[0])
    assert np.all(res["chain"][:, 0] == p0[0])
    inside = np.all((res["chain"][:, 1:] >= b[:, 0]) & (res["chain"][:, 1:] <= b[:, 1]), axis=2)
    assert inside.all() and res["naccept"][1:].sum() > 0
    zero, _, _, _, _, _ = _run(c, iterations=0)
    assert np.array_equal(zero["coords"], p0) and zero["chain"].shape == (0, 5, 2)
    want = gpo.predict(y, p0[1:], return_cov=False)
    assert np.isneginf(zero["final_log_prob"][0]) and np.allclose(zero["final_log_prob"][1:], want, rtol=1e-7, atol=1e-7)
    quiet = gp.sample_hmc(y, p0, 30, b, c[5], c[4], jitter=c[7], seed=hr.REPLAY_SEED, store=False, gRows=1)
    assert quiet["chain"] is None and quiet["log_prob"] is None
    for k in ("coords", "final_log_prob", "naccept", "accept_prob", "ndiverge"):
        assert np.array_equal(quiet[k], res[k]), k
    wild = gp.sample_hmc(y, p0, 20, b, 50.0, 7, jitter=0.0, seed=3, gRows=4)
    assert wild["ndiverge"][1:].sum() > 0 and np.all(np.isfinite(wild["chain"]))
    assert np.all((wild["chain"][:, 1:] >= b[:, 0]) & (wild["chain"][:, 1:] <= b[:, 1]))
    assert np.all(wild["naccept"] + wild["ndiverge"] <= 20)


# ---------------------------------------------------------------------------------------------------------------------
# 5. stationarity
# ---------------------------------------------------------------------------------------------------------------------
def _gauss_problem(D, n, seed):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((D, D)) * 0.3 + np.eye(D)
    cov = 0.16 * (A @ A.T) / D + 0.04 * np.eye(D)
    cov[0, 1] = cov[1, 0] = 0.7 * np.sqrt(cov[0, 0] * cov[1, 1])
    Pm = np.linalg.inv(cov)
    b = np.array([(-1.2, 1.0)] * D)
    X = rs.uniform(b[:, 0], b[:, 1], size=(n, D))
    y = -0.5 * np.einsum("ni,ij,nj->n", X, Pm, X)
    gp = agp.GP(kernel=np.var(y) * agp.ExpSquaredKernel([0.5 * D] * D, ndim=D), fit_mean=True, mean=float(np.mean(y)),
                white_noise=-6.0, fit_white_noise=False)
    gp.compute(X)
    return X, y, gp, b


def _moments_check(chain, mean, cov, ref_mean_err=0.0, ref_cov_err=0.0):
    """Mean and covariance of the chain within 5 standard errors of the truth: the chain's batch-means standard error
    and the reference's own error (a quadrature bound, or the standard error of an importance-sampling estimate)
    combined in quadrature."""
    from approxposterior_amd.mcmcUtils import batchMeansMCSE
    T, C, D = chain.shape
    series = chain.mean(axis=1)                                                  # (T, D): the chains' mean per iteration
    se = np.asarray(batchMeansMCSE(series))
    print("mean", series.mean(axis=0), "truth", mean, "se", se, "reference error", ref_mean_err)
    assert np.all(np.abs(series.mean(axis=0) - mean) <= 5.0 * np.sqrt(se ** 2 + np.asarray(ref_mean_err) ** 2))
    r = chain - mean
    prods = np.einsum("tci,tcj->tij", r, r).reshape(T, D * D) / C
    sec = np.asarray(batchMeansMCSE(prods))
    print("cov diag", prods.mean(axis=0).reshape(D, D).diagonal(), "truth", np.diag(cov))
    assert np.all(np.abs(prods.mean(axis=0) - cov.ravel()) <= 5.0 * np.sqrt(sec ** 2 + np.asarray(ref_cov_err) ** 2))


def test_stationary_d2_against_quadrature():
    mcmc = _mcmc()
    X, y, gp, b = _gauss_problem(2, 120, 11)

    def grid(m):
        e = [lo + (np.arange(m) + 0.5) * ((hi - lo) / m) for lo, hi in b]
        pts = np.array(np.meshgrid(*e, indexing="ij")).reshape(2, -1).T
        mu = np.asarray(gp.predict(y, pts, return_cov=False), dtype=np.float64).ravel()
        w = np.exp(mu - mu.max())
        w /= w.sum()
        mean = w @ pts
        return mean, (pts - mean).T @ ((pts - mean) * w[:, None])
    (m1, c1), (m2, c2) = grid(256), grid(512)
    rs = np.random.RandomState(5)
    p0 = rs.uniform(-0.3, 0.3, size=(64, 2))
    coords, eps, mass, hist, it = mcmc.hmc_warmup(gp, y, p0, b, 0.2, 8, nWarmup=200, adaptEvery=20, targetAccept=0.8, seed=9)
    res = gp.sample_hmc(y, coords, 600, b, eps, 8, seed=9, iteration0=it)
    acc = float(res["accept_prob"].mean())
    print("eps history", hist, "-> eps %.4f, acceptance %.3f, divergences %d" % (eps, acc, res["ndiverge"].sum()))
    assert it == 200 and len(hist) == 10 and abs(acc - 0.8) <= 0.1
    _moments_check(res["chain"], m2, c2, np.abs(m2 - m1), np.abs(c2 - c1).ravel())


def test_stationary_d8_against_evidence():
    from approxposterior_amd import approx
    mcmc = _mcmc()
    D = 8
    X, y, gp, b = _gauss_problem(D, 300, 12)
    ap = approx.ApproxPosterior(theta=X, y=y, gp=gp, lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                                priorSample=lambda m: np.random.uniform(b[:, 0], b[:, 1], size=(m, D)), bounds=b,
                                algorithm="agp", distributed=False)
    # the truth and ITS error: eight independent importance-sampling estimates, their mean and its standard error
    ev = [ap.evidence(nSamples=2 ** 21, proposal="box", seed=s) for s in range(1, 9)]
    tm, tc = np.array([e["mean"] for e in ev]), np.array([np.asarray(e["cov"]).ravel() for e in ev])
    e1 = {"mean": tm.mean(axis=0), "cov": tc.mean(axis=0).reshape(D, D), "ess": np.mean([e["ess"] for e in ev])}
    em, ec = tm.std(axis=0, ddof=1) / np.sqrt(len(ev)), tc.std(axis=0, ddof=1) / np.sqrt(len(ev))
    rs = np.random.RandomState(6)
    p0 = rs.uniform(-0.2, 0.2, size=(64, D))
    coords, eps, mass, hist, it = mcmc.hmc_warmup(gp, y, p0, b, 0.1, 8, nWarmup=200, adaptEvery=20, targetAccept=0.8, seed=10)
    res = gp.sample_hmc(y, coords, 600, b, eps, 8, seed=10, iteration0=it)
    acc = float(res["accept_prob"].mean())
    print("eps %.4f, acceptance %.3f, importance ess %.0f per estimate" % (eps, acc, e1["ess"]))
    assert abs(acc - 0.8) <= 0.1
    _moments_check(res["chain"], e1["mean"], e1["cov"], em, ec)


# ---------------------------------------------------------------------------------------------------------------------
# 6. API and refusals
# ---------------------------------------------------------------------------------------------------------------------
def _ap(joint):
    from approxposterior_amd import approx, priors as P
    X, y, gp, b = _gauss_problem(2, 120, 11)
    lo, hi = b[:, 0], b[:, 1]
    if joint:
        J = P.JointPrior([P.UniformPrior(*r) for r in b])
        lnprior, sample = J, J.sample
    else:
        lnprior = lambda t: 0.0 if np.all((np.asarray(t) >= lo) & (np.asarray(t) <= hi)) else -np.inf      # noqa: E731
        sample = lambda m: np.random.uniform(lo, hi, size=(int(m), 2))                                     # noqa: E731
    return approx.ApproxPosterior(theta=X.copy(), y=y.copy(), gp=gp, lnprior=lnprior, lnlike=lambda t, *a, **k: 0.0,
                                  priorSample=sample, bounds=[tuple(r) for r in b], algorithm="agp", distributed=False)


@pytest.mark.parametrize("joint,device_tau", [(False, False), (True, False), (False, True)],
                         ids=["box", "joint-prior", "device-autocorr"])
def test_run_mcmc_with_hmc(joint, device_tau):
    mcmc = _mcmc()
    ap = _ap(joint)
    W, N = 16, 300
    p0 = np.random.RandomState(2).uniform(-0.2, 0.2, size=(W, 2))
    np.random.seed(4)
    sampler, iburn, ithin = ap.runMCMC(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": N, "initial_state": p0},
                                       cache=False, estBurnin=True, thinChains=True, onDevice=True, deviceAutocorr=device_tau,
                                       hmc={"eps": 0.2, "nLeap": 8, "nWarmup": 100, "adaptEvery": 20})
    assert isinstance(sampler, mcmc.HMCChain) and sampler is ap.sampler
    assert sampler.get_chain().shape == (N, W, 2) and sampler.get_log_prob().shape == (N, W)
    assert sampler.accept_prob.shape == (W,) and sampler.ndiverge.shape == (W,) and len(sampler.warmup) == 5
    assert sampler.step_size > 0 and 0 <= iburn < N and ithin >= 1 and ap._chainCut == (iburn, ithin)
    assert (sampler._chain_device is not None) == device_tau
    assert np.all(sampler.acceptance_fraction > 0.3)
    blobs = sampler.get_blobs()
    if joint:
        assert blobs.shape == (N, W) and np.allclose(blobs, -np.log(2.2 ** 2))
    else:
        assert blobs is None
    ev = ap.evidence(nSamples=2 ** 16, proposal="gmm", seed=1)
    assert np.isfinite(ev["logZ"])
    np.random.seed(4)
    s2, _, _ = ap.runMCMC(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": 20, "initial_state": p0}, cache=False,
                          estBurnin=False, thinChains=False, onDevice=True, hmc=True)
    assert isinstance(s2, mcmc.HMCChain) and s2.get_chain().shape == (20, W, 2) and len(s2.warmup) == 10


def test_refused_combinations_and_arguments():
    from approxposterior_amd import _lib, gp as agp
    mcmc = _mcmc()
    ap = _ap(False)
    W = 8
    p0 = np.random.RandomState(2).uniform(-0.2, 0.2, size=(W, 2))
    base = dict(samplerKwargs={"nwalkers": W}, mcmcKwargs={"iterations": 5, "initial_state": p0}, cache=False)
    with pytest.raises(ValueError, match="onDevice"):
        ap.runMCMC(hmc=True, **base)
    with pytest.raises(ValueError, match="tempering"):
        ap.runMCMC(hmc=True, onDevice=True, tempering=3, **base)
    with pytest.raises(ValueError, match="moves"):
        ap.runMCMC(hmc=True, onDevice=True, cache=False, mcmcKwargs=base["mcmcKwargs"],
                   samplerKwargs={"nwalkers": W, "moves": mcmc.DEMove()})
    with pytest.raises(ValueError, match="keys"):
        ap.runMCMC(hmc={"stepsize": 0.1}, onDevice=True, **base)
    with pytest.raises(ValueError, match="onDevice"):
        ap.run(m=1, nmax=1, hmc=True, cache=False)
    ap._ranks = lambda: (0, 2)
    with pytest.raises(NotImplementedError):
        ap.runMCMC(hmc=True, onDevice=True, **base)
    # GP.sample_hmc
    X, y, gp, gpo = rp._problem(2, 40, "se", 1)
    b = rp._bounds(2)
    q = np.zeros((3, 2))
    ok = dict(iterations=5, bounds=b, eps=0.1, nLeap=4)
    for bad in (dict(eps=0.0), dict(eps=np.nan), dict(eps=-1.0), dict(jitter=1.0), dict(jitter=-0.1), dict(nLeap=0),
                dict(nLeap=1025), dict(gRows=2), dict(gRows=16), dict(iterations=-1), dict(iteration0=-1),
                dict(mass=[1.0]), dict(mass=[1.0, 0.0]), dict(mass=[1.0, np.inf]), dict(bounds=[(0, 1)]),
                dict(bounds=[(1.0, -1.0), (-1.0, 1.0)])):
        a = dict(ok, **bad)
        with pytest.raises(ValueError):
            gp.sample_hmc(y, q, a.pop("iterations"), a.pop("bounds"), a.pop("eps"), a.pop("nLeap"), **a)
    with pytest.raises(ValueError):
        gp.sample_hmc(y, np.zeros((3, 3)), 5, b, 0.1, 4)
    with pytest.raises(ValueError):
        gp.sample_hmc(y, np.full((3, 2), np.nan), 5, b, 0.1, 4)
    # apgp_hmc_sample through ctypes: -1 before any HIP call (the pointers are never dereferenced)
    lib = _lib.load()
    ks = gp._kernel_struct()
    one = ctypes.c_void_p(8)
    lo, hi = agp._box(b, 2, optional=False)
    swapped = agp._box([(1.0, -1.0), (-1.0, 1.0)], 2, optional=False)
    nanbox = agp._box([(np.nan, 1.0), (-1.0, 1.0)], 2, optional=False)

    def call(**kw):
        a = dict(xs=one, n=40, lo=lo, hi=hi, C=3, iters=5, eps=0.1, jitter=0.1, nleap=4, g=0, it0=0, mass=[1.0, 1.0],
                 coords=one, logp=one, nacc=one, accp=one, ndiv=one, opt=True, ks=ks)
        a.update(kw)
        o = _lib.HmcOptions()
        o.eps, o.jitter, o.nleap, o.g_rows, o.iteration0 = a["eps"], a["jitter"], a["nleap"], a["g"], a["it0"]
        o.mass[:2] = a["mass"]
        return lib.apgp_hmc_sample(a["xs"], a["n"], ctypes.byref(a["ks"]) if a["ks"] is not None else None, 0.0, a["lo"],
                                   a["hi"], a["C"], a["iters"], ctypes.byref(o) if a["opt"] else None, 1, a["coords"],
                                   a["logp"], None, None, a["nacc"], a["accp"], a["ndiv"], None, None, None, None)
    badks = _lib.KernelStruct()
    rows = [(dict(xs=None), b"null pointer"), (dict(coords=None), b"null pointer"), (dict(logp=None), b"null pointer"),
            (dict(nacc=None), b"null pointer"), (dict(accp=None), b"null pointer"), (dict(ndiv=None), b"null pointer"),
            (dict(opt=False), b"null pointer"), (dict(lo=None), b"null pointer"), (dict(ks=None), b"null pointer"),
            (dict(n=0), b"n <="), (dict(n=(1 << 24) + 1), b"n <="), (dict(C=0), b"nchains"), (dict(C=(1 << 24) + 1), b"nchains"),
            (dict(iters=-1), b"iterations"), (dict(iters=(1 << 40) + 1), b"iterations"), (dict(ks=badks), b"kernel parameters"),
            (dict(eps=0.0), b"eps"), (dict(eps=np.inf), b"eps"), (dict(eps=np.nan), b"eps"), (dict(jitter=1.0), b"jitter"),
            (dict(jitter=-0.5), b"jitter"), (dict(jitter=np.nan), b"jitter"), (dict(nleap=0), b"nleap"),
            (dict(nleap=1025), b"nleap"), (dict(g=2), b"g_rows"), (dict(g=16), b"g_rows"), (dict(g=-1), b"g_rows"),
            (dict(it0=-1), b"iteration0"), (dict(mass=[0.0, 1.0]), b"mass"), (dict(mass=[1.0, np.nan]), b"mass"),
            (dict(mass=[np.inf, 1.0]), b"mass"), (dict(lo=swapped[0], hi=swapped[1]), b"lo <= hi"),
            (dict(lo=nanbox[0], hi=nanbox[1]), b"lo <= hi")]
    for bad, text in rows:
        assert call(**bad) == -1, bad
        msg = lib.apgp_last_error()
        assert b"apgp_hmc_sample" in msg and b"bad argument" in msg and text in msg, (bad, msg)
    assert lib.apgp_hmc_rule(0, 40, 2) == -1 and lib.apgp_hmc_rule(3, 40, 33) == -1
    assert lib.apgp_hmc_rule(3, 40, 2) in _lib.HMC_G_ROWS
