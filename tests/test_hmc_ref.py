"""The NumPy restatement of the device HMC sampler (tests/hmc_ref.py) checked on its own, on the CPU: the integrator is
reversible and volume-preserving with and without reflections, its energy error is second order, its gradient is the
derivative of the oracle's predictive mean, a free run has the right moments, and on every input of the GPU replay the
reference's own near-ties and near-face drifts stay below the cap the GPU test asserts."""
import numpy as np
import pytest

import hmc_ref as hr


def _smooth(D, n=30, seed=0):
    rs = np.random.RandomState(seed)
    return hr.Model(rs.uniform(-1, 1, size=(n, D)), rs.standard_normal(n), 0.3)


def _traj(target, q, p, eps, L, lo, hi, minv):
    mu, g = target.mg(q)
    refl = 0
    for _ in range(L):
        q, p, mu, g, info = hr.leapfrog(target, q, p, g, eps, minv, lo, hi)
        refl = refl + info["count"]
    return q, p, refl


@pytest.mark.parametrize("name", ["free", "reflecting", "corner"])
def test_reversible(name):
    D = 2 if name == "corner" else 3
    tgt = _smooth(D)
    minv = 1.0 / np.linspace(0.7, 1.4, D)
    if name == "free":
        lo, hi = np.full(D, -np.inf), np.full(D, np.inf)
        q, p = np.random.RandomState(1).uniform(-0.5, 0.5, (6, D)), np.random.RandomState(2).standard_normal((6, D))
    elif name == "reflecting":
        lo, hi = np.full(D, -0.6), np.array([0.6, np.inf, 0.5])
        q, p = np.random.RandomState(1).uniform(-0.5, 0.5, (6, D)), 2.0 * np.random.RandomState(2).standard_normal((6, D))
    else:
        lo, hi = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
        q, p = np.array([[0.9, 0.95]]), np.array([[3.0, 2.5]])
    qL, pL, refl = _traj(tgt, q, p, 0.1, 9, lo, hi, minv)
    if name == "reflecting":
        assert (refl.sum(axis=1) > 0).sum() >= 3
    if name == "corner":
        q1, _, _, _, info = hr.leapfrog(tgt, q, p, tgt.mg(q)[1], 0.1, minv, lo, hi)
        assert np.all(info["count"] == 1), "both dimensions reflect in the same drift"
    qb, pb, _ = _traj(tgt, qL, -pL, 0.1, 9, lo, hi, minv)
    assert np.allclose(qb, q, rtol=0, atol=1e-12) and np.allclose(-pb, p, rtol=0, atol=1e-12)


def test_energy_error_is_second_order():
    tgt = _smooth(3, seed=3)
    q, p = np.random.RandomState(4).uniform(-0.4, 0.4, (20, 3)), np.random.RandomState(5).standard_normal((20, 3))
    inf = np.full(3, np.inf)
    H = lambda q_, p_: hr.kinetic(p_, np.ones(3)) - tgt.mg(q_)[0]      # noqa: E731
    errs = []
    for eps, L in ((0.08, 8), (0.04, 16), (0.02, 32)):
        qL, pL, _ = _traj(tgt, q, p, eps, L, -inf, inf, np.ones(3))
        errs.append(np.abs(H(qL, pL) - H(q, p)).mean())
    print("mean |dH|", errs)
    assert 3.0 < errs[0] / errs[1] < 5.0 and 3.0 < errs[1] / errs[2] < 5.0


@pytest.mark.parametrize("reflecting", [False, True])
def test_one_step_preserves_volume(reflecting):
    tgt = _smooth(2, seed=6)
    minv = np.array([1.0, 0.6])
    lo, hi = np.array([-1.0, -1.0]), np.array([1.0, 0.3 if reflecting else 1.0])
    z0 = np.array([0.1, 0.2, 0.4, 1.5])

    def step(z):
        q, p = z[None, :2], z[None, 2:]
        q1, p1, _, _, info = hr.leapfrog(tgt, q, p, tgt.mg(q)[1], 0.2, minv, lo, hi)
        return np.concatenate([q1[0], p1[0]]), int(info["count"].sum())
    _, cnt = step(z0)
    assert cnt == (1 if reflecting else 0)
    h = 1e-6
    J = np.array([(step(z0 + h * e)[0] - step(z0 - h * e)[0]) / (2 * h) for e in np.eye(4)]).T
    assert abs(np.linalg.det(J) - 1.0) < 1e-7


@pytest.mark.parametrize("kern", ["se", "amp", "selin1", "amplin2"])
def test_gradient_is_the_derivative_of_the_oracle_mean(kern):
    import test_gpu_ensemble_replay as rp
    D = 3
    X, y, gp, gpo = hr.problem(D, 40, kern)
    model = hr.Model.from_gps(gp, gpo, y)
    q = np.random.RandomState(7).uniform(-1, 1, (5, D)) * model.sc
    mu, g = model.mg(q)
    lp = rp._oracle(gpo, y, D)
    assert np.allclose(mu, lp(q / model.sc), rtol=1e-10, atol=1e-10)
    h = 1e-5
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd = (lp((q + e) / model.sc) - lp((q - e) / model.sc)) / (2 * h)
        assert np.allclose(g[:, d], fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_free_run_on_a_gaussian_has_its_moments():
    from approxposterior_amd.mcmcUtils import batchMeansMCSE
    cov = np.array([[1.0, 0.6, 0.0], [0.6, 0.8, -0.2], [0.0, -0.2, 0.5]])
    c = np.array([0.3, -0.2, 0.1])
    tgt = hr.Gaussian(c, cov)
    inf = np.full(3, np.inf)
    T, C = 1500, 16
    r = hr.run(tgt, np.tile(c, (C, 1)), T, -inf, inf, 0.35, 6, jitter=0.2, seed=5)
    ch = r["chain"][100:]
    assert 0.6 < r["accept"].mean() <= 1.0
    series = ch.mean(axis=1)
    assert np.all(np.abs(series.mean(axis=0) - c) <= 5.0 * np.asarray(batchMeansMCSE(series)))
    d = ch - c
    prods = np.einsum("tci,tcj->tij", d, d).reshape(len(ch), 9) / C
    assert np.all(np.abs(prods.mean(axis=0) - cov.ravel()) <= 5.0 * np.asarray(batchMeansMCSE(prods)))


@pytest.mark.parametrize("c", hr.REPLAY_CASES, ids=hr.case_id)
def test_replay_inputs_leave_the_reference_few_near_ties(c):
    D, C, n, kern, L, eps, G, jitter, box = c
    X, y, gp, gpo, model, b, p0 = hr.case_inputs(c)
    sc = model.sc
    lo, hi = b[:, 0] * sc, b[:, 1] * sc
    r = hr.run(model, p0 * sc, hr.REPLAY_ITERATIONS, lo, hi, eps, L, jitter=jitter, seed=hr.REPLAY_SEED,
               canon=(sc, b[:, 0], b[:, 1]))
    f = hr.forced(model, p0 * sc, r["trace"], r["accept"], lo, hi, eps, L, jitter=jitter, seed=hr.REPLAY_SEED, G=G)
    live = ~f["gated"]
    assert np.array_equal(f["accept"], r["accept"]) and not r["diverge"].any()
    tie = live & (f["margin"] <= f["BdH"] + 4.0 * hr.U * np.abs(f["logu"]))
    print("%s: %d near-ties of %d, %d near-face drifts of %d, acceptance %.2f, reflecting %.2f, B_dH up to %.2e" % (
        hr.case_id(c), tie.sum(), tie.size, f["near"].sum(), f["near"].size, r["accept"][live].mean(),
        r["reflected"][live].mean(), f["BdH"][live].max()))
    assert tie.sum() <= hr.NEAR_CAP * tie.size and f["near"].sum() <= hr.NEAR_CAP * f["near"].size
    assert r["accept"][live].mean() > 0.3
    if box == "tight":
        assert r["reflected"][live].mean() >= 0.1
    if C >= 5:
        assert f["gated"][:, 0].all() and not r["accept"][:, 0].any()
