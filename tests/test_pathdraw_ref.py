"""CPU: posterior function draws without a GPU -- the entry points of the C ABI (exported, bound, sized, refusing bad
arguments before any HIP call), the NumPy restatement of tests/pathdraw_ref.py (the mean with zero weights, the
training-point identity, the moments of many draws against the predictive mean and the surrogate variance, a budget that
is not vacuous) and the argument checks of batchMethod / bayesOpt(batchSize=)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from approxposterior_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kvalue_ref as kr  # noqa: E402
import pathdraw_ref as pr  # noqa: E402


def test_path_draws_entry_points_are_exported_bound_and_sized():
    lib = _lib.load()
    for name in ("apgp_path_draws", "apgp_path_draws_work_len", "apgp_path_draws_mode"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # the contraction switch: returns the previous value, a negative argument only queries, 3 is refused
    was = lib.apgp_path_draws_mode(-1)
    assert lib.apgp_path_draws_mode(2) == was and lib.apgp_path_draws_mode(-1) == 2
    assert lib.apgp_path_draws_mode(3) == -1 and lib.apgp_path_draws_mode(was) == 2
    assert lib.apgp_abi_version() == 8 and _lib.MAX_DRAWS == 32 == pr.MAX_DRAWS
    assert _lib.MAX_FEATURES == pr.MAX_FEATURES
    # one (value, index) partial per 256-candidate workgroup and draw
    for m, s in ((1, 1), (256, 5), (257, 5), (10 ** 6, 32), (0, 3), (5, 0), (1 << 41, 1), (5, 33)):
        assert lib.apgp_path_draws_work_len(m, s) == pr.work_len(m, s)
    assert lib.apgp_path_draws_work_len(10 ** 6, 16) == 2 * 16 * 3907


def _call(lib, **kw):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ks = _lib.KernelStruct()
    ks.ndim = 2
    ks.amp = 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    a = dict(T=p, m=4, off=0, xs=p, n=4, mean=0.0, V=p, Z=p, b=p, W=p, Wl=p, R=4, S=2, lo=None, hi=None, mask=None,
             F=None, part=p, best=p)
    a.update(kw)
    if "ndim" in kw:
        ks.ndim = kw["ndim"]
    if "lin_coef" in kw:
        ks.lin_coef = kw["lin_coef"]
    return lib.apgp_path_draws(a["T"], a["m"], a["off"], a["xs"], a["n"], ctypes.byref(ks), a["mean"], a["V"], a["Z"],
                               a["b"], a["W"], a["Wl"], a["R"], a["S"], a["lo"], a["hi"], a["mask"], a["F"], a["part"],
                               a["best"], None)


@pytest.mark.parametrize("bad, message", [
    (dict(T=None), b"null pointer"), (dict(Z=None), b"null pointer"), (dict(b=None), b"null pointer"),
    (dict(W=None), b"null pointer"), (dict(part=None), b"null pointer"), (dict(best=None), b"null pointer"),
    (dict(xs=None), b"xs is required"), (dict(Wl=None, lin_coef=0.5), b"Wl is required"),
    (dict(S=0), b"APGP_MAX_DRAWS"), (dict(S=33), b"APGP_MAX_DRAWS"), (dict(S=-1), b"APGP_MAX_DRAWS"),
    (dict(R=0), b"APGP_MAX_FEATURES"), (dict(R=65537), b"APGP_MAX_FEATURES"),
    (dict(m=0), b"m >= 1"), (dict(m=1 << 41), b"m >= 1"), (dict(n=0), b"n >= 1"),
    (dict(ndim=_lib.MAX_DIM + 1), b"kernel parameters"),
    (dict(lo=(ctypes.c_double * _lib.MAX_DIM)()), b"together"),
])
def test_path_draws_bad_arguments_are_refused_without_a_gpu(bad, message):
    lib = _lib.load()
    assert _call(lib, **bad) == -1
    assert message in lib.apgp_last_error()


def test_cosine_restatement_is_within_its_term_of_the_budget():
    rs = np.random.RandomState(0)
    p = np.concatenate([rs.uniform(-40.0, 40.0, 200000), rs.uniform(-0.5, 0.5, 100000), np.arange(-8, 9) * 0.125,
                        rs.uniform(-1e-9, 1e-9, 1000), [0.25, -0.25, 0.5, 1e6 + 0.375]])
    want = np.cos(np.longdouble("6.283185307179586476925286766559005768") * np.asarray(p, dtype=np.longdouble))
    err = np.abs(pr.cos_turns_restate(p) - want).astype(np.float64)
    # the phase is taken as given here: only 2 pi p's long-double rounding (|p| 2^-63) joins the polynomial's term
    assert np.all(err <= pr.E_COS * pr.U + 2.0 * np.pi * np.abs(p) * 2.0 ** -62), err.max() / pr.U


def _zero_weight_case(order):
    c = pr.case(40, 25, 96, 3, 3, order=order, seed=5 + (order or 0))
    c["W"] = np.zeros_like(c["W"])
    c["Wl"] = np.zeros_like(c["Wl"])
    return c


@pytest.mark.parametrize("order", [None, 0, 2])
def test_zero_weights_give_the_predictive_mean(order):
    c = _zero_weight_case(order)
    k, X, T = c["k"], c["X"], c["T"]
    rs = np.random.RandomState(1)
    y = rs.standard_normal(len(X))
    K = kr.truth_ld(X, None, k).astype(np.float64)
    alpha = np.linalg.solve(K, y - c["mean"])
    V = np.repeat(alpha[:, None], 3, axis=1)
    F = pr.draws(T, X, V, c["Z"], c["b"], c["W"], c["Wl"], k, c["mean"])
    mu = c["mean"] + kr.truth_ld(T, X, k).astype(np.float64) @ alpha
    tol = 4 * len(X) * pr.U * (abs(c["mean"]) + np.abs(kr.truth_ld(T, X, k).astype(np.float64)) @ np.abs(alpha))
    assert np.all(np.abs(F - mu) <= tol)


@pytest.mark.parametrize("order", [None, 1])
def test_training_point_identity(order):
    """f_s(X) = y - eps_s - diag_add v_s, to the residual of the host's solve."""
    c = pr.case(48, 1, 128, 4, 2, order=order, seed=9)
    k, X = c["k"], c["X"]
    rs = np.random.RandomState(2)
    y = rs.standard_normal(len(X))
    eps = np.sqrt(k.diag_add) * rs.standard_normal((4, len(X)))
    K = kr.truth_ld(X, None, k).astype(np.float64)
    gX = pr.draws(X, None, None, c["Z"], c["b"], c["W"], c["Wl"], k, 0.0)            # (S, n)
    rhs = (y - c["mean"])[:, None] - gX.T - eps.T
    V = np.linalg.solve(K, rhs)
    F = pr.draws(X, X, V, c["Z"], c["b"], c["W"], c["Wl"], k, c["mean"])
    want = y[None, :] - eps - k.diag_add * V.T
    resid = np.abs(K @ V - rhs).T                                                    # what the solve left
    mag = pr.budget(X, X, V, c["Z"], c["b"], c["W"], c["Wl"], k, c["mean"])[1]
    assert np.all(np.abs(F - want) <= resid + 8 * len(X) * pr.U * mag)


MOMENT_SEEDS = (0, 3)


@pytest.mark.parametrize("seed", MOMENT_SEEDS)
def test_moments_of_many_draws(seed):
    """4096 draws in batches of 32 at 16 points: the mean within 5 standard errors of mu, s^2 / v-hat within
    5 sqrt(2 / S) of 1 (v-hat: the variance of the draws for the fixed features)."""
    fx = pr.moment_fixture(seed)
    k, y, mean = fx["k"], fx["y"], fx["mean"]
    rs = np.random.RandomState(1000 + seed)
    F = []
    for _ in range(4096 // 32):
        W = rs.standard_normal((32, fx["phiT"].shape[1]))
        eps = np.sqrt(k.diag_add) * rs.standard_normal((32, len(y)))
        F.append(pr.fast_draws(fx["phiT"], fx["phiX"], fx["Kxt"], fx["solve"], y, mean, W, eps)[0])
    F = np.vstack(F)
    mu = mean + fx["Kxt"].T @ fx["solve"](y - mean)
    vhat = pr.surrogate_variance(fx["phiT"], fx["phiX"], fx["Kxt"], fx["solve"], k.diag_add)
    assert np.all(vhat > 0.0)
    zm, zv = pr.moment_scores(F, mu, vhat)
    print("max |z| mean %.2f variance %.2f" % (np.abs(zm).max(), np.abs(zv).max()))
    assert np.abs(zm).max() <= 5.0 and np.abs(zv).max() <= 5.0
    # and the surrogate variance is the GP's up to the feature approximation, O(R^-1/2)
    var = k.amp - np.sum(fx["Kxt"] * fx["solve"](fx["Kxt"]), axis=0)
    assert np.abs(vhat - var).max() <= 5.0 * k.amp / np.sqrt(len(fx["Z"]))


@pytest.mark.parametrize("order", [None, 0, 1, 2])
def test_the_budget_is_not_vacuous(order):
    c = pr.case(130, 20, 1028, 5, 8, order=order, seed=4)
    bud, mag = pr.budget(c["T"], c["X"], c["V"], c["Z"], c["b"], c["W"], c["Wl"], c["k"], c["mean"])
    assert np.all(bud > 0.0) and np.all(bud <= 1e-10 * mag), (bud / mag).max()
    fx = pr.moment_fixture(0)
    W = np.random.RandomState(0).standard_normal((2, 4096))
    V = np.random.RandomState(1).standard_normal((64, 2))
    bud, mag = pr.budget(fx["T"], fx["X"], V, fx["Z"], fx["b"], W, np.zeros((2, 2)), fx["k"], fx["mean"])
    assert np.all(bud <= 1e-10 * mag), (bud / mag).max()


def test_argmin_contract_of_the_restatement():
    F = np.array([1.0, 3.0, np.nan, 3.0, 7.0, 2.0])
    adm = np.array([1, 1, 1, 1, 0, 1], dtype=bool)
    assert pr.argmin(F, adm, 10) == (11, -3.0)                   # ties -> the lowest index; NaN and the gated 7 never win
    assert pr.argmin(F, np.zeros(6, dtype=bool)) == (-1, np.inf)
    T = np.array([[0.0, 0.0], [np.nan, 0.0], [3.0, 0.0], [1.0, 1.0]])
    assert pr.admissible(T, bounds=[(-2, 2), (-2, 2)], mask=[1, 1, 1, 0]).tolist() == [True, False, False, False]


class _NoDevice(object):
    """A stand-in GP: any method call would be device work."""

    def __getattr__(self, name):
        raise AssertionError("device work before the argument checks: GP.%s" % name)


def _ap():
    from approxposterior_amd import approx, likelihood as lh
    theta = np.array([[0.0, 1.0], [1.0, 2.0], [-1.0, 0.5]])
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    return approx.ApproxPosterior(theta=theta, y=y, gp=_NoDevice(), lnprior=lh.rosenbrockLnprior,
                                  lnlike=lh.rosenbrockLnlike, priorSample=lh.rosenbrockSample,
                                  bounds=[(-5, 5), (-5, 5)], algorithm="bape", distributed=False)


@pytest.mark.parametrize("kw", [dict(batchMethod="thompson"), dict(batchMethod="thompson", nCandidates=100),
                                dict(batchMethod="kriging", batchSize=2, nCandidates=100),
                                dict(batchMethod="thompson", batchSize=33, nCandidates=100),
                                dict(batchMethod="thompson", batchSize=2)])
def test_batch_method_arguments_are_checked_first(kw, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    with pytest.raises(ValueError):
        ap.findNextPoint(computeLnLike=True, numNewPoints=4, verbose=False, **kw)
    assert len(ap.y) == 3


@pytest.mark.parametrize("kw", [dict(batchMethod="thompson"), dict(batchMethod="kriging", batchSize=2, nCandidates=100)])
def test_run_checks_batch_method_first(kw, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    with pytest.raises(ValueError):
        ap.run(m=4, nmax=1, verbose=False, cache=False, **kw)
    assert len(ap.y) == 3


def test_thompson_batches_under_a_process_group_are_not_implemented(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    monkeypatch.setattr(ap, "_ranks", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="process group"):
        ap.findNextPoint(computeLnLike=False, numNewPoints=4, nCandidates=100, batchSize=2, batchMethod="thompson",
                         verbose=False)


@pytest.mark.parametrize("kw", [dict(batchSize=2), dict(batchSize=0, nCandidates=100), dict(batchSize=33, nCandidates=100),
                                dict(batchSize=2.5, nCandidates=100), dict(batchMethod="thompson", nCandidates=100),
                                dict(batchSize=2, nCandidates=100, batchMethod="kriging")])
def test_bayes_opt_batch_arguments_are_checked_first(kw, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ap = _ap()
    with pytest.raises(ValueError):
        ap.bayesOpt(nmax=2, verbose=False, cache=False, **kw)
    assert len(ap.y) == 3
