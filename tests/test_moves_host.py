"""CPU: the ensemble moves of mcmc.py (StretchMove, DEMove, DESnookerMove and weighted mixtures) on the host sampler --
argument handling, the untouched default stream, stationarity on a correlated Gaussian, the snooker's degenerate start --
and the refusal of bad move tables by apgp_ensemble_sample_moves before anything reaches a device.  The device side is
tests/test_gpu_ensemble_moves.py."""
import ctypes

import numpy as np
import pytest

from approxposterior_amd import _lib, mcmc

COV = np.array([[1.0, 0.6, 0.0], [0.6, 2.0, -0.5], [0.0, -0.5, 0.5]])
PREC = np.linalg.inv(COV)


def _gauss(x):
    x = np.atleast_2d(x)
    return -0.5 * np.einsum("ni,ij,nj->n", x, PREC, x)


def _flat(x):
    return 0.0


# ---------------------------------------------------------------------------------------------- argument handling
def test_every_accepted_form_of_moves():
    de, sn, st = mcmc.DEMove(), mcmc.DESnookerMove(), mcmc.StretchMove(2.5)
    assert mcmc.moves.DEMove is mcmc.DEMove and mcmc.moves.DESnookerMove is mcmc.DESnookerMove
    assert mcmc.moves.StretchMove is mcmc.StretchMove
    s = mcmc.EnsembleSampler(12, 3, _flat)
    assert len(s.moves) == 1 and isinstance(s.moves[0][0], mcmc.StretchMove) and s.moves[0][0].a == 2.0 and s.moves[0][1] == 1.0
    s = mcmc.EnsembleSampler(12, 3, _flat, a=3.0)
    assert s.moves[0][0].a == 3.0 and s.a == 3.0
    s = mcmc.EnsembleSampler(12, 3, _flat, moves=de)
    assert s.moves == [(de, 1.0)]
    s = mcmc.EnsembleSampler(12, 3, _flat, moves=[de, sn, st])
    assert [m for m, _ in s.moves] == [de, sn, st] and np.allclose([w for _, w in s.moves], 1.0 / 3.0)
    s = mcmc.EnsembleSampler(12, 3, _flat, moves=[(de, 4.0), (sn, 1.0)])
    assert [m for m, _ in s.moves] == [de, sn] and np.allclose([w for _, w in s.moves], [0.8, 0.2])
    s = mcmc.EnsembleSampler(12, 3, _flat, moves=[(de, 0.8), sn])                 # pairs and bare moves may be mixed
    assert np.allclose([w for _, w in s.moves], [0.8 / 1.8, 1.0 / 1.8])
    s = mcmc.EnsembleSampler(16, 3, _flat, moves=[de] * 8)
    assert len(s.moves) == 8 and abs(sum(w for _, w in s.moves) - 1.0) < 1e-15


def test_move_parameters_are_validated():
    assert mcmc.DEMove().sigma == 1.0e-5 and mcmc.DEMove().gamma0 is None and mcmc.DESnookerMove().gammas == 1.7
    assert mcmc.DEMove().g0(8) == 2.38 / np.sqrt(16.0) and mcmc.DEMove(gamma0=1.0).g0(8) == 1.0
    assert mcmc.DEMove(sigma=0.0).sigma == 0.0
    for bad in (lambda: mcmc.DEMove(sigma=-1e-3), lambda: mcmc.DEMove(gamma0=0.0), lambda: mcmc.DEMove(gamma0=-1.0),
                lambda: mcmc.DEMove(sigma=np.nan), lambda: mcmc.DESnookerMove(gammas=0.0),
                lambda: mcmc.DESnookerMove(gammas=np.inf), lambda: mcmc.StretchMove(a=1.0), lambda: mcmc.StretchMove(a=0.5)):
        with pytest.raises(ValueError):
            bad()


def test_bad_move_arguments_are_value_errors_and_pool_stays_refused():
    de, sn = mcmc.DEMove(), mcmc.DESnookerMove()
    with pytest.raises(ValueError):
        mcmc.EnsembleSampler(2, 1, _flat, moves=de)                  # DE needs W >= 4
    mcmc.EnsembleSampler(4, 1, _flat, moves=de)
    with pytest.raises(ValueError):
        mcmc.EnsembleSampler(4, 1, _flat, moves=sn)                  # the snooker needs W >= 6
    with pytest.raises(ValueError):
        mcmc.EnsembleSampler(4, 1, _flat, moves=[(de, 0.9), (sn, 0.1)])
    mcmc.EnsembleSampler(6, 1, _flat, moves=sn)
    with pytest.raises(ValueError):
        mcmc.EnsembleSampler(12, 3, _flat, a=3.0, moves=de)          # a belongs to the default stretch move
    mcmc.EnsembleSampler(12, 3, _flat, a=2.0, moves=de)
    with pytest.raises(ValueError):
        mcmc.EnsembleSampler(20, 3, _flat, moves=[de] * 9)           # more than 8 entries
    for bad in ([], [(de, 0.0)], [(de, -1.0)], [(de, np.nan)], ["de"], [(de, 1.0, 2.0)], 3.0):
        with pytest.raises(ValueError):
            mcmc.EnsembleSampler(12, 3, _flat, moves=bad)
    with pytest.raises(NotImplementedError):
        mcmc.EnsembleSampler(12, 3, _flat, pool=object())
    with pytest.raises(NotImplementedError):
        mcmc.EnsembleSampler(12, 3, _flat, moves=de, pool=object())


def test_device_chain_records_the_move_table():
    res = {"chain": np.zeros((5, 8, 2)), "log_prob": np.zeros((5, 8)), "naccept": np.zeros(8), "coords": np.zeros((8, 2)),
           "final_log_prob": np.zeros(8)}
    de, sn = mcmc.DEMove(), mcmc.DESnookerMove()
    dc = mcmc.DeviceChain(res, moves=[(de, 0.8), (sn, 0.2)])
    assert [m for m, _ in dc.moves] == [de, sn] and np.allclose([w for _, w in dc.moves], [0.8, 0.2]) and dc.a == 2.0
    dc = mcmc.DeviceChain(res, a=3.0)
    assert dc.a == 3.0 and len(dc.moves) == 1 and dc.moves[0][0].a == 3.0


# ---------------------------------------------------------------------------------------------- unchanged default
def _stretch_loop_as_it_stood(rs, lp_fn, p0, iterations, a):
    """The sampler's loop before it knew any other move (mcmc.py, EnsembleSampler.sample), restated on a bare RandomState."""
    coords = np.array(p0, dtype=float, copy=True)
    nw, nd = coords.shape
    lp = lp_fn(coords)
    chain = []
    for _ in range(iterations):
        inds = np.arange(nw) % 2
        rs.shuffle(inds)
        halves = (np.flatnonzero(inds == 0), np.flatnonzero(inds == 1))
        for split in range(2):
            S, C = halves[split], halves[1 - split]
            s, c = coords[S], coords[C]
            zz = ((a - 1.0) * rs.rand(len(S)) + 1.0) ** 2.0 / a
            factors = (nd - 1.0) * np.log(zz)
            rint = rs.randint(len(C), size=(len(S),))
            q = c[rint] - (c[rint] - s) * zz[:, None]
            new_lp = lp_fn(q)
            lnpdiff = factors + new_lp - lp[S]
            accepted = np.log(rs.rand(len(S))) < lnpdiff
            idx = S[accepted]
            coords[idx] = q[accepted]
            lp[idx] = new_lp[accepted]
        chain.append(coords.copy())
    return np.asarray(chain)


@pytest.mark.parametrize("a", [2.0, 1.7])
def test_default_draws_are_what_they_were(a):
    """moves=None: the chain and the RandomState's final state are those of the loop as it stood; at a = 2,
    moves=StretchMove(2.0) gives the same chain."""
    p0 = np.random.RandomState(5).normal(size=(12, 3))
    T, seed = 200, 314
    s0 = mcmc.EnsembleSampler(12, 3, _gauss, vectorize=True, seed=seed, a=a)
    s0.run_mcmc(p0, T)
    rs = np.random.RandomState(seed)
    want = _stretch_loop_as_it_stood(rs, _gauss, p0, T, a)
    assert np.array_equal(s0.get_chain(), want)
    after, ref = s0._random.get_state(), rs.get_state()
    assert after[0] == ref[0] and np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]
    if a == 2.0:
        s1 = mcmc.EnsembleSampler(12, 3, _gauss, vectorize=True, seed=seed, moves=mcmc.StretchMove(2.0))
        s1.run_mcmc(p0, T)
        assert np.array_equal(s1.get_chain(), s0.get_chain()) and np.array_equal(s1.get_log_prob(), s0.get_log_prob())


# ---------------------------------------------------------------------------------------------- stationarity
CONFIGS = {
    "de": lambda: mcmc.DEMove(),
    "snooker": lambda: mcmc.DESnookerMove(),
    "de+snooker": lambda: [(mcmc.DEMove(), 0.8), (mcmc.DESnookerMove(), 0.2)],
    "stretch+de+jump": lambda: [(mcmc.StretchMove(), 0.5), (mcmc.DEMove(), 0.4), (mcmc.DEMove(gamma0=1.0), 0.1)],
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_moves_leave_a_correlated_gaussian_stationary(name):
    """Zero-mean Gaussian, D = 3, W = 12, 6000 iterations of which the first 1000 are dropped, three seeds: every marginal
    mean within 0.12 standard deviations of zero and max|C^ - C| / max|C| <= 0.12 on every seed.  0.12: a stand-alone NumPy
    prototype of exactly these moves stayed within 0.06 (means) and 0.04 (covariance) over 8 seeds, and with a wrong
    snooker factor (0, (D - 1) / 2 or D in place of D - 1) gave 0.26 to 0.54 on the covariance: three times the worst
    correct value, under half the best wrong one."""
    L = np.linalg.cholesky(COV)
    for seed in (11, 12, 13):
        p0 = np.random.RandomState(1000 + seed).normal(size=(12, 3)) @ L.T
        s = mcmc.EnsembleSampler(12, 3, _gauss, vectorize=True, seed=seed, moves=CONFIGS[name]())
        s.run_mcmc(p0, 6000)
        x = s.get_chain(discard=1000, flat=True)
        mean_err = np.abs(x.mean(axis=0)) / np.sqrt(np.diag(COV))
        cov_err = np.abs(np.cov(x.T) - COV).max() / np.abs(COV).max()
        acc = s.acceptance_fraction.mean()
        print("%s seed %d: mean %.3f sd, covariance %.3f, acceptance %.3f" % (name, seed, mean_err.max(), cov_err, acc))
        assert np.all(np.isfinite(x)) and acc > 0.05
        assert np.all(mean_err <= 0.12), (name, seed, mean_err)
        assert cov_err <= 0.12, (name, seed, cov_err)


# ---------------------------------------------------------------------------------------------- degenerate start
def test_snooker_from_identical_walkers_rejects_instead_of_spreading_nan():
    """Three walkers at one point and three at another, so that whatever the halves are a walker's pivot z is often a
    copy of itself in the other half (counted): those proposals are NaN and are rejected -- nothing non-finite reaches the
    log-probability function, the chain or the stored log-probabilities -- while the other proposals move the ensemble."""
    p0 = np.array([[0.4, -0.3]] * 3 + [[-0.2, 0.5]] * 3)
    seen = {"nan_in": 0, "nan_proposed": 0}

    def lp(x):
        seen["nan_in"] += int(np.sum(~np.isfinite(x)))
        return -0.5 * np.sum(np.atleast_2d(x) ** 2, axis=1)
    s = mcmc.EnsembleSampler(6, 2, lp, vectorize=True, seed=9, moves=mcmc.DESnookerMove())
    inner = s._propose

    def spy(move, act, comp):
        q, f = inner(move, act, comp)
        seen["nan_proposed"] += int(np.sum(np.any(np.isnan(q), axis=1)))
        return q, f
    s._propose = spy
    s.run_mcmc(p0, 200)
    assert seen["nan_proposed"] > 0, "the start never produced s == z: the test shows nothing"
    assert seen["nan_in"] == 0 and np.all(np.isfinite(s.get_chain())) and np.all(np.isfinite(s.get_log_prob()))
    assert s._naccepted.sum() > 0


def test_a_nan_snooker_proposal_is_a_rejection():
    """_propose on a walker that IS its pivot: q is NaN and the factor -inf; sample() then keeps the walker where it is."""
    s = mcmc.EnsembleSampler(6, 2, _flat, seed=1, moves=mcmc.DESnookerMove())
    pts = np.array([[0.3, -0.2]] * 3)
    comp = np.array([[0.3, -0.2]] * 3)                # every complement walker equals every active walker: s == z always
    q, f = s._propose(s.moves[0][0], pts, comp)
    assert np.all(np.isnan(q)) and np.all(np.isneginf(f))
    p0 = np.array([[0.3, -0.2]] * 6)
    calls = []
    s2 = mcmc.EnsembleSampler(6, 2, lambda x: calls.append(np.array(x)) or np.zeros(len(x)), vectorize=True, seed=1,
                              moves=mcmc.DESnookerMove())
    s2.run_mcmc(p0, 5)
    assert np.array_equal(s2.get_chain(), np.broadcast_to(p0, (5, 6, 2))) and np.all(s2._naccepted == 0)
    assert all(np.all(np.isfinite(c)) for c in calls)


# ---------------------------------------------------------------------------------------------- C ABI: bad tables
def _moves_call(lib, W, recs, nmoves=None, null_table=False):
    ks = _lib.KernelStruct()
    ks.ndim, ks.lin_order, ks.amp, ks.diag_add, ks.lin_coef = 2, 0, 1.0, 0.0, 0.0
    for d in range(2):
        ks.inv_metric[d] = 1.0
    buf = (ctypes.c_double * 4096)()
    ibuf = (ctypes.c_int64 * 512)()
    lo = (ctypes.c_double * _lib.MAX_DIM)(*([-1.0] * _lib.MAX_DIM))
    hi = (ctypes.c_double * _lib.MAX_DIM)(*([1.0] * _lib.MAX_DIM))
    table = (_lib.EnsMove * max(1, len(recs)))()
    for r, (kind, w, p0, p1) in zip(table, recs):
        r.kind, r.weight, r.p0, r.p1 = kind, w, p0, p1
    p = ctypes.addressof(buf)
    return lib.apgp_ensemble_sample_moves(p, 8, ctypes.byref(ks), 0.0, lo, hi, W, 1, 1, 2.0, 7, p, p, None, None,
                                          ctypes.addressof(ibuf), 1, None if null_table else table,
                                          len(recs) if nmoves is None else nmoves, None)


def test_bad_move_tables_are_refused_without_a_gpu():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.EnsMove) == 32 and _lib.ENS_MAX_MOVES == 8
    S, DE, SN = _lib.ENS_MOVE_STRETCH, _lib.ENS_MOVE_DE, _lib.ENS_MOVE_SNOOKER
    inf, nan = float("inf"), float("nan")
    bad = [
        (8, [(DE, 1.0, 1e-5, 0.0)], 0, b"nmoves"),                         # nmoves out of range
        (8, [(DE, 1.0, 1e-5, 0.0)], 9, b"nmoves"),
        (8, [(DE, 1.0, 1e-5, 0.0)], -1, b"nmoves"),
        (8, [(3, 1.0, 1.0, 0.0)], None, b"unknown move kind"),
        (8, [(-1, 1.0, 1.0, 0.0)], None, b"unknown move kind"),
        (8, [(DE, 0.0, 1e-5, 0.0)], None, b"weights"),
        (8, [(DE, -1.0, 1e-5, 0.0)], None, b"weights"),
        (8, [(DE, nan, 1e-5, 0.0)], None, b"weights"),
        (8, [(S, 0.5, 2.0, 0.0), (DE, inf, 1e-5, 0.0)], None, b"weights"),
        (8, [(S, 1.0, 1.0, 0.0)], None, b"stretch"),
        (8, [(S, 1.0, nan, 0.0)], None, b"stretch"),
        (8, [(DE, 1.0, -1e-5, 0.0)], None, b"sigma"),
        (8, [(DE, 1.0, inf, 0.0)], None, b"sigma"),
        (8, [(DE, 1.0, 1e-5, -1.0)], None, b"gamma0"),
        (8, [(DE, 1.0, 1e-5, nan)], None, b"gamma0"),
        (8, [(SN, 1.0, 0.0, 0.0)], None, b"gammas"),
        (8, [(SN, 1.0, nan, 0.0)], None, b"gammas"),
        (4, [(S, 0.5, 2.0, 0.0), (SN, 0.5, 1.7, 0.0)], None, b"6 walkers"),   # too few walkers for a listed move
    ]
    for W, recs, nmoves, msg in bad:
        assert _moves_call(lib, W, recs, nmoves) == -1, (W, recs, nmoves)
        err = lib.apgp_last_error()
        assert b"apgp_ensemble_sample_moves" in err and msg in err, (recs, err)
    assert _moves_call(lib, 8, [], 3, null_table=True) == -1 and b"NULL" in lib.apgp_last_error()
    # W = 2 < 4 for DE: refused by the table check (ndim 1 so that W >= 2 ndim holds)
    ks = _lib.KernelStruct()
    ks.ndim, ks.amp = 1, 1.0
    ks.inv_metric[0] = 1.0
    buf = (ctypes.c_double * 4096)()
    ibuf = (ctypes.c_int64 * 16)()
    lo = (ctypes.c_double * _lib.MAX_DIM)(*([-1.0] * _lib.MAX_DIM))
    hi = (ctypes.c_double * _lib.MAX_DIM)(*([1.0] * _lib.MAX_DIM))
    table = (_lib.EnsMove * 1)()
    table[0].kind, table[0].weight, table[0].p0, table[0].p1 = DE, 1.0, 1e-5, 0.0
    p = ctypes.addressof(buf)
    assert lib.apgp_ensemble_sample_moves(p, 8, ctypes.byref(ks), 0.0, lo, hi, 2, 1, 1, 2.0, 7, p, p, None, None,
                                          ctypes.addressof(ibuf), 1, table, 1, None) == -1
    assert b"4 walkers" in lib.apgp_last_error()
    # the old entry points still refuse a <= 1 before any launch
    assert lib.apgp_ensemble_sample_ex(p, 8, ctypes.byref(ks), 0.0, lo, hi, 2, 1, 1, 1.0, 7, p, p, None, None,
                                       ctypes.addressof(ibuf), 1, None) == -1
    assert b"stretch" in lib.apgp_last_error()
