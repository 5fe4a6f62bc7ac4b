"""GPU (``-m gpu``): the argument handling the acquisition entry points of GP share (gp.py: ``_box``, ``_candidates``,
``_mask``, the routes behind ``predict`` and the one sweep behind ``acquire`` / ``acquire_batch``).

Shape: N = 20, D = 2, M = 70 -- two 64-candidate blocks, the second ragged: the smallest at which block and offset
handling can go wrong.  Both variance forms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
N, D, M = 20, 2, 70
BOX = [(-5.0, 5.0)] * D
MODES = ["inverse", "solve"]
DERIVED = ("_xs", "_packed", "_packed_solve", "_work", "_alpha")


def _fixture(mode):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(5)
    X = rs.uniform(-5.0, 5.0, size=(N, D))
    y = -(100.0 * (X[:, 1] - X[:, 0] ** 2) ** 2 + (1.0 - X[:, 0]) ** 2) / 1000.0
    metric, log_c, wn = np.array([9.0, 16.0]), float(np.log(np.var(y) / D)), -12.0
    gp = agp.GP(kernel=agp.Product(agp.ConstantKernel(log_c, ndim=D), agp.ExpSquaredKernel(metric, ndim=D)),
                fit_mean=True, mean=float(np.mean(y)), white_noise=wn, fit_white_noise=False)
    gp.variance_mode = mode
    gp.compute(X)
    T = rs.uniform(-5.5, 5.5, size=(M, D))
    mask = rs.rand(M) > 0.2                  # refuses about a fifth of the rows
    # the bound of test_gpu_parity.py for mu and sigma^2: 200 cond(K) eps, times sum |alpha| for mu
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 / metric).sum(axis=2)
    K = D * np.exp(log_c) * np.exp(-0.5 * d2) + np.exp(wn) * np.eye(N)
    tol = max(1e-13, 200 * np.linalg.cond(K) * EPS)
    tol_mu = tol * max(np.abs(np.linalg.solve(K, y - np.mean(y))).sum(), 1e-300)
    return gp, y, T, mask, tol_mu, tol


def _refused(call, exc=ValueError):
    with pytest.raises(exc) as info:
        call()
    return str(info.value)


@pytest.mark.parametrize("mode", MODES)
def test_refusals_are_uniform_and_come_before_device_work(mode):
    import torch
    gp, y, T, mask, _, _ = _fixture(mode)
    Td = torch.from_numpy(T).cuda()
    starts, walkers = T[:3], T[:8]

    bad_box = BOX + [(-5.0, 5.0)]
    box_messages = {
        _refused(lambda: gp.acquire(y, T, "agp", bounds=bad_box)),
        _refused(lambda: gp.acquire(y, Td, "agp", bounds=bad_box)),
        _refused(lambda: gp.acquire_batch(y, T, "agp", 2, bounds=bad_box)),
        _refused(lambda: gp.nelder_mead_search(y, starts, "agp", bounds=bad_box)),
        _refused(lambda: gp.box_candidates(M, bad_box, seed=1)),
        _refused(lambda: gp.sample_ensemble(y, walkers, 2, bad_box)),
    }
    assert box_messages == {"bounds must have one (lo, hi) pair per dimension"}

    mask_messages = {
        _refused(lambda: gp.acquire(y, T, "agp", mask=mask[:-1])),
        _refused(lambda: gp.acquire(y, Td, "agp", mask=mask[:-1])),
        _refused(lambda: gp.acquire_batch(y, T, "agp", 2, mask=mask[:-1])),
        _refused(lambda: gp.acquire_batch(y, Td, "agp", 2, mask=mask[:-1])),
    }
    assert mask_messages == {"mask must have one entry per candidate"}

    wide = torch.zeros((M, 2 * D), dtype=torch.float64, device="cuda")
    tensors = [Td.float(), wide[:, :D], torch.from_numpy(T)]      # float32, non-contiguous, on the host
    assert not tensors[1].is_contiguous() and tensors[1].shape == (M, D)
    tensor_messages = set()
    for t in tensors:
        tensor_messages.add(_refused(lambda: gp.acquire(y, t, "agp")))
        tensor_messages.add(_refused(lambda: gp.acquire(y, t, "agp", device_record=True)))
        tensor_messages.add(_refused(lambda: gp.acquire_batch(y, t, "agp", 2)))
    assert tensor_messages == {"device candidates must be a contiguous (M, D) float64 CUDA tensor"}

    _refused(lambda: gp.acquire(y, T, "nosuch"), KeyError)
    _refused(lambda: gp.acquire_batch(y, T, "nosuch", 2), KeyError)
    _refused(lambda: gp.acquire_batch(y, T, ["agp", "nosuch"], 2), KeyError)
    _refused(lambda: gp.nelder_mead_search(y, starts, "nosuch"))
    _refused(lambda: gp.acquire_batch(y, T, "agp", 0))
    _refused(lambda: gp.acquire_batch(y, T, ["agp", "bape", "agp"], 2))
    _refused(lambda: gp.nelder_mead_search(y, starts, "agp", options={"xtol": 1e-3}))
    _refused(lambda: gp.nelder_mead_search(y, starts, "agp", options={"maxiter": 0}))

    for name in DERIVED:
        assert getattr(gp, name) is None, name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["agp", "bape", "jones"])
def test_a_batch_of_one_is_acquire_with_every_argument(kind, device, mode):
    import torch
    gp, y, T, mask, _, _ = _fixture(mode)
    t = torch.from_numpy(T).cuda() if device else T
    kw = dict(bounds=BOX, mask=mask, idx_offset=1000, return_all=True)
    bi, bu, u, mu, var = gp.acquire(y, t, kind, **kw)
    idx, ub, u_b, mu_b, var_b = gp.acquire_batch(y, t, kind, 1, **kw)
    assert 1000 <= bi < 1000 + M and mask[bi - 1000] and np.all(np.abs(T[bi - 1000]) <= 5.0)
    assert idx.tolist() == [bi]
    assert np.float64(ub[0]).tobytes() == np.float64(bu).tobytes()
    for a, b in ((u, u_b), (mu, mu_b), (var, var_b)):
        assert a.shape == (M,) and a.tobytes() == b.tobytes()
    assert np.all(np.isposinf(u[~mask])) and bu == u[bi - 1000]


@pytest.mark.parametrize("mode", MODES)
def test_the_routes_of_predict_agree_where_they_overlap(mode):
    gp, y, T, mask, tol_mu, tol = _fixture(mode)
    # the sweep (M rows) and the one-candidate route at row 0
    mu, var = gp.predict(y, T, return_var=True)
    mu1, var1 = gp.predict(y, T[:1], return_var=True)
    assert mu1.shape == var1.shape == (1,) and "one" in gp._replays
    print("one-candidate route against the sweep: |dmu| = %.3e (bound %.3e), |dvar| = %.3e (bound %.3e)"
          % (abs(mu1[0] - mu[0]), tol_mu, abs(var1[0] - var[0]), tol))
    assert abs(mu1[0] - mu[0]) <= tol_mu and abs(var1[0] - var[0]) <= tol
    # the host-buffer mean route, then its replay
    m_first = gp.predict(y, T, return_cov=False)
    replay = gp._replays["mean"]
    m_again = gp.predict(y, T, return_cov=False)
    assert gp._replays["mean"] is replay        # (the generic path would have planted a new one)
    assert replay.args[6] == m_again.ctypes.data    # ... and the replay wrote the second result
    assert m_first.shape == (M,) and m_first.tobytes() == m_again.tobytes()
    # ... against the sweep's mean array.  Not bit for bit, and it was not before the routes were split either (same
    # library calls): the mean-only kernel sums k(t, X) alpha in its own order, the sweep on the matrix cores -- 2e-12
    # apart at this shape on an MI355X in both variance forms.  So the bound of test_gpu_parity.py for mu, as above.
    mu_all = gp.acquire(y, T, "agp", return_all=True)[3]
    print("host-buffer mean route against the sweep: max |dmu| = %.3e (bound %.3e)"
          % (np.abs(m_first - mu_all).max(), tol_mu))
    assert np.abs(m_first - mu_all).max() <= tol_mu


@pytest.mark.parametrize("mode", MODES)
def test_the_prune_switch_and_the_event_hook_are_restored(mode):
    from approxposterior_amd import _lib
    gp, y, T, mask, _, _ = _fixture(mode)
    lib = _lib.load()
    was = lib.apgp_set_sweep_prune(1)
    try:
        gp.sweep_prune = 0
        want = gp.acquire(y, T, "bape", bounds=BOX, mask=mask)
        assert lib.apgp_get_sweep_prune() == 1
        # a call the library itself refuses before it touches the GPU: a zero amplitude in the kernel struct (planted
        # behind the object's back, so that the factor, alpha and the packed buffers of the call above still stand)
        log_c = gp.kernel.k1.log_constant
        gp.kernel.k1.log_constant = -np.inf
        try:
            assert gp.computed
            with pytest.raises(_lib.ApgpError, match="kernel parameters"):
                gp.acquire(y, T, "bape", bounds=BOX, mask=mask)
        finally:
            gp.kernel.k1.log_constant = log_c
        assert lib.apgp_get_sweep_prune() == 1
        gp.kernel_events = []
        assert gp.acquire(y, T, "bape", bounds=BOX, mask=mask) == want
        assert len(gp.kernel_events) == 1 and len(gp.kernel_events[0]) == 2
        assert lib.apgp_get_sweep_prune() == 1
    finally:
        lib.apgp_set_sweep_prune(was)
