# -*- coding: utf-8 -*-
"""CPU: the autocorrelation estimator's host side -- the NumPy restatement of the device sums (tests/autocorr_ref.py)
against today's FFT estimator, the C entry's argument checks, the ``deviceAutocorr`` keyword's guard, and the
block-growing loop of ``mcmc.integrated_time(onDevice=True)`` driven by a stub that serves the autocorrelation function
from the restatement.  No device code runs here."""
import ctypes

import numpy as np
import pytest

import autocorr_ref as ar
import george_oracle as go
from approxposterior_amd import _lib, approx, likelihood as lh, mcmc


@pytest.mark.parametrize("case", range(len(ar.CHAINS)))
def test_direct_sums_agree_with_the_fft_estimator(case):
    n_t, n_w, n_d, rhos = ar.CHAINS[case]
    x = ar.ar1_chain(n_t, n_w, n_d, rhos)
    want = mcmc.integrated_time(x, tol=0)
    tau_h, win_h, margin = ar.host_windows(x)
    assert np.allclose(tau_h, want, rtol=1e-12, atol=0)          # host_windows is the host estimator, window exposed
    tau, win = ar.integrated_time_direct(x)
    print("windows", win, "max rel", np.max(np.abs(tau - want) / np.abs(want)), "margin", margin.min())
    assert np.array_equal(win, win_h)
    assert np.max(np.abs(tau - want) / np.abs(want)) <= 1e-12


def test_bad_arguments_are_refused_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(8)          # never dereferenced: the checks come before any HIP call
    ok = dict(x=one, n_t=100, n_w=4, n_d=2, row0=0, stride=1, lag0=0, nlags=16, reuse=0, work=one, f=one)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.apgp_autocorr_block(a["x"], a["n_t"], a["n_w"], a["n_d"], a["row0"], a["stride"], a["lag0"], a["nlags"],
                                       a["reuse"], a["work"], a["f"], None)
    for bad, text in ((dict(x=None), b"null pointer"), (dict(work=None), b"null pointer"), (dict(f=None), b"null pointer"),
                      (dict(n_t=0), b"n_t"), (dict(n_t=1 << 31), b"n_t"), (dict(n_w=0), b"n_w"),
                      (dict(n_d=0), b"n_d"), (dict(n_d=_lib.MAX_DIM + 1), b"n_d"), (dict(nlags=0), b"nlags"),
                      (dict(nlags=1 << 31), b"nlags"), (dict(lag0=-1), b"lag0"), (dict(stride=0), b"row_stride"),
                      (dict(row0=-1), b"row0"),
                      (dict(n_t=(1 << 31) - 1, stride=(1 << 31) - 1, n_w=1 << 24, n_d=32), b"2^60")):
        assert call(**bad) == -1, bad
        msg = lib.apgp_last_error()
        assert b"apgp_autocorr_block" in msg and b"bad argument" in msg and text in msg, (bad, msg)
    assert lib.apgp_autocorr_work_len(0, 4, 2) == -1 and lib.apgp_autocorr_work_len(100, 4, 33) == -1
    assert lib.apgp_autocorr_work_len(100, 0, 2) == -1 and lib.apgp_autocorr_work_len(1 << 31, 4, 2) == -1
    # means, A(0) and one 256-lag block of partials per time chunk (64-step tiles in at most 32 chunks)
    assert lib.apgp_autocorr_work_len(100, 4, 2) == 8 * (2 + 256 * 2)
    assert lib.apgp_autocorr_work_len(1, 1, 1) == 2 + 256
    assert lib.apgp_autocorr_work_len(20000, 64, 8) == 512 * (2 + 256 * 32)


def _host_ap():
    np.random.seed(57)
    theta = np.array(list(lh.rosenbrockSample(20)) + [[-5, 5], [5, 5]])
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = go.GP(kernel=go.ExpSquaredKernel(metric=[1.0, 1.0], ndim=2), fit_mean=True, mean=np.median(y), white_noise=-12,
               fit_white_noise=False)
    gp.compute(theta)
    return approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                  priorSample=lh.rosenbrockSample, bounds=((-5, 5), (-5, 5)), algorithm="bape")


def test_device_autocorr_needs_the_device_sampler():
    ap = _host_ap()
    with pytest.raises(ValueError, match="onDevice=True"):
        ap.runMCMC(samplerKwargs={"nwalkers": 4}, mcmcKwargs={"iterations": 5}, cache=False, onDevice=False,
                   deviceAutocorr=True)
    with pytest.raises(ValueError, match="onDevice=True"):
        ap.run(m=1, nmax=1, cache=False, verbose=False, onDevice=False, deviceAutocorr=True)
    assert ap.sampler is None if hasattr(ap, "sampler") else True


class _Stub(object):
    """serves blocks of the restatement's f; remembers what was asked for"""

    def __init__(self, x):
        self.x, self.asked = np.asarray(x), []

    def __call__(self, lag0, nlags):
        self.asked.append((lag0, nlags))
        return ar.acf_direct(self.x, lag0, nlags)


def _run_stubbed(monkeypatch, x, block, cap, **kw):
    stubs = []

    def make(xd):
        stubs.append(_Stub(xd))
        return stubs[-1]
    monkeypatch.setattr(mcmc, "_device_acf", make)
    monkeypatch.setattr(mcmc, "AUTOCORR_BLOCK", block)
    monkeypatch.setattr(mcmc, "AUTOCORR_LAG_CAP", cap)
    before = mcmc.autocorr_fallbacks
    tau = mcmc.integrated_time(x, onDevice=True, **kw)
    assert len(stubs) == 1
    return tau, stubs[0].asked, mcmc.autocorr_fallbacks - before


def test_block_growing_loop_matches_the_one_shot_estimator(monkeypatch):
    n_t, n_w, n_d, rhos = ar.CHAINS[1]
    x = ar.ar1_chain(n_t, n_w, n_d, rhos)
    want = mcmc.integrated_time(x, tol=0)
    _, win, _ = ar.host_windows(x)
    assert list(win) == [96, 281]
    rel = lambda tau: np.max(np.abs(tau - want) / np.abs(want))      # noqa: E731
    # the usual block: both windows need the second request
    tau, asked, fb = _run_stubbed(monkeypatch, x, 256, 4096, tol=0)
    assert asked == [(0, 256), (256, 256)] and fb == 0 and rel(tau) <= 1e-12
    # the window on a block's last lag, then on the next block's first lag
    tau, asked, fb = _run_stubbed(monkeypatch, x, 97, 4096, tol=0)
    assert asked == [(0, 97), (97, 97), (194, 194)] and fb == 0 and rel(tau) <= 1e-12
    tau, asked, fb = _run_stubbed(monkeypatch, x, 96, 4096, tol=0)
    assert asked == [(0, 96), (96, 96), (192, 192)] and fb == 0 and rel(tau) <= 1e-12
    tau, asked, fb = _run_stubbed(monkeypatch, x, 282, 4096, tol=0)
    assert asked == [(0, 282)] and rel(tau) <= 1e-12
    tau, asked, fb = _run_stubbed(monkeypatch, x, 281, 4096, tol=0)
    assert asked == [(0, 281), (281, 281)] and rel(tau) <= 1e-12
    # the cap cuts the last request short and still settles when the window is inside it
    tau, asked, fb = _run_stubbed(monkeypatch, x, 256, 300, tol=0)
    assert asked == [(0, 256), (256, 44)] and fb == 0 and rel(tau) <= 1e-12
    # past the cap: the host estimator finishes the call, counted once, same values as the host call
    tau, asked, fb = _run_stubbed(monkeypatch, x, 128, 256, tol=0)
    assert asked == [(0, 128), (128, 128)] and fb == 1 and np.array_equal(tau, want)
    # the AutocorrError rule is the host's: n_t = 5000 < 100 tau, but > 50 tau
    with pytest.raises(mcmc.AutocorrError):
        mcmc.integrated_time(x, tol=100)
    with pytest.raises(mcmc.AutocorrError) as err:
        _run_stubbed(monkeypatch, x, 256, 4096, tol=100)
    assert rel(err.value.tau) <= 1e-12
    tau, _, _ = _run_stubbed(monkeypatch, x, 256, 4096, tol=100, quiet=True)
    assert rel(tau) <= 1e-12
    tau, _, _ = _run_stubbed(monkeypatch, x, 256, 4096)
    assert rel(tau) <= 1e-12


def test_block_growing_loop_short_chains(monkeypatch):
    n_t, n_w, n_d, rhos = ar.CHAINS[2]
    full = ar.ar1_chain(n_t, n_w, n_d, rhos)
    for n in (100, 1, 2, 257):
        x = full[:n]
        with np.errstate(all="ignore"):
            want = mcmc.integrated_time(x, tol=0)
            tau, asked, fb = _run_stubbed(monkeypatch, x, 256, 4096, tol=0)
        assert asked[0] == (0, min(n, 256)) and fb == 0
        assert sum(a[1] for a in asked) <= n
        assert np.allclose(tau, want, rtol=1e-12, atol=0, equal_nan=True), (n, tau, want)
    # 1-D and 2-D inputs take the same shapes as on the host
    want = mcmc.integrated_time(full[:, 0, 1], tol=0)
    tau, _, _ = _run_stubbed(monkeypatch, full[:, 0, 1], 256, 4096, tol=0)
    assert tau.shape == want.shape and np.allclose(tau, want, rtol=1e-12)
    want = mcmc.integrated_time(full[:, :, 1], tol=0)
    tau, _, _ = _run_stubbed(monkeypatch, full[:, :, 1], 256, 4096, tol=0)
    assert tau.shape == want.shape and np.allclose(tau, want, rtol=1e-12)


def test_nan_dimension_stays_nan_in_the_loop(monkeypatch):
    n_t, n_w, n_d, rhos = ar.CHAINS[2]
    x = ar.ar1_chain(n_t, n_w, n_d, rhos)
    x[:, 3, 1] = 0.5                        # one walker never moves in dimension 1: A(0) = 0 there
    with np.errstate(all="ignore"):
        want = mcmc.integrated_time(x, tol=0)
        tau, _, fb = _run_stubbed(monkeypatch, x, 256, 4096, tol=0)
    assert np.isnan(want[1]) and np.isnan(tau[1]) and fb == 0
    assert np.allclose(tau[[0, 2]], want[[0, 2]], rtol=1e-12)
