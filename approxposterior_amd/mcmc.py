# -*- coding: utf-8 -*-
"""
:py:mod:`mcmc.py` - affine-invariant ensemble sampler driving the batched GP
---------------------------------------------------------------------------

The reference samples its GP surrogate with ``emcee.EnsembleSampler``
(approx.py:839-846); emcee is a third-party dependency that is neither vendored
in the reference nor installed here, so this module restates the published
algorithm it relies on -- the Goodman & Weare (2010) stretch move as emcee >= 3
implements it (red/blue split, a = 2) -- behind the
subset of emcee's interface the reference touches:

    EnsembleSampler(nwalkers, ndim, log_prob_fn, args=, kwargs=, backend=, blobs_dtype=)
    sampler.sample(initial_state, iterations=...)   (generator, approx.py:846)
    sampler.run_mcmc(initial_state, nsteps)
    sampler.get_chain(discard=, thin=, flat=)       (approx.py:479)
    sampler.get_log_prob(...), sampler.get_blobs(...)
    sampler.get_autocorr_time(tol=0)                (mcmcUtils.py:198)
    sampler.acceptance_fraction, sampler.iteration
    EnsembleSampler(..., moves=...) with moves.StretchMove, moves.DEMove, moves.DESnookerMove and weighted mixtures

What is new relative to the reference's usage: with ``vectorize=True`` the
log-probability function receives the whole half-ensemble (S, D) in ONE call,
which ``ApproxPosterior._gpllBatch`` turns into one mean-only GP launch on the
MI355X instead of S scalar ``predict`` calls per half-step.  The chain is a
sequential process (each half-step depends on the previous one), so only that
per-half-step batch is parallel; independent ensembles shard across GPUs as
whole replicas.
"""

import numpy as np

__all__ = ["EnsembleSampler", "integrated_time", "AutocorrError", "StretchMove", "DEMove", "DESnookerMove", "moves",
           "nested_weights", "NestedResult"]


class AutocorrError(Exception):
    """Chain too short for a reliable autocorrelation time (emcee semantics)."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super(AutocorrError, self).__init__(*args, **kwargs)


def _next_pow_two(n):
    i = 1
    while i < n:
        i <<= 1
    return i


def _autocorr_1d(x):
    """Normalised autocorrelation function of a 1-D series via FFT."""
    x = np.atleast_1d(x)
    n = _next_pow_two(len(x))
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
    acf /= acf[0]
    return acf


def _auto_window(taus, c):
    m = np.arange(len(taus)) < c * taus
    if np.any(m):
        return int(np.argmin(m))
    return len(taus) - 1


# Device path of integrated_time (csrc/autocorr.hip, DESIGN.md "Chain diagnostics"): the autocorrelation function is
# asked for in blocks of lags -- AUTOCORR_BLOCK first, then as many again as are there already -- until every dimension
# has its window.
AUTOCORR_BLOCK = 256
# Lags after which the device path stops extending and the call is finished by the host FFT estimator below: the
# direct sum costs O(n_t * lags) per series, the FFT O(n_t log n_t) whatever the window.
# Measured (tools/autocorr_timing.py, profiles/autocorr_timing.json, MI355X against 16 host threads): no crossing up to
# all n_t lags at 2e4 x 64 x 8 -- lags 0..4095 take 5.3 ms, all 20000 lags 18.4 ms, the host call 168 ms -- and a near
# tie at all lags at 2e4 x 20 x 2 (10.3 ms against 10.9 ms; 2.3 ms at 4096).  The cap sits below both, so a chain that
# reaches it and is then handed to the host pays at most those 5.3 ms (3 %) on top of the host call.
AUTOCORR_LAG_CAP = 4096
autocorr_fallbacks = 0      # calls the device path handed to the host estimator because the window lay past the cap


class _DeviceAcf(object):
    """Blocks of the walker-averaged autocorrelation function of one chain, from ``apgp_autocorr_block``.
    ``x``: a (n_t, n_w, n_d) NumPy array (uploaded once) or torch tensor; a device tensor whose steps are whole
    rows of a contiguous chain (``chain[discard::thin]``) is read in place through the row stride."""

    def __init__(self, x):
        import ctypes
        import torch
        from . import _lib
        self._torch, self._lib, self._check, self._vp = torch, _lib.load(), _lib.check, ctypes.c_void_p
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.device("cuda", torch.cuda.current_device()))
        elif x.device.type != "cuda":
            x = x.to(torch.device("cuda", torch.cuda.current_device()))
        if x.dtype != torch.float64:
            x = x.to(torch.float64)
        self.n_t, self.n_w, self.n_d = (int(v) for v in x.shape)
        series = self.n_w * self.n_d
        rows = x.stride(0) if self.n_t > 1 else series
        if x.stride(2) != 1 or x.stride(1) != self.n_d or rows < series or rows % series != 0:
            x = x.contiguous()
            rows = series
        self._x, self._stride = x, rows // series
        need = int(self._lib.apgp_autocorr_work_len(self.n_t, self.n_w, self.n_d))
        if need < 0:
            raise ValueError("chain of shape %s is outside the limits of apgp_autocorr_block" % (tuple(x.shape),))
        with torch.cuda.device(x.device):
            self._work = torch.empty(need, dtype=torch.float64, device=x.device)
        self._have_stats = False

    def __call__(self, lag0, nlags):
        torch, x = self._torch, self._x
        with torch.cuda.device(x.device):
            f = torch.empty((self.n_d, nlags), dtype=torch.float64, device=x.device)
            st = self._vp(torch.cuda.current_stream().cuda_stream)
            self._check(self._lib.apgp_autocorr_block(x.data_ptr(), self.n_t, self.n_w, self.n_d, 0, self._stride,
                                                      int(lag0), int(nlags), int(self._have_stats),
                                                      self._work.data_ptr(), f.data_ptr(), st), "apgp_autocorr_block")
            self._have_stats = True
            return f.cpu().numpy()


def _windows_from_blocks(acf, n_t, n_d, c, block, cap):
    """Sokal's window and tau per dimension from an autocorrelation function served in blocks of lags:
    ``acf(lag0, nlags) -> (n_d, nlags)``.  After each block the host lines of :func:`integrated_time` run on the lags
    that are there; a dimension is done at the first lag M >= c tau(M), all are done when every one of the n_t lags is
    there.  Returns ``(tau, windows)``, or ``None`` once ``cap`` lags did not settle every dimension."""
    f = np.empty((n_d, 0))
    tau_est = np.empty(n_d)
    windows = np.empty(n_d, dtype=int)
    limit = min(n_t, max(int(cap), 1))
    while True:
        have = f.shape[1]
        more = min(max(have, int(block)), limit - have)
        f = np.concatenate([f, np.asarray(acf(have, more), dtype=float)[:, :more]], axis=1)
        have += more
        open_dims = 0
        for d in range(n_d):
            taus = 2.0 * np.cumsum(f[d]) - 1.0
            m = np.arange(have) < c * taus
            if have < n_t and m.all():
                open_dims += 1                # no lag with M >= c tau(M) yet
                continue
            windows[d] = _auto_window(taus, c)
            tau_est[d] = taus[windows[d]]
        if open_dims == 0:
            return tau_est, windows
        if have >= limit:
            return None


def integrated_time(x, c=5, tol=50, quiet=False, onDevice=False):
    """Integrated autocorrelation time per dimension of a chain ``x`` of shape
    (nsteps, nwalkers, ndim), Sokal's automated windowing with window constant
    ``c`` (the estimator behind emcee's ``get_autocorr_time``; with ``tol=0`` it
    always returns an estimate, which is how mcmcUtils.py:198 calls it).

    ``onDevice=True``, or an ``x`` that is a torch tensor on the GPU: the autocorrelation function comes from the
    device in blocks of lags, summed directly (``apgp_autocorr_block``), and only as far as the windows need it; the
    windowing lines are the ones below.  A chain whose window lies past ``AUTOCORR_LAG_CAP`` lags is handed to the host
    estimator for that call (``autocorr_fallbacks`` counts them).  Same return value either way."""
    global autocorr_fallbacks
    if onDevice or _is_device_tensor(x):
        if _is_tensor(x):
            xd = x if x.dim() == 3 else (x[:, None, None] if x.dim() == 1 else (x[:, :, None] if x.dim() == 2 else None))
        else:
            xd = np.atleast_1d(x)
            xd = xd[:, np.newaxis, np.newaxis] if xd.ndim == 1 else (xd[:, :, np.newaxis] if xd.ndim == 2 else xd)
        if xd is None or len(xd.shape) != 3:
            raise ValueError("invalid dimensions")
        n_t, n_d = int(xd.shape[0]), int(xd.shape[2])
        done = _windows_from_blocks(_device_acf(xd), n_t, n_d, c, AUTOCORR_BLOCK, AUTOCORR_LAG_CAP)
        if done is not None:
            return _checked_tau(done[0], n_t, tol, quiet)
        autocorr_fallbacks += 1
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.atleast_1d(x)
    if x.ndim == 1:
        x = x[:, np.newaxis, np.newaxis]
    if x.ndim == 2:
        x = x[:, :, np.newaxis]
    if x.ndim != 3:
        raise ValueError("invalid dimensions")
    n_t, n_w, n_d = x.shape
    tau_est = np.empty(n_d)
    windows = np.empty(n_d, dtype=int)
    # real transforms (half the work of emcee's complex ones, same values to rounding), the series spread over a few host
    # threads (pocketfft releases the GIL): 0.6 s per call at 2e4 x 64 x 8 with the per-series complex FFTs -- 6 s of
    # BASELINE config 5's ten MCMC post-processing steps
    import os
    from concurrent.futures import ThreadPoolExecutor
    n2 = 2 * _next_pow_two(n_t)

    def acf_of(series):
        spec = np.fft.rfft(series - np.mean(series), n=n2)
        acf = np.fft.irfft(spec.real ** 2 + spec.imag ** 2, n=n2)[:n_t]
        return acf / acf[0]
    cols = [np.ascontiguousarray(x[:, k, d]) for d in range(n_d) for k in range(n_w)]
    with ThreadPoolExecutor(max_workers=max(1, min(16, (os.cpu_count() or 2) // 2))) as pool:
        acfs = list(pool.map(acf_of, cols))
    for d in range(n_d):
        f = np.zeros(n_t)
        for k in range(n_w):
            f += acfs[d * n_w + k]
        f /= n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        windows[d] = _auto_window(taus, c)
        tau_est[d] = taus[windows[d]]
    return _checked_tau(tau_est, n_t, tol, quiet)


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _is_device_tensor(x):
    return _is_tensor(x) and x.device.type == "cuda"


def _device_acf(x):
    return _DeviceAcf(x)


def _checked_tau(tau_est, n_t, tol, quiet):
    """``tau_est``, or :class:`AutocorrError` when the chain is shorter than ``tol`` times it (emcee's rule)."""
    flag = tol * tau_est > n_t
    if np.any(flag) and tol > 0:
        msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} "
               "parameter(s). Use this estimate with caution and run a longer chain!\n"
               "N/{0} = {2:.0f};\ntau: {3}").format(tol, np.sum(flag), n_t / tol, tau_est)
        if not quiet:
            raise AutocorrError(tau_est, msg)
    return tau_est


class StretchMove(object):
    """The Goodman & Weare (2010) stretch move with scale ``a`` > 1: the sampler's default."""
    kind = 0          # APGP_ENS_MOVE_STRETCH
    min_walkers = 2

    def __init__(self, a=2.0):
        self.a = float(a)
        if not (np.isfinite(self.a) and self.a > 1.0):
            raise ValueError("StretchMove: a must be > 1")

    def record(self, ndim):
        """``(kind, p0, p1)`` of ``apgp_ens_move_t`` (include/apgp.h)."""
        return self.kind, self.a, 0.0

    def __repr__(self):
        return "StretchMove(a=%r)" % self.a


class DEMove(object):
    """Differential evolution (ter Braak 2006) with the jitter on gamma of Nelson et al. (2013): for walker s, an ordered
    pair of distinct walkers c_j, c_k of the other half and n ~ N(0, 1),
    ``q = s + gamma0 (1 + sigma n) (c_j - c_k)``, log proposal factor 0; ``gamma0`` defaults to 2.38 / sqrt(2 ndim).
    ``DEMove(gamma0=1.0)`` mixed in with a small weight is the usual mode-jumping idiom.  Needs 4 walkers.

    The textbook move behind emcee's interface: a valid sampler of the same family (pinned by a stationarity test), not
    draw-for-draw emcee -- emcee is neither installed here nor was its source at hand."""
    kind = 1          # APGP_ENS_MOVE_DE
    min_walkers = 4

    def __init__(self, sigma=1.0e-5, gamma0=None):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        if not (np.isfinite(self.sigma) and self.sigma >= 0.0):
            raise ValueError("DEMove: sigma must be >= 0")
        if self.gamma0 is not None and not (np.isfinite(self.gamma0) and self.gamma0 > 0.0):
            raise ValueError("DEMove: gamma0 must be > 0 or None")

    def g0(self, ndim):
        return 2.38 / np.sqrt(2.0 * ndim) if self.gamma0 is None else self.gamma0

    def record(self, ndim):
        return self.kind, self.sigma, float(self.g0(ndim))

    def __repr__(self):
        return "DEMove(sigma=%r, gamma0=%r)" % (self.sigma, self.gamma0)


class DESnookerMove(object):
    """The snooker update (ter Braak & Vrugt 2008): for walker s and three distinct walkers z = c_j, z1 = c_k, z2 = c_l of
    the other half, ``e = (s - z) / |s - z|``, ``q = s + gammas (e . (z1 - z2)) e``, log proposal factor
    ``(ndim - 1) (log|q - z| - log|s - z|)``.  ``s == z`` gives a NaN proposal, which is rejected like one outside the
    prior.  Needs 6 walkers.  The host sampler takes the norms in plain coordinates, the device sampler in the GP's
    scaled coordinates (DESIGN.md "Ensemble moves").

    The textbook move behind emcee's interface: a valid sampler of the same family (pinned by a stationarity test), not
    draw-for-draw emcee -- emcee is neither installed here nor was its source at hand."""
    kind = 2          # APGP_ENS_MOVE_SNOOKER
    min_walkers = 6

    def __init__(self, gammas=1.7):
        self.gammas = float(gammas)
        if not (np.isfinite(self.gammas) and self.gammas > 0.0):
            raise ValueError("DESnookerMove: gammas must be > 0")

    def record(self, ndim):
        return self.kind, self.gammas, 0.0

    def __repr__(self):
        return "DESnookerMove(gammas=%r)" % self.gammas


class _Moves(object):
    """``mcmc.moves``: the namespace emcee calls ``emcee.moves``."""
    StretchMove, DEMove, DESnookerMove = StretchMove, DEMove, DESnookerMove


moves = _Moves()
MAX_MOVES = 8         # APGP_ENS_MAX_MOVES


def move_table(moves, nwalkers, a=2.0):
    """``[(move, weight), ...]`` with the weights normalised, from what ``EnsembleSampler(moves=...)`` accepts: ``None``
    (the stretch move at ``a``), one move, a list of moves (equal weights) or a list of ``(move, weight)`` pairs, at most
    ``MAX_MOVES`` entries.  ``ValueError`` for ``a`` other than 2.0 beside ``moves`` (``a`` belongs to the default move
    alone), a weight that is not positive and finite, or fewer walkers than a listed move needs."""
    if moves is None:
        return [(StretchMove(a), 1.0)]
    if float(a) != 2.0:
        raise ValueError("a belongs to the default stretch move: with moves, pass StretchMove(a) in the list")
    known = (StretchMove, DEMove, DESnookerMove)
    if isinstance(moves, known):
        moves = [moves]
    try:
        entries = list(moves)
    except TypeError:
        raise ValueError("moves must be a move, a list of moves or a list of (move, weight) pairs")
    if not 1 <= len(entries) <= MAX_MOVES:
        raise ValueError("moves must list between 1 and %d moves" % MAX_MOVES)
    pairs = []
    for e in entries:
        mv, w = (e, 1.0) if isinstance(e, known) else (tuple(e) if np.ndim(e) == 1 and len(e) == 2 else (None, 0.0))
        if not isinstance(mv, known):
            raise ValueError("moves: %r is not a StretchMove, DEMove or DESnookerMove (or a (move, weight) pair)" % (e,))
        w = float(w)
        if not (np.isfinite(w) and w > 0.0):
            raise ValueError("moves: weights must be positive and finite")
        if nwalkers < mv.min_walkers:
            raise ValueError("%r needs at least %d walkers" % (mv, mv.min_walkers))
        pairs.append((mv, w))
    total = 0.0
    for _, w in pairs:
        total = total + w
    return [(mv, w / total) for mv, w in pairs]


class EnsembleSampler(object):
    """Red/blue ensemble sampler (emcee-3 semantics): the Goodman-Weare stretch move by default, or ``moves`` -- a
    :class:`StretchMove`, :class:`DEMove` or :class:`DESnookerMove`, a list of them, or a list of ``(move, weight)``
    pairs; one move is drawn per iteration for the whole ensemble.  ``sampler.moves`` is the normalised table."""

    def __init__(self, nwalkers, ndim, log_prob_fn, args=None, kwargs=None, backend=None,
                 blobs_dtype=None, vectorize=False, a=2.0, seed=None, moves=None, pool=None):
        if nwalkers < 2 * ndim or nwalkers % 2 != 0:
            # emcee's own constraints for the red/blue move
            if nwalkers % 2 != 0:
                raise ValueError("The number of walkers must be even.")
            raise ValueError("The number of walkers needs to be at least twice the dimension.")
        if pool is not None:
            raise NotImplementedError("no pool: the log-probability is evaluated in this process")
        self._default_move = moves is None
        self.moves = move_table(moves, int(nwalkers), a)
        self.nwalkers = int(nwalkers)
        self.ndim = int(ndim)
        self.log_prob_fn = log_prob_fn
        self.args = () if args is None else tuple(args)
        self.kwargs = {} if kwargs is None else dict(kwargs)
        self.vectorize = bool(vectorize)
        self.a = float(a)
        self.blobs_dtype = blobs_dtype
        self.backend = backend
        # own RandomState, like emcee: independent of numpy's global stream unless seeded
        self._random = np.random.RandomState(seed)
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        self.iteration = 0
        self._chain = []
        self._log_prob = []
        self._blobs = []
        self._naccepted = np.zeros(self.nwalkers)
        self._coords = None
        self._lp = None
        self._bl = None

    @property
    def acceptance_fraction(self):
        return self._naccepted / max(self.iteration, 1)

    # -------------------------------------------------------------- log-prob
    def compute_log_prob(self, coords):
        """log-probability (and first blob, if any) for every row of ``coords``."""
        coords = np.atleast_2d(coords)
        if not np.isfinite(coords).all():                 # (one pass in the usual case; the two messages as before)
            if np.isinf(coords).any():
                raise ValueError("At least one parameter value was infinite")
            raise ValueError("At least one parameter value was NaN")
        if self.vectorize:
            res = self.log_prob_fn(coords, *self.args, **self.kwargs)
            if isinstance(res, tuple):
                lp = np.asarray(res[0], dtype=float).reshape(len(coords))
                blob = np.asarray(res[1], dtype=float).reshape(len(coords)) if len(res) > 1 else None
            else:
                lp = np.asarray(res, dtype=float).reshape(len(coords))
                blob = None
        else:
            lp = np.empty(len(coords))
            blob = None
            for i, c in enumerate(coords):
                r = self.log_prob_fn(c, *self.args, **self.kwargs)
                if isinstance(r, (tuple, list)):
                    lp[i] = float(np.ravel(r[0])[0])
                    if len(r) > 1:
                        if blob is None:
                            blob = np.full(len(coords), np.nan)
                        blob[i] = float(np.ravel(r[1])[0])
                else:
                    lp[i] = float(np.ravel(r)[0])
        if np.isnan(lp).any():
            raise ValueError("Probability function returned NaN")
        return lp, blob

    # ---------------------------------------------------------------- sample
    def sample(self, initial_state, iterations=1, store=True, progress=False, **unused):
        """Advance the ensemble ``iterations`` steps; yields (coords, log_prob,
        blobs) after each step (the reference just drains it, approx.py:846)."""
        p = np.array(initial_state, dtype=float, copy=True)
        if p.ndim == 1:
            p = p.reshape(self.nwalkers, self.ndim)
        if p.shape != (self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions")
        if self._coords is None or initial_state is not None:
            self._coords = p
            self._lp, self._bl = self.compute_log_prob(p)
            if np.any(np.isneginf(self._lp)) and np.all(np.isneginf(self._lp)):
                raise ValueError("Initial state has a zero probability for every walker")
        nw, nd, a = self.nwalkers, self.ndim, self.a
        weights = np.cumsum([w for _, w in self.moves])
        for _ in range(int(iterations)):
            inds = np.arange(nw) % 2
            self._random.shuffle(inds)
            halves = (np.flatnonzero(inds == 0), np.flatnonzero(inds == 1))
            # the iteration's move (a table of one draws nothing: the default's stream is the stretch sampler's)
            move = self.moves[0][0] if len(self.moves) == 1 else \
                self.moves[min(int(np.searchsorted(weights, self._random.rand(), side="right")), len(self.moves) - 1)][0]
            for split in range(2):
                S, C = halves[split], halves[1 - split]
                s, c = self._coords[S], self._coords[C]
                if self._default_move:
                    zz = ((a - 1.0) * self._random.rand(len(S)) + 1.0) ** 2.0 / a
                    factors = (nd - 1.0) * np.log(zz)
                    rint = self._random.randint(len(C), size=(len(S),))
                    q = c[rint] - (c[rint] - s) * zz[:, None]
                    valid = None
                else:
                    q, factors = self._propose(move, s, c)
                    valid = np.all(np.isfinite(q), axis=1)        # (a snooker walker on its own pivot: q is NaN)
                    if not valid.all():
                        q[~valid] = s[~valid]                       # evaluated in place of the proposal, then rejected
                new_lp, new_bl = self.compute_log_prob(q)
                with np.errstate(invalid="ignore"):      # -inf - -inf for walkers outside the prior
                    lnpdiff = factors + new_lp - self._lp[S]
                accepted = np.log(self._random.rand(len(S))) < lnpdiff
                if valid is not None:
                    accepted &= valid
                idx = S[accepted]
                self._coords[idx] = q[accepted]
                self._lp[idx] = new_lp[accepted]
                if new_bl is not None:
                    if self._bl is None:
                        self._bl = np.full(nw, np.nan)
                    self._bl[idx] = new_bl[accepted]
                self._naccepted[idx] += 1
            self.iteration += 1
            if store:
                self._chain.append(self._coords.copy())
                self._log_prob.append(self._lp.copy())
                if self._bl is not None:
                    self._blobs.append(self._bl.copy())
            yield self._coords, self._lp, self._bl

    def _propose(self, move, s, c):
        """Proposals and log proposal factors of ``move`` for the active half ``s`` (S, D) against the complement ``c``."""
        ns, nc, nd = len(s), len(c), self.ndim
        rs = self._random
        if isinstance(move, StretchMove):
            zz = ((move.a - 1.0) * rs.rand(ns) + 1.0) ** 2.0 / move.a
            rint = rs.randint(nc, size=(ns,))
            return c[rint] - (c[rint] - s) * zz[:, None], (nd - 1.0) * np.log(zz)
        j = rs.randint(nc, size=(ns,))
        k = rs.randint(nc - 1, size=(ns,))
        k += k >= j                                              # ordered pair, j != k
        if isinstance(move, DEMove):
            gamma = move.g0(nd) * (1.0 + move.sigma * rs.randn(ns))
            return s + gamma[:, None] * (c[j] - c[k]), np.zeros(ns)
        l = rs.randint(nc - 2, size=(ns,))
        l += l >= np.minimum(j, k)
        l += l >= np.maximum(j, k)                               # ordered triple, all distinct
        z, z1, z2 = c[j], c[k], c[l]
        with np.errstate(invalid="ignore", divide="ignore"):
            delta = s - z
            norm = np.sqrt(np.sum(delta * delta, axis=1))
            e = delta / norm[:, None]
            q = s + move.gammas * np.sum(e * (z1 - z2), axis=1)[:, None] * e
            qn = np.sqrt(np.sum((q - z) ** 2, axis=1))
            factors = (nd - 1.0) * (np.log(qn) - np.log(norm))
        return q, np.where(np.isfinite(factors), factors, -np.inf)

    def run_mcmc(self, initial_state, nsteps, **kwargs):
        out = None
        for out in self.sample(initial_state, iterations=nsteps, **kwargs):
            pass
        return out

    # ---------------------------------------------------------------- access
    def _get(self, store, discard, thin, flat):
        if len(store) == 0:
            raise AttributeError("you must run the sampler before accessing the results")
        v = np.asarray(store)[discard + thin - 1::thin]
        if flat:
            v = v.reshape((-1,) + v.shape[2:])
        return v

    def get_chain(self, discard=0, thin=1, flat=False):
        return self._get(self._chain, int(discard), int(thin), flat)

    def get_log_prob(self, discard=0, thin=1, flat=False):
        return self._get(self._log_prob, int(discard), int(thin), flat)

    def get_blobs(self, discard=0, thin=1, flat=False):
        if len(self._blobs) == 0:
            return None
        return self._get(self._blobs, int(discard), int(thin), flat)

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        return thin * integrated_time(self.get_chain(discard=discard, thin=thin), **kwargs)


class DeviceChain(EnsembleSampler):
    """Result of an on-device run (``GP.sample_ensemble``) behind the same accessors
    as :class:`EnsembleSampler` (``get_chain``, ``get_log_prob``,
    ``get_autocorr_time``, ``acceptance_fraction``), so burn-in estimation and the
    reference-style post-processing work unchanged."""

    def __init__(self, result, a=2.0, moves=None):
        chain = result["chain"]
        self.nwalkers = chain.shape[1]
        self.ndim = chain.shape[2]
        self.log_prob_fn = None
        self.args, self.kwargs = (), {}
        self.vectorize = True
        self.a = float(a)                 # the stretch scale the chain was run with
        self._default_move = moves is None
        self.moves = move_table(moves, self.nwalkers, a)      # ... and the move table
        self.blobs_dtype = None
        self.backend = None
        self._random = None
        self.iteration = chain.shape[0]
        self._chain = chain
        self._chain_device = result.get("chain_device")   # the same chain as a device tensor (sample_ensemble(keep_device=True))
        self._log_prob = result["log_prob"]
        blobs = result.get("blobs")
        self._blobs = [] if blobs is None else blobs      # (iterations, walkers) lnprior values of a gathered host chain
        self._naccepted = np.asarray(result["naccept"], dtype=float)
        self._coords = result["coords"]
        self._lp = result["final_log_prob"]
        self._bl = None

    def sample(self, *args, **kwargs):
        raise NotImplementedError("a finished on-device chain cannot be advanced from the host")

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """As :meth:`EnsembleSampler.get_autocorr_time`; a chain that is still on the device is diagnosed there
        (``integrated_time(onDevice=True)`` on the strided view, no copy)."""
        if self._chain_device is None:
            return super(DeviceChain, self).get_autocorr_time(discard=discard, thin=thin, **kwargs)
        discard, thin = int(discard), int(thin)
        kwargs["onDevice"] = True
        return thin * integrated_time(self._chain_device[discard + thin - 1::thin], **kwargs)


PT_MAX_TEMPS = 64     # APGP_PT_MAX_TEMPS


def tempering_ladder(ntemps, betaMin=1.0e-3, zero=True):
    """Inverse temperatures of a tempering ladder of ``ntemps`` rungs: beta_0 = 1, then geometrically down to
    ``betaMin`` (0 < betaMin < 1) and, with ``zero``, a final rung beta = 0 -- the rung that samples the prior's box
    uniformly, which :meth:`TemperedChain.log_evidence` needs.  ``ntemps`` counts the zero rung.  One rung is [1]; with
    ``zero``, two rungs are [1, 0]."""
    ntemps = int(ntemps)
    if not 1 <= ntemps <= PT_MAX_TEMPS:
        raise ValueError("ntemps must lie between 1 and %d" % PT_MAX_TEMPS)
    if not 0.0 < float(betaMin) < 1.0:
        raise ValueError("betaMin must lie strictly between 0 and 1")
    geo = ntemps - 1 if (zero and ntemps > 1) else ntemps      # rungs of the geometric part
    betas = np.ones(geo) if geo == 1 else float(betaMin) ** (np.arange(geo) / (geo - 1.0))
    betas[0] = 1.0
    if geo > 1:
        betas[-1] = float(betaMin)
    return np.append(betas, 0.0) if geo < ntemps else betas


def _trapezoid_weights(betas):
    """w with sum_k w_k f(beta_k) = the trapezoid rule of f over [beta_last, beta_0] for non-increasing ``betas``."""
    b = np.asarray(betas, dtype=np.float64)
    w = np.zeros(len(b))
    if len(b) > 1:
        gaps = b[:-1] - b[1:]
        w[:-1] += 0.5 * gaps
        w[1:] += 0.5 * gaps
    return w


class TemperedChain(DeviceChain):
    """Result of a parallel-tempering run (``GP.sample_tempered``): the cold rungs (beta = 1, the posterior) of all
    ladders behind the accessors of :class:`DeviceChain`, the ladder's own diagnostics, and the evidence by
    thermodynamic integration."""

    def __init__(self, result, a=2.0, moves=None):
        super(TemperedChain, self).__init__(result, a=a, moves=moves)
        self.betas = np.asarray(result["betas"], dtype=np.float64)
        self.swap_every = result.get("swap_every")
        self._rung_naccept = np.asarray(result["rung_naccept"], dtype=float)                 # (L, T, W)
        self._swap_proposed = np.asarray(result["swap_proposed"], dtype=float)               # (L, T - 1)
        self._swap_accepted = np.asarray(result["swap_accepted"], dtype=float)
        self._rung_mean = np.asarray(result["rung_mean_log_prob"], dtype=np.float64)         # (iterations, L, T)
        self._log_volume = result.get("log_volume")
        self.nladders = self._rung_mean.shape[1]
        self.ntemps = len(self.betas)

    @property
    def swap_acceptance_fraction(self):
        """Accepted / proposed exchanges per neighbouring pair, summed over the ladders (T - 1,); NaN where none was proposed."""
        prop, acc = self._swap_proposed.sum(axis=0), self._swap_accepted.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(prop > 0, acc / prop, np.nan)

    @property
    def rung_acceptance_fraction(self):
        """Acceptance fraction of the moves per rung, averaged over ladders and walkers (T,)."""
        return self._rung_naccept.mean(axis=(0, 2)) / max(self.iteration, 1)

    def rung_means(self, discard=0):
        """Mean of mu per ladder and rung over the iterations after ``discard`` (L, T)."""
        rows = self._rung_mean[int(discard):]
        if len(rows) == 0:
            raise ValueError("discard leaves no iterations")
        return rows.mean(axis=0)

    def log_evidence(self, discard=0, logVolume=None):
        """``(logZ, discErr, mcErr)`` by thermodynamic integration: ``logZ = log V + int_0^1 E_beta[mu] d beta``, V the
        volume of the box (``logVolume``; default: the box the chain ran in), the integral by the trapezoid rule over
        the rungs' means of mu after ``discard`` iterations.  ``discErr`` is the distance to the same rule over every
        other rung (the end rungs kept): the size of the discretisation error, not a bound.  ``mcErr`` is the standard
        error between the ladders' own estimates when there are several ladders, else the rungs' batch-means standard
        errors (``mcmcUtils.batchMeansMCSE``) combined with the trapezoid weights.  ``ValueError`` unless the ladder
        ends at beta = 0."""
        if self.betas[-1] != 0.0 or self.betas[0] != 1.0:
            raise ValueError("log_evidence integrates over beta from 0 to 1: the ladder must start at 1 and end at 0")
        if logVolume is None:
            logVolume = self._log_volume
        if logVolume is None:
            raise ValueError("log_evidence needs logVolume, the log-volume of the prior's box")
        per = self.rung_means(discard)                                   # (L, T)
        w = _trapezoid_weights(self.betas)
        mean = per.mean(axis=0)
        integral = float(np.dot(w, mean))
        keep = sorted(set(range(0, self.ntemps, 2)) | {self.ntemps - 1})
        coarse = float(np.dot(_trapezoid_weights(self.betas[keep]), mean[keep]))
        if self.nladders > 1:
            mc = float(np.std(per @ w, ddof=1) / np.sqrt(self.nladders))
        else:
            from .mcmcUtils import batchMeansMCSE
            se = np.asarray(batchMeansMCSE(self._rung_mean[int(discard):, 0, :]), dtype=np.float64)
            mc = float(np.sqrt(np.sum((w * se) ** 2)))
        return float(logVolume) + integral, abs(integral - coarse), mc


class HMCChain(DeviceChain):
    """Result of a Hamiltonian Monte Carlo run on the device (``GP.sample_hmc``): the chains behind the accessors of
    :class:`DeviceChain` (a chain stands where a walker does, so ``estimateBurnin``, ``get_autocorr_time``, caching and
    ``evidence(proposal="gmm")`` work unchanged), and the sampler's own diagnostics."""

    def __init__(self, result, warmup=None):
        super(HMCChain, self).__init__(result)
        self.moves = None                  # no ensemble move made this chain
        self.accept_prob = np.asarray(result["accept_prob"], dtype=np.float64)   # (C,) mean of min(1, exp(-dH))
        self.ndiverge = np.asarray(result["ndiverge"], dtype=np.int64)           # (C,) divergent trajectories
        self.step_size = float(result["eps"])                                    # eps of the sampling run
        self.mass = result.get("mass")                                           # the diagonal mass (user's coordinates) or None
        self.warmup = [] if warmup is None else list(warmup)                     # eps of every warm-up segment, in order


def hmc_warmup(gp, y, initial_state, bounds, eps, nLeap, nWarmup=200, adaptEvery=20, targetAccept=0.8, kappa=1.0,
               jitter=0.1, mass=None, adaptMass=False, seed=0, iteration0=0, prior=None, gRows=0):
    """Warm up :meth:`GP.sample_hmc`: ``nWarmup`` iterations in segments of ``adaptEvery`` with consecutive
    ``iteration0``, each started where the previous one ended.  After a segment ``eps <- eps * exp(kappa * (a -
    targetAccept))``, ``a`` the segment's mean of ``accept_prob`` over the chains: C numbers cross per segment, no chain.
    ``adaptMass``: at the end the diagonal mass becomes the inverse of the per-dimension variance pooled over the chains
    and the second half of the warm-up segments (their pooled first and second moments; in the user's coordinates).
    Returns ``(coords, eps, mass, history, iteration)``: the chains' final state, the adapted step, the mass (None: the
    default), the step of every segment in order, and the global iteration number the sampling run starts at."""
    nWarmup, adaptEvery = int(nWarmup), int(adaptEvery)
    if nWarmup < 0 or adaptEvery < 1:
        raise ValueError("nWarmup must be >= 0 and adaptEvery >= 1")
    if not 0.0 < float(targetAccept) < 1.0:
        raise ValueError("targetAccept must lie strictly between 0 and 1")
    coords = np.asarray(initial_state, dtype=np.float64)
    eps, it, history = float(eps), int(iteration0), []
    nseg = -(-nWarmup // adaptEvery) if nWarmup else 0
    cnt, s1, s2 = 0, 0.0, 0.0
    for k in range(nseg):
        m = min(adaptEvery, nWarmup - k * adaptEvery)
        pool = adaptMass and k >= nseg // 2
        res = gp.sample_hmc(y, coords, m, bounds, eps, nLeap, jitter=jitter, mass=mass, seed=seed, iteration0=it,
                            prior=prior, store=pool, gRows=gRows)
        history.append(eps)
        coords, it = res["coords"], it + m
        if pool:
            x = res["chain"].reshape(-1, coords.shape[1])
            cnt, s1, s2 = cnt + len(x), s1 + x.sum(axis=0), s2 + (x * x).sum(axis=0)
        eps = eps * float(np.exp(kappa * (float(np.mean(res["accept_prob"])) - float(targetAccept))))
    if adaptMass and cnt > 1:
        var = (s2 - s1 * s1 / cnt) / (cnt - 1)
        if np.all(np.isfinite(var)) and np.all(var > 0.0):
            mass = 1.0 / var
    return coords, eps, mass, history, it


def _logsumexp(v):
    v = np.asarray(v, dtype=np.float64)
    m = np.max(v) if len(v) else -np.inf
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(v - m))))


def nested_weights(logL, logLBirth, run=None):
    """The accounting of nested sampling for ANY set of points, each with its log-likelihood ``logL`` and the threshold
    it was born under ``logLBirth`` (-inf for a point drawn from the whole prior): one rule for the batched removal of a
    run (live counts n, n - 1, ... inside a batch), its final flush (n, n - 1, ..., 1) and the merge of several runs
    (the counts add), which is then nothing more than concatenation -- the live-count rule dynesty uses for merged and
    dynamic runs.

    The points are ordered stably by ``(logL, run, serial)``, serial the input position.  Point j is live at point k iff
    ``logLBirth[j] < logL[k]`` and j is not before k in the order; ``n_k`` counts them (k included).  Then
    ``logX_k = -sum_{i <= k} 1 / n_i`` (``E[log t] = -1 / n``) and the rectangle weights are
    ``logWt_k = logL_k + logX_{k-1} + log(1 - exp(-1 / n_k))``, with ``logX_{-1} = 0``: the prior measure is normalised,
    a box's log-volume is the caller's to add.

    Returns a dict, every array in the INPUT order: ``order`` (the sorting permutation), ``nlive``, ``logX``, ``logWt``,
    and the scalars ``logZ``; ``H``, the information; ``logZErr = sqrt(sum_k dH_k / n_k)``, which is ``sqrt(H / n)``
    for a constant live count; ``ess``, Kish's effective sample size of the posterior weights."""
    logL = np.asarray(logL, dtype=np.float64).ravel()
    birth = np.asarray(logLBirth, dtype=np.float64).ravel()
    M = len(logL)
    if len(birth) != M or M < 1:
        raise ValueError("nested_weights: logL and logLBirth must be non-empty and of one length")
    if np.any(np.isnan(logL)) or np.any(np.isnan(birth)):
        raise ValueError("nested_weights: NaN in logL or logLBirth")
    run = np.zeros(M, dtype=np.int64) if run is None else np.asarray(run, dtype=np.int64).ravel()
    if len(run) != M:
        raise ValueError("nested_weights: run must have one entry per point")
    order = np.lexsort((np.arange(M), run, logL))
    ls = logL[order]
    # every point before k in the order was born below its own logL <= logL_k: it counts among the births below logL_k
    n = np.searchsorted(np.sort(birth), ls, side="left") - np.arange(M)
    n = np.maximum(n, 1).astype(np.float64)
    inv = 1.0 / n
    lx = -np.cumsum(inv)
    lw = ls + np.concatenate([[0.0], lx[:-1]]) + np.log(-np.expm1(-inv))
    logZ = _logsumexp(lw)
    if np.isfinite(logZ):
        w = np.exp(lw - logZ)
        cz = np.cumsum(w)
        cl = np.cumsum(np.where(w > 0.0, w * np.where(w > 0.0, ls, 0.0), 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            Hk = np.where(cz > 0.0, cl / cz - (logZ + np.log(cz)), 0.0)
        H = float(Hk[-1])
        var = float(np.sum(np.diff(np.concatenate([[0.0], Hk])) * inv))
        ess = float(np.sum(w) ** 2 / np.sum(w * w))
    else:
        H, var, ess = np.nan, np.nan, 0.0
    out = {"order": order, "logZ": logZ, "H": H, "logZErr": float(np.sqrt(max(var, 0.0))) if var == var else np.nan,
           "ess": ess}
    for key, v in (("nlive", n), ("logX", lx), ("logWt", lw)):
        a = np.empty(M)
        a[order] = v
        out[key] = a
    return out


class NestedResult(object):
    """Result of nested-sampling runs over the surrogate (``GP.sample_nested``): every point the runs wrote -- the dead
    points and the final live points of all runs, concatenated -- with the evidence, its error, the information and the
    weighted posterior.  ``logWt`` and ``logZ`` include ``logVolume``, the log-volume of the prior's box, as
    ``evidence(proposal="box")`` reports it.

    ``points`` (M, D), ``logL``, ``logLBirth``, ``run`` (M,), ``logX``, ``logWt``, ``logZ``, ``logZErr``, ``H``, ``ess``,
    ``mean`` (D,), ``cov`` (D, D), ``logZRuns`` (nruns,: every run's own evidence, whose scatter is a second error
    estimate: ``logZRunsErr`` is its standard error of the mean in log space, NaN for one run), ``nbatch``, ``ncall``,
    ``naccept``, ``nstuck`` (per run), ``efficiency`` (accepted steps per likelihood call of the walkers)."""

    def __init__(self, points, logL, logLBirth, run, logVolume=0.0, counts=None, nlive=None, info=None):
        self.points = np.asarray(points, dtype=np.float64)
        self.logL = np.asarray(logL, dtype=np.float64)
        self.logLBirth = np.asarray(logLBirth, dtype=np.float64)
        self.run = np.asarray(run, dtype=np.int64)
        self.logVolume = float(logVolume)
        w = nested_weights(self.logL, self.logLBirth, self.run)
        self.logX, self.nliveAt, self.H, self.logZErr, self.ess = w["logX"], w["nlive"], w["H"], w["logZErr"], w["ess"]
        self.logWt = w["logWt"] + self.logVolume
        self.logZ = w["logZ"] + self.logVolume
        p = self.weights()
        self.mean = p @ self.points
        r = self.points - self.mean
        self.cov = (r * p[:, None]).T @ r
        runs = np.unique(self.run)
        self.nruns = len(runs)
        by = np.argsort(self.run, kind="stable")                    # (the runs' rows, each in its input order)
        cut = np.searchsorted(self.run[by], runs)
        self.logZRuns = np.array([nested_weights(self.logL[rows], self.logLBirth[rows])["logZ"]
                                  for rows in np.split(by, cut[1:])]) + self.logVolume
        self.logZRunsErr = float(np.std(self.logZRuns, ddof=1) / np.sqrt(self.nruns)) if self.nruns > 1 else np.nan
        counts = np.zeros((self.nruns, 4), dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
        self.nbatch, self.ncall, self.naccept, self.nstuck = counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3]
        self.nlive = nlive
        walk = float(np.sum(self.ncall)) - (0 if nlive is None else float(nlive) * self.nruns)
        self.efficiency = float(np.sum(self.naccept)) / walk if walk > 0 else np.nan
        self.info = {} if info is None else dict(info)

    def weights(self):
        """The normalised posterior weights ``exp(logWt - logZ)`` (M,)."""
        return np.exp(self.logWt - self.logZ)

    def samples_equal(self, size=None, seed=None):
        """``size`` equally weighted posterior samples (default: ``ess`` rounded down, at least 1) by systematic
        resampling: one uniform ``u`` (from ``seed``; None: NumPy's global stream) places the comb ``(u + i) / size``
        on the cumulative weights."""
        size = max(1, int(self.ess)) if size is None else int(size)
        if size < 1:
            raise ValueError("samples_equal: size must be positive")
        rs = np.random if seed is None else np.random.RandomState(int(seed) & 0xFFFFFFFF)
        c = np.cumsum(self.weights())
        c = c / c[-1]
        pos = (rs.uniform() + np.arange(size)) / size
        return self.points[np.minimum(np.searchsorted(c, pos, side="left"), len(c) - 1)]
