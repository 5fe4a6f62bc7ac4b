# -*- coding: utf-8 -*-
"""
:py:mod:`approx.py` - ApproxPosterior: the callers of the GP-surrogate hot path
-------------------------------------------------------------------------------

The class the reference's users hold (``approxposterior/approx.py``): same public
method names, argument names, defaults, return shapes, random-number draw order
and cache files --

    ApproxPosterior(theta, y, lnprior, lnlike, priorSample, bounds, gp, algorithm)  :77-145
    _gpll(theta)                          surrogate log-probability        :148-189
    optGP(...)                            hyper-parameter re-fit           :192-226
    run(m, nmax, ...)                     BAPE / AGP outer loop            :229-524
    findNextPoint(...)                    design-point selection           :527-754
    runMCMC(...)                          surrogate MCMC                   :757-859
    findMAP(...)                          MAP of the GP mean               :862-926
    bayesOpt(nmax, ...)                   Bayesian optimisation            :929-1151

-- organised around the device path instead of the reference's inline loops: a
design point is found by :meth:`_selectPoint` (restarted Nelder-Mead as in the
reference, or the fused HIP sweep over ``nCandidates`` prior draws), absorbed by
:meth:`_absorbPoint` (training set + O(N^2) extension of the device-resident
Cholesky factor) and the stopping rules live in two small monitor classes.  The
supported way to run the reference's *own* loop on the MI355X is INTEGRATION.md
level 1 (hand the reference's ``ApproxPosterior`` a ``gp=`` from this package);
this class is for scripts that import ``approxposterior_amd`` directly.

Additions the reference does not have (all off by default):

* ``nCandidates=M`` (``findNextPoint`` / ``run`` / ``bayesOpt``): point search by the
  fused sweep over ``M`` ``priorSample`` draws, optionally ``polish``-ed by one
  Nelder-Mead run from the winner;
* ``_gpllBatch``: the surrogate log-probability of a whole walker ensemble in one
  launch (what the ensemble sampler calls with ``vectorize=True``);
* ``runMCMC(onDevice=True)`` / ``run(onDevice=True)``: the whole chain as one
  persistent kernel (a box prior, or a :class:`~approxposterior_amd.priors.JointPrior`
  of Uniform and Gaussian factors as ``lnprior``: then the chain runs under its
  support and the lnprior blobs come from the device);
* several GPUs: launched as ``python -m torch.distributed.run --nproc-per-node N script.py`` with a
  process group initialised before the object is used (``tools/run_c5_dist.py``), every rank runs the
  same outer loop on an identical training set -- the ``nCandidates`` sweep is sharded by rank with one
  16-byte-per-rank all-gather (:func:`dist.sharded_acquire`), each rank samples its own replica
  ensemble and the chains are gathered once (:func:`dist.replicated_ensembles`), optimiser restarts are
  spread over the ranks (:func:`dist.spread_restarts`), the forward model runs on rank 0 only and its
  value is broadcast, and only rank 0 prints and writes the caches (BASELINE config 5 "on 8 GPUs").

The emcee HDF5 backend is replaced by a ``<runName>.npz`` chain dump (h5py and emcee
are not installable here; :py:mod:`approxposterior_amd.mcmc` restates the sampler).
"""

import time

import numpy as np

from . import _lib
from . import dist as apdist
from . import gp as george
from . import gmmUtils
from . import gpUtils
from . import mcmc as emcee   # drop-in for the ``emcee`` names used below
from . import mcmcUtils
from . import priors as appriors
from . import utility as ut

__all__ = ["ApproxPosterior"]

_UTILITIES = {"bape": ut.BAPEUtility, "agp": ut.AGPUtility,
              "alternate": ut.AGPUtility, "jones": ut.JonesUtility}


def _cacheName(runName, suffix):
    return "%s%s.npz" % (runName, suffix)


class _ForwardModel(object):
    """``lnlike(point, *args, **kwargs)`` (its first element when it returns several) plus ``lnprior(point)``: the
    value findNextPoint absorbs, as a picklable callable for the ``pool.map`` of a batch."""

    def __init__(self, lnlike, lnprior, args, kwargs):
        self.lnlike, self.lnprior, self.args, self.kwargs = lnlike, lnprior, args, kwargs

    def __call__(self, point):
        like = self.lnlike(point, *self.args, **self.kwargs)
        like = like[0] if hasattr(like, "__iter__") else like      # (lnlike, blobs...) allowed
        return np.array([like + self.lnprior(point)], dtype=np.float64).reshape(1)


class _MarginalMonitor(object):
    """Stop rule of ``run`` (approx.py:476-523): the marginal posterior means of
    successive iterations, in units of the previous iteration's marginal standard
    deviations, must stay below ``eps`` for ``kmax`` consecutive iterations."""

    def __init__(self, eps, kmax):
        self.eps, self.kmax = eps, kmax
        self.means, self.stds, self.zscores = [], [], []
        self.streak = 0

    def update(self, samples):
        mean, std = np.mean(samples, axis=0), np.std(samples, axis=0)
        if self.means:
            z = np.fabs((mean - self.means[-1]) / self.stds[-1])
            self.zscores.append(z)
            self.streak = self.streak + 1 if np.all(z < self.eps) else 0
        self.means.append(mean)
        self.stds.append(std)
        return self.streak >= self.kmax

    def save(self, path):
        np.savez(path, means=self.means, stds=self.stds, zscores=self.zscores,
                 eps=self.eps, kmax=self.kmax, finalIteration=self.streak)


class _PlateauMonitor(object):
    """Stop rule of ``bayesOpt`` (approx.py:1118-1128): ``kmax`` consecutive
    iterations whose best value moved by less than ``tol``."""

    def __init__(self, tol, kmax):
        self.tol, self.kmax = tol, kmax
        self.last = None
        self.streak = 0

    def update(self, value):
        if self.last is not None:
            self.streak = self.streak + 1 if np.fabs(value - self.last) < self.tol else 0
        self.last = value
        return self.streak >= self.kmax


class ApproxPosterior(object):
    """Approximate-posterior driver around a GP surrogate (approx.py:29-145).

    ``theta`` (N, D) / ``y`` (N,) is the initial training set, ``lnprior``,
    ``lnlike`` and ``priorSample`` the user's callables, ``bounds`` one (lo, hi)
    pair per dimension, ``gp`` an optional pre-built GP and ``algorithm`` one of
    "bape", "agp", "alternate", "jones".  ``distributed`` (None: whenever a
    ``torch.distributed`` process group is initialised; False: never) and ``group``
    select the multi-GPU paths; the training set handed to every rank must be the same.
    """

    def __init__(self, theta, y, lnprior, lnlike, priorSample, bounds, gp=None,
                 algorithm="bape", distributed=None, group=None):
        self.distributed, self.group = distributed, group
        self.deviceCandidates = False      # nCandidates drawn on the device (see findNextPoint)
        self.deviceSearch = False          # the Nelder-Mead point search runs on the device (see findNextPoint)
        if theta is None or y is None:
            raise ValueError("Must supply both theta and y for initial GP training set.")
        self.theta = np.array(theta).squeeze()
        self.y = np.array(y).squeeze()
        self.ndim = theta.shape[-1] if self.theta.ndim > 1 else 1
        if not (np.all(np.isfinite(self.theta)) and np.all(np.isfinite(self.y))):
            raise ValueError("All theta and y values must be finite!")
        if len(bounds) != self.ndim:
            raise ValueError("ERROR: bounds provided but len(bounds) != ndim.\n"
                             "ndim = %d, len(bounds) = %d" % (self.ndim, len(bounds)))
        self.bounds = bounds
        self._lnprior, self._lnlike, self.priorSample = lnprior, lnlike, priorSample
        self.algorithm = str(algorithm).lower()
        if self.algorithm not in _UTILITIES:
            raise ValueError("Unknown algorithm. Valid options: bape, agp, naive, or alternate.")
        self.utility = _UTILITIES[self.algorithm]
        self.iburns, self.ithins, self.backends, self.gpPar = [], [], [], []
        self.sampler = None
        if gp is None:
            print("INFO: No GP specified. Initializing GP using ExpSquaredKernel.")
            gp = gpUtils.defaultGP(self.theta, self.y)
        self.gp = gp

    # ---------------------------------------------------------------- several GPUs
    def _ranks(self):
        """``(rank, world)`` under an initialised process group (unless ``distributed=False``), else None."""
        return apdist.context(self.group, self.distributed)

    def _chief(self):
        """True on the rank that prints, writes caches and calls the forward model."""
        ranks = self._ranks()
        return ranks is None or ranks[0] == 0

    def _agree(self, *values):
        """Rank 0's float64 arrays on every rank (a no-op without a process group)."""
        if self._ranks() is None:
            return values if len(values) > 1 else values[0]
        out = tuple(apdist.broadcast_bytes(np.asarray(v, dtype=np.float64), 0, self.group, enabled=self.distributed)
                    for v in values)
        return out if len(out) > 1 else out[0]

    # ------------------------------------------------------- surrogate log-probability
    def _gpll(self, theta, *args, **kwargs):
        """``(mu(theta), lnprior(theta))``, or ``(-inf, nan)`` when theta has no finite
        coordinate, the prior excludes it, or the prediction fails / is not finite
        (the three guards of approx.py:148-189)."""
        rejected = (-np.inf, np.nan)
        if not np.any(np.isfinite(theta)):
            return rejected
        prior = self._lnprior(theta)
        if not np.isfinite(prior):
            return rejected
        try:
            mean = self.gp.predict(self.y, np.array(theta).reshape(1, -1),
                                   return_cov=False, return_var=False)
        except ValueError:
            return rejected
        return (mean, prior) if np.isfinite(mean) else rejected

    def _gpllBatch(self, thetas):
        """:meth:`_gpll` for a whole walker ensemble ``thetas`` (W, D) with one
        mean-only device launch: ``(logp (W,), lnprior (W,))``, guarded row by row."""
        pts = np.asarray(thetas, dtype=float)
        if pts.ndim == 1:
            pts = pts.reshape(-1, self.ndim)
        fin = np.isfinite(pts)
        batch = getattr(self._lnprior, "batch", None)
        if batch is not None and fin.all():
            # the usual half-step of the sampler, without the row-by-row bookkeeping below: every coordinate finite, the
            # prior's vectorised twin (likelihood.py) in one call, one mean-only launch for the walkers inside the prior
            prior = np.asarray(batch(pts), dtype=float).reshape(len(pts))
            inside = np.isfinite(prior)
            if inside.all():
                mean = self.gp.predict(self.y, pts, return_cov=False, return_var=False)
                ok = np.isfinite(mean)
                if ok.all():
                    return mean, prior
                return np.where(ok, mean, -np.inf), np.where(ok, prior, np.nan)
            logp = np.full(len(pts), -np.inf)
            blob = np.full(len(pts), np.nan)
            rows = np.flatnonzero(inside)
            if rows.size:
                mean = self.gp.predict(self.y, pts[rows], return_cov=False, return_var=False)
                ok = np.isfinite(mean)
                keep = rows[ok]
                logp[keep] = mean[ok]
                blob[keep] = prior[keep]
            return logp, blob
        logp = np.full(len(pts), -np.inf)
        blob = np.full(len(pts), np.nan)
        some = fin.any(axis=1)                      # (a walker without a finite coordinate is rejected before the prior)
        if batch is not None and some.all():
            # the prior's vectorised twin (likelihood.py): one call per ensemble instead of one per walker
            prior = np.asarray(batch(pts), dtype=float).reshape(len(pts))
        else:
            prior = np.array([self._lnprior(p) if ok else -np.inf for p, ok in zip(pts, some)], dtype=float)
        rows = np.flatnonzero(np.isfinite(prior))
        if rows.size:
            if rows.size == len(pts) and fin.all():
                finite, sel = np.ones(len(pts), dtype=bool), pts                      # (the usual half-step: nothing to mask)
            else:
                finite = np.all(fin[rows], axis=1)
                sel = np.where(fin[rows], pts[rows], 0.0)
            mean = self.gp.predict(self.y, sel, return_cov=False, return_var=False)
            ok = finite & np.isfinite(mean)
            keep = rows[ok]
            logp[keep] = mean[ok]
            blob[keep] = prior[keep]
        return logp, blob

    # ------------------------------------------------------------------ GP re-fit
    def optGP(self, seed=None, method="powell", options=None, p0=None,
              nGPRestarts=1, gpHyperPrior=gpUtils.defaultHyperPrior):
        """Re-fit the GP hyper-parameters in place (approx.py:192-226).  Under a process group the
        restarts are spread over the ranks and every rank ends with the same optimum."""
        if self._ranks() is not None:
            apdist.sync_random_state(0, self.group, enabled=self.distributed)      # the restart start points are one global draw
        self.gp = gpUtils.optimizeGP(self.gp, self.theta, self.y, seed=seed,
                                     method=method, options=options, p0=p0,
                                     nGPRestarts=nGPRestarts, gpHyperPrior=gpHyperPrior,
                                     distributed=self.distributed, group=self.group)

    def _jointPrior(self):
        """``lnprior`` when it is a :class:`~approxposterior_amd.priors.JointPrior` (the prior the device paths
        can evaluate), else None."""
        return self._lnprior if isinstance(self._lnprior, appriors.JointPrior) else None

    # ------------------------------------------------------- design-point selection
    def _selectPoint(self, utility, theta0, nRestarts, method, options, nCandidates, polish, searchJac=False):
        """One design point: the minimiser of ``utility`` over the prior.  Under a process group the
        ``nCandidates`` draw is ONE global matrix (same random state on every rank), each rank sweeps its
        contiguous rows and the winners meet in a 16-byte-per-rank all-gather; the Nelder-Mead search is
        replicated and rank 0's answer kept."""
        scalarArgs = (self.y, self.gp, self._lnprior)
        ranks = self._ranks()
        joint = self._jointPrior()
        # the device gate (sweep and point search): the reference's utilities return +inf exactly where lnprior is not
        # finite, which for a JointPrior is outside its support (infinite edges on Gaussian dimensions)
        gate = self.bounds if joint is None else [tuple(r) for r in joint.support()]
        # (the device point search is gated by `gate`; the host search forwards `bounds` as the reference does)
        searchBounds = gate if self.deviceSearch else self.bounds
        if nCandidates is None:
            point, value = ut.minimizeObjective(utility, self.y, self.gp, sampleFn=self.priorSample,
                                                priorFn=self._lnprior, nRestarts=nRestarts, method=method,
                                                options=options, bounds=searchBounds, theta0=theta0,
                                                args=scalarArgs, onDevice=self.deviceSearch, jac=searchJac)
            return self._agree(point, value) if ranks is not None else (point, value)
        total = int(nCandidates)
        kind = ut.utilityKind(utility) if (ranks is not None or self.deviceCandidates) else None
        lo, hi = apdist.shard_bounds(total, ranks[1], ranks[0]) if ranks is not None else (0, total)
        mine, row = self._candidateDraw(total, joint, lo, hi)
        if ranks is None and not self.deviceCandidates:
            point, value = ut.sweepObjective(utility, self.y, self.gp, mine, bounds=gate)
        else:
            best, value = apdist.sharded_acquire(
                lambda offset: self.gp.acquire(self.y, mine, kind, bounds=gate, idx_offset=offset,
                                               device_record=True),
                lo, group=self.group if ranks is not None else None,
                enabled=self.distributed if ranks is not None else False)     # (no ranks: this process's own record, no gather)
            if best < 0:
                raise RuntimeError("ERROR: Cannot find a valid solution: no candidate is allowed by the prior")
            point = row(best)
        if polish:
            point, value = ut.minimizeObjective(utility, self.y, self.gp,
                                                sampleFn=self.priorSample, priorFn=self._lnprior,
                                                nRestarts=1, method=method, options=options,
                                                bounds=searchBounds, theta0=point, args=scalarArgs,
                                                onDevice=self.deviceSearch, jac=searchJac)
            if ranks is not None:
                point, value = self._agree(point, value)
        return point, value

    def _candidateDraw(self, total, joint, lo=0, hi=None):
        """``(cands, row)``: rows ``lo .. hi - 1`` (default: all) of ONE global candidate draw of ``total`` rows, and
        ``row(g)``, global row ``g`` alone as a host array -- the draw every ``nCandidates`` selection starts from.
        Without ``deviceCandidates`` the rows are ``priorSample`` draws on the host.  With it they are generated on the
        device from one integer of NumPy's global stream, from the prior itself when ``lnprior`` is a JointPrior
        (``joint``), else uniformly in the box ``bounds`` (which then IS the prior: priorSample is not consulted): no host
        draw, no H2D copy, and the global matrix is a function of (seed, row) alone, so a rank generates its own rows and
        the winning row is regenerated alone.  ``True``: the Philox streams (``GP.prior_candidates``,
        ``GP.box_candidates``); ``"sobol"``: one scrambled Sobol replicate (``GP.sobol_candidates``)."""
        hi = total if hi is None else hi
        mode = self.deviceCandidates
        if not mode:
            draws = np.asarray(self.priorSample(total), dtype=float).reshape(total, -1)
            return (draws if (lo, hi) == (0, total) else np.ascontiguousarray(draws[lo:hi])), lambda g: np.array(draws[g])
        if mode == "sobol" and total > george.SOBOL_MAX_ROWS:
            raise ValueError('deviceCandidates="sobol": the sequence has 2^30 rows, nCandidates = %d is beyond it' % total)
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        if mode == "sobol":
            source = {"bounds": self.bounds} if joint is None else {"prior": joint}
            gen = lambda m, off: self.gp.sobol_candidates(m, seed=seed, idx_offset=off, **source)         # noqa: E731
        elif joint is not None:
            gen = lambda m, off: self.gp.prior_candidates(m, joint, seed, idx_offset=off)                 # noqa: E731
        else:
            gen = lambda m, off: self.gp.box_candidates(m, self.bounds, seed, idx_offset=off)             # noqa: E731
        return gen(hi - lo, lo), lambda g: gen(1, g).cpu().numpy()[0]

    @staticmethod
    def _candidatesMode(deviceCandidates):
        """``deviceCandidates`` as kept on the object: False, True (the Philox streams) or "sobol"."""
        if isinstance(deviceCandidates, str):
            if deviceCandidates != "sobol":
                raise ValueError('deviceCandidates must be False, True or "sobol"')
            return "sobol"
        return bool(deviceCandidates)

    def _selectBatch(self, utilities, nCandidates, batchMethod="believer"):
        """``len(utilities)`` design points chosen jointly (:meth:`GP.acquire_batch`, the kriging believer) from
        ONE candidate draw -- the draw :meth:`_selectPoint` makes for one point; pick j minimises
        ``utilities[j]``.  A batch of one is :meth:`_selectPoint`'s sweep: same draw, same point.
        ``batchMethod="thompson"``: the points are the arg-maxes of posterior function draws over the same candidate
        draw (:meth:`GP.thompson_batch`); slots the draws left empty are topped up by the kriging believer under
        ``utilities``, with the rows already picked masked out."""
        total = int(nCandidates)
        kinds = [ut.utilityKind(fn) for fn in utilities]
        joint = self._jointPrior()
        gate = self.bounds if joint is None else [tuple(r) for r in joint.support()]
        cands, row = self._candidateDraw(total, joint)
        if not self.deviceCandidates:
            cands = self.gp.parse_samples(cands)
        if batchMethod == "thompson":
            idx = self.gp.thompson_batch(self.y, cands, len(kinds), bounds=gate)
            picked = [int(g) for g in idx if g >= 0]
            if len(picked) < len(kinds):
                free = np.ones(total, dtype=np.uint8)
                free[picked] = 0
                more, _ = self.gp.acquire_batch(self.y, cands, kinds[len(picked):], len(kinds) - len(picked),
                                                bounds=gate, mask=free)
                idx = np.array(picked + [int(g) for g in more], dtype=np.int64)
        else:
            idx, _ = self.gp.acquire_batch(self.y, cands, kinds, len(kinds), bounds=gate)
        if idx[0] < 0:
            raise RuntimeError("ERROR: Cannot find a valid solution: no candidate is allowed by the prior")
        # (a later step without an admissible candidate cannot happen: the earlier picks stay admissible)
        return [row(int(g)) for g in idx if g >= 0]

    def _integrationRefs(self, integrated):
        """(refs (J, D), density) of ``findNextPoint(integrated=...)``: an array is used as given, as samples of the
        surrogate posterior; an int J takes J thinned, flattened samples of ``self.sampler``'s chain after its estimated
        burn-in -- or, before any chain exists, J ``priorSample`` draws, uniform weights."""
        if not isinstance(integrated, (int, np.integer)):
            return np.asarray(integrated, dtype=np.float64), "posterior"
        J = int(integrated)
        cut = getattr(self, "_chainCut", None)
        if self.sampler is None or cut is None:
            return np.asarray(self.priorSample(J), dtype=np.float64).reshape(J, -1), "uniform"
        flat = self.sampler.get_chain(discard=cut[0], flat=True, thin=cut[1])
        if len(flat) < J:       # (a short chain: every post-burn-in sample, unthinned, then all of it)
            flat = self.sampler.get_chain(discard=cut[0], flat=True)
        if len(flat) < J:
            flat = self.sampler.get_chain(flat=True)
        rows = np.linspace(0, len(flat) - 1, min(J, len(flat))).astype(np.int64)
        return np.asarray(flat[rows], dtype=np.float64), "posterior"

    def _selectIntegrated(self, nCandidates, integrated):
        """One design point by the integrated acquisition (:meth:`GP.acquire_integrated`) over the candidate draw
        :meth:`_selectPoint` makes, behind the same gate."""
        total = int(nCandidates)
        joint = self._jointPrior()
        gate = self.bounds if joint is None else [tuple(r) for r in joint.support()]
        cands, row = self._candidateDraw(total, joint)
        if not self.deviceCandidates:
            cands = self.gp.parse_samples(cands)
        refs, density = self._integrationRefs(integrated)
        weights = self.gp.integration_weights(self.y, refs, density)
        best, value = self.gp.acquire_integrated(self.y, cands, refs, logWeights=weights, bounds=gate)
        if best < 0:
            raise RuntimeError("ERROR: Cannot find a valid solution: no candidate is allowed by the prior")
        return row(best), value

    def _absorbPoint(self, point, value):
        """Append (point, value) to the training set and move the GP onto it: same
        kernel / mean / white-noise objects and hyper-parameters (approx.py:693-717); the
        device GP extends its factor by one row instead of refactorising."""
        stack = np.vstack if self.theta.ndim > 1 else np.hstack
        self.theta = stack([self.theta, np.array(point)])
        self.y = np.hstack([self.y, value])
        hyper = self.gp.get_parameter_vector()
        grown = george.GP(kernel=self.gp.kernel, fit_mean=True, mean=self.gp.mean,
                          white_noise=self.gp.white_noise, fit_white_noise=False)
        grown.set_parameter_vector(hyper)
        if hasattr(grown, "_try_extend"):
            grown.compute(self.theta, previous=self.gp)
        else:
            grown.compute(self.theta)
        self.gp = grown
        return hyper

    def findNextPoint(self, theta0=None, computeLnLike=True, seed=None,
                      cache=True, gpOptions=None, gpP0=None, verbose=True,
                      nGPRestarts=1, nMinObjRestarts=5, gpMethod="powell",
                      minObjMethod="nelder-mead", minObjOptions=None,
                      runName="apRun", numNewPoints=1, optGPEveryN=1,
                      gpHyperPrior=gpUtils.defaultHyperPrior, args=None,
                      nCandidates=None, polish=False, deviceCandidates=None, batchSize=None, pool=None,
                      deviceSearch=None, searchJac=False, batchMethod="believer", integrated=None, **kwargs):
        """Select ``numNewPoints`` design points by minimising the (negative) utility;
        with ``computeLnLike`` evaluate the forward model at each, absorb it into the
        training set / GP and re-fit the hyper-parameters every ``optGPEveryN`` points
        (approx.py:527-754).  Returns ``theta`` or ``(theta, y)`` -- a single point /
        value when ``numNewPoints == 1``, arrays otherwise (approx.py:745-753).

        ``nCandidates`` replaces the restarted Nelder-Mead search by the fused device
        sweep over that many ``priorSample`` draws (box ``bounds`` as the prior);
        ``polish`` refines the sweep winner with one Nelder-Mead run;
        ``deviceCandidates=True`` draws the candidates on the device, uniformly in ``bounds``
        (counter-based Philox keyed by one integer from NumPy's global stream) instead of calling
        ``priorSample`` -- valid when the prior IS that box; when ``lnprior`` is a
        :class:`~approxposterior_amd.priors.JointPrior` they are drawn from that prior instead
        (``GP.prior_candidates``), and every ``nCandidates`` sweep is gated by ``lnprior.support()``.
        ``deviceCandidates="sobol"`` draws them quasi-randomly instead: one scrambled Sobol replicate
        (``GP.sobol_candidates``) keyed by the same integer, from the same prior or box, sharded and regenerated
        row by row in the same way -- a sweep that covers the prior without clumps or holes.  At most 2^30
        candidates (``ValueError`` beyond).

        ``batchSize=q`` (with ``nCandidates``): the points are chosen ``q`` at a time from one candidate draw
        per batch by :meth:`GP.acquire_batch` (each pick conditions the GP on the previous picks at their
        predicted values), so that the batch's forward models can run at once -- through ``pool.map`` when
        ``pool`` is given (any object with an ordered ``map``: a ``multiprocessing.Pool``, a
        ``concurrent.futures`` executor), else serially in pick order.  They are then absorbed in pick order,
        the GP is re-fitted once per batch when a point of the batch meets the ``optGPEveryN`` rule, and the
        cache is written after each batch.  ``batchSize=1`` is the plain ``nCandidates`` search.
        ``batchMethod="thompson"`` (with ``batchSize``) chooses the batch as the arg-maxes of ``q`` functions drawn
        from the GP posterior instead (:meth:`GP.thompson_batch`: one pass over the candidates, no variance sweep,
        whatever the utility); slots on which the draws agreed are filled by the kriging believer.

        ``deviceSearch=True`` (opt-in; kept on the object like ``deviceCandidates``) runs the Nelder-Mead point search
        -- the default without ``nCandidates``, and ``polish`` after a sweep -- on the device: all ``nMinObjRestarts``
        restarts in one launch (``utility.minimizeObjective(onDevice=True)``, :meth:`GP.nelder_mead_search`), same
        simplex arithmetic as SciPy.  The device evaluates the utility inside ``bounds`` -- or inside
        ``lnprior.support()`` when ``lnprior`` is a :class:`~approxposterior_amd.priors.JointPrior` -- and +inf
        outside: it assumes the prior is that box or support.  The solutions are still checked with ``lnprior`` on
        the host.  Under a process group the search is replicated and rank 0's answer kept, as on the host.

        ``searchJac=True`` (opt-in, with a gradient ``minObjMethod`` such as "l-bfgs-b"; not with ``deviceSearch``) gives
        the host point search -- and ``polish`` -- the utility's exact gradient (``utility.minimizeObjective(jac=True)``,
        :meth:`GP.predict_grad`) instead of SciPy's finite differences.

        ``integrated`` (with ``nCandidates``) replaces the utility's pick by the integrated acquisition
        (:meth:`GP.acquire_integrated`): the candidate whose evaluation most reduces the variance of the posterior
        estimate exp(f) integrated over reference points.  An int J takes J thinned samples of the last
        :meth:`runMCMC` chain after its estimated burn-in (before any chain: J ``priorSample`` draws, uniform weights);
        a (J, D) array is used as given, as posterior samples.  Same candidate draw and gate as the utility sweep;
        absorbing and re-fitting are unchanged.  Not with ``batchSize``, ``polish`` or a process group.
        """
        if batchMethod not in ("believer", "thompson"):
            raise ValueError('batchMethod must be "believer" or "thompson"')
        if batchMethod == "thompson" and batchSize is None:
            raise ValueError('batchMethod="thompson" needs batchSize: it chooses batches')
        if integrated is not None:
            if nCandidates is None:
                raise ValueError("integrated needs nCandidates: the integrated acquisition is a device pass over candidates")
            if isinstance(integrated, (bool, np.bool_)) or (isinstance(integrated, (int, np.integer))
                                                           and not 1 <= integrated <= _lib.MAX_REFS):
                raise ValueError("integrated must be a number of reference points between 1 and %d, or a (J, D) array"
                                 % _lib.MAX_REFS)
            if batchSize is not None:
                raise ValueError("integrated cannot be combined with batchSize: it chooses one point at a time")
            if polish:
                raise ValueError("integrated cannot be combined with polish=True")
            if self._ranks() is not None:
                raise NotImplementedError("integrated under a process group: every rank would need the same "
                                          "reference points and the winners' records gathered")
        if batchSize is not None:
            if nCandidates is None:
                raise ValueError("batchSize needs nCandidates: batches are chosen by the device sweep")
            if not isinstance(batchSize, (int, np.integer)) or not 1 <= batchSize <= _lib.MAX_FANTASY:
                raise ValueError("batchSize must be an integer between 1 and %d" % _lib.MAX_FANTASY)
            if polish:
                raise ValueError("batchSize cannot be combined with polish=True")
            if self._ranks() is not None:
                raise NotImplementedError("batchSize under a process group: a sharded batch would need the winning "
                                          "row's fantasy columns broadcast from the rank that owns it")
        if deviceCandidates is not None:
            self.deviceCandidates = self._candidatesMode(deviceCandidates)
        if deviceSearch is not None:
            self.deviceSearch = bool(deviceSearch)
        assert isinstance(numNewPoints, int) and numNewPoints >= 1
        assert isinstance(optGPEveryN, int) and optGPEveryN >= 1
        if verbose and numNewPoints < optGPEveryN:
            print("WARNING: numNewPoints < optGPEveryN: the GP hyperparameters will not be "
                  "re-optimized during this call.")
        fwdArgs = () if args is None else args
        points, values = [], []
        ranks = self._ranks()
        chief = self._chief()
        verbose, cache = verbose and chief, cache and chief      # one rank talks and writes
        if batchSize is not None:
            return self._findBatches(numNewPoints, int(batchSize), computeLnLike, nCandidates, pool, fwdArgs,
                                     kwargs, cache, verbose, optGPEveryN, runName,
                                     dict(seed=seed, method=gpMethod, options=gpOptions, p0=gpP0,
                                          nGPRestarts=nGPRestarts, gpHyperPrior=gpHyperPrior), batchMethod)
        for count in range(numNewPoints):
            if ranks is not None:
                # one global random stream: the candidate matrix / restart draws below are the same on
                # every rank whatever the forward model (rank 0 only) did to rank 0's stream
                apdist.sync_random_state(0, self.group, enabled=self.distributed)
            if self.algorithm == "alternate":      # AGP, BAPE, AGP, ... (approx.py:656-661)
                self.utility = (ut.AGPUtility, ut.BAPEUtility)[count % 2]
            if integrated is not None:
                point, _ = self._selectIntegrated(nCandidates, integrated)
            else:
                point, _ = self._selectPoint(self.utility, theta0, nMinObjRestarts, minObjMethod,
                                             minObjOptions, nCandidates, polish, searchJac=searchJac)
            points.append(point)
            if not computeLnLike:
                continue
            failure = None
            value = np.zeros(1)
            if chief:
                try:
                    like = self._lnlike(point, *fwdArgs, **kwargs)
                    like = like[0] if hasattr(like, "__iter__") else like      # (lnlike, blobs...) allowed
                    value = np.array([like + self._lnprior(point)], dtype=np.float64).reshape(1)
                except Exception as err:       # noqa: BLE001 -- raised on every rank just below
                    if ranks is None:
                        raise
                    failure = err
            if ranks is not None:
                # only rank 0 ran the forward model: if it raised there, every rank raises here instead of waiting
                # for a broadcast that never comes
                apdist.raise_together(failure, "the forward model (lnlike)", group=self.group, enabled=self.distributed)
            value = self._agree(value)             # the forward model ran once, on rank 0
            values.append(value)
            try:
                hyper = self._absorbPoint(point, value)
                if verbose:
                    print("hyperparameters", hyper)
                if cache:
                    self.gpPar.append(hyper)
                if count % optGPEveryN == 0:
                    self.optGP(seed=seed, method=gpMethod, options=gpOptions, p0=gpP0,
                               nGPRestarts=nGPRestarts, gpHyperPrior=gpHyperPrior)
            except ValueError:
                raise ValueError("GP couldn't optimize! names %s, parameters %s, %d training points"
                                 % (self.gp.get_parameter_names(), self.gp.get_parameter_vector(),
                                    len(self.y)))
            if cache:
                np.savez(_cacheName(runName, "APFModelCache"), theta=self.theta, y=self.y)
        if numNewPoints == 1:
            points = points[0]
            values = values[0] if computeLnLike else values
        if computeLnLike:
            return np.asarray(points), np.asarray(values)
        return np.asarray(points)

    def _findBatches(self, numNewPoints, q, computeLnLike, nCandidates, pool, fwdArgs, kwargs, cache, verbose,
                     optGPEveryN, runName, fit, batchMethod="believer"):
        """findNextPoint with ``batchSize=q`` (single process): ``numNewPoints`` points, ``q`` per batch."""
        points, values = [], []
        forward = _ForwardModel(self._lnlike, self._lnprior, fwdArgs, kwargs)
        for first in range(0, numNewPoints, q):
            counts = range(first, min(first + q, numNewPoints))
            if self.algorithm == "alternate":      # AGP, BAPE, AGP, ... by point index, as one point at a time
                utilities = [(ut.AGPUtility, ut.BAPEUtility)[count % 2] for count in counts]
                self.utility = utilities[-1]
            else:
                utilities = [self.utility] * len(counts)
            batch = self._selectBatch(utilities, nCandidates, batchMethod)
            points.extend(batch)
            if not computeLnLike:
                continue
            vals = list(pool.map(forward, batch)) if pool is not None else [forward(p) for p in batch]
            values.extend(vals)
            try:
                for point, value in zip(batch, vals):
                    hyper = self._absorbPoint(point, value)
                    if verbose:
                        print("hyperparameters", hyper)
                    if cache:
                        self.gpPar.append(hyper)
                if any(count % optGPEveryN == 0 for count in counts):
                    self.optGP(**fit)
            except ValueError:
                raise ValueError("GP couldn't optimize! names %s, parameters %s, %d training points"
                                 % (self.gp.get_parameter_names(), self.gp.get_parameter_vector(),
                                    len(self.y)))
            if cache:
                np.savez(_cacheName(runName, "APFModelCache"), theta=self.theta, y=self.y)
        if numNewPoints == 1:
            points = points[0]
            values = values[0] if computeLnLike else values
        if computeLnLike:
            return np.asarray(points), np.asarray(values)
        return np.asarray(points)

    # ------------------------------------------------------------------ surrogate MCMC
    def _dumpChain(self, runName):
        path = _cacheName(runName, "")
        self.backends.append(path)
        blobs = self.sampler.get_blobs()
        np.savez(path, chain=self.sampler.get_chain(), log_prob=self.sampler.get_log_prob(),
                 blobs=np.array([]) if blobs is None else blobs)

    def _requireBoxPrior(self):
        """For an ``lnprior`` that is not a :class:`~approxposterior_amd.priors.JointPrior`, the on-device
        sampler (``GP.sample_ensemble``) knows ONE prior: constant inside ``self.bounds``, -inf outside.
        ``_gpll`` returns the pair ``(mu(theta), lnprior(theta))`` (approx.py:167-188): the sampler takes
        ``mu`` as the log-probability and ``lnprior`` as a blob, so the prior only gates the chain (a walker is
        rejected where it is not finite).  The device cannot evaluate an arbitrary Python ``lnprior``, neither
        for that gate nor for the blobs, so it insists on the one prior it reproduces exactly -- the box -- and
        records no blobs.  ``lnprior`` is probed (own RandomState: the caller's NumPy stream is untouched) at
        the centre, at seeded points inside, just inside every corner and just outside every face: it must be
        one finite constant inside and non-finite outside, else ``ValueError``."""
        lo = np.array([b[0] for b in self.bounds], dtype=np.float64)
        hi = np.array([b[1] for b in self.bounds], dtype=np.float64)
        span = hi - lo
        rs = np.random.RandomState(20260304)
        inside = [0.5 * (lo + hi)] + list(lo + span * rs.uniform(0.0, 1.0, size=(8, len(lo))))
        for corner in range(min(2 ** len(lo), 16)):
            pick = np.array([(corner >> d) & 1 for d in range(len(lo))], dtype=np.float64)
            inside.append(lo + span * (1e-6 + pick * (1.0 - 2e-6)))
        vals = np.array([float(np.asarray(self._lnprior(p)).ravel()[0]) for p in inside])
        ok = np.all(np.isfinite(vals)) and np.all(np.abs(vals - vals[0]) <= 1e-12 * max(1.0, abs(vals[0])))
        outside = []
        for d in range(len(lo)):
            for sign, edge in ((-1.0, lo), (1.0, hi)):
                p = 0.5 * (lo + hi)
                p[d] = edge[d] + sign * 1e-2 * span[d]
                outside.append(p)
        with np.errstate(all="ignore"):
            out_vals = np.array([float(np.asarray(self._lnprior(p)).ravel()[0]) for p in outside])
        ok = ok and not np.any(np.isfinite(out_vals))
        if not ok:
            raise ValueError("runMCMC(onDevice=True) samples mu(theta) under the box prior self.bounds only; lnprior is not "
                             "constant inside / -inf outside these bounds (probed %d + %d points). Use onDevice=False "
                             "(batched=True keeps the GP on the device)." % (len(inside), len(outside)))

    def runMCMC(self, samplerKwargs=None, mcmcKwargs=None, runName="apRun",
                cache=True, estBurnin=True, thinChains=True, verbose=False,
                args=None, batched=True, onDevice=False, deviceAutocorr=False, tempering=None, hmc=None, **kwargs):
        """Sample the GP-surrogate posterior with the stretch-move ensemble sampler and
        estimate burn-in / thinning (approx.py:757-859): ``(sampler, iburn, ithin)``.
        ``samplerKwargs["moves"]`` (``mcmc.moves.DEMove()``, ``DESnookerMove()``, weighted lists, as emcee's ``moves``)
        replaces the stretch move on the host sampler and on the device sampler alike.

        ``batched`` (default) evaluates each half-ensemble with ONE mean-only GP launch
        (:meth:`_gpllBatch`); ``batched=False`` calls :meth:`_gpll` once per walker as
        emcee does for the reference; ``onDevice=True`` runs the entire chain as one
        persistent kernel (``GP.sample_ensemble``) -- valid when ``lnprior`` is the box
        prior ``self.bounds`` (constant inside, -inf outside): checked (:meth:`_requireBoxPrior`,
        ``ValueError`` otherwise) -- or a :class:`~approxposterior_amd.priors.JointPrior`: then the chain
        runs under ``lnprior.support()`` and carries the lnprior blobs, as the host chain does.
        With ``cache`` the chain goes to ``<runName>.npz`` (keys chain, log_prob, blobs)
        where the reference writes ``<runName>.h5``.
        ``deviceAutocorr=True`` (opt-in, needs ``onDevice=True``): the chain also stays on the device and
        ``estimateBurnin`` gets its autocorrelation time from there (``mcmc.integrated_time(onDevice=True)``); under a
        process group every rank uploads the gathered chain once and computes the same ``(iburn, ithin)``.
        ``tempering`` (opt-in, needs ``onDevice=True``): parallel tempering (``GP.sample_tempered``) for a multimodal
        surrogate -- an int (the rungs of the default ladder, ``mcmc.tempering_ladder``) or a dict with any of ``betas``,
        ``ntemps``, ``betaMin``, ``swapEvery``, ``ladders``.  ``self.sampler`` is then a :class:`mcmc.TemperedChain`:
        the cold rungs behind the usual accessors (burn-in, blobs, caching and ``evidence(proposal="gmm")`` work on
        them as they do on a ``DeviceChain``), plus the ladder's diagnostics and ``log_evidence()``.
        ``NotImplementedError`` under a process group.
        ``hmc`` (opt-in, needs ``onDevice=True``): Hamiltonian Monte Carlo with the surrogate's exact gradient
        (``GP.sample_hmc``) in place of the ensemble moves, for posteriors of more than ten or so dimensions -- ``True``
        or a dict with any of ``eps`` (step in the kernel's scaled coordinates, default 0.1), ``nLeap`` (16), ``jitter``
        (0.1), ``nWarmup`` (200), ``adaptEvery`` (20), ``targetAccept`` (0.8), ``adaptMass`` (False), ``mass``; another
        key is a ``ValueError``.  The ``nwalkers`` rows of ``initial_state`` start one chain each, ``mcmc.hmc_warmup``
        adapts the step over ``nWarmup`` iterations that are not kept, and ``iterations`` counts the iterations after it.
        ``self.sampler`` is then a :class:`mcmc.HMCChain`.  ``ValueError`` together with ``tempering`` or
        ``samplerKwargs["moves"]``; ``NotImplementedError`` under a process group.
        """
        if hmc is not None and hmc is not False:
            if not onDevice:
                raise ValueError("runMCMC(hmc=...) runs on the device: it needs onDevice=True")
            if tempering is not None:
                raise ValueError("runMCMC(hmc=...) and tempering=... are two samplers: choose one")
            if samplerKwargs is not None and samplerKwargs.get("moves") is not None:
                raise ValueError("runMCMC(hmc=...) makes no ensemble move: samplerKwargs['moves'] does not apply")
            hmcSpec = self._hmcSpec(hmc)
            if self._ranks() is not None:
                raise NotImplementedError("hmc under a process group: the chains would have to be sharded over the ranks "
                                          "and the warm-up's acceptance averaged across them")
        else:
            hmc = None
        if deviceAutocorr and not onDevice:
            raise ValueError("runMCMC(deviceAutocorr=True) diagnoses the chain of the device sampler: it needs onDevice=True")
        if tempering is not None and not onDevice:
            raise ValueError("runMCMC(tempering=...) tempers the device sampler: it needs onDevice=True")
        ranks = self._ranks()
        if tempering is not None and ranks is not None:
            raise NotImplementedError("tempering under a process group: the ladders would have to be sharded over the "
                                      "ranks and their rung means gathered")
        if ranks is not None:
            apdist.sync_random_state(0, self.group, enabled=self.distributed)
            verbose, cache = verbose and ranks[0] == 0, cache and ranks[0] == 0
        samplerKwargs, mcmcKwargs = mcmcUtils.validateMCMCKwargs(self, samplerKwargs,
                                                                 mcmcKwargs, verbose)
        if onDevice:
            if self._jointPrior() is None:
                self._requireBoxPrior()
            # the host sampler's shape check (EnsembleSampler.sample): the device would quietly take the row count
            p0 = np.asarray(mcmcKwargs["initial_state"], dtype=float)
            if p0.ndim == 1:
                p0 = p0.reshape(samplerKwargs["nwalkers"], self.ndim)
            if p0.shape != (samplerKwargs["nwalkers"], self.ndim):
                raise ValueError("incompatible input dimensions")
        if hmc is not None:
            self.sampler = self._sampleHMC(np.random.randint(0, 2 ** 31 - 1), mcmcKwargs, hmcSpec, deviceAutocorr)
        elif tempering is not None:
            self.sampler = self._sampleTempered(np.random.randint(0, 2 ** 31 - 1), samplerKwargs, mcmcKwargs, tempering,
                                                deviceAutocorr)
        elif onDevice or ranks is not None:
            # one ensemble per rank, seeded base + rank, gathered once along the walker axis
            # (no ranks -- no process group, or distributed=False inside somebody else's: the local chain, seed
            # ``base``, and no collective whatever group the process has open)
            base = np.random.randint(0, 2 ** 31 - 1)
            kept = []     # this rank's chain as the device sampler left it (deviceAutocorr)
            merged = apdist.replicated_ensembles(
                lambda seed: self._sampleReplica(seed, samplerKwargs, mcmcKwargs, args, kwargs,
                                                 batched, onDevice, keep=kept if deviceAutocorr else None),
                seed=base, group=self.group if ranks is not None else None,
                enabled=self.distributed if ranks is not None else False)
            chain, logp, naccept = merged[0], merged[1], merged[2]
            result = {"chain": chain, "log_prob": logp, "naccept": naccept,
                      "coords": chain[-1], "final_log_prob": logp[-1],
                      "blobs": merged[3] if len(merged) > 3 else None}
            if deviceAutocorr:
                if ranks is None:
                    result["chain_device"] = kept[0]
                else:
                    # the gathered chain of every rank's ensemble, uploaded once: the same input, hence the same
                    # (iburn, ithin), on every rank without a collective
                    import torch
                    result["chain_device"] = torch.from_numpy(chain).to(kept[0].device)
            self.sampler = emcee.DeviceChain(result, a=samplerKwargs.get("a", 2.0), moves=samplerKwargs.get("moves"))
        else:
            self.sampler = self._hostSampler(samplerKwargs, args, kwargs, batched)
            for _ in self.sampler.sample(**mcmcKwargs):
                pass
        if verbose:
            print("mcmc finished")
        if cache:
            self._dumpChain(runName)
        iburn, ithin = mcmcUtils.estimateBurnin(self.sampler, estBurnin=estBurnin,
                                                thinChains=thinChains, verbose=verbose)
        self._chainCut = (iburn, ithin)     # (evidence(proposal="gmm") fits its proposal to the chain cut this way)
        return self.sampler, iburn, ithin

    _HMC_DEFAULTS = {"eps": 0.1, "nLeap": 16, "jitter": 0.1, "nWarmup": 200, "adaptEvery": 20, "targetAccept": 0.8,
                     "adaptMass": False, "mass": None}

    def _hmcSpec(self, hmc):
        """``runMCMC``'s ``hmc`` argument as the full dict of settings; ``ValueError`` for anything else than True or a
        dict of known keys."""
        spec = dict(self._HMC_DEFAULTS)
        if hmc is True:
            return spec
        if not isinstance(hmc, dict) or any(k not in spec for k in hmc):
            raise ValueError("hmc must be True or a dict with keys from %s" % (tuple(spec),))
        spec.update(hmc)
        return spec

    def _sampleHMC(self, seed, mcmcKwargs, spec, keepDevice):
        """The :class:`mcmc.HMCChain` of ``runMCMC(hmc=...)``: the warm-up (``mcmc.hmc_warmup``), then the sampling run
        at the adapted step, its global iteration numbers following the warm-up's."""
        joint = self._jointPrior()
        extra = {} if joint is None else {"prior": joint}
        coords, eps, mass, history, it = emcee.hmc_warmup(
            self.gp, self.y, mcmcKwargs["initial_state"], self.bounds, spec["eps"], spec["nLeap"], nWarmup=spec["nWarmup"],
            adaptEvery=spec["adaptEvery"], targetAccept=spec["targetAccept"], jitter=spec["jitter"], mass=spec["mass"],
            adaptMass=bool(spec["adaptMass"]), seed=seed, **extra)
        res = self.gp.sample_hmc(self.y, coords, mcmcKwargs["iterations"], self.bounds, eps, spec["nLeap"],
                                 jitter=spec["jitter"], mass=mass, seed=seed, iteration0=it, keep_device=bool(keepDevice),
                                 **extra)
        res["mass"] = mass
        return emcee.HMCChain(res, warmup=history)

    def _sampleTempered(self, seed, samplerKwargs, mcmcKwargs, tempering, keepDevice):
        """The :class:`mcmc.TemperedChain` of ``runMCMC(tempering=...)``: ``tempering`` is the number of rungs of the
        default ladder or a dict (``betas`` | ``ntemps``, ``betaMin``; ``swapEvery``, ``ladders``).  The default ladder
        ends at beta = 0 where the box is finite."""
        spec = {"ntemps": tempering} if isinstance(tempering, (int, np.integer)) and not isinstance(tempering, bool) \
            else tempering
        known = ("betas", "ntemps", "betaMin", "swapEvery", "ladders")
        if not isinstance(spec, dict) or any(k not in known for k in spec):
            raise ValueError("tempering must be an int (rungs) or a dict with keys from %s" % (known,))
        joint = self._jointPrior()
        box = np.asarray(self.bounds if joint is None else joint.support(), dtype=np.float64).reshape(-1, 2)
        if "betas" in spec:
            if "ntemps" in spec or "betaMin" in spec:
                raise ValueError("tempering: betas is the whole ladder; ntemps and betaMin describe the default one")
            betas = np.asarray(spec["betas"], dtype=np.float64)
        else:
            ladder = {} if "betaMin" not in spec else {"betaMin": spec["betaMin"]}
            betas = emcee.tempering_ladder(spec.get("ntemps", 4), zero=bool(np.all(np.isfinite(box))), **ladder)
        extra = {} if joint is None else {"prior": joint}
        if "swapEvery" in spec:
            extra["swapEvery"] = spec["swapEvery"]
        moves, a = samplerKwargs.get("moves"), samplerKwargs.get("a", 2.0)
        if moves is None and float(a) != 2.0:
            moves = emcee.StretchMove(a)
        res = self.gp.sample_tempered(self.y, mcmcKwargs["initial_state"], mcmcKwargs["iterations"], self.bounds, betas,
                                      seed=seed, ladders=spec.get("ladders", 1), moves=moves, keep_device=bool(keepDevice),
                                      **extra)
        return emcee.TemperedChain(res, a=a, moves=samplerKwargs.get("moves"))

    def _hostSampler(self, samplerKwargs, args, kwargs, batched, seed=None):
        setup = dict(samplerKwargs)
        if batched:
            setup["log_prob_fn"] = lambda pts, *a, **k: self._gpllBatch(pts)
            setup["vectorize"] = True
        if seed is not None:
            setup["seed"] = seed
        return emcee.EnsembleSampler(**setup, backend=None, args=args, kwargs=kwargs,
                                     blobs_dtype=[("lnprior", float)])

    def _sampleReplica(self, seed, samplerKwargs, mcmcKwargs, args, kwargs, batched, onDevice, keep=None):
        """This rank's ensemble: ``(chain, log_prob, naccept[, blobs])`` for :func:`dist.replicated_ensembles`.
        ``keep``: a list that receives the device tensor of the chain (device sampler only)."""
        if onDevice:
            joint = self._jointPrior()
            extra = {} if joint is None else {"prior": joint}
            if keep is not None:
                extra["keep_device"] = True
            if samplerKwargs.get("moves") is not None:
                extra["moves"] = samplerKwargs["moves"]
            res = self.gp.sample_ensemble(self.y, mcmcKwargs["initial_state"], mcmcKwargs["iterations"],
                                          self.bounds, a=samplerKwargs.get("a", 2.0), seed=seed, **extra)
            if keep is not None:
                keep.append(res["chain_device"])
            out = (res["chain"], res["log_prob"], res["naccept"])
            return out if joint is None else out + (res["blobs"],)
        sampler = self._hostSampler(samplerKwargs, args, kwargs, batched, seed=seed)
        for _ in sampler.sample(**mcmcKwargs):
            pass
        blobs = sampler.get_blobs()
        out = (sampler.get_chain(), sampler.get_log_prob(), sampler._naccepted)
        return out if blobs is None else out + (blobs,)

    # ------------------------------------------------------- evidence by importance sampling
    def _mixtureProposal(self, proposal):
        """(weights, means, covariances) of a mixture proposal: a tuple of the three, or an object with ``weights_``,
        ``means_``, ``covariances_`` of ``covariance_type == "full"`` (sklearn's GaussianMixture, ``fitGMM``'s result)."""
        if isinstance(proposal, (tuple, list)):
            if len(proposal) != 3:
                raise ValueError("a mixture proposal is the tuple (weights, means, covariances)")
            return proposal
        if all(hasattr(proposal, a) for a in ("weights_", "means_", "covariances_")):
            if getattr(proposal, "covariance_type", "full") != "full":
                raise ValueError("evidence: a mixture proposal needs covariance_type == 'full', not %r"
                                 % (proposal.covariance_type,))
            return proposal.weights_, proposal.means_, proposal.covariances_
        raise ValueError("evidence: proposal must be 'prior', 'box', 'gmm', a (weights, means, covariances) tuple or a "
                         "fitted full-covariance mixture, not %r" % (proposal,))

    def evidence(self, nSamples=2 ** 20, proposal="prior", seed=None, chunk=2 ** 20, samples=None, maxComp=3,
                 covScale=1.0, surrogateDraws=0, nFeatures=2048, qmc=None):
        """The model evidence and chain-free posterior moments of the surrogate by importance sampling on the device.
        The GP models the unnormalised log-posterior (``y = lnlike + lnprior``), so ``Z = int exp(mu(t)) dt`` over the
        prior's support is the evidence; with ``nSamples`` draws from a proposal ``q`` the weights ``exp(mu - ln q)``
        give ``logZ`` with a standard error, the posterior mean and covariance -- an independent check on
        :meth:`runMCMC`'s chain -- and an effective sample size that says when to distrust both.  Returns
        :func:`utility.importanceSummary`'s dict (``logZ``, ``logZErr``, ``ess``, ``mean``, ``cov``, ``nInside``).

        ``proposal``: ``"box"`` -- uniform on ``self.bounds`` (``GP.box_candidates``), ``ln q = -sum log(hi - lo)``;
        ``"prior"`` -- draws from ``lnprior``, which must be a :class:`~approxposterior_amd.priors.JointPrior`
        (``ValueError`` otherwise), ``ln q`` its log-density; a mixture -- a tuple ``(weights, means, covariances)``
        or an object with ``weights_``, ``means_``, ``covariances_`` of ``covariance_type == "full"``, covariances
        scaled by ``covScale`` (``GP.mixture_candidates``); ``"gmm"`` -- :func:`gmmUtils.fitGMM` ``(samples,
        maxComp=maxComp)`` (needs scikit-learn), ``samples`` defaulting to the last :meth:`runMCMC` chain after its
        burn-in and thinning (``ValueError`` when there is none).

        Rows are gated by ``lnprior.support()`` for a JointPrior, else by ``self.bounds``; a gated row weighs nothing
        and still counts in ``nSamples``.  The moments are taken about the training point with the largest ``y``.
        Rows are processed ``chunk`` at a time; chunk j draws rows ``j chunk ..`` of the global proposal matrix, a
        function of (seed, row) alone, so the estimate does not depend on ``chunk`` beyond the rounding of
        :func:`utility.mergeImportance`.  ``seed=None`` takes one from NumPy's global stream.  Under a process group
        every rank computes the same numbers from the same seed.

        ``logZErr`` measures the scatter of the weights that were drawn.  A proposal with lighter tails than
        ``exp(mu)`` rarely draws the rows that carry the weight, and ``logZErr`` comes out misleadingly small: watch
        ``ess`` (a small fraction of ``nSamples`` is the warning) and widen a mixture proposal with ``covScale``.

        All of the above is the plug-in estimate: the GP's mean taken for the log-posterior.  ``surrogateDraws = S > 0``
        adds the surrogate's own error bar: S functions are drawn from the GP posterior (:meth:`gp.GP.sample_paths` with
        ``nFeatures`` random features, in groups of at most 32) and every draw is integrated over the SAME proposal rows
        (:meth:`gp.GP.importance_paths`), so the result gains :func:`utility.importanceDrawsSummary`'s keys --
        ``logZDraws``, ``essDraws``, ``meanDraws``, ``covDraws``, ``logZSurrogateErr``, ``meanSurrogateErr``,
        ``logZExpected``, ``nEmptyDraws`` -- while the keys above keep the bits of the ``surrogateDraws=0`` call with
        the same seed.  ``logZSurrogateErr`` is the scatter of ``logZ`` over the draws: large where the GP has few
        training points under the posterior's mass, whatever ``logZErr`` says.  NumPy's global stream is used in this
        order: the seed (if ``seed`` is None), then every group's ``sample_paths`` in turn, all before the first chunk;
        under a process group the stream is synchronised first, so every rank draws the same functions.  The
        hyper-parameters are held fixed, and the random-feature error is O(nFeatures^-1/2) in the draws' covariance.

        ``qmc = R >= 2`` (randomised quasi-Monte Carlo; ``ValueError`` for 1 and for R > nSamples) replaces the
        pseudo-random rows by R independently scrambled replicates of a Sobol sequence (``GP.sobol_candidates``):
        replicate r is rows ``0 .. n - 1`` of the sequence with ``replicate=r`` under the same ``seed``,
        ``n = nSamples // R`` -- take ``n`` a power of two, the sizes at which the sequence is balanced.  Every proposal
        kind works, ``chunk`` and ``surrogateDraws`` work as before (draw records merged across replicates), and the
        result is :func:`utility.importanceReplicatesSummary`'s: ``logZ``, ``mean``, ``cov``, ``ess``, ``nInside`` pooled
        over the ``R n`` rows, ``logZErr`` the scatter of the replicates' evidences, plus ``logZReplicates``,
        ``meanReplicates``, ``meanErr``, ``logZErrIID`` (the delta-method figure above, which over-states a
        quasi-random error) and ``qmc``.  The integrand is smooth -- a GP mean -- so at low dimension the error falls
        far faster than ``nSamples^-1/2``; the gain shrinks with the dimension and where the proposal covers the mass
        badly, and a proposal that misses the mass still gives a small error bar next to a small ``ess``.  The default
        ``qmc=None`` is the pseudo-random estimate, bit for bit."""
        nSamples, chunk = int(nSamples), int(chunk)
        if nSamples < 1 or chunk < 1:
            raise ValueError("evidence: nSamples and chunk must be positive")
        if qmc is not None:
            qmc = int(qmc)
            if qmc < 2 or qmc > nSamples:
                raise ValueError("evidence: qmc is the number of scrambled replicates: 2 <= qmc <= nSamples (the error "
                                 "bar is their scatter)")
            if nSamples // qmc > george.SOBOL_MAX_ROWS:
                raise ValueError("evidence: a Sobol replicate has at most 2^30 rows")
        surrogateDraws = int(surrogateDraws)
        if surrogateDraws < 0:
            raise ValueError("evidence: surrogateDraws must not be negative")
        joint = self._jointPrior()
        gate = self.bounds if joint is None else [tuple(r) for r in joint.support()]
        logVolume, mixture = 0.0, None
        if isinstance(proposal, str) and proposal == "prior":
            if joint is None:
                raise ValueError("evidence(proposal='prior') draws from lnprior on the device: lnprior must be a "
                                 "priors.JointPrior. Use proposal='box', 'gmm' or a mixture.")
        elif isinstance(proposal, str) and proposal == "box":
            b = np.asarray(self.bounds, dtype=np.float64).reshape(-1, 2)
            logVolume = float(np.sum(np.log(b[:, 1] - b[:, 0])))
        elif isinstance(proposal, str) and proposal == "gmm":
            if samples is None:
                cut = getattr(self, "_chainCut", None)
                if getattr(self, "sampler", None) is None or cut is None:
                    raise ValueError("evidence(proposal='gmm') fits its proposal to posterior samples: pass samples= or "
                                     "call runMCMC first")
                samples = self.sampler.get_chain(discard=cut[0], flat=True, thin=cut[1])
            mixture = self._mixtureProposal(gmmUtils.fitGMM(samples, maxComp=maxComp))
        else:
            mixture = self._mixtureProposal(proposal)
        if seed is None or surrogateDraws > 0:
            if self._ranks() is not None:       # one NumPy stream on every rank, as runMCMC arranges: the same seed
                apdist.sync_random_state(0, self.group, enabled=self.distributed)     # (and the same function draws)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        groups = [self.gp.sample_paths(self.y, min(_lib.MAX_DRAWS, surrogateDraws - g), nFeatures)
                  for g in range(0, surrogateDraws, _lib.MAX_DRAWS)]
        drawRecords = [None] * surrogateDraws
        centre = np.array(self.theta[int(np.argmax(self.y))], dtype=np.float64).ravel()
        # the rows: one Philox stream of nSamples rows, or qmc Sobol replicates of nSamples // qmc rows each
        nRows = nSamples if qmc is None else nSamples // qmc

        def draw(mc, off, rep):
            """(T, lnq) of rows off .. off + mc - 1 (lnq None: the constant -logVolume of the box)."""
            sobol = None if qmc is None else dict(seed=seed, replicate=rep, idx_offset=off)
            if mixture is not None:
                if sobol is not None:
                    return self.gp.sobol_candidates(mc, mixture=mixture, covScale=covScale, **sobol)
                return self.gp.mixture_candidates(mc, mixture[0], mixture[1], mixture[2], seed, idx_offset=off,
                                                  covScale=covScale)
            if proposal == "prior":
                T = (self.gp.prior_candidates(mc, joint, seed, idx_offset=off) if sobol is None
                     else self.gp.sobol_candidates(mc, prior=joint, **sobol))
                return T, self.gp.prior_lnprior(T, joint)
            return (self.gp.box_candidates(mc, self.bounds, seed, idx_offset=off) if sobol is None
                    else self.gp.sobol_candidates(mc, bounds=self.bounds, **sobol)), None

        records = []
        for rep in range(1 if qmc is None else qmc):
            record = None
            for off in range(0, nRows, chunk):
                T, lnq = draw(min(chunk, nRows - off), off, rep)
                part = self.gp.importance_pass(self.y, T, lnq=lnq, bounds=gate, centre=centre)
                record = part if record is None else ut.mergeImportance(record, part)
                for g, paths in enumerate(groups):
                    parts = self.gp.importance_paths(self.y, T, paths, lnq=lnq, bounds=gate, centre=centre)
                    for j, p in enumerate(parts):
                        s = g * _lib.MAX_DRAWS + j
                        drawRecords[s] = p if drawRecords[s] is None else ut.mergeImportance(drawRecords[s], p)
            records.append(record)
        if qmc is None:
            out = ut.importanceSummary(records[0], nSamples, logVolume=logVolume)
        else:
            out = ut.importanceReplicatesSummary(records, nRows, logVolume=logVolume)
        if surrogateDraws > 0:
            out.update(ut.importanceDrawsSummary(drawRecords, len(records) * nRows, logVolume=logVolume))
        return out

    def runNested(self, nlive=512, batch=16, nsteps=None, nruns=None, dlogz=0.01, maxBatches=None, seed=None,
                  sigma=1.0e-5, gamma0=None):
        """The model evidence, its error, the information and weighted posterior samples of the surrogate by nested
        sampling on the device (:meth:`gp.GP.sample_nested`): what :meth:`evidence` gives, without a proposal to choose --
        the runs start from the prior's box and compress towards the modes wherever they are.  The prior measure is
        the uniform one on the box, as for ``evidence(proposal="box")``: the GP models the unnormalised log-posterior,
        so the prior's density is already inside ``mu``.

        The box is ``self.bounds``, intersected with ``lnprior.support()`` under a
        :class:`~approxposterior_amd.priors.JointPrior` (the gate of :meth:`evidence`); a box that is not finite raises
        ``ValueError``.  ``seed=None`` takes one from NumPy's global stream; under a process group every rank computes
        the same numbers from the same seed.  The :class:`mcmc.NestedResult` is returned and kept as ``self.nested``;
        ``self.sampler`` and everything :meth:`run`, :meth:`runMCMC` and :meth:`evidence` keep are left alone."""
        b = np.asarray(self.bounds, dtype=np.float64).reshape(-1, 2)
        joint = self._jointPrior()
        if joint is not None:
            s = np.asarray([tuple(r) for r in joint.support()], dtype=np.float64).reshape(-1, 2)
            if s.shape != b.shape:
                raise ValueError("runNested: lnprior.support() and bounds disagree on the dimension")
            b = np.stack([np.maximum(b[:, 0], s[:, 0]), np.minimum(b[:, 1], s[:, 1])], axis=1)
        if not (np.all(np.isfinite(b)) and np.all(b[:, 0] < b[:, 1])):
            raise ValueError("runNested needs a finite, non-empty box: the uniform measure on it is the prior measure")
        args = george.GP._nested_arguments(len(b), b, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0)
        if seed is None:
            if self._ranks() is not None:       # one NumPy stream on every rank, as evidence() arranges: the same seed
                apdist.sync_random_state(0, self.group, enabled=self.distributed)
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        _, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0 = args
        self.nested = self.gp.sample_nested(self.y, b, nlive=nlive, batch=batch, nsteps=nsteps, nruns=nruns, dlogz=dlogz,
                                            maxBatches=maxBatches, seed=seed, sigma=sigma,
                                            gamma0=gamma0 if gamma0 > 0.0 else None)
        return self.nested

    # ---------------------------------------------------------------------- outer loop
    def run(self, m=10, nmax=2, seed=None, timing=False, verbose=True,
            mcmcKwargs=None, samplerKwargs=None, estBurnin=False,
            thinChains=False, runName="apRun", cache=True, gpMethod="powell",
            gpOptions=None, gpP0=None, optGPEveryN=1, nGPRestarts=1,
            nMinObjRestarts=5, onlyLastMCMC=False, initGPOpt=True, kmax=3,
            gpHyperPrior=gpUtils.defaultHyperPrior, eps=1.0, convergenceCheck=False,
            minObjMethod="nelder-mead", minObjOptions=None, args=None,
            nCandidates=None, onDevice=False, batched=True, deviceCandidates=None, batchSize=None, pool=None,
            deviceSearch=None, deviceAutocorr=False, searchJac=False, batchMethod="believer", tempering=None, hmc=None,
            integrated=None, **kwargs):
        """BAPE / AGP outer loop (approx.py:229-524): ``nmax`` times, find ``m`` design
        points (re-fitting the GP every ``optGPEveryN``), sample the surrogate posterior,
        record burn-in / thinning, and -- with ``convergenceCheck`` -- stop once the
        marginal means have moved by less than ``eps`` previous standard deviations for
        ``kmax`` consecutive iterations.  (The reference honours that rule only when
        ``verbose`` is set, quirk Q4; here it does not depend on verbosity.)
        ``nCandidates`` switches the point search to the fused device sweep
        (``deviceCandidates``: drawn on the device, see :meth:`findNextPoint`);
        ``onDevice`` / ``batched`` are passed to :meth:`runMCMC`; ``batchSize`` / ``pool`` to
        :meth:`findNextPoint` (design points chosen and their forward models run in batches; ``batchMethod``:
        "believer" or "thompson", how a batch is chosen), and ``deviceSearch``
        (the Nelder-Mead point search on the device) and ``searchJac`` (exact gradients for a gradient
        ``minObjMethod``).  ``deviceAutocorr`` is passed to :meth:`runMCMC` too (burn-in and
        thinning from the device's autocorrelation estimate; needs ``onDevice=True``), and so is ``tempering``
        (parallel tempering of the device sampler; needs ``onDevice=True``) and ``hmc`` (Hamiltonian Monte Carlo on the
        device in place of the ensemble moves; needs ``onDevice=True``).  ``integrated`` is passed to
        :meth:`findNextPoint` (the integrated acquisition; needs ``nCandidates``)."""
        if deviceAutocorr and not onDevice:
            raise ValueError("run(deviceAutocorr=True) needs onDevice=True")
        if tempering is not None and not onDevice:
            raise ValueError("run(tempering=...) tempers the device sampler: it needs onDevice=True")
        if hmc is not None and hmc is not False and not onDevice:
            raise ValueError("run(hmc=...) runs on the device: it needs onDevice=True")
        if batchMethod not in ("believer", "thompson"):
            raise ValueError('batchMethod must be "believer" or "thompson"')
        if batchMethod == "thompson" and batchSize is None:
            raise ValueError('batchMethod="thompson" needs batchSize: it chooses batches')
        if convergenceCheck and onlyLastMCMC:
            raise RuntimeError("If convergenceCheck is True, must run an MCMC each iteration.\n"
                               "convergenceCheck = %d onlyLastMCMC = %d" % (convergenceCheck, onlyLastMCMC))
        verbose, cache = verbose and self._chief(), cache and self._chief()
        if cache:
            np.savez(_cacheName(runName, "APFModelCache"), theta=self.theta, y=self.y)
            self.gpPar = []
        if seed is not None:
            np.random.seed(seed)
        if timing:
            self.trainingTime, self.mcmcTime = [], []
        monitor = _MarginalMonitor(eps, kmax) if convergenceCheck else None
        if monitor is not None:
            self.marginalMeans, self.marginalStds = monitor.means, monitor.stds
            self.marginalZScores = monitor.zscores
        fit = dict(seed=seed, nGPRestarts=nGPRestarts, gpHyperPrior=gpHyperPrior)
        if initGPOpt:
            self.optGP(method=gpMethod, options=gpOptions, p0=gpP0, **fit)
        for iteration in range(nmax):
            if verbose:
                print("Iteration: %d" % iteration)
            clock = time.time()
            self.findNextPoint(computeLnLike=True, cache=cache, gpMethod=gpMethod,
                               gpOptions=gpOptions, nMinObjRestarts=nMinObjRestarts,
                               optGPEveryN=optGPEveryN, numNewPoints=m,
                               minObjMethod=minObjMethod, minObjOptions=minObjOptions,
                               runName=runName, theta0=None, args=args, verbose=verbose,
                               nCandidates=nCandidates, deviceCandidates=deviceCandidates, batchSize=batchSize,
                               pool=pool, deviceSearch=deviceSearch, searchJac=searchJac, batchMethod=batchMethod,
                               **({} if integrated is None else {"integrated": integrated}), **fit, **kwargs)
            if timing:
                self.trainingTime.append(time.time() - clock)
            if cache:
                np.savez(_cacheName(runName, "APGP"), gpParamNames=self.gp.get_parameter_names(),
                         gpParamValues=self.gpPar)
            if onlyLastMCMC and iteration != nmax - 1:
                self.sampler = None
                continue
            clock = time.time()
            _, iburn, ithin = self.runMCMC(samplerKwargs=samplerKwargs, mcmcKwargs=mcmcKwargs,
                                           runName="%s%d" % (runName, iteration), cache=cache,
                                           estBurnin=estBurnin, thinChains=thinChains,
                                           verbose=verbose, args=args, onDevice=onDevice,
                                           batched=batched, deviceAutocorr=deviceAutocorr, tempering=tempering, hmc=hmc,
                                           **kwargs)
            self.iburns.append(iburn)
            self.ithins.append(ithin)
            if timing:
                self.mcmcTime.append(time.time() - clock)
                if cache:
                    np.savez(_cacheName(runName, "APTiming"), trainingTime=self.trainingTime,
                             mcmcTime=self.mcmcTime)
            if monitor is None:
                continue
            converged = monitor.update(self.sampler.get_chain(discard=iburn, flat=True, thin=ithin))
            if cache:
                monitor.save(_cacheName(runName, "ConvergenceCache"))
            if converged:
                if verbose:
                    print("Approximate marginal posterior distributions converged: |z| = %s < eps = %e "
                          "for %d iterations" % (monitor.zscores[-1], eps, kmax))
                break

    # ----------------------------------------------------------------------------- MAP
    def findMAP(self, theta0=None, method="nelder-mead", options=None, nRestarts=15, deviceSearch=None,
                searchJac=False):
        """Maximum of the function the GP has learned: minimise minus the GP mean from
        ``nRestarts`` starts around ``theta0`` (default: the best training point)
        (approx.py:862-926).  Returns ``(MAP, MAPVal)``.
        ``deviceSearch`` (default: the object's ``deviceSearch``) runs the restarts on the device
        over -mu, gated by ``bounds`` or the JointPrior's support (see :meth:`findNextPoint`).
        ``searchJac=True`` (with a gradient ``method``) gives the host search the exact gradient of -mu."""
        if theta0 is None:
            start = self.theta[np.argmax(self.y)]
        else:
            start = np.array(theta0).reshape(1, self.theta.shape[-1])
        if options is None and str(method).lower() == "nelder-mead":
            options = {"adaptive": True}

        def minusMean(x):
            return -(self._gpll(x)[0]) if np.isfinite(self._lnprior(x)) else np.inf
        minusMean.searchKind = "negmean"           # -mu on the device (utility.searchKind)

        onDevice = self.deviceSearch if deviceSearch is None else bool(deviceSearch)
        joint = self._jointPrior()
        if onDevice:
            bounds = self.bounds if joint is None else [tuple(r) for r in joint.support()]
        else:
            bounds = self.bounds
        if self._ranks() is not None:
            apdist.sync_random_state(0, self.group, enabled=self.distributed)
        best, value = ut.minimizeObjective(minusMean, self.y, self.gp, self.priorSample,
                                           self._lnprior, nRestarts=nRestarts, args=None,
                                           method=method, options=options, bounds=bounds,
                                           theta0=start, onDevice=onDevice, jac=searchJac)
        if self._ranks() is not None:
            best, value = self._agree(best, value)
        return best, -value

    # ---------------------------------------------------------- Bayesian optimisation
    def bayesOpt(self, nmax, theta0=None, tol=1.0e-3, kmax=3, seed=None,
                 verbose=True, runName="apRun", cache=True, gpMethod="powell",
                 gpOptions=None, gpP0=None, optGPEveryN=1, nGPRestarts=1,
                 nMinObjRestarts=5, initGPOpt=True, minObjMethod="nelder-mead",
                 gpHyperPrior=gpUtils.defaultHyperPrior, minObjOptions=None,
                 findMAP=True, args=None, nCandidates=None, deviceCandidates=None, deviceSearch=None,
                 searchJac=False, batchSize=None, pool=None, batchMethod="believer", **kwargs):
        """Bayesian optimisation (approx.py:929-1151): one design point per iteration by
        the object's utility (use algorithm="jones"), optionally the MAP of the GP mean
        after each, stop after ``kmax`` consecutive iterations whose best value changed
        by less than ``tol``.  Returns the reference's solution dictionary (thetaBest,
        valBest, thetas, vals, nev [, thetasMAP, valsMAP, thetaMAPBest, valMAPBest]).
        ``deviceSearch`` runs the point searches and the MAP searches on the device (see :meth:`findNextPoint`);
        ``searchJac`` gives both host searches exact gradients (with a gradient ``minObjMethod``).
        ``batchSize=q`` (with ``nCandidates``): each iteration chooses ``q`` points as one batch and evaluates their
        forward models together, through ``pool.map`` when ``pool`` is given (see :meth:`findNextPoint`;
        ``batchMethod="thompson"`` draws the batch from the posterior, which suits optimisation whatever the
        utility); ``nev`` counts forward-model evaluations, ``q`` per iteration."""
        if batchSize is None and batchMethod != "believer":
            raise ValueError('batchMethod needs batchSize: it chooses batches')
        if batchSize is not None:
            if nCandidates is None:
                raise ValueError("batchSize needs nCandidates: batches are chosen by the device sweep")
            if not isinstance(batchSize, (int, np.integer)) or not 1 <= batchSize <= _lib.MAX_FANTASY:
                raise ValueError("batchSize must be an integer between 1 and %d" % _lib.MAX_FANTASY)
            if batchMethod not in ("believer", "thompson"):
                raise ValueError('batchMethod must be "believer" or "thompson"')
        batch = {} if batchSize is None else dict(batchSize=int(batchSize), pool=pool, batchMethod=batchMethod)
        perIteration = 1 if batchSize is None else int(batchSize)
        verbose, cache = verbose and self._chief(), cache and self._chief()
        if cache:
            np.savez(_cacheName(runName, "APFModelCache"), theta=self.theta, y=self.y)
        if seed is not None:
            np.random.seed(seed)
        fit = dict(seed=seed, nGPRestarts=nGPRestarts, gpHyperPrior=gpHyperPrior)
        if initGPOpt:
            self.optGP(method=gpMethod, options=gpOptions, p0=gpP0, **fit)
        plateau = _PlateauMonitor(tol, kmax)
        history = {"thetas": [], "vals": [], "thetasMAP": [], "valsMAP": []}
        evaluations = 0
        for iteration in range(nmax):
            if verbose:
                print("Iteration: %d" % iteration)
            # re-fit on every optGPEveryN-th iteration: a period no single call can reach otherwise
            period = 1 if iteration % optGPEveryN == 0 else 99999999
            point, value = self.findNextPoint(computeLnLike=True, cache=cache, gpMethod=gpMethod,
                                              gpOptions=gpOptions, nMinObjRestarts=nMinObjRestarts,
                                              optGPEveryN=period, numNewPoints=perIteration,
                                              minObjMethod=minObjMethod, minObjOptions=minObjOptions,
                                              runName=runName, args=args, verbose=verbose,
                                              nCandidates=nCandidates, deviceCandidates=deviceCandidates,
                                              deviceSearch=deviceSearch, searchJac=searchJac, **batch, **fit,
                                              **kwargs)
            evaluations = (iteration + 1) * perIteration
            if verbose:
                print("Forward model evaluation at: ", point, ", function value: ", value)
            if cache:
                np.savez(_cacheName(runName, "APGP"), gpParamNames=self.gp.get_parameter_names(),
                         gpParamValues=self.gp.get_parameter_vector())
            top = int(np.argmax(self.y))
            history["thetas"].append(self.theta[top])
            history["vals"].append(self.y[top])
            if findMAP:
                mapPoint, mapValue = self.findMAP(theta0=theta0, method=minObjMethod,
                                                  options=minObjOptions, nRestarts=nMinObjRestarts,
                                                  searchJac=searchJac)
                if verbose:
                    print("Current MAP solution: ", mapPoint, mapValue)
                history["thetasMAP"].append(mapPoint)
                history["valsMAP"].append(mapValue)
            if plateau.update(history["vals"][-1]):
                break
        soln = {"thetaBest": history["thetas"][-1], "valBest": history["vals"][-1],
                "thetas": np.asarray(history["thetas"]).squeeze(),
                "vals": np.asarray(history["vals"]).squeeze(), "nev": evaluations}
        if findMAP:
            soln["thetasMAP"] = np.asarray(history["thetasMAP"]).squeeze()
            soln["valsMAP"] = np.asarray(history["valsMAP"]).squeeze()
            top = int(np.argmax(soln["valsMAP"]))
            soln["thetaMAPBest"] = soln["thetasMAP"][top]
            soln["valMAPBest"] = soln["valsMAP"][top]
        return soln
