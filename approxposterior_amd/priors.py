# -*- coding: utf-8 -*-
"""
:py:mod:`priors.py` - prior distributions built from independent factors
------------------------------------------------------------------------

The reference's prior objects (``approxposterior/priors.py``) with the same names,
signatures, defaults and results: :class:`Prior`, :class:`UniformPrior`,
:class:`GaussianPrior` and the list utilities :func:`get_lnprior`,
:func:`get_prior_unit_cube`, :func:`get_theta_bounds`, :func:`get_theta_names`.
Each factor keeps its frozen ``scipy.stats`` distribution as ``.dist`` and draws
from NumPy's global random state, as the reference does.

New here: :class:`JointPrior`, a product of Uniform and Gaussian factors that the
device paths recognise.  Handed to :class:`~approxposterior_amd.approx.ApproxPosterior`
as ``lnprior`` (and ``.sample`` as ``priorSample``), it lets ``runMCMC(onDevice=True)``
run under the prior's support with the log-prior blobs computed on the device, and
``deviceCandidates=True`` draw the ``nCandidates`` matrix from the prior itself
(``GP.prior_candidates``).
"""

import numpy as np
import scipy.stats
from scipy.special import erfcinv

__all__ = ["Prior", "UniformPrior", "GaussianPrior", "JointPrior", "get_lnprior",
           "get_prior_unit_cube", "get_theta_bounds", "get_theta_names"]

_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# per-dimension record kinds of the C ABI (include/apgp.h, apgp_prior_candidates / apgp_prior_lnprior)
KIND_UNIFORM, KIND_GAUSSIAN = 0, 1


class Prior(object):
    """Base class of a one-dimensional prior; ``theta_name`` labels the parameter.

    Calling the object returns :meth:`lnprior`.  The methods a subclass provides
    (``lnprior``, ``random_sample``, ``transform_uniform``, ``get_bounds``) raise
    ``NotImplementedError`` here.  (The reference *returns* the exception object
    instead of raising it; raising makes a missing override fail where it happens.)
    """

    def __init__(self, theta_name=None):
        self.theta_name = theta_name

    def __call__(self, x):
        return self.lnprior(x)

    def __repr__(self):
        # the first two attributes, as the reference prints them: UniformPrior(low=0.000, high=1.000)
        items = list(self.__dict__.items())[:2]
        return "%s(%s)" % (self.__class__.__name__, ", ".join("%s=%.3f" % (k, v) for k, v in items
                                                             if isinstance(v, (int, float, np.number))))

    def __str__(self):
        return self.__repr__()

    def lnprior(self, x):
        raise NotImplementedError("You must specify `lnprior` function in a subclass.")

    def random_sample(self, size=None):
        raise NotImplementedError("You must specify `random_sample` function in a subclass.")

    def transform_uniform(self, r):
        raise NotImplementedError("`transform_uniform` must be specified by a specific subclass.")

    def get_bounds(self):
        raise NotImplementedError("You must specify `get_bounds` in a subclass.")


class UniformPrior(Prior):
    """Uniform density on ``[low, high]``; ``.dist`` is ``scipy.stats.uniform(low, high - low)``."""

    def __init__(self, low, high, **kwargs):
        self.low = low
        self.high = high
        self.dist = scipy.stats.uniform(loc=self.low, scale=self.high - self.low)
        super(UniformPrior, self).__init__(**kwargs)

    def lnprior(self, x):
        """``-log(high - low)`` inside ``[low, high]``, ``-inf`` outside."""
        return self.dist.logpdf(x)

    def random_sample(self, size=None):
        """``size`` draws (a float for ``None``) from NumPy's global random state."""
        return self.dist.rvs(size=size)

    def transform_uniform(self, r):
        """The unit-interval value ``r`` mapped onto ``[low, high]``."""
        return self.low + r * (self.high - self.low)

    def get_bounds(self):
        return (self.low, self.high)


class GaussianPrior(Prior):
    """Normal density with mean ``mu`` and standard deviation ``sigma``; ``.dist`` is
    ``scipy.stats.norm(mu, sigma)``."""

    def __init__(self, mu, sigma, **kwargs):
        self.mu = mu
        self.sigma = sigma
        self.dist = scipy.stats.norm(loc=self.mu, scale=self.sigma)
        super(GaussianPrior, self).__init__(**kwargs)

    def lnprior(self, x):
        return self.dist.logpdf(x)

    def random_sample(self, size=None):
        """``size`` draws (a float for ``None``) from NumPy's global random state."""
        return self.dist.rvs(size=size)

    def transform_uniform(self, r):
        """Inverse CDF at ``r`` in (0, 1): ``mu + sigma sqrt(2) erfcinv(2 (1 - r))``.  The device
        draw (``GP.prior_candidates``) evaluates this expression in this order."""
        return self.mu + self.sigma * np.sqrt(2.0) * erfcinv(2.0 * (1.0 - r))

    def get_bounds(self, Nstd=5.0):
        """``(mu - Nstd sigma, mu + Nstd sigma)``."""
        return (self.dist.mean() - Nstd * self.dist.std(), self.dist.mean() + Nstd * self.dist.std())


def get_lnprior(theta, priors):
    """Sum of ``priors[i].lnprior(theta[i])``."""
    assert len(theta) == len(priors)
    lp = 0.0
    for value, prior in zip(theta, priors):
        lp += prior.lnprior(value)
    return lp


def get_prior_unit_cube(cube, priors):
    """``cube[i]`` (values in (0, 1)) mapped through ``priors[i].transform_uniform``, in place; returns ``cube``."""
    for i, prior in enumerate(priors):
        cube[i] = prior.transform_uniform(cube[i])
    return cube


def get_theta_bounds(priors):
    """One ``get_bounds()`` pair per prior."""
    return [prior.get_bounds() for prior in priors]


def get_theta_names(priors):
    """One ``theta_name`` per prior."""
    return [prior.theta_name for prior in priors]


class JointPrior(object):
    """Product of independent :class:`UniformPrior` (finite ``low < high``) and
    :class:`GaussianPrior` (finite ``mu``, finite ``sigma > 0``) factors, one per
    dimension.  Anything else is refused (``TypeError`` / ``ValueError``).

    * ``prior(theta)``: :func:`get_lnprior` -- pass the object as ``lnprior``;
    * :meth:`batch`: the same for a (W, D) array in closed form (what ``_gpllBatch`` calls);
    * :meth:`sample`: pass as ``priorSample``;
    * :meth:`support`: the axis-aligned box where the density is positive (infinite edges
      for Gaussian factors) -- the gate of the device sampler and of the candidate sweep;
    * :meth:`bounds`: :func:`get_theta_bounds`, for ``ApproxPosterior(bounds=...)``.
    """

    def __init__(self, priors):
        priors = list(priors)
        if not priors:
            raise ValueError("JointPrior needs at least one factor")
        kinds, p0, p1 = [], [], []
        for p in priors:
            if type(p) is UniformPrior:
                lo, hi = float(p.low), float(p.high)
                if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(hi - lo)):
                    raise ValueError("UniformPrior factors need finite low < high, got (%r, %r)" % (p.low, p.high))
                kinds.append(KIND_UNIFORM)
                p0.append(lo)
                p1.append(hi)
            elif type(p) is GaussianPrior:
                mu, sigma = float(p.mu), float(p.sigma)
                if not (np.isfinite(mu) and np.isfinite(sigma) and sigma > 0.0):
                    raise ValueError("GaussianPrior factors need finite mu and sigma > 0, got (%r, %r)" % (p.mu, p.sigma))
                kinds.append(KIND_GAUSSIAN)
                p0.append(mu)
                p1.append(sigma)
            else:
                raise TypeError("JointPrior takes UniformPrior and GaussianPrior factors only, got %s" % type(p).__name__)
        self.priors = priors
        self.kinds = np.array(kinds, dtype=np.int32)
        self.p0 = np.array(p0, dtype=np.float64)
        self.p1 = np.array(p1, dtype=np.float64)

    @property
    def ndim(self):
        return len(self.priors)

    def __len__(self):
        return len(self.priors)

    def __repr__(self):
        return "JointPrior([%s])" % ", ".join(repr(p) for p in self.priors)

    def __call__(self, theta):
        return get_lnprior(theta, self.priors)

    def records(self):
        """``(kind, p0, p1)``: the per-dimension records of the C ABI (int32, float64, float64 arrays of D)."""
        return self.kinds, self.p0, self.p1

    def batch(self, thetas):
        """Log-prior of every row of ``thetas`` (W, D) -> (W,): ``-log(high - low)`` inside a Uniform
        factor's ``[low, high]``, ``-z^2 / 2 - log(sigma) - log(2 pi) / 2`` for a Gaussian one; ``-inf``
        where a coordinate is not finite or lies outside a Uniform factor."""
        x = np.asarray(thetas, dtype=np.float64).reshape(-1, self.ndim)
        uni = self.kinds == KIND_UNIFORM
        lo, hi = self.p0[uni], self.p1[uni]
        mu, sigma = self.p0[~uni], self.p1[~uni]
        with np.errstate(invalid="ignore", over="ignore"):
            z = (x[:, ~uni] - mu) / sigma
            out = -np.sum(np.log(hi - lo)) + np.sum(-0.5 * z * z - np.log(sigma) - _HALF_LOG_2PI, axis=1)
            inside = np.all(np.isfinite(x), axis=1) & np.all((x[:, uni] >= lo) & (x[:, uni] <= hi), axis=1)
        return np.where(inside, out, -np.inf)

    def sample(self, n):
        """(n, D) draws, column d from factor d: ``np.vstack([p.random_sample(n) for p in priors]).T``."""
        return np.vstack([p.random_sample(n) for p in self.priors]).T

    def support(self):
        """(D, 2): ``(low, high)`` for Uniform factors, ``(-inf, inf)`` for Gaussian ones."""
        out = np.empty((self.ndim, 2))
        uni = self.kinds == KIND_UNIFORM
        out[:, 0] = np.where(uni, self.p0, -np.inf)
        out[:, 1] = np.where(uni, self.p1, np.inf)
        return out

    def bounds(self):
        """:func:`get_theta_bounds` of the factors (Gaussian: mu +- 5 sigma)."""
        return get_theta_bounds(self.priors)
