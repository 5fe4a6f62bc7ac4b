# -*- coding: utf-8 -*-
"""
:py:mod:`gp.py` - MI355X-backed drop-in for the ``george.GP`` members that
approxposterior touches
--------------------------------------------------------------------------------

The reference (dflemin3/approxposterior) has no plugin/FFI interface: its seam is
the duck-typed ``george.GP`` instance passed as ``gp=`` (approx.py:77,140-144)
and re-created at approx.py:712-715.  This module provides objects exposing
exactly the members the reference calls:

  ``kernels.ExpSquaredKernel(metric, ndim)``, ``float * kernel``   gpUtils.py:160-165
  ``GP(kernel, fit_mean, mean, white_noise, fit_white_noise)``     gpUtils.py:176-177
  ``gp.compute(x)`` / ``gp.recompute()``                           gpUtils.py:178,244,254
  ``set/get_parameter_vector``, ``get_parameter_names``, ``len``   gpUtils.py:74,227,243
  ``gp.log_likelihood(y, quiet=True)``                             gpUtils.py:78,247
  ``gp.grad_log_likelihood(y, quiet=True)``                        gpUtils.py:110
  ``gp.predict(y, t, return_var=True)`` / mean only                utility.py:131; approx.py:178
  ``gp.computed``, ``gp.kernel``, ``gp.mean``, ``gp.white_noise``  utility.py:130; approx.py:712-714

All arithmetic -- including the blocked Cholesky factorisation (csrc/potrf.hip)
-- runs in the hand-written HIP kernels of ``libapgp.so`` (include/apgp.h) on one
MI355X.  PyTorch is only the device allocator / stream provider.  There is no
CPU fallback: without a GPU or without the built extension every compute entry
point raises.

Beyond george's API the GP also offers the batched counterparts the reference
lacks: ``acquire`` (fused predict + utility + arg-min over a candidate matrix)
and array-valued ``predict``.
"""

import collections
import ctypes
import math
from operator import is_

import numpy as np
from numpy.linalg import LinAlgError
from scipy.linalg import solve_triangular

from . import _lib
from .george_extras import GeorgeExtras

__all__ = ["GP", "ExpSquaredKernel", "ConstantKernel", "Product", "ConstantModel",
           "kernels", "UTILITY_KINDS", "sobolSample"]

UTILITY_KINDS = {"agp": _lib.UTIL_AGP, "bape": _lib.UTIL_BAPE, "jones": _lib.UTIL_JONES}
# objectives of the device point search (GP.nelder_mead_search): the utilities and -mu (ApproxPosterior.findMAP)
SEARCH_KINDS = dict(UTILITY_KINDS, negmean=_lib.UTIL_NEG_MEAN)
NM_OPTIONS = ("adaptive", "maxiter", "maxfev", "xatol", "fatol")


def nm_coefficients(ndim, adaptive):
    """(rho, chi, psi, sigma) of SciPy's Nelder-Mead, computed as SciPy 1.15 computes them (same bits)."""
    if adaptive:
        dim = float(ndim)
        return 1.0, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1.0, 2.0, 0.5, 0.5


def nm_limits(ndim, maxiter=None, maxfev=None):
    """SciPy's (maxiter, maxfev) defaults (N * 200 when neither is given; the other one unbounded when one is).  An
    unbounded maxfev becomes the most evaluations ``maxiter`` iterations can make (N + 1, then at most N + 2 per
    iteration), an unbounded maxiter the most iterations ``maxfev`` evaluations allow: the search stops where SciPy's
    does."""
    if maxiter is None and maxfev is None:
        maxiter = maxfev = ndim * 200
    elif maxiter is None:
        maxiter = ndim * 200 if maxfev == np.inf else np.inf
    elif maxfev is None:
        maxfev = ndim * 200 if maxiter == np.inf else np.inf
    if maxfev == np.inf:
        maxfev = (ndim + 1) + (int(maxiter) - 1) * (ndim + 2)
    if maxiter == np.inf:
        maxiter = int(maxfev)
    return int(maxiter), int(maxfev)


class _NullContext(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL_CONTEXT = _NullContext()

# Above this condition estimate ((max L_ii / min L_ii)^2) the explicit L^-1
# contraction is no longer trusted for the predictive variance (SURVEY.md
# section 7, "Conditioning vs. formulation") and the solve-based sweep
# (apgp_acquire_solve) is used instead.  ``GP.variance_mode`` = "solve" | "inverse"
# overrides the choice for one object (tests); no environment variable is read.
COND_SOLVE = 1.0e10
# from this size on a missing L^-1 is formed before the solves WHEN ALPHA IS WANTED (a sweep, a gradient or the
# sampler follows -- they need W anyway): apgp_trtri_pack + two matrix-vector products, 0.11 + 0.02 ms at N = 512
# against 0.08 + 0.09 ms for the two triangular solves, 0.82 + 0.05 ms against 2 x 0.72 ms at N = 4096
# (profiles/r03n_fit_timing.txt).  A bare log_likelihood on a new y keeps the single forward solve.
W_FIRST_MIN_N = 512
_LOG_2PI = np.log(2.0 * np.pi)
_F64 = np.dtype(np.float64)     # (a dtype compares with a dtype faster than with a type: replay guards)


# ---------------------------------------------------------------------------
# Host-side parameter objects (no arithmetic lives here)
# ---------------------------------------------------------------------------

class ConstantModel(object):
    """Mirror of george.modeling.ConstantModel (``gp.mean``, ``gp.white_noise``)."""

    def __init__(self, value):
        self.value = float(value)

    def get_value(self, x):
        return self.value + np.zeros(len(x))

    def __len__(self):
        return 1

    def __repr__(self):
        return "ConstantModel(value=%r)" % self.value


def _as_model(obj, default):
    if obj is None:
        return ConstantModel(default)
    if isinstance(obj, ConstantModel) or (hasattr(obj, "value") and hasattr(obj, "get_value")):
        return obj
    return ConstantModel(float(obj))


class Kernel(object):
    is_kernel = True
    ndim = 1

    def __rmul__(self, b):
        # george: ``c * kernel`` -> Product(ConstantKernel(log(c/ndim)), kernel);
        # the constant kernel evaluates to ndim*exp(log_constant) = c
        # (gpUtils.py:165; pinned by test_InitGP.py:43 + test_GPUtil.py:50-62).
        if hasattr(b, "is_kernel"):
            return Product(b, self)
        return Product(ConstantKernel(log_constant=np.log(float(b) / self.ndim),
                                      ndim=self.ndim), self)

    __mul__ = __rmul__

    def __add__(self, other):
        # george: ``kernel + other`` -> Sum(kernel, other) (gpUtils.py:170, the optional
        # linear-regression term of defaultGP(order=...))
        if not hasattr(other, "is_kernel"):
            raise NotImplementedError("only kernel + kernel sums are on the MI355X hot path")
        return Sum(self, other)

    def __radd__(self, other):
        if not hasattr(other, "is_kernel"):
            raise NotImplementedError("only kernel + kernel sums are on the MI355X hot path")
        return Sum(other, self)

    def __len__(self):
        return len(self.get_parameter_vector())


class ConstantKernel(Kernel):
    def __init__(self, log_constant, ndim=1):
        self.log_constant = float(log_constant)
        self.ndim = int(ndim)
        self.dirty = True

    def get_parameter_names(self):
        return ("log_constant",)

    def get_parameter_vector(self):
        return np.array([self.log_constant])

    def set_parameter_vector(self, v):
        self.log_constant = float(v[0])
        self.dirty = True

    def __len__(self):
        return 1


class ExpSquaredKernel(Kernel):
    """k(x,x') = exp(-0.5 sum_d (x_d-x'_d)^2 / M_d); parameters are log M_d."""

    def __init__(self, metric, ndim=1):
        self.ndim = int(ndim)
        metric = np.atleast_1d(np.asarray(metric, dtype=np.float64))
        if metric.size == 1 and self.ndim > 1:
            metric = np.full(self.ndim, float(metric[0]))
        if metric.size != self.ndim:
            raise ValueError("Dimension mismatch")
        self.log_M = np.log(metric)
        self.dirty = True

    def get_parameter_names(self):
        return tuple("metric:log_M_%d_%d" % (d, d) for d in range(self.ndim))

    def get_parameter_vector(self):
        return np.array(self.log_M)

    def set_parameter_vector(self, v):
        self.log_M = np.array(v, dtype=np.float64)
        self.dirty = True

    def __len__(self):
        return len(self.log_M)


class LinearKernel(Kernel):
    """george.kernels.LinearKernel(log_gamma2, order, ndim) (gpUtils.py:170-173):
    k(x,x') = sum_d (x_d x'_d)^P / gamma^2 with the per-axis sum george uses for its
    non-stationary kernels; ``order`` P is a constant, ``log_gamma2`` the
    only parameter.  No reference test pins it ("parity unpinned"); P must be an integer
    >= 0 here."""

    def __init__(self, log_gamma2=None, order=None, bounds=None, ndim=1, axes=None):
        if log_gamma2 is None or order is None:
            raise ValueError("log_gamma2 and order are required")
        if axes is not None:
            raise NotImplementedError("axes subsets are not on the MI355X hot path")
        if int(order) != order or order < 0 or order > 16:
            raise NotImplementedError("LinearKernel order must be an integer in [0, 16] on the device path")
        self.log_gamma2 = float(log_gamma2)
        self.order = int(order)
        self.ndim = int(ndim)
        self.dirty = True

    def get_parameter_names(self):
        return ("log_gamma2",)

    def get_parameter_vector(self):
        return np.array([self.log_gamma2])

    def set_parameter_vector(self, v):
        self.log_gamma2 = float(v[0])
        self.dirty = True

    def __len__(self):
        return 1


class Product(Kernel):
    def __init__(self, k1, k2):
        self.k1 = k1
        self.k2 = k2
        self.ndim = k2.ndim

    @property
    def dirty(self):
        return self.k1.dirty or self.k2.dirty

    @dirty.setter
    def dirty(self, v):
        self.k1.dirty = v
        self.k2.dirty = v

    def get_parameter_names(self):
        return tuple(["k1:" + n for n in self.k1.get_parameter_names()] +
                     ["k2:" + n for n in self.k2.get_parameter_names()])

    def get_parameter_vector(self):
        return np.concatenate([self.k1.get_parameter_vector(),
                               self.k2.get_parameter_vector()])

    def set_parameter_vector(self, v):
        n1 = len(self.k1)
        self.k1.set_parameter_vector(v[:n1])
        self.k2.set_parameter_vector(v[n1:])

    def __len__(self):
        return len(self.k1) + len(self.k2)


class Sum(Product):
    """george.kernels.Sum: same parameter protocol as Product (k1:..., k2:...)."""


class _KernelsNamespace(object):
    """Stands in for ``george.kernels``."""
    ExpSquaredKernel = ExpSquaredKernel
    ConstantKernel = ConstantKernel
    LinearKernel = LinearKernel
    Product = Product
    Sum = Sum


kernels = _KernelsNamespace()


def _flatten_term(kernel):
    """One additive term: (constant factor, ExpSquaredKernel or None, LinearKernel or None)."""
    amp, se, lin = 1.0, None, None
    stack = [kernel]
    while stack:
        k = stack.pop()
        if isinstance(k, Sum):
            raise NotImplementedError("nested kernel sums are not on the MI355X hot path")
        if isinstance(k, Product):
            stack += [k.k1, k.k2]
        elif isinstance(k, ConstantKernel):
            amp *= k.ndim * np.exp(k.log_constant)
        elif isinstance(k, ExpSquaredKernel):
            if se is not None or lin is not None:
                raise NotImplementedError("product of two non-constant kernels")
            se = k
        elif isinstance(k, LinearKernel):
            if se is not None or lin is not None:
                raise NotImplementedError("product of two non-constant kernels")
            lin = k
        else:
            raise NotImplementedError("kernel type %r is not on the MI355X hot path" % type(k))
    return float(amp), se, lin


def _flatten_kernel(kernel, with_linear=False):
    """(amp, log_M) of an ExpSquared kernel, optionally times constants; with
    ``with_linear`` also (lin_coef, lin_order) of an added [constant *] LinearKernel
    (``kernel + c * LinearKernel``, gpUtils.py:170-173), (0.0, 0) if there is none."""
    # the two shapes gpUtils.defaultGP builds without a linear term (gpUtils.py:160-165), without the generic walk:
    # this runs once per objective evaluation of an optimiser loop
    tk = type(kernel)
    if tk is ExpSquaredKernel:
        return (1.0, kernel.log_M, 0.0, 0) if with_linear else (1.0, kernel.log_M)
    if tk is Product and type(kernel.k1) is ConstantKernel and type(kernel.k2) is ExpSquaredKernel:
        amp = float(kernel.k1.ndim * np.exp(kernel.k1.log_constant))
        return (amp, kernel.k2.log_M, 0.0, 0) if with_linear else (amp, kernel.k2.log_M)
    terms = [kernel.k1, kernel.k2] if isinstance(kernel, Sum) else [kernel]
    amp = log_M = None
    lin_coef, lin_order = 0.0, 0
    for term in terms:
        c, se, lin = _flatten_term(term)
        if se is not None:
            if amp is not None:
                raise NotImplementedError("sum of two ExpSquaredKernel terms")
            amp, log_M = c, np.asarray(se.log_M, dtype=np.float64)
        elif lin is not None:
            if lin_coef != 0.0:
                raise NotImplementedError("sum of two LinearKernel terms")
            lin_coef, lin_order = c * float(np.exp(-lin.log_gamma2)), lin.order
        else:
            raise NotImplementedError("a purely constant kernel term is not on the MI355X hot path")
    if amp is None:
        raise NotImplementedError("an ExpSquaredKernel term is required")
    if with_linear:
        return amp, log_M, float(lin_coef), int(lin_order)
    return amp, log_M


class _Replay(object):
    """One library call kept for the next call that differs only in the per-call slots of ``args`` (the caller fills
    them in): what a hot loop saves by skipping the generic path's checks and set-up.  It applies while the device and
    current stream it was built on are current, ``y`` has the bytes it was built for and every object of ``deps`` --
    the buffers the arguments point into -- is still the GP's own.  ``data``: what the call site keeps with it (its host
    arrays, its own limits)."""
    __slots__ = ("fn", "args", "data", "device", "stream", "ybytes", "n", "deps", "current_device", "raw_stream")

    def __init__(self, fn, args, device, stream, y, deps, queries, data=None):
        self.fn, self.args, self.data = fn, args, data
        self.device, self.stream = device, stream
        self.ybytes, self.n = y.tobytes(), y.size
        self.deps = deps
        self.current_device, self.raw_stream = queries     # () -> device index, (index) -> raw stream handle

    def fits(self, y, deps):
        if not all(map(is_, deps, self.deps)):
            return False
        if type(y) is not np.ndarray or y.dtype != _F64 or y.size != self.n or not y.flags.c_contiguous:
            return False
        cur = self.current_device()
        if cur != self.device or self.raw_stream is None or self.raw_stream(cur) != self.stream:
            return False
        return y.tobytes() == self.ybytes


def _box(bounds, D, optional=True):
    """The box ``bounds`` (a low and a high edge for each dimension) as the C ABI's two ``double[MAX_DIM]``; (None, None) for no
    box where the call can do without one."""
    if bounds is None and optional:
        return None, None
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    if len(b) != D:
        raise ValueError("bounds must have one (lo, hi) pair per dimension")
    arr = ctypes.c_double * _lib.MAX_DIM
    return arr(*b[:, 0]), arr(*b[:, 1])


def _triu_colmajor(D):
    """(rows, cols) of the upper triangle packed column by column: U[i][j] at j(j+1)/2 + i (include/apgp.h)."""
    j = np.repeat(np.arange(D), np.arange(1, D + 1))
    i = np.concatenate([np.arange(c + 1) for c in range(D)])
    return i, j


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _ptr(tensor):
    return None if tensor is None else tensor.data_ptr()


def _best_record(best):
    """(index, utility) of the sweep's 16-byte ``apgp_best_t`` record ``best`` (device): one copy to the host."""
    bb = best.cpu().numpy()
    return int(bb[1:2].view(np.int64)[0]), float(bb[0])


# what one sweep left on the device: the arg-min record and the per-candidate arrays that were asked for (else None)
_Swept = collections.namedtuple("_Swept", "best mu var u")

# nll_batch's work space, kept between the rounds of a fit on one training set, y and stream: the device copy of y, the
# (K, z, info, record) buffers of each batch size up to 256 MB, the means of a replayed batch
_BatchWork = collections.namedtuple("_BatchWork", "x x_d stream ybytes y_d bufs means")


def _records_nll(o, n):
    """-log-likelihood of each factorisation record (B x 5: log-determinant, min / max L_ii, z.z, info) by the element
    operations of ``log_likelihood``, in its order; +inf where the factorisation failed or the value is not finite."""
    with np.errstate(all="ignore"):
        ll = (-0.5 * (n * _LOG_2PI + o[:, 0])) - 0.5 * o[:, 3]
    bad = (o[:, 4] != 0.0) | ~np.isfinite(o[:, 0]) | ~np.isfinite(ll)
    return np.where(bad, np.inf, -ll)


class PathDraws(object):
    """``size`` functions drawn from a GP's posterior (:meth:`GP.sample_paths`): the random features ``Z``, ``b``, their
    weights ``W``, ``Wl`` and the data weights ``V`` on the device, with the kernel struct ``ks`` and the mean they were
    drawn for.  It belongs to the factor it was solved against: after the GP's training set, hyper-parameters or mean
    changed, :meth:`evaluate` and :meth:`argmax` raise."""

    def __init__(self, gp, Z, b, W, Wl):
        self.gp, self.Z, self.b, self.W, self.Wl, self.V = gp, Z, b, W, Wl, None
        self.size, self.nFeatures = int(W.shape[0]), int(W.shape[1])
        if Z.shape != (self.nFeatures, gp.kernel.ndim) or b.shape != (self.nFeatures,) \
                or Wl.shape != (self.size, gp.kernel.ndim):
            raise ValueError("Z (R, D), b (R,), W (S, R) and Wl (S, D) do not fit together")
        self.ks = gp._kernel_struct()
        self.mean = float(gp.mean.value)
        self._key, self._x = (gp._factor_key(), self.mean), gp._x

    def _check_current(self):
        gp = self.gp
        if not gp.computed or gp._x is not self._x or (gp._factor_key(), float(gp.mean.value)) != self._key:
            raise RuntimeError("these draws belong to a factor the GP no longer holds: call sample_paths again")

    def _call(self, t, bounds, mask, idx_offset, with_f):
        gp = self.gp
        self._check_current()
        lo, hi = _box(bounds, gp.kernel.ndim)
        T = gp._candidates(t)
        mask_d = mask if hasattr(mask, "data_ptr") else gp._mask(mask, T.shape[0])
        if mask_d is not None and (tuple(mask_d.shape) != (T.shape[0],) or str(mask_d.dtype) != "torch.uint8"):
            raise ValueError("a device mask must be a (M,) uint8 tensor")
        if T.shape[0] == 0:
            return np.empty((self.size, 0)), np.full(self.size, -1, dtype=np.int64), np.full(self.size, np.inf)
        return gp._path_call(T, self.ks, self.mean, self, self.V, lo, hi, mask_d, idx_offset, with_f)

    def evaluate(self, t):
        """f_s(t) at the points ``t`` (M, D; host array or device tensor) as an (S, M) array."""
        F = self._call(t, None, None, 0, True)[0]
        return F if isinstance(F, np.ndarray) else F.cpu().numpy()

    def argmax(self, t, bounds=None, mask=None, idx_offset=0):
        """Each draw's arg-max over the admissible rows of ``t``: (global indices (S,), values (S,)).  The sweep's
        contract: the lowest index on ties, NaN never wins, a row outside ``bounds``, with ``mask == 0`` or with a
        NaN coordinate is inadmissible; index -1 and -inf where no row is admissible."""
        _, idx, u = self._call(t, bounds, mask, idx_offset, False)
        return idx, -u


# ---------------------------------------------------------------------------
# GP
# ---------------------------------------------------------------------------

class GP(GeorgeExtras):
    """``george.GP``-shaped object whose arithmetic runs on one MI355X.  (The members of ``george.GP`` the reference
    never calls -- ``apply_inverse``, ``get_matrix``, ``predict``'s covariance form, the ``nll`` aliases -- live in
    :py:mod:`approxposterior_amd.george_extras`, off the hot path.)"""

    def __init__(self, kernel=None, fit_kernel=True, mean=None, fit_mean=None,
                 white_noise=None, fit_white_noise=None, solver=None, device=None,
                 **kwargs):
        if kernel is None:
            raise ValueError("a kernel is required")
        self.kernel = kernel
        self.mean = _as_model(mean, 0.0)
        self.white_noise = _as_model(white_noise, np.log(1.25e-12))
        self.fit_mean = bool(fit_mean)
        self.fit_white_noise = bool(fit_white_noise)
        self._device_arg = device
        self.variance_mode = None     # None: by condition estimate; "solve" / "inverse": forced
        self.extend_max_rows = None   # rows compute(x, previous=...) may append before it refactorises (None: by cost)
        # arg-min-only sweeps skip candidate blocks that cannot win (apgp_set_sweep_prune): None: the library's
        # process-wide setting (default on); False / 0: the full sweep; True / 1: on; >= 2: on from that many candidates
        self.sweep_prune = None
        # the pruned sweep's seed launch sends the 256-row blocks of W from this one on as two 128-row workgroups each
        # (apgp_set_seed_rowsplit; same bits whatever the value): None: the library's process-wide setting (default:
        # its rule); -1: the rule; 0: every row block; >= ceil(n / 256): none
        self.seed_rowsplit = None
        # the same launch reads its blocks' k* from a stream generated once per call instead of generating it in every
        # workgroup (apgp_set_seed_park; same bits either way): None: the library's process-wide setting (default: on);
        # True / 1: on; False / 0: off
        self.seed_park = None
        # that launch's row-part workgroups request their re-read tiles up to this many tiles ahead, through a ring of
        # stages in LDS (apgp_set_seed_prefetch; same bits whatever the value): None: the library's process-wide setting
        # (default: 6, as far as the ring of the part size holds); 0: one tile ahead, the launch as it was
        self.seed_prefetch = None
        # the 16 seed blocks go in two waves, the first seed_first of them and then those of the rest that could still
        # win (apgp_set_seed_first; same winner whatever the value): None: the library's process-wide setting (default:
        # its rule, 4 where the parked seed route applies); -1: the rule; 1 .. 16: that many (16: one wave)
        self.seed_first = None
        # sub-block pairs (32 rows) per workgroup of a split row block of the seed launches (apgp_set_seed_parts; same
        # bits whatever the value): None: the library's process-wide setting (default: its rule); -1: the rule; 8 / 4 / 2 / 1
        self.seed_parts = None
        # the coarse bound of the pruned sweep reads the fit's rows sorted by alpha's sign and runs one sum chain per
        # kernel value (apgp_pack_prune_srows; same winner either way, the bounds differ in their last bits):
        # True (default): that route; False: the rows in their own order, two chains (the route of _prune_rows)
        self.prune_signed = True
        # that route's bound kernel runs its row loop in a pinned, pipelined order of issue (apgp_set_prune_pipe; same
        # bits either way): None: the library's process-wide setting (default: on); True / 1: on; False / 0: off
        self.prune_pipe = None
        self.sweep_prune_stats = False   # True: keep (seed blocks, surviving blocks, bits of tau, blocks the coarse
        self.last_prune_counts = None     # bound left, second-wave seeds swept) of the last pruned sweep here, as a
                                          # device int64[5] tensor
        self._computed = False
        self._x = None
        self._yerr2 = 0.0
        self._nllMemo = None          # gpUtils._nll: values already evaluated on this training set
        self._rt_cache = None         # (torch, device, lib), see _rt
        self._queries = None          # (current device, raw current stream) queries of torch, see _rt
        self._x_d = None              # device copy of the training set
        self._mean_work = None        # scratch of the small predictions and of the evaluations: survives refits
        self._p1_work = None
        self._imp_work = None         # scratch of importance_pass
        self._pimp_work = None        # scratch of importance_paths
        self._pg_work = None
        self._nll_scratch = None
        self._nll_stream = None       # the stream the private buffers of the last _nll evaluation were made on
        self._batch = None            # nll_batch's _BatchWork
        # The previous call's argument list of the hot loops, ready for the next (_Replay): "nll" (the optimiser's
        # evaluations), "one" (a candidate with variance), "mean" (a few points, mean only), "pgrad" (a point with its
        # gradients) belong to the factor and go with it; ("batch", B) belongs to self._batch and goes with that.
        self._replays = {}
        self._reset_device_state()

    # -- device plumbing -------------------------------------------------------
    def _reset_device_state(self):
        self._L = None            # (N,N) lower Cholesky factor (device); a view of _L_store["buf"] after appends
        self._L_store = None      # growable store shared along a chain of appended GPs (compute(previous=))
        self._ld = None           # leading dimension of _L in memory
        self._nll_owned = False   # _L / _z are private buffers of an _nll evaluation (reusable by the next)
        self._alpha_y = None      # host copy of the y alpha/z were computed for
        self._alpha_mean = None
        self._y_d = None
        self._ztz_host = None
        self._z = None
        self._alpha = None
        self._packed = None       # packed L^-1 tiles
        self._packed_solve = None  # packed tiles of the substitution form (apgp_pack_lsolve)
        self._work = None         # trtri work (dense L^-1 in first panel)
        self._xs = None           # packed training stream (depends on alpha)
        self._prune_rows = None   # its rows split for the coarse prune bound (apgp_pack_prune_rows); lives and dies with _xs
        self._prune_srows = None  # the same rows sorted by alpha's sign (apgp_pack_prune_srows); lives and dies with _xs
        self._xs_key = None
        for key in ("nll", "one", "mean", "pgrad"):
            self._replays.pop(key, None)
        self.cond_estimate = None
        self.log_determinant = None

    def _rt(self):
        """(torch, device, lib) -- fails loudly without GPU / extension."""
        if self._rt_cache is not None:
            return self._rt_cache
        import torch
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.ApgpError("no MI355X visible: approxposterior_amd has no CPU fallback")
        dev = self._device_arg
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        elif not isinstance(dev, torch.device):
            dev = torch.device(dev)
        self._queries = (torch.cuda.current_device, getattr(torch._C, "_cuda_getCurrentRawStream", None))
        self._rt_cache = (torch, dev, lib)
        return self._rt_cache

    @staticmethod
    def _on(torch, dev):
        """Context that makes ``dev`` current -- a no-op object when it already is (the context manager of
        torch.cuda.device costs ~4 us, on the per-evaluation path of gpUtils._nll)."""
        if torch.cuda.current_device() == dev.index:
            return _NULL_CONTEXT
        return torch.cuda.device(dev)

    @staticmethod
    def _stream(torch):
        # the raw-handle query is ~30x cheaper than torch.cuda.current_stream() and this
        # sits on the per-call path of the sampler's log-probability
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return ctypes.c_void_p(raw(torch.cuda.current_device()))
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _kernel_struct(self, ks=None):
        """The kernel's hyper-parameters as the C ABI's struct (``ks``: refilled in place)."""
        amp, log_M, lin_coef, lin_order = _flatten_kernel(self.kernel, with_linear=True)
        if ks is None:
            ks = _lib.KernelStruct()
        elif ks.ndim != len(log_M):
            raise ValueError("dimension mismatch")
        ks.ndim = len(log_M)
        ks.amp = amp
        ks.lin_coef = lin_coef
        ks.lin_order = lin_order
        ks.diag_add = float(self._yerr2) + float(np.exp(self.white_noise.value))
        ks.inv_metric[:len(log_M)] = np.exp(-np.asarray(log_M, dtype=np.float64)).tolist()   # (the rest stays 0)
        return ks

    # -- parameter-vector protocol (george) -------------
    def get_parameter_names(self):
        names = []
        if self.fit_mean:
            names.append("mean:value")
        if self.fit_white_noise:
            names.append("white_noise:value")
        names += ["kernel:" + n for n in self.kernel.get_parameter_names()]
        return tuple(names)

    def get_parameter_vector(self):
        v = []
        if self.fit_mean:
            v.append(self.mean.value)
        if self.fit_white_noise:
            v.append(self.white_noise.value)
        return np.concatenate([np.array(v, dtype=np.float64),
                               self.kernel.get_parameter_vector()])

    def set_parameter_vector(self, p):
        p = np.asarray(p, dtype=np.float64).ravel()
        if len(p) != len(self):
            raise ValueError("dimension mismatch")
        n = 0
        if self.fit_mean:
            self.mean.value = float(p[n]); n += 1
        if self.fit_white_noise:
            self.white_noise.value = float(p[n]); n += 1
        self.kernel.set_parameter_vector(p[n:])
        self.kernel.dirty = True   # marks dirty; no compute (george semantics)

    def __len__(self):
        return int(self.fit_mean) + int(self.fit_white_noise) + len(self.kernel)

    @property
    def computed(self):
        return self._computed and not self.kernel.dirty

    # -- helpers -----------------------------------------------------------------
    def parse_samples(self, t):
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        if t.ndim == 1:
            t = t[:, None]
        if t.ndim != 2 or t.shape[1] != self.kernel.ndim:
            raise ValueError("Dimension mismatch")
        return np.ascontiguousarray(t)

    def _check_dimensions(self, y):
        y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        if self._x is None or y.shape[0] != len(self._x):
            raise ValueError("Dimension mismatch")
        return np.ascontiguousarray(y)

    # -- compute / recompute: K1 gram + blocked Cholesky (+ fused forward solve) + K2 ------
    def compute(self, x, yerr=0.0, previous=None, **kwargs):
        """george GP.compute.  ``previous`` (extension): a GP factorised with the
        same hyper-parameters on a training set that is a PREFIX of ``x`` -- what
        ApproxPosterior.findNextPoint has at hand when it appends a design point
        (approx.py:693-717).  The factor is then extended row by row in O(N^2) per
        new point instead of refactorised in O(N^3)."""
        x_in = x
        x = self.parse_samples(x)
        if x.shape[1] > _lib.MAX_DIM:
            raise ValueError("approxposterior_amd supports at most %d input dimensions (APGP_MAX_DIM in include/apgp.h: the "
                             "kernels keep a point's coordinates in registers); got %d" % (_lib.MAX_DIM, x.shape[1]))
        if not np.isfinite(x).all():
            # george: scipy's cholesky refuses the NaN Gram matrix a non-finite coordinate gives (ValueError).  Here the
            # kernels' exp clamps its argument, NaN included, to -700: K would come out finite and factorise
            raise ValueError("array must not contain infs or NaNs")
        if x is x_in or (isinstance(x_in, np.ndarray) and np.shares_memory(x, x_in)):
            x = x.copy()              # the object owns its training set: a caller who edits x in place afterwards is not seen
        same_x = self._x is not None and self._x.shape == x.shape and np.array_equal(self._x, x)
        self._x = x
        self._nllMemo = None          # gpUtils._nll's table of evaluated points belongs to the old training set
        self._yerr2 = float(yerr) ** 2
        if previous is not None and self._try_extend(previous):
            return
        self._factor(None, upload_x=not same_x)

    def _trust_inverse(self):
        """True when the explicit L^-1 (sweep contraction, alpha by matrix-vector products, row
        appends) may stand in for triangular solves: forced by ``variance_mode``, otherwise by the
        condition estimate against COND_SOLVE."""
        mode = (self.variance_mode or "").lower()
        if mode == "inverse":
            return True
        if mode == "solve":
            return False
        return self.cond_estimate is not None and self.cond_estimate <= COND_SOLVE

    def _factor_key(self):
        """What the factor depends on: the bytes of the C ABI's kernel struct (amplitude, inverse metric, linear term,
        white noise + yerr^2) -- the mean is not part of it."""
        return bytes(self._kernel_struct())

    def _try_extend(self, prev):
        """Extend ``prev``'s Cholesky factor by the rows of self._x it does not cover:
        l = L^-1 k(x_new, X_old), d = sqrt(k(x_new,x_new) + diag_add - l.l)."""
        if getattr(prev, "_L", None) is None or getattr(prev, "_x", None) is None:
            return False
        if getattr(prev, "_factored_key", None) != self._factor_key():
            return False
        n0, n1 = len(prev._x), len(self._x)
        # one appended row costs a triangular solve (0.40 us per row of N) and the whole Cholesky
        # 0.47 us per row of N + 30 us: beyond one row (two below N = 512) the
        # refactorisation is the faster way.  ``extend_max_rows`` overrides the rule (up to 64).
        limit = self.extend_max_rows if self.extend_max_rows is not None else (1 if n1 >= 512 else 2)
        if not (0 < n0 < n1 and n1 - n0 <= min(64, int(limit)) and prev._x.shape[1] == self._x.shape[1]
                and np.array_equal(prev._x, self._x[:n0])):
            return False
        torch, dev, lib = self._rt()
        ks = self._kernel_struct()
        w_prev = None
        if getattr(prev, "_work", None) is not None and prev._trust_inverse():
            w_prev = prev._work
        prev_L, prev_store = prev._L, getattr(prev, "_L_store", None)
        self._reset_device_state()
        self._computed = False
        with self._on(torch, dev):
            st = self._stream(torch)
            self._x_d = torch.from_numpy(self._x).to(dev)
            # The factor lives in a growable store shared along the chain of GP objects findNextPoint
            # creates (approx.py:712-717: a new GP per appended point): rows are appended IN PLACE while
            # the store has room and nobody else has appended to it (``used`` == the previous size: a
            # second child of the same parent gets its own copy); otherwise a 1.5x larger zeroed store
            # is allocated and the old factor copied once -- not an n x n allocation + copy per point.
            if prev_store is not None and prev_store["used"] == n0 and prev_store["buf"].shape[0] >= n1:
                store = prev_store
            else:
                cap = ((max(n1 + 63, int(1.5 * n1)) + 63) // 64) * 64
                store = {"buf": torch.zeros((cap, cap), dtype=torch.float64, device=dev), "used": n0}
                store["buf"][:n0, :n0].copy_(prev_L[:n0, :n0])
            buf = store["buf"]
            ld = buf.shape[1]
            L = buf[:n1, :n1]
            row = torch.empty(n1, dtype=torch.float64, device=dev)
            ss = torch.empty(1, dtype=torch.float64, device=dev)
            info = torch.zeros(1, dtype=torch.int32, device=dev)
            for j in range(n0, n1):
                # row j: l = L^-1 k(x_j, X[:j]), pivot sqrt(k(x_j,x_j) + diag_add - l.l) -- all enqueued,
                # no host round trip per row (a failed pivot is reported through `info`)
                _lib.check(lib.apgp_kernel_cross(self._x_d[j:].data_ptr(), 1, self._x_d.data_ptr(), j,
                                                 ctypes.byref(ks), row.data_ptr(), n1, st), "apgp_kernel_cross")
                if j == n0 and w_prev is not None:
                    # the previous fit's dense L^-1 is resident (a sweep ran on it): l = W k is an
                    # HBM-rate matrix-vector product (18 us at N = 4096; the solve: 0.7 ms)
                    _lib.check(lib.apgp_winv_apply(w_prev.data_ptr(), (n0 + 63) // 64 * 64, n0, row.data_ptr(), 0.0,
                                                   0, L[j].data_ptr(), ss.data_ptr(), None, st),
                               "apgp_winv_apply(append)")
                else:
                    _lib.check(lib.apgp_trsv(L.data_ptr(), j, ld, row.data_ptr(), 0.0, 0, L[j].data_ptr(),
                                             ss.data_ptr(), st), "apgp_trsv(append)")
                kxx = ks.amp            # k(x_new, x_new): amplitude + the linear term's sum_d (x_d^2)^P
                if ks.lin_coef != 0.0:
                    kxx += ks.lin_coef * float(np.sum((self._x[j] * self._x[j]) ** ks.lin_order))
                _lib.check(lib.apgp_append_diag(L[j, j:].data_ptr(), ss.data_ptr(), kxx + ks.diag_add,
                                                info.data_ptr(), j + 1, st), "apgp_append_diag")
            store["used"] = n1
            out5 = torch.empty(5, dtype=torch.float64, device=dev)
            _lib.check(lib.apgp_fit_summary(L.data_ptr(), n1, ld, None, info.data_ptr(), out5.data_ptr(), st),
                       "apgp_fit_summary")
            o = out5.cpu().numpy()          # the only synchronisation of the extension
        try:
            self._take_record(o, n1, bytes(ks))
        except LinAlgError:
            store["used"] = -1            # (the failed rows stay in the store: nobody may append to it again)
            self._reset_device_state()
            raise
        self._L = L
        self._L_store = store
        self._ld = ld
        return True

    def _take_record(self, o, n, key):
        """Object state from the 5-double record of a factorisation of n rows (log-determinant, min / max L_ii, z.z,
        LAPACK info); raises as scipy.linalg.cholesky inside george does when it failed.  ``key``: its _factor_key."""
        if o[4] != 0.0:
            raise LinAlgError("%d-th leading minor of the array is not positive definite" % int(o[4]))
        if not math.isfinite(o[0]):          # (np.isfinite on a scalar costs 0.5 us more: once per evaluation)
            raise LinAlgError("non-finite log-determinant")
        self.log_determinant = float(o[0])
        self.cond_estimate = float((o[2] / o[1]) ** 2)
        self._const = -0.5 * (n * _LOG_2PI + self.log_determinant)
        self._computed = True
        self.kernel.dirty = False
        self._factored_key = key

    def _factor(self, y, upload_x=False):
        """Gram + Cholesky (+ z = L^-1 (y - mean) carried through the factorisation)
        + log-determinant / diagonal range / z.z / info, fetched with ONE 40-byte
        device-to-host copy.  This is one gpUtils._nll evaluation."""
        r = self._replays.get("nll")
        if (r is not None and y is not None and not upload_x
                and r.fits(y, (self._x, self._x_d, self._y_d, self._L, self._z))):
            # one more evaluation in the buffers of the last one (same training set, y and stream), minus everything
            # that cannot have changed -- the optimiser loop's path (SciPy asks for ~6e5 evaluations in BASELINE
            # config 5; the generic path's 17 us of Python between two device evaluations were 7 % of each)
            ks, o = r.data
            self._kernel_struct(ks)
            # (as _reset_device_state: whatever was derived from the previous factor is stale)
            self._alpha = self._packed = self._packed_solve = self._work = self._xs = self._xs_key = None
            self._prune_rows = self._prune_srows = None
            self._computed = False
            r.args[4] = float(self.mean.value)
            try:
                _lib.check(r.fn(*r.args), "apgp_nll_eval")
                self._take_record(o, r.n, bytes(ks))
            except Exception:
                self._reset_device_state()
                raise
            self._ztz_host = float(o[3])
            self._alpha_mean = self.mean.value
            return
        torch, dev, lib = self._rt()
        x = self._x
        n = len(x)
        yv = None if y is None else self._check_dimensions(y)
        keep_x = None if upload_x else self._x_d
        keep_y = self._y_d if (yv is not None and self._alpha_y is not None
                               and np.array_equal(self._alpha_y, yv)) else None
        keep_nll = (self._L, self._z) if (self._L is not None and self._z is not None and self._L_store is None
                                          and self._nll_owned) else None
        keep_stream = self._nll_stream
        self._reset_device_state()
        self._computed = False
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._x_d = keep_x if keep_x is not None else torch.from_numpy(x).to(dev)
            # zeroed: the library reads and writes the lower triangle only (Gram, factor in place -- LAPACK's
            # dpotrf contract), so what is kept as the factor is a clean lower-triangular L.
            # (n <= 64 with y: the fused kernel writes the whole n x n itself.)
            # An optimiser's evaluations (set_parameter_vector + log_likelihood, over and over) refactorise in
            # the SAME buffers: the previous factor is dead once its hyper-parameters are, and nothing else
            # references an exactly-sized private factor (appended chains share a store: never reused here).
            # ... on the SAME stream only: the in-place refactorisation (memset + Gram) is ordered behind the previous
            # evaluation's readers by stream order, not by the caching allocator -- a caller that switched the current
            # stream between two evaluations gets fresh buffers
            reuse = keep_nll if (keep_nll is not None and yv is not None and keep_nll[0].shape[0] == n
                                 and keep_stream == st.value) else None
            if reuse is not None:
                # (no memset: the tiles on and below the diagonal are rewritten in full by the Gram kernel, the strict
                # upper tiles are still the zeros of the allocation -- nothing in the library writes them; the memset
                # was a fourth dependent launch per evaluation, 14 us on average over N = 512 .. 4096)
                K, z = reuse
            else:
                K = (torch.empty if (yv is not None and n <= 64) else torch.zeros)((n, n), dtype=torch.float64, device=dev)
                z = None
            # the whole evaluation as ONE library call and one synchronisation: Gram + Cholesky on the persistent /
            # hybrid plan (+ z = L^-1 (y - mean) riding along when y is given: a gpUtils._nll evaluation; without y:
            # compute() / recompute(), the same plan -- round 4 still sent these through a launch per 64-column step)
            y_d = None
            if yv is not None:
                y_d = keep_y if keep_y is not None else torch.from_numpy(yv).to(dev)
                if z is None:
                    z = torch.empty(n, dtype=torch.float64, device=dev)
            scr = self._nll_scratch
            if scr is None:
                scr = self._nll_scratch = (torch.empty(1, dtype=torch.int32, device=dev),
                                           torch.empty(5, dtype=torch.float64, device=dev))
            o = np.empty(5, dtype=np.float64)
            args = [self._x_d.data_ptr(), n, ctypes.byref(ks), y_d.data_ptr() if y_d is not None else None,
                    float(self.mean.value), K.data_ptr(), z.data_ptr() if yv is not None else None,
                    scr[0].data_ptr(), scr[1].data_ptr(), o.ctypes.data, st]
            _lib.check(lib.apgp_nll_eval(*args), "apgp_nll_eval")
            if yv is None:
                z = None
            L = K
        self._take_record(o, n, bytes(ks))      # (raises as scipy.linalg.cholesky inside george)
        self._L = L
        self._ld = n
        if z is not None:
            self._z = z
            self._ztz_host = float(o[3])
            self._y_d = y_d
            self._alpha_y = np.array(yv, copy=True)
            self._alpha_mean = self.mean.value
            self._nll_owned = True    # (K, z) came from an _nll evaluation: the next one may refactorise in place
            self._nll_stream = st.value
            # everything the NEXT evaluation on this training set, y and stream needs, ready to go
            self._replays["nll"] = _Replay(lib.apgp_nll_eval, args, dev.index, st.value or 0, yv,
                                           (x, self._x_d, y_d, K, z), self._queries, data=(ks, o))

    def recompute(self, quiet=False, **kwargs):
        if self.kernel.dirty or not self._computed:
            if self._x is None:
                raise RuntimeError("You need to compute the model first")
            try:
                self._factor(None)
            except (ValueError, LinAlgError):
                if quiet:
                    return False
                raise
        return True

    # -- arguments of the acquisition-side library calls --------------------------------
    def _candidates(self, t):
        """The candidate matrix ``t`` as a device tensor (M, D): a torch tensor is checked and taken as it is (candidates
        already resident in HBM), anything else is parsed and uploaded once."""
        if hasattr(t, "data_ptr"):
            if t.dim() != 2 or t.shape[1] != self.kernel.ndim or not t.is_contiguous() \
                    or str(t.dtype) != "torch.float64" or not t.is_cuda:
                raise ValueError("device candidates must be a contiguous (M, D) float64 CUDA tensor")
            return t
        torch, dev, _ = self._rt()
        return torch.from_numpy(self.parse_samples(t)).to(dev)

    def _mask(self, mask, m):
        """The admissibility ``mask`` of ``m`` candidates as a device uint8 tensor (None: no mask)."""
        if mask is None:
            return None
        mk = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        if mk.shape != (m,):
            raise ValueError("mask must have one entry per candidate")
        torch, dev, _ = self._rt()
        return torch.from_numpy(mk).to(dev)

    def _variance_operand(self, use_solve):
        """The (W, ldw, L, ldl) arguments of the calls that take sigma^2 from the resident dense W = L^-1 or, with
        ``use_solve``, by substitution against the factor -- and the buffer a replay of such a call depends on."""
        if use_solve:
            return (None, 0, self._L.data_ptr(), self._ld), self._L
        return (self._work.data_ptr(), (len(self._x) + 63) // 64 * 64, None, 0), self._work

    def _trsv(self, st, src, shift, trans, dst, ss, what, retry_ss=None):
        """dst = L^-1 (src - shift) (``trans`` 1: L^-T) by the persistent solve on stream ``st``, dst . dst into ``ss``;
        returns that as a float.  NaN there: the solve could not get its workgroups resident (apgp.h: it writes NaN
        instead of hanging) -- or the factor is not finite, in which case the re-run says so too.  Once more then, a
        launch per 256 rows, chosen for THIS call only: other threads' and streams' solves keep their path.
        ``retry_ss``: where the re-run writes dst . dst (None: nowhere); given, its value is the one returned."""
        lib = self._rt()[2]
        solve = (self._L.data_ptr(), len(self._x), self._ld, src.data_ptr(), shift, trans, dst.data_ptr())
        _lib.check(lib.apgp_trsv(*solve, ss.data_ptr(), st), "apgp_trsv(%s)" % what)
        norm2 = float(ss.item())
        if norm2 != norm2:
            _lib.check(lib.apgp_trsv_ex(*solve, _ptr(retry_ss), 1, st), "apgp_trsv(%s, multi-launch)" % what)
            if retry_ss is not None:
                norm2 = float(retry_ss.item())
        return norm2

    # -- K3: z = L^-1 (y - mean), alpha = L^-T z -----------------------------------
    def _solve(self, y, need_alpha):
        """Ensures z (and alpha) for this y; returns z.z as a float.  With the dense
        W = L^-1 resident (every sweep set-up) and a trusted condition estimate, both are
        HBM-rate matrix-vector products (``apgp_winv_apply``); otherwise the triangular
        solves (``apgp_trsv``), which also serve ill-conditioned factors."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n = len(y)
        same = (self._alpha_y is not None and self._alpha_mean == self.mean.value
                and np.array_equal(self._alpha_y, y))
        trust_w = self._trust_inverse()
        need_solve = (not same or self._z is None) or (need_alpha and self._alpha is None)
        if trust_w and need_solve and need_alpha and self._work is None and n >= W_FIRST_MIN_N:
            # alpha wanted (a sweep, a gradient or the sampler follows) and no inverse yet: L^-1
            # (0.8 ms at N = 4096) + two matrix-vector products beat the two triangular solves
            # (0.7 ms each), and the sweep / gradient needs W anyway.  A bare log_likelihood on a new
            # y (need_alpha False) keeps the ONE forward solve: it is cheaper than the O(N^3) inverse.
            self._ensure_linv()
        via_w = self._work is not None and trust_w
        np64 = (n + 63) // 64 * 64
        with self._on(torch, dev):
            st = self._stream(torch)
            if not same or self._z is None:
                self._y_d = torch.from_numpy(y).to(dev)
                self._z = torch.empty(n, dtype=torch.float64, device=dev)
                ztz = torch.empty(1, dtype=torch.float64, device=dev)
                if via_w:
                    _lib.check(lib.apgp_winv_apply(self._work.data_ptr(), np64, n, self._y_d.data_ptr(),
                                                   float(self.mean.value), 0, self._z.data_ptr(),
                                                   ztz.data_ptr(), None, st), "apgp_winv_apply(forward)")
                    self._ztz_host = float(ztz.item())
                else:
                    self._ztz_host = self._trsv(st, self._y_d, float(self.mean.value), 0, self._z, ztz, "forward",
                                                retry_ss=ztz)
                self._alpha = None
                self._xs = self._prune_rows = self._prune_srows = None
                self._alpha_y = np.array(y, copy=True)
                self._alpha_mean = self.mean.value
            if need_alpha and self._alpha is None:
                self._alpha = torch.empty(n, dtype=torch.float64, device=dev)
                if via_w:
                    wk = torch.empty(int(lib.apgp_winv_apply_work_len(n)), dtype=torch.float64, device=dev)
                    _lib.check(lib.apgp_winv_apply(self._work.data_ptr(), np64, n, self._z.data_ptr(), 0.0, 1,
                                                   self._alpha.data_ptr(), None, wk.data_ptr(), st),
                               "apgp_winv_apply(backward)")
                else:
                    self._trsv(st, self._z, 0.0, 1, self._alpha, torch.empty(1, dtype=torch.float64, device=dev), "backward")
                self._xs = self._prune_rows = self._prune_srows = None
        return self._ztz_host

    def log_likelihood(self, y, quiet=False):
        """george GP.log_likelihood (gpUtils.py:78,247): never raises when quiet.
        When the model is dirty (the gpUtils._nll pattern: set_parameter_vector then
        log_likelihood) the refactorisation carries y along, so the whole evaluation
        is gram + potrf + one reduction + one 40-byte copy."""
        try:
            if self.kernel.dirty or not self._computed:
                if self._x is None:
                    raise RuntimeError("You need to compute the model first")
                self._factor(y)
                ztz = self._ztz_host          # (z = L^-1 (y - mean) rode along with the factorisation)
            else:
                ztz = self._solve(y, need_alpha=False)
            ll = self._const - 0.5 * ztz
        except (ValueError, LinAlgError):
            if quiet:
                return -np.inf
            raise
        return ll if np.isfinite(ll) else -np.inf

    # Powell look-ahead (gpUtils._powellAhead): how many points beyond the one asked for are worth evaluating in the same
    # device call -- where a small batch costs little more than one evaluation (apgp_nll_eval_batch: one launch with a
    # workgroup per matrix up to n = 128; the persistent factorisations side by side in one launch above that, each on
    # 1 / batch of the CUs -- tools/nll_side_batch.py, profiles/r06c_*: 6 matrices 1.2 / 1.2 / 1.3 x one evaluation at
    # n = 512 / 832 / 1152, 4 matrices 1.4 x at 1664, 2 matrices 1.13 x at 2048); widths measured inside SciPy's Powell
    # (tools/nll_powell_rate.py --width 3,4,5; profiles/r06p_*): 5 is best up to n = 1152, 3 at 1600; 0 = off.
    lookahead = None              # None: by size; 0: off; k: that many points

    def lookahead_width(self):
        if self.lookahead is not None:
            return int(self.lookahead)
        n = 0 if self._x is None else len(self._x)
        if n <= 0:
            return 0
        return 5 if n <= 1216 else (3 if n <= 1728 else (1 if n <= 2112 else 0))

    def _fast_structs(self, P, out):
        """The C ABI's kernel structs + means of the hyper-vectors ``P`` (B x len(self)) written straight into ``out``
        (B x 36 doubles = B ``apgp_kernel_t``), for the two kernel shapes ``defaultGP`` builds without a linear term
        (gpUtils.py:160-165) -- every field by the expression ``_kernel_struct`` uses after ``set_parameter_vector``, so
        the same bits, without touching the object's state.  None for any other kernel."""
        k = self.kernel
        tk = type(k)
        if tk is ExpSquaredKernel:
            amp_dim, d = 0, k.ndim
        elif tk is Product and type(k.k1) is ConstantKernel and type(k.k2) is ExpSquaredKernel:
            amp_dim, d = k.k1.ndim, k.k2.ndim
        else:
            return None
        at = 0
        if self.fit_mean:
            means = P[:, 0].copy(); at += 1
        else:
            means = np.full(len(P), float(self.mean.value))
        ints = out.view(np.int32)
        out[:] = 0.0
        ints[:, 0] = d
        c = at + int(self.fit_white_noise)
        # (np.exp is an element-wise ufunc: the value of an element does not depend on the array it sits in, so these are
        # the bits of _kernel_struct's scalar / length-d calls -- asserted by the look-ahead tests, which compare an
        # optimiser's whole trajectory through this path with the one through single evaluations)
        if self.fit_white_noise:
            out[:, 2] = float(self._yerr2) + np.exp(np.ascontiguousarray(P[:, at]))      # (contiguous: the ufunc's SIMD loop)
        else:
            out[:, 2] = float(self._yerr2) + float(np.exp(self.white_noise.value))
        if amp_dim:
            out[:, 1] = amp_dim * np.exp(np.ascontiguousarray(P[:, c]))
            c += 1
        else:
            out[:, 1] = 1.0
        out[:, 3:3 + d] = np.exp(-P[:, c:c + d])
        return means

    def nll_batch(self, P, y):
        """Negative marginal log-likelihood at each hyper-parameter vector of ``P`` (B x P),
        evaluated by ONE batched Gram + Cholesky + solve call (``apgp_nll_eval_batch``;
        SURVEY.md section 8(f) rank 3).  Entry b is what ``gpUtils._nll(P[b], gp, y, None)``
        returns -- bit-identical, every matrix takes the code path of the single call --
        with ``+inf`` for a non-positive-definite Gram matrix.  The GP's own parameter
        vector is restored; its factorisation is marked stale."""
        torch, dev, lib = self._rt()
        if self._x is None:
            raise RuntimeError("You need to compute the model first")
        P = np.atleast_2d(np.asarray(P, dtype=np.float64))
        B, n = len(P), len(self._x)
        if P.shape[1] != len(self):
            raise ValueError("dimension mismatch")
        r = self._replays.get(("batch", B))
        if r is not None and r.fits(y, (self._x, self._batch)):
            # a small batch on the training set, y and stream of the previous one (the look-ahead of a Powell line search,
            # the rounds of a lock-step fit): buffers, argument list and struct array are ready
            karr, o = r.data
            means = self._fast_structs(P, karr)
            if means is not None:
                self._batch.means[:B] = means
                self.kernel.dirty = True          # (the buffers the object's own factor may share are not touched; as below)
                self._computed = False
                _lib.check(r.fn(*r.args), "apgp_nll_eval_batch")
                return _records_nll(o, n)
        yv = self._check_dimensions(y)
        out = np.full(B, np.inf)
        saved = self.get_parameter_vector()
        structs, means, live = [], [], []
        try:
            for b in range(B):
                try:
                    self.set_parameter_vector(P[b])
                    ks = self._kernel_struct()
                except (LinAlgError, ValueError, OverflowError):
                    continue
                structs.append(ks)
                means.append(float(self.mean.value))
                live.append(b)
        finally:
            self.set_parameter_vector(saved)
        if not live:
            return out
        # chunks bounded by 2 GiB of Gram-matrix work space
        per = max(1, int((2 << 30) // (8 * n * n)))
        with self._on(torch, dev):
            st = self._stream(torch)
            if self._x_d is None:
                self._x_d = torch.from_numpy(self._x).to(dev)
            # the rounds of a lock-step fit (gpUtils._minimizeLockStep) come back with the same y, batch size and stream a few
            # hundred times: the device copy of y and the work buffers are kept (the call is synchronous: nothing of the
            # previous round is in flight)
            ybytes = yv.tobytes()
            work = self._batch
            if (work is None or work.x_d is not self._x_d or work.stream != (st.value or 0) or work.ybytes != ybytes
                    or work.x is not self._x):
                work = self._batch = _BatchWork(self._x, self._x_d, st.value or 0, ybytes, torch.from_numpy(yv).to(dev),
                                                {}, np.empty(8, dtype=np.float64))
                self._replays = {k: v for k, v in self._replays.items() if type(k) is not tuple}   # (the old space's)
            for c0 in range(0, len(live), per):
                idx = live[c0:c0 + per]
                nb = len(idx)
                karr = (_lib.KernelStruct * nb)(*structs[c0:c0 + nb])
                marr = np.array(means[c0:c0 + nb], dtype=np.float64)
                bufs = work.bufs.get(nb)
                if bufs is None:
                    bufs = (torch.empty((nb, n, n), dtype=torch.float64, device=dev),
                            torch.empty((nb, n), dtype=torch.float64, device=dev),
                            torch.empty(nb, dtype=torch.int32, device=dev),
                            torch.empty((nb, 5), dtype=torch.float64, device=dev))
                    if 8 * nb * n * n <= (256 << 20):     # (larger work spaces are not hoarded; 6 matrices of N = 2300 fit)
                        work.bufs[nb] = bufs
                K, z, info, o_d = bufs
                o = np.empty((nb, 5), dtype=np.float64)
                _lib.check(lib.apgp_nll_eval_batch(self._x_d.data_ptr(), n, nb, ctypes.addressof(karr),
                                                   work.y_d.data_ptr(), marr.ctypes.data, K.data_ptr(), z.data_ptr(),
                                                   info.data_ptr(), o_d.data_ptr(), o.ctypes.data, st),
                           "apgp_nll_eval_batch")
                if nb == B and B <= 8 and nb in work.bufs and ctypes.sizeof(_lib.KernelStruct) == 36 * 8:
                    # the next batch of this size on this training set, y and stream: everything but the hyper-vectors ready
                    ka = np.zeros((B, 36), dtype=np.float64)
                    oo = np.empty((B, 5), dtype=np.float64)
                    args = [self._x_d.data_ptr(), n, B, ka.ctypes.data, work.y_d.data_ptr(), work.means.ctypes.data,
                            K.data_ptr(), z.data_ptr(), info.data_ptr(), o_d.data_ptr(), oo.ctypes.data, st]
                    self._replays[("batch", B)] = _Replay(lib.apgp_nll_eval_batch, args, dev.index, st.value or 0, yv,
                                                          (self._x, work), self._queries, data=(ka, oo))
                out[idx] = _records_nll(o, n)
        return out

    # -- packed factor / training stream for the sweep -------------------------------
    def _ensure_linv(self):
        torch, dev, lib = self._rt()
        if self._packed is not None:
            return
        n = len(self._x)
        with self._on(torch, dev):
            st = self._stream(torch)
            self._work = torch.empty(lib.apgp_trtri_work_len(n), dtype=torch.float64, device=dev)
            self._packed = torch.empty(lib.apgp_packed_linv_len(n), dtype=torch.float64, device=dev)
            _lib.check(lib.apgp_trtri_pack(self._L.data_ptr(), n, self._ld, self._work.data_ptr(),
                                           self._packed.data_ptr(), None, st), "apgp_trtri_pack")

    def _ensure_lsolve(self):
        """Tiles of the substitution form of the sweep: one O(N^2) pass over the factor."""
        torch, dev, lib = self._rt()
        if self._packed_solve is not None:
            return
        n = len(self._x)
        with self._on(torch, dev):
            st = self._stream(torch)
            self._packed_solve = torch.empty(lib.apgp_packed_lsolve_len(n), dtype=torch.float64, device=dev)
            _lib.check(lib.apgp_pack_lsolve(self._L.data_ptr(), n, self._ld, self._packed_solve.data_ptr(), st),
                       "apgp_pack_lsolve")

    def _ensure_xs(self, y):
        torch, dev, lib = self._rt()
        self._solve(y, need_alpha=True)
        if self._xs is not None:
            return
        n = len(self._x)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._xs = torch.empty(lib.apgp_packed_train_len(n, ks.ndim), dtype=torch.float64,
                                   device=dev)
            _lib.check(lib.apgp_pack_train(self._x_d.data_ptr(), self._alpha.data_ptr(), n,
                                           ctypes.byref(ks), self._xs.data_ptr(), st),
                       "apgp_pack_train")
            # the rows split into bf16 parts for the coarse bound of the pruned arg-min: once per fit, not per call
            rows_len = int(lib.apgp_prune_rows_len(n, ks.ndim))
            self._prune_rows = None
            if rows_len > 0:
                self._prune_rows = torch.empty(rows_len, dtype=torch.float64, device=dev)
                _lib.check(lib.apgp_pack_prune_rows(self._xs.data_ptr(), n, ctypes.byref(ks),
                                                    self._prune_rows.data_ptr(), st), "apgp_pack_prune_rows")
            # and sorted by alpha's sign, for the bound's one-chain route (prune_signed)
            srows_len = int(lib.apgp_prune_srows_len(n, ks.ndim))
            self._prune_srows = None
            if srows_len > 0:
                self._prune_srows = torch.empty(srows_len, dtype=torch.float64, device=dev)
                _lib.check(lib.apgp_pack_prune_srows(self._xs.data_ptr(), n, ctypes.byref(ks),
                                                     self._prune_srows.data_ptr(), st), "apgp_pack_prune_srows")

    def _prune_stream(self):
        """(pointer or None, APGP_PRUNE_ROWS_* kind) of the row stream the coarse bound reads: ``prune_signed``."""
        if self.prune_signed and self._prune_srows is not None:
            return self._prune_srows.data_ptr(), _lib.PRUNE_ROWS_SIGNED
        return _ptr(self._prune_rows), _lib.PRUNE_ROWS_SPLIT

    # -- predict (george GP.predict) ----------------------------
    def predict(self, y, t, return_cov=True, return_var=False, cache=True, **kwargs):
        if (self._computed and not self.kernel.dirty and type(t) is np.ndarray and t.dtype == _F64
                and t.ndim == 2 and t.flags.c_contiguous):
            # the replays of the small calls (_mean_host, _predict_one): the previous call's arguments with new points
            if return_var:
                r = self._replays.get("one")
                # (the factor of the variance form in use: a switch of form is a different object)
                if (r is not None and t.shape == r.data[1] and r.args[4] == self.mean.value
                        and r.fits(y, (self._xs, self._p1_work, self._work if self._trust_inverse() else self._L))):
                    r.args[0] = t.ctypes.data
                    _lib.check(r.fn(*r.args), "apgp_predict1_host")
                    o2 = r.data[0]
                    return np.array([o2[0]]), np.array([o2[1]])
            elif not return_cov:
                r = self._replays.get("mean")
                m, d = t.shape
                if (r is not None and d == r.data[0] and 0 < m <= r.data[1] and r.args[5] == self.mean.value
                        and r.fits(y, (self._xs, self._mean_work))):
                    mu_h = np.empty(m)
                    r.args[0], r.args[1], r.args[6] = t.ctypes.data, m, mu_h.ctypes.data
                    _lib.check(r.fn(*r.args), "apgp_predict_mean_host")
                    return mu_h
        self.recompute()
        xs = self.parse_samples(t)
        if return_cov and not return_var:
            return self._predict_cov(y, xs)
        if not return_var:
            return self._mean(y, xs)
        if len(xs) == 1:
            return self._predict_one(y, xs)
        y = self._check_dimensions(y)
        if len(xs) == 0:        # (as every empty candidate set: y is still checked, nothing is prepared on the device)
            return np.empty(0), np.empty(0)
        torch, dev, _ = self._rt()
        s = self._sweep(y, torch.from_numpy(xs).to(dev), _lib.UTIL_NONE, with_mu=True, with_var=True)
        return s.mu.cpu().numpy(), s.var.cpu().numpy()

    def _mean(self, y, xs):
        """The predictive mean at the host points ``xs`` (M, D), by the route of their number."""
        if len(xs) == 0:
            self._check_dimensions(y)
            return np.empty(0)
        if len(xs) <= 4096:
            return self._mean_host(y, xs)
        torch, dev, _ = self._rt()
        return self._mean_device(y, torch.from_numpy(xs).to(dev)).cpu().numpy()

    def _mean_host(self, y, xs):
        """Latency-bound mean-only call (the sampler's _gpll batches) at 1 .. 4096 host points: host buffers in and out
        through ONE library call and one synchronisation."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n, m = len(self._x), len(xs)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            need = m * (ks.ndim + 1)
            if self._mean_work is None or self._mean_work.numel() < need:
                self._mean_work = torch.empty(max(need, 1024), dtype=torch.float64, device=dev)
            mu_h = np.empty(m, dtype=np.float64)
            args = [xs.ctypes.data, m, self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value),
                    mu_h.ctypes.data, self._mean_work.data_ptr(), st]
            _lib.check(lib.apgp_predict_mean_host(*args), "apgp_predict_mean_host")
            # the sampler asks again, for another few points of the same model and y, 4e4 times per chain (the walker
            # ensembles of ApproxPosterior._gpllBatch, approx.py:148-189)
            max_m = min(4096, self._mean_work.numel() // (ks.ndim + 1))
            self._replays["mean"] = _Replay(lib.apgp_predict_mean_host, args, dev.index, st.value or 0, y,
                                            (self._xs, self._mean_work), self._queries, data=(ks.ndim, max_m))
        return mu_h

    def _mean_device(self, y, T):
        """The predictive mean at the rows of the device tensor ``T`` (M >= 1, D), as a device tensor."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            self._ensure_xs(y)
            mu = torch.empty(T.shape[0], dtype=torch.float64, device=dev)
            _lib.check(lib.apgp_predict_mean(T.data_ptr(), T.shape[0], self._xs.data_ptr(), len(self._x),
                                             ctypes.byref(ks), float(self.mean.value), mu.data_ptr(),
                                             self._stream(torch)), "apgp_predict_mean")
        return mu

    def _predict_one(self, y, xs):
        """(mu, sigma^2) at ONE host point: the reference's scalar utilities (utility.py:131,178,224), once per
        Nelder-Mead step of minimizeObjective -- three small launches, the result through the mailbox."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n = len(self._x)
        ks = self._kernel_struct()
        use_solve = not self._trust_inverse()
        with self._on(torch, dev):
            st = self._stream(torch)
            if not use_solve:
                self._ensure_linv()     # first: with W resident alpha is two matrix-vector products
            self._ensure_xs(y)          # (above the conditioning gate a single candidate solves against L itself)
            if self._p1_work is None or self._p1_work.numel() < int(lib.apgp_predict1_work_len(n)):
                self._p1_work = torch.empty(int(lib.apgp_predict1_work_len(n)), dtype=torch.float64, device=dev)
            o2 = np.empty(2, dtype=np.float64)
            inv, factor = self._variance_operand(use_solve)
            args = [xs.ctypes.data, self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), *inv,
                    self._p1_work.data_ptr(), o2.ctypes.data, st]
            _lib.check(lib.apgp_predict1_host(*args), "apgp_predict1_host")
            # the reference's scalar utilities ask again at the next simplex point, ~460 times per search
            self._replays["one"] = _Replay(lib.apgp_predict1_host, args, dev.index, st.value or 0, y,
                                           (self._xs, self._p1_work, factor), self._queries, data=(o2, (1, ks.ndim)))
        return np.array([o2[0]]), np.array([o2[1]])

    # -- predictive gradients (apgp_predict_grad) -----------------------------------------------
    def predict_grad(self, y, t, kind=None, bounds=None, zeta=0.01, return_device=False):
        """mu, sigma^2 and their gradients with respect to the query point, at every row of ``t`` ((M, D) or one point
        (D,); host array or device tensor as in :meth:`acquire`), by ``apgp_predict_grad``: dmu = J^T alpha,
        dvar = d k(t,t)/dt - 2 J^T K^-1 k with J_nd = d k(t, x_n)/d t_d, K^-1 k through the dense inverse or, above the
        conditioning gate, by a forward and a backward substitution against the factor (``variance_mode`` forces one).

        ``kind=None``: returns ``(mu (M,), var (M,), dmu (M, D), dvar (M, D))``.  ``kind`` "agp" / "bape" / "jones"
        (with ``zeta`` and max(y)) / "negmean": returns ``(u (M,), du (M, D), mu, var)``, du by the chain rule through the
        utility's derivatives.  ``bounds``: the box prior; a row outside it or with a non-finite coordinate has
        mu = var = dmu = dvar = NaN, u = +inf, du = 0.  Where a utility leaves its smooth branch (BAPE with var <= 0,
        Jones with a standard deviation not > 0) du = 0.  NumPy arrays, or with ``return_device`` device tensors
        (stream-ordered on the current stream)."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        if kind is None:
            kid = _lib.UTIL_NONE
        else:
            try:
                kid = SEARCH_KINDS[str(kind).lower()]
            except KeyError:
                raise ValueError("kind must be None or one of %s" % sorted(SEARCH_KINDS))
        D = self.kernel.ndim
        bkey = None if bounds is None else np.asarray(bounds, dtype=np.float64).tobytes()
        host_point = (type(t) is np.ndarray and t.dtype == _F64 and t.size == D and t.ndim in (1, 2)
                      and t.flags.c_contiguous and not return_device)
        if host_point:
            # the optimiser's next evaluation: the previous call's arguments, buffers and checks with a new point
            r = self._replays.get("pgrad")
            if (r is not None and r.data[0] == (kid, bkey, float(zeta), self.mean.value)
                    and r.fits(y, (self._xs, self._pg_work, self._work if self._trust_inverse() else self._L))):
                _, torch, T_d, out = r.data
                T_d.copy_(torch.from_numpy(t.reshape(1, D)))
                _lib.check(r.fn(*r.args), "apgp_predict_grad")
                return self._pgrad_split(out.cpu().numpy(), 1, D, kid)
        torch, dev, lib = self._rt()
        lo, hi = _box(bounds, D)
        if hasattr(t, "data_ptr"):
            T = self._candidates(t)
        else:
            arr = np.asarray(t, dtype=np.float64)
            if arr.ndim == 1:
                if arr.size != D:
                    raise ValueError("Dimension mismatch")
                arr = arr.reshape(1, D)
            if arr.ndim != 2 or arr.shape[1] != D:
                raise ValueError("Dimension mismatch")
            T = None
        y = self._check_dimensions(y)
        n = len(self._x)
        m = int(T.shape[0] if T is not None else arr.shape[0])
        ks = self._kernel_struct()
        use_solve = not self._trust_inverse()
        with self._on(torch, dev):
            st = self._stream(torch)
            if T is None:
                T = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            out = torch.empty(m * (3 + 3 * D), dtype=torch.float64, device=dev)
            if m == 0:
                res = self._pgrad_split(out, 0, D, kid)
                return res if return_device else tuple(o.cpu().numpy() for o in res)
            if not use_solve:
                self._ensure_linv()     # first: with W resident alpha is two matrix-vector products
            self._ensure_xs(y)
            need = int(lib.apgp_predict_grad_work_len(m, n))
            if self._pg_work is None or self._pg_work.numel() < need:
                self._pg_work = torch.empty(need, dtype=torch.float64, device=dev)
            inv, factor = self._variance_operand(use_solve)
            p0 = out.data_ptr()
            with_u = kid != _lib.UTIL_NONE
            args = [T.data_ptr(), m, self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), *inv, kid,
                    lo, hi, float(zeta), float(np.max(y)),
                    p0, p0 + 8 * m, p0 + 16 * m if with_u else None, p0 + 24 * m, p0 + 8 * m * (3 + D),
                    p0 + 8 * m * (3 + 2 * D) if with_u else None, self._pg_work.data_ptr(), st]
            _lib.check(lib.apgp_predict_grad(*args), "apgp_predict_grad")
            if host_point:
                self._replays["pgrad"] = _Replay(
                    lib.apgp_predict_grad, args, dev.index, st.value or 0, y, (self._xs, self._pg_work, factor),
                    self._queries, data=((kid, bkey, float(zeta), self.mean.value), torch, T, out))
            if return_device:
                return self._pgrad_split(out, m, D, kid)
            return self._pgrad_split(out.cpu().numpy(), m, D, kid)

    @staticmethod
    def _pgrad_split(out, m, D, kid):
        """The results of :meth:`predict_grad` from its packed output buffer (mu | var | u | dmu | dvar | du)."""
        mu, var, u = out[:m], out[m:2 * m], out[2 * m:3 * m]
        dmu, dvar, du = (out[m * (3 + j * D):m * (3 + (j + 1) * D)].reshape(m, D) for j in range(3))
        if kid == _lib.UTIL_NONE:
            return mu, var, dmu, dvar
        return u, du, mu, var

    def _sweep(self, y, T, kind_id, lo=None, hi=None, mask_d=None, zeta=0.01, idx_offset=0,
               with_mu=False, with_var=False, with_u=False):
        """The fused predict + utility + arg-min over the rows of the device tensor ``T`` (M >= 1, D), sigma^2 through
        the dense inverse or, above the conditioning gate, by substitution against the factor.  ``kind_id``: a utility
        or ``UTIL_NONE`` (prediction only); ``with_mu`` / ``with_var`` / ``with_u``: keep that per-candidate array.  Everything stays
        on the device (``_Swept``): the callers decide what to copy to the host."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n, m = len(self._x), T.shape[0]
        ks = self._kernel_struct()
        use_solve = not self._trust_inverse()
        with self._on(torch, dev):
            st = self._stream(torch)
            if use_solve:
                self._ensure_lsolve()
            else:
                self._ensure_linv()     # first: with W resident alpha is two matrix-vector products
            self._ensure_xs(y)
            f64 = dict(dtype=torch.float64, device=dev)
            mu, var, u = (torch.empty(m, **f64) if keep else None for keep in (with_mu, with_var, with_u))
            part = torch.empty(max(int(lib.apgp_acquire_work_len(m, n)), 2), **f64)
            best = torch.empty(2, **f64)
            ev = getattr(self, "kernel_events", None)   # bench.py: HIP events around the launch
            if ev is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            args = (self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), kind_id, lo, hi, _ptr(mask_d),
                    float(zeta), float(np.max(y)), _ptr(mu), _ptr(var), _ptr(u), part.data_ptr(), best.data_ptr(),
                    *self._prune_stream(), st)
            prune_was = None if self.sweep_prune is None else lib.apgp_set_sweep_prune(int(self.sweep_prune))
            rowsplit_was = None if self.seed_rowsplit is None else lib.apgp_set_seed_rowsplit(int(self.seed_rowsplit))
            park_was = None if self.seed_park is None else lib.apgp_set_seed_park(int(self.seed_park))
            prefetch_was = None if self.seed_prefetch is None else lib.apgp_set_seed_prefetch(int(self.seed_prefetch))
            first_was = None if self.seed_first is None else lib.apgp_set_seed_first(int(self.seed_first))
            parts_was = None if self.seed_parts is None else lib.apgp_set_seed_parts(int(self.seed_parts))
            pipe_was = None if self.prune_pipe is None else lib.apgp_set_prune_pipe(int(self.prune_pipe))
            try:
                if use_solve:
                    _lib.check(lib.apgp_acquire_solve_rows2(T.data_ptr(), m, int(idx_offset),
                                                            self._packed_solve.data_ptr(), *args), "apgp_acquire_solve_rows2")
                else:
                    _lib.check(lib.apgp_acquire_rows2(T.data_ptr(), m, int(idx_offset), self._packed.data_ptr(), *args),
                               "apgp_acquire_rows2")
            finally:
                if prune_was is not None:
                    lib.apgp_set_sweep_prune(prune_was)
                if rowsplit_was is not None:
                    lib.apgp_set_seed_rowsplit(rowsplit_was)
                if park_was is not None:
                    lib.apgp_set_seed_park(park_was)
                if prefetch_was is not None:
                    lib.apgp_set_seed_prefetch(prefetch_was)
                if first_was is not None:
                    lib.apgp_set_seed_first(first_was)
                if parts_was is not None:
                    lib.apgp_set_seed_parts(parts_was)
                if pipe_was is not None:
                    lib.apgp_set_prune_pipe(pipe_was)
            if self.sweep_prune_stats and kind_id != _lib.UTIL_NONE and mu is None and var is None and u is None:
                off = int(lib.apgp_sweep_prune_counts_offset(m, n))
                self.last_prune_counts = part[off:off + 5].view(torch.int64).clone()
            if ev is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                ev.append((e0, e1))
        return _Swept(best, mu, var, u)

    def acquire(self, y, t, kind, bounds=None, mask=None, zeta=0.01, return_all=False,
                idx_offset=0, device_record=False):
        """Fused predict + utility + arg-min over the candidate matrix ``t`` (M,D).

        The batched counterpart of utility.minimizeObjective (utility.py:253-372)
        for ``kind`` in {"agp","bape","jones"}.  ``bounds`` (sequence of (lo,hi))
        is the box prior fused into the kernel (candidates outside get +inf as
        utility.py:126-127 does); ``mask`` (M,) uint8/bool marks admissible
        candidates for arbitrary priors evaluated on the host.

        Returns (best_index, best_u) or, with return_all, additionally the
        arrays (u, mu, var).  best_index is -1 when no candidate is admissible.
        ``device_record``: return the sweep's 16-byte ``apgp_best_t`` record where the arg-min
        kernel left it -- a device int64[2] tensor (bit pattern of best_u, best_index), stream-ordered,
        no copy to the host: what ``dist.sharded_acquire`` hands to the RCCL all-gather.
        """
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        kind_id = UTILITY_KINDS[str(kind).lower()]
        if device_record and return_all:
            raise ValueError("device_record returns the arg-min record only")
        torch, dev, _ = self._rt()
        lo, hi = _box(bounds, self.kernel.ndim)
        T = self._candidates(t)
        mask_d = self._mask(mask, T.shape[0])
        y = self._check_dimensions(y)
        if T.shape[0] == 0:
            # empty candidate set: nothing admissible (index -1, +inf), empty arrays -- and nothing prepared on the device
            if device_record:
                return torch.tensor([int(np.float64(np.inf).view(np.int64)), -1], dtype=torch.int64, device=dev)
            return (-1, float("inf")) + ((np.empty(0),) * 3 if return_all else ())
        s = self._sweep(y, T, kind_id, lo, hi, mask_d, zeta, idx_offset, with_mu=return_all, with_var=return_all,
                        with_u=return_all)
        if device_record:
            return s.best.view(torch.int64)
        if not return_all:
            return _best_record(s.best)
        return _best_record(s.best) + (s.u.cpu().numpy(), s.mu.cpu().numpy(), s.var.cpu().numpy())

    def prune_bounds(self, y, t, kind, coarse=True, bounds=None, mask=None, zeta=0.01):
        """The bound pass of the pruned arg-min alone (``apgp_prune_bounds``; the tests): for every 64-row block of the
        candidates ``t`` the smallest lower bound of a row's utility, +inf for a block without an admissible row --
        ``coarse``: the single-precision stage, else the double-precision one.  Arguments as :meth:`acquire`'s."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        kind_id = UTILITY_KINDS[str(kind).lower()]
        torch, dev, lib = self._rt()
        lo, hi = _box(bounds, self.kernel.ndim)
        T = self._candidates(t)
        m = T.shape[0]
        mask_d = self._mask(mask, m)
        y = self._check_dimensions(y)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            self._ensure_xs(y)
            bmin = torch.empty((m + 63) // 64, dtype=torch.float64, device=dev)
            pipe_was = None if self.prune_pipe is None else lib.apgp_set_prune_pipe(int(self.prune_pipe))
            try:
                _lib.check(lib.apgp_prune_bounds_rows2(T.data_ptr(), m, self._xs.data_ptr(), len(self._x), ctypes.byref(ks),
                                                       float(self.mean.value), kind_id, lo, hi, _ptr(mask_d), float(zeta),
                                                       float(np.max(y)), int(bool(coarse)), bmin.data_ptr(),
                                                       *self._prune_stream(), None, self._stream(torch)),
                           "apgp_prune_bounds_rows2")
            finally:
                if pipe_was is not None:
                    lib.apgp_set_prune_pipe(pipe_was)
        return bmin.cpu().numpy()

    def nelder_mead_search(self, y, starts, kind, bounds=None, zeta=0.01, options=None, trace=False):
        """SciPy's Nelder-Mead (``bounds=None``) from every row of ``starts`` (R, D) at once on the device
        (``apgp_nm_search``: one workgroup per restart, one launch) over the objective ``kind``: "agp", "bape",
        "jones" (the utilities of :mod:`utility`; Jones with ``zeta`` and max(y)) or "negmean" (-mu, +inf where mu is
        not finite).  The objective is +inf where a coordinate is not finite or lies outside ``bounds`` (the box prior;
        None: no box).  sigma^2 comes from the dense inverse or from the factor by the usual gate (``variance_mode`` /
        the condition estimate); through the inverse at N <= 256 every (mu, sigma^2) is ``predict``'s, bit for bit.

        ``options``: SciPy's ``adaptive``, ``maxiter``, ``maxfev``, ``xatol``, ``fatol`` (any other key raises
        ``ValueError``; None = SciPy's defaults).  Returns ``(x (R, D), fun (R,), nfev (R,), nit (R,), status (R,))``;
        with ``trace`` also a list of one dict per restart: ``x`` (nfev, D), ``mu``, ``var``, ``u`` (nfev,) of every
        evaluation in order (mu = var = NaN where the box refused the point) and ``steps`` (the step of each
        iteration, ``_lib.NM_STEPS`` codes)."""
        try:
            kid = SEARCH_KINDS[str(kind).lower()]
        except KeyError:
            raise ValueError("kind must be one of %s" % sorted(SEARCH_KINDS))
        opts = dict(options or {})
        unknown = sorted(set(opts) - set(NM_OPTIONS))
        if unknown:
            raise ValueError("the device Nelder-Mead search does not take the option(s) %s (it takes %s)"
                             % (unknown, ", ".join(NM_OPTIONS)))
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        y = self._check_dimensions(y)
        D = self.kernel.ndim
        lo, hi = _box(bounds, D)
        X0 = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, D))
        R = len(X0)
        if not 1 <= R <= _lib.NM_MAX_RESTARTS:
            raise ValueError("between 1 and %d restarts per call" % _lib.NM_MAX_RESTARTS)
        rho, chi, psi, sigma = nm_coefficients(D, bool(opts.get("adaptive", False)))
        maxiter, maxfev = nm_limits(D, opts.get("maxiter"), opts.get("maxfev"))
        if not (1 <= maxiter <= _lib.NM_MAX_FEV and 1 <= maxfev <= _lib.NM_MAX_FEV):
            raise ValueError("maxiter and maxfev must lie between 1 and %d" % _lib.NM_MAX_FEV)
        opt = _lib.NmOptions(kind=kid, maxiter=maxiter, maxfev=maxfev, reserved=0, zeta=float(zeta),
                             ybest=float(np.max(y)), xatol=float(opts.get("xatol", 1e-4)),
                             fatol=float(opts.get("fatol", 1e-4)), rho=rho, chi=chi, psi=psi, sigma=sigma)
        torch, dev, lib = self._rt()
        n = len(self._x)
        ks = self._kernel_struct()
        use_solve = not self._trust_inverse()
        with self._on(torch, dev):
            st = self._stream(torch)
            if not use_solve:
                self._ensure_linv()
            self._ensure_xs(y)
            f64 = dict(dtype=torch.float64, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            starts_d = torch.from_numpy(X0).to(dev)
            x_out = torch.empty((R, D), **f64)
            f_out = torch.empty(R, **f64)
            stats = torch.zeros((R, 3), **i32)
            work = torch.empty(int(lib.apgp_nm_search_work_len(R, n)), **f64)
            tr = torch.empty(R * maxfev * (D + 3), **f64) if trace else None
            steps = torch.zeros(R * maxiter, **i32) if trace else None
            inv, _ = self._variance_operand(use_solve)
            _lib.check(lib.apgp_nm_search(starts_d.data_ptr(), R, self._xs.data_ptr(), n, ctypes.byref(ks),
                                          float(self.mean.value), *inv, lo, hi, ctypes.byref(opt),
                                          x_out.data_ptr(), f_out.data_ptr(), stats.data_ptr(),
                                          _ptr(tr), _ptr(steps), work.data_ptr(), st),
                       "apgp_nm_search")
            x = x_out.cpu().numpy()
            fun = f_out.cpu().numpy()
            sts = stats.cpu().numpy()
            if trace:
                trh = tr.cpu().numpy().reshape(R, maxfev, D + 3)
                sth = steps.cpu().numpy().reshape(R, maxiter)
        nfev, nit, status = sts[:, 0].copy(), sts[:, 1].copy(), sts[:, 2].copy()
        if not trace:
            return x, fun, nfev, nit, status
        recs = []
        for r in range(R):
            rec = trh[r, :nfev[r]]
            recs.append({"x": rec[:, :D].copy(), "mu": rec[:, D].copy(), "var": rec[:, D + 1].copy(),
                         "u": rec[:, D + 2].copy(), "steps": [int(s) for s in sth[r] if s != 0]})
        return x, fun, nfev, nit, status, recs

    def acquire_batch(self, y, t, kind, q, bounds=None, mask=None, zeta=0.01, idx_offset=0, return_all=False):
        """``q`` design points chosen jointly from the candidate matrix ``t`` (M, D; host array or device
        tensor, as in :meth:`acquire`) by the kriging believer: pick the arg-min, pretend it was observed at
        its predictive mean, condition on that fantasy with the hyper-parameters unchanged, pick again.

        One full sweep gives mu and sigma^2 of every candidate; each later pick costs one fantasy pass
        (``apgp_acquire_fantasy``): the mean does not move and every variance drops by a rank-one term,
        O(N D) per candidate instead of the sweep's O(N^2).  The GP itself is not modified.

        ``kind``: one utility name, or a sequence of ``q`` names (pick j uses ``kind[j]``).  Returns
        ``(indices (q,), u (q,))`` with ``u[j]`` pick j's utility under j fantasies; index -1 and +inf for a
        step without an admissible candidate and every step after it.  ``return_all`` adds the last step's
        ``(u, mu, var)`` arrays.  ``q = 1`` is :meth:`acquire`: same index, same bits."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        q = int(q)
        if not 1 <= q <= _lib.MAX_FANTASY:
            raise ValueError("q must be between 1 and %d (APGP_MAX_FANTASY)" % _lib.MAX_FANTASY)
        kinds = [kind] * q if isinstance(kind, str) else list(kind)
        if len(kinds) != q:
            raise ValueError("kind must be one utility name or a sequence of q names")
        kind_ids = [UTILITY_KINDS[str(k).lower()] for k in kinds]
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n, D = len(self._x), self.kernel.ndim
        lo, hi = _box(bounds, D)
        T = self._candidates(t)
        m = T.shape[0]
        mask_d = self._mask(mask, m)
        idx = np.full(q, -1, dtype=np.int64)
        ub = np.full(q, np.inf)
        if m == 0:
            return (idx, ub, np.empty(0), np.empty(0), np.empty(0)) if return_all else (idx, ub)
        # the first pick is acquire's sweep, with its prune override and event hook: neither changes this call, whose mu
        # and var arrays are always asked for -- the library prunes only when none of mu, var, u is (acquire_impl)
        s = self._sweep(y, T, kind_ids[0], lo, hi, mask_d, zeta, idx_offset, with_mu=True, with_var=True,
                        with_u=return_all)
        best, mu, u = s.best, s.mu, s.u
        ks = self._kernel_struct()
        ybest = float(np.max(y))
        with self._on(torch, dev):
            st = self._stream(torch)
            f64 = dict(dtype=torch.float64, device=dev)
            var = [s.var, torch.empty(m, **f64) if q > 1 else None]
            if q > 1:
                C = torch.empty((q - 1) * m, **f64)          # column-major, ldc = m: column j - 1 holds C_j
                fpart = torch.empty(max(int(lib.apgp_acquire_fantasy_work_len(m)), 2), **f64)
                krow = torch.empty(n, **f64)
                z = torch.empty(n, **f64)
                beta = torch.empty(n, **f64)
                ss = torch.empty(1, **f64)
            cur = 0
            for j in range(q):
                bi, bu = _best_record(best)                  # the 16-byte record of the last sweep / pass
                if bi < 0:
                    break
                idx[j], ub[j] = bi, bu
                if j == q - 1:
                    break
                r = bi - int(idx_offset)
                ybest = max(ybest, float(mu[r].item()))      # (Jones: the fantasy joins the observed values)
                # beta_j = K^-1 k(X, x_j): the cross row from the candidate row in HBM, two solves against the factor
                _lib.check(lib.apgp_kernel_cross(T.data_ptr() + 8 * r * D, 1, self._x_d.data_ptr(), n,
                                                 ctypes.byref(ks), krow.data_ptr(), n, st), "apgp_kernel_cross")
                self._trsv(st, krow, 0.0, 0, z, ss, "fantasy")
                self._trsv(st, z, 0.0, 1, beta, ss, "fantasy")
                _lib.check(lib.apgp_acquire_fantasy(T.data_ptr(), m, int(idx_offset), self._xs.data_ptr(), n,
                                                    ctypes.byref(ks), beta.data_ptr(), r, j + 1, C.data_ptr(), m,
                                                    mu.data_ptr(), var[cur].data_ptr(), var[1 - cur].data_ptr(),
                                                    kind_ids[j + 1], lo, hi, _ptr(mask_d), float(zeta), ybest,
                                                    _ptr(u), fpart.data_ptr(), best.data_ptr(), st),
                           "apgp_acquire_fantasy")
                cur = 1 - cur
            if return_all:
                return idx, ub, u.cpu().numpy(), mu.cpu().numpy(), var[cur].cpu().numpy()
        return idx, ub

    # -- integrated acquisition (DESIGN.md "Integrated acquisition") ------------------
    def _references(self, refs):
        R = np.ascontiguousarray(np.asarray(refs, dtype=np.float64))
        if R.ndim != 2 or R.shape[1] != self.kernel.ndim or not 1 <= len(R) <= _lib.MAX_REFS:
            raise ValueError("refs must be a (J, D) array of 1 <= J <= %d reference points (APGP_MAX_REFS)" % _lib.MAX_REFS)
        if not np.all(np.isfinite(R)):
            raise ValueError("refs must be finite")
        return R

    def integration_weights(self, y, refs, density="posterior"):
        """The log-weights ``a_j = log w_j + 2 mu(r_j) + var(r_j)`` of :meth:`acquire_integrated` for reference points
        ``refs`` (J, D) that are samples of the surrogate posterior (``density="posterior"``: w_j proportional to
        exp(-mu), a_j = mu_j + var_j) or uniform in the box (``"uniform"``: a_j = 2 mu_j + var_j), from one
        ``predict(return_var=True)`` over them.  Only differences of the a_j matter."""
        if density not in ("posterior", "uniform"):
            raise ValueError("density must be 'posterior' or 'uniform'")
        R = self._references(refs)
        mu, var = self.predict(y, R, return_cov=False, return_var=True)
        mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
        return (mu if density == "posterior" else 2.0 * mu) + var

    def acquire_integrated(self, y, t, refs, logWeights=None, bounds=None, mask=None, idx_offset=0, return_all=False):
        """The candidate of ``t`` (M, D; host array or device tensor, as in :meth:`acquire`) whose evaluation most
        reduces the integrated variance of the posterior estimate exp(f) (the expected integrated variance of
        Jarvenpaa et al. 2021), the integral taken over the reference points ``refs`` (J, D) with the log-weights
        ``logWeights`` (J; None: :meth:`integration_weights` for samples of the surrogate posterior):

            u(t) = -log sum_j exp(a_j + c_j(t)^2 / (var(t) + diag_add)),   c_j(t) = k(t, r_j) - k(t, X) K^-1 k(X, r_j)

        One prediction sweep gives var(t); B = K^-1 k(X, R) is solved once for all J columns against the resident
        factor (O(N^2 J), off the per-candidate path); one pass (``apgp_acquire_integrated``) forms all M x J posterior
        covariances and reduces them, O(N J) per candidate.  The GP is not modified.

        Returns ``(index, u)`` -- index -1 and +inf without an admissible candidate -- and with ``return_all``
        additionally the arrays ``(u, mu, var)``."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        if self.kernel.ndim > _lib.INTEGRATED_MAX_DIM:
            raise NotImplementedError("the integrated acquisition pass takes at most %d dimensions" % _lib.INTEGRATED_MAX_DIM)
        R = self._references(refs)
        J = len(R)
        if logWeights is None:
            a = self.integration_weights(y, R, "posterior")
        else:
            a = np.ascontiguousarray(np.asarray(logWeights, dtype=np.float64)).reshape(-1)
            if a.shape != (J,):
                raise ValueError("logWeights must have one entry per reference point")
        if np.any(np.isnan(a)) or np.any(a == np.inf) or not np.any(a > -np.inf):
            raise ValueError("logWeights must not be NaN or +inf, and not all -inf")
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n, D = len(self._x), self.kernel.ndim
        lo, hi = _box(bounds, D)
        T = self._candidates(t)
        m = T.shape[0]
        mask_d = self._mask(mask, m)
        if m == 0:
            return (-1, float("inf")) + ((np.empty(0),) * 3 if return_all else ())
        s = self._sweep(y, T, _lib.UTIL_NONE, idx_offset=idx_offset, with_mu=return_all, with_var=True)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            f64 = dict(dtype=torch.float64, device=dev)
            R_d = torch.from_numpy(R).to(dev)
            a_d = torch.from_numpy(a).to(dev)
            kxr = torch.empty((n, J), **f64)
            if self._x_d is None or self._x_d.shape[0] != n:
                self._x_d = torch.from_numpy(self._x).to(dev)
            _lib.check(lib.apgp_kernel_cross(self._x_d.data_ptr(), n, R_d.data_ptr(), J, ctypes.byref(ks),
                                             kxr.data_ptr(), J, st), "apgp_kernel_cross")
            # B = K^-1 k(X, R) = L^-T (L^-1 k(X, R)): all J right-hand sides at once (row-major (N, J): what the pass reads)
            L = torch.tril(self._L[:n, :n])                   # (bytes above the diagonal are undefined)
            z = torch.linalg.solve_triangular(L, kxr, upper=False)
            B = torch.linalg.solve_triangular(L.t(), z, upper=True).contiguous()
            u = torch.empty(m, **f64) if return_all else None
            part = torch.empty(max(int(lib.apgp_integrated_work_len(m, J)), 2), **f64)
            best = torch.empty(2, **f64)
            _lib.check(lib.apgp_acquire_integrated(T.data_ptr(), m, int(idx_offset), self._xs.data_ptr(), n,
                                                   ctypes.byref(ks), R_d.data_ptr(), J, B.data_ptr(), a_d.data_ptr(),
                                                   s.var.data_ptr(), lo, hi, _ptr(mask_d), None, 0, _ptr(u),
                                                   part.data_ptr(), best.data_ptr(), st), "apgp_acquire_integrated")
            rec = _best_record(best)
            if return_all:
                return rec + (u.cpu().numpy(), s.mu.cpu().numpy(), s.var.cpu().numpy())
        return rec

    # -- posterior function draws (DESIGN.md "Posterior function draws") ------------------
    def _path_call(self, T, ks, mean, paths, V, lo=None, hi=None, mask_d=None, idx_offset=0, with_f=False):
        """``apgp_path_draws`` over the rows of the device tensor ``T`` (M >= 1, D) with the weights of ``paths`` and the
        data weights ``V`` (None: the prior draws alone).  Returns (F (S, M) device or None, indices (S,), u (S,))."""
        torch, dev, lib = self._rt()
        m, S = T.shape[0], paths.size
        with self._on(torch, dev):
            st = self._stream(torch)
            f64 = dict(dtype=torch.float64, device=dev)
            F = torch.empty((S, m), **f64) if with_f else None
            part = torch.empty(max(int(lib.apgp_path_draws_work_len(m, S)), 2), **f64)
            best = torch.empty(2 * S, **f64)
            _lib.check(lib.apgp_path_draws(T.data_ptr(), m, int(idx_offset), _ptr(self._xs if V is not None else None),
                                           len(self._x), ctypes.byref(ks), float(mean), _ptr(V), paths.Z.data_ptr(),
                                           paths.b.data_ptr(), paths.W.data_ptr(), paths.Wl.data_ptr(),
                                           paths.nFeatures, S, lo, hi, _ptr(mask_d), _ptr(F), part.data_ptr(),
                                           best.data_ptr(), st), "apgp_path_draws")
            bb = best.cpu().numpy().reshape(S, 2)
        return F, bb[:, 1].copy().view(np.int64), bb[:, 0].copy()

    def sample_paths(self, y, size, nFeatures=2048):
        """``size`` functions drawn from the GP posterior given ``y``, as a :class:`PathDraws` that evaluates them --
        and finds each one's arg-max -- over any number of points in one device pass of O(N + nFeatures) per point and
        draw, with no N^2 contraction.  By Matheron's rule a posterior draw is a prior draw plus a data term,
        ``f_s(t) = mean + g_s(t) + k(t, X).v_s`` with ``v_s = K^-1 (y - mean - g_s(X) - eps_s)``; the squared-exponential
        part of the prior draw ``g_s`` is a sum of ``nFeatures`` random cosines (error O(nFeatures^-1/2) in
        distribution: it blurs the draws' covariance, not their mean -- the data term is exact), the linear term's
        feature map is exact.
        The random numbers come from NumPy's global stream, in the order Z (nFeatures x D), b (nFeatures), W (size x
        nFeatures), Wl (size x D), eps (size x N); the device only evaluates.  The set-up -- g_s(X) by the same kernel,
        then two triangular solves per draw against the resident factor (through the explicit inverse where
        :meth:`_trust_inverse` allows and it is resident, as ``_solve`` does) -- is O(size N^2), off the per-point path."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        size, nFeatures = int(size), int(nFeatures)
        if not 1 <= size <= _lib.MAX_DRAWS:
            raise ValueError("size must be between 1 and %d (APGP_MAX_DRAWS)" % _lib.MAX_DRAWS)
        if not 1 <= nFeatures <= _lib.MAX_FEATURES:
            raise ValueError("nFeatures must be between 1 and %d (APGP_MAX_FEATURES)" % _lib.MAX_FEATURES)
        y = self._check_dimensions(y)
        n, D = len(self._x), self.kernel.ndim
        diag_add = self._kernel_struct().diag_add
        Z = np.random.standard_normal((nFeatures, D))
        b = np.random.uniform(0.0, 2.0 * np.pi, nFeatures)
        W = np.random.standard_normal((size, nFeatures))
        Wl = np.random.standard_normal((size, D))
        eps = np.sqrt(diag_add) * np.random.standard_normal((size, n))
        return self._paths_from(y, Z, b, W, Wl, eps)

    def _paths_from(self, y, Z, b, W, Wl, eps):
        """The :class:`PathDraws` of given random numbers (host arrays, shapes as in :meth:`sample_paths`)."""
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n = len(self._x)
        self._ensure_xs(y)              # the packed training stream (and, where the gate allows, the resident L^-1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)       # noqa: E731
        paths = PathDraws(self, up(Z), up(b), up(W), up(Wl))
        S = paths.size
        via_w = self._work is not None and self._trust_inverse()
        np64 = (n + 63) // 64 * 64
        with self._on(torch, dev):
            st = self._stream(torch)
            f64 = dict(dtype=torch.float64, device=dev)
            G, _, _ = self._path_call(self._x_d, paths.ks, 0.0, paths, None, with_f=True)        # g_s(X), (S, N)
            rhs = (up(y) - float(self.mean.value)).unsqueeze(0) - G - up(eps)
            Vt = torch.empty((S, n), **f64)
            z, ss = torch.empty(n, **f64), torch.empty(1, **f64)
            wk = torch.empty(int(lib.apgp_winv_apply_work_len(n)), **f64) if via_w else None
            for s in range(S):
                if via_w:
                    w = self._work.data_ptr()
                    _lib.check(lib.apgp_winv_apply(w, np64, n, rhs[s].data_ptr(), 0.0, 0, z.data_ptr(), None, None, st),
                               "apgp_winv_apply(paths, forward)")
                    _lib.check(lib.apgp_winv_apply(w, np64, n, z.data_ptr(), 0.0, 1, Vt[s].data_ptr(), None,
                                                   wk.data_ptr(), st), "apgp_winv_apply(paths, backward)")
                else:
                    self._trsv(st, rhs[s], 0.0, 0, z, ss, "paths")
                    self._trsv(st, z, 0.0, 1, Vt[s], ss, "paths")
            paths.V = Vt.t().contiguous()                     # (N, S): a training row's S weights side by side
        return paths

    def thompson_batch(self, y, t, q, bounds=None, mask=None, idx_offset=0, nFeatures=2048, maxRounds=4,
                       return_draws=False):
        """``q`` distinct candidates of ``t`` (M, D; host array or device tensor, as in :meth:`acquire`) chosen by
        Thompson sampling: each is the arg-max of one function drawn from the posterior (:meth:`sample_paths`), in
        draw order.  A round draws min(APGP_MAX_DRAWS, 2 x the missing slots) functions and evaluates them over all
        candidates in one launch; a winner already in the batch is skipped.  After ``maxRounds`` rounds the remaining
        slots are -1 -- a concentrated posterior legitimately keeps electing the same row.  The GP is not modified.
        Returns the global indices (q,) int64; ``return_draws`` adds the (round, draw) pair that elected each slot."""
        q = int(q)
        if not 1 <= q <= _lib.MAX_DRAWS:
            raise ValueError("q must be between 1 and %d (APGP_MAX_DRAWS)" % _lib.MAX_DRAWS)
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        T = self._candidates(t)
        mask_d = self._mask(mask, T.shape[0])
        idx, draws = [], []
        for rnd in range(int(maxRounds)):
            if len(idx) == q or T.shape[0] == 0:
                break
            paths = self.sample_paths(y, min(_lib.MAX_DRAWS, 2 * (q - len(idx))), nFeatures)
            winners, _ = paths.argmax(T, bounds=bounds, mask=mask_d, idx_offset=idx_offset)
            for s, g in enumerate(winners.tolist()):
                if g >= 0 and g not in idx and len(idx) < q:
                    idx.append(g)
                    draws.append((rnd, s))
        out = np.full(q, -1, dtype=np.int64)
        out[:len(idx)] = idx
        return (out, draws) if return_draws else out

    # -- candidate matrix of the sweep drawn on the device -----------------------------
    def box_candidates(self, m, bounds, seed, idx_offset=0):
        """Rows ``idx_offset .. idx_offset + m - 1`` of the global candidate matrix ``U[bounds]`` keyed by ``seed``
        (counter-based Philox: a row depends on (seed, row number) only), as a device tensor (m, D) ready for
        :meth:`acquire` -- the batched counterpart of the ``sampleFn`` draws utility.minimizeObjective starts from
        (utility.py:334-338) without the host draw and the H2D copy (26 ms per 1e6 x 8 against an 18 ms sweep)."""
        torch, dev, lib = self._rt()
        D = self.kernel.ndim
        lo, hi = _box(bounds, D, optional=False)
        with self._on(torch, dev):
            T = torch.empty((int(m), D), dtype=torch.float64, device=dev)
            if int(m) == 0:
                return T
            _lib.check(lib.apgp_box_candidates(T.data_ptr(), int(m), D, lo, hi, _seed64(seed),
                                               int(idx_offset), self._stream(torch)), "apgp_box_candidates")
        return T

    @staticmethod
    def _prior_records(prior, D):
        kind, p0, p1 = prior.records()
        if len(kind) != D:
            raise ValueError("the prior must have one factor per dimension")
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        p0 = np.ascontiguousarray(p0, dtype=np.float64)
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        return kind, p0, p1

    def prior_candidates(self, m, prior, seed, idx_offset=0):
        """Rows ``idx_offset .. idx_offset + m - 1`` of the global candidate matrix drawn from ``prior`` (a
        :class:`~approxposterior_amd.priors.JointPrior`) keyed by ``seed``, as a device tensor (m, D) ready for
        :meth:`acquire`.  Same stream as :meth:`box_candidates`: a Uniform dimension is bit-identical to the box
        draw of the same row; a Gaussian dimension is the factor's inverse CDF at the same uniform."""
        torch, dev, lib = self._rt()
        D = self.kernel.ndim
        kind, p0, p1 = self._prior_records(prior, D)
        with self._on(torch, dev):
            T = torch.empty((int(m), D), dtype=torch.float64, device=dev)
            if int(m) == 0:
                return T
            _lib.check(lib.apgp_prior_candidates(T.data_ptr(), int(m), D, kind.ctypes.data, p0.ctypes.data,
                                                 p1.ctypes.data, _seed64(seed), int(idx_offset),
                                                 self._stream(torch)), "apgp_prior_candidates")
        return T

    # -- evidence by importance sampling (DESIGN.md "Evidence by importance sampling") ------
    @staticmethod
    def _mixture_params(weights, means, covariances, covScale):
        """The host record of ``apgp_mix_candidates`` (include/apgp.h) of a full-covariance mixture: per component the
        cumulative weight (summed sequentially, the last forced to 1.0), the ``apgp_gmm_pass`` record (log weight,
        log det U, centre, U packed) and the lower Cholesky factor A of ``covScale`` x covariance packed row by row."""
        w = np.asarray(weights, dtype=np.float64).ravel()
        mu = np.atleast_2d(np.asarray(means, dtype=np.float64))
        cov = np.asarray(covariances, dtype=np.float64)
        K, D = mu.shape
        if w.shape != (K,) or cov.shape != (K, D, D):
            raise ValueError("a mixture needs weights (K,), means (K, D) and full covariances (K, D, D)")
        if not 1 <= K <= _lib.GMM_MAX_COMP:
            raise ValueError("a mixture proposal has between 1 and %d components" % _lib.GMM_MAX_COMP)
        if not (np.all(np.isfinite(w)) and np.all(w >= 0.0) and w.sum() > 0.0 and float(covScale) > 0.0):
            raise ValueError("mixture weights must be finite and non-negative with a positive sum, covScale positive")
        w = w / w.sum()
        cum = np.empty(K)
        run = 0.0
        for k in range(K):
            run = min(run + w[k], 1.0)
            cum[k] = run
        cum[K - 1] = 1.0
        iu, ju = _triu_colmajor(D)
        il, jl = np.tril_indices(D)
        rec = np.empty((K, 3 + D + D * (D + 1)))
        with np.errstate(divide="ignore"):
            logw = np.log(w)
        for k in range(K):
            try:
                A = np.linalg.cholesky(float(covScale) * cov[k])
            except np.linalg.LinAlgError:
                raise ValueError("covariance %d of the mixture is not positive definite" % k)
            if not np.all(np.isfinite(A)):
                raise ValueError("covariance %d of the mixture is not positive definite" % k)
            U = solve_triangular(A, np.eye(D), lower=True).T        # precision = U U^T
            rec[k] = np.concatenate([[cum[k], logw[k], np.sum(np.log(np.diag(U)))], mu[k], U[iu, ju], A[il, jl]])
        return K, D, rec

    def mixture_candidates(self, m, weights, means, covariances, seed, idx_offset=0, covScale=1.0):
        """Rows ``idx_offset .. idx_offset + m - 1`` of the global matrix of draws from the Gaussian mixture
        (``weights`` (K,), ``means`` (K, D), full ``covariances`` (K, D, D) scaled by ``covScale``) keyed by ``seed``
        -- a row depends on (seed, row number) only -- and the mixture's log-density at every draw: device tensors
        ``(T (m, D), lnq (m,))``.  The factors come from NumPy on the host; ``ValueError`` for a covariance that is not
        positive definite."""
        torch, dev, lib = self._rt()
        K, D, rec = self._mixture_params(weights, means, covariances, covScale)
        if D != self.kernel.ndim:
            raise ValueError("the mixture must have the GP's dimension")
        m = int(m)
        with self._on(torch, dev):
            T = torch.empty((m, D), dtype=torch.float64, device=dev)
            lnq = torch.empty(m, dtype=torch.float64, device=dev)
            if m == 0:
                return T, lnq
            rec = np.ascontiguousarray(rec.ravel())
            assert rec.size == lib.apgp_mix_params_len(D, K)
            _lib.check(lib.apgp_mix_candidates(T.data_ptr(), lnq.data_ptr(), m, D, K, rec.ctypes.data, _seed64(seed),
                                               int(idx_offset), self._stream(torch)), "apgp_mix_candidates")
        return T, lnq

    # -- quasi-random draws (DESIGN.md "Quasi-random draws") ---------------------------------
    def sobol_candidates(self, m, bounds=None, prior=None, mixture=None, seed=0, replicate=0, scramble=True,
                         idx_offset=0, covScale=1.0):
        """Rows ``idx_offset .. idx_offset + m - 1`` of replicate ``replicate`` of the scrambled Sobol sequence keyed by
        ``seed``, pushed through the transform of exactly one source: ``bounds`` (the box of :meth:`box_candidates`),
        ``prior`` (a :class:`~approxposterior_amd.priors.JointPrior`, as :meth:`prior_candidates`) or ``mixture``
        (``(weights, means, covariances)``, covariances scaled by ``covScale``, as :meth:`mixture_candidates`: Sobol
        dimensions 0 .. D - 1 give the normals, dimension D the component).  Returns the device tensor ``T (m, D)``, or
        ``(T, lnq (m,))`` for a mixture.  A row depends on (seed, replicate, row number) only, so sharding by
        ``idx_offset``, chunking and regenerating one row work as for the Philox draws.  ``scramble=False`` is the plain
        sequence (torch's ``SobolEngine``, whose row 0 is the origin).  The sequence has 2^30 rows."""
        if (bounds is not None) + (prior is not None) + (mixture is not None) != 1:
            raise ValueError("sobol_candidates draws from exactly one of bounds, prior and mixture")
        torch, dev, lib = self._rt()
        with self._on(torch, dev):
            return _sobol_draw(torch, dev, lib, self._stream(torch), int(m), self.kernel.ndim, bounds, prior, mixture,
                               seed, replicate, scramble, idx_offset, covScale)

    def prior_lnprior(self, T, prior):
        """``prior``'s log-density (a :class:`~approxposterior_amd.priors.JointPrior`) at the rows of the device
        tensor ``T`` (M, D), as a device tensor (M,)."""
        torch, dev, lib = self._rt()
        T = self._candidates(T)
        kind, p0, p1 = self._prior_records(prior, self.kernel.ndim)
        with self._on(torch, dev):
            out = torch.empty(T.shape[0], dtype=torch.float64, device=dev)
            if T.shape[0]:
                _lib.check(lib.apgp_prior_lnprior(T.data_ptr(), T.shape[0], self.kernel.ndim, kind.ctypes.data,
                                                  p0.ctypes.data, p1.ctypes.data, out.data_ptr(), self._stream(torch)),
                           "apgp_prior_lnprior")
        return out

    def importance_pass(self, y, T, lnq=None, bounds=None, centre=None, return_logw=False):
        """One importance-sampling record over the rows of ``T`` (M >= 1, D; host array or device tensor) drawn from a
        proposal with log-density ``lnq`` (M,; device tensor or host array; None: zeros):
        ``logw = mu(t) - lnq`` where every coordinate is finite and inside ``bounds`` and ``mu`` and ``lnq`` are finite,
        else -inf.  Returns a dict of NumPy values -- ``lmax``, ``S0 = sum e``, ``S2 = sum e^2``, ``cnt``, ``s1 = sum e
        (t - c)``, ``S = sum e (t - c)(t - c)^T`` (D, D), ``centre`` -- with ``e = exp(logw - lmax)`` and ``c`` =
        ``centre`` (default: the training point with the largest ``y``); ``utility.importanceSummary`` reads it,
        ``utility.mergeImportance`` joins two.  ``return_logw`` adds the device tensor of ``logw``.  One device pass:
        the means, the weights and the moments never visit the host."""
        torch, dev, lib = self._rt()
        y, T, m, c, lo, hi = self._importance_args(y, T, centre, bounds, "importance_pass")
        D = self.kernel.ndim
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            f64 = dict(dtype=torch.float64, device=dev)
            lnq = self._importance_lnq(torch, dev, lnq, m)
            logw = torch.empty(m, **f64) if return_logw else None
            nstat = int(lib.apgp_importance_stats_len(D))
            stats = torch.empty(nstat, **f64)
            need = int(lib.apgp_importance_work_len(m)) - (m if return_logw else 0)
            if self._imp_work is None or self._imp_work.numel() < need:
                self._imp_work = torch.empty(need, **f64)
            cc = (ctypes.c_double * _lib.MAX_DIM)(*c)
            _lib.check(lib.apgp_importance_pass(T.data_ptr(), m, _ptr(lnq), self._xs.data_ptr(), len(self._x),
                                                ctypes.byref(ks), float(self.mean.value), lo, hi,
                                                ctypes.addressof(cc), _ptr(logw), stats.data_ptr(),
                                                self._imp_work.data_ptr(), st), "apgp_importance_pass")
            r = stats.cpu().numpy()
        rec = self._importance_record(r, c)
        return (rec, logw) if return_logw else rec

    def _importance_args(self, y, T, centre, bounds, who):
        """The checked arguments the importance passes share: (y, T on the device, M, centre (D,), lo, hi)."""
        if not self.computed:
            raise RuntimeError("ERROR: Need to compute GP before using it!")
        y = self._check_dimensions(y)
        D = self.kernel.ndim
        T = self._candidates(T)
        m = int(T.shape[0])
        if m < 1:
            raise ValueError("%s needs at least one row" % who)
        c = np.array(self._x[int(np.argmax(y))] if centre is None else centre, dtype=np.float64).ravel()
        if c.shape != (D,) or not np.all(np.isfinite(c)):
            raise ValueError("centre must be D finite numbers")
        lo, hi = _box(bounds, D)
        return y, T, m, c, lo, hi

    @staticmethod
    def _importance_lnq(torch, dev, lnq, m):
        """``lnq`` as the importance passes take it: None, or a contiguous (M,) float64 tensor on the device."""
        if lnq is not None and not hasattr(lnq, "data_ptr"):
            lnq = torch.from_numpy(np.ascontiguousarray(lnq, dtype=np.float64)).to(dev)
        if lnq is not None and (tuple(lnq.shape) != (m,) or str(lnq.dtype) != "torch.float64" or not lnq.is_cuda
                                or not lnq.is_contiguous()):
            raise ValueError("lnq must be a contiguous (M,) float64 tensor on the device")
        return lnq

    @staticmethod
    def _importance_record(r, c):
        """The record dict of one ``[lmax, S0, S2, cnt, s1 (D), S packed]`` row of the device's statistics."""
        D = len(c)
        iu, ju = _triu_colmajor(D)
        S = np.zeros((D, D))
        S[iu, ju] = r[4 + D:]
        S[ju, iu] = r[4 + D:]
        return {"lmax": float(r[0]), "S0": float(r[1]), "S2": float(r[2]), "cnt": float(r[3]), "s1": r[4:4 + D].copy(),
                "S": S, "centre": c}

    def importance_paths(self, y, T, paths, lnq=None, bounds=None, centre=None, return_logw=False):
        """One importance-sampling record PER POSTERIOR FUNCTION DRAW of ``paths`` (:meth:`sample_paths`) over the rows
        of ``T``: :meth:`importance_pass` with the draw ``f_s`` in place of the mean, ``logw_s = f_s(t) - lnq`` where
        every coordinate is finite and inside ``bounds`` and ``f_s`` and ``lnq`` are finite, else -inf.  Returns a list
        of ``paths.size`` record dicts with :meth:`importance_pass`'s keys, taken about the same ``centre``; their
        scatter over the draws is the surrogate's own uncertainty about the evidence and the posterior moments
        (``utility.importanceDrawsSummary``).  ``return_logw`` adds the (S, M) device tensor of the log-weights.
        One fused device pass (``apgp_path_importance``): the S x M matrix of draw values is never stored unless
        ``return_logw`` asks for the weights, and nothing visits the host but the S records.  The arguments are
        checked as :meth:`importance_pass` checks them; draws that belong to a factor the GP no longer holds are
        refused as :meth:`PathDraws.evaluate` refuses them."""
        torch, dev, lib = self._rt()
        if not isinstance(paths, PathDraws) or paths.gp is not self:
            raise ValueError("importance_paths needs the PathDraws of this GP's sample_paths")
        paths._check_current()
        y, T, m, c, lo, hi = self._importance_args(y, T, centre, bounds, "importance_paths")
        S = paths.size
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            f64 = dict(dtype=torch.float64, device=dev)
            lnq = self._importance_lnq(torch, dev, lnq, m)
            logw = torch.empty((S, m), **f64) if return_logw else None
            nstat = int(lib.apgp_importance_stats_len(self.kernel.ndim))
            stats = torch.empty((S, nstat), **f64)
            need = int(lib.apgp_path_importance_work_len(m, S)) - (S * m if return_logw else 0)
            if self._pimp_work is None or self._pimp_work.numel() < need:
                self._pimp_work = torch.empty(need, **f64)
            cc = (ctypes.c_double * _lib.MAX_DIM)(*c)
            V = paths.V
            _lib.check(lib.apgp_path_importance(T.data_ptr(), m, _ptr(lnq), _ptr(self._xs if V is not None else None),
                                                len(self._x), ctypes.byref(paths.ks), float(paths.mean), _ptr(V),
                                                paths.Z.data_ptr(), paths.b.data_ptr(), paths.W.data_ptr(),
                                                paths.Wl.data_ptr(), paths.nFeatures, S, lo, hi, ctypes.addressof(cc),
                                                _ptr(logw), stats.data_ptr(), self._pimp_work.data_ptr(), st),
                       "apgp_path_importance")
            r = stats.cpu().numpy()
        recs = [self._importance_record(r[s], c) for s in range(S)]
        return (recs, logw) if return_logw else recs

    # -- on-device ensemble MCMC over the GP mean ------------------------------------
    def sample_ensemble(self, y, initial_state, iterations, bounds, a=2.0, seed=0, store=True, prior=None,
                        keep_device=False, moves=None):
        """Run the stretch-move ensemble sampler entirely on the device with
        log-probability = GP mean (what ApproxPosterior._gpll returns) and the box
        prior ``bounds``.  ``initial_state`` is (W, D) for one ensemble or (E, W, D)
        for E independent ensembles (one workgroup each).  Returns a dict with
        ``chain`` (iterations, E*W, D), ``log_prob`` (iterations, E*W), ``coords``,
        ``final_log_prob`` and ``naccept``.

        ``prior``: a :class:`~approxposterior_amd.priors.JointPrior`.  The walkers are then gated by
        ``prior.support()`` (``bounds`` is not used) and, with ``store``, the result also has ``blobs``
        (iterations, E*W): the prior's log-density at every stored state, NaN where it is -inf, as
        ``ApproxPosterior._gpllBatch`` returns for a rejected walker.

        ``keep_device``: with ``store``, the result also has ``chain_device``, the device tensor (iterations, E*W, D)
        that ``chain`` was copied from (``DeviceChain.get_autocorr_time`` then reads it in place).

        ``moves``: what ``mcmc.EnsembleSampler(moves=...)`` accepts -- a ``mcmc.StretchMove``, ``DEMove`` or
        ``DESnookerMove``, a list of them or of ``(move, weight)`` pairs; one move is drawn per iteration for the whole
        ensemble (``apgp_ensemble_sample_moves``).  ``None`` is the stretch move at ``a``; ``a`` other than 2.0 beside
        ``moves`` is a ``ValueError``.  The snooker's norms are taken in the kernel's scaled coordinates."""
        self.recompute()
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        p0 = np.ascontiguousarray(np.asarray(initial_state, dtype=np.float64))
        D = self.kernel.ndim
        if p0.ndim == 1:
            p0 = p0.reshape(-1, D)
        if p0.ndim == 2:
            p0 = p0[None]
        if p0.ndim != 3 or p0.shape[2] != D:
            raise ValueError("initial_state must be (W, D) or (E, W, D)")
        if not np.all(np.isfinite(p0)):
            raise ValueError("At least one parameter value was NaN or infinite")
        E, W, _ = p0.shape
        if prior is not None:
            records = self._prior_records(prior, D)
            bounds = prior.support()
        lo, hi = _box(bounds, D, optional=False)
        n = len(self._x)
        ks = self._kernel_struct()
        iterations = int(iterations)
        table, ntable = None, 0
        if moves is not None:
            from . import mcmc
            pairs = mcmc.move_table(moves, W, a)
            table, ntable = (_lib.EnsMove * len(pairs))(), len(pairs)
            for rec, (mv, w) in zip(table, pairs):
                rec.kind, rec.p0, rec.p1 = mv.record(D)
                rec.weight = w
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            coords = torch.from_numpy(p0).to(dev)
            logp = torch.empty((E, W), dtype=torch.float64, device=dev)
            nacc = torch.empty((E, W), dtype=torch.int64, device=dev)
            chain = torch.empty((iterations, E, W, D), dtype=torch.float64, device=dev) if store else None
            lchain = torch.empty((iterations, E, W), dtype=torch.float64, device=dev) if store else None
            def launch(mode):
                coords.copy_(torch.from_numpy(p0))
                args = (self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), lo, hi, W, E,
                        iterations, float(a), _seed64(seed), coords.data_ptr(), logp.data_ptr(),
                        chain.data_ptr() if store else None, lchain.data_ptr() if store else None,
                        nacc.data_ptr(), mode)
                if table is None:
                    _lib.check(lib.apgp_ensemble_sample_ex(*args, st), "apgp_ensemble_sample")
                else:
                    _lib.check(lib.apgp_ensemble_sample_moves(*args, table, ntable, st), "apgp_ensemble_sample_moves")
                return logp.cpu().numpy().reshape(E * W)
            final = launch(-1)
            if np.any(np.isnan(final)):
                # the multi-workgroup launch could not get its workgroups resident (another stream or process holds
                # compute units; the launch's sticky word turned every log-probability into NaN): once more on the
                # single-workgroup kernel -- slower, same posterior -- chosen for THIS call only (no process-wide switch
                # is flipped under other threads' calls)
                self.ensemble_fallbacks = getattr(self, "ensemble_fallbacks", 0) + 1
                final = launch(1)
                if np.any(np.isnan(final)):
                    raise FloatingPointError("the ensemble sampler returned NaN log-probabilities on both of its kernels: "
                                             "the GP mean is not finite at the walkers' positions")
            out = {"coords": coords.cpu().numpy().reshape(E * W, D),
                   "final_log_prob": final,
                   "naccept": nacc.cpu().numpy().reshape(E * W),
                   "chain": chain.cpu().numpy().reshape(iterations, E * W, D) if store else None,
                   "log_prob": lchain.cpu().numpy().reshape(iterations, E * W) if store else None}
            if keep_device and store:
                out["chain_device"] = chain.view(iterations, E * W, D)
            if prior is not None and store:
                # the lnprior blobs: one pass of the prior's log-density over the stored chain
                lp = torch.empty(iterations * E * W, dtype=torch.float64, device=dev)
                if iterations:
                    kind, q0, q1 = records
                    _lib.check(lib.apgp_prior_lnprior(chain.data_ptr(), iterations * E * W, D, kind.ctypes.data,
                                                      q0.ctypes.data, q1.ctypes.data, lp.data_ptr(), st),
                               "apgp_prior_lnprior")
                blobs = lp.cpu().numpy().reshape(iterations, E * W)
                out["blobs"] = np.where(np.isneginf(blobs), np.nan, blobs)
        return out

    def sample_tempered(self, y, initial_state, iterations, bounds, betas, swapEvery=10, seed=0, ladders=1, storeRungs=1,
                        moves=None, prior=None, keep_device=False, swapLog=False):
        """Parallel tempering of :meth:`sample_ensemble` on the device (``apgp_tempered_sample``): ``ladders``
        independent ladders of ``len(betas)`` ensembles ("rungs"); rung k samples ``exp(betas[k] * mu)`` on the box
        with the moves of :meth:`sample_ensemble`, and neighbouring rungs propose to exchange walkers every
        ``swapEvery`` iterations.  ``betas`` starts at 1 (the cold rung is the posterior), stays in [0, 1] and does
        not increase; a final 0 -- the rung that samples the box uniformly, which needs finite ``bounds`` -- makes
        ``mcmc.TemperedChain.log_evidence`` possible.

        ``initial_state`` is (W, D), used for every rung, (T, W, D), used for every ladder, or (L, T, W, D).
        Returns the keys of :meth:`sample_ensemble` for the cold rungs, the ladders' side by side on the walker axis
        (``chain`` (iterations, L*W, D), ``log_prob``, ``coords``, ``final_log_prob``, ``naccept``; ``blobs`` with
        ``prior``, ``chain_device`` with ``keep_device``), and ``betas``, ``rung_naccept`` (L, T, W), ``swap_proposed``
        and ``swap_accepted`` (L, T - 1), ``rung_mean_log_prob`` (iterations, L, T) -- the walker mean of mu per rung,
        reduced on the device --, ``rung_coords`` (L, T, W, D), ``rung_final_log_prob`` (L, T, W), ``swap_every``.
        ``storeRungs=S`` > 1 also stores rungs 0 .. S - 1: ``rung_chain`` (iterations, L, S, W, D) and
        ``rung_log_prob`` (iterations, L, S, W).  ``swapLog`` adds ``swap_log`` (rounds, L, T - 1, W) uint8: 0 = not
        proposed, 1 = rejected, 2 = accepted.  ``moves`` and ``prior`` as for :meth:`sample_ensemble`."""
        self.recompute()
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        D = self.kernel.ndim
        betas = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).ravel())
        T, L, S = len(betas), int(ladders), int(storeRungs)
        if T < 1 or betas[0] != 1.0:
            raise ValueError("betas must start at 1: the cold rung is the posterior")
        if L < 1:
            raise ValueError("ladders must be at least 1")
        if not 1 <= S <= T:
            raise ValueError("storeRungs must lie between 1 and the number of rungs")
        p0 = np.asarray(initial_state, dtype=np.float64)
        if p0.ndim not in (2, 3, 4) or p0.shape[-1] != D or (p0.ndim >= 3 and p0.shape[-3] != T) or \
                (p0.ndim == 4 and p0.shape[0] != L):
            raise ValueError("initial_state must be (W, D), (T, W, D) or (L, T, W, D)")
        W = p0.shape[-2]
        # (a writable copy in C order: the default order of a copy follows the broadcast view's zero strides)
        p0 = np.array(np.broadcast_to(p0, (L, T, W, D)), order="C")
        if not np.all(np.isfinite(p0)):
            raise ValueError("At least one parameter value was NaN or infinite")
        if prior is not None:
            records = self._prior_records(prior, D)
            bounds = prior.support()
        lo, hi = _box(bounds, D, optional=False)
        n = len(self._x)
        ks = self._kernel_struct()
        iterations, swapEvery = int(iterations), int(swapEvery)
        if swapEvery < 1:
            raise ValueError("swapEvery must be at least 1")
        rounds = max(0, -(-iterations // swapEvery) - 1)
        table, ntable = None, 0
        if moves is not None:
            from . import mcmc
            pairs = mcmc.move_table(moves, W)
            table, ntable = (_lib.EnsMove * len(pairs))(), len(pairs)
            for rec, (mv, w) in zip(table, pairs):
                rec.kind, rec.p0, rec.p1 = mv.record(D)
                rec.weight = w
        need = int(lib.apgp_tempered_work_len(W, T, L, D))
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
            coords = torch.from_numpy(p0).to(dev)
            logp = torch.empty((L, T, W), **f64)
            nacc = torch.empty((L, T, W), **i64)
            chain = torch.empty((iterations, L, S, W, D), **f64)
            lchain = torch.empty((iterations, L, T, W), **f64)
            sprop, sacc = torch.zeros((L, max(T - 1, 1)), **i64), torch.zeros((L, max(T - 1, 1)), **i64)
            slog = torch.zeros((rounds, L, max(T - 1, 1), W), dtype=torch.uint8, device=dev) if swapLog else None
            work = torch.empty(max(need, 1), **f64)
            bb = (ctypes.c_double * T)(*betas)
            _lib.check(lib.apgp_tempered_sample(self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), lo, hi,
                                                W, T, L, bb, iterations, swapEvery, _seed64(seed), coords.data_ptr(),
                                                logp.data_ptr(), chain.data_ptr(), S, lchain.data_ptr(), nacc.data_ptr(),
                                                sprop.data_ptr(), sacc.data_ptr(), _ptr(slog), table, ntable,
                                                work.data_ptr(), st), "apgp_tempered_sample")
            final = logp.cpu().numpy()
            if np.any(np.isnan(final)):
                raise FloatingPointError("the tempered sampler returned NaN log-probabilities: the GP mean is not finite at "
                                         "the walkers' positions")
            cold = chain[:, :, 0].contiguous() if S > 1 else chain.view(iterations, L, W, D)
            rc = coords.cpu().numpy()
            rn = nacc.cpu().numpy()
            out = {"coords": rc[:, 0].reshape(L * W, D), "final_log_prob": final[:, 0].reshape(L * W),
                   "naccept": rn[:, 0].reshape(L * W),
                   "chain": cold.cpu().numpy().reshape(iterations, L * W, D),
                   "log_prob": lchain[:, :, 0].cpu().numpy().reshape(iterations, L * W),
                   "betas": betas.copy(), "swap_every": swapEvery, "rung_naccept": rn, "rung_coords": rc,
                   "rung_final_log_prob": final,
                   "swap_proposed": sprop.cpu().numpy()[:, :T - 1], "swap_accepted": sacc.cpu().numpy()[:, :T - 1],
                   "rung_mean_log_prob": lchain.mean(dim=3).cpu().numpy()}
            span = np.array([hi[d] - lo[d] for d in range(D)])
            if np.all(np.isfinite(span)) and np.all(span > 0.0):
                out["log_volume"] = float(np.sum(np.log(span)))
            if S > 1:
                out["rung_chain"] = chain.cpu().numpy()
                out["rung_log_prob"] = lchain[:, :, :S].cpu().numpy()
            if swapLog:
                out["swap_log"] = slog.cpu().numpy()[:, :, :T - 1]
            if keep_device:
                out["chain_device"] = cold.view(iterations, L * W, D)
            if prior is not None:
                lp = torch.empty(iterations * L * W, **f64)
                if iterations:
                    kind, q0, q1 = records
                    _lib.check(lib.apgp_prior_lnprior(cold.data_ptr(), iterations * L * W, D, kind.ctypes.data,
                                                      q0.ctypes.data, q1.ctypes.data, lp.data_ptr(), st),
                               "apgp_prior_lnprior")
                blobs = lp.cpu().numpy().reshape(iterations, L * W)
                out["blobs"] = np.where(np.isneginf(blobs), np.nan, blobs)
        return out

    def hmc_scale(self):
        """``sc`` (D,): the factor between the user's coordinates and the scaled coordinates ``q = theta * sc`` in which
        :meth:`sample_hmc` takes ``eps`` and integrates (``sc_d = sqrt(inv_metric_d / 2)``: the squared-exponential
        term is ``amp * exp(-|q - q'|^2)`` there)."""
        ks = self._kernel_struct()
        return np.sqrt(0.5 * np.array(ks.inv_metric[:ks.ndim], dtype=np.float64))

    def sample_hmc(self, y, initial_state, iterations, bounds, eps, nLeap, jitter=0.1, mass=None, seed=0, iteration0=0,
                   prior=None, keep_device=False, store=True, debug=False, gRows=0):
        """Hamiltonian Monte Carlo over the surrogate, whole chains on the device (``apgp_hmc_sample``): the target of
        :meth:`sample_ensemble` -- density ``exp(mu)`` on the box ``bounds`` (edges may be infinite), or on
        ``prior.support()`` under a :class:`~approxposterior_amd.priors.JointPrior` -- sampled by ``C`` independent
        chains started at ``initial_state`` (C, D), with the exact gradient of the predictive mean.

        One iteration draws a Gaussian momentum, takes ``nLeap`` leapfrog steps of size ``eps * (1 + jitter * (2u - 1))``
        (one ``u`` per iteration, the same for every chain), reflecting at the finite faces of the box, and accepts
        with probability ``min(1, exp(-dH))``.  ``eps`` is a step in the kernel's SCALED coordinates ``theta * sc``
        (:meth:`hmc_scale`), in which the GP's length scales are all 1 / sqrt(2); ``mass`` (D,) is a diagonal mass in
        the USER's coordinates (converted with ``sc``) and defaults to the identity in scaled coordinates, which makes
        the GP's own length scales the preconditioner.  The random numbers of chain c at global iteration
        ``iteration0 + it`` depend on ``(seed, c, iteration0 + it)`` only: a run cut into calls with consecutive
        ``iteration0``, each fed the previous ``coords``, is the uncut run, bit for bit.

        Returns the dict of :meth:`sample_ensemble` (``chain`` (iterations, C, D), ``log_prob``, ``coords``,
        ``final_log_prob``, ``naccept``; ``blobs`` with ``prior``; ``chain_device`` with ``keep_device``) and
        ``accept_prob`` (C,: the mean of ``min(1, exp(-dH))``), ``ndiverge`` (C,: trajectories rejected for a
        non-finite energy error, one above 1000 or a reflection that did not end), ``eps``, ``g_rows``.  ``debug``
        adds ``proposals`` (iterations, C, D), ``dH`` (iterations, C) and ``trace`` (iterations, C, nLeap, 2, D): q and
        p after every leapfrog step in scaled coordinates.  ``gRows``: wavefronts per chain, 0 = the library's rule."""
        D = self.kernel.ndim
        p0 = np.ascontiguousarray(np.asarray(initial_state, dtype=np.float64))
        if p0.ndim == 1:
            p0 = p0.reshape(-1, D)
        if p0.ndim != 2 or p0.shape[1] != D or p0.shape[0] < 1:
            raise ValueError("initial_state must be (C, D)")
        if not np.all(np.isfinite(p0)):
            raise ValueError("At least one parameter value was NaN or infinite")
        C = p0.shape[0]
        iterations, nLeap, gRows, iteration0 = int(iterations), int(nLeap), int(gRows), int(iteration0)
        eps, jitter = float(eps), float(jitter)
        if iterations < 0:
            raise ValueError("iterations must be >= 0")
        if not (np.isfinite(eps) and eps > 0.0):
            raise ValueError("eps must be finite and > 0")
        if not 0.0 <= jitter < 1.0:
            raise ValueError("jitter must lie in [0, 1)")
        if not 1 <= nLeap <= _lib.HMC_MAX_LEAP:
            raise ValueError("nLeap must lie between 1 and %d" % _lib.HMC_MAX_LEAP)
        if gRows != 0 and gRows not in _lib.HMC_G_ROWS:
            raise ValueError("gRows must be 0 (the library's rule) or one of %s" % (_lib.HMC_G_ROWS,))
        if iteration0 < 0:
            raise ValueError("iteration0 must be >= 0")
        if mass is not None:
            mass = np.asarray(mass, dtype=np.float64).ravel()
            if mass.shape != (D,) or not np.all(np.isfinite(mass)) or not np.all(mass > 0.0):
                raise ValueError("mass must be D finite positive numbers (a diagonal mass in the user's coordinates)")
        if prior is not None:
            records = self._prior_records(prior, D)
            bounds = prior.support()
        lo, hi = _box(bounds, D, optional=False)
        if any(not lo[d] <= hi[d] for d in range(D)):
            raise ValueError("bounds: every low edge must be <= its high edge")
        self.recompute()
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n = len(self._x)
        ks = self._kernel_struct()
        opt = _lib.HmcOptions()
        opt.eps, opt.jitter, opt.nleap, opt.g_rows, opt.iteration0 = eps, jitter, nLeap, gRows, iteration0
        sc = self.hmc_scale()
        ms = np.ones(D) if mass is None else mass / (sc * sc)
        if not (np.all(np.isfinite(ms)) and np.all(ms > 0.0)):
            raise ValueError("mass is not finite and positive in the kernel's scaled coordinates")
        opt.mass[:D] = ms.tolist()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
            coords = torch.from_numpy(p0).to(dev)
            logp, accp = torch.empty(C, **f64), torch.empty(C, **f64)
            nacc, ndiv = torch.empty(C, **i64), torch.empty(C, **i64)
            chain = torch.empty((iterations, C, D), **f64) if store else None
            lchain = torch.empty((iterations, C), **f64) if store else None
            prop = torch.empty((iterations, C, D), **f64) if debug else None
            dH = torch.empty((iterations, C), **f64) if debug else None
            trace = torch.empty((iterations, C, nLeap, 2, D), **f64) if debug else None
            _lib.check(lib.apgp_hmc_sample(self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), lo, hi, C,
                                           iterations, ctypes.byref(opt), _seed64(seed), coords.data_ptr(), logp.data_ptr(),
                                           _ptr(chain), _ptr(lchain), nacc.data_ptr(), accp.data_ptr(), ndiv.data_ptr(),
                                           _ptr(prop), _ptr(dH), _ptr(trace), st), "apgp_hmc_sample")
            final = logp.cpu().numpy()
            if np.any(np.isnan(final)):
                raise FloatingPointError("the HMC sampler returned NaN log-probabilities: the GP mean is not finite at the "
                                         "chains' positions")
            out = {"coords": coords.cpu().numpy(), "final_log_prob": final, "naccept": nacc.cpu().numpy(),
                   "chain": chain.cpu().numpy() if store else None,
                   "log_prob": lchain.cpu().numpy() if store else None,
                   "accept_prob": accp.cpu().numpy() / max(iterations, 1), "ndiverge": ndiv.cpu().numpy(),
                   "eps": eps, "g_rows": gRows if gRows else int(lib.apgp_hmc_rule(C, n, D))}
            if debug:
                out["proposals"], out["dH"], out["trace"] = prop.cpu().numpy(), dH.cpu().numpy(), trace.cpu().numpy()
            if keep_device and store:
                out["chain_device"] = chain
            if prior is not None and store:
                lp = torch.empty(iterations * C, **f64)
                if iterations:
                    kind, q0, q1 = records
                    _lib.check(lib.apgp_prior_lnprior(chain.data_ptr(), iterations * C, D, kind.ctypes.data,
                                                      q0.ctypes.data, q1.ctypes.data, lp.data_ptr(), st),
                               "apgp_prior_lnprior")
                blobs = lp.cpu().numpy().reshape(iterations, C)
                out["blobs"] = np.where(np.isneginf(blobs), np.nan, blobs)
        return out

    @staticmethod
    def _nested_arguments(D, bounds, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0):
        """The checked arguments of :meth:`sample_nested` (host arithmetic only; ``nruns`` may stay None)."""
        nlive, batch = int(nlive), int(batch)
        if not 1 <= batch <= _lib.NESTED_MAX_BATCH:
            raise ValueError("batch must lie between 1 and %d (a wavefront per walker)" % _lib.NESTED_MAX_BATCH)
        if not 4 <= nlive <= _lib.NESTED_MAX_LIVE:
            raise ValueError("nlive must lie between 4 and %d" % _lib.NESTED_MAX_LIVE)
        if nlive < 2 * batch:
            raise ValueError("nlive must be at least 2 * batch")
        nsteps = max(20, 5 * D) if nsteps is None else int(nsteps)
        if nsteps < 1:
            raise ValueError("nsteps must be >= 1")
        if nruns is not None:
            nruns = int(nruns)
            if nruns < 1:
                raise ValueError("nruns must be >= 1")
        dlogz, sigma = float(dlogz), float(sigma)
        if not (np.isfinite(dlogz) and dlogz >= 0.0):
            raise ValueError("dlogz must be finite and >= 0 (0: stop at maxBatches only)")
        if not (np.isfinite(sigma) and sigma >= 0.0):
            raise ValueError("sigma must be finite and >= 0")
        gamma0 = 0.0 if gamma0 is None else float(gamma0)
        if not (np.isfinite(gamma0) and gamma0 > 0.0) and gamma0 != 0.0:
            raise ValueError("gamma0 must be finite and > 0 (None: 2.38 / sqrt(2 D))")
        maxBatches = -(-50 * nlive // batch) if maxBatches is None else int(maxBatches)
        if maxBatches < 1:
            raise ValueError("maxBatches must be >= 1")
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        if len(b) != D:
            raise ValueError("bounds must have one (lo, hi) pair per dimension")
        if not (np.all(np.isfinite(b)) and np.all(b[:, 0] < b[:, 1])):
            raise ValueError("nested sampling needs a finite, non-empty box: its uniform measure is the prior measure")
        return b, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0

    def sample_nested(self, y, bounds, nlive=512, batch=16, nsteps=None, nruns=None, dlogz=0.01, maxBatches=None, seed=0,
                      sigma=1.0e-5, gamma0=None, debug=False, timeDevice=False):
        """Nested sampling over the surrogate, whole runs on the device (``apgp_nested_sample``): the evidence
        ``Z = V int exp(mu) dU`` under the uniform measure on the finite box ``bounds`` (the measure of
        ``evidence(proposal="box")``), its error, the information ``H`` and weighted posterior samples, from ``nruns``
        independent runs merged by :func:`mcmc.nested_weights`.  Nothing is tuned from outside: the runs start from
        the box and compress towards the modes wherever they are.

        A run keeps ``nlive`` live points.  Per batch the ``batch`` lowest die and each is replaced by a walker that
        starts at a random survivor and takes ``nsteps`` (default ``max(20, 5 D)``) constrained differential-evolution
        steps ``q' = q + gamma0 (1 + sigma n)(c_a - c_b)`` in the kernel's scaled coordinates, accepted iff inside the
        box and ``mu(q') >`` the batch's threshold.  A run stops after the first batch for which the live points could
        add less than ``dlogz`` to ``logZ``, or after ``maxBatches`` (default ``50 nlive / batch``; ``dlogz=0``: then
        only).  ``nruns=None`` takes one run per compute unit of the device.  Run r's numbers depend on ``(seed, r)``
        only.  Returns a :class:`mcmc.NestedResult`.  Too few ``nsteps`` bias a step sampler (``nstuck`` and
        ``efficiency`` are the symptoms to watch).  ``debug`` adds ``info["trace"]`` (nruns, maxBatches, batch, nsteps,
        D + 2): every step's proposal, its mean (NaN: outside the box, not evaluated) and 1 / 0 for accepted / not; rows
        of batches that were not run are NaN.  ``timeDevice`` adds ``info["deviceSeconds"]``, the launch between two
        events on its stream (the copies and the host's accounting are not in it)."""
        from .mcmc import NestedResult
        D = self.kernel.ndim
        b, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0 = self._nested_arguments(
            D, bounds, nlive, batch, nsteps, nruns, dlogz, maxBatches, sigma, gamma0)
        lo, hi = _box(b, D, optional=False)
        self.recompute()
        torch, dev, lib = self._rt()
        y = self._check_dimensions(y)
        n = len(self._x)
        ks = self._kernel_struct()
        with self._on(torch, dev):
            st = self._stream(torch)
            self._ensure_xs(y)
            if nruns is None:
                nruns = int(torch.cuda.get_device_properties(dev).multi_processor_count)
            wlen = int(lib.apgp_nested_work_len(D, nlive, nruns))
            if wlen < 0:
                raise ValueError("sample_nested: nlive or nruns beyond the library's limits")
            cap = nlive + batch * maxBatches
            f64 = dict(dtype=torch.float64, device=dev)
            work = torch.empty(wlen, **f64)
            pts = torch.empty((nruns, cap, D), **f64)
            logl, birth = torch.empty((nruns, cap), **f64), torch.empty((nruns, cap), **f64)
            rec = torch.empty((nruns, cap), dtype=torch.int32, device=dev)
            counts = torch.empty((nruns, 4), dtype=torch.int64, device=dev)
            logz = torch.empty((nruns, 2), **f64)
            trace = torch.full((nruns, maxBatches, batch, nsteps, D + 2), float("nan"), **f64) if debug else None
            if timeDevice:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            _lib.check(lib.apgp_nested_sample(self._xs.data_ptr(), n, ctypes.byref(ks), float(self.mean.value), lo, hi, nlive,
                                              batch, nsteps, maxBatches, dlogz, sigma, gamma0, nruns, _seed64(seed),
                                              work.data_ptr(), pts.data_ptr(), logl.data_ptr(), birth.data_ptr(),
                                              rec.data_ptr(), counts.data_ptr(), logz.data_ptr(), _ptr(trace), st),
                       "apgp_nested_sample")
            if timeDevice:
                ev1.record()
            cn = counts.cpu().numpy()
            used = cn[:, 0] * batch + nlive
            top = int(used.max())
            P, Ll, Lb, R = (v[:, :top].cpu().numpy() for v in (pts, logl, birth, rec))
            lz = logz.cpu().numpy()
        keep = np.arange(top)[None, :] < used[:, None]
        if np.any(np.isnan(Ll[keep])):
            raise FloatingPointError("the nested sampler returned NaN log-likelihoods: the GP mean is not finite in the box")
        run = np.broadcast_to(np.arange(nruns)[:, None], keep.shape)
        info = {"record": R[keep], "deviceLogZ": lz[:, 0], "deviceLogX": lz[:, 1], "nsteps": nsteps, "batch": batch,
                "dlogz": dlogz, "maxBatches": maxBatches, "seed": seed}
        if debug:
            info["trace"] = trace.cpu().numpy()
        if timeDevice:
            info["deviceSeconds"] = 1.0e-3 * ev0.elapsed_time(ev1)
        return NestedResult(P[keep], Ll[keep], Lb[keep], run[keep], logVolume=float(np.sum(np.log(b[:, 1] - b[:, 0]))),
                            counts=cn, nlive=nlive, info=info)

    # -- K4: gradient of the log-likelihood ------------------------------------------
    def grad_log_likelihood(self, y, quiet=False):
        """george GP.grad_log_likelihood (gpUtils.py:110): zeros on failure when quiet."""
        try:
            if not self.recompute(quiet=quiet):
                return np.zeros(len(self), dtype=np.float64)
            torch, dev, lib = self._rt()
            y = self._check_dimensions(y)
            n = len(y)
            ks = self._kernel_struct()
            with self._on(torch, dev):
                st = self._stream(torch)
                self._solve(y, need_alpha=True)
                work = torch.empty(lib.apgp_grad_work_len(n), dtype=torch.float64, device=dev)
                out = torch.empty(4 + _lib.MAX_DIM, dtype=torch.float64, device=dev)
                np64 = (n + 63) // 64 * 64
                if self._trust_inverse():
                    # K^-1 = W^T W with the resident dense W = L^-1 (one MFMA-f64 product)
                    self._ensure_linv()
                    winv = self._work.data_ptr()
                else:
                    # above the conditioning gate: K^-1 by two triangular solves against the identity, as george's
                    # cho_solve(L, I) (gpUtils.py:110 -> GP.grad_log_likelihood) -- never a product of inverses
                    xw = torch.empty(int(lib.apgp_kinv_solve_work_len(n)), dtype=torch.float64, device=dev)
                    _lib.check(lib.apgp_kinv_solve(self._L.data_ptr(), n, self._ld, xw.data_ptr(), work.data_ptr(), st),
                               "apgp_kinv_solve")
                    winv = None
                _lib.check(lib.apgp_grad_loglik(self._x_d.data_ptr(), self._alpha.data_ptr(),
                                                winv, np64, n, ctypes.byref(ks),
                                                work.data_ptr(), out.data_ptr(), st),
                           "apgp_grad_loglik")
                o = out.cpu().numpy()
        except (ValueError, LinAlgError):
            if quiet:
                return np.zeros(len(self), dtype=np.float64)
            raise
        return self._assemble_gradient(o, ks.ndim)

    def _assemble_gradient(self, o, ndim):
        """Order device results as george orders its parameter vector."""
        grad = []
        if self.fit_mean:
            grad.append(o[0])
        if self.fit_white_noise:
            # d/d white_noise = 0.5 * exp(wn) * trace(alpha alpha^T - K^-1)  
            grad.append(float(np.exp(self.white_noise.value)) * o[2 + _lib.MAX_DIM])

        o_lin = o[3 + _lib.MAX_DIM]       # 0.5 sum A K_lin

        def walk(k, in_linear_term):
            if isinstance(k, Sum):
                for term in (k.k1, k.k2):
                    walk(term, _flatten_term(term)[2] is not None)
            elif isinstance(k, Product):
                walk(k.k1, in_linear_term); walk(k.k2, in_linear_term)
            elif isinstance(k, ConstantKernel):
                grad.append(o_lin if in_linear_term else o[1])     # d/d log_constant = that term
            elif isinstance(k, LinearKernel):
                grad.append(-o_lin)                                # d/d log_gamma2 = -K_lin
            else:
                grad.extend(o[2:2 + ndim])
        walk(self.kernel, False)
        return np.array(grad, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# quasi-random draws (DESIGN.md "Quasi-random draws")
# ---------------------------------------------------------------------------------------------------------------------
SOBOL_MAX_ROWS = 1 << 30        # the sequence's length: idx_offset + m may not exceed it


def _sobol_draw(torch, dev, lib, stream, m, D, bounds, prior, mixture, seed, replicate, scramble, idx_offset, covScale):
    """Rows of the Sobol sequence through one of the three transforms (exactly one of ``bounds``, ``prior``, ``mixture``
    is given; ``dev`` is current): the device tensor ``T (m, D)``, with ``lnq (m,)`` for a mixture."""
    key = (_seed64(seed), int(replicate), 1 if scramble else 0, int(idx_offset), stream)
    T = torch.empty((m, D), dtype=torch.float64, device=dev)
    if mixture is not None:
        K, Dm, rec = GP._mixture_params(mixture[0], mixture[1], mixture[2], covScale)
        if Dm != D:
            raise ValueError("the mixture must have %d dimensions" % D)
        lnq = torch.empty(m, dtype=torch.float64, device=dev)
        rec = np.ascontiguousarray(rec.ravel())
        if m:
            _lib.check(lib.apgp_sobol_mix_candidates(T.data_ptr(), lnq.data_ptr(), m, D, K, rec.ctypes.data, *key),
                       "apgp_sobol_mix_candidates")
        return T, lnq
    if m == 0:
        return T
    if prior is not None:
        kind, p0, p1 = GP._prior_records(prior, D)
        _lib.check(lib.apgp_sobol_prior_candidates(T.data_ptr(), m, D, kind.ctypes.data, p0.ctypes.data, p1.ctypes.data,
                                                   *key), "apgp_sobol_prior_candidates")
    else:
        lo, hi = _box(bounds, D, optional=False)
        _lib.check(lib.apgp_sobol_box_candidates(T.data_ptr(), m, D, lo, hi, *key), "apgp_sobol_box_candidates")
    return T


def sobolSample(n, bounds=None, prior=None, seed=None):
    """A space-filling initial design: ``n`` rows of one scrambled Sobol replicate in the box ``bounds`` (a (lo, hi) pair
    per dimension) or under ``prior`` (a :class:`~approxposterior_amd.priors.JointPrior`) -- exactly one of the two -- as
    a NumPy array (n, D), from the kernels behind :meth:`GP.sobol_candidates`; no GP is needed.  ``seed=None`` takes one
    integer from NumPy's global stream.  For the best balance take ``n`` a power of two."""
    if (bounds is None) == (prior is None):
        raise ValueError("sobolSample draws from exactly one of bounds and prior")
    n = int(n)
    if not 0 <= n <= SOBOL_MAX_ROWS:
        raise ValueError("sobolSample: 0 <= n <= 2^30 required")
    D = len(np.asarray(bounds, dtype=np.float64).reshape(-1, 2)) if prior is None else len(prior.records()[0])
    if not 1 <= D <= _lib.MAX_DIM:
        raise ValueError("sobolSample: between 1 and %d dimensions" % _lib.MAX_DIM)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    import torch
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.ApgpError("no MI355X visible: approxposterior_amd has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    T = _sobol_draw(torch, dev, lib, GP._stream(torch), n, D, bounds, prior, None, seed, 0, True, 0, 1.0)
    return T.cpu().numpy()
