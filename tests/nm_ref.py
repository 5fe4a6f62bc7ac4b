# -*- coding: utf-8 -*-
"""NumPy restatement of SciPy 1.15's ``_minimize_neldermead`` (``bounds=None``) as ``apgp_nm_search`` runs it: the same
simplex arithmetic, comparisons and ``maxfev`` accounting, the vertices re-sorted after every iteration by a STABLE sort on
the previous position (NaN last) -- the device's documented tie rule -- and a record of every evaluated point and of the
step each iteration took (``approxposterior_amd._lib.NM_STEPS`` codes).

On objectives without ties it gives SciPy's ``x``, ``fun``, ``nfev`` and ``nit`` bit for bit (tests/test_nm_ref.py).
A teacher-forced replay passes an objective that hands back the device's own values in evaluation order and checks
that every point asked for is the device's next point (tests/test_gpu_nm_search.py)."""
import numpy as np

REFLECT, EXPAND, REFLECT_EXP, CONTRACT_OUT, CONTRACT_IN, SHRINK_OUT, SHRINK_IN, MAXFEV = range(1, 9)


class _MaxFev(Exception):
    pass


def coefficients(ndim, adaptive=True):
    """(rho, chi, psi, sigma) exactly as SciPy computes them."""
    if adaptive:
        dim = float(ndim)
        return 1, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1, 2, 0.5, 0.5


def limits(ndim, maxiter=None, maxfev=None):
    """SciPy's (maxiter, maxfev) defaults; an unbounded maxfev becomes the most evaluations maxiter allows."""
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


def _sort(sim, fsim):
    ind = np.argsort(fsim, kind="stable")
    return np.take(sim, ind, 0), np.take(fsim, ind, 0)


def neldermead(fun, x0, maxiter=None, maxfev=None, xatol=1e-4, fatol=1e-4, adaptive=True):
    """Minimise ``fun`` from ``x0``; returns a dict with x, fun, nfev, nit, status, points (evaluated, in order),
    values and steps (one code per loop body)."""
    x0 = np.atleast_1d(np.asarray(x0, dtype=np.float64)).flatten()
    N = len(x0)
    rho, chi, psi, sigma = coefficients(N, adaptive)
    maxiter, maxfun = limits(N, maxiter, maxfev)
    nonzdelt, zdelt = 0.05, 0.00025
    sim = np.empty((N + 1, N), dtype=x0.dtype)
    sim[0] = x0
    for k in range(N):
        y = np.array(x0, copy=True)
        if y[k] != 0:
            y[k] = (1 + nonzdelt) * y[k]
        else:
            y[k] = zdelt
        sim[k + 1] = y
    points, values, steps = [], [], []
    ncalls = [0]

    def func(x):
        if ncalls[0] >= maxfun:
            raise _MaxFev()
        ncalls[0] += 1
        points.append(np.array(x, copy=True))
        fx = float(fun(np.copy(x)))
        values.append(fx)
        return fx

    fsim = np.full((N + 1,), np.inf, dtype=float)
    try:
        for k in range(N + 1):
            fsim[k] = func(sim[k])
    except _MaxFev:
        pass
    sim, fsim = _sort(sim, fsim)
    iterations = 1
    while ncalls[0] < maxfun and iterations < maxiter:
        if (np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= xatol and
                np.max(np.abs(fsim[0] - fsim[1:])) <= fatol):
            break
        step = MAXFEV
        try:
            xbar = np.add.reduce(sim[:-1], 0) / N
            xr = (1 + rho) * xbar - rho * sim[-1]
            fxr = func(xr)
            doshrink = 0
            if fxr < fsim[0]:
                xe = (1 + rho * chi) * xbar - rho * chi * sim[-1]
                fxe = func(xe)
                if fxe < fxr:
                    sim[-1], fsim[-1], step = xe, fxe, EXPAND
                else:
                    sim[-1], fsim[-1], step = xr, fxr, REFLECT_EXP
            else:
                if fxr < fsim[-2]:
                    sim[-1], fsim[-1], step = xr, fxr, REFLECT
                else:
                    if fxr < fsim[-1]:
                        xc = (1 + psi * rho) * xbar - psi * rho * sim[-1]
                        fxc = func(xc)
                        if fxc <= fxr:
                            sim[-1], fsim[-1], step = xc, fxc, CONTRACT_OUT
                        else:
                            doshrink, step = 1, SHRINK_OUT
                    else:
                        xcc = (1 - psi) * xbar + psi * sim[-1]
                        fxcc = func(xcc)
                        if fxcc < fsim[-1]:
                            sim[-1], fsim[-1], step = xcc, fxcc, CONTRACT_IN
                        else:
                            doshrink, step = 1, SHRINK_IN
                    if doshrink:
                        for j in range(1, N + 1):
                            sim[j] = sim[0] + sigma * (sim[j] - sim[0])
                            fsim[j] = func(sim[j])
            iterations += 1
        except _MaxFev:
            step = MAXFEV
        finally:
            steps.append(step)
            sim, fsim = _sort(sim, fsim)
    if ncalls[0] >= maxfun:
        status = 1
    elif iterations >= maxiter:
        status = 2
    else:
        status = 0
    return dict(x=sim[0].copy(), fun=np.min(fsim), nfev=ncalls[0], nit=iterations, status=status,
                points=points, values=values, steps=steps)


def replay(trace_x, trace_u, x0, **options):
    """Teacher-forced replay of one device restart: ``trace_x`` (nfev, D) / ``trace_u`` (nfev,) are the points the
    device evaluated and the values it got.  Each point the restatement asks for must equal the device's next point bit
    for bit (AssertionError otherwise); it is then handed the device's value.  Returns :func:`neldermead`'s record."""
    trace_x = np.asarray(trace_x, dtype=np.float64)
    trace_u = np.asarray(trace_u, dtype=np.float64)
    k = [0]

    def fun(x):
        i = k[0]
        assert i < len(trace_x), "the replay asks for evaluation %d, the device made %d" % (i + 1, len(trace_x))
        assert np.array_equal(x.view(np.uint64), trace_x[i].view(np.uint64)), \
            "evaluation %d: replay %r, device %r" % (i, x.tolist(), trace_x[i].tolist())
        k[0] += 1
        return trace_u[i]

    return neldermead(fun, x0, **options)
