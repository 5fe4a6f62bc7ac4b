#!/usr/bin/env python
"""Likelihood-gradient fixtures beyond one 64 x 64 tile -> tests/golden/grad_n130_cond1e8.npz, grad_n130_cond1e13.npz.

A seeded synthetic set of N = 130 points in 2-D (three tiles, the last of two rows) under the fitAmp kernel
(amplitude * ExpSquared, white noise e^-30), at two hyper-parameter vectors whose TRUE 2-norm cond(K) is 1e8 and 1e13:
one on either side of GP's conditioning gate (the Cholesky-diagonal estimate it reads is asserted below to fall on
the intended side with a margin).  Each file holds theta, y, the parameter vector p (mean, log_constant, log_M_0_0,
log_M_1_1), white_noise, fit_amp, cond, the gradient of oracle/george_oracle.py (``grad``) and a 60-digit mpmath
gradient (``grad_truth``: a Cholesky factorisation and substitutions written out below, no matrix inverse).
Runs on the CPU in ten seconds; the GPU tests read only the files.

    python tools/make_grad_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import george_oracle as go  # noqa: E402

N, D = 130, 2
WHITE_NOISE = -30.0
LOG_CONSTANT = 0.5
TARGETS = (1e8, 1e13)
GATE = 1e10            # approxposterior_amd.gp.COND_SOLVE


def data():
    rs = np.random.RandomState(130)
    X = rs.uniform(-5.0, 5.0, size=(N, D))
    y = -0.1 * (X[:, 0] ** 2 + 0.5 * X[:, 1] ** 2) + np.sin(X[:, 0]) + 0.3 * np.cos(2.0 * X[:, 1]) + 0.01 * rs.normal(size=N)
    return X, y


def params(t, y):
    return np.array([float(np.median(y)), LOG_CONSTANT, t, t + 0.7])


def gram(X, p):
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 * np.exp(-p[2:])).sum(-1)
    K = D * np.exp(p[1]) * np.exp(-0.5 * d2)
    K[np.diag_indices_from(K)] += np.exp(WHITE_NOISE)
    return K


def oracle_gradient(X, y, p):
    k = go.Product(go.ConstantKernel(p[1], ndim=D), go.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    gp = go.GP(kernel=k, fit_mean=True, mean=float(p[0]), white_noise=WHITE_NOISE, fit_white_noise=False)
    gp.compute(X)
    assert np.allclose(gp.get_parameter_vector(), p)
    return gp.grad_log_likelihood(y)


def mp_gradient(X, y, p, digits=60):
    """g_mean = sum(alpha), g_k = 1/2 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta_k with dK/dlog_constant = K
    (without the white noise) and dK/dlog_M_d = K o (w_d (x_id - x_jd)^2 / 2), w_d = exp(-log_M_d)."""
    import mpmath as mp
    mp.mp.dps = digits
    f = mp.mpf
    n = len(X)
    amp = f(D) * mp.exp(f(float(p[1])))
    w = [mp.exp(-f(float(v))) for v in p[2:]]
    wn = mp.exp(f(WHITE_NOISE))
    Xm = [[f(float(v)) for v in row] for row in X]
    h = [[[w[d] * (Xm[i][d] - Xm[j][d]) ** 2 / 2 for d in range(D)] for j in range(n)] for i in range(n)]
    Kc = [[amp * mp.exp(-sum(h[i][j])) for j in range(n)] for i in range(n)]
    L = [[f(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = Kc[i][j] + (wn if i == j else 0) - mp.fdot(L[i][:j], L[j][:j])
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
    Lt = [[L[k][i] for k in range(n)] for i in range(n)]        # rows of L^T

    def solve(b):
        z = [f(0)] * n
        for i in range(n):
            z[i] = (b[i] - mp.fdot(L[i][:i], z[:i])) / L[i][i]
        x = [f(0)] * n
        for i in range(n - 1, -1, -1):
            x[i] = (z[i] - mp.fdot(Lt[i][i + 1:], x[i + 1:])) / L[i][i]
        return x
    alpha = solve([f(float(v)) - f(float(p[0])) for v in y])
    g = [sum(alpha)] + [f(0)] * (1 + D)
    for j in range(n):
        col = solve([f(1) if i == j else f(0) for i in range(n)])       # column j of K^-1
        for i in range(n):
            a = (alpha[i] * alpha[j] - col[i]) * Kc[i][j]
            g[1] += a
            for d in range(D):
                g[2 + d] += a * h[i][j][d]
    return np.array([float(g[0])] + [float(v / 2) for v in g[1:]])


def main():
    from scipy.optimize import brentq
    X, y = data()
    golden = os.path.join(ROOT, "tests", "golden")
    for target in TARGETS:
        t = brentq(lambda v: np.log10(np.linalg.cond(gram(X, params(v, y)))) - np.log10(target), -3.0, 2.0, xtol=1e-10)
        p = params(t, y)
        K = gram(X, p)
        cond = float(np.linalg.cond(K))
        dg = np.diag(np.linalg.cholesky(K))
        est = float((dg.max() / dg.min()) ** 2)
        # the gate reads the estimate: well clear of it on the intended side
        assert est < GATE / 10.0 if target < 1e10 else est > 2.0 * GATE, (target, est)
        grad = oracle_gradient(X, y, p)
        truth = mp_gradient(X, y, p)
        name = "grad_n130_cond1e%d" % int(round(np.log10(target)))
        np.savez_compressed(os.path.join(golden, name + ".npz"), theta=X, y=y, p=p, white_noise=np.array(WHITE_NOISE),
                            fit_amp=np.array(1), cond=np.array(cond), cond_estimate=np.array(est), grad=grad,
                            grad_truth=truth)
        print("%s: log_M %.6f, cond %.3e, estimate %.3e, truth %s, oracle error %s" % (name, t, cond, est, truth,
                                                                                   np.abs(grad - truth)), flush=True)


if __name__ == "__main__":
    main()
