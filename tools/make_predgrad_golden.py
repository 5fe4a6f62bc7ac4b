#!/usr/bin/env python
"""Extended-precision truth of the predictive gradients on the committed fixtures -> tests/golden/predgrad_truth.npz.

For each fixture: 8 seeded query points inside the box of the training set and, at each, mu, var, dmu, dvar of
include/apgp.h's ``apgp_predict_grad`` formulas evaluated with mpmath at 60 digits (a Cholesky factorisation and the
two substitutions written out below), from the float64 hyper-parameters exactly as ``GP._kernel_struct`` hands them
to the library; plus the scale vectors of the error bound,
    S_mu[d]  = sum_n |alpha_n J_nd|          S_var[d] = |d k(t,t)/d t_d| + 2 sum_n |w_n J_nd|.
Runs on the CPU (a few minutes: the N = 300 factorisation dominates); the GPU tests read only the file.

    python tools/make_predgrad_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predgrad_ref as ref  # noqa: E402

FIXTURES = ["rosen2d_n50_noamp", "rosen2d_n50_amp", "c2small_d2_n200", "c3small_d8_n300", "d5_n130_amp",
            "rosen2d_n50_amp_cond1e8", "rosen2d_n50_amp_cond1e11", "rosen2d_n50_amp_cond1e13"]
NPOINTS = 8
SEED = 20240611


def query_points(X, index):
    """NPOINTS seeded points inside the box of the training set (the middle 90 % of each side)."""
    rs = np.random.RandomState(SEED + index)
    lo, hi = X.min(axis=0), X.max(axis=0)
    return lo + (hi - lo) * rs.uniform(0.05, 0.95, size=(NPOINTS, X.shape[1]))


def truth(X, y, prm, T, digits=60):
    import mpmath as mp
    mp.mp.dps = digits
    n, D = X.shape
    f = mp.mpf
    Xm = [[f(float(v)) for v in row] for row in X]
    im = [f(float(v)) for v in prm["inv_metric"]]
    amp, c, P = f(prm["amp"]), f(prm["lin_coef"]), prm["lin_order"]
    half = f(1) / 2

    def kfun(a, b):
        s = sum((a[d] - b[d]) ** 2 * im[d] for d in range(D))
        k = amp * mp.exp(-half * s)
        if c != 0:
            k += c * (D if P == 0 else sum((a[d] * b[d]) ** P for d in range(D)))
        return k

    def jfun(a, b, d):
        s = sum((a[e] - b[e]) ** 2 * im[e] for e in range(D))
        j = -amp * mp.exp(-half * s) * (a[d] - b[d]) * im[d]
        if c != 0 and P > 0:
            j += c * P * (a[d] * b[d]) ** (P - 1) * b[d]
        return j

    # Cholesky K = L L^T, row by row
    L = [[f(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = kfun(Xm[i], Xm[j]) + (f(prm["diag_add"]) if i == j else 0)
            s -= mp.fdot(L[i][:j], L[j][:j])
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]

    def fwd(b):
        z = [f(0)] * n
        for i in range(n):
            z[i] = (b[i] - mp.fdot(L[i][:i], z[:i])) / L[i][i]
        return z

    def bwd(b):
        x = [f(0)] * n
        for i in range(n - 1, -1, -1):
            x[i] = (b[i] - sum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
        return x

    alpha = bwd(fwd([f(float(v)) - f(prm["mean"]) for v in y]))
    out = {k: np.zeros((len(T),) + ((D,) if k not in ("mu", "var") else ())) for k in
           ("mu", "var", "dmu", "dvar", "S_mu", "S_var")}
    for m, t in enumerate(T):
        tm = [f(float(v)) for v in t]
        k = [kfun(tm, Xm[i]) for i in range(n)]
        v = fwd(k)
        w = bwd(v)
        ktt = amp + (c * (D if P == 0 else sum((tm[d] * tm[d]) ** P for d in range(D))) if c != 0 else 0)
        out["mu"][m] = float(mp.fdot(k, alpha) + f(prm["mean"]))
        out["var"][m] = float(ktt - mp.fdot(v, v))
        for d in range(D):
            J = [jfun(tm, Xm[i], d) for i in range(n)]
            dktt = c * 2 * P * tm[d] ** (2 * P - 1) if (c != 0 and P > 0) else f(0)
            out["dmu"][m, d] = float(mp.fdot(alpha, J))
            out["dvar"][m, d] = float(dktt - 2 * mp.fdot(w, J))
            out["S_mu"][m, d] = float(sum(abs(a * j) for a, j in zip(alpha, J)))
            out["S_var"][m, d] = float(abs(dktt) + 2 * sum(abs(a * j) for a, j in zip(w, J)))
    return out


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    store = {}
    for index, name in enumerate(FIXTURES):
        g = np.load(os.path.join(golden, name + ".npz"))
        prm = ref.fixture_params(g)
        T = query_points(g["theta"], index)
        res = truth(g["theta"], g["y"], prm, T)
        store[name + "/T"] = T
        for key, val in res.items():
            store[name + "/" + key] = val
        print(name, "done: max |dmu| %.3g, max |dvar| %.3g" % (np.abs(res["dmu"]).max(), np.abs(res["dvar"]).max()),
              flush=True)
    np.savez(os.path.join(golden, "predgrad_truth.npz"), **store)


if __name__ == "__main__":
    main()
