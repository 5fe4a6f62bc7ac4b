"""What the predictive gradients (GP.predict_grad, apgp_predict_grad) cost, on one MI355X at N = 512, 1152, 4096 and
D = 8, through the dense inverse and through the factor (``variance_mode`` forced), medians after a warm-up:

 (a) per evaluation: one ``predict_grad`` at one host point (utility and gradient) against the D + 1 single-point
     ``predict(return_var=True)`` calls SciPy's finite differences make for the same gradient; host clock, both
     return host arrays (they end in a synchronisation);
 (b) per search: ``minimizeObjective(method="l-bfgs-b", nRestarts=5)`` with ``jac=True`` against ``jac=False``, and
     against the default Nelder-Mead search on the host and on the device (``onDevice=True``); AGP, starts drawn from
     the inner half of the box (an L-BFGS-B run that steps into the prior's +inf wall ends where it stands, with either
     gradient); evaluations (device calls), wall time, utility reached;
 (c) batched: m = 256 and 4096 points resident on the device, HIP events; with the fraction of the HBM rate a single
     point reaches (two passes over the lower triangle of W, against the 8 TB/s of the data sheet) and of the FP64
     vector peak (78.6 TFLOP/s) the batches reach (4 m N^2 / 2 flops: two triangular passes, an FMA per element and
     point).
Usage: python tools/predict_grad_timing.py [--reps R] [--sizes 512,1152,4096] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
FP64_VECTOR_FLOPS = 78.6e12


def problem(N, D):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(N + 7 * D)
    X = rs.uniform(-5, 5, size=(N, D))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
    y = y - np.median(y)
    kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
    gp = agp.GP(kernel=kern, fit_mean=True, mean=0.0, white_noise=np.log(1e-6 * np.var(y)), fit_white_noise=False)
    gp.compute(X)
    return y, gp


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def events(torch, fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)) * 1e-3


class Counted(object):
    """Counts the calls of ``gp.predict`` / ``gp.predict_grad`` while it is installed."""

    def __init__(self, gp):
        self.gp, self.n = gp, 0

    def __enter__(self):
        for name in ("predict", "predict_grad"):
            real = getattr(self.gp, name)

            def counted(*a, _real=real, **k):
                self.n += 1
                return _real(*a, **k)
            setattr(self.gp, name, counted)
        return self

    def __exit__(self, *exc):
        for name in ("predict", "predict_grad"):
            delattr(self.gp, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="512,1152,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_grad_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("predict_grad_timing needs an MI355X")
    from approxposterior_amd import utility as ut
    D = 8
    lo, hi = -5.0 * np.ones(D), 5.0 * np.ones(D)

    def prior(x):
        x = np.ravel(x)
        return 0.0 if np.all((x >= lo) & (x <= hi)) else -np.inf

    def sample(m):
        return np.random.uniform(0.5 * lo, 0.5 * hi, size=(m, D))

    rows = []
    for N in [int(v) for v in a.sizes.split(",")]:
        y, gp = problem(N, D)
        rs = np.random.RandomState(3)
        for mode in ("inverse", "solve"):
            gp.variance_mode = mode
            row = dict(N=N, D=D, route=mode)
            # (a)
            x = rs.uniform(-2, 2, size=D)
            pts = [np.ascontiguousarray(x.reshape(1, D) + 1e-6 * np.eye(D + 1, D)[i]) for i in range(D + 1)]
            row["eval_grad_us"] = 1e6 * wall(lambda: gp.predict_grad(y, x, kind="agp"), 10 * a.reps)
            row["eval_fd_us"] = 1e6 * wall(lambda: [gp.predict(y, p, return_var=True) for p in pts], 10 * a.reps)
            row["eval_speedup"] = row["eval_fd_us"] / row["eval_grad_us"]
            # (b)
            searches = {"lbfgsb_jac": dict(method="l-bfgs-b", jac=True), "lbfgsb_fd": dict(method="l-bfgs-b"),
                        "nm_host": {}, "nm_device": dict(onDevice=True, bounds=list(zip(lo, hi)))}
            for key, kw in searches.items():
                def run():
                    np.random.seed(1)
                    with np.errstate(all="ignore"):
                        return ut.minimizeObjective(ut.AGPUtility, y, gp, sample, prior, nRestarts=5,
                                                    args=(y, gp, prior), **kw)
                sec = wall(run, max(1, a.reps // 2))
                with Counted(gp) as c:
                    res = run()
                row[key] = dict(ms=1e3 * sec, device_calls=c.n, u=float(np.ravel(res[1])[0]))
            # (c)
            for m in (1, 256, 4096):
                T = torch.from_numpy(rs.uniform(-5, 5, size=(m, D))).to("cuda")
                sec = events(torch, lambda: gp.predict_grad(y, T, kind="agp", return_device=True), a.reps)
                tri = N * (N + 1) / 2
                row["batch_m%d" % m] = dict(ms=1e3 * sec, us_per_point=1e6 * sec / m,
                                            hbm_fraction=2 * tri * 8 / sec / HBM_BYTES_PER_S if m == 1 else None,
                                            fp64_fraction=4 * m * tri / sec / FP64_VECTOR_FLOPS)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(what="GP.predict_grad on one MI355X, D = 8: (a) one exact utility gradient against the D + 1 predict calls "
                    "of a finite difference, host clock; (b) 5-restart AGP point search, l-bfgs-b with exact and with "
                    "differenced gradients, Nelder-Mead on host and device; (c) batched calls on resident points, HIP "
                    "events.  Medians after a warm-up (%d runs; (a) %d; (b) %d)" % (a.reps, 10 * a.reps, max(1, a.reps // 2)),
               hbm_bytes_per_s=HBM_BYTES_PER_S, fp64_vector_flops=FP64_VECTOR_FLOPS, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
