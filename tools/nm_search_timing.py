"""The restarted Nelder-Mead point search of findNextPoint (5 restarts, AGP, adaptive) on the host path
(utility.minimizeObjective: SciPy over one apgp_predict1_host per evaluation) against the device search
(minimizeObjective(onDevice=True): apgp_nm_search, every restart in one launch), at N = 50, 90, 256, 512, 1152, 4096
and D = 2, 8; HIP events around each call, median of --reps runs after one warm-up.  Then the README configuration
(C1: Rosenbrock, m0 = 50, m = 20, nmax = 2, BAPE, 20 walkers x 2e4 iterations) end to end, default against
deviceSearch=True, one run each.  DESIGN.md "Device point search" quotes the result.
Usage: python tools/nm_search_timing.py [--reps R] [--no-c1] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(N, D):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(N + 7 * D)
    X = rs.uniform(-5, 5, size=(N, D))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0 if D > 1 else \
        -np.sum(X ** 2, axis=1)
    y = y - np.median(y)
    kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
    gp = agp.GP(kernel=kern, fit_mean=True, mean=0.0, white_noise=np.log(1e-6 * np.var(y)), fit_white_noise=False)
    gp.compute(X)
    return y, gp


def timed(torch, fn, reps):
    fn()                                           # warm-up: resident inverse / factor, compiled code objects
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [float(m) for m in ms]


def c1(deviceSearch):
    from approxposterior_amd import approx, gpUtils, likelihood as lh
    np.random.seed(57)
    theta = lh.rosenbrockSample(50)
    y = np.array([lh.rosenbrockLnlike(t) + lh.rosenbrockLnprior(t) for t in theta])
    gp = gpUtils.defaultGP(theta, y, white_noise=-12)
    ap = approx.ApproxPosterior(theta=theta, y=y, gp=gp, lnprior=lh.rosenbrockLnprior, lnlike=lh.rosenbrockLnlike,
                                priorSample=lh.rosenbrockSample, bounds=[(-5, 5), (-5, 5)], algorithm="bape")
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        ap.run(m=20, nmax=2, estBurnin=True, nGPRestarts=3, mcmcKwargs={"iterations": int(2.0e4)}, cache=False,
               samplerKwargs={"nwalkers": 20}, verbose=False, thinChains=False, onlyLastMCMC=True,
               deviceSearch=deviceSearch)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="50,90,256,512,1152,4096")
    ap.add_argument("--dims", default="2,8")
    ap.add_argument("--no-c1", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nm_search_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nm_search_timing needs an MI355X")
    from approxposterior_amd import utility as ut
    rows = []
    for D in [int(v) for v in a.dims.split(",")]:
        for N in [int(v) for v in a.sizes.split(",")]:
            y, gp = problem(N, D)
            lo, hi = -5.0 * np.ones(D), 5.0 * np.ones(D)

            def prior(x):
                x = np.ravel(x)
                return 0.0 if np.all((x >= lo) & (x <= hi)) else -np.inf

            def sample(m):
                return np.random.uniform(lo, hi, size=(m, D))

            def run(on):
                np.random.seed(1)
                with np.errstate(all="ignore"):
                    ut.minimizeObjective(ut.AGPUtility, y, gp, sample, prior, nRestarts=5, args=(y, gp, prior),
                                         onDevice=on, bounds=list(zip(lo, hi)))
            host, host_all = timed(torch, lambda: run(False), a.reps)
            dev, dev_all = timed(torch, lambda: run(True), a.reps)
            np.random.seed(1)
            starts = sample(5)
            res = gp.nelder_mead_search(y, starts, "agp", bounds=list(zip(lo, hi)), options={"adaptive": True})
            row = dict(N=N, D=D, form="inverse" if gp._trust_inverse() else "solve",
                       host_ms=host, device_ms=dev, speedup=host / dev, host_runs_ms=host_all, device_runs_ms=dev_all,
                       nfev_per_restart=[int(v) for v in res[2]],
                       device_us_per_evaluation=1e3 * dev / max(1, int(np.max(res[2]))))
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(what="findNextPoint point search, 5 restarts, AGP, adaptive Nelder-Mead: host path vs device search "
                    "(HIP events, median of %d runs after a warm-up)" % a.reps, rows=rows)
    if not a.no_c1:
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                c1(False)                          # warm-up (code objects, allocator)
                out["c1_default_s"] = c1(False)
                out["c1_device_search_s"] = c1(True)
            finally:
                os.chdir(cwd)
        print("C1 end to end: default %.3f s, deviceSearch %.3f s" % (out["c1_default_s"], out["c1_device_search_s"]),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
