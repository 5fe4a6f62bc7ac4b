"""Batch design points at C3 (N = 4096, D = 8, M = 1e6, BAPE, q = 8), in both variance forms, timed with HIP events in
one process (DESIGN.md "Batch design points"):
  sweep   the first full sweep (apgp_acquire / apgp_acquire_solve)
  step    one fantasy step: record read, mu(x_j), cross row, two triangular solves, the fantasy pass
  pass    the fantasy pass alone (apgp_acquire_fantasy + its arg-min)
  slow    one step of the slow path: absorb the fantasy row (compute(previous=)), repack, full sweep
  total   GP.acquire_batch(q = 8) end to end, against q slow steps
Usage: python tools/batch_acquire_timing.py [--reps R] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("batch_acquire_timing needs an MI355X")
    import ctypes
    from approxposterior_amd import gp as agp, _lib
    rs = np.random.RandomState(0)
    N, D, M, q = a.n, a.d, a.m, a.q
    X = rs.uniform(-5, 5, size=(N, D))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
    kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
    gp = agp.GP(kernel=kern, fit_mean=True, mean=float(np.mean(y)), white_noise=np.log(1e-6 * np.var(y)))
    gp.compute(X)
    Td = torch.from_numpy(rs.uniform(-5.2, 5.2, size=(M, D))).cuda()
    lib = _lib.load()
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    res = {"N": N, "D": D, "M": M, "q": q, "kind": "bape", "cond_estimate": gp.cond_estimate, "forms": {}}
    for mode in ("inverse", "solve"):
        gp.variance_mode = mode
        gp.acquire_batch(y, Td, "bape", 2)                  # warm-up: factor images, alpha, stream, code objects
        torch.cuda.synchronize()
        r = {"sweep_ms": [], "total_ms": [], "pass_ms": [], "step_ms": [], "slow_step_ms": []}
        for _ in range(a.reps):
            e0, e1 = ev(), ev()
            e0.record()
            gp.acquire(y, Td, "bape")
            e1.record()
            torch.cuda.synchronize()
            r["sweep_ms"].append(e0.elapsed_time(e1))
            # end to end, and the fantasy passes inside it (events around each library call of the pass)
            marks = []
            real = lib.apgp_acquire_fantasy

            def timed(*args):
                s0, s1 = ev(), ev()
                s0.record()
                rc = real(*args)
                s1.record()
                marks.append((s0, s1))
                return rc
            lib.apgp_acquire_fantasy = timed
            t0 = time.perf_counter()
            e0.record()
            idx, ub = gp.acquire_batch(y, Td, "bape", q)
            e1.record()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            lib.apgp_acquire_fantasy = real
            r["total_ms"].append(e0.elapsed_time(e1))
            r["pass_ms"].extend(s0.elapsed_time(s1) for s0, s1 in marks)
            r.setdefault("total_wall_ms", []).append(1e3 * wall)
            r["step_ms"].append((e0.elapsed_time(e1) - r["sweep_ms"][-1]) / (q - 1))
        # the slow path, one step: absorb the fantasy row, repack, full sweep
        Th = Td.cpu().numpy()
        b0 = int(idx[0])
        mu0 = float(gp.predict(y, Th[b0:b0 + 1], return_cov=False)[0])
        for _ in range(a.reps):
            g = agp.GP(kernel=gp.kernel, fit_mean=True, mean=gp.mean, white_noise=gp.white_noise)
            g.set_parameter_vector(gp.get_parameter_vector())
            g.variance_mode = mode
            torch.cuda.synchronize()
            e0.record()
            g.compute(np.vstack([X, Th[b0:b0 + 1]]), previous=gp)
            g.acquire(np.append(y, mu0), Td, "bape")
            e1.record()
            torch.cuda.synchronize()
            r["slow_step_ms"].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in r.items()}
        med["step_over_sweep"] = med["step_ms"] / med["sweep_ms"]
        med["batch_over_sweep"] = med["total_ms"] / med["sweep_ms"]
        med["slow_batch_over_sweep"] = (med["sweep_ms"] + (q - 1) * med["slow_step_ms"]) / med["sweep_ms"]
        med["picks"] = [int(i) for i in idx]
        res["forms"][mode] = med
        print(mode, json.dumps(med), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
