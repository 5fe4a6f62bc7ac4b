"""Posterior function draws (DESIGN.md "Posterior function draws") at N = 4096, D = 8, M = 1e6 and N = 1152, D = 8,
M = 1e5, for R in {1024, 2048, 4096} features and S in {1, 8, 16, 32} draws, timed with HIP events in one process after
a warm-up, median of --reps:
  setup      GP.sample_paths: the host draws, g_s(X) by the kernel, 2 S triangular solves (or products with L^-1)
  pass       one apgp_path_draws launch over all candidates plus its arg-min (PathDraws.argmax): the library's choice
             of contraction, then the vector and the matrix-core contraction forced (apgp_path_draws_mode)
  thompson   GP.thompson_batch(q = 8) end to end (R = 2048)
against, in the same process: the full sweep (GP.acquire), GP.acquire_batch(q = 8) and one apgp_acquire_fantasy pass.
Usage: python tools/path_draws_timing.py [--reps R] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x8x1000000,1152x8x100000")
    ap.add_argument("--features", default="1024,2048,4096")
    ap.add_argument("--draws", default="1,8,16,32")
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("path_draws_timing needs an MI355X")
    from approxposterior_amd import gp as agp, _lib
    lib = _lib.load()
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def median(fn, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        return float(np.median([timed(fn)[0] for _ in range(a.reps)]))

    res = {"reps": a.reps, "q": a.q, "shapes": []}
    for shape in a.shapes.split(","):
        N, D, M = (int(v) for v in shape.split("x"))
        rs = np.random.RandomState(0)
        np.random.seed(0)
        X = rs.uniform(-5, 5, size=(N, D))
        y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
        kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
        gp = agp.GP(kernel=kern, fit_mean=True, mean=float(np.mean(y)), white_noise=np.log(1e-6 * np.var(y)))
        gp.compute(X)
        Td = torch.from_numpy(rs.uniform(-5.2, 5.2, size=(M, D))).cuda()
        r = {"N": N, "D": D, "M": M, "cond_estimate": gp.cond_estimate, "trust_inverse": bool(gp._trust_inverse())}
        # yardsticks: the full sweep, the kriging-believer batch, one fantasy pass inside it
        r["sweep_ms"] = median(lambda: gp.acquire(y, Td, "bape"))
        marks, real = [], lib.apgp_acquire_fantasy

        def fantasy(*args):
            s0, s1 = ev(), ev()
            s0.record()
            rc = real(*args)
            s1.record()
            marks.append((s0, s1))
            return rc
        lib.apgp_acquire_fantasy = fantasy
        try:
            r["acquire_batch_ms"] = median(lambda: gp.acquire_batch(y, Td, "bape", a.q))
        finally:
            lib.apgp_acquire_fantasy = real
        r["fantasy_pass_ms"] = float(np.median([s0.elapsed_time(s1) for s0, s1 in marks[a.q - 1:]]))
        print(json.dumps(r), flush=True)
        r["draws"] = []
        for R in (int(v) for v in a.features.split(",")):
            for S in (int(v) for v in a.draws.split(",")):
                setup = median(lambda: gp.sample_paths(y, S, R))
                paths = gp.sample_paths(y, S, R)
                passed = median(lambda: paths.argmax(Td))
                forms = {}
                for name, mode in (("vector", 1), ("matrix", 2)):      # the contraction forced onto one unit
                    was = lib.apgp_path_draws_mode(mode)
                    try:
                        forms[name] = median(lambda: paths.argmax(Td))
                    finally:
                        lib.apgp_path_draws_mode(was)
                c = {"R": R, "S": S, "setup_ms": setup, "pass_ms": passed, "pass_vector_ms": forms["vector"],
                     "pass_matrix_ms": forms["matrix"],
                     "values_per_s": M * (N + R) / (1e-3 * passed),
                     "pass_over_fantasy": passed / r["fantasy_pass_ms"], "pass_over_sweep": passed / r["sweep_ms"],
                     "pass_over_acquire_batch": passed / r["acquire_batch_ms"]}
                r["draws"].append(c)
                print(json.dumps(c), flush=True)
        th = median(lambda: gp.thompson_batch(y, Td, a.q, nFeatures=2048))
        r["thompson_batch_ms"] = th
        r["thompson_over_acquire_batch"] = th / r["acquire_batch_ms"]
        r["thompson_over_sweep"] = th / r["sweep_ms"]
        print(json.dumps({k: v for k, v in r.items() if k != "draws"}), flush=True)
        res["shapes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
