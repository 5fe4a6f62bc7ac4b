"""Candidates drawn from a JointPrior on the device (GP.prior_candidates) against the host draw the sweep otherwise starts
from (JointPrior.sample, i.e. scipy's per-factor rvs, plus the H2D copy of the matrix): 1e6 x 8 with four Uniform and four
Gaussian factors, the median of --reps runs each, plus one blob pass (apgp_prior_lnprior) over the same matrix.  Prints
one JSON line.

    python tools/prior_timing.py [--reps 5] [--out profiles/prior_timing.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=10 ** 6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prior_timing needs the GPU")
    from approxposterior_amd import _lib, gp as agp, priors
    D, m = 8, args.m
    J = priors.JointPrior([priors.UniformPrior(-5.0 + d, 5.0 + d) if d % 2 == 0 else priors.GaussianPrior(0.1 * d, 1.0 + d)
                           for d in range(D)])
    rs = np.random.RandomState(0)
    g = agp.GP(kernel=agp.ExpSquaredKernel(np.ones(D), ndim=D), fit_mean=True, mean=0.0, white_noise=-8.0,
               fit_white_noise=False)
    g.compute(rs.uniform(-1, 1, size=(64, D)))
    lib = _lib.load()
    dev = torch.device("cuda:0")

    def timed(fn):
        runs = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        return float(np.median(runs))

    g.prior_candidates(1024, J, 1)                                        # load the code objects
    t_dev = timed(lambda: g.prior_candidates(m, J, 12345))
    np.random.seed(0)
    t_host = timed(lambda: torch.from_numpy(np.ascontiguousarray(J.sample(m))).to(dev))
    T = g.prior_candidates(m, J, 12345)
    out = torch.empty(m, dtype=torch.float64, device=dev)
    kind, p0, p1 = J.records()

    def blob():
        _lib.check(lib.apgp_prior_lnprior(T.data_ptr(), m, D, kind.ctypes.data, p0.ctypes.data, p1.ctypes.data,
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream), "apgp_prior_lnprior")
    blob()
    t_blob = timed(blob)
    res = {"what": "JointPrior candidates, %d x %d (4 Uniform + 4 Gaussian factors)" % (m, D),
           "device_prior_candidates_ms": round(1e3 * t_dev, 3),
           "host_sample_plus_h2d_ms": round(1e3 * t_host, 3),
           "speedup": round(t_host / t_dev, 1),
           "device_lnprior_pass_ms": round(1e3 * t_blob, 3),
           "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
