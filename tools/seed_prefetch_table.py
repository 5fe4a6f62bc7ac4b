#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""The pruned arg-min's time by prefetch distance of the parked seed launch (apgp_set_seed_prefetch),
in ONE process: per size and forced part size (``GP.seed_parts``; -1: the library's rule) the distances 0 (the launch as it
was), 1, 2, 3, 4 and 6 in turn, round after round, each call timed by the HIP events GP._sweep records around the library
call.  Everything but the seed launches is the same work at every distance, so the differences are the seed launches'.
The winner must have the same bits at every setting -- the tool stops if it has not.

    python tools/seed_prefetch_table.py [--rounds 7] [--out profiles/r31_seed_prefetch_table.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTANCES = (0, 1, 2, 3, 4, 6)
PARTS = (-1, 4, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from approxposterior_amd import gp as agp
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = {"tool": "tools/seed_prefetch_table.py", "rounds": args.rounds, "sweep_source_sha": bench.sweep_source_hash(),
           "unit": "ms per pruned call, median [min, max]", "sizes": {}}
    for n in (4096, 2048, 1152):
        d, m = 8, 1000000
        X, y = bench.synthetic_c3(n, d)
        g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y), white_noise=-12,
                   fit_white_noise=False, device=dev)
        g.compute(X)
        T = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, d))).to(dev)
        box = [(-5.0, 5.0)] * d
        g.sweep_prune = 1
        want = None
        rows = {}
        for parts in PARTS:
            g.seed_parts = parts
            t = {v: [] for v in DISTANCES}
            for rnd in range(args.rounds + 1):          # (round 0: warm-up)
                for v in DISTANCES:
                    g.seed_prefetch = v
                    g.kernel_events = ev = []
                    r = g.acquire(y, T, "agp", bounds=box)
                    torch.cuda.synchronize()
                    got = (int(r[0]), int(np.float64(r[1]).view(np.uint64)))
                    if want is None:
                        want = got
                    if got != want:
                        raise SystemExit("seed_prefetch_table: winner %r != %r at n=%d parts=%d distance=%d" % (got, want, n, parts, v))
                    if rnd > 0:
                        t[v].append(ev[0][0].elapsed_time(ev[0][1]))
            rows[str(parts)] = {str(v): [float(np.median(t[v])), float(min(t[v])), float(max(t[v]))] for v in DISTANCES}
            print(n, parts, json.dumps(rows[str(parts)]), flush=True)
        g.kernel_events = None
        out["sizes"][str(n)] = {"candidates": m, "ndim": d, "best": [want[0], float(np.uint64(want[1]).view(np.float64))], "parts": rows}
        del g
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
