#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""A/B of the pruned arg-min against the full sweep (apgp_set_sweep_prune), in ONE process:
per shape a warm-up, then alternating pairs switch off / switch on of ``GP.acquire`` on the same inputs, timed by the
HIP events GP._sweep records around the library call (what bench.py reports as kernel_ms).

Legs:  the benchmark's C3 (N = 4096, D = 8, 1e6 candidates, AGP), C2 (1024, 2, 1e5, BAPE) and the C5 size (1152, 8,
1e6, AGP) on bench.py's inputs;  the worst case -- constant y at the C3 size, where the bound separates nothing and
bound pass + seeds are pure overhead;  the crossover in m at N = 1152 and N = 4096 (switch value 2: pruned at every m).

    python tools/sweep_prune_ab.py [--pairs 10] [--out profiles/r07_sweep_prune_ab.json] [--legs c3,c2,c5,flat,cross]

Prints one JSON document (and writes it to --out): per leg the medians, min / max, the ratio, the seed and surviving
block counts (and the blocks the coarse bound left) and the winner of both legs (they must be equal, bit for bit -- the tool stops if they are not)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": int(len(v))}


def ab(gp, y, T, kind, box, pairs, warmup, on_value):
    import torch
    res = {}
    for sw in (0, on_value):                        # warm-up of both legs (first call: module load, attributes)
        gp.sweep_prune = sw
        for _ in range(warmup):
            res[sw] = gp.acquire(y, T, kind, bounds=box)
    t = {0: [], on_value: []}
    gp.sweep_prune_stats = True
    for _ in range(pairs):
        for sw in (0, on_value):
            gp.sweep_prune = sw
            gp.kernel_events = ev = []
            r = gp.acquire(y, T, kind, bounds=box)
            torch.cuda.synchronize()
            t[sw].append(ev[0][0].elapsed_time(ev[0][1]))
            if (r[0], np.float64(r[1]).view(np.uint64)) != (res[sw][0], np.float64(res[sw][1]).view(np.uint64)):
                raise SystemExit("sweep_prune_ab: result changed between calls: %r vs %r" % (r, res[sw]))
    c = gp.last_prune_counts.cpu().numpy()
    gp.kernel_events = None
    gp.sweep_prune = None
    gp.sweep_prune_stats = False
    if res[0][0] != res[on_value][0] or np.float64(res[0][1]).view(np.uint64) != np.float64(res[on_value][1]).view(np.uint64):
        raise SystemExit("sweep_prune_ab: pruned %r != full %r" % (res[on_value], res[0]))
    off, on = stats(t[0]), stats(t[on_value])
    return {"off": off, "on": on, "on_over_off": on["median_ms"] / off["median_ms"],
            "blocks": (T.shape[0] + 63) // 64, "seed_blocks": int(c[0]), "surviving_blocks": int(c[1]),
            "coarse_blocks": int(c[3]) if len(c) > 3 else None,
            "second_wave_seeds_swept": int(c[4]) if len(c) > 4 else None,
            "tau": float(c[2:3].view(np.float64)[0]), "best": [int(res[0][0]), float(res[0][1])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="c3,c2,c5,flat,cross")
    args = ap.parse_args()
    import torch
    import bench
    from approxposterior_amd import gp as agp
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    legs = args.legs.split(",")
    out = {"tool": "tools/sweep_prune_ab.py", "pairs": args.pairs, "warmup": args.warmup,
           "sweep_source_sha": bench.sweep_source_hash(), "legs": {}}

    def make(n, d, y_of=None):
        X, y = bench.synthetic_c3(n, d)
        if y_of is not None:
            y = y_of(y)
        g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y),
                   white_noise=-12, fit_white_noise=False, device=dev)
        g.compute(X)
        return g, y

    def cands(m, d):
        return torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, d))).to(dev)

    shapes = {"c3": (4096, 8, 1000000, "agp"), "c2": (1024, 2, 100000, "bape"), "c5": (1152, 8, 1000000, "agp")}
    for name in ("c3", "c2", "c5"):
        if name in legs:
            n, d, m, kind = shapes[name]
            g, y = make(n, d)
            r = ab(g, y, cands(m, d), kind, [(-5.0, 5.0)] * d, args.pairs, args.warmup, 1)
            r.update({"n_train": n, "ndim": d, "candidates": m, "utility": kind})
            out["legs"][name] = r
            print(name, json.dumps(r), flush=True)
            del g
    if "flat" in legs:
        n, d, m, kind = shapes["c3"]
        g, y = make(n, d, y_of=lambda y: np.full_like(y, float(np.median(y))))
        r = ab(g, y, cands(m, d), kind, [(-5.0, 5.0)] * d, max(3, args.pairs // 2), 1, 1)
        r.update({"n_train": n, "ndim": d, "candidates": m, "utility": kind, "y": "constant (the worst case)"})
        out["legs"]["flat"] = r
        print("flat", json.dumps(r), flush=True)
        del g
    if "cross" in legs:
        rows = []
        for n in (1152, 4096):
            g, y = make(n, 8)
            for m in (4096, 16384, 65536, 262144):
                r = ab(g, y, cands(m, 8), "agp", [(-5.0, 5.0)] * 8, args.pairs, args.warmup, 2)
                r.update({"n_train": n, "ndim": 8, "candidates": m, "utility": "agp"})
                rows.append(r)
                print("cross", json.dumps(r), flush=True)
            del g
        out["legs"]["cross"] = rows
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
