#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Prices of a re-read and of a generating tile of the parked seed launch's row items, by round 27's procedure
(docs/experiments.md): a first wave of no more items than CUs lasts its heaviest item, row block nrb - 1 with
16 (nrb - 1) re-read and 16 generating tiles, so the launch times at N = 4096 and 2048 give both prices and N = 1024 checks
them.  Two steps:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/seed_tile_prices.py run DIR/order.json
    python tools/seed_tile_prices.py solve DIR/order.json DIR/t_kernel_trace.csv [--out profiles/...json]

`run` makes, per (N, pairs per item, prefetch distance), CALLS pruned calls with every row block split (seed_rowsplit 0)
and a first wave of K seeds (two waves: two row-part launches per call, the first wave's the longer), and writes the
order of the configurations; `solve` takes the row-part launches of the trace in time order, CALLS pairs per
configuration, and solves median(4096) = 240 a + 16 b, median(2048) = 112 a + 16 b."""
import collections
import csv
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 6
SIZES = (4096, 2048, 1024)
# pairs per item -> seeds of the first wave (items of a seed at N = 4096: 32 / 64 / 128 for 4 / 2 / 1 pairs)
FIRST = {4: 4, 2: 4, 1: 2}
DISTANCES = (0, 6)


def run(order_path):
    import torch
    import bench
    from approxposterior_amd import gp as agp
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, m = 8, 1000000
    T = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, d))).to(dev)
    order = []
    for n in SIZES:
        X, y = bench.synthetic_c3(n, d)
        g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y), white_noise=-12,
                   fit_white_noise=False, device=dev)
        g.compute(X)
        g.sweep_prune, g.seed_rowsplit = 1, 0
        for pairs, first in FIRST.items():
            for dist in DISTANCES:
                g.seed_parts, g.seed_first, g.seed_prefetch = pairs, first, dist
                for _ in range(CALLS):
                    g.acquire(y, T, "agp", bounds=[(-5.0, 5.0)] * d)
                torch.cuda.synchronize()
                order.append({"n": n, "pairs": pairs, "first": first, "distance": dist})
        del g
    with open(order_path, "w") as f:
        json.dump({"calls": CALLS, "order": order}, f)


def solve(order_path, trace_path, out_path=None):
    meta = json.load(open(order_path))
    calls = meta["calls"]
    rows = []
    for r in csv.DictReader(open(trace_path)):
        if re.search(r"sweep2_kernel<\d+, false, 0, true, true", r["Kernel_Name"]):
            t0 = int(r["Start_Timestamp"])
            rows.append((t0, (int(r["End_Timestamp"]) - t0) / 1e3))
    rows.sort()
    us = [d for _, d in rows]
    if len(us) != 2 * calls * len(meta["order"]):
        raise SystemExit("seed_tile_prices: %d row-part launches, expected %d" % (len(us), 2 * calls * len(meta["order"])))
    med = {}
    for k, cfg in enumerate(meta["order"]):
        chunk = us[2 * calls * k:2 * calls * (k + 1)]
        first = [max(chunk[i], chunk[i + 1]) for i in range(0, len(chunk), 2)][1:]        # (the first call: warm-up)
        med[(cfg["n"], cfg["pairs"], cfg["distance"])] = statistics.median(first)
    out = collections.OrderedDict()
    for pairs in FIRST:
        for dist in DISTANCES:
            t4, t2, t1 = (med[(n, pairs, dist)] for n in SIZES)
            a = (t4 - t2) / 128.0
            b = (t2 - 112.0 * a) / 16.0
            out["pairs %d, distance %d" % (pairs, dist)] = {
                "launch_us": {"4096": t4, "2048": t2, "1024": t1}, "re_read_us": a, "generating_us": b,
                "modelled_1024_us": 48.0 * a + 16.0 * b}
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


def table(out_path=None, rounds=7):
    """Round 27's table again: the pruned call at the C3 and the C5 size by K (seeds of the first wave) and pairs per
    item, and what the library's rule gives (K = pairs = -1), ms per call by the events of GP._sweep, median of `rounds`
    calls per setting."""
    import torch
    import bench
    from approxposterior_amd import gp as agp
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, m = 8, 1000000
    T = torch.from_numpy(np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, d))).to(dev)
    # (the rule's row first and again last: the first rows of a process are timed on a chip that is still warming up)
    settings = [(-1, -1, "")] + [(k, p, "") for k in (2, 4, 8, 16) for p in (8, 4, 2, 1)] + [(-1, -1, " again")]
    out = {}
    for n in (4096, 1152):
        X, y = bench.synthetic_c3(n, d)
        g = agp.GP(kernel=agp.ExpSquaredKernel(np.full(d, 8.0), ndim=d), fit_mean=True, mean=np.median(y), white_noise=-12,
                   fit_white_noise=False, device=dev)
        g.compute(X)
        g.sweep_prune = 1
        t = {s: [] for s in settings}
        want = None
        # (a setting at a time: the library remembers its last few launch plans, and a walk through all settings
        # would have it work every plan out again on the host, inside the timed interval)
        for s in settings:
            g.seed_first, g.seed_parts = s[0], s[1]
            for rnd in range(rounds + 2):           # (two warm-up calls)
                g.kernel_events = ev = []
                r = g.acquire(y, T, "agp", bounds=[(-5.0, 5.0)] * d)
                torch.cuda.synchronize()
                got = (int(r[0]), int(np.float64(r[1]).view(np.uint64)))
                want = got if want is None else want
                if got != want:
                    raise SystemExit("seed_tile_prices: winner %r != %r at n=%d K=%d pairs=%d" % (got, want, n, s[0], s[1]))
                if rnd > 1:
                    t[s].append(ev[0][0].elapsed_time(ev[0][1]))
        out[str(n)] = {"K=%d pairs=%d%s" % s: round(float(np.median(t[s])), 4) for s in settings}
        print(n, json.dumps(out[str(n)]), flush=True)
        del g
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "table":
        table(sys.argv[2] if len(sys.argv) > 2 else None)
    elif sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        solve(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--out" else None)
