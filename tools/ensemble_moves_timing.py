"""Time of a device chain (GP.sample_ensemble, device events around the call, after a warm-up) under the stretch move, DE,
the snooker, the 0.8 / 0.2 DE + snooker mixture and the stretch chain sent through the kernels that hold every move, the
configurations alternating within one process, for two chains:
BASELINE config 5's (64 walkers x 2e4 iterations, N = 1152, D = 8, one ensemble) and the README's (20 x 2e4, N = 90,
D = 2).  Writes one JSON document with every repeat and the SHA-256 of the stretch chain.

The yardstick is the parent commit: run this script with --lib on a build of the parent's libapgp.so (stretch only: it has
no move table) in the same session, and hand its output to the second run with --parent; that run then records whether
the stretch chain's hash is the parent's, whether the stretch time lies within the parent's own spread (max - min over its
repeats), and the ratio of every configuration to the parent's stretch time.

    timeout -k 10 300 python tools/ensemble_moves_timing.py --lib /path/to/parent/libapgp.so --out parent.json
    timeout -k 10 600 python tools/ensemble_moves_timing.py --parent parent.json --out profiles/ensemble_moves_timing.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = (("C5", 64, 20000, 1152, 8), ("README", 20, 20000, 90, 2))


def problem(N, D, W):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(7)
    X = rs.uniform(-5, 5, size=(N, D))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                fit_white_noise=False)
    gp.compute(X)
    return gp, y, rs.uniform(-1, 1, size=(W, D)), [(-5.0, 5.0)] * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="time this build of libapgp.so instead of the tree's (the parent commit's)")
    ap.add_argument("--stretch-only", action="store_true", help="time the stretch chain alone, as a --lib run of the parent does")
    ap.add_argument("--parent", default=None, help="JSON written by a --lib run on the parent's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_moves_timing.json"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repeats")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_moves_timing needs the GPU")
    from approxposterior_amd import _lib, mcmc
    with_moves = True
    if args.lib is not None:
        import ctypes
        _lib.LIB_PATH = os.path.abspath(args.lib)
        if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "apgp_ensemble_sample_moves"):
            with_moves = False
            del _lib.SIGNATURES["apgp_ensemble_sample_moves"]
    configs = [("stretch", None)]
    if with_moves and not args.stretch_only:
        # "stretch, all-moves kernels": a DE entry whose weight vanishes beside 1 (the cumulative weight of the stretch
        # entry rounds to 1, so every iteration takes it and the chain is the stretch chain, hash checked) sends the
        # launch to the kernel instantiation that holds every move: what the default would cost without the
        # stretch-only instantiation
        configs += [("de", mcmc.DEMove()), ("snooker", mcmc.DESnookerMove()),
                    ("de0.8+snooker0.2", [(mcmc.DEMove(), 0.8), (mcmc.DESnookerMove(), 0.2)]),
                    ("stretch, all-moves kernels", [(mcmc.StretchMove(), 1.0), (mcmc.DEMove(), 1e-300)])]
    doc = dict(tool="ensemble_moves_timing", reps=args.reps, lib=args.lib or "tree", chains=[])
    for name, W, T, N, D in CHAINS:
        gp, y, p0, bounds = problem(N, D, W)
        runs = {c: [] for c, _ in configs}
        acc, sha = {}, None
        fb0 = getattr(gp, "ensemble_fallbacks", 0)
        for rep in range(-1, args.reps):                 # rep -1: the warm-up
            for cfg, moves in configs:
                kw = {} if moves is None else {"moves": moves}
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                res = gp.sample_ensemble(y, p0, T, bounds, seed=11, **kw)
                t1.record()
                torch.cuda.synchronize()
                if rep >= 0:
                    runs[cfg].append(round(t0.elapsed_time(t1) * 1e-3, 6))
                acc[cfg] = round(float(res["naccept"].sum()) / (T * W), 4)
                if cfg.startswith("stretch"):
                    h = hashlib.sha256(np.ascontiguousarray(res["chain"]).tobytes()).hexdigest()
                    assert sha in (None, h), "the stretch chain is not reproducible"
                    sha = h
        row = dict(chain=name, walkers=W, iterations=T, n=N, ndim=D, stretch_chain_sha256=sha,
                   fallbacks=getattr(gp, "ensemble_fallbacks", 0) - fb0, acceptance=acc,
                   seconds={c: runs[c] for c, _ in configs}, median_s={c: float(np.median(runs[c])) for c, _ in configs})
        doc["chains"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if args.parent is not None:
        with open(args.parent) as fh:
            parent = json.load(fh)
        doc["parent"] = parent
        doc["against_parent"] = []
        for row, prow in zip(doc["chains"], parent["chains"]):
            ps = prow["seconds"]["stretch"]
            spread, pmed = max(ps) - min(ps), float(np.median(ps))
            doc["against_parent"].append(dict(
                chain=row["chain"], parent_stretch_median_s=pmed, parent_spread_s=round(spread, 6),
                same_stretch_chain=row["stretch_chain_sha256"] == prow["stretch_chain_sha256"],
                stretch_within_parent_spread=bool(abs(row["median_s"]["stretch"] - pmed) <= spread),
                ratio_to_parent_stretch={c: round(m / pmed, 4) for c, m in row["median_s"].items()}))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc.get("against_parent", doc["chains"])))


if __name__ == "__main__":
    main()
