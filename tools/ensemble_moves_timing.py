"""Time and bits of a device chain (GP.sample_ensemble, device events around the call, after a warm-up) under the stretch
move, DE, the snooker, the 0.8 / 0.2 DE + snooker mixture and the stretch chain sent through the kernels that hold every
move, the configurations alternating within one process, for two chains:
BASELINE config 5's (64 walkers x 2e4 iterations, N = 1152, D = 8, one ensemble) and the README's (20 x 2e4, N = 90,
D = 2).  --mode picks the kernel (0: several workgroups per ensemble where that helps, the default; 1: the
single-workgroup kernel).  Writes one JSON document with every repeat and, for every configuration, the SHA-256 of chain,
log_prob, naccept and final_log_prob.  A third, short set of chains is hashed only, not timed: the instantiations the two
long chains (DPAD 8 and 2, training stream in LDS, one ensemble) never reach.

The yardstick is the parent commit: run this script with --lib on a build of the parent's libapgp.so in the same session,
and hand its output to the second run with --parent; that run then records, per configuration, whether the four hashes
are the parent's and whether the median time lies within the parent's own spread (max - min over its repeats) of the
parent's median.

    timeout -k 10 600 python tools/ensemble_moves_timing.py --mode 0 --lib /path/to/parent/libapgp.so --out parent.json
    timeout -k 10 600 python tools/ensemble_moves_timing.py --mode 0 --parent parent.json --out profiles/ensemble_moves_timing.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = (("C5", 64, 20000, 1152, 8), ("README", 20, 20000, 90, 2))
# hashed only: name, D, W, n, ensembles, linear term's order (0: none), iterations
SHORT = (("D3 se+lin1", 3, 34, 400, 1, 1, 120), ("D9 n300 (DPAD 16, stream in LDS)", 9, 18, 300, 1, 0, 100),
         ("D9 n700 (DPAD 16, stream in L2)", 9, 18, 700, 1, 0, 100), ("D17 (DPAD 32)", 17, 34, 300, 1, 0, 100),
         ("E3 W6", 2, 6, 300, 3, 0, 100))
HASHED = ("chain", "log_prob", "naccept", "final_log_prob")


def problem(N, D, W, E=1, lin=0):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(7)
    X = rs.uniform(-5, 5, size=(N, D))
    if D > 1:
        y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
    else:
        y = -X[:, 0] ** 2
    k = agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D)
    if lin:
        k = k + 0.3 * agp.kernels.LinearKernel(log_gamma2=0.4, order=lin, bounds=None, ndim=D)
    gp = agp.GP(kernel=k, fit_mean=True, mean=np.median(y), white_noise=-12 if not lin else -4.0, fit_white_noise=False)
    gp.compute(X)
    p0 = rs.uniform(-1, 1, size=(W, D) if E == 1 else (E, W, D))
    return gp, y, p0, [(-5.0, 5.0)] * D


def hashes(res):
    return {k: hashlib.sha256(np.ascontiguousarray(res[k]).tobytes()).hexdigest() for k in HASHED}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", type=int, choices=(0, 1), default=0, help="apgp_ensemble_mode for the run (restored afterwards)")
    ap.add_argument("--lib", default=None, help="time this build of libapgp.so instead of the tree's (the parent commit's)")
    ap.add_argument("--stretch-only", action="store_true", help="the stretch configuration alone")
    ap.add_argument("--parent", default=None, help="JSON written by a --lib run on the parent's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_moves_timing.json"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repeats")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_moves_timing needs the GPU")
    from approxposterior_amd import _lib, mcmc
    if args.lib is not None:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    configs = [("stretch", None)]
    if not args.stretch_only:
        # "stretch, all-moves kernels": a DE entry whose weight vanishes beside 1 (the cumulative weight of the stretch
        # entry rounds to 1, so every iteration takes it and the chain is the stretch chain, hash checked) sends the
        # launch to the kernel instantiation that holds every move: what the default would cost without the
        # stretch-only instantiation
        configs += [("de", mcmc.DEMove()), ("snooker", mcmc.DESnookerMove()),
                    ("de0.8+snooker0.2", [(mcmc.DEMove(), 0.8), (mcmc.DESnookerMove(), 0.2)]),
                    ("stretch, all-moves kernels", [(mcmc.StretchMove(), 1.0), (mcmc.DEMove(), 1e-300)])]
    doc = dict(tool="ensemble_moves_timing", reps=args.reps, mode=args.mode, lib=args.lib or "tree", chains=[], short=[])
    lib = _lib.load()
    prev = lib.apgp_ensemble_mode(args.mode)
    try:
        for name, W, T, N, D in CHAINS:
            gp, y, p0, bounds = problem(N, D, W)
            runs = {c: [] for c, _ in configs}
            acc, sha = {}, {}
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
                    h = hashes(res)
                    assert sha.setdefault(cfg, h) == h, "the %s chain is not reproducible" % cfg
            assert sha["stretch"] == sha.get("stretch, all-moves kernels", sha["stretch"]), "the all-moves kernels' stretch chain"
            row = dict(chain=name, walkers=W, iterations=T, n=N, ndim=D, sha256=sha,
                       fallbacks=getattr(gp, "ensemble_fallbacks", 0) - fb0, acceptance=acc,
                       seconds={c: runs[c] for c, _ in configs}, median_s={c: float(np.median(runs[c])) for c, _ in configs})
            doc["chains"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        for name, D, W, N, E, lin, T in SHORT:
            gp, y, p0, bounds = problem(N, D, W, E, lin)
            fb0 = getattr(gp, "ensemble_fallbacks", 0)
            sha = {cfg: hashes(gp.sample_ensemble(y, p0, T, bounds, seed=11, **({} if moves is None else {"moves": moves})))
                   for cfg, moves in configs}
            row = dict(chain=name, walkers=W, iterations=T, n=N, ndim=D, ensembles=E, sha256=sha,
                       fallbacks=getattr(gp, "ensemble_fallbacks", 0) - fb0)
            doc["short"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    finally:
        lib.apgp_ensemble_mode(prev)
    if args.parent is not None:
        with open(args.parent) as fh:
            parent = json.load(fh)
        assert parent["mode"] == args.mode, "the parent's run was of the other kernel"
        doc["parent"] = parent
        doc["against_parent"] = []
        for row, prow in zip(doc["chains"] + doc["short"], parent["chains"] + parent["short"]):
            assert row["chain"] == prow["chain"]
            out = dict(chain=row["chain"], same_chain={c: h == prow["sha256"].get(c) for c, h in row["sha256"].items()})
            if "seconds" in row:
                out["parent_median_s"], out["parent_spread_s"], out["median_s"] = {}, {}, row["median_s"]
                out["within_parent_spread"], out["ratio_to_parent"] = {}, {}
                for c, m in row["median_s"].items():
                    ps = prow["seconds"][c]
                    spread, pmed = max(ps) - min(ps), float(np.median(ps))
                    out["parent_median_s"][c], out["parent_spread_s"][c] = pmed, round(spread, 6)
                    out["within_parent_spread"][c] = bool(abs(m - pmed) <= spread)
                    out["ratio_to_parent"][c] = round(m / pmed, 4)
            doc["against_parent"].append(out)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc.get("against_parent", doc["chains"] + doc["short"])))


if __name__ == "__main__":
    main()
