"""What a segment boundary of the tempered sampler costs (apgp_tempered_sample: one launch per swapEvery iterations, the
training stream re-staged and the walkers reloaded at each) against the same work without segments or exchanges: T = 8
rungs for swapEvery in 1, 2, 5, 10, 20, 50 beside apgp_ensemble_sample_moves(mode = 1, nensembles = 8) at the same
iterations, for two chains: BASELINE config 5's (64 walkers x 2e4 iterations, N = 1152, D = 8) and the README's (20 x 2e4,
N = 90, D = 2).  Both sides store the chain and log-probability of all eight ensembles, so they write the same bytes; the
tempered call is also timed storing the cold rung alone, as GP.sample_tempered does by default.  Beside them the single
ensemble on several workgroups (mode = 0, nensembles = 1), the sampler a user without a ladder runs: what a cold chain costs
through a ladder against it.

Device events around the C call (buffers allocated before, nothing copied back inside the window), one warm-up round, then
--reps rounds with the configurations alternating inside each round; the JSON keeps every repeat, the median and the
spread (max - min).  --lib times another build's floor (the parent commit's libapgp.so) in a run of its own.

    timeout -k 10 900 python tools/tempering_timing.py --out profiles/tempering_timing.json"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = (("C5", 64, 20000, 1152, 8), ("README", 20, 20000, 90, 2))
SWAP_EVERY = (1, 2, 5, 10, 20, 50)
RUNGS = 8


def problem(N, D):
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(7)
    X = rs.uniform(-5, 5, size=(N, D))
    y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(D, 8.0), ndim=D), fit_mean=True, mean=np.median(y), white_noise=-12,
                fit_white_noise=False)
    gp.compute(X)
    return gp, y, [(-5.0, 5.0)] * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="time this build of libapgp.so (the parent commit's: the floor alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempering_timing.json"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repeats")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tempering_timing needs the GPU")
    from approxposterior_amd import _lib, gp as agp, mcmc
    if args.lib is not None:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    tempered = hasattr(lib, "apgp_tempered_sample") and args.lib is None
    doc = dict(tool="tempering_timing", reps=args.reps, lib=args.lib or "tree", rungs=RUNGS, chains=[])
    for name, W, N, n, D in CHAINS:
        gp, y, bounds = problem(n, D)
        gp.recompute()
        _, dev, _ = gp._rt()
        gp._ensure_xs(gp._check_dimensions(y))
        lo, hi = agp._box(bounds, D, optional=False)
        ks = gp._kernel_struct()
        st = gp._stream(torch)
        T = RUNGS
        betas = mcmc.tempering_ladder(T, 1e-3)
        bb = (ctypes.c_double * T)(*betas)
        p0 = np.random.RandomState(3).uniform(-1, 1, size=(T, W, D))
        f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
        coords = torch.empty((T, W, D), **f64)
        logp, nacc = torch.empty((T, W), **f64), torch.empty((T, W), **i64)
        chain, lchain = torch.empty((N, T, W, D), **f64), torch.empty((N, T, W), **f64)
        sprop, sacc = torch.zeros(T - 1, **i64), torch.zeros(T - 1, **i64)
        work = torch.empty(int(lib.apgp_tempered_work_len(W, T, 1, D)) if tempered else 1, **f64)
        head = (gp._xs.data_ptr(), len(gp._x), ctypes.byref(ks), float(gp.mean.value), lo, hi)

        def floor(E, mode):
            return lambda: lib.apgp_ensemble_sample_moves(*head, W, E, N, 2.0, 11, coords.data_ptr(), logp.data_ptr(),
                                                          chain.data_ptr(), lchain.data_ptr(), nacc.data_ptr(), mode, None, 0, st)

        def ladder(every, nstore):
            return lambda: lib.apgp_tempered_sample(*head, W, T, 1, bb, N, every, 11, coords.data_ptr(), logp.data_ptr(),
                                                    chain.data_ptr(), nstore, lchain.data_ptr(), nacc.data_ptr(),
                                                    sprop.data_ptr(), sacc.data_ptr(), None, None, 0, work.data_ptr(), st)
        configs = [("floor: 8 ensembles, one workgroup each", floor(T, 1)), ("one ensemble, several workgroups", floor(1, 0))]
        if tempered:
            configs += [("swapEvery %d" % e, ladder(e, T)) for e in SWAP_EVERY]
            configs += [("swapEvery %d, cold rung stored" % e, ladder(e, 1)) for e in (10,)]
        runs = {c: [] for c, _ in configs}
        swaps = {}
        for rep in range(-1, args.reps):                 # rep -1: the warm-up
            for cfg, call in configs:
                coords.copy_(torch.from_numpy(p0))
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                _lib.check(call(), cfg)
                t1.record()
                torch.cuda.synchronize()
                assert not torch.isnan(logp[:1 if "one ensemble" in cfg else T]).any(), cfg
                if rep >= 0:
                    runs[cfg].append(round(t0.elapsed_time(t1) * 1e-3, 6))
                if cfg.startswith("swapEvery"):
                    swaps[cfg] = (sacc.cpu().numpy() / np.maximum(sprop.cpu().numpy(), 1)).round(3).tolist()
        med = {c: float(np.median(v)) for c, v in runs.items()}
        base = med["floor: 8 ensembles, one workgroup each"]
        row = dict(chain=name, walkers=W, iterations=N, n=n, ndim=D, betas=[float(b) for b in betas], seconds=runs, median_s=med,
                   spread_s={c: round(max(v) - min(v), 6) for c, v in runs.items()},
                   ratio_to_floor={c: round(m / base, 4) for c, m in med.items()},
                   ratio_to_one_ensemble={c: round(m / med["one ensemble, several workgroups"], 4) for c, m in med.items()},
                   seconds_per_boundary={c: round((med[c] - base) / max(1, -(-N // int(c.split()[1].rstrip(","))) - 1), 9)
                                         for c in med if c.startswith("swapEvery")},
                   exchange_acceptance=swaps)
        doc["chains"].append(row)
        print(json.dumps({k: row[k] for k in ("chain", "median_s", "spread_s", "ratio_to_floor", "seconds_per_boundary")}),
              file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps([dict(chain=r["chain"], ratio_to_floor=r["ratio_to_floor"]) for r in doc["chains"]]))


if __name__ == "__main__":
    main()
