"""What the on-device nested sampler (apgp_nested_sample, GP.sample_nested) costs and what it buys.

1. Time per likelihood call at D = 8, N = 1152 and at D = 2, N = 90 (nlive 512, batch 16, a run per compute unit): one call
   of ``--batches`` batches with dlogz = 0, the launch timed between two events on its stream (``timeDevice``), minus the
   same call with a fifth of the batches -- the slope, which leaves the start values and the final flush out -- divided
   by the likelihood calls of a run in between; and the same slope per step of a batch (all 16 walkers).  Beside it
   the per-proposal time of the single-workgroup ensemble kernel (the same mean evaluation; 64 walkers, an ensemble per
   compute unit, the slope over iterations): the difference is what ordering, draws and bookkeeping cost.
2. The same algorithm driven from the host: tests/nested_ref.py's loop with the means taken from ``GP.predict`` on the
   device, one run, time per likelihood call.
3. Wall time and logZErr of a whole default run on the D = 8 Gaussian surrogate and on the two-well surrogate of the
   tests, beside ``evidence()`` (a widened one-Gaussian mixture proposal on the Gaussian, the box proposal on the wells)
   and, on the wells, ``TemperedChain.log_evidence()``; ``seconds_to_nested_error`` scales the other estimator's time by
   (its error / nested's)^2 -- an extrapolation by the 1 / sqrt(n) law, not a measurement.
4. nruns from 1 to the compute-unit count on the D = 8 Gaussian: the launch's time, the wall time of the whole call (with
   the copies and the host's accounting, which grow with the points written) and logZErr.

One warm-up round, then --reps rounds; the JSON keeps every repeat, the median and the spread (max - min).

    timeout -k 10 900 python tools/nested_timing.py --out profiles/nested_timing.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SIZES = (("D8", 8, 1152), ("README", 2, 90))
NLIVE, BATCH = 512, 16


def stats(v):
    v = [float(x) for x in v]
    return {"repeats": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))}


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class DeviceMean(object):
    """nested_ref's target with the means taken from GP.predict on the device (scaled coordinates in, as the reference asks)."""

    def __init__(self, gp, y):
        self.gp, self.y, self.sc = gp, y, gp.hmc_scale()

    def mg(self, q, G=1, budgets=False):
        return np.asarray(self.gp.predict(self.y, np.atleast_2d(q) / self.sc, return_cov=False), dtype=np.float64).ravel(), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_timing.json"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repeats")
    import torch
    import hmc_timing as ht
    import nested_ref as nr
    from approxposterior_amd import _lib, approx, mcmc
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    out = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": args.reps, "nlive": NLIVE, "batch": BATCH,
           "batches": args.batches, "call": {}, "host": {}, "whole": {}, "nruns": {}}
    lib = _lib.load()
    for name, D, N in SIZES:
        gp, y, b = ht.problem(N, D)
        nsteps = max(20, 5 * D)
        few = max(args.batches // 5, 1)
        run = lambda mb: gp.sample_nested(y, b, nlive=NLIVE, batch=BATCH, nsteps=nsteps, nruns=cus, dlogz=0.0,      # noqa: E731
                                          maxBatches=mb, seed=1, timeDevice=True)
        W, iters = 64, 200
        p0 = np.random.RandomState(3).uniform(-0.5, 0.5, size=(cus, W, D))
        ens = lambda it: gp.sample_ensemble(y, p0, it, b, seed=1, store=False)                                         # noqa: E731
        nest, ensemble, host, step = [], [], [], []
        target = DeviceMean(gp, y)
        prev = lib.apgp_ensemble_mode(1)
        try:
            for rep in range(args.reps + 1):
                r1, r0 = run(args.batches), run(few)
                t1, t0 = r1.info["deviceSeconds"], r0.info["deviceSeconds"]
                calls = float(np.mean(r1.ncall - r0.ncall))
                steps = float((args.batches - few) * nsteps)
                (e1, _), (e0, _) = clock(lambda: ens(iters)), clock(lambda: ens(iters // 5))
                h1, ha = clock(lambda: nr.run_one(target, b[:, 0], b[:, 1], target.sc, NLIVE, BATCH, nsteps, 10, 0.0, 1, 0))
                h0, hb = clock(lambda: nr.run_one(target, b[:, 0], b[:, 1], target.sc, NLIVE, BATCH, nsteps, 2, 0.0, 1, 0))
                if rep:
                    nest.append((t1 - t0) / calls)
                    step.append((t1 - t0) / steps)
                    ensemble.append((e1 - e0) / ((iters - iters // 5) * W))
                    host.append((h1 - h0) / (ha["ncall"] - hb["ncall"]))
        finally:
            lib.apgp_ensemble_mode(prev)
        out["call"][name] = {"D": D, "N": N, "nsteps": nsteps, "runs": cus, "calls_per_run": calls,
                             "seconds_per_likelihood_call": stats(nest), "seconds_per_step_of_a_batch": stats(step),
                             "evaluated_share_of_steps": calls / (steps * BATCH),
                             "ensemble_seconds_per_proposal": stats(ensemble),
                             "nested_over_ensemble": float(np.median(nest) / np.median(ensemble))}
        out["host"][name] = {"seconds_per_likelihood_call": stats(host),
                             "host_over_device": float(np.median(host) / np.median(nest))}
        print(name, "device %.2f us per call, ensemble %.2f us per proposal, host %.1f us per call" % (
            1e6 * np.median(nest), 1e6 * np.median(ensemble), 1e6 * np.median(host)), flush=True)

    # whole runs
    import test_gpu_hmc as th
    import test_gpu_tempering as tt
    X, y8, gp8, b8 = th._gauss_problem(8, 300, 12)
    ap8 = approx.ApproxPosterior(theta=X, y=y8, gp=gp8, lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                                 priorSample=lambda m: np.random.uniform(b8[:, 0], b8[:, 1], size=(m, 8)), bounds=b8,
                                 algorithm="agp", distributed=False)
    box = ap8.evidence(nSamples=2 ** 21, proposal="box", seed=1)
    mix = ([1.0], [box["mean"]], [np.asarray(box["cov"])])
    z = tt._two_wells()
    apw = approx.ApproxPosterior(theta=z["X"], y=z["y"], gp=z["gp"], lnprior=lambda t: 0.0, lnlike=lambda t: 0.0,
                                 priorSample=lambda m: np.random.uniform(-2, 2, size=(m, 2)), bounds=z["bounds"],
                                 algorithm="agp", distributed=False)
    rows = {"D8": {"nested": [], "evidence_mixture": []}, "wells": {"nested": [], "evidence_box": [], "tempering": []}}
    for rep in range(args.reps + 1):
        t, r = clock(lambda: ap8.runNested(nsteps=40, seed=rep))
        te, e = clock(lambda: ap8.evidence(nSamples=2 ** 19, proposal=mix, covScale=1.5, seed=rep))
        tw, rw = clock(lambda: apw.runNested(nsteps=20, seed=rep))
        tb, eb = clock(lambda: apw.evidence(nSamples=2 ** 18, proposal="box", seed=rep))
        p0 = np.array([-1.25, -0.25]) + 0.05 * np.random.RandomState(3).standard_normal((8, 2))
        tp, ch = clock(lambda: mcmc.TemperedChain(z["gp"].sample_tempered(z["y"], p0, 4000, z["bounds"], z["betas"], seed=rep,
                                                                        ladders=8)))
        lz, disc, mc = ch.log_evidence(discard=1000)
        if rep:
            rows["D8"]["nested"].append((t, r.logZ, r.logZErr, r.logZRunsErr))
            rows["D8"]["evidence_mixture"].append((te, e["logZ"], e["logZErr"], float("nan")))
            rows["wells"]["nested"].append((tw, rw.logZ, rw.logZErr, rw.logZRunsErr))
            rows["wells"]["evidence_box"].append((tb, eb["logZ"], eb["logZErr"], float("nan")))
            rows["wells"]["tempering"].append((tp, lz, float(np.hypot(disc, mc)), float("nan")))
    for prob, d in rows.items():
        out["whole"][prob] = {}
        for k, v in d.items():
            v = np.array(v)
            out["whole"][prob][k] = {"seconds": stats(v[:, 0]), "logZ": stats(v[:, 1]), "logZErr": stats(v[:, 2])}
            if k == "nested":
                out["whole"][prob][k]["logZRunsErr"] = stats(v[:, 3])
        ne = out["whole"][prob]["nested"]["logZErr"]["median"]
        for k in d:
            if k != "nested":
                o = out["whole"][prob][k]
                o["seconds_to_nested_error"] = o["seconds"]["median"] * (o["logZErr"]["median"] / ne) ** 2
        print(prob, {k: "%.3f s, logZ %.3f +- %.4f" % (v["seconds"]["median"], v["logZ"]["median"], v["logZErr"]["median"])
                     for k, v in out["whole"][prob].items()}, flush=True)

    # nruns scaling on the D = 8 Gaussian
    ladder = sorted(set([1, 4, 16, 64, cus]))
    sc = {k: [] for k in ladder}
    for rep in range(args.reps + 1):
        for k in ladder:
            t, r = clock(lambda: gp8.sample_nested(y8, b8, nsteps=40, nruns=k, seed=100 + rep, timeDevice=True))
            if rep:
                sc[k].append((t, r.logZErr, r.logZ, r.info["deviceSeconds"]))
    for k, v in sc.items():
        v = np.array(v)
        out["nruns"][str(k)] = {"seconds": stats(v[:, 0]), "device_seconds": stats(v[:, 3]), "logZErr": stats(v[:, 1]),
                                "logZ": stats(v[:, 2])}
    print("nruns", {k: "%.3f s (launch %.3f s), logZErr %.4f" % (v["seconds"]["median"], v["device_seconds"]["median"],
                                                                  v["logZErr"]["median"]) for k, v in out["nruns"].items()},
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
