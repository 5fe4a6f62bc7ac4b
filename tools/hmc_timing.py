"""What the on-device HMC sampler (apgp_hmc_sample, GP.sample_hmc) costs and what it buys.

1. Time per leapfrog step for every offered group width G (wavefronts per chain), at D = 8, N = 1152 with 64 chains, at
   D = 32, N = 1152 with 64 chains and at D = 2, N = 90 with 20 chains: one call of ``--iters`` iterations of L = 32 steps
   without any stored output, timed with a host clock around the call (it ends in the copy of the final state, a device
   synchronise), minus the same call with a fifth of the iterations -- the slope, which leaves launch, upload and copies
   out.  The G rule of csrc/hmc.hip is read off this table.
2. The same trajectory driven from the host: one ``GP.predict_grad(kind=None)`` call per leapfrog step for all chains at
   once (the kicks and the drift are NumPy on C x D numbers), time per step.  The device step must be faster at every size.
3. Effective samples per second on a surrogate of a correlated Gaussian log-density at D = 8 and D = 32 (N = 1152): HMC
   (64 chains; the warm-up's time is counted) against ``GP.sample_ensemble`` with 64 walkers (the stretch move), each given
   about ``--budget`` seconds of wall clock by sizing its iterations from a pilot run.  ESS = samples / tau with tau from
   ``mcmc.integrated_time`` (quiet), the worst dimension; a chain too short for its tau is reported as such.

One warm-up round, then --reps rounds with the configurations alternating inside each round; the JSON keeps every repeat,
the median and the spread (max - min).

    timeout -k 10 900 python tools/hmc_timing.py --out profiles/hmc_timing.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (("D8", 8, 1152, 64), ("D32", 32, 1152, 64), ("README", 2, 90, 20))
LEAP = 32


def problem(N, D, seed=7):
    """A GP surrogate of a correlated Gaussian log-density on [-3, 3]^D."""
    from approxposterior_amd import gp as agp
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((D, D)) * 0.3 + np.eye(D)
    cov = (A @ A.T) / D * 0.5 + 0.1 * np.eye(D)
    P = np.linalg.inv(cov)
    X = rs.uniform(-3, 3, size=(N, D))
    y = -0.5 * np.einsum("ni,ij,nj->n", X, P, X)
    gp = agp.GP(kernel=np.var(y) * agp.ExpSquaredKernel(np.full(D, 2.0 * D), ndim=D), fit_mean=True, mean=float(np.mean(y)),
                white_noise=-6.0, fit_white_noise=False)
    gp.compute(X)
    return gp, y, np.array([(-3.0, 3.0)] * D)


def stats(v):
    v = [float(x) for x in v]
    return {"repeats": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))}


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def host_steps(gp, y, p0, b, eps, nsteps):
    """nsteps leapfrog steps of all chains with one predict_grad call per step (scaled coordinates, unit mass)."""
    sc = gp.hmc_scale()
    q = p0 * sc
    p = np.random.RandomState(1).standard_normal(q.shape)
    g = np.asarray(gp.predict_grad(y, q / sc, kind=None)[2]) / sc
    lo, hi = b[:, 0] * sc, b[:, 1] * sc
    for _ in range(nsteps):
        p = p + 0.5 * eps * g
        q = q + eps * p
        over, under = q > hi, q < lo
        q = np.where(over, 2 * hi - q, np.where(under, 2 * lo - q, q))
        p = np.where(over | under, -p, p)
        g = np.asarray(gp.predict_grad(y, q / sc, kind=None)[2]) / sc
        p = p + 0.5 * eps * g
    return q


def ess_of(chain, mcmc):
    """(ess, tau of the worst dimension, reliable) of a (T, W, D) chain."""
    tau = np.asarray(mcmc.integrated_time(chain, quiet=True), dtype=np.float64)
    worst = float(np.nanmax(tau))
    return chain.shape[0] * chain.shape[1] / worst, worst, bool(chain.shape[0] >= 50 * worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--budget", type=float, default=1.0, help="seconds of wall clock per sampler in the ESS comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_timing.json"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repeats")
    import torch
    from approxposterior_amd import _lib, mcmc
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "leap": LEAP, "iters": args.iters, "step": {},
           "host_step": {}, "ess": {}}
    for name, D, N, C in SIZES:
        gp, y, b = problem(N, D)
        p0 = np.random.RandomState(3).uniform(-0.5, 0.5, size=(C, D))
        eps = 0.02
        few = max(args.iters // 5, 1)
        run = lambda it, G: gp.sample_hmc(y, p0, it, b, eps, LEAP, jitter=0.1, seed=1, store=False, gRows=G)      # noqa: E731
        nhost = 40
        rows = {G: [] for G in _lib.HMC_G_ROWS}
        host = []
        for rep in range(args.reps + 1):
            for G in _lib.HMC_G_ROWS:
                dt = clock(lambda: run(args.iters, G)) - clock(lambda: run(few, G))
                if rep:
                    rows[G].append(dt / ((args.iters - few) * LEAP))
            dt = clock(lambda: host_steps(gp, y, p0, b, eps, nhost)) - clock(lambda: host_steps(gp, y, p0, b, eps, nhost // 5))
            if rep:
                host.append(dt / (nhost - nhost // 5))
        out["step"][name] = {"D": D, "N": N, "chains": C, "rule": int(_lib.load().apgp_hmc_rule(C, N, D)),
                             "seconds_per_step": {str(G): stats(v) for G, v in rows.items()}}
        out["host_step"][name] = {"seconds_per_step": stats(host)}
        best = min(np.median(v) for v in rows.values())
        out["host_step"][name]["host_over_best_device"] = float(np.median(host) / best)
        print(name, {G: "%.2f us" % (1e6 * np.median(v)) for G, v in rows.items()}, "host %.1f us" % (1e6 * np.median(host)),
              flush=True)
    for name, D, N, C in SIZES[:2]:
        gp, y, b = problem(N, D)
        p0 = np.random.RandomState(3).uniform(-0.3, 0.3, size=(C, D))
        L = 8
        # pilots size the runs to the budget
        t_h = clock(lambda: gp.sample_hmc(y, p0, 50, b, 0.05, L, seed=1))
        t_e = clock(lambda: gp.sample_ensemble(y, p0, 500, b, seed=1))
        t_h = clock(lambda: gp.sample_hmc(y, p0, 50, b, 0.05, L, seed=1))
        t_e = clock(lambda: gp.sample_ensemble(y, p0, 500, b, seed=1))
        n_h = max(int(args.budget / (t_h / 50)) - 200, 200)
        n_e = max(int(args.budget / (t_e / 500)), 1000)
        rec = {"D": D, "N": N, "walkers": C, "hmc": {"iterations": n_h, "warmup": 200, "nLeap": L, "runs": []},
               "ensemble": {"iterations": n_e, "runs": []}}
        for rep in range(args.reps):
            def hmc():
                coords, eps, mass, hist, it = mcmc.hmc_warmup(gp, y, p0, b, 0.05, L, nWarmup=200, adaptEvery=20, seed=rep)
                hmc.res = gp.sample_hmc(y, coords, n_h, b, eps, L, seed=rep, iteration0=it)
            dt = clock(hmc)
            ess, tau, ok = ess_of(hmc.res["chain"], mcmc)
            rec["hmc"]["runs"].append({"seconds": dt, "ess": ess, "tau": tau, "tau_reliable": ok, "ess_per_second": ess / dt,
                                       "eps": hmc.res["eps"], "accept": float(hmc.res["accept_prob"].mean())})

            def ens():
                ens.res = gp.sample_ensemble(y, p0, n_e, b, seed=rep)
            dt = clock(ens)
            ess, tau, ok = ess_of(ens.res["chain"][n_e // 5:], mcmc)
            rec["ensemble"]["runs"].append({"seconds": dt, "ess": ess, "tau": tau, "tau_reliable": ok,
                                            "ess_per_second": ess / dt,
                                            "accept": float(ens.res["naccept"].mean() / n_e)})
        for k in ("hmc", "ensemble"):
            rec[k]["ess_per_second"] = stats([r["ess_per_second"] for r in rec[k]["runs"]])
            rec[k]["tau"] = stats([r["tau"] for r in rec[k]["runs"]])
        rec["hmc_over_ensemble"] = rec["hmc"]["ess_per_second"]["median"] / rec["ensemble"]["ess_per_second"]["median"]
        out["ess"][name] = rec
        print(name, "ESS/s hmc %.0f (tau %.1f) ensemble %.0f (tau %.1f)" % (
            rec["hmc"]["ess_per_second"]["median"], rec["hmc"]["tau"]["median"], rec["ensemble"]["ess_per_second"]["median"],
            rec["ensemble"]["tau"]["median"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
