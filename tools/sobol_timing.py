"""Quasi-random draws (DESIGN.md "Quasi-random draws") at M = 2^20, D = 8, timed with HIP events in one process after a
warm-up, alternating, --reps times each (median, minimum, maximum):
  generators  apgp_sobol_{box,prior,mix}_candidates against their Philox siblings apgp_{box,prior,mix}_candidates into a
              preallocated matrix (the C entry points themselves: no allocation, no Python layer in the timed region);
              the mixture has K = 3 components and writes ln q
  evidence    ApproxPosterior.evidence(nSamples=M, qmc=16) against evidence(nSamples=M) on the N = 1152, D = 8 surrogate of
              a correlated Gaussian log-density (tools/hmc_timing.py problem) for the box, prior and mixture proposals:
              wall time, logZErr of both, ess / M, and over --seeds different seeds the scatter (standard deviation) of
              logZ of both -- the check that the replicate error bar is calibrated: the scatter should be the error bar's
              size -- with every seed's numbers kept.
Usage: python tools/sobol_timing.py [--reps R] [--seeds S] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2 ** 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--qmc", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sobol_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sobol_timing needs an MI355X")
    import hmc_timing as ht
    import approxposterior_amd as apx
    from approxposterior_amd import _lib, gp as agp, priors as P
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def stats(ts):
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)),
                "spread_ms": float(max(ts) - min(ts))}

    M, D, K = a.m, 8, 3
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "M": M, "D": D, "generators": {}, "evidence": {}}
    lib = _lib.load()
    gp, y, b = ht.problem(1152, D)
    stream = gp._stream(torch)

    # ---- generators ------------------------------------------------------------------------------------------------
    T = torch.empty((M, D), dtype=torch.float64, device="cuda")
    lnq = torch.empty(M, dtype=torch.float64, device="cuda")
    lo, hi = agp._box(b, D, optional=False)
    joint = P.JointPrior([P.UniformPrior(-3.0, 3.0) if d % 2 == 0 else P.GaussianPrior(0.0, 1.0) for d in range(D)])
    kind, p0, p1 = agp.GP._prior_records(joint, D)
    rs = np.random.RandomState(5)
    Bm = rs.normal(size=(K, D, D))
    covs = 0.3 * np.einsum("kij,klj->kil", Bm, Bm) / D + 0.05 * np.eye(D)
    _, _, rec = agp.GP._mixture_params(rs.uniform(0.2, 1.0, size=K), rs.uniform(-2, 2, size=(K, D)), covs, 1.0)
    rec = np.ascontiguousarray(rec.ravel())
    pairs = {
        "box": (lambda: lib.apgp_box_candidates(T.data_ptr(), M, D, lo, hi, 7, 0, stream),
                lambda: lib.apgp_sobol_box_candidates(T.data_ptr(), M, D, lo, hi, 7, 0, 1, 0, stream)),
        "prior": (lambda: lib.apgp_prior_candidates(T.data_ptr(), M, D, kind.ctypes.data, p0.ctypes.data, p1.ctypes.data, 7, 0,
                                                    stream),
                  lambda: lib.apgp_sobol_prior_candidates(T.data_ptr(), M, D, kind.ctypes.data, p0.ctypes.data,
                                                          p1.ctypes.data, 7, 0, 1, 0, stream)),
        "mixture": (lambda: lib.apgp_mix_candidates(T.data_ptr(), lnq.data_ptr(), M, D, K, rec.ctypes.data, 7, 0, stream),
                    lambda: lib.apgp_sobol_mix_candidates(T.data_ptr(), lnq.data_ptr(), M, D, K, rec.ctypes.data, 7, 0, 1, 0,
                                                          stream)),
    }
    for name, (philox, sobol) in pairs.items():
        for _ in range(3):
            assert philox() == 0 and sobol() == 0
        torch.cuda.synchronize()
        tp, ts = [], []
        for _ in range(a.reps):                             # alternating: both see the same machine at the same time
            tp.append(timed(philox)[0])
            ts.append(timed(sobol)[0])
        r = {"philox": stats(tp), "sobol": stats(ts)}
        r["sobol_over_philox"] = r["sobol"]["median_ms"] / r["philox"]["median_ms"]
        r["within_the_siblings_spread"] = bool(r["sobol"]["median_ms"] <= r["philox"]["median_ms"] + r["philox"]["spread_ms"])
        r["bytes_stored"] = M * D * 8 + (M * 8 if name == "mixture" else 0)
        r["sobol_store_GBps"] = r["bytes_stored"] / (1e-3 * r["sobol"]["median_ms"]) / 1e9
        print(json.dumps({name: r}), flush=True)
        res["generators"][name] = r

    # ---- evidence --------------------------------------------------------------------------------------------------
    box_prior = lambda t: 0.0 if np.all(np.abs(t) <= 3.0) else -np.inf                             # noqa: E731
    sample = lambda n=1: np.random.uniform(-3, 3, size=(n, D))                                     # noqa: E731
    post = lambda prior: apx.ApproxPosterior(theta=gp._x, y=y, lnprior=prior, lnlike=lambda t: 0.0,     # noqa: E731
                                             priorSample=sample, bounds=[tuple(r) for r in b], gp=gp, distributed=False)
    pilot = post(box_prior).evidence(nSamples=2 ** 22, proposal="box", seed=1)
    mix = ([1.0], [pilot["mean"]], [np.asarray(pilot["cov"])])
    kinds = {"box": (box_prior, "box", {}), "prior": (joint, "prior", {}), "mixture": (box_prior, mix, {"covScale": 1.5})}
    for name, (prior, proposal, kw) in kinds.items():
        obj = post(prior)
        plain = lambda seed: obj.evidence(nSamples=M, proposal=proposal, seed=seed, **kw)          # noqa: E731
        quasi = lambda seed: obj.evidence(nSamples=M, proposal=proposal, seed=seed, qmc=a.qmc, **kw)     # noqa: E731
        plain(11), quasi(11)
        tp, tq = [], []
        for _ in range(a.reps):
            tp.append(timed(lambda: plain(11))[0])
            tq.append(timed(lambda: quasi(11))[0])
        per = {"philox": [], "qmc": []}
        for seed in range(100, 100 + a.seeds):
            for key, fn in (("philox", plain), ("qmc", quasi)):
                o = fn(seed)
                per[key].append({"seed": seed, "logZ": float(o["logZ"]), "logZErr": float(o["logZErr"]),
                                 "ess_over_M": float(o["ess"]) / M, "nInside": int(o["nInside"])})
        r = {"qmc": a.qmc, "philox_ms": stats(tp), "qmc_ms": stats(tq), "seeds": per}
        for key in per:
            lz = np.array([o["logZ"] for o in per[key]])
            r[key + "_logZ_scatter"] = float(np.std(lz, ddof=1))
            r[key + "_logZErr_median"] = float(np.median([o["logZErr"] for o in per[key]]))
            r[key + "_logZ_mean"] = float(lz.mean())
        r["ess_over_M"] = float(np.median([o["ess_over_M"] for o in per["philox"]]))
        r["error_bar_gain"] = r["philox_logZErr_median"] / r["qmc_logZErr_median"]
        r["scatter_gain"] = r["philox_logZ_scatter"] / r["qmc_logZ_scatter"]
        print(json.dumps({name: {k: v for k, v in r.items() if k != "seeds"}}), flush=True)
        res["evidence"][name] = r
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
