"""Evidence by importance sampling (DESIGN.md "Evidence by importance sampling") at M = 2^20, D = 8, N = 1152 and N = 4096:
two ways to the same record on the same box, timed with HIP events in one process after a warm-up, alternating, --reps
times each (median, minimum, maximum):
  pass         one GP.importance_pass (apgp_importance_pass: log w, maxima, moments, reduction; the record's copy to the host)
  composition  what the parent needs: apgp_predict_mean over the same rows, then the gate, the weights about their maximum
               and the moments through torch, and the same copy
and one full ApproxPosterior.evidence call per proposal kind (box, prior, mixture, gmm) at N = 1152.
The share of the FP64 roof counts, per kernel value k(t, x) at the padded dimension DP, DP subtractions, DP fused
multiply-adds (2 flop), the sum of the paired accumulators, 22 flop of apgp_exp, the amplitude and the accumulating
multiply-add: 3 DP + 26 flop, over 78.6 TFLOP/s.
Usage: python tools/evidence_timing.py [--reps R] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1152x8,4096x8")
    ap.add_argument("--m", type=int, default=2 ** 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evidence_timing needs an MI355X")
    import approxposterior_amd as apx
    from approxposterior_amd import gp as agp, priors as P
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

    M = a.m
    res = {"reps": a.reps, "M": M, "fp64_peak_flops": FP64_PEAK, "shapes": []}
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        rs = np.random.RandomState(0)
        X = rs.uniform(-5, 5, size=(N, D))
        y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
        kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
        gp = agp.GP(kernel=kern, fit_mean=True, mean=float(np.mean(y)), white_noise=np.log(1e-6 * np.var(y)))
        gp.compute(X)
        bounds = [(-5.0, 5.0)] * D
        Td = gp.box_candidates(M, [(-5.2, 5.2)] * D, 7)
        lnq = torch.from_numpy(rs.normal(size=M)).cuda()
        c = X[int(np.argmax(y))]
        lo = torch.tensor([b[0] for b in bounds], dtype=torch.float64, device="cuda")
        hi = torch.tensor([b[1] for b in bounds], dtype=torch.float64, device="cuda")
        cd = torch.from_numpy(c).cuda()

        def one_pass():
            return gp.importance_pass(y, Td, lnq=lnq, bounds=bounds, centre=c)

        def weights_moments(mu, matmul):
            ok = torch.isfinite(Td).all(dim=1) & (Td >= lo).all(dim=1) & (Td <= hi).all(dim=1)
            ok = ok & torch.isfinite(mu) & torch.isfinite(lnq)
            logw = torch.where(ok, mu - lnq, torch.full_like(mu, -np.inf))
            lmax = logw.max()
            e = torch.exp(logw - lmax)
            dx = torch.where(ok[:, None], Td - cd, torch.zeros_like(Td))
            ex = e[:, None] * dx
            S = ex.t() @ dx if matmul else (ex[:, :, None] * dx[:, None, :]).sum(dim=0)
            rec = torch.cat([lmax.reshape(1), e.sum().reshape(1), (e * e).sum().reshape(1),
                             ok.sum().to(torch.float64).reshape(1), ex.sum(dim=0), S.reshape(-1)])
            return rec.cpu().numpy()

        def composition(matmul=False):
            return weights_moments(gp._mean_device(y, Td), matmul)

        # the parts of the composition, and the faster of two ways to form S in torch (a (D, M) x (M, D) product, or a
        # broadcast product summed over the rows): the comparison below uses the faster
        mu0 = gp._mean_device(y, Td)
        parts = {}
        for name, fn in (("predict_mean", lambda: gp._mean_device(y, Td)), ("torch_matmul", lambda: weights_moments(mu0, True)),
                         ("torch_broadcast", lambda: weights_moments(mu0, False))):
            fn()
            parts[name + "_ms"] = float(np.median([timed(fn)[0] for _ in range(a.reps)]))
        use_matmul = parts["torch_matmul_ms"] < parts["torch_broadcast_ms"]
        full_composition = composition
        composition = lambda: full_composition(use_matmul)      # noqa: E731

        for _ in range(2):                                  # warm both routes (code objects, torch's kernels, work buffers)
            rec, comp = one_pass(), composition()
        # the two routes compute the same record (sums in another order)
        agree = {"lmax": abs(rec["lmax"] - comp[0]), "S0_rel": abs(rec["S0"] - comp[1]) / comp[1],
                 "S2_rel": abs(rec["S2"] - comp[2]) / comp[2], "cnt": abs(rec["cnt"] - comp[3]),
                 "s1_abs": float(np.abs(rec["s1"] - comp[4:4 + D]).max()),
                 "S_abs": float(np.abs(rec["S"] - comp[4 + D:].reshape(D, D)).max())}
        tp, tc = [], []
        for _ in range(a.reps):                             # alternating: both see the same box at the same time
            tp.append(timed(one_pass)[0])
            tc.append(timed(composition)[0])
        dp = 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32
        flop = float(M) * ((N + 3) // 4 * 4) * (3 * dp + 26)
        r = {"N": N, "D": D, "pass": stats(tp), "composition": stats(tc), "composition_parts": parts, "agreement": agree,
             "flop_per_pass": flop}
        r["pass_over_composition"] = r["pass"]["median_ms"] / r["composition"]["median_ms"]
        r["pass_fp64_roof_fraction"] = flop / (1e-3 * r["pass"]["median_ms"]) / FP64_PEAK
        r["not_slower_beyond_spread"] = bool(r["pass"]["median_ms"] <= r["composition"]["median_ms"] + r["composition"]["spread_ms"])
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)

        if N == 1152:                                       # one full evidence() call per proposal kind
            joint = P.JointPrior([P.UniformPrior(-5.0, 5.0) if d % 2 == 0 else P.GaussianPrior(0.0, 2.0) for d in range(D)])
            sample = lambda n=1: rs.uniform(-5, 5, size=(n, D))                                   # noqa: E731
            box_prior = lambda t: 0.0 if np.all(np.abs(t) <= 5.0) else -np.inf                     # noqa: E731
            mix = ([0.5, 0.5], np.stack([c, X[int(np.argsort(y)[-2])]]), np.stack([np.eye(D), 2.0 * np.eye(D)]))
            kinds = {"box": (box_prior, "box"), "prior": (joint, "prior"), "mixture": (box_prior, mix)}
            try:
                import sklearn  # noqa: F401
                kinds["gmm"] = (box_prior, "gmm")
            except ImportError:
                pass
            chain = c + rs.normal(size=(20000, D)) * 0.5
            full = {}
            for name, (prior, proposal) in kinds.items():
                post = apx.ApproxPosterior(theta=X, y=y, lnprior=prior, lnlike=lambda t: 0.0, priorSample=sample,
                                           bounds=bounds, gp=gp)
                call = lambda: post.evidence(nSamples=M, proposal=proposal, seed=11,            # noqa: E731
                                             samples=chain if proposal == "gmm" else None)
                call()
                ts, out = zip(*[timed(call) for _ in range(a.reps)])
                full[name] = dict(stats(ts), logZ=float(out[-1]["logZ"]), logZErr=float(out[-1]["logZErr"]),
                                  ess=float(out[-1]["ess"]), nInside=int(out[-1]["nInside"]))
                print(json.dumps({name: full[name]}), flush=True)
            res["evidence_calls"] = {"N": N, "D": D, "nSamples": M, "kinds": full}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
