"""Evidence over posterior function draws (DESIGN.md "Evidence over path draws") at D = 8, M = 2^20, R = 2048, N = 1152
and 4096, S = 8, 16 and 32: three things on the same box, timed with HIP events in one process after a warm-up,
alternating, --reps times each (median, minimum, maximum):
  pass         one GP.importance_paths (apgp_path_importance: the contraction with the weights epilogue, the draws'
               maxima, the moments per draw, the reduction; the S records' copy to the host)
  composition  what the parent commit needs: apgp_path_draws writing the S x M matrix F, then per draw the gate, the
               maximum, the weights and the moments through torch -- the moments as broadcast products, as
               tools/evidence_timing.py's comparator forms them -- and the same copy
  floor        apgp_path_draws without F: the shared contraction with its arg-min epilogue and nothing else
Before timing the records of the first two are compared (relative differences, reported as "agreement").
The share of the FP64 vector roof counts, at the padded dimension DP and S draws, per random feature 2 DP flop of
phase, 27 of the cosine (range reduction 3, h^2 1, eleven fused multiply-adds 22, the product 1) and 2 S of
contraction; per kernel value 3 DP + 24 flop as tools/evidence_timing.py counts them (without its accumulating
multiply-add) and 2 S of contraction; rows and features padded to the 64-row tiles; over 78.6 TFLOP/s.  (Above 8 draws
the 2 S contraction flop run on the matrix cores: the share is still stated against the vector roof.)
Usage: python tools/path_importance_timing.py [--reps R] [--out FILE]   (needs an MI355X)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12


def flop_count(M, N, R, S, D):
    dp = 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32
    pad = lambda v: (v + 63) // 64 * 64      # noqa: E731
    return float(M) * (pad(R) * (2 * dp + 27 + 2 * S) + pad(N) * (3 * dp + 24 + 2 * S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1152,4096")
    ap.add_argument("--draws", default="8,16,32")
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--m", type=int, default=2 ** 20)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_importance_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("path_importance_timing needs an MI355X")
    from approxposterior_amd import gp as agp
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

    M, D, R = a.m, a.dim, a.features
    res = {"reps": a.reps, "M": M, "D": D, "R": R, "fp64_peak_flops": FP64_PEAK, "shapes": []}
    for N in (int(v) for v in a.ns.split(",")):
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
        for S in (int(v) for v in a.draws.split(",")):
            np.random.seed(100 + S)
            paths = gp.sample_paths(y, S, R)

            def one_pass():
                return gp.importance_paths(y, Td, paths, lnq=lnq, bounds=bounds, centre=c)

            def composition():
                F, _, _ = gp._path_call(Td, paths.ks, paths.mean, paths, paths.V, with_f=True)
                ok = torch.isfinite(Td).all(dim=1) & (Td >= lo).all(dim=1) & (Td <= hi).all(dim=1) & torch.isfinite(lnq)
                dx = torch.where(ok[:, None], Td - cd, torch.zeros_like(Td))
                recs = []
                for s in range(S):
                    oks = ok & torch.isfinite(F[s])
                    logw = torch.where(oks, F[s] - lnq, torch.full_like(lnq, -np.inf))
                    lmax = logw.max()
                    e = torch.exp(logw - lmax)
                    ex = e[:, None] * dx
                    Sm = (ex[:, :, None] * dx[:, None, :]).sum(dim=0)
                    recs.append(torch.cat([lmax.reshape(1), e.sum().reshape(1), (e * e).sum().reshape(1),
                                           oks.sum().to(torch.float64).reshape(1), ex.sum(dim=0), Sm.reshape(-1)]))
                return torch.stack(recs).cpu().numpy()

            def floor():
                return gp._path_call(Td, paths.ks, paths.mean, paths, paths.V, with_f=False)

            for _ in range(2):                              # warm every route (code objects, torch's kernels, work buffers)
                recs, comp, _ = one_pass(), composition(), floor()
            rel = lambda x, y_: float(np.max(np.abs(np.asarray(x) - y_) / np.maximum(np.abs(y_), 1e-300)))     # noqa: E731
            agree = {"lmax_abs": max(abs(r["lmax"] - comp[s, 0]) for s, r in enumerate(recs)),
                     "S0_rel": max(rel(r["S0"], comp[s, 1]) for s, r in enumerate(recs)),
                     "S2_rel": max(rel(r["S2"], comp[s, 2]) for s, r in enumerate(recs)),
                     "cnt_abs": max(abs(r["cnt"] - comp[s, 3]) for s, r in enumerate(recs)),
                     "s1_rel_to_largest": max(float(np.abs(r["s1"] - comp[s, 4:4 + D]).max() / np.abs(comp[s, 4:4 + D]).max())
                                              for s, r in enumerate(recs)),
                     "S_rel_to_largest": max(float(np.abs(r["S"] - comp[s, 4 + D:].reshape(D, D)).max()
                                                   / np.abs(comp[s, 4 + D:]).max()) for s, r in enumerate(recs))}
            agree["within_1e-12"] = bool(agree["lmax_abs"] == 0.0 and agree["cnt_abs"] == 0.0 and
                                         max(agree["S0_rel"], agree["S2_rel"], agree["s1_rel_to_largest"],
                                             agree["S_rel_to_largest"]) <= 1e-12)
            tp, tc, tf = [], [], []
            for _ in range(a.reps):                         # alternating: all three see the same box at the same time
                tp.append(timed(one_pass)[0])
                tc.append(timed(composition)[0])
                tf.append(timed(floor)[0])
            flop = flop_count(M, N, R, S, D)
            r = {"N": N, "S": S, "pass": stats(tp), "composition": stats(tc), "floor": stats(tf), "agreement": agree,
                 "flop_per_pass": flop, "ess_of_the_draws_min": float(min(q["S0"] ** 2 / q["S2"] for q in recs))}
            r["pass_over_composition"] = r["pass"]["median_ms"] / r["composition"]["median_ms"]
            r["pass_over_floor"] = r["pass"]["median_ms"] / r["floor"]["median_ms"]
            r["pass_fp64_roof_fraction"] = flop / (1e-3 * r["pass"]["median_ms"]) / FP64_PEAK
            r["not_slower_beyond_spreads"] = bool(r["pass"]["median_ms"] <= r["composition"]["median_ms"]
                                                  + r["composition"]["spread_ms"] + r["pass"]["spread_ms"])
            print(json.dumps(r), flush=True)
            res["shapes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
