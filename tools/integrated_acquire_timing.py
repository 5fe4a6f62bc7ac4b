"""The integrated acquisition (DESIGN.md "Integrated acquisition") at M = 2^20 candidates, D = 8, N = 1152 and 4096
training points, J = 64, 256, 1024 reference points, timed with HIP events in one process, after a warm-up of every shape:
  pass    apgp_acquire_integrated alone (contraction, k(t, r_j), log-sum-exp, arg-min), B / a / var resident
  call    GP.acquire_integrated end to end (host clock around a call that ends in a copy of the 16-byte record): the
          UTIL_NONE sweep, k(X, R), the two triangular solves for B, the pass
  sweep   the UTIL_NONE sweep that precedes the pass (GP._sweep, with_var)
  torch   the same u from library pieces: chunks of apgp_kernel_cross (k(t, X) and k(t, R)) + torch.matmul +
          torch.logsumexp, and an arg-min at the end
Every figure is the median of --reps repeats with the min and max beside it.  2 M N J / t of the pass is reported as a
fraction of the 78.6 TFLOP/s FP64 matrix peak.
Usage: python tools/integrated_acquire_timing.py [--reps R] [--out FILE]   (needs an MI355X)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--n", type=int, nargs="+", default=[1152, 4096])
    ap.add_argument("--j", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrated_acquire_timing.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("integrated_acquire_timing needs an MI355X")
    from approxposterior_amd import gp as agp, _lib
    lib = _lib.load()
    M, D = a.m, a.d
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = ev(), ev()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    res = {"M": M, "D": D, "fp64_peak_tflops": FP64_PEAK / 1e12, "shapes": []}
    for N in a.n:
        rs = np.random.RandomState(N)
        X = rs.uniform(-5, 5, size=(N, D))
        y = -np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1) / 100.0
        kern = agp.Product(agp.ConstantKernel(np.log(np.var(y) / D), ndim=D), agp.ExpSquaredKernel(np.full(D, 9.0), ndim=D))
        gp = agp.GP(kernel=kern, fit_mean=True, mean=float(np.mean(y)), white_noise=np.log(1e-6 * np.var(y)))
        gp.compute(X)
        Td = torch.from_numpy(rs.uniform(-5.0, 5.0, size=(M, D))).cuda()
        bounds = [(-5.0, 5.0)] * D
        ks = gp._kernel_struct()
        sweep = lambda: gp._sweep(y, Td, _lib.UTIL_NONE, with_var=True)      # noqa: E731
        var = sweep().var
        torch.cuda.synchronize()
        sweep_ms = timed(sweep, a.reps)
        for J in a.j:
            R = rs.uniform(-5.0, 5.0, size=(J, D))
            w = gp.integration_weights(y, R, "uniform")
            bi, bu, u_dev, _, _ = gp.acquire_integrated(y, Td, R, logWeights=w, bounds=bounds, return_all=True)    # warm-up
            # the pass alone, on resident operands
            R_d, a_d = torch.from_numpy(R).cuda(), torch.from_numpy(w).cuda()
            kxr = torch.empty((N, J), dtype=torch.float64, device="cuda")
            _lib.check(lib.apgp_kernel_cross(gp._x_d.data_ptr(), N, R_d.data_ptr(), J, ctypes.byref(ks), kxr.data_ptr(), J,
                                             None), "apgp_kernel_cross")
            L = torch.tril(gp._L[:N, :N])
            B = torch.linalg.solve_triangular(L.t(), torch.linalg.solve_triangular(L, kxr, upper=False), upper=True).contiguous()
            part = torch.empty(max(int(lib.apgp_integrated_work_len(M, J)), 2), dtype=torch.float64, device="cuda")
            best = torch.empty(2, dtype=torch.float64, device="cuda")
            arr = ctypes.c_double * _lib.MAX_DIM
            lo, hi = arr(*[b[0] for b in bounds]), arr(*[b[1] for b in bounds])

            def the_pass():
                _lib.check(lib.apgp_acquire_integrated(Td.data_ptr(), M, 0, gp._xs.data_ptr(), N, ctypes.byref(ks),
                                                       R_d.data_ptr(), J, B.data_ptr(), a_d.data_ptr(), var.data_ptr(), lo, hi,
                                                       None, None, 0, None, part.data_ptr(), best.data_ptr(), None),
                           "apgp_acquire_integrated")

            the_pass()
            torch.cuda.synchronize()
            pass_ms = timed(the_pass, a.reps)
            call_ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                gp.acquire_integrated(y, Td, R, logWeights=w, bounds=bounds)
                call_ms.append(1e3 * (time.perf_counter() - t0))
            # the torch composition of the same quantity
            s_d = var + ks.diag_add
            u_t = torch.empty(M, dtype=torch.float64, device="cuda")
            ktx = torch.empty((a.chunk, N), dtype=torch.float64, device="cuda")
            ktr = torch.empty((a.chunk, J), dtype=torch.float64, device="cuda")

            def composition():
                for c0 in range(0, M, a.chunk):
                    mc = min(a.chunk, M - c0)
                    Tc = Td[c0:c0 + mc]
                    _lib.check(lib.apgp_kernel_cross(Tc.data_ptr(), mc, gp._x_d.data_ptr(), N, ctypes.byref(ks),
                                                     ktx.data_ptr(), N, None), "apgp_kernel_cross")
                    _lib.check(lib.apgp_kernel_cross(Tc.data_ptr(), mc, R_d.data_ptr(), J, ctypes.byref(ks),
                                                     ktr.data_ptr(), J, None), "apgp_kernel_cross")
                    c = ktr[:mc] - torch.matmul(ktx[:mc], B)
                    u_t[c0:c0 + mc] = -torch.logsumexp(a_d.unsqueeze(0) + c * c / s_d[c0:c0 + mc].unsqueeze(1), dim=1)
                return torch.argmin(u_t)

            bt = int(composition().item())
            torch_ms = timed(composition, a.reps)
            agree = float(np.nanmax(np.abs(u_t.cpu().numpy() - u_dev)[np.isfinite(u_dev)]))
            flops = 2.0 * M * N * J
            med = float(np.median(pass_ms))
            row = {"N": N, "J": J, "pass": stats(pass_ms), "call": stats(call_ms), "sweep": stats(sweep_ms),
                   "torch": stats(torch_ms), "pass_tflops": flops / (med * 1e-3) / 1e12,
                   "pass_fraction_of_fp64_peak": flops / (med * 1e-3) / FP64_PEAK,
                   "pass_over_torch": med / float(np.median(torch_ms)), "pass_over_sweep": med / float(np.median(sweep_ms)),
                   "same_pick_as_torch": bool(bt == bi), "max_abs_u_difference": agree}
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
            del ktx, ktr, u_t, B, kxr
        del gp, Td
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
