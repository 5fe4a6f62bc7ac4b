"""mcmc.integrated_time on the host (per-series FFTs on host threads) against the device path (direct lag sums,
csrc/autocorr.hip) at 2e4 x 64 x 8 (BASELINE config 5's chain) and 2e4 x 20 x 2, for AR(1) chains whose window is about
100, about 1000 and beyond the lag cap; the time of one 256-lag block of apgp_autocorr_block at several starting lags;
and the cap crossing: the number of lags at which the direct sum (one call, result back on the host) stops beating the
host estimator.  Medians of repeated timed calls after a warm-up.  Writes one JSON document.

    timeout -k 10 600 python tools/autocorr_timing.py --out profiles/autocorr_timing.json [--reps 5]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ar1(n_t, n_w, n_d, rho, seed=0):
    from scipy.signal import lfilter
    e = np.random.RandomState(seed).randn(n_t, n_w, n_d)
    e[1:] *= np.sqrt(1.0 - rho * rho)
    return np.ascontiguousarray(lfilter([1.0], [1.0, -rho], e, axis=0) * (1.0 + np.arange(n_d)) + 3.0 * np.arange(n_d))


def median_time(fn, reps, sync):
    fn()
    sync()
    runs = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        runs.append(time.perf_counter() - t0)
    return float(np.median(runs)), [round(r, 6) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autocorr_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("autocorr_timing needs the GPU")
    from approxposterior_amd import _lib, mcmc
    lib = _lib.load()
    sync = torch.cuda.synchronize
    rows, blocks, crossing = [], [], []
    for n_t, n_w, n_d in ((20000, 64, 8), (20000, 20, 2)):
        for label, rho in (("window~100", 0.905), ("window~1000", 0.99), ("beyond the cap", 0.9995)):
            x = ar1(n_t, n_w, n_d, rho)
            xd = torch.from_numpy(x).cuda()
            host_s, host_runs = median_time(lambda: mcmc.integrated_time(x, tol=0), args.reps, sync)
            before = mcmc.autocorr_fallbacks
            dev_s, dev_runs = median_time(lambda: mcmc.integrated_time(x, tol=0, onDevice=True), args.reps, sync)
            ten_s, ten_runs = median_time(lambda: mcmc.integrated_time(xd, tol=0), args.reps, sync)
            fallbacks = (mcmc.autocorr_fallbacks - before) // (2 * (args.reps + 1))
            tau_h, tau_d = mcmc.integrated_time(x, tol=0), mcmc.integrated_time(xd, tol=0)
            asked = []
            acf = mcmc._DeviceAcf(xd)
            mcmc._windows_from_blocks(lambda a, b: (asked.append((a, b)), acf(a, b))[1], n_t, n_d, 5, mcmc.AUTOCORR_BLOCK,
                                      mcmc.AUTOCORR_LAG_CAP)
            rows.append(dict(shape=[n_t, n_w, n_d], chain=label, rho=rho, tau_max=round(float(np.nanmax(tau_h)), 2),
                             lags_computed=int(sum(b for _, b in asked)), fell_back_to_host=bool(fallbacks),
                             host_s=round(host_s, 5), host_runs_s=host_runs,
                             device_numpy_input_s=round(dev_s, 5), device_numpy_input_runs_s=dev_runs,
                             device_tensor_input_s=round(ten_s, 5), device_tensor_input_runs_s=ten_runs,
                             max_rel_dtau=float(np.nanmax(np.abs(tau_d - tau_h) / np.abs(tau_h)))))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        # one 256-lag block of the C entry (kernels only: no copy back), and the cost of the first call's statistics
        work = torch.empty(int(lib.apgp_autocorr_work_len(n_t, n_w, n_d)), dtype=torch.float64, device="cuda")
        f = torch.empty((n_d, 256), dtype=torch.float64, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def block(lag0, reuse, nl=256, out=f):
            _lib.check(lib.apgp_autocorr_block(xd.data_ptr(), n_t, n_w, n_d, 0, 1, lag0, nl, reuse, work.data_ptr(),
                                               out.data_ptr(), st), "apgp_autocorr_block")
        for lag0, reuse in ((0, 0), (0, 1), (1024, 1), (8192, 1), (16384, 1)):
            t, _ = median_time(lambda: block(lag0, reuse), 4 * args.reps, sync)
            fma = sum(max(n_t - l, 0) for l in range(lag0, lag0 + 256)) * n_w * n_d
            blocks.append(dict(shape=[n_t, n_w, n_d], lag0=lag0, nlags=256, with_statistics=not reuse, ms=round(t * 1e3, 4),
                               gflops=round(2.0 * fma / t * 1e-9, 1)))
            print(json.dumps(blocks[-1]), file=sys.stderr, flush=True)
        # the crossing: all lags 0 .. L-1 in one call and back on the host, against the host estimator's whole call
        host_s = float(np.median([r["host_s"] for r in rows if r["shape"] == [n_t, n_w, n_d]]))
        ladder, cross = [], None
        L = 256
        while True:
            L = min(L, n_t)
            big = torch.empty((n_d, L), dtype=torch.float64, device="cuda")
            t, _ = median_time(lambda: (block(0, 0, L, big), big.cpu()), max(3, args.reps), sync)
            ladder.append(dict(lags=L, device_s=round(t, 5)))
            if cross is None and t > host_s:
                cross = L
            if L == n_t:
                break
            L *= 2
        crossing.append(dict(shape=[n_t, n_w, n_d], host_s=round(host_s, 5), ladder=ladder, first_lags_slower_than_host=cross))
        print(json.dumps(crossing[-1]), file=sys.stderr, flush=True)
    doc = dict(tool="autocorr_timing", reps=args.reps, host_threads=os.environ.get("OMP_NUM_THREADS"),
               block=mcmc.AUTOCORR_BLOCK, lag_cap=mcmc.AUTOCORR_LAG_CAP, estimator=rows, lag_blocks=blocks, cap_crossing=crossing)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
