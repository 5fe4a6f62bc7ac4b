"""fitGMM on the device against the reference-style host fit (sklearn's GaussianMixture: n = 1..maxComp, lowest
BIC, refit), two-cluster data in D = 8, maxComp = 3, at n = 2e4, 2e5, 1.28e6 rows.  Also the time of one EM pass
(pass + reduction + statistics back on the host) and one score pass at K = 3, and one EM / score pass at wider shapes
(D up to 32, K up to 16).  Prints one JSON line.

    python tools/gmm_timing.py [--no-host] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def two_clusters(n, D=8, seed=0):
    rs = np.random.RandomState(seed)
    lab = rs.rand(n) < 0.4
    X = rs.normal(size=(n, D))
    X[lab] = X[lab] * 0.5 + 4.0
    return X + 100.0


def host_fit(X, maxComp=3):
    """the reference's fitGMM procedure (approxposterior/gmmUtils.py) on the host"""
    from sklearn.mixture import GaussianMixture
    best, bestN = np.inf, None
    gmm = GaussianMixture()
    for k in range(1, maxComp + 1):
        gmm.set_params(n_components=k, covariance_type="full")
        gmm.fit(X)
        b = gmm.bic(X)
        if b < best:
            best, bestN = b, k
    return GaussianMixture(n_components=bestN, covariance_type="full").fit(X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gmm_timing needs the GPU")
    from approxposterior_amd import _lib, gmmUtils
    rows = []
    gmmUtils.fitGMM(two_clusters(5000), maxComp=3)                 # load the code objects
    for n in (20000, 200000, 1280000):
        X = two_clusters(n)
        runs = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = gmmUtils.fitGMM(X, maxComp=3)
            runs.append(time.perf_counter() - t0)
        Xd = torch.from_numpy(X).cuda()
        gt = time.perf_counter()
        gmmUtils.fitGMM(Xd, maxComp=3)
        t_tensor = time.perf_counter() - gt
        dev = gmmUtils._Device(Xd)
        K = 3
        params = dev.pack(np.full(K, 1.0 / K), X[:K], np.broadcast_to(np.eye(8), (K, 8, 8)))
        per = {}
        for name, mode in (("em", _lib.GMM_EM), ("score", _lib.GMM_SCORE), ("kmeans", _lib.GMM_KMEANS)):
            dev.run(Xd, params, mode, K)
            t0 = time.perf_counter()
            for _ in range(50):
                dev.run(Xd, params, mode, K)
            per[name] = (time.perf_counter() - t0) / 50 * 1e3
        row = dict(n=n, device_fit_s=min(runs), device_fit_runs_s=[round(r, 4) for r in runs],
                   device_fit_tensor_input_s=round(t_tensor, 4), device_n_components=int(g.n_components),
                   device_n_iter=int(g.n_iter_), em_pass_ms=round(per["em"], 4), score_pass_ms=round(per["score"], 4),
                   kmeans_pass_ms=round(per["kmeans"], 4), pass_bytes=int(X.nbytes))
        if not args.no_host:
            t0 = time.perf_counter()
            h = host_fit(X)
            row.update(host_fit_s=round(time.perf_counter() - t0, 3), host_n_components=int(h.n_components))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    # one pass at wide shapes (the outer-product statistics at their largest), 1.28e6 rows
    wide = []
    for D, K in ((8, 16), (16, 3), (16, 16), (32, 3), (32, 16)):
        rs = np.random.RandomState(D + K)
        Xd = torch.from_numpy(rs.normal(size=(1280000, D))).cuda()
        dev = gmmUtils._Device(Xd)
        params = dev.pack(np.full(K, 1.0 / K), rs.normal(size=(K, D)), np.broadcast_to(np.eye(D), (K, D, D)))
        per = {}
        for name, mode in (("em", _lib.GMM_EM), ("score", _lib.GMM_SCORE)):
            dev.run(Xd, params, mode, K)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                dev.run(Xd, params, mode, K)
            per[name] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
        # multiply-adds of the statistics (outer products) and of the E-step, per pass
        stat_fma = 1280000 * (1 + K * (1 + D + D * (D + 1) // 2))
        estep_fma = 1280000 * K * (D * (D + 1) // 2 + D)
        wide.append(dict(D=D, K=K, n=1280000, em_pass_ms=per["em"], score_pass_ms=per["score"],
                         em_stat_gflops=round(2 * stat_fma / per["em"] * 1e-6, 1),
                         em_total_gflops=round(2 * (stat_fma + estep_fma) / per["em"] * 1e-6, 1)))
        print(json.dumps(wide[-1]), file=sys.stderr, flush=True)
        del Xd, dev
    print(json.dumps(dict(tool="gmm_timing", D=8, maxComp=3, covType="full", host_threads=os.environ.get("OMP_NUM_THREADS"),
                          rows=rows, wide_passes=wide)))


if __name__ == "__main__":
    main()
