// Gaussian-mixture passes over a sample matrix (gmmUtils.fitGMM): one E-step + sufficient statistics, a scoring pass, or
// one k-means assignment, each as ONE pass over X (every row read once) and a fixed-order reduction of the per-workgroup
// partials.  No floating-point atomics: the same input gives the same bits on every run.
//
// Layout (DESIGN.md "GMM fit"):
//   * params (device, user layout, apgp_gmm_params_len doubles): per component k, Q = 2 + D + D(D+1)/2 doubles
//       [log w_k, log det U_k, c_k (D), U_k packed upper triangle column by column (U[i][j] at j(j+1)/2 + i, i <= j)]
//     U_k is the precision Cholesky factor (precision = U U^T, sklearn's precisions_cholesky_), c_k the centre the
//     statistics are taken about (the current mean).  The column-major packing makes the first D columns of the
//     DP-padded copy in LDS sit at the same offsets: padding is zeros appended.
//   * stats (apgp_gmm_stats_len doubles): [G, then per component (s0, s1 (D), S (D(D+1)/2, packed as U))]
//       EM:     G = sum log_prob_norm, s0 = sum r, s1 = sum r (x - c), S = sum r (x - c)(x - c)^T
//       score:  G only (nothing else is written)
//       kmeans: G = inertia (sum of squared distances to the nearest centre), r = the one-hot nearest-centre label
//   * row_lp / row_label (optional): per row log_prob_norm (kmeans: squared distance) and the arg-max (kmeans: arg-min)
//     component, lowest index on ties.
// Per tile of TILE rows a workgroup stages the rows in LDS (one extra slot per row holds 1.0, so that s0, s1 and S are
// all sum_rows w * a * b for two slots a, b of the row), computes one row per thread, then each thread owns a set of
// outputs and sums them over the tile's rows; the per-thread totals run over the workgroup's tiles in order.
#include "apgp_common.h"
#include "gmm_logpdf.h"
#include "scratch.h"
#include <mutex>

#define GMM_MAX_K 16
#define GMM_NB_MAX 512                 // workgroups of a pass (fixed: the reduction order depends on it only)
#define GMM_SCRATCH_SLOT 5

namespace {

#define GMM_NT 256                     // threads of a pass workgroup
constexpr int gmm_tile(int DP) { return DP >= 32 ? 128 : 256; }     // rows per tile (LDS: <= 123 KB at D = 32, K = 16)
constexpr int gmm_tri(int d) { return d * (d + 1) / 2; }
// dynamic LDS of a pass: parameters (K x padded record) + tile (TILE x (DP + 1)) + responsibilities ((K + 1) x TILE)
constexpr size_t gmm_lds_bytes(int DP, int K) {
    return sizeof(double) * ((size_t)K * (2 + DP + gmm_tri(DP)) + (size_t)gmm_tile(DP) * (DP + 1) + (size_t)(K + 1) * gmm_tile(DP));
}

struct GmmArgs {
    const double* X;
    const double* params;
    double* partial;                   // [nout][nb]
    double* row_lp;
    int32_t* row_label;
    long long n;
    long long ntiles;
    int D;
    int K;
    int nout;
};

template <int DP, int MODE>
__global__ __launch_bounds__(GMM_NT) void gmm_pass_kernel(GmmArgs a) {
    constexpr int TILE = gmm_tile(DP);
    constexpr int QP = 2 + DP + gmm_tri(DP);          // per-component params in LDS (padded)
    constexpr int XS = DP + 1;                        // LDS row stride: DP coordinates + the constant 1
    constexpr int NO = MODE == APGP_GMM_SCORE ? 1 : (1 + GMM_MAX_K * (1 + DP + gmm_tri(DP)) + GMM_NT - 1) / GMM_NT;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int K = a.K, D = a.D, tid = threadIdx.x;
    const int Q = 2 + D + gmm_tri(D);
    const int QS = 1 + D + gmm_tri(D);                // per-component statistics
    double* sp = lds;
    double* xt = sp + K * QP;
    double* rt = xt + TILE * XS;                      // [K + 1][TILE]: r (or one-hot) per component, then the row's G term

    for (int e = tid; e < K * QP; e += GMM_NT) {
        const int k = e / QP, q = e - k * QP;
        double v = 0.0;
        if (q < 2 + D) v = a.params[(long long)k * Q + q];
        else if (q >= 2 + DP && q - 2 - DP < gmm_tri(D)) v = a.params[(long long)k * Q + 2 + D + (q - 2 - DP)];
        sp[e] = v;
    }
    for (int e = tid; e < TILE * XS; e += GMM_NT) xt[e] = (e % XS == DP) ? 1.0 : 0.0;

    double acc[NO];
#pragma unroll
    for (int m = 0; m < NO; ++m) acc[m] = 0.0;

    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const long long r0 = t * TILE;
        const int rows = (int)(a.n - r0 < TILE ? a.n - r0 : TILE);
        __syncthreads();                              // the previous tile's statistics are read
        const double* src = a.X + r0 * D;
        for (int e = tid; e < rows * D; e += GMM_NT) {
            const int r = e / D;
            xt[r * XS + (e - r * D)] = src[e];
        }
        __syncthreads();

        if (tid < rows) {
            const double* x = xt + tid * XS;
            double g;
            int lab = 0;
            if (MODE == APGP_GMM_KMEANS) {
                double best = INFINITY;
                for (int k = 0; k < K; ++k) {
                    const double* c = sp + k * QP + 2;
                    double d2 = 0.0;
#pragma unroll
                    for (int i = 0; i < DP; ++i) {
                        const double z = x[i] - c[i];
                        d2 = fma(z, z, d2);
                    }
                    if (d2 < best) { best = d2; lab = k; }
                }
                for (int k = 0; k < K; ++k) rt[k * TILE + tid] = k == lab ? 1.0 : 0.0;
                g = best;
            } else {
                double mx = -INFINITY;
                for (int k = 0; k < K; ++k) {
                    const double lp = gmm_logpdf<DP>(x, sp + k * QP, D);
                    rt[k * TILE + tid] = lp;
                    if (lp > mx) { mx = lp; lab = k; }
                }
                double s = 0.0;
                for (int k = 0; k < K; ++k) s += exp(rt[k * TILE + tid] - mx);
                g = mx + log(s);
                if (MODE == APGP_GMM_EM)
                    for (int k = 0; k < K; ++k) rt[k * TILE + tid] = exp(rt[k * TILE + tid] - g);
            }
            rt[K * TILE + tid] = g;
            if (a.row_lp) a.row_lp[r0 + tid] = g;
            if (a.row_label) a.row_label[r0 + tid] = lab;
        }
        __syncthreads();

#pragma unroll
        for (int m = 0; m < NO; ++m) {
            const int o = m * GMM_NT + tid;
            if (o < a.nout) {
                int kc = K, ia = DP, ib = DP;
                double ca = 0.0, cb = 0.0;
                if (o > 0) {
                    const int k = (o - 1) / QS, q = (o - 1) - k * QS;
                    const double* c = sp + k * QP + 2;
                    kc = k;
                    if (q >= 1 && q <= D) {
                        ia = q - 1; ca = c[ia];
                    } else if (q > D) {
                        const int tt = q - 1 - D;
                        int j = 0;
                        while ((j + 1) * (j + 2) / 2 <= tt) ++j;
                        ia = tt - j * (j + 1) / 2; ib = j; ca = c[ia]; cb = c[ib];
                    }
                }
                const double* w = rt + kc * TILE;
                double s = 0.0;
                for (int r = 0; r < rows; ++r) s = fma(w[r] * (xt[r * XS + ia] - ca), xt[r * XS + ib] - cb, s);
                acc[m] += s;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < NO; ++m) {
        const int o = m * GMM_NT + tid;
        if (o < a.nout) a.partial[(long long)o * gridDim.x + blockIdx.x] = acc[m];
    }
}

// out[o] = sum_b partial[o][b], one workgroup per output, a fixed tree
__global__ __launch_bounds__(256) void gmm_reduce_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    __shared__ double red[256];
    const int o = blockIdx.x, tid = threadIdx.x;
    const double* p = partial + (long long)o * nb;
    double s = 0.0;
    for (int b = tid; b < nb; b += 256) s += p[b];
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[o] = red[0];
}

template <int DP, int MODE>
int gmm_launch(const GmmArgs& a, int nb, size_t lds, hipStream_t s) {
    // the limit is declared once per device and instantiation, so it is the instantiation's largest need (K = 16),
    // not this call's: a later call with more components must not launch above what was declared
    constexpr size_t lds_max = gmm_lds_bytes(DP, GMM_MAX_K);
    static ApgpLdsOnce once;
    if (lds_max > 65536) {
        const int dev = apgp_stream_device(s);
        if (dev < 0 || dev >= 64) {
            apgp_set_error("apgp_gmm_pass: no device for the stream");
            return -2;
        }
        if (apgp_raise_lds(once, "apgp_gmm_pass", dev, (int)lds_max, {(const void*)gmm_pass_kernel<DP, MODE>}) != 0) return -2;
    }
    hipLaunchKernelGGL((gmm_pass_kernel<DP, MODE>), dim3((unsigned)nb), dim3(GMM_NT), lds, s, a);
    return 0;
}

template <int DP>
int gmm_launch_mode(const GmmArgs& a, int mode, int nb, size_t lds, hipStream_t s) {
    switch (mode) {
        case APGP_GMM_EM: return gmm_launch<DP, APGP_GMM_EM>(a, nb, lds, s);
        case APGP_GMM_SCORE: return gmm_launch<DP, APGP_GMM_SCORE>(a, nb, lds, s);
        default: return gmm_launch<DP, APGP_GMM_KMEANS>(a, nb, lds, s);
    }
}

}  // namespace

extern "C" int64_t apgp_gmm_params_len(int32_t ndim, int32_t ncomp) {
    if (ndim < 1 || ndim > APGP_MAX_DIM || ncomp < 1 || ncomp > GMM_MAX_K) return -1;
    return (int64_t)ncomp * (2 + ndim + gmm_tri(ndim));
}

extern "C" int64_t apgp_gmm_stats_len(int32_t ndim, int32_t ncomp) {
    if (ndim < 1 || ndim > APGP_MAX_DIM || ncomp < 1 || ncomp > GMM_MAX_K) return -1;
    return 1 + (int64_t)ncomp * (1 + ndim + gmm_tri(ndim));
}

extern "C" int apgp_gmm_pass(const double* X, int64_t n, int32_t ndim, int32_t ncomp, const double* params, int32_t mode,
                             double* stats_out, double* row_lp, int32_t* row_label, void* stream) {
    APGP_CHECK_ARG(X && params && stats_out, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n < (1ll << 31), "1 <= n < 2^31 required");
    APGP_CHECK_ARG(ndim >= 1 && ndim <= APGP_MAX_DIM, "1 <= ndim <= APGP_MAX_DIM required");
    APGP_CHECK_ARG(ncomp >= 1 && ncomp <= GMM_MAX_K, "1 <= ncomp <= 16 required");
    APGP_CHECK_ARG(mode == APGP_GMM_EM || mode == APGP_GMM_SCORE || mode == APGP_GMM_KMEANS, "unknown mode");
    hipStream_t s = (hipStream_t)stream;
    const int DP = apgp_dpad(ndim);
    const int tile = gmm_tile(DP);
    GmmArgs a;
    a.X = X; a.params = params; a.row_lp = row_lp; a.row_label = row_label;
    a.n = n; a.ntiles = (n + tile - 1) / tile; a.D = ndim; a.K = ncomp;
    a.nout = mode == APGP_GMM_SCORE ? 1 : (int)apgp_gmm_stats_len(ndim, ncomp);
    const int nb = (int)(a.ntiles < GMM_NB_MAX ? a.ntiles : GMM_NB_MAX);
    const size_t lds = gmm_lds_bytes(DP, ncomp);

    std::lock_guard<std::mutex> lock(apgp_stream_lock(s));
    a.partial = apgp_stream_scratch(GMM_SCRATCH_SLOT, s, (size_t)nb * a.nout);
    if (!a.partial) {
        apgp_set_error("apgp_gmm_pass: scratch allocation failed");
        return -2;
    }
    const int rc = apgp_by_dpad(DP, [&](auto dp) { return gmm_launch_mode<decltype(dp)::value>(a, mode, nb, lds, s); });
    if (rc) return rc;
    APGP_CHECK_LAUNCH();
    hipLaunchKernelGGL(gmm_reduce_kernel, dim3((unsigned)a.nout), dim3(256), 0, s, (const double*)a.partial, nb, stats_out);
    APGP_CHECK_LAUNCH();
    return 0;
}
