// Walker-averaged normalised autocorrelation function of an ensemble chain (mcmc.integrated_time(onDevice=True)): the lag
// products are summed DIRECTLY over a block of lags -- no FFT, no spectrum buffer.  Sokal's window stops after about five
// autocorrelation times, so the lags that are needed are a small part of the n_t lags a padded transform computes.
//
//   f[d][l - lag0] = (1 / n_w) * sum_k A_kd(l) / A_kd(0),   A_kd(l) = sum_{t < n_t - l} (x[t,k,d] - m_kd) (x[t+l,k,d] - m_kd)
//
// Layout (DESIGN.md "Chain diagnostics").  x is (n_t, n_w, n_d) row-major: the S = n_w * n_d series are contiguous
// within a step, so a LANE owns a series and a wave-instruction reads 64 neighbouring series of one step (coalesced).
// Time is cut into tiles of AC_TC steps and the tiles into at most AC_MAX_CHUNKS chunks of consecutive tiles; the cut
// depends on n_t only.  A workgroup of the lag kernel owns (64 series, one chunk, AC_LW lags): per tile it stages the
// centred values x - m of the AC_TC steps (rows "A") and of the AC_TC + AC_LW steps the lags reach (rows "W", zeros
// past the chain's end, which makes every sum stop at t + l < n_t) in LDS, and each of its 8 waves takes AC_JL lags:
// AC_JL accumulators and a ring of AC_JL W values stay in registers, so one step costs 2 LDS reads for AC_JL FMAs.
// The per-chunk sums go to a partials buffer; a reduce pass adds the chunks in order, divides by A(0) and adds the
// walkers in order.  No floating-point atomics: the same input gives the same bits, whatever the lag blocks asked for.
// m = x[0] + mean(x - x[0]) (a series that never moved has m = x[0] exactly, hence A(0) = 0 and f = 0/0 = NaN for its
// dimension, as the host estimator gives); A(0) is lag 0 of the lag kernel itself, so f(0) = 1 exactly.
#include "apgp_common.h"
#include "scratch.h"
#include <mutex>

#define AC_TC 64                        // steps per tile
#define AC_JL 16                        // lags per wave: accumulators and ring kept in registers
#define AC_WAVES 8
#define AC_LW (AC_JL * AC_WAVES)        // lags per workgroup (128)
#define AC_NT (64 * AC_WAVES)           // threads of a lag workgroup
#define AC_ROWS (2 * AC_TC + AC_LW)     // LDS rows of 64 doubles: A (AC_TC) + W (AC_TC + AC_LW) = 128 KiB
#define AC_LB 256                       // lags per internal pass (what the partials buffer holds)
#define AC_MAX_CHUNKS 32                // time chunks of the lag kernel
#define AC_MEAN_CHUNKS 256              // time chunks of the mean pass (<= AC_LB: its partials fit the same buffer)
#define AC_MAX_T (1ll << 31)            // n_t, lag0, nlags, row0, row_stride below this
#define AC_MAX_ELEMS (1ll << 60)        // (last row + 1) * n_w * n_d below this

namespace {

struct AcShape {
    long long n_t, S, row0, stride;
    int tiles_per_chunk, nch;           // lag kernel: chunk = tiles_per_chunk tiles of AC_TC steps
    long long mean_chunk;               // mean pass: steps per chunk
    int nchm;
};

AcShape ac_shape(long long n_t, long long S, long long row0, long long stride) {
    AcShape sh;
    sh.n_t = n_t; sh.S = S; sh.row0 = row0; sh.stride = stride;
    const long long ntiles = (n_t + AC_TC - 1) / AC_TC;
    sh.tiles_per_chunk = (int)((ntiles + AC_MAX_CHUNKS - 1) / AC_MAX_CHUNKS);
    sh.nch = (int)((ntiles + sh.tiles_per_chunk - 1) / sh.tiles_per_chunk);
    sh.mean_chunk = (n_t + AC_MEAN_CHUNKS - 1) / AC_MEAN_CHUNKS;
    if (sh.mean_chunk < 16) sh.mean_chunk = 16;
    sh.nchm = (int)((n_t + sh.mean_chunk - 1) / sh.mean_chunk);
    return sh;
}

__device__ __forceinline__ const double* ac_row(const double* x, const AcShape& sh, long long t) {
    return x + (sh.row0 + t * sh.stride) * sh.S;
}

// part[c][s] = sum over the chunk's steps of x[t][s] - x[0][s], in step order
__global__ __launch_bounds__(64) void autocorr_mean_partial_kernel(const double* x, AcShape sh, double* part) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= sh.S) return;
    const long long t0 = (long long)blockIdx.y * sh.mean_chunk;
    const long long t1 = t0 + sh.mean_chunk < sh.n_t ? t0 + sh.mean_chunk : sh.n_t;
    const double x0 = ac_row(x, sh, 0)[s];
    double sum = 0.0;
    for (long long t = t0; t < t1; ++t) sum += ac_row(x, sh, t)[s] - x0;
    part[(long long)blockIdx.y * sh.S + s] = sum;
}

__global__ __launch_bounds__(64) void autocorr_mean_reduce_kernel(const double* x, AcShape sh, const double* part, double* mean) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= sh.S) return;
    double sum = 0.0;
    for (int c = 0; c < sh.nchm; ++c) sum += part[(long long)c * sh.S + s];
    mean[s] = ac_row(x, sh, 0)[s] + sum / (double)sh.n_t;
}

// partial[c][j][s] = sum over chunk c's steps t of xc[t][s] * xc[t + lagbase + j][s], j < AC_LW * gridDim.z
__global__ __launch_bounds__(AC_NT) void autocorr_lag_kernel(const double* x, AcShape sh, const double* mean, long long lagbase,
                                                             double* partial) {
    extern __shared__ double ac_tile[];
    double* A = ac_tile;
    double* W = ac_tile + AC_TC * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long s = (long long)blockIdx.x * 64 + lane;
    const bool live = s < sh.S;
    const int c = blockIdx.y;
    const long long L = lagbase + (long long)blockIdx.z * AC_LW;     // first lag of this workgroup
    const int l0 = wave * AC_JL;                                     // first lag of this wave, relative to L
    const double m = live ? mean[s] : 0.0;
    const long long ntiles = (sh.n_t + AC_TC - 1) / AC_TC;
    const long long tile0 = (long long)c * sh.tiles_per_chunk;
    const long long tile1 = tile0 + sh.tiles_per_chunk < ntiles ? tile0 + sh.tiles_per_chunk : ntiles;

    double acc[AC_JL];
#pragma unroll
    for (int j = 0; j < AC_JL; ++j) acc[j] = 0.0;

    for (long long tile = tile0; tile < tile1; ++tile) {
        const long long t0 = tile * AC_TC;
        if (t0 + L >= sh.n_t) break;                                 // every product of this and the later tiles is zero
        __syncthreads();                                             // the previous tile has been read
        for (int r = wave; r < AC_ROWS; r += AC_WAVES) {
            const long long t = r < AC_TC ? t0 + r : t0 + L + (r - AC_TC);
            double v = 0.0;
            if (live && t < sh.n_t) v = ac_row(x, sh, t)[s] - m;
            ac_tile[r * 64 + lane] = v;
        }
        __syncthreads();
        // ring[(u + j) % AC_JL] holds W[tb + l0 + u + j] at step tb + u: each step retires one value and reads one
        double ring[AC_JL];
#pragma unroll
        for (int j = 0; j < AC_JL; ++j) ring[j] = W[(l0 + j) * 64 + lane];
#pragma unroll 1
        for (int tb = 0; tb < AC_TC; tb += AC_JL) {
#pragma unroll
            for (int u = 0; u < AC_JL; ++u) {
                const double av = A[(tb + u) * 64 + lane];
#pragma unroll
                for (int j = 0; j < AC_JL; ++j) acc[j] = fma(av, ring[(u + j) % AC_JL], acc[j]);
                ring[u] = W[(tb + l0 + u + AC_JL) * 64 + lane];      // row <= AC_TC + AC_LW - 1: inside W
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < AC_JL; ++j) {
            const long long jl = (long long)blockIdx.z * AC_LW + l0 + j;      // < AC_LB
            partial[((long long)c * AC_LB + jl) * sh.S + s] = acc[j];
        }
    }
}

// A(0) of every series from the lag-0 partials (chunks in order)
__global__ __launch_bounds__(64) void autocorr_a0_kernel(AcShape sh, const double* partial, double* a0) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= sh.S) return;
    double sum = 0.0;
    for (int c = 0; c < sh.nch; ++c) sum += partial[(long long)c * AC_LB * sh.S + s];
    a0[s] = sum;
}

// one workgroup per lag: chunks in order per series, / A(0), then the walkers in order per dimension
__global__ __launch_bounds__(256) void autocorr_reduce_kernel(AcShape sh, double* partial, const double* a0, int n_w, int n_d,
                                                              double* f, long long ldf, long long col0) {
    const long long j = blockIdx.x;
    double* q = partial + j * sh.S;                                  // chunk 0's slot of this lag: each thread reads, then writes, its own s
    for (long long s = threadIdx.x; s < sh.S; s += 256) {
        double sum = 0.0;
        for (int c = 0; c < sh.nch; ++c) sum += partial[((long long)c * AC_LB + j) * sh.S + s];
        q[s] = sum / a0[s];
    }
    __threadfence_block();
    __syncthreads();
    if ((int)threadIdx.x < n_d) {
        double sum = 0.0;
        for (int k = 0; k < n_w; ++k) sum += q[(long long)k * n_d + threadIdx.x];
        f[(long long)threadIdx.x * ldf + col0 + j] = sum / (double)n_w;
    }
}

int ac_prepare_lds(hipStream_t s) {
    static ApgpLdsOnce once;
    const int dev = apgp_stream_device(s);
    if (dev < 0 || dev >= 64) {
        apgp_set_error("apgp_autocorr_block: no device for the stream");
        return -2;
    }
    return apgp_raise_lds(once, "apgp_autocorr_block", dev, (int)(AC_ROWS * 64 * sizeof(double)), {(const void*)autocorr_lag_kernel});
}

bool ac_sizes_ok(int64_t n_t, int64_t n_w, int32_t n_d) {
    return n_t >= 1 && n_t < AC_MAX_T && n_w >= 1 && n_w <= APGP_MAX_N && n_d >= 1 && n_d <= APGP_MAX_DIM;
}

}  // namespace

extern "C" int64_t apgp_autocorr_work_len(int64_t n_t, int64_t n_w, int32_t n_d) {
    if (!ac_sizes_ok(n_t, n_w, n_d)) return -1;
    const long long S = (long long)n_w * n_d;
    const AcShape sh = ac_shape(n_t, S, 0, 1);
    return S * (2 + (long long)AC_LB * sh.nch);
}

extern "C" int apgp_autocorr_block(const double* x, int64_t n_t, int64_t n_w, int32_t n_d, int64_t row0, int64_t row_stride,
                                   int64_t lag0, int64_t nlags, int32_t reuse_stats, double* work, double* f, void* stream) {
    APGP_CHECK_ARG(x && work && f, "null pointer");
    APGP_CHECK_ARG(n_t >= 1 && n_t < AC_MAX_T, "1 <= n_t < 2^31 required");
    APGP_CHECK_ARG(n_w >= 1 && n_w <= APGP_MAX_N, "1 <= n_w <= 2^24 required");
    APGP_CHECK_ARG(n_d >= 1 && n_d <= APGP_MAX_DIM, "1 <= n_d <= APGP_MAX_DIM required");
    APGP_CHECK_ARG(row0 >= 0 && row0 < AC_MAX_T, "0 <= row0 < 2^31 required");
    APGP_CHECK_ARG(row_stride >= 1 && row_stride < AC_MAX_T, "1 <= row_stride < 2^31 required");
    APGP_CHECK_ARG(lag0 >= 0 && lag0 < AC_MAX_T, "0 <= lag0 < 2^31 required");
    APGP_CHECK_ARG(nlags >= 1 && nlags < AC_MAX_T, "1 <= nlags < 2^31 required");
    const long long S = (long long)n_w * n_d;                        // < 2^29
    // rows < 2^31 + 2^62 fits int64; its product with S is checked by division
    const long long rows = row0 + (n_t - 1) * row_stride + 1;
    APGP_CHECK_ARG(rows <= AC_MAX_ELEMS / S, "the chain view spans 2^60 elements or more");
    hipStream_t s = (hipStream_t)stream;
    const AcShape sh = ac_shape(n_t, S, row0, row_stride);
    double* mean = work;
    double* a0 = work + S;
    double* partial = work + 2 * S;
    const unsigned sg = (unsigned)((S + 63) / 64);
    const size_t lds = (size_t)AC_ROWS * 64 * sizeof(double);
    const int rc = ac_prepare_lds(s);
    if (rc) return rc;

    if (!reuse_stats) {
        hipLaunchKernelGGL(autocorr_mean_partial_kernel, dim3(sg, (unsigned)sh.nchm), dim3(64), 0, s, x, sh, partial);
        APGP_CHECK_LAUNCH();
        hipLaunchKernelGGL(autocorr_mean_reduce_kernel, dim3(sg), dim3(64), 0, s, x, sh, (const double*)partial, mean);
        APGP_CHECK_LAUNCH();
        if (lag0 != 0) {
            // A(0) from a pass over the first lags, as a block that starts at lag 0 gets it
            hipLaunchKernelGGL(autocorr_lag_kernel, dim3(sg, (unsigned)sh.nch, 1), dim3(AC_NT), lds, s, x, sh, (const double*)mean,
                               0ll, partial);
            APGP_CHECK_LAUNCH();
            hipLaunchKernelGGL(autocorr_a0_kernel, dim3(sg), dim3(64), 0, s, sh, (const double*)partial, a0);
            APGP_CHECK_LAUNCH();
        }
    }
    for (long long done = 0; done < nlags; done += AC_LB) {
        const long long nl = nlags - done < AC_LB ? nlags - done : AC_LB;
        const unsigned lg = (unsigned)((nl + AC_LW - 1) / AC_LW);
        hipLaunchKernelGGL(autocorr_lag_kernel, dim3(sg, (unsigned)sh.nch, lg), dim3(AC_NT), lds, s, x, sh, (const double*)mean,
                           (long long)(lag0 + done), partial);
        APGP_CHECK_LAUNCH();
        if (!reuse_stats && lag0 == 0 && done == 0) {
            hipLaunchKernelGGL(autocorr_a0_kernel, dim3(sg), dim3(64), 0, s, sh, (const double*)partial, a0);
            APGP_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(autocorr_reduce_kernel, dim3((unsigned)nl), dim3(256), 0, s, sh, partial, (const double*)a0, (int)n_w,
                           (int)n_d, f, (long long)nlags, done);
        APGP_CHECK_LAUNCH();
    }
    return 0;
}
