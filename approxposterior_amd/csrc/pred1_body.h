// The body of pred1_small_kernel (linalg.hip) as a device function, shared with the device point search
// (nmsearch.hip) so that every (mu, sigma^2) the search evaluates through the dense inverse at n <= 256 carries the
// bits of apgp_predict1_host at the same point.  One workgroup of 256 threads; n <= 256.
//   tt:  the scaled candidate (DPAD doubles, x_d * sc_d; zero in the padded coordinates)
//   lw:  the linear term's per-dimension weights (KernConst::lw)
// On return (after the last barrier) red[0..3] hold the four wavefront partials of k*.alpha and red2[0..3] those of
// sum v^2, v = W k*; the caller forms mu = (red[0] + red[1]) + (red[2] + red[3]) + mean and q = sum_i red2[i] in that
// order (thread 0).  etab: the exp table in LDS, loaded by the caller.
#pragma once
#include "apgp_common.h"

template <int DPAD>
__device__ __forceinline__ void apgp_pred1_small_body(const double* xs, long long n, const double* tt, const double* lw,
                                                      double amp, double lin_coef, int ndim, int lin_order,
                                                      const double* W, long long ldw, const double* etab,
                                                      double* red, double* red2, double* ks, double* vs) {
    constexpr int XS = DPAD + 2;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double contrib = 0.0, kv = 0.0;
    if (t < n) {
        const double* xr = xs + (long long)t * XS;
        double s = 0.0, s3 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            const double df0 = tt[d] - xr[d], df1 = tt[d + 1] - xr[d + 1];
            s = fma(df0, df0, s);
            s3 = fma(df1, df1, s3);
        }
        kv = amp * apgp_exp(-(s + s3), etab);
        if (lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, ndim, lin_order, tt[d_] * xr[d_] * lw[d_]);
            kv = fma(lin_coef, ls, kv);
        }
        contrib = kv * xr[DPAD];                       // k* alpha
    }
    ks[t] = kv;
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o);
    if (lane == 0) red[w] = contrib;
    __syncthreads();
    // v = W k*: one wavefront per row, as winv_gemv_kernel (shift 0)
    for (long long i = w; i < n; i += 4) {
        const double* wr = W + i * ldw;
        double s0 = 0.0, s1 = 0.0;
        for (long long k = 2 * lane; k <= i; k += 128) {
            const f64x2 w2 = *(const f64x2*)(wr + k);
            s0 = fma(w2.x, ks[k] - 0.0, s0);
            if (k + 1 <= i) s1 = fma(w2.y, ks[k + 1] - 0.0, s1);
        }
        double s = s0 + s1;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) vs[i] = s;
    }
    __syncthreads();
    // sum v^2: virtual thread t of pred1_final_kernel's 1,024
    double sq = 0.0;
    if (t < n) sq = fma(vs[t], vs[t], sq);
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if (lane == 0) red2[w] = sq;
    __syncthreads();
}
