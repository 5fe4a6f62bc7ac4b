// Evidence and posterior moments by importance sampling over the GP-mean surrogate (DESIGN.md "Evidence by importance
// sampling").  The surrogate models the unnormalised log-posterior, so Z = int exp(mu(t)) dt; with M draws t_i from a
// proposal q, log w_i = mu(t_i) - ln q(t_i), and everything the estimate needs is one record of weighted sums.
//
//   apgp_mix_candidates   draws from a Gaussian mixture (counter-based, a row depends on (seed, global row) only) and the
//                         proposal density at every stored draw;
//   apgp_importance_pass  log w per row -- the hot path: a candidate per thread, the training stream staged tile by tile
//                         in LDS and read as broadcasts, so a row of xs is fetched once per workgroup instead of once
//                         per candidate as in predict_mean_kernel -- then the record
//                           [lmax, S0, S2, cnt, s1 (D), S (D(D+1)/2)],  e_i = exp(log w_i - lmax),
//                         in three launches: log w and per-workgroup maxima; the weighted moments per workgroup about
//                         the global maximum; a fixed-tree reduction of the partials.  No atomics: every sum runs in an
//                         order that depends on m alone.
#include "apgp_common.h"
#include "draws.h"
#include "ens_moves.h"
#include "gmm_logpdf.h"
#include "scratch.h"
#include <cmath>
#include <mutex>
#include <vector>

#define MIX_TAG 0x4d495854u            // "MIXT": the mixture proposal's Philox counter tag
#define IMP_THREADS APGP_IMP_BLOCK     // candidates per workgroup pass, one per thread
#define IMP_NB_MAX APGP_IMP_MAX_BLOCKS // workgroups of a pass: beyond it a workgroup takes further tiles of candidates
#define IMP_ROWS 128                   // training rows per LDS tile

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Mixture proposal (the parameters' device image, MixArgs and the row's arithmetic: draws.h, shared with sobol.hip).
// Row g: Philox4x32-10, key = seed, counter (g low, g high, j, "MIXT"); j = 0: u01(words 0, 1) picks the component (the
// first k with u < cumw[k]); j = 1 + d / 2: words 0, 1 give dimension d's uniform, words 2, 3 dimension d + 1's;
// z_d = prior_gauss(0, 1, u); t_i = c_i + sum_{j <= i} A_ij z_j (an fma chain in ascending j, then one addition).
// ln q is evaluated at the stored t: logsumexp_k(gmm_logpdf(t | k)), the arithmetic of gmm_pass_kernel's score.
// ---------------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void mix_candidates_kernel(MixArgs a) {
    __shared__ double slp[MIX_MAX_K][256];
    const int tid = threadIdx.x;
    const unsigned int k0 = (unsigned int)a.seed, k1 = (unsigned int)(a.seed >> 32);
    for (long long i = (long long)blockIdx.x * 256 + tid; i < a.m; i += (long long)gridDim.x * 256) {
        const unsigned long long g = (unsigned long long)(a.idx_offset + i);
        unsigned int c[4] = {(unsigned int)g, (unsigned int)(g >> 32), 0u, MIX_TAG};
        philox4x32(c, k0, k1);
        const int k = mix_pick(a, u01(c[0], c[1]));
        double z[DP];
#pragma unroll
        for (int d = 0; d < DP; d += 2) {
            z[d] = 0.0;
            z[d + 1] = 0.0;
            if (d < a.D) {
                unsigned int cd[4] = {(unsigned int)g, (unsigned int)(g >> 32), (unsigned int)(1 + (d >> 1)), MIX_TAG};
                philox4x32(cd, k0, k1);
                z[d] = prior_gauss(0.0, 1.0, u01(cd[0], cd[1]));
                if (d + 1 < a.D) z[d + 1] = prior_gauss(0.0, 1.0, u01(cd[2], cd[3]));
            }
        }
        mix_row<DP>(a, i, tid, k, z, slp);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// log w per row.  The kernel-value arithmetic is predict_mean_kernel's (paired accumulators, apgp_exp's table path,
// APGP_LIN_SUM), four training rows per step through apgp_exp4 into four partial sums as in fantasy_kernel; the sum over
// the training rows therefore runs in another order than apgp_predict_mean's: the two agree to rounding, not to the bit.
// Rows past n of the packed stream are zeros with alpha = 0: the loop stops at n rounded up to 4.
// ---------------------------------------------------------------------------------------------------------------------
struct ImpArgs {
    const double* T;
    const double* lnq;
    const double* xs;
    double* logw;
    double* pmax;
    long long m, nrow;
    int ndim, lin_order, has_box;
    double mean, amp, lin_coef;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

template <int DPAD>
__global__ __launch_bounds__(IMP_THREADS) void imp_logw_kernel(ImpArgs a) {
    constexpr int XS = DPAD + 2;                 // packed stream row: scaled x | alpha | 0
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double tile[IMP_ROWS * XS];
    __shared__ double smax[IMP_THREADS / 64];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x;
    const long long nct = (a.m + IMP_THREADS - 1) / IMP_THREADS;
    double wmax = -INFINITY;
    for (long long ct = blockIdx.x; ct < nct; ct += gridDim.x) {
        const long long row = ct * IMP_THREADS + tid;
        const bool live = row < a.m;
        double tt[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) tt[d] = (live && d < a.ndim) ? a.T[row * a.ndim + d] * a.sc[d] : 0.0;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (long long r0 = 0; r0 < a.nrow; r0 += IMP_ROWS) {
            const int rows = (int)(a.nrow - r0 < IMP_ROWS ? a.nrow - r0 : IMP_ROWS);      // a multiple of 4
            __syncthreads();                     // the previous tile has been consumed (and etab is loaded)
            const f64x2* src = (const f64x2*)(a.xs + r0 * XS);
            for (int e = tid; e < rows * (XS / 2); e += IMP_THREADS) ((f64x2*)tile)[e] = src[e];
            __syncthreads();
            for (int r = 0; r < rows; r += 4) {
                double ex[4], kv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double* xr = tile + (r + q) * XS;
                    double s = 0.0, s3 = 0.0;
#pragma unroll
                    for (int d = 0; d < DPAD; d += 2) {
                        const double df0 = tt[d] - xr[d];
                        const double df1 = tt[d + 1] - xr[d + 1];
                        s = fma(df0, df0, s);
                        s3 = fma(df1, df1, s3);
                    }
                    ex[q] = -(s + s3);
                }
                apgp_exp4(ex, kv, etab);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double* xr = tile + (r + q) * XS;
                    double k = a.amp * kv[q];
                    if (a.lin_coef != 0.0) {
                        double ls;
                        APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xr[d_] * a.lw[d_]);
                        k = fma(a.lin_coef, ls, k);
                    }
                    acc[q] = fma(k, xr[DPAD], acc[q]);
                }
            }
        }
        if (live) {
            const double mu = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + a.mean;
            const double lq = a.lnq ? a.lnq[row] : 0.0;
            bool ok = isfinite(mu) && isfinite(lq);
            for (int d = 0; d < a.ndim; ++d) {
                const double x = a.T[row * a.ndim + d];
                if (!isfinite(x)) ok = false;
                if (a.has_box && !(x >= a.lo[d] && x <= a.hi[d])) ok = false;
            }
            const double lw = ok ? mu - lq : -INFINITY;
            a.logw[row] = lw;
            wmax = fmax(wmax, lw);
        }
    }
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o));
    if ((tid & 63) == 0) smax[tid >> 6] = wmax;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < IMP_THREADS / 64; ++w) wmax = fmax(wmax, smax[w]);
        a.pmax[blockIdx.x] = wmax;
    }
}

// the largest of the nb per-workgroup maxima, in every thread of the workgroup (a maximum does not depend on the order)
__device__ __forceinline__ double imp_global_max(const double* pmax, long long nb, double* sred) {
    double v = -INFINITY;
    for (long long b = threadIdx.x; b < nb; b += IMP_THREADS) v = fmax(v, pmax[b]);
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sred[0];
    for (int w = 1; w < IMP_THREADS / 64; ++w) v = fmax(v, sred[w]);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weighted moments about the centre c, per workgroup.  A tile of imp_mom_tile(DP) rows is staged in LDS as t - c (zeros for a
// row whose log w is -inf: its coordinates may be NaN) with a constant 1 in slot DP, beside three weights per row: e =
// exp(log w - lmax) (apgp_exp; 0 below -700 and for log w = -inf), e^2, and 1 where log w is finite.  Every output is
// sum_rows (w a) b for one weight and two slots; a thread owns outputs tid, tid + 256, .. and sums the tile's rows in
// order, then its tiles in order.  Outputs: 0 = S0, 1 = S2, 2 = cnt, 3 .. 2 + D = s1, then S packed as apgp_gmm_pass
// packs it (S[i][j], i <= j, at j (j + 1) / 2 + i).
// blockIdx.y is the draw (apgp_path_importance: one vector of log-weights, one set of maxima and one set of partials per
// draw over the same rows; apgp_importance_pass launches one): a draw's sums see nothing of the others.
// ---------------------------------------------------------------------------------------------------------------------
struct MomArgs {
    const double* T;
    const double* logw;
    const double* pmax;
    double* partial;               // [draw][nout][nb]
    long long m, npmax;            // npmax maxima per draw, whose largest is the draw's lmax
    int D, nb, nout;
    double c[APGP_MAX_DIM];
};

constexpr int imp_mom_tile(int DP) { return DP >= 32 ? 128 : 256; }      // rows per tile: 256 x 33 doubles pass 64 KB of LDS

template <int DP>
__global__ __launch_bounds__(IMP_THREADS) void imp_moments_kernel(MomArgs a) {
    constexpr int XS = DP + 1;
    constexpr int MT = imp_mom_tile(DP);
    constexpr int NO = (3 + DP + ev_tri(DP) + IMP_THREADS - 1) / IMP_THREADS;
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double sred[IMP_THREADS / 64];
    __shared__ double xt[MT * XS];
    __shared__ double wt[3][MT];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x, D = a.D;
    const double* logw = a.logw + (long long)blockIdx.y * a.m;
    double* partial = a.partial + (long long)blockIdx.y * a.nout * a.nb;
    const double lmax = imp_global_max(a.pmax + (long long)blockIdx.y * a.npmax, a.npmax, sred);
    // this thread's outputs: weight and the two slots
    int ow[NO], oa[NO], ob[NO];
    double acc[NO];
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        const int o = q * IMP_THREADS + tid;
        int w = 0, ia = DP, ib = DP;
        if (o == 1) w = 1;
        else if (o == 2) w = 2;
        else if (o >= 3 && o < 3 + D) ia = o - 3;
        else if (o >= 3 + D) {
            const int tt = o - 3 - D;
            int j = 0;
            while ((j + 1) * (j + 2) / 2 <= tt && j < DP) ++j;
            ia = tt - j * (j + 1) / 2; ib = j;
        }
        ow[q] = w; oa[q] = ia; ob[q] = ib; acc[q] = 0.0;
    }
    const long long nct = (a.m + MT - 1) / MT;
    for (long long ct = blockIdx.x; ct < nct; ct += gridDim.x) {
        const long long r0 = ct * MT;
        const int rows = (int)(a.m - r0 < MT ? a.m - r0 : MT);
        __syncthreads();                         // the previous tile's sums are done (and etab, lmax are in place)
        if (tid < rows) {
            const double lw = logw[r0 + tid];
            const bool fin = lw > -INFINITY;
            double e = 0.0;
            if (fin) {
                const double d = lw - lmax;
                e = d < -700.0 ? 0.0 : apgp_exp(d, etab);
            }
            wt[0][tid] = e; wt[1][tid] = e * e; wt[2][tid] = fin ? 1.0 : 0.0;
            const double* t = a.T + (r0 + tid) * D;
            for (int d = 0; d < D; ++d) xt[tid * XS + d] = fin ? t[d] - a.c[d] : 0.0;
            for (int d = D; d < DP; ++d) xt[tid * XS + d] = 0.0;
            xt[tid * XS + DP] = 1.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NO; ++q) {
            if (q * IMP_THREADS + tid < a.nout) {
                const double* w = wt[ow[q]];
                const int ia = oa[q], ib = ob[q];
                double s = 0.0;
                for (int r = 0; r < rows; ++r) s = fma(w[r] * xt[r * XS + ia], xt[r * XS + ib], s);
                acc[q] += s;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        const int o = q * IMP_THREADS + tid;
        if (o < a.nout) partial[(long long)o * a.nb + blockIdx.x] = acc[q];
    }
}

// record[0] = lmax (workgroup 0); record[1 + o] = sum_b partial[o][b] (workgroup 1 + o), a fixed tree over the nb partials;
// blockIdx.y is the draw: its npmax maxima, its nout x nb partials, its record of 1 + nout doubles
__global__ __launch_bounds__(IMP_THREADS) void imp_final_kernel(const double* __restrict__ pmax, long long npmax,
                                                                const double* __restrict__ partial, int nb,
                                                                double* __restrict__ record) {
    __shared__ double red[IMP_THREADS];
    const int tid = threadIdx.x;
    const int nout = gridDim.x - 1;
    pmax += (long long)blockIdx.y * npmax;
    partial += (long long)blockIdx.y * nout * nb;
    record += (long long)blockIdx.y * (1 + nout);
    if (blockIdx.x == 0) {
        const double v = imp_global_max(pmax, npmax, red);
        if (tid == 0) record[0] = v;
        return;
    }
    const int o = blockIdx.x - 1;
    const double* p = partial + (long long)o * nb;
    double s = 0.0;
    for (int b = tid; b < nb; b += IMP_THREADS) s += p[b];
    red[tid] = s;
    __syncthreads();
    for (int h = IMP_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) record[1 + o] = red[0];
}

// dmax[draw] = the largest of the draw's npmax maxima (workgroup = draw)
__global__ __launch_bounds__(IMP_THREADS) void imp_draw_max_kernel(const double* __restrict__ pmax, long long npmax,
                                                                   double* __restrict__ dmax) {
    __shared__ double sred[IMP_THREADS / 64];
    const double v = imp_global_max(pmax + (long long)blockIdx.x * npmax, npmax, sred);
    if (threadIdx.x == 0) dmax[blockIdx.x] = v;
}

inline int imp_nb(long long m) {
    const long long t = (m + IMP_THREADS - 1) / IMP_THREADS;
    return (int)(t < IMP_NB_MAX ? t : IMP_NB_MAX);
}

}  // namespace

extern "C" int64_t apgp_mix_params_len(int32_t ndim, int32_t ncomp) {
    if (ndim < 1 || ndim > APGP_MAX_DIM || ncomp < 1 || ncomp > MIX_MAX_K) return -1;
    return (int64_t)ncomp * mix_user_len(ndim);
}

extern "C" int apgp_mix_candidates(double* T, double* lnq, int64_t m, int32_t ndim, int32_t ncomp, const double* params,
                                   uint64_t seed, int64_t idx_offset, void* stream) {
    return mix_draw_call(__func__, T, lnq, m, ndim, ncomp, params, seed, idx_offset, stream,
                         [](const MixArgs& a, int DP, long long blocks, hipStream_t s) {
                             const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
                             apgp_by_dpad(DP, [&](auto dp) {
                                 hipLaunchKernelGGL(mix_candidates_kernel<decltype(dp)::value>, grid, block, 0, s, a);
                             });
                         });
}

extern "C" int64_t apgp_importance_stats_len(int32_t ndim) {
    if (ndim < 1 || ndim > APGP_MAX_DIM) return -1;
    return 4 + ndim + ev_tri(ndim);
}

// Scratch: the per-workgroup maxima and partial sums (sized for the largest record), then m doubles of log w.
extern "C" int64_t apgp_importance_work_len(int64_t m) {
    if (m < 1) return 0;
    if (m > APGP_MAX_M) return -1;
    return (int64_t)imp_nb(m) * (1 + 3 + APGP_MAX_DIM + ev_tri(APGP_MAX_DIM)) + m;
}

extern "C" int apgp_importance_pass(const double* T, int64_t m, const double* lnq, const double* xs, int64_t n,
                                    const apgp_kernel_t* kern, double mean, const double* lo, const double* hi,
                                    const double* centre, double* logw_out, double* stats_out, double* work,
                                    void* stream) {
    APGP_CHECK_ARG(T && xs && kern && centre && stats_out && work, "null pointer");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M && n >= 1 && n <= APGP_MAX_N, "1 <= m <= APGP_MAX_M and 1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(std::isfinite(centre[d]), "the centre must be finite");
    const int nb = imp_nb(m), D = kc.ndim;
    const int nout = 3 + D + ev_tri(D);
    double* pmax = work;
    double* partial = work + nb;
    double* logw = logw_out ? logw_out : work + (long long)nb * (1 + 3 + APGP_MAX_DIM + ev_tri(APGP_MAX_DIM));
    ImpArgs a;
    a.T = T; a.lnq = lnq; a.xs = xs; a.logw = logw; a.pmax = pmax; a.m = m; a.nrow = apgp_round_up(n, 4); a.mean = mean;
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, D, lo, hi);
    MomArgs b;
    b.T = T; b.logw = logw; b.pmax = pmax; b.partial = partial; b.m = m; b.npmax = nb; b.D = D; b.nb = nb; b.nout = nout;
    for (int d = 0; d < APGP_MAX_DIM; ++d) b.c[d] = d < D ? centre[d] : 0.0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nb), block(IMP_THREADS);
    apgp_by_dpad(kc.dpad, [&](auto dp) { hipLaunchKernelGGL(imp_logw_kernel<decltype(dp)::value>, grid, block, 0, s, a); });
    APGP_CHECK_LAUNCH();
    apgp_by_dpad(kc.dpad, [&](auto dp) { hipLaunchKernelGGL(imp_moments_kernel<decltype(dp)::value>, grid, block, 0, s, b); });
    APGP_CHECK_LAUNCH();
    hipLaunchKernelGGL(imp_final_kernel, dim3((unsigned)(1 + nout)), block, 0, s, (const double*)pmax, (long long)nb,
                       (const double*)partial, nb, stats_out);
    APGP_CHECK_LAUNCH();
    return 0;
}

// The records of ndraws vectors of log-weights over the same rows (apgp_common.h; pathdraw.hip's apgp_path_importance):
// each draw's npmax maxima reduced to one, then the two kernels above with the draw as the grid's second dimension.
// Scratch: the draws' maxima, then their partial sums.
int64_t apgp_imp_draw_records_work_len(int64_t m, int32_t ndraws) {
    return (int64_t)ndraws * (1 + (int64_t)imp_nb(m) * (3 + APGP_MAX_DIM + ev_tri(APGP_MAX_DIM)));
}

int apgp_imp_draw_records(const double* T, int64_t m, int ndim, const double* centre, int ndraws, const double* logw,
                          const double* pmax, int64_t npmax, double* work, double* stats_out, hipStream_t s) {
    const int nb = imp_nb(m), D = ndim;
    const int nout = 3 + D + ev_tri(D);
    double* dmax = work;
    MomArgs b;
    b.T = T; b.logw = logw; b.pmax = dmax; b.partial = work + ndraws; b.m = m; b.npmax = 1; b.D = D; b.nb = nb; b.nout = nout;
    for (int d = 0; d < APGP_MAX_DIM; ++d) b.c[d] = d < D ? centre[d] : 0.0;
    const dim3 block(IMP_THREADS);
    hipLaunchKernelGGL(imp_draw_max_kernel, dim3((unsigned)ndraws), block, 0, s, pmax, (long long)npmax, dmax);
    APGP_CHECK_LAUNCH();
    apgp_by_dpad(apgp_dpad(D), [&](auto dp) {
        hipLaunchKernelGGL(imp_moments_kernel<decltype(dp)::value>, dim3((unsigned)nb, (unsigned)ndraws), block, 0, s, b);
    });
    APGP_CHECK_LAUNCH();
    hipLaunchKernelGGL(imp_final_kernel, dim3((unsigned)(1 + nout), (unsigned)ndraws), block, 0, s, (const double*)dmax,
                       1ll, (const double*)b.partial, nb, stats_out);
    APGP_CHECK_LAUNCH();
    return 0;
}
