// Posterior function draws (apgp_path_draws; DESIGN.md "Posterior function draws").  By Matheron's rule a draw from the
// GP posterior is a prior draw plus a data term:
//   f_s(t) = mean + g_s(t) + k(t, X).v_s ,
//   g_s(t) = A sum_r W[s,r] cos(sqrt2 Z[r,:].ts + b_r) + sqrt(lin_coef) sum_d Wl[s,d] t_d^P ,   A = sqrt(2 amp / R)
// (random Fourier features of the squared-exponential part in the scaled coordinates ts = t sc, the exact D-feature map
// of the linear term).  Both sums have the shape (candidates x generated values).(values x draws): a value -- a kernel
// value k(t, x_n) or a cosine -- is generated once per candidate and contracted with the S weights of its row.
// One thread per candidate, PD_THREADS candidates per workgroup, as the fantasy pass of sweep.hip: the candidate's scaled
// coordinates and its S running sums stay in registers; training rows with their V rows, then frequency rows with their
// W columns, are staged through LDS in tiles of PD_ROWS shared by the workgroup (every lane reads the same LDS word: a
// broadcast).  Four values per step are generated together (four independent fp64 chains, apgp_exp4 / cos_turns4) and
// then contracted in one cluster of 4 S FMAs.  The epilogue adds the linear features and the mean, stores F and reduces
// the S arg-min partials of the workgroup; argmin_draws_kernel merges the partials, one workgroup per draw.
// Above APGP_PD_MMA_MIN_DRAWS draws (and D padded to at most 8) the contraction runs on the matrix cores instead:
// path_draws_mma_kernel below, same tiles, same epilogue.
// apgp_path_importance runs the same two kernels with a second epilogue chosen at compile time (WEIGHTS): log w = f - ln q
// under the importance gate and the workgroups' maxima instead of F and the arg-min partials; evidence.hip's moments
// kernels then turn each draw's log-weights into a record.
#include "apgp_common.h"
#include <cmath>

#define PD_THREADS 256
#define PD_ROWS 64         // rows per LDS tile (divides the packed stream's 512-row padding)
#define APGP_PD_INV_2PI 0x1.45f306dc9c883p-3
#define APGP_PD_MMA_MIN_DRAWS 8       // default: matrix-core contraction above this many draws (D padded to <= 8)

struct PathArgs {
    const double* T;
    const double* xs;
    const double* V;
    const double* Z;
    const double* b;
    const double* W;
    const double* Wl;
    double* F;
    const unsigned char* mask;
    const double* lnq;             // the weights epilogue only: ln q per row (NULL: zeros); F then receives log w
    double* part_u;
    long long* part_i;
    long long m, idx_offset, n, nblk;
    int ndim, nfeat, ndraws, has_box, lin_order;
    double mean, amp, lin_coef, feat_amp, lin_amp, zscale;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

// as best_merge of sweep.hip: NaN and +inf never win; ties resolve to the lowest global index
__device__ __forceinline__ void pd_best_merge(double& bu, long long& bi, double u, long long i) {
    if (i >= 0 && u < INFINITY && (u < bu || (u == bu && (bi < 0 || i < bi)))) { bu = u; bi = i; }
}

// cos(2 pi p) for four phases given in turns.  f = p - rint(p) is exact and lies in [-1/2, 1/2]; cos(2 pi f) =
// sin(2 pi h) with h = 1/4 - |f| in [-1/4, 1/4] (exact unless |p| < 1/8, where the rounding is below 2^-56 turns); an odd
// polynomial of degree 23 in h with (2 pi)^(2k+1) / (2k+1)! folded into the coefficients (the next Taylor term is below
// 1e-20 at h = 1/4).  Full-rate fp64 operations only; no table, no branch, no large-argument path.  The error is the
// rounding of the phase itself times 2 pi, plus a few ulp of 1 from the polynomial (tests/pathdraw_ref.py counts both).
__device__ __forceinline__ void pd_cos_turns4(const double (&ph)[4], double (&out)[4]) {
    double h[4], h2[4], p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = 0.25 - fabs(ph[i] - rint(ph[i]));
#pragma unroll
    for (int i = 0; i < 4; ++i) h2[i] = h[i] * h[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], -0x1.7215f879e1ac9p-14, 0x1.2877020d52cf0p-10);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], -0x1.8a404211f9547p-7);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], 0x1.aaec32af93359p-4);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], -0x1.6fadb9f155744p-1);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], 0x1.e8f434d018d63p+1);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], -0x1.e3074fde8871fp+3);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], 0x1.50783487ee782p+5);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], -0x1.32d2cce62bd86p+6);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], 0x1.466bc6775aae2p+6);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], -0x1.4abbce625be53p+5);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fma(h2[i], p[i], 0x1.921fb54442d18p+2);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = h[i] * p[i];
}

// The epilogue of one candidate (this thread's `row`; loads from the clamped `lrow`) for the NS draws s0 .. s0 + NS - 1
// whose sums are in f: the linear features and the mean, the gate (box, mask, NaN coordinate: u = +inf, F = NaN), the F
// store, and the wavefront's arg-min of u = -f per draw into su / si (SPAD x wavefronts).
// WEIGHTS (apgp_path_importance): the same f + mean, then log w = (f + mean) - ln q into F where the row passes the
// importance gate (every coordinate finite and inside the box, f and ln q finite) and -inf elsewhere, and the
// wavefront's maximum of log w per draw into su.
template <int NS, bool WEIGHTS>
__device__ __forceinline__ void pd_epilogue(const PathArgs& a, double (&f)[NS], int s0, long long row, long long lrow,
                                            bool live, double* su, long long* si) {
    constexpr int NW = PD_THREADS / 64;
    const int tid = threadIdx.x;
    bool adm = WEIGHTS || !(a.mask && a.mask[lrow] == 0);
    for (int d = 0; d < a.ndim; ++d) {
        const double x = a.T[lrow * a.ndim + d];
        if (a.has_box && !(x >= a.lo[d] && x <= a.hi[d])) adm = false;
        if (WEIGHTS ? !isfinite(x) : x != x) adm = false;        // a row with a NaN coordinate is inadmissible, as in the sweep
        if (a.lin_coef != 0.0) {
            double tp = 1.0;
            for (int e = 0; e < a.lin_order; ++e) tp *= x;
            tp *= a.lin_amp;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double wl = a.Wl[(s0 + s < a.ndraws ? s0 + s : 0) * a.ndim + d];
                f[s] = fma(s0 + s < a.ndraws ? wl : 0.0, tp, f[s]);
            }
        }
    }
    const int wave = tid >> 6;
    if constexpr (WEIGHTS) {
        const double lq = a.lnq ? a.lnq[lrow] : 0.0;
        if (!isfinite(lq)) adm = false;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double fs = f[s] + a.mean;
            const double lw = adm && isfinite(fs) ? fs - lq : -INFINITY;
            if (live && s0 + s < a.ndraws) a.F[(long long)(s0 + s) * a.m + row] = lw;
            double wm = live ? lw : -INFINITY;
            for (int o = 32; o > 0; o >>= 1) wm = fmax(wm, __shfl_xor(wm, o));
            if ((tid & 63) == 0) su[(s0 + s) * NW + wave] = wm;
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double fs = adm ? f[s] + a.mean : NAN;
        if (live && a.F && s0 + s < a.ndraws) a.F[(long long)(s0 + s) * a.m + row] = fs;
        double bu = INFINITY;
        long long bi = -1;
        if (live) pd_best_merge(bu, bi, adm ? -fs : INFINITY, a.idx_offset + row);
        for (int o = 32; o > 0; o >>= 1) {
            const double ou = __shfl_xor(bu, o);
            const long long oi = __shfl_xor(bi, o);
            pd_best_merge(bu, bi, ou, oi);
        }
        if ((tid & 63) == 0) { su[(s0 + s) * NW + wave] = bu; si[(s0 + s) * NW + wave] = bi; }
    }
}

// the workgroup's partial of every draw from its wavefronts' (call from every thread)
template <bool WEIGHTS>
__device__ __forceinline__ void pd_write_partials(const PathArgs& a, const double* su, const long long* si) {
    constexpr int NW = PD_THREADS / 64;
    const int tid = threadIdx.x;
    __syncthreads();
    if constexpr (WEIGHTS) {                     // the maxima alone, [draw][workgroup]
        if (tid < a.ndraws) {
            double wm = su[tid * NW];
            for (int w = 1; w < NW; ++w) wm = fmax(wm, su[tid * NW + w]);
            a.part_u[(long long)tid * a.nblk + blockIdx.x] = wm;
        }
        return;
    }
    if (tid < a.ndraws) {
        double bu = su[tid * NW];
        long long bi = si[tid * NW];
        for (int w = 1; w < NW; ++w) pd_best_merge(bu, bi, su[tid * NW + w], si[tid * NW + w]);
        a.part_u[(long long)tid * a.nblk + blockIdx.x] = bu;
        a.part_i[(long long)tid * a.nblk + blockIdx.x] = bi;
    }
}

// The three staging steps, shared by both kernels (call from every thread, between barriers).
template <int DPAD, int SPAD>
__device__ __forceinline__ void pd_stage_features(const PathArgs& a, int r0, double* xt, double* wt, double* bt) {
    const int tid = threadIdx.x;
    for (int e = tid; e < PD_ROWS * DPAD; e += PD_THREADS) {
        const int r = e / DPAD, d = e - r * DPAD;
        const bool in = r0 + r < a.nfeat && d < a.ndim;
        const double z = a.Z[in ? (long long)(r0 + r) * a.ndim + d : 0];
        xt[e] = in ? z * a.zscale : 0.0;
    }
    for (int e = tid; e < PD_ROWS * SPAD; e += PD_THREADS) {
        const int s = e / PD_ROWS, r = e - s * PD_ROWS;              // consecutive threads read consecutive features
        const bool in = r0 + r < a.nfeat && s < a.ndraws;
        const double w = a.W[in ? (long long)s * a.nfeat + r0 + r : 0];
        wt[r * SPAD + s] = in ? w : 0.0;                             // a feature past nfeat weighs nothing
    }
    if (tid < PD_ROWS) {
        const bool in = r0 + tid < a.nfeat;
        const double bb = a.b[in ? r0 + tid : 0];
        bt[tid] = in ? bb * APGP_PD_INV_2PI : 0.0;
    }
}

template <int DPAD, int SPAD>
__device__ __forceinline__ void pd_stage_train(const PathArgs& a, long long r0, double* xt, double* wt) {
    constexpr int XS = DPAD + 2;                 // packed stream row: scaled x | alpha | 0 (the last two are not read)
    const int tid = threadIdx.x;
    for (int e = tid; e < PD_ROWS * DPAD / 2; e += PD_THREADS) {     // (rows < ntile * PD_ROWS <= npad: inside the stream)
        const int r = e / (DPAD / 2), p = e - r * (DPAD / 2);
        *(f64x2*)(xt + r * DPAD + 2 * p) = *(const f64x2*)(a.xs + (r0 + r) * XS + 2 * p);
    }
    for (int e = tid; e < PD_ROWS * SPAD; e += PD_THREADS) {
        const int r = e / SPAD, s = e - r * SPAD;
        const bool in = r0 + r < a.n && s < a.ndraws;
        const double v = a.V[in ? (r0 + r) * a.ndraws + s : 0];
        wt[e] = in ? v : 0.0;                                        // 0 on the padding rows
    }
}

// SPAD: the draws padded to 1 / 8 / 16 / 32 columns (zero weights past ndraws), so that the running sums are indexed
// statically.  One draw alone would be one dependent FMA chain: it gets four partial sums, as the fantasy pass has.
// WEIGHTS selects the epilogue: false -- F and the arg-min partials (apgp_path_draws); true -- the log-weights and the
// per-workgroup maxima (apgp_path_importance).  The sums above it are the same code, hence the same bits.
template <int DPAD, int SPAD, bool WEIGHTS = false>
__global__ __launch_bounds__(PD_THREADS) void path_draws_kernel(PathArgs a) {
    constexpr int NACC = SPAD == 1 ? 4 : 1;
    constexpr int NW = PD_THREADS / 64;
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double xt[PD_ROWS * DPAD];   // scaled x rows, then frequency rows in turns
    __shared__ __attribute__((aligned(16))) double wt[PD_ROWS * SPAD];   // V rows, then W columns
    __shared__ double bt[PD_ROWS];                                       // phase offsets in turns
    __shared__ double su[SPAD * NW];
    __shared__ long long si[SPAD * NW];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * PD_THREADS + tid;
    const bool live = row < a.m;
    const long long lrow = live ? row : a.m - 1;                         // loads are clamped, stores are masked
    double tt[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) tt[d] = d < a.ndim ? a.T[lrow * a.ndim + d] * a.sc[d] : 0.0;
    double acc[NACC][SPAD];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int s = 0; s < SPAD; ++s) acc[q][s] = 0.0;

    // ---- random Fourier features: sum_r W[s,r] cos(2 pi (Zt[r,:].ts + bt[r])) ----
    const int nftile = (a.nfeat + PD_ROWS - 1) / PD_ROWS;
    for (int ti = 0; ti < nftile; ++ti) {
        __syncthreads();                         // the previous tile has been consumed
        const int r0 = ti * PD_ROWS;
        pd_stage_features<DPAD, SPAD>(a, r0, xt, wt, bt);
        __syncthreads();
        for (int r = 0; r < PD_ROWS; r += 4) {
            double ph[4], cv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* zr = xt + (r + q) * DPAD;
                double p = bt[r + q];
#pragma unroll
                for (int d = 0; d < DPAD; ++d) p = fma(zr[d], tt[d], p);
                ph[q] = p;
            }
            pd_cos_turns4(ph, cv);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < SPAD; ++s) acc[q % NACC][s] = fma(cv[q], wt[(r + q) * SPAD + s], acc[q % NACC][s]);
        }
    }
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int s = 0; s < SPAD; ++s) acc[q][s] *= a.feat_amp;

    // ---- data term: sum_n k(t, x_n) V[n,s] ----
    const long long ntile = a.V ? (a.n + PD_ROWS - 1) / PD_ROWS : 0;
    for (long long ti = 0; ti < ntile; ++ti) {
        __syncthreads();
        pd_stage_train<DPAD, SPAD>(a, ti * PD_ROWS, xt, wt);
        __syncthreads();
        for (int r = 0; r < PD_ROWS; r += 4) {
            double ex[4], kv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* xr = xt + (r + q) * DPAD;
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
                const double* xr = xt + (r + q) * DPAD;
                double k = a.amp * kv[q];
                if (a.lin_coef != 0.0) {
                    double ls;
                    APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xr[d_] * a.lw[d_]);
                    k = fma(a.lin_coef, ls, k);
                }
                kv[q] = k;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < SPAD; ++s) acc[q % NACC][s] = fma(kv[q], wt[(r + q) * SPAD + s], acc[q % NACC][s]);
        }
    }

    // ---- epilogue: linear features, mean, gate, F, arg-min partials ----
    double f[SPAD];
#pragma unroll
    for (int s = 0; s < SPAD; ++s) f[s] = NACC == 4 ? (acc[0][s] + acc[1 % NACC][s]) + (acc[2 % NACC][s] + acc[3 % NACC][s]) : acc[0][s];
    pd_epilogue<SPAD, WEIGHTS>(a, f, 0, row, lrow, live, su, si);
    pd_write_partials<WEIGHTS>(a, su, si);
}

// The same sums with the contraction on the matrix cores (apgp_mma16's fragments: v_mfma_f64_4x4x4_4b, A lane = row +
// 16 k, B lane = column + 16 k, the B fragment read at four rotated columns).  A wavefront still owns 64 candidates, as
// four blocks of 16: lane l generates, for tile row r + (l >> 4), the values of the four candidates 16 b + (l & 15) --
// which ARE the A fragments of the four blocks, so no value crosses lanes -- and reads ONE weight per column block and
// rotation instead of every weight of the row: the vector form's 16 S bytes of LDS per value become 32 NCB.  Same number
// of generated values per lane and step; 16 NCB matrix instructions per step in one cluster.  The sums come back to
// one-thread-per-candidate through a 64 x 16 tile per wavefront in LDS, a column block at a time, and take the shared
// epilogue.  For D padded to at most 8 (four candidates' coordinates per lane) and S padded to 16 NCB, NCB = 1, 2.
template <int DPAD, int NCB, bool WEIGHTS = false>
__global__ __launch_bounds__(PD_THREADS) void path_draws_mma_kernel(PathArgs a) {
    constexpr int SPAD = 16 * NCB;
    constexpr int NW = PD_THREADS / 64;
    constexpr int FT = 17;                                               // row stride of the hand-back tile
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double xt[PD_ROWS * DPAD];
    __shared__ __attribute__((aligned(16))) double wt[PD_ROWS * SPAD];
    __shared__ double bt[PD_ROWS];
    __shared__ double ft[NW * 64 * FT];
    __shared__ double su[SPAD * NW];
    __shared__ long long si[SPAD * NW];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const long long base = (long long)blockIdx.x * PD_THREADS + wave * 64;
    double tt[4][DPAD];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const long long c = base + 16 * b + li;
        const long long lc = c < a.m ? c : a.m - 1;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) tt[b][d] = d < a.ndim ? a.T[lc * a.ndim + d] * a.sc[d] : 0.0;
    }
    int bcol[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bcol[r] = (li - 4 * r) & 15;
    double acc[4][NCB][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[b][c][r] = 0.0;
    auto contract = [&](const double (&val)[4], int trow) {
        double bf[NCB][4];
#pragma unroll
        for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) bf[c][r] = wt[trow * SPAD + 16 * c + bcol[r]];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[b][c][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(val[b], bf[c][r], acc[b][c][r], 0, 0, 0);
    };

    const int nftile = (a.nfeat + PD_ROWS - 1) / PD_ROWS;
    for (int ti = 0; ti < nftile; ++ti) {
        __syncthreads();
        pd_stage_features<DPAD, SPAD>(a, ti * PD_ROWS, xt, wt, bt);
        __syncthreads();
        for (int r = 0; r < PD_ROWS; r += 4) {
            const double* zr = xt + (r + kq) * DPAD;
            double ph[4], cv[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double p = bt[r + kq];
#pragma unroll
                for (int d = 0; d < DPAD; ++d) p = fma(zr[d], tt[b][d], p);
                ph[b] = p;
            }
            pd_cos_turns4(ph, cv);
            contract(cv, r + kq);
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[b][c][r] *= a.feat_amp;

    const long long ntile = a.V ? (a.n + PD_ROWS - 1) / PD_ROWS : 0;
    for (long long ti = 0; ti < ntile; ++ti) {
        __syncthreads();
        pd_stage_train<DPAD, SPAD>(a, ti * PD_ROWS, xt, wt);
        __syncthreads();
        for (int r = 0; r < PD_ROWS; r += 4) {
            const double* xr = xt + (r + kq) * DPAD;
            double ex[4], kv[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double s = 0.0, s3 = 0.0;
#pragma unroll
                for (int d = 0; d < DPAD; d += 2) {
                    const double df0 = tt[b][d] - xr[d];
                    const double df1 = tt[b][d + 1] - xr[d + 1];
                    s = fma(df0, df0, s);
                    s3 = fma(df1, df1, s3);
                }
                ex[b] = -(s + s3);
            }
            apgp_exp4(ex, kv, etab);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double k = a.amp * kv[b];
                if (a.lin_coef != 0.0) {
                    double ls;
                    APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[b][d_] * xr[d_] * a.lw[d_]);
                    k = fma(a.lin_coef, ls, k);
                }
                kv[b] = k;
            }
            contract(kv, r + kq);
        }
    }

    // back to one thread per candidate: acc[b][c][r] of lane l is row 4 ((l >> 2) & 3) + (l >> 4) of block b and column
    // 4 ((((l >> 2) & 3) - r) & 3) + (l & 3) of column block c (csrc/mma16.h)
    const long long row = (long long)blockIdx.x * PD_THREADS + tid;
    const bool live = row < a.m;
    const long long lrow = live ? row : a.m - 1;
    double* fw = ft + wave * 64 * FT;
    const int frow = 4 * ((lane >> 2) & 3) + (lane >> 4);
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
        __syncthreads();                         // the previous column block has been read
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                fw[(16 * b + frow) * FT + 4 * ((((lane >> 2) & 3) - r) & 3) + (lane & 3)] = acc[b][c][r];
        __syncthreads();
        double f[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) f[s] = fw[lane * FT + s];
        pd_epilogue<16, WEIGHTS>(a, f, 16 * c, row, lrow, live, su, si);
    }
    pd_write_partials<WEIGHTS>(a, su, si);
}

// final arg-min over the per-workgroup partials: workgroup s merges the nblk partials of draw s
__global__ __launch_bounds__(256) void argmin_draws_kernel(const double* part_u, const long long* part_i,
                                                           long long nblk, apgp_best_t* best) {
    __shared__ double su[4];
    __shared__ long long si[4];
    const double* pu = part_u + (long long)blockIdx.x * nblk;
    const long long* pi = part_i + (long long)blockIdx.x * nblk;
    double bu = INFINITY;
    long long bi = -1;
    for (long long p = threadIdx.x; p < nblk; p += 256) pd_best_merge(bu, bi, pu[p], pi[p]);
    for (int o = 32; o > 0; o >>= 1) {
        const double ou = __shfl_xor(bu, o);
        const long long oi = __shfl_xor(bi, o);
        pd_best_merge(bu, bi, ou, oi);
    }
    if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = bu; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) pd_best_merge(bu, bi, su[i], si[i]);
        best[blockIdx.x].u = bu;
        best[blockIdx.x].index = bi;
    }
}

// Scratch: the arg-min partials (value, index) of every workgroup for every draw -- 2 ndraws doubles per workgroup.
extern "C" int64_t apgp_path_draws_work_len(int64_t m, int32_t ndraws) {
    if (m < 1 || ndraws < 1) return 0;
    if (m > APGP_MAX_M || ndraws > APGP_MAX_DRAWS) return -1;
    return 2 * (int64_t)ndraws * ((m + PD_THREADS - 1) / PD_THREADS);
}

// 0: the faster form per shape (below), 1: the vector contraction, 2: the matrix-core contraction wherever it exists
static int g_pd_mode = 0;
extern "C" int apgp_path_draws_mode(int mode) {
    const int was = g_pd_mode;
    if (mode > 2) return -1;
    if (mode >= 0) g_pd_mode = mode;
    return was;
}

template <int DPAD, bool WEIGHTS>
static void path_draws_launch(int ndraws, dim3 grid, hipStream_t s, const PathArgs& a) {
    const dim3 block(PD_THREADS);
    if constexpr (DPAD <= 8) {
        const bool mma = g_pd_mode == 2 ? ndraws > 1 : g_pd_mode == 0 && ndraws > APGP_PD_MMA_MIN_DRAWS;
        if (mma) {
            if (ndraws <= 16) hipLaunchKernelGGL((path_draws_mma_kernel<DPAD, 1, WEIGHTS>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((path_draws_mma_kernel<DPAD, 2, WEIGHTS>), grid, block, 0, s, a);
            return;
        }
    }
    if (ndraws == 1) hipLaunchKernelGGL((path_draws_kernel<DPAD, 1, WEIGHTS>), grid, block, 0, s, a);
    else if (ndraws <= 8) hipLaunchKernelGGL((path_draws_kernel<DPAD, 8, WEIGHTS>), grid, block, 0, s, a);
    else if (ndraws <= 16) hipLaunchKernelGGL((path_draws_kernel<DPAD, 16, WEIGHTS>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((path_draws_kernel<DPAD, 32, WEIGHTS>), grid, block, 0, s, a);
}

// what both entry points put into the argument struct once their arguments are checked (the outputs are theirs)
static void pd_fill_args(PathArgs& a, const KernConst& kc, const double* T, int64_t m, const double* xs, int64_t n,
                         double mean, const double* V, const double* Z, const double* b, const double* W,
                         const double* Wl, int32_t nfeat, int32_t ndraws, const double* lo, const double* hi) {
    a.T = T; a.xs = xs; a.V = V; a.Z = Z; a.b = b; a.W = W; a.Wl = Wl;
    a.nblk = (m + PD_THREADS - 1) / PD_THREADS;
    a.m = m; a.n = V ? n : 0; a.nfeat = nfeat; a.ndraws = ndraws; a.mean = mean;
    a.feat_amp = sqrt(2.0 * kc.amp / (double)nfeat);
    a.lin_amp = sqrt(kc.lin_coef);
    a.zscale = sqrt(2.0) * APGP_PD_INV_2PI;      // sqrt2 / (2 pi): the frequencies in turns per scaled unit
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
}

extern "C" int apgp_path_draws(const double* T, int64_t m, int64_t idx_offset, const double* xs, int64_t n,
                               const apgp_kernel_t* kern, double mean, const double* V, const double* Z,
                               const double* b, const double* W, const double* Wl, int32_t nfeat, int32_t ndraws,
                               const double* lo, const double* hi, const uint8_t* mask, double* F, void* part,
                               apgp_best_t* best, void* stream) {
    APGP_CHECK_ARG(T && kern && Z && b && W && part && best, "null pointer");
    APGP_CHECK_ARG(V == NULL || xs != NULL, "null pointer (xs is required with V)");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M, "m >= 1 required");
    APGP_CHECK_ARG(V == NULL || (n >= 1 && n <= APGP_MAX_N), "n >= 1 required");
    APGP_CHECK_ARG((m + PD_THREADS - 1) / PD_THREADS < (1ll << 31), "m too large for one grid");
    APGP_CHECK_ARG(ndraws >= 1 && ndraws <= APGP_MAX_DRAWS, "1 <= ndraws <= APGP_MAX_DRAWS required");
    APGP_CHECK_ARG(nfeat >= 1 && nfeat <= APGP_MAX_FEATURES, "1 <= nfeat <= APGP_MAX_FEATURES required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(Wl != NULL || kc.lin_coef == 0.0, "null pointer (Wl is required with a linear term)");
    PathArgs a;
    pd_fill_args(a, kc, T, m, xs, n, mean, V, Z, b, W, Wl, nfeat, ndraws, lo, hi);
    a.F = F; a.mask = mask; a.lnq = NULL; a.idx_offset = idx_offset;
    a.part_u = (double*)part;
    a.part_i = (long long*)((double*)part + (long long)ndraws * a.nblk);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nblk);
    apgp_by_dpad(kc.dpad, [&](auto dp) { path_draws_launch<decltype(dp)::value, false>(ndraws, grid, s, a); });
    hipLaunchKernelGGL(argmin_draws_kernel, dim3((unsigned)ndraws), dim3(256), 0, s, a.part_u, a.part_i, a.nblk, best);
    APGP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// apgp_path_importance (DESIGN.md "Evidence over path draws"): the contraction above with the weights epilogue, then
// evidence.hip's moments once per draw.  Scratch, per draw: the workgroups' maxima of stage one, what stage two needs
// (apgp_imp_draw_records_work_len), and m doubles of log w (unused when the caller takes logw_out).
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t apgp_path_importance_work_len(int64_t m, int32_t ndraws) {
    if (m < 1 || ndraws < 1) return 0;
    if (m > APGP_MAX_M || ndraws > APGP_MAX_DRAWS) return -1;
    return (int64_t)ndraws * ((m + PD_THREADS - 1) / PD_THREADS + m) + apgp_imp_draw_records_work_len(m, ndraws);
}

extern "C" int apgp_path_importance(const double* T, int64_t m, const double* lnq, const double* xs, int64_t n,
                                    const apgp_kernel_t* kern, double mean, const double* V, const double* Z,
                                    const double* b, const double* W, const double* Wl, int32_t nfeat, int32_t ndraws,
                                    const double* lo, const double* hi, const double* centre, double* logw_out,
                                    double* stats_out, double* work, void* stream) {
    APGP_CHECK_ARG(T && kern && Z && b && W && centre && stats_out && work, "null pointer");
    APGP_CHECK_ARG(V == NULL || xs != NULL, "null pointer (xs is required with V)");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M, "1 <= m <= APGP_MAX_M required");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG((m + PD_THREADS - 1) / PD_THREADS < (1ll << 31), "m too large for one grid");
    APGP_CHECK_ARG(ndraws >= 1 && ndraws <= APGP_MAX_DRAWS, "1 <= ndraws <= APGP_MAX_DRAWS required");
    APGP_CHECK_ARG(nfeat >= 1 && nfeat <= APGP_MAX_FEATURES, "1 <= nfeat <= APGP_MAX_FEATURES required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(Wl != NULL || kc.lin_coef == 0.0, "null pointer (Wl is required with a linear term)");
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(std::isfinite(centre[d]),"the centre must be finite");
    PathArgs a;
    pd_fill_args(a, kc, T, m, xs, n, mean, V, Z, b, W, Wl, nfeat, ndraws, lo, hi);
    double* pmax = work;                                                  // [draw][workgroup of stage one]
    double* rwork = pmax + (long long)ndraws * a.nblk;
    double* logw = logw_out ? logw_out : rwork + apgp_imp_draw_records_work_len(m, ndraws);
    a.F = logw; a.mask = NULL; a.lnq = lnq; a.idx_offset = 0;
    a.part_u = pmax; a.part_i = NULL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nblk);
    apgp_by_dpad(kc.dpad, [&](auto dp) { path_draws_launch<decltype(dp)::value, true>(ndraws, grid, s, a); });
    APGP_CHECK_LAUNCH();
    return apgp_imp_draw_records(T, m, kc.ndim, centre, ndraws, logw, pmax, a.nblk, rwork, stats_out, s);
}
