// Integrated acquisition (apgp_acquire_integrated; DESIGN.md "Integrated acquisition").  The expected integrated
// variance of the posterior estimate exp(f) after one more evaluation at t, up to terms that do not depend on t:
//   u(t) = -log sum_j exp(a_j + c_j(t)^2 / s(t)),   c_j(t) = k(t, r_j) - sum_n k(t, x_n) B[n, j],   s(t) = var(t) + diag_add
// over J = nref reference points r_j (B = K^-1 k(X, R), a_j: log-weights; both inputs).  The sum over n has the shape
// (candidates x generated values).(values x columns), as the data term of the posterior function draws (pathdraw.hip):
// a kernel value k(t, x_n) is generated once per candidate and column pass and contracted with the columns of its row.
// A workgroup owns IV_THREADS candidates and walks the reference columns in passes of SPAD columns; per pass the training
// rows and their B columns are staged through LDS in tiles of IV_ROWS rows, the sums of the pass are handed to one thread
// per candidate, which adds k(t, r_j) (the same operation sequence as every other k value), stores c_j and feeds
// e_j = a_j + c_j^2 / s into a running (max, sum) pair -- one element at a time, j ascending, so that the result is a
// function of the sequence of finite e_j alone: a column with a_j = -inf changes no bit.  u = -(max + log(sum)).
// integrated_mma_kernel: the contraction on the matrix cores (v_mfma_f64_4x4x4_4b through the fragments of csrc/mma16.h,
// as path_draws_mma_kernel), 64 candidates x up to 64 columns per wavefront, for D padded to at most 8.
// integrated_kernel: one thread per candidate and 16 columns per pass on the vector units, for D padded up to 16 (the
// entry point refuses more dimensions than APGP_INTEGRATED_MAX_DIM).
// No atomics; every sum has a fixed order; a row's results do not depend on the other rows of the call.
#include "apgp_common.h"

// every product and sum below rounds where it is written (the explicit fma()s stay): a kernel value has the bits of
// apgp_gram_value, and tests/integrated_ref.py restates the vector form operation by operation
#pragma clang fp contract(off)

#define IV_THREADS 256
#define IV_ROWS 64         // training rows per LDS tile (divides the packed stream's 512-row padding)
#define IV_NW (IV_THREADS / 64)

struct IntegArgs {
    const double* T;
    const double* xs;
    const double* R;
    const double* B;
    const double* a;
    const double* var;
    double* C;
    double* u;
    const unsigned char* mask;
    double* part_u;
    long long* part_i;
    long long m, idx_offset, n, ldc;
    int ndim, nref, has_box, lin_order;
    double amp, lin_coef, diag_add;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

// as best_merge of sweep.hip: NaN and +inf never win; ties resolve to the lowest global index
__device__ __forceinline__ void iv_best_merge(double& bu, long long& bi, double u, long long i) {
    if (i >= 0 && u < INFINITY && (u < bu || (u == bu && (bi < 0 || i < bi)))) { bu = u; bi = i; }
}

// This thread's candidate: scaled coordinates (from the clamped row `lrow`), s = var + diag_add, and the gate (box,
// mask, NaN coordinate, s not positive or not finite).
template <int DPAD>
__device__ __forceinline__ bool iv_row_setup(const IntegArgs& a, long long lrow, double (&tw)[DPAD], double& s) {
    bool adm = !(a.mask && a.mask[lrow] == 0);
#pragma unroll
    for (int d = 0; d < DPAD; ++d) {
        const double x = d < a.ndim ? a.T[lrow * a.ndim + d] : 0.0;
        if (d < a.ndim && a.has_box && !(x >= a.lo[d] && x <= a.hi[d])) adm = false;
        if (x != x) adm = false;
        tw[d] = d < a.ndim ? x * a.sc[d] : 0.0;
    }
    s = a.var[lrow] + a.diag_add;
    if (!(s > 0.0 && s < INFINITY)) adm = false;
    return adm;
}

// exponents of four kernel values: -(sum_d (t_d - x_d)^2) in the two-lane order of apgp_gram_value
template <int DPAD>
__device__ __forceinline__ double iv_exponent(const double (&tt)[DPAD], const double* xr) {
    double s = 0.0, s3 = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; d += 2) {
        const double df0 = tt[d] - xr[d];
        const double df1 = tt[d + 1] - xr[d + 1];
        s = fma(df0, df0, s);
        s3 = fma(df1, df1, s3);
    }
    return -(s + s3);
}

template <int DPAD>
__device__ __forceinline__ double iv_finish_value(const IntegArgs& a, const double (&tt)[DPAD], const double* xr, double e) {
    double k = a.amp * e;
    if (a.lin_coef != 0.0) {
        double ls;
        APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, (tt[d_] * xr[d_]) * a.lw[d_]);
        k = fma(a.lin_coef, ls, k);
    }
    return k;
}

// Stage the scaled reference points and log-weights of the columns j0 .. j0 + SPAD - 1 (zeros and -inf past nref), and
// tile `r0` of the training rows with those columns of B (zeros past n and past nref).  Call from every thread, between
// barriers.
template <int DPAD, int SPAD>
__device__ __forceinline__ void iv_stage_refs(const IntegArgs& a, int j0, double* rt, double* at) {
    const int tid = threadIdx.x;
    for (int c = tid; c < SPAD; c += IV_THREADS) {                   // (a thread per column: sc is indexed statically)
        const bool in = j0 + c < a.nref;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            const double r = a.R[in && d < a.ndim ? (long long)(j0 + c) * a.ndim + d : 0];
            rt[c * DPAD + d] = in && d < a.ndim ? r * a.sc[d] : 0.0;
        }
        const double w = a.a[in ? j0 + c : 0];
        at[c] = in ? w : -INFINITY;
    }
}

template <int DPAD, int SPAD>
__device__ __forceinline__ void iv_stage_train(const IntegArgs& a, long long r0, int j0, double* xt, double* wt) {
    constexpr int XS = DPAD + 2;                 // packed stream row: scaled x | alpha | 0 (the last two are not read)
    const int tid = threadIdx.x;
    for (int e = tid; e < IV_ROWS * DPAD / 2; e += IV_THREADS) {     // (rows < ntile * IV_ROWS <= npad: inside the stream)
        const int r = e / (DPAD / 2), p = e - r * (DPAD / 2);
        *(f64x2*)(xt + r * DPAD + 2 * p) = *(const f64x2*)(a.xs + (r0 + r) * XS + 2 * p);
    }
    for (int e = tid; e < IV_ROWS * SPAD; e += IV_THREADS) {
        const int r = e / SPAD, c = e - r * SPAD;
        const bool in = r0 + r < a.n && j0 + c < a.nref;
        const double v = a.B[in ? (r0 + r) * a.nref + j0 + c : 0];
        wt[e] = in ? v : 0.0;                                        // 0 on the padding rows and columns
    }
}

// Four columns of this thread's candidate, `f` their sums over n: c_j = k(t, r_j) - f_j, the C store, and the running
// (max, sum) of e_j = a_j + c_j^2 / s, one element at a time.  rt / at: the staged reference points and log-weights of
// these four columns; j0: the global index of the first.  Columns past nref carry a = -inf and are skipped as any other
// -inf column is.
template <int DPAD>
__device__ __forceinline__ void iv_columns4(const IntegArgs& a, const double (&tw)[DPAD], const double (&f)[4], int j0,
                                            const double* rt, const double* at, const double* etab, long long row,
                                            bool live, bool adm, double s, double& mx, double& sm) {
    double ex[4], kv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ex[q] = iv_exponent<DPAD>(tw, rt + q * DPAD);
    apgp_exp4(ex, kv, etab);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double c = iv_finish_value<DPAD>(a, tw, rt + q * DPAD, kv[q]) - f[q];
        if (a.C && live && j0 + q < a.nref) a.C[(long long)(j0 + q) * a.ldc + row] = adm ? c : NAN;
        const double e = at[q] + (c * c) / s;
        if (e != -INFINITY) {
            const double d = e - mx;                                 // (+inf on the first finite element: mx = -inf)
            const bool gt = d > 0.0;
            const double x = apgp_exp(gt ? -d : d, etab);
            sm = gt ? fma(sm, x, 1.0) : sm + x;
            mx = gt ? e : mx;
            if (e != e) sm = e;                                      // (the clamp of apgp_exp would swallow a NaN)
        }
    }
}

// u of this thread's candidate, its store, and the workgroup's arg-min partial (call from every thread)
__device__ __forceinline__ void iv_finish(const IntegArgs& a, long long row, bool live, bool adm, double mx, double sm,
                                          double* su, long long* si) {
    const int tid = threadIdx.x;
    const double u = adm ? -(mx + log(sm)) : INFINITY;               // (no finite column: -(-inf + log 0) = +inf)
    if (live && a.u) a.u[row] = u;
    double bu = INFINITY;
    long long bi = -1;
    if (live) iv_best_merge(bu, bi, u, a.idx_offset + row);
    for (int o = 32; o > 0; o >>= 1) {
        const double ou = __shfl_xor(bu, o);
        const long long oi = __shfl_xor(bi, o);
        iv_best_merge(bu, bi, ou, oi);
    }
    if ((tid & 63) == 0) { su[tid >> 6] = bu; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < IV_NW; ++w) iv_best_merge(bu, bi, su[w], si[w]);
        a.part_u[blockIdx.x] = bu;
        a.part_i[blockIdx.x] = bi;
    }
}

// One thread per candidate, 16 columns per pass, four kernel values per step (four independent chains through
// apgp_exp4), each contracted with the 16 staged weights of its row: one fma chain over n per column.
template <int DPAD>
__global__ __launch_bounds__(IV_THREADS) void integrated_kernel(IntegArgs a) {
    constexpr int SPAD = 16;
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double xt[IV_ROWS * DPAD];
    __shared__ __attribute__((aligned(16))) double wt[IV_ROWS * SPAD];
    __shared__ double rt[SPAD * DPAD];
    __shared__ double at[SPAD];
    __shared__ double su[IV_NW];
    __shared__ long long si[IV_NW];
    apgp_exp_tab_load(etab);
    const long long row = (long long)blockIdx.x * IV_THREADS + threadIdx.x;
    const bool live = row < a.m;
    const long long lrow = live ? row : a.m - 1;                     // loads are clamped, stores are masked
    double tw[DPAD], s;
    const bool adm = iv_row_setup<DPAD>(a, lrow, tw, s);
    double mx = -INFINITY, sm = 0.0;
    const long long ntile = (a.n + IV_ROWS - 1) / IV_ROWS;
    for (int j0 = 0; j0 < a.nref; j0 += SPAD) {
        double acc[SPAD];
#pragma unroll
        for (int c = 0; c < SPAD; ++c) acc[c] = 0.0;
        for (long long ti = 0; ti < ntile; ++ti) {
            __syncthreads();                     // the previous tile (and the previous pass's rt / at) has been consumed
            iv_stage_train<DPAD, SPAD>(a, ti * IV_ROWS, j0, xt, wt);
            if (ti == 0) iv_stage_refs<DPAD, SPAD>(a, j0, rt, at);
            __syncthreads();
            for (int r = 0; r < IV_ROWS; r += 4) {
                double ex[4], kv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) ex[q] = iv_exponent<DPAD>(tw, xt + (r + q) * DPAD);
                apgp_exp4(ex, kv, etab);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double k = iv_finish_value<DPAD>(a, tw, xt + (r + q) * DPAD, kv[q]);
#pragma unroll
                    for (int c = 0; c < SPAD; ++c) acc[c] = fma(k, wt[(r + q) * SPAD + c], acc[c]);
                }
            }
        }
#pragma unroll
        for (int c4 = 0; c4 < SPAD; c4 += 4) {
            if (j0 + c4 >= a.nref) break;        // (the same for every thread)
            const double f[4] = {acc[c4], acc[c4 + 1], acc[c4 + 2], acc[c4 + 3]};
            iv_columns4<DPAD>(a, tw, f, j0 + c4, rt + c4 * DPAD, at + c4, etab, row, live, adm, s, mx, sm);
        }
    }
    iv_finish(a, row, live, adm, mx, sm, su, si);
}

// The same sums with the contraction on the matrix cores, in the layout of path_draws_mma_kernel: a wavefront owns 64
// candidates as four blocks of 16; lane l generates, for tile row r + (l >> 4), the values of the four candidates
// 16 b + (l & 15) -- the A fragments of the four blocks -- and reads one weight per column block and rotation.  With
// NCB = 4 column blocks a generated value feeds 16 matrix instructions (8 in the draws' kernel): the exponentials per
// flop halve.  The sums come back to one thread per candidate through a 64 x 16 tile per wavefront, a column block at a
// time; that tile shares its LDS with the B tile, which nobody reads any more by then.  D padded to at most 8.
template <int DPAD, int NCB>
__global__ __launch_bounds__(IV_THREADS) void integrated_mma_kernel(IntegArgs a) {
    constexpr int SPAD = 16 * NCB;
    constexpr int FT = 17;                                               // row stride of the hand-back tile
    constexpr int WT_LEN = IV_ROWS * SPAD > IV_NW * 64 * FT ? IV_ROWS * SPAD : IV_NW * 64 * FT;
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double xt[IV_ROWS * DPAD];
    __shared__ __attribute__((aligned(16))) double wt[WT_LEN];           // the B tile, then the hand-back tiles
    __shared__ double rt[SPAD * DPAD];
    __shared__ double at[SPAD];
    __shared__ double su[IV_NW];
    __shared__ long long si[IV_NW];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const long long base = (long long)blockIdx.x * IV_THREADS + wave * 64;
    double tt[4][DPAD];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const long long c = base + 16 * b + li;
        const long long lc = c < a.m ? c : a.m - 1;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) tt[b][d] = d < a.ndim ? a.T[lc * a.ndim + d] * a.sc[d] : 0.0;
    }
    const long long row = (long long)blockIdx.x * IV_THREADS + tid;
    const bool live = row < a.m;
    const long long lrow = live ? row : a.m - 1;
    double mx = -INFINITY, sm = 0.0;
    int bcol[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bcol[r] = (li - 4 * r) & 15;
    bool adm = false;
    double* fw = wt + wave * 64 * FT;
    const int frow = 4 * ((lane >> 2) & 3) + (lane >> 4);
    const long long ntile = (a.n + IV_ROWS - 1) / IV_ROWS;

    for (int j0 = 0; j0 < a.nref; j0 += SPAD) {
        double acc[4][NCB][4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[b][c][r] = 0.0;
        for (long long ti = 0; ti < ntile; ++ti) {
            __syncthreads();                     // the previous tile (or the previous pass's hand-back) has been consumed
            iv_stage_train<DPAD, SPAD>(a, ti * IV_ROWS, j0, xt, wt);
            if (ti == 0) iv_stage_refs<DPAD, SPAD>(a, j0, rt, at);
            __syncthreads();
#pragma unroll 1
            for (int r = 0; r < IV_ROWS; r += 4) {
                const double* xr = xt + (r + kq) * DPAD;
                double ex[4], kv[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) ex[b] = iv_exponent<DPAD>(tt[b], xr);
                apgp_exp4(ex, kv, etab);
#pragma unroll
                for (int b = 0; b < 4; ++b) kv[b] = iv_finish_value<DPAD>(a, tt[b], xr, kv[b]);
                double bf[NCB][4];
#pragma unroll
                for (int c = 0; c < NCB; ++c)
#pragma unroll
                    for (int q = 0; q < 4; ++q) bf[c][q] = wt[(r + kq) * SPAD + 16 * c + bcol[q]];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int c = 0; c < NCB; ++c)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[b][c][q] = __builtin_amdgcn_mfma_f64_4x4x4f64(kv[b], bf[c][q], acc[b][c][q], 0, 0, 0);
            }
        }
        // back to one thread per candidate: acc[b][c][r] of lane l is row 4 ((l >> 2) & 3) + (l >> 4) of block b and
        // column 4 ((((l >> 2) & 3) - r) & 3) + (l & 3) of column block c (csrc/mma16.h)
        // (this thread's own candidate is loaded here, once per pass, not held across the contraction: its registers
        // are what keeps the 64-column form of D = 8 out of scratch)
        double tw[DPAD], s;
        adm = iv_row_setup<DPAD>(a, lrow, tw, s);
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            if (j0 + 16 * c >= a.nref) break;    // (the same for every thread)
            __syncthreads();                     // the B tile / the previous column block has been read
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    fw[(16 * b + frow) * FT + 4 * ((((lane >> 2) & 3) - r) & 3) + (lane & 3)] = acc[b][c][r];
            __syncthreads();
#pragma unroll 1
            for (int c4 = 16 * c; c4 < 16 * c + 16; c4 += 4) {
                if (j0 + c4 >= a.nref) break;    // (the same for every thread)
                const double* fr = fw + lane * FT + (c4 - 16 * c);
                const double f[4] = {fr[0], fr[1], fr[2], fr[3]};
                iv_columns4<DPAD>(a, tw, f, j0 + c4, rt + c4 * DPAD, at + c4, etab, row, live, adm, s, mx, sm);
            }
        }
    }
    iv_finish(a, row, live, adm, mx, sm, su, si);
}

// final arg-min over the per-workgroup partials (one workgroup; as argmin_draws_kernel of pathdraw.hip for one draw)
__global__ __launch_bounds__(256) void integrated_argmin_kernel(const double* part_u, const long long* part_i,
                                                                long long nblk, apgp_best_t* best) {
    __shared__ double su[4];
    __shared__ long long si[4];
    double bu = INFINITY;
    long long bi = -1;
    for (long long p = threadIdx.x; p < nblk; p += 256) iv_best_merge(bu, bi, part_u[p], part_i[p]);
    for (int o = 32; o > 0; o >>= 1) {
        const double ou = __shfl_xor(bu, o);
        const long long oi = __shfl_xor(bi, o);
        iv_best_merge(bu, bi, ou, oi);
    }
    if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = bu; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) iv_best_merge(bu, bi, su[i], si[i]);
        best->u = bu;
        best->index = bi;
    }
}

// Scratch: the arg-min partial (value, index) of every workgroup.
extern "C" int64_t apgp_integrated_work_len(int64_t m, int32_t nref) {
    if (m < 0 || m > APGP_MAX_M || nref < 1 || nref > APGP_MAX_REFS) return -1;
    return 2 * ((m + IV_THREADS - 1) / IV_THREADS);
}

// 0: the matrix-core contraction where it exists (D padded to at most 8), 1: the vector contraction always
static int g_iv_mode = 0;
extern "C" int apgp_integrated_mode(int mode) {
    const int was = g_iv_mode;
    if (mode > 1) return -1;
    if (mode >= 0) g_iv_mode = mode;
    return was;
}

template <int DPAD>
static void integrated_launch(int nref, dim3 grid, hipStream_t s, const IntegArgs& a) {
    const dim3 block(IV_THREADS);
    if constexpr (DPAD <= 8) {
        if (g_iv_mode == 0) {
            if (nref <= 16) hipLaunchKernelGGL((integrated_mma_kernel<DPAD, 1>), grid, block, 0, s, a);
            else if (nref <= 32) hipLaunchKernelGGL((integrated_mma_kernel<DPAD, 2>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((integrated_mma_kernel<DPAD, 4>), grid, block, 0, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((integrated_kernel<DPAD>), grid, block, 0, s, a);
}

extern "C" int apgp_acquire_integrated(const double* T, int64_t m, int64_t idx_offset, const double* xs, int64_t n,
                                       const apgp_kernel_t* kern, const double* R, int32_t nref, const double* B,
                                       const double* a_w, const double* var, const double* lo, const double* hi,
                                       const uint8_t* mask, double* C, int64_t ldc, double* u, void* part,
                                       apgp_best_t* best, void* stream) {
    APGP_CHECK_ARG(T && xs && kern && R && B && a_w && var && part && best, "null pointer");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M, "1 <= m <= APGP_MAX_M required");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG((m + IV_THREADS - 1) / IV_THREADS < (1ll << 31), "m too large for one grid");
    APGP_CHECK_ARG(nref >= 1 && nref <= APGP_MAX_REFS, "1 <= nref <= APGP_MAX_REFS required");
    APGP_CHECK_ARG(C == NULL || ldc >= m, "ldc >= m required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(kc.ndim <= APGP_INTEGRATED_MAX_DIM, "ndim <= APGP_INTEGRATED_MAX_DIM required");
    IntegArgs a;
    a.T = T; a.xs = xs; a.R = R; a.B = B; a.a = a_w; a.var = var; a.C = C; a.u = u; a.mask = mask;
    const long long nblk = (m + IV_THREADS - 1) / IV_THREADS;
    a.part_u = (double*)part;
    a.part_i = (long long*)((double*)part + nblk);
    a.m = m; a.idx_offset = idx_offset; a.n = n; a.ldc = ldc; a.nref = nref; a.diag_add = kc.diag_add;
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk);
    switch (kc.dpad) {                            // (not apgp_by_dpad: no instantiation for D padded to 32)
        case 2: integrated_launch<2>(nref, grid, s, a); break;
        case 4: integrated_launch<4>(nref, grid, s, a); break;
        case 8: integrated_launch<8>(nref, grid, s, a); break;
        default: integrated_launch<16>(nref, grid, s, a); break;
    }
    hipLaunchKernelGGL(integrated_argmin_kernel, dim3(1), dim3(256), 0, s, a.part_u, a.part_i, nblk, best);
    APGP_CHECK_LAUNCH();
    return 0;
}
