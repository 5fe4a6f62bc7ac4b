// Predictive gradients: for each query point t the GP's mu, sigma^2, a utility of them, and the derivatives of all three
// with respect to t (apgp_predict_grad, include/apgp.h).
//
//   k_n = k(t, x_n)            J_nd = d k(t, x_n) / d t_d
//   mu  = k.alpha + mean       dmu_d  = sum_n alpha_n J_nd
//   v   = L^-1 k,  w = L^-T v  (= K^-1 k)
//   var = k(t,t) - |v|^2       dvar_d = d k(t,t) / d t_d - 2 sum_n w_n J_nd
//
// Launches per chunk of points (the chunk is what the scratch holds):
//   pg_kstar_kernel   k_n of a block of points from the packed training stream, one thread per training point
//   inverse route     pg_fwd_kernel: v = W k, a workgroup per 8 rows of W and block of 8 points, a wavefront per pair
//                     of rows; pg_bwd_kernel: w = W^T v, a workgroup per 64 columns, chunk of rows and block of points,
//                     a thread per column, the row-chunk partials kept apart -- each launch reads W once per block of
//                     points, whatever the number of points in the block
//   solve route       pg_solve_kernel: a workgroup per block of 4 points substitutes forward, then backward, against L
//                     in 64-row blocks (a wavefront per row / a thread per column for the off-diagonal part, the
//                     diagonal block in LDS, one wavefront per point)
//   pg_finish_kernel  a workgroup per point and group of 8 dimensions: regenerates k_n and the derivative factors from
//                     the training stream and finishes the 2 D + 2 sums (wavefront butterflies, then the four wavefronts' partials in a fixed
//                     order), the utility and the chain rule.
// A block of points is 8 (4 on the solve route) where that many are left in the chunk and ONE otherwise; a point's
// arithmetic does not depend on the block it travels in or on its neighbours, so a batch returns the bits of the
// single-point calls.  No atomics; every sum has a fixed order.  Everything below the includes is uncontracted: the
// FMAs are the ones written out, the same in every instantiation.
#include "apgp_common.h"
#include "util_value.h"
#include "util_grad.h"

#pragma clang fp contract(off)

#define PG_T 256            // threads per workgroup
#define PG_PB 8             // points per workgroup, inverse route
#define PG_PBS 4            // points per workgroup, solve route (one wavefront per point in the diagonal solves)
#define PG_FR 8             // rows of W per workgroup of the forward product (two per wavefront)
#define PG_NRC 8            // row chunks of the transposed product at most
#define PG_B 64             // rows per block of the substitutions, columns per workgroup of the transposed product
#define PG_PER_POINT (2 + PG_NRC)        // scratch vectors per point: k (v on the solve route), v, PG_NRC partials of w
#define PG_CHUNK_DOUBLES (1ll << 24)     // scratch of a chunk of points (128 MB) unless 8 points need more

struct PgArgs {
    const double* T;
    const double* xs;
    const double* W;
    const double* L;
    double* kbuf;
    double* vbuf;
    double* wbuf;
    const double* vsrc;                  // v as the finish kernel reads it: vbuf (inverse route) or kbuf (solve route)
    double *mu, *var, *u, *dmu, *dvar, *du;
    long long n, ns, ldw, ldl, m0, mc, rc, wstride;
    int nrc, ndim, kind, lin_order, has_box;
    double mean, amp, lin_coef, zeta, ybest;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

// The block of points of workgroup `by` in a chunk of mc points: the full blocks first, then the rest one by one.
template <int PB>
__device__ __forceinline__ void pg_block(long long mc, int by, long long& p0, int& np) {
    const long long nfull = mc / PB;
    if (by < nfull) { p0 = (long long)by * PB; np = PB; }
    else { p0 = nfull * PB + (by - nfull); np = 1; }
}
template <int PB>
static inline unsigned pg_blocks(long long mc) { return (unsigned)(mc / PB + mc % PB); }

// squared-exponential part of k(t, x): the arithmetic of the library's other k* generators
template <int DPAD>
__device__ __forceinline__ double pg_kse(const double* tt, const double* xr, double amp, const double* etab) {
    double q0 = 0.0, q1 = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; d += 2) {
        const double df0 = tt[d] - xr[d], df1 = tt[d + 1] - xr[d + 1];
        q0 = fma(df0, df0, q0);
        q1 = fma(df1, df1, q1);
    }
    return amp * apgp_exp(-(q0 + q1), etab);
}

template <int DPAD>
__device__ __forceinline__ double pg_kval(const double* tt, const double* xr, const PgArgs& a, const double* lw,
                                          const double* etab) {
    double kv = pg_kse<DPAD>(tt, xr, a.amp, etab);
    if (a.lin_coef != 0.0) {
        double ls;
        APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xr[d_] * lw[d_]);
        kv = fma(a.lin_coef, ls, kv);
    }
    return kv;
}

// ---- k* ----------------------------------------------------------------------------------------------------------
template <int DPAD, int NP>
__device__ __forceinline__ void pg_kstar_body(const PgArgs& a, long long p0, double (*tt)[DPAD], double* slw,
                                              const double* etab) {
    constexpr int XS = DPAD + 2;
    const int t = threadIdx.x;
    if (t < DPAD) slw[t] = a.lw[t];
    for (int e = t; e < NP * DPAD; e += PG_T) {
        const int p = e / DPAD, d = e % DPAD;
        tt[p][d] = d < a.ndim ? a.T[(a.m0 + p0 + p) * a.ndim + d] * a.sc[d] : 0.0;
    }
    __syncthreads();
    const long long k = (long long)blockIdx.x * PG_T + t;
    if (k >= a.ns) return;
    if (k < a.n) {
        const double* xr = a.xs + k * XS;
#pragma unroll
        for (int p = 0; p < NP; ++p) a.kbuf[(p0 + p) * a.ns + k] = pg_kval<DPAD>(tt[p], xr, a, slw, etab);
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) a.kbuf[(p0 + p) * a.ns + k] = 0.0;        // the pad the paired loads reach into
    }
}

template <int DPAD>
__global__ __launch_bounds__(PG_T) void pg_kstar_kernel(PgArgs a, int pb) {
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double tt[PG_PB][DPAD];
    __shared__ double slw[DPAD];
    apgp_exp_tab_load(etab);
    long long p0;
    int np;
    if (pb == PG_PB) pg_block<PG_PB>(a.mc, blockIdx.y, p0, np);
    else pg_block<PG_PBS>(a.mc, blockIdx.y, p0, np);
    if (np == PG_PB) pg_kstar_body<DPAD, PG_PB>(a, p0, tt, slw, etab);
    else if (np == PG_PBS) pg_kstar_body<DPAD, PG_PBS>(a, p0, tt, slw, etab);
    else pg_kstar_body<DPAD, 1>(a, p0, tt, slw, etab);
}

// ---- v = W k (inverse route) -----------------------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void pg_fwd_body(const PgArgs& a, long long p0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * PG_FR + 2 * w;
    if (i0 >= a.n) return;
    const bool two = i0 + 1 < a.n;
    const long long i1 = two ? i0 + 1 : i0;
    const double* r0 = a.W + i0 * a.ldw;
    const double* r1 = a.W + i1 * a.ldw;
    double ax[2][NP], ay[2][NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) { ax[0][p] = ay[0][p] = ax[1][p] = ay[1][p] = 0.0; }
    // (k even, k <= i1 <= n - 1: k + 1 <= n stays inside the row, ldw even >= n, and inside the zeroed pad of kbuf)
    for (long long k = 2 * lane; k <= i1; k += 128) {
        const f64x2 a0 = *(const f64x2*)(r0 + k);
        const f64x2 a1 = *(const f64x2*)(r1 + k);
        const double w0x = k <= i0 ? a0.x : 0.0, w0y = k + 1 <= i0 ? a0.y : 0.0;
        const double w1x = a1.x, w1y = k + 1 <= i1 ? a1.y : 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const f64x2 kk = *(const f64x2*)(a.kbuf + (p0 + p) * a.ns + k);
            ax[0][p] = fma(w0x, kk.x, ax[0][p]);
            ay[0][p] = fma(w0y, kk.y, ay[0][p]);
            ax[1][p] = fma(w1x, kk.x, ax[1][p]);
            ay[1][p] = fma(w1y, kk.y, ay[1][p]);
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double s0 = ax[0][p] + ay[0][p], s1 = ax[1][p] + ay[1][p];
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o);
            s1 += __shfl_xor(s1, o);
        }
        if (lane == 0) {
            a.vbuf[(p0 + p) * a.ns + i0] = s0;
            if (two) a.vbuf[(p0 + p) * a.ns + i1] = s1;
        }
    }
}

__global__ __launch_bounds__(PG_T) void pg_fwd_kernel(PgArgs a) {
    long long p0;
    int np;
    pg_block<PG_PB>(a.mc, blockIdx.y, p0, np);
    if (np == PG_PB) pg_fwd_body<PG_PB>(a, p0);
    else pg_fwd_body<1>(a, p0);
}

// ---- w = W^T v (inverse route): the partial of one chunk of rows -----------------------------------------------------
template <int NP>
__device__ __forceinline__ void pg_bwd_body(const PgArgs& a, long long p0, double (*part)[PG_PB][PG_B]) {
    const int c = threadIdx.x & 63, rs = threadIdx.x >> 6;
    const long long c0 = (long long)blockIdx.x * PG_B, k = c0 + c;
    const long long rc = blockIdx.z;
    const long long ibeg = rc * a.rc > c0 ? rc * a.rc : c0;
    const long long iend = (rc + 1) * a.rc < a.n ? (rc + 1) * a.rc : a.n;
    if (ibeg >= iend) return;                     // (the whole workgroup: this chunk lies above the diagonal)
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0;
#pragma unroll 4
    for (long long i = ibeg + rs; i < iend; i += 4) {
        double wv = 0.0;
        if (k <= i) wv = a.W[i * a.ldw + k];      // (k <= i < n)
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = fma(wv, a.vbuf[(p0 + p) * a.ns + i], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) part[rs][p][c] = acc[p];
    __syncthreads();
    for (int p = rs; p < NP; p += 4) {
        const double s = (part[0][p][c] + part[1][p][c]) + (part[2][p][c] + part[3][p][c]);
        a.wbuf[rc * a.wstride + (p0 + p) * a.ns + k] = s;       // k < ns
    }
}

__global__ __launch_bounds__(PG_T) void pg_bwd_kernel(PgArgs a) {
    __shared__ double part[4][PG_PB][PG_B];
    long long p0;
    int np;
    pg_block<PG_PB>(a.mc, blockIdx.y, p0, np);
    if (np == PG_PB) pg_bwd_body<PG_PB>(a, p0, part);
    else pg_bwd_body<1>(a, p0, part);
}

// ---- v = L^-1 k in place in kbuf, w = L^-T v in wbuf (solve route) ----------------------------------------------------
// the 64 x 64 diagonal block at j0 into LDS, the identity where the factor ends
__device__ __forceinline__ void pg_stage_diag(const PgArgs& a, long long j0, int bs, double (*Lb)[PG_B + 1]) {
    for (int e = threadIdx.x; e < PG_B * PG_B; e += PG_T) {
        const int i = e >> 6, k = e & 63;
        double v = (i == k) ? 1.0 : 0.0;
        if (i < bs && k <= i) v = a.L[(j0 + i) * a.ldl + j0 + k];
        Lb[i][k] = v;
    }
}

template <int NP>
__device__ __forceinline__ void pg_solve_body(const PgArgs& a, long long p0, double (*Lb)[PG_B + 1],
                                              double (*part)[PG_PBS][PG_B]) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long n = a.n, nb = (n + PG_B - 1) / PG_B;
    // forward: L v = k
    for (long long jb = 0; jb < nb; ++jb) {
        const long long j0 = jb * PG_B;
        const int bs = (int)((n - j0) < PG_B ? (n - j0) : PG_B);
        for (int row = w; row < bs; row += 4) {               // a wavefront per row against the solved part
            const double* lrow = a.L + (j0 + row) * a.ldl;
            double acc[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = 0.0;
            for (long long k = lane; k < j0; k += 64) {
                const double lv = lrow[k];
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[p] = fma(lv, a.kbuf[(p0 + p) * a.ns + k], acc[p]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double s = acc[p];
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0) a.kbuf[(p0 + p) * a.ns + j0 + row] -= s;      // (rows >= j0: nobody reads them here)
            }
        }
        pg_stage_diag(a, j0, bs, Lb);
        __syncthreads();
        if (w < NP) {
            double* r = a.kbuf + (p0 + w) * a.ns + j0;
            double ri = lane < bs ? r[lane] : 0.0;
            for (int k = 0; k < PG_B; ++k) {
                const double zk = __shfl(ri, k) / Lb[k][k];
                if (lane == k) ri = zk;
                else if (lane > k) ri = fma(-Lb[lane][k], zk, ri);
            }
            if (lane < bs) r[lane] = ri;
        }
        __syncthreads();
    }
    // backward: L^T w = v
    for (long long jb = nb - 1; jb >= 0; --jb) {
        const long long j0 = jb * PG_B;
        const int bs = (int)((n - j0) < PG_B ? (n - j0) : PG_B);
        double acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = 0.0;
        if (lane < bs) {                                       // a thread per column against the solved rows below
            for (long long i = j0 + PG_B + w; i < n; i += 4) {
                const double lv = a.L[i * a.ldl + j0 + lane];
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[p] = fma(lv, a.wbuf[(p0 + p) * a.ns + i], acc[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) part[w][p][lane] = acc[p];
        pg_stage_diag(a, j0, bs, Lb);
        __syncthreads();
        if (w < NP) {
            const double* v = a.kbuf + (p0 + w) * a.ns + j0;
            double* x = a.wbuf + (p0 + w) * a.ns + j0;
            double ri = 0.0;
            if (lane < bs)
                ri = v[lane] - ((part[0][w][lane] + part[1][w][lane]) + (part[2][w][lane] + part[3][w][lane]));
            for (int k = PG_B - 1; k >= 0; --k) {
                const double wk = __shfl(ri, k) / Lb[k][k];
                if (lane == k) ri = wk;
                else if (lane < k) ri = fma(-Lb[k][lane], wk, ri);
            }
            if (lane < bs) x[lane] = ri;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PG_T) void pg_solve_kernel(PgArgs a) {
    __shared__ double Lb[PG_B][PG_B + 1];
    __shared__ double part[4][PG_PBS][PG_B];
    long long p0;
    int np;
    pg_block<PG_PBS>(a.mc, blockIdx.x, p0, np);
    if (np == PG_PBS) pg_solve_body<PG_PBS>(a, p0, Lb, part);
    else pg_solve_body<1>(a, p0, Lb, part);
}

// ---- the 2 D + 2 sums of one point, the utility and the chain rule ---------------------------------------------------
// (blockIdx.y: the group of DG = min(DPAD, 8) dimensions whose derivatives this workgroup sums -- 2 DG + 2 running sums
// a thread keep the kernel clear of spills at D = 32; every group forms mu and sigma^2 by the same operations, group 0
// stores them)
template <int DPAD>
__global__ __launch_bounds__(PG_T) void pg_finish_kernel(PgArgs a) {
    constexpr int XS = DPAD + 2, DG = DPAD < 8 ? DPAD : 8, NS = 2 * DG + 2;
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double tt[DPAD], tr[DPAD], ssc[DPAD], slw[DPAD];
    __shared__ double red[4][NS];
    __shared__ double tot[NS];
    __shared__ double head[4];             // du/dmu, du/dvar, flat, gate
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long pl = blockIdx.x, row = a.m0 + pl;
    const int D = a.ndim, P = a.lin_order, d0 = blockIdx.y * DG;
    apgp_exp_tab_load(etab);
    if (t < DPAD) {
        const double v = t < D ? a.T[row * D + t] : 0.0;
        tr[t] = v;
        tt[t] = t < D ? v * a.sc[t] : 0.0;
        ssc[t] = a.sc[t];
        slw[t] = a.lw[t];
    }
    __syncthreads();
    double smu = 0.0, sq = 0.0, gmu[DG], gvar[DG];
#pragma unroll
    for (int d = 0; d < DG; ++d) { gmu[d] = 0.0; gvar[d] = 0.0; }
    const double* vv = a.vsrc + pl * a.ns;
    const double* wp = a.wbuf + pl * a.ns;
    for (long long k = t; k < a.n; k += PG_T) {
        const double* xr = a.xs + k * XS;
        const double alpha = xr[DPAD];
        const double kse = pg_kse<DPAD>(tt, xr, a.amp, etab);
        double kv = kse;
        if (a.lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, D, P, tt[d_] * xr[d_] * slw[d_]);
            kv = fma(a.lin_coef, ls, kv);
        }
        const double v = vv[k];
        double wk = 0.0;
        for (long long r = k / a.rc; r < a.nrc; ++r) wk += wp[r * a.wstride + k];     // the row chunks at and below k
        smu = fma(kv, alpha, smu);
        sq = fma(v, v, sq);
#pragma unroll
        for (int g = 0; g < DG; ++g) {
            // d k / d t_d: -2 sc_d (tt_d - xs_d) k_se  +  lin_coef P (t_d x_d)^(P-1) x_d,  x_d = xs_d lw_d sc_d
            const int d = d0 + g;
            const double xd = xr[d], sd = ssc[d];
            double J = (-2.0 * sd) * (tt[d] - xd) * kse;
            if (a.lin_coef != 0.0 && P > 0) {
                const double pd = tt[d] * xd * slw[d];
                double q = (double)P;
                for (int e = 1; e < P; ++e) q *= pd;
                J = fma(a.lin_coef * q, xd * slw[d] * sd, J);
            }
            gmu[g] = fma(alpha, J, gmu[g]);
            gvar[g] = fma(wk, J, gvar[g]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        smu += __shfl_xor(smu, o);
        sq += __shfl_xor(sq, o);
    }
#pragma unroll
    for (int d = 0; d < DG; ++d)
        for (int o = 32; o > 0; o >>= 1) {
            gmu[d] += __shfl_xor(gmu[d], o);
            gvar[d] += __shfl_xor(gvar[d], o);
        }
    if (lane == 0) {
        red[w][0] = smu;
        red[w][1] = sq;
#pragma unroll
        for (int d = 0; d < DG; ++d) { red[w][2 + d] = gmu[d]; red[w][2 + DG + d] = gvar[d]; }
    }
    __syncthreads();
    if (t < NS) tot[t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    __syncthreads();
    if (t == 0) {
        int ok = 1;
        for (int d = 0; d < D; ++d) {
            const double v = tr[d];
            if (!isfinite(v) || (a.has_box && !(v >= a.lo[d] && v <= a.hi[d]))) ok = 0;
        }
        // k(t, t), no white noise (george predict): apgp_predict1_host's arithmetic
        double ktl = P == 0 ? (double)D : 0.0;
        if (a.lin_coef != 0.0 && P > 0)
            for (int d = 0; d < D; ++d) {
                const double p = tr[d] * tr[d];
                double qq = p;
                for (int e = 1; e < P; ++e) qq *= p;
                ktl += qq;
            }
        const double ktt = a.lin_coef != 0.0 ? fma(a.lin_coef, ktl, a.amp) : a.amp;
        const double mu = ok ? tot[0] + a.mean : NAN;
        const double var = ok ? ktt - tot[1] : NAN;
        if (a.mu && d0 == 0) a.mu[row] = mu;
        if (a.var && d0 == 0) a.var[row] = var;
        UtilGrad g;
        g.u = INFINITY; g.dmu = 0.0; g.dvar = 0.0; g.flat = 1;
        if (ok && a.kind != APGP_UTIL_NONE) g = util_grad(a.kind, mu, var, a.zeta, a.ybest);
        if (a.u && a.kind != APGP_UTIL_NONE && d0 == 0) a.u[row] = g.u;
        head[0] = g.dmu; head[1] = g.dvar; head[2] = (double)g.flat; head[3] = (double)ok;
    }
    __syncthreads();
    if (t < DG && d0 + t < D) {
        const bool ok = head[3] != 0.0;
        const int d = d0 + t;
        const double dmu = tot[2 + t];
        // d k(t,t) / d t_d = lin_coef 2 P t_d^(2P-1)
        double dktt = 0.0;
        if (a.lin_coef != 0.0 && P > 0) {
            double q = 2.0 * (double)P;
            for (int e = 1; e < 2 * P; ++e) q *= tr[d];
            dktt = a.lin_coef * q;
        }
        const double dvar = fma(-2.0, tot[2 + DG + t], dktt);
        if (a.dmu) a.dmu[row * D + d] = ok ? dmu : NAN;
        if (a.dvar) a.dvar[row * D + d] = ok ? dvar : NAN;
        if (a.du && a.kind != APGP_UTIL_NONE)
            a.du[row * D + d] = head[2] != 0.0 ? 0.0 : fma(head[0], dmu, head[1] * dvar);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// points per chunk: what PG_CHUNK_DOUBLES of scratch hold, a multiple of 8, at least 8 and no more than the call has
static int64_t pg_chunk(int64_t m, int64_t n) {
    const int64_t ns = apgp_round_up(n, 64);
    int64_t ch = PG_CHUNK_DOUBLES / (PG_PER_POINT * ns) / PG_PB * PG_PB;
    if (ch > 4096) ch = 4096;
    if (ch < PG_PB) ch = PG_PB;
    const int64_t mr = apgp_round_up(m, PG_PB);
    return ch < mr ? ch : mr;
}

extern "C" int64_t apgp_predict_grad_work_len(int64_t m, int64_t n) {
    if (m < 1 || m > APGP_MAX_M || n < 1 || n > APGP_MAX_N) return -1;
    return pg_chunk(m, n) * PG_PER_POINT * apgp_round_up(n, 64);
}

template <int DPAD>
static void pg_launch(hipStream_t s, const PgArgs& a, bool inverse) {
    const unsigned gy = inverse ? pg_blocks<PG_PB>(a.mc) : pg_blocks<PG_PBS>(a.mc);
    hipLaunchKernelGGL((pg_kstar_kernel<DPAD>), dim3((unsigned)((a.ns + PG_T - 1) / PG_T), gy), dim3(PG_T), 0, s, a,
                       inverse ? PG_PB : PG_PBS);
    if (inverse) {
        hipLaunchKernelGGL(pg_fwd_kernel, dim3((unsigned)((a.n + PG_FR - 1) / PG_FR), gy), dim3(PG_T), 0, s, a);
        hipLaunchKernelGGL(pg_bwd_kernel, dim3((unsigned)(a.ns / PG_B), gy, (unsigned)a.nrc), dim3(PG_T), 0, s, a);
    } else {
        hipLaunchKernelGGL(pg_solve_kernel, dim3(gy), dim3(PG_T), 0, s, a);
    }
    hipLaunchKernelGGL((pg_finish_kernel<DPAD>), dim3((unsigned)a.mc, DPAD < 8 ? 1 : DPAD / 8), dim3(PG_T), 0, s, a);
}

extern "C" int apgp_predict_grad(const double* T, int64_t m, const double* xs, int64_t n,
                                 const apgp_kernel_t* kern, double mean,
                                 const double* winv, int64_t ldw, const double* L, int64_t ldl,
                                 int32_t kind, const double* lo, const double* hi, double zeta, double ybest,
                                 double* mu, double* var, double* u, double* dmu, double* dvar, double* du,
                                 double* work, void* stream) {
    APGP_CHECK_ARG(m >= 0 && m <= APGP_MAX_M, "0 <= m <= APGP_MAX_M required");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG(xs && kern, "null pointer");
    APGP_CHECK_ARG((winv && ldw >= n && ldw % 2 == 0 && ((uintptr_t)winv & 15) == 0) || (!winv && L && ldl >= n),
                   "the dense inverse (16-byte aligned, even ldw >= n) or the factor (ldl >= n) is required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi go together");
    APGP_CHECK_ARG(kind == APGP_UTIL_AGP || kind == APGP_UTIL_BAPE || kind == APGP_UTIL_JONES ||
                   kind == APGP_UTIL_NONE || kind == APGP_UTIL_NEG_MEAN, "kind: AGP, BAPE, JONES, NONE or NEG_MEAN");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    if (m == 0) return 0;
    APGP_CHECK_ARG(T && work, "null pointer");
    APGP_CHECK_ARG(((uintptr_t)work & 15) == 0, "work must be 16-byte aligned");
    const bool inverse = winv != NULL;
    const int64_t ns = apgp_round_up(n, 64), ch = pg_chunk(m, n);
    PgArgs a;
    a.T = T; a.xs = xs; a.W = winv; a.L = inverse ? NULL : L;
    a.kbuf = work; a.vbuf = work + ch * ns; a.wbuf = work + 2 * ch * ns;
    a.vsrc = inverse ? a.vbuf : a.kbuf;
    a.mu = mu; a.var = var; a.u = u; a.dmu = dmu; a.dvar = dvar; a.du = du;
    a.n = n; a.ns = ns; a.ldw = inverse ? ldw : 0; a.ldl = inverse ? 0 : ldl;
    a.wstride = ch * ns;
    if (inverse) {
        // rows per chunk of the transposed product: a multiple of 64, at least 512, at most PG_NRC chunks
        a.rc = apgp_round_up((n + PG_NRC - 1) / PG_NRC, 64);
        if (a.rc < 512) a.rc = 512;
        a.nrc = (int)((n + a.rc - 1) / a.rc);
    } else {
        a.rc = ns;
        a.nrc = 1;
    }
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    a.kind = kind; a.mean = mean; a.zeta = zeta; a.ybest = ybest;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t m0 = 0; m0 < m; m0 += ch) {
        a.m0 = m0;
        a.mc = (m - m0) < ch ? (m - m0) : ch;
        apgp_by_dpad(kc.dpad, [&](auto dp) { pg_launch<decltype(dp)::value>(s, a, inverse); });
        APGP_CHECK_LAUNCH();
    }
    return 0;
}
