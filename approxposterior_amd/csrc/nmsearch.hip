// Restarted Nelder-Mead point search on the device: the default design-point search of
// ApproxPosterior.findNextPoint (utility.minimizeObjective, utility.py:253-372: nRestarts SciPy adaptive Nelder-Mead runs
// over a scalar utility) with every restart in ONE launch.
//
// Layout: one workgroup (256 threads) per restart; workgroups never communicate.  The simplex (D + 1 vertices of D
// coordinates), its values and the vertex order live in LDS.  Every thread runs the same control flow: each decision
// reads values that a barrier has published, and is taken into a register before any thread writes the state it read.
// Coordinate d of every simplex operation is formed by thread d; thread 0 sorts and tests convergence.  Each evaluation
// is done by the whole workgroup:
//   FORM 0  the dense inverse W = L^-1, n <= 256: the body of pred1_small_kernel (pred1_body.h) -> the bits of
//           apgp_predict1_host at the same point;
//   FORM 1  the dense inverse, any n: k* into the restart's slice of `work`, then a wavefront per row of W;
//   FORM 2  the factor L: k* into `work`, a blocked forward substitution in the workgroup (64-row blocks: a 4-thread
//           dot product per row against the solved part, then the 64 x 64 diagonal block staged in LDS and solved by
//           wavefront 0 with shuffles).
//
// The simplex arithmetic restates SciPy 1.15's _minimize_neldermead (bounds=None) operation by operation and must not be
// contracted into FMAs (a NumPy replay must reproduce every point): it lies under `fp contract(off)` below; the shared
// evaluation bodies (pred1_body.h, util_value.h) are included above the pragma and keep the library's defaults.
// Ties in the sort are broken by the vertex's previous position (a stable sort), NaN sorts last.
#include "apgp_common.h"
#include "pred1_body.h"
#include "util_value.h"

#pragma clang fp contract(off)

#define NM_T 256                       // threads per workgroup (one restart)
#define NM_V (APGP_MAX_DIM + 1)        // simplex vertices at most
#define NM_B 64                        // rows per block of the triangular solve

struct NmArgs {
    const double* starts;
    const double* xs;
    const double* W;
    const double* L;
    double* work;
    double* x_out;
    double* f_out;
    int* stats;
    double* trace;
    int* steps;
    long long n, ldw, ldl, wstride;
    int ndim, kind, maxiter, maxfev, lin_order, has_box;
    double mean, amp, lin_coef, zeta, ybest, xatol, fatol, rho, chi, psi, sigma;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

struct NmShared {
    double etab[APGP_EXP_TAB_N];
    double red[4], red2[4];
    __attribute__((aligned(16))) double ks[256];
    double vs[256];
    double sim[NM_V][APGP_MAX_DIM];
    double fsim[NM_V];
    double xbar[APGP_MAX_DIM], xr[APGP_MAX_DIM], xt[APGP_MAX_DIM], tt[APGP_MAX_DIM];
    double f;
    int ord[NM_V];
    int gate, conv;
};

// k(t, t) of the point in s.xt (no white noise, george predict): apgp_predict1_host's host arithmetic.
__device__ double nm_ktt(const NmArgs& a, const NmShared& s) {
    double ktl = a.lin_order == 0 ? (double)a.ndim : 0.0;
    if (a.lin_coef != 0.0 && a.lin_order > 0) {
        for (int d = 0; d < a.ndim; ++d) {
            const double v = s.xt[d];
            double p = v * v, qq = p;
            for (int e = 1; e < a.lin_order; ++e) qq *= p;
            ktl += qq;
        }
    }
    return a.lin_coef != 0.0 ? fma(a.lin_coef, ktl, a.amp) : a.amp;
}

// k* into kst (n doubles, global), k*.alpha partials into s.red: one thread per training point, strided.
template <int DPAD>
__device__ void nm_kstar(const NmArgs& a, NmShared& s, double* kst) {
    constexpr int XS = DPAD + 2;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double contrib = 0.0;
    for (long long k = t; k < a.n; k += NM_T) {
        const double* xr = a.xs + k * XS;
        double q0 = 0.0, q1 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            const double df0 = s.tt[d] - xr[d], df1 = s.tt[d + 1] - xr[d + 1];
            q0 = fma(df0, df0, q0);
            q1 = fma(df1, df1, q1);
        }
        double kv = a.amp * apgp_exp(-(q0 + q1), s.etab);
        if (a.lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, s.tt[d_] * xr[d_] * a.lw[d_]);
            kv = fma(a.lin_coef, ls, kv);
        }
        kst[k] = kv;
        contrib = fma(kv, xr[DPAD], contrib);
    }
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o);
    if (lane == 0) s.red[w] = contrib;
    __syncthreads();
}

// sum_i (W k*)_i^2 partials into s.red2: a wavefront per row of the dense inverse.
__device__ void nm_quad_inverse(const NmArgs& a, NmShared& s, const double* kst) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double qw = 0.0;
    for (long long i = w; i < a.n; i += 4) {
        const double* wr = a.W + i * a.ldw;
        double s0 = 0.0;
        for (long long k = lane; k <= i; k += 64) s0 = fma(wr[k], kst[k], s0);
        for (int o = 32; o > 0; o >>= 1) s0 += __shfl_xor(s0, o);
        qw = fma(s0, s0, qw);
    }
    if (lane == 0) s.red2[w] = qw;
    __syncthreads();
}

// |L^-1 k*|^2 into s.red2[0] (s.red2[1..3] = 0): blocked forward substitution, r = k* in place.
__device__ void nm_quad_solve(const NmArgs& a, NmShared& s, double* r) {
    __shared__ double Lb[NM_B][NM_B + 1];
    const int t = threadIdx.x, lane = t & 63;
    const long long n = a.n;
    const long long nb = (n + NM_B - 1) / NM_B;
    double qacc = 0.0;
    for (long long jb = 0; jb < nb; ++jb) {
        const long long j0 = jb * NM_B;
        const int bs = (int)((n - j0) < NM_B ? (n - j0) : NM_B);
        const int row = t >> 2, part = t & 3;              // 64 rows x 4 threads
        double acc = 0.0;
        if (row < bs) {
            const double* lrow = a.L + (j0 + row) * a.ldl;
            for (long long k = part; k < j0; k += 4) acc = fma(lrow[k], r[k], acc);
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        for (int e = t; e < NM_B * NM_B; e += NM_T) {
            const int i = e >> 6, k = e & 63;
            double v = (i == k) ? 1.0 : 0.0;
            if (i < bs && k <= i) v = a.L[(j0 + i) * a.ldl + j0 + k];
            Lb[i][k] = v;
        }
        if (part == 0 && row < bs) r[j0 + row] -= acc;     // (rows >= j0: nobody reads them in this phase)
        __syncthreads();
        if (t < 64) {
            double ri = lane < bs ? r[j0 + lane] : 0.0;
            for (int k = 0; k < NM_B; ++k) {
                const double zk = __shfl(ri, k) / Lb[k][k];
                if (lane == k) ri = zk;
                else if (lane > k) ri = fma(-Lb[lane][k], zk, ri);
            }
            if (lane < bs) {
                r[j0 + lane] = ri;
                qacc = fma(ri, ri, qacc);
            }
        }
        __syncthreads();
    }
    if (t < 64) {
        for (int o = 32; o > 0; o >>= 1) qacc += __shfl_xor(qacc, o);
        if (t == 0) { s.red2[0] = qacc; s.red2[1] = 0.0; s.red2[2] = 0.0; s.red2[3] = 0.0; }
    }
    __syncthreads();
}

// The objective at the point in s.xt (written by threads d < ndim before the call); every thread gets u.  Record `rec`
// of the trace is written when a trace is kept.
template <int DPAD, int FORM>
__device__ double nm_eval(const NmArgs& a, NmShared& s, double* trace, int rec) {
    const int t = threadIdx.x;
    const int D = a.ndim;
    __syncthreads();                                           // s.xt complete
    if (t < DPAD) s.tt[t] = t < D ? s.xt[t] * a.sc[t] : 0.0;
    if (t == 0) {
        int ok = 1;
        for (int d = 0; d < D; ++d) {
            const double v = s.xt[d];
            if (!isfinite(v) || (a.has_box && !(v >= a.lo[d] && v <= a.hi[d]))) ok = 0;
        }
        s.gate = ok;
    }
    __syncthreads();
    double mu = NAN, var = NAN, u = INFINITY;
    if (s.gate) {
        if constexpr (FORM == 0) {
            apgp_pred1_small_body<DPAD>(a.xs, a.n, s.tt, a.lw, a.amp, a.lin_coef, a.ndim, a.lin_order, a.W, a.ldw,
                                        s.etab, s.red, s.red2, s.ks, s.vs);
        } else {
            double* kst = a.work + (long long)blockIdx.x * a.wstride;
            nm_kstar<DPAD>(a, s, kst);
            if constexpr (FORM == 1) nm_quad_inverse(a, s, kst);
            else nm_quad_solve(a, s, kst);
        }
        if (t == 0) {
            // (the epilogue of pred1_small_kernel: same order of the partial sums)
            double q = 0.0;
            for (int i = 0; i < 4; ++i) q += s.red2[i];
            mu = 0.0;
            mu += (s.red[0] + s.red[1]) + (s.red[2] + s.red[3]);
            mu += a.mean;
            var = nm_ktt(a, s) - q;
            if (a.kind == APGP_UTIL_NEG_MEAN) u = isfinite(mu) ? -mu : INFINITY;
            else u = util_value(a.kind, mu, var, a.zeta, a.ybest);
        }
    }
    if (trace) {
        double* tr = trace + (long long)rec * (D + 3);
        if (t < D) tr[t] = s.xt[t];
        if (t == 0) { tr[D] = mu; tr[D + 1] = var; tr[D + 2] = u; }
    }
    if (t == 0) s.f = u;
    __syncthreads();
    return s.f;
}

// a before b in np.argsort's order: NaN last
__device__ __forceinline__ bool nm_before(double a, double b) { return isnan(b) ? !isnan(a) : a < b; }

// Stable insertion sort of the vertex order by value (thread 0), between barriers.
__device__ void nm_sort(NmShared& s, int D) {
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i <= D; ++i) {
            const int v = s.ord[i];
            const double fv = s.fsim[v];
            int j = i - 1;
            while (j >= 0 && nm_before(fv, s.fsim[s.ord[j]])) {
                s.ord[j + 1] = s.ord[j];
                --j;
            }
            s.ord[j + 1] = v;
        }
    }
    __syncthreads();
}

template <int DPAD, int FORM>
__global__ __launch_bounds__(NM_T) void nm_search_kernel(NmArgs a) {
    __shared__ NmShared s;
    const int t = threadIdx.x;
    const int D = a.ndim;
    const long long rs = blockIdx.x;
    apgp_exp_tab_load(s.etab);
    double* trace = a.trace ? a.trace + rs * (long long)a.maxfev * (D + 3) : nullptr;
    int* steps = a.steps ? a.steps + rs * (long long)a.maxiter : nullptr;
    // initial simplex: x0, then x0 with coordinate k scaled by 1.05 (0.00025 for a zero coordinate)
    if (t < D) {
        const double x0 = a.starts[rs * D + t];
        s.sim[0][t] = x0;
        for (int k = 0; k < D; ++k) s.sim[k + 1][t] = (t == k) ? (x0 != 0.0 ? (1.0 + 0.05) * x0 : 0.00025) : x0;
    }
    if (t <= D) {
        s.fsim[t] = INFINITY;
        s.ord[t] = t;
    }
    int nfev = 0;
    for (int k = 0; k <= D; ++k) {
        if (nfev >= a.maxfev) break;
        __syncthreads();
        if (t < D) s.xt[t] = s.sim[k][t];
        const double f = nm_eval<DPAD, FORM>(a, s, trace, nfev);
        ++nfev;
        if (t == 0) s.fsim[k] = f;
    }
    nm_sort(s, D);
    int it = 1, body = 0;
    while (nfev < a.maxfev && it < a.maxiter) {
        if (t == 0) {
            // np.max(np.abs(sim[1:] - sim[0])) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol, NaN-propagating
            const int b = s.ord[0];
            bool nan = false;
            double xm = 0.0, fm = 0.0;
            for (int j = 1; j <= D; ++j) {
                const int v = s.ord[j];
                for (int d = 0; d < D; ++d) {
                    const double e = fabs(s.sim[v][d] - s.sim[b][d]);
                    if (isnan(e)) nan = true;
                    else if (e > xm) xm = e;
                }
            }
            bool conv = !nan && xm <= a.xatol;
            if (conv) {
                for (int j = 1; j <= D; ++j) {
                    const double e = fabs(s.fsim[b] - s.fsim[s.ord[j]]);
                    if (isnan(e)) nan = true;
                    else if (e > fm) fm = e;
                }
                conv = !nan && fm <= a.fatol;
            }
            s.conv = conv ? 1 : 0;
        }
        __syncthreads();
        if (s.conv) break;
        const int b0 = s.ord[0], bl = s.ord[D], b2 = s.ord[D - 1];
        // xbar = np.add.reduce(sim[:-1], 0) / N (row order); xr = (1 + rho) xbar - rho sim[-1]
        if (t < D) {
            double acc = s.sim[b0][t];
            for (int j = 1; j < D; ++j) acc += s.sim[s.ord[j]][t];
            const double xb = acc / (double)D;
            s.xbar[t] = xb;
            const double xr = (1.0 + a.rho) * xb - a.rho * s.sim[bl][t];
            s.xr[t] = xr;
            s.xt[t] = xr;
        }
        int step = APGP_NM_STEP_MAXFEV;
        bool take_xt = false, take_xr = false, shrink = false;
        double fnew = 0.0;
        const double fxr = nm_eval<DPAD, FORM>(a, s, trace, nfev);
        ++nfev;
        if (fxr < s.fsim[b0]) {
            if (t < D) s.xt[t] = (1.0 + a.rho * a.chi) * s.xbar[t] - a.rho * a.chi * s.sim[bl][t];
            if (nfev < a.maxfev) {
                const double fxe = nm_eval<DPAD, FORM>(a, s, trace, nfev);
                ++nfev;
                if (fxe < fxr) { take_xt = true; fnew = fxe; step = APGP_NM_STEP_EXPAND; }
                else { take_xr = true; fnew = fxr; step = APGP_NM_STEP_REFLECT_EXP; }
            }
        } else if (fxr < s.fsim[b2]) {
            take_xr = true; fnew = fxr; step = APGP_NM_STEP_REFLECT;
        } else if (fxr < s.fsim[bl]) {
            if (t < D) s.xt[t] = (1.0 + a.psi * a.rho) * s.xbar[t] - a.psi * a.rho * s.sim[bl][t];
            if (nfev < a.maxfev) {
                const double fxc = nm_eval<DPAD, FORM>(a, s, trace, nfev);
                ++nfev;
                if (fxc <= fxr) { take_xt = true; fnew = fxc; step = APGP_NM_STEP_CONTRACT_OUT; }
                else { shrink = true; step = APGP_NM_STEP_SHRINK_OUT; }
            }
        } else {
            if (t < D) s.xt[t] = (1.0 - a.psi) * s.xbar[t] + a.psi * s.sim[bl][t];
            if (nfev < a.maxfev) {
                const double fxcc = nm_eval<DPAD, FORM>(a, s, trace, nfev);
                ++nfev;
                if (fxcc < s.fsim[bl]) { take_xt = true; fnew = fxcc; step = APGP_NM_STEP_CONTRACT_IN; }
                else { shrink = true; step = APGP_NM_STEP_SHRINK_IN; }
            }
        }
        __syncthreads();                                       // every thread has decided before the state changes
        if (take_xt || take_xr) {
            if (t < D) s.sim[bl][t] = take_xt ? s.xt[t] : s.xr[t];
            if (t == 0) s.fsim[bl] = fnew;
        }
        if (shrink) {
            for (int j = 1; j <= D; ++j) {
                const int v = s.ord[j];
                if (t < D) {
                    const double x = s.sim[b0][t] + a.sigma * (s.sim[v][t] - s.sim[b0][t]);
                    s.sim[v][t] = x;
                    s.xt[t] = x;
                }
                if (nfev >= a.maxfev) { step = APGP_NM_STEP_MAXFEV; break; }   // (the vertex moved, its value did not)
                const double f = nm_eval<DPAD, FORM>(a, s, trace, nfev);
                ++nfev;
                if (t == 0) s.fsim[v] = f;
            }
        }
        if (step != APGP_NM_STEP_MAXFEV) ++it;
        if (steps && t == 0) steps[body] = step;
        ++body;
        nm_sort(s, D);
    }
    __syncthreads();
    const int b = s.ord[0];
    if (t < D) a.x_out[rs * D + t] = s.sim[b][t];
    if (t == 0) {
        bool nan = false;
        for (int j = 0; j <= D; ++j) nan = nan || isnan(s.fsim[j]);
        a.f_out[rs] = nan ? NAN : s.fsim[b];
        a.stats[3 * rs] = nfev;
        a.stats[3 * rs + 1] = it;
        a.stats[3 * rs + 2] = nfev >= a.maxfev ? 1 : (it >= a.maxiter ? 2 : 0);
    }
}

extern "C" int64_t apgp_nm_search_work_len(int64_t restarts, int64_t n) {
    if (restarts < 1 || restarts > APGP_NM_MAX_RESTARTS || n < 1 || n > APGP_MAX_N) return -1;
    return restarts * apgp_round_up(n, 64);
}

template <int FORM>
static void nm_launch(int dpad, hipStream_t s, const NmArgs& a, unsigned grid) {
    apgp_by_dpad(dpad, [&](auto dp) {
        hipLaunchKernelGGL((nm_search_kernel<decltype(dp)::value, FORM>), dim3(grid), dim3(NM_T), 0, s, a);
    });
}

extern "C" int apgp_nm_search(const double* starts, int64_t restarts, const double* xs, int64_t n,
                              const apgp_kernel_t* kern, double mean,
                              const double* winv, int64_t ldw, const double* L, int64_t ldl,
                              const double* lo, const double* hi, const apgp_nm_options_t* opt,
                              double* x_out, double* f_out, int32_t* stats, double* trace, int32_t* steps,
                              double* work, void* stream) {
    APGP_CHECK_ARG(starts && xs && kern && opt && x_out && f_out && stats && work, "null pointer");
    APGP_CHECK_ARG(restarts >= 1 && restarts <= APGP_NM_MAX_RESTARTS, "1 <= restarts <= APGP_NM_MAX_RESTARTS required");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG((winv && ldw >= n && ldw % 2 == 0) || (!winv && L && ldl >= n),
                   "the dense inverse (even ldw >= n) or the factor (ldl >= n) is required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi go together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(opt->kind == APGP_UTIL_AGP || opt->kind == APGP_UTIL_BAPE || opt->kind == APGP_UTIL_JONES ||
                   opt->kind == APGP_UTIL_NEG_MEAN, "kind: AGP, BAPE, JONES or NEG_MEAN");
    APGP_CHECK_ARG(opt->maxiter >= 1 && opt->maxiter <= APGP_NM_MAX_FEV && opt->maxfev >= 1 &&
                   opt->maxfev <= APGP_NM_MAX_FEV, "1 <= maxiter, maxfev <= APGP_NM_MAX_FEV required");
    NmArgs a;
    a.starts = starts; a.xs = xs; a.W = winv; a.L = L; a.work = work;
    a.x_out = x_out; a.f_out = f_out; a.stats = (int*)stats; a.trace = trace; a.steps = (int*)steps;
    a.n = n; a.ldw = winv ? ldw : 0; a.ldl = L ? ldl : 0; a.wstride = apgp_round_up(n, 64);
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    a.kind = opt->kind; a.maxiter = opt->maxiter; a.maxfev = opt->maxfev;
    a.mean = mean; a.zeta = opt->zeta; a.ybest = opt->ybest;
    a.xatol = opt->xatol; a.fatol = opt->fatol;
    a.rho = opt->rho; a.chi = opt->chi; a.psi = opt->psi; a.sigma = opt->sigma;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)restarts;
    if (winv && n <= 256) nm_launch<0>(kc.dpad, s, a, grid);
    else if (winv) nm_launch<1>(kc.dpad, s, a, grid);
    else nm_launch<2>(kc.dpad, s, a, grid);
    APGP_CHECK_LAUNCH();
    return 0;
}
