// The sampler body of the on-device ensemble samplers: the argument struct, the steps every sampler kernel shares -- each
// spelled once and force-inlined (as ens_propose of ens_moves.h is) -- and the host-side checks that fill the arguments.
// ensemble_kernel and ensemble_mw_kernel (ensemble.hip) and tempered_kernel (tempering.hip) are schedules around them: who
// evaluates which proposals, and how the values reach the accept step.
#pragma once
#include "apgp_common.h"
#include "ens_moves.h"

struct EnsArgs {
    const double* xs;      // packed training stream: Npad x (DPAD+2): scaled x | alpha | 0
    double* coords;        // E x W x D  (in: initial state, out: final state)
    double* logp;          // E x W      (out: final log-probability)
    double* chain;         // iterations x E x W x D or NULL
    double* logp_chain;    // iterations x E x W or NULL
    long long* naccept;    // E x W
    long long n, iterations;
    int ndim, nwalkers, lin_order;
    unsigned long long seed;
    double mean, amp, lin_coef;
    EnsMoves mv;           // the move table; ens_propose (ens_moves.h) forms the proposals
    double sc[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM], lw[APGP_MAX_DIM];
};

// Lane sums of k(p, x_k) alpha_k over the training rows first, first + stride, ... (xs: the stream, in LDS or L2) for TWO
// points t0 / t1 (scaled coordinates), butterflied over the wavefront.  Every row read serves both points: the stream is
// 80 B per row and is read by all wavefronts of every half-step; with one point per pass the LDS, not the arithmetic, set
// the pace.  Each point's sum runs in the order of ens_rows1.
template <int DPAD>
__device__ __forceinline__ void ens_rows2(const EnsArgs& a, const double* xs, const double* etab, const double (&t0)[DPAD],
                                          const double (&t1)[DPAD], const int first, const int stride, double& r0, double& r1) {
    double acc0 = 0.0, acc1 = 0.0;
    const int nn = (int)a.n;
    for (int k = first; k < nn; k += stride) {
        const double* xr = xs + k * (DPAD + 2);
        double xv[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) xv[d] = xr[d];
        const double al = xr[DPAD];
        double s0 = 0.0, s03 = 0.0, s1 = 0.0, s13 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            const double a0 = t0[d] - xv[d], a1 = t0[d + 1] - xv[d + 1];
            const double b0 = t1[d] - xv[d], b1 = t1[d + 1] - xv[d + 1];
            s0 = fma(a0, a0, s0); s03 = fma(a1, a1, s03);
            s1 = fma(b0, b0, s1); s13 = fma(b1, b1, s13);
        }
        double kv0 = a.amp * apgp_exp(-(s0 + s03), etab);
        double kv1 = a.amp * apgp_exp(-(s1 + s13), etab);
        if (a.lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, t0[d_] * xv[d_] * a.lw[d_]);
            kv0 = fma(a.lin_coef, ls, kv0);
            APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, t1[d_] * xv[d_] * a.lw[d_]);
            kv1 = fma(a.lin_coef, ls, kv1);
        }
        acc0 = fma(kv0, al, acc0);
        acc1 = fma(kv1, al, acc1);
    }
    for (int o = 32; o > 0; o >>= 1) { acc0 += __shfl_xor(acc0, o); acc1 += __shfl_xor(acc1, o); }
    r0 = acc0;
    r1 = acc1;
}
// its one-point sibling, the same chain per point (start-up; and D > 8, where two points' registers do not fit 16 wavefronts)
template <int DPAD>
__device__ __forceinline__ double ens_rows1(const EnsArgs& a, const double* xs, const double* etab, const double* p,
                                            const int first, const int stride) {
    double tt[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) tt[d] = p[d];
    double acc = 0.0;
    const int nn = (int)a.n;
    for (int k = first; k < nn; k += stride) {
        const double* xr = xs + k * (DPAD + 2);
        double s = 0.0, s3 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            const double df0 = tt[d] - xr[d], df1 = tt[d + 1] - xr[d + 1];
            s = fma(df0, df0, s);
            s3 = fma(df1, df1, s3);
        }
        double kv = a.amp * apgp_exp(-(s + s3), etab);
        if (a.lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xr[d_] * a.lw[d_]);
            kv = fma(a.lin_coef, ls, kv);
        }
        acc = fma(kv, xr[DPAD], acc);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}

// Walker load by a workgroup of NT threads: scaled coordinates, accept counters zeroed.  XLDS: the packed training stream
// (Npad x (DPAD+2) doubles) is staged into LDS once (it is re-read by every walker of every half-step); it stays in L2
// when it does not fit beside the sampler state.
template <int DPAD, bool XLDS, int NT>
__device__ __forceinline__ void ens_load(const EnsArgs& a, const double* gc, double (*cs)[DPAD], int* nacc, double* xsl, const int t) {
    const int W = a.nwalkers, D = a.ndim;
    for (int e = t; e < W * DPAD; e += NT) {
        const int w = e / DPAD, d = e % DPAD;
        cs[w][d] = d < D ? gc[w * D + d] * a.sc[d] : 0.0;
    }
    if (t < W) nacc[t] = 0;
    if (XLDS) {
        for (long long e = t; e < a.n * (DPAD + 2); e += NT) xsl[e] = a.xs[e];
    }
}

// the start gate: a walker c outside the prior's box has zero probability (as _gpll returns -inf): m, or -inf there
__device__ __forceinline__ double ens_gate(const EnsArgs& a, const double* c, double m) {
    for (int d = 0; d < a.ndim; ++d)
        if (!(c[d] >= a.lo[d] && c[d] <= a.hi[d])) m = -INFINITY;
    return m;
}

// walker of slot i of half `half` of the red/blue partition: the active half S of a split is half `split`, its
// complement C half `1 - split`
__device__ __forceinline__ int ens_slot(const int i, const int half, const int H, const int rot, const int W) {
    const int v = i + half * H + rot;
    return v >= W ? v - W : v;
}

// The iteration's prologue (Philox tag 5): returns the random cyclic offset of the red/blue partition and, for a mixed
// table, sets the iteration's move, uniform over the workgroup(s).  (The move of a one-entry table, the default, is read
// once before the loop, not per iteration.)
__device__ __forceinline__ int ens_iteration(const EnsMoves& mv, const bool mixed, const long long it, const unsigned int k0,
                                             const unsigned int k1, const int W, int& mkind, double& mp0, double& mp1) {
    unsigned int cr[4] = {(unsigned int)it, (unsigned int)(it >> 32), 0xFFFFFFFFu, 0x5u};
    philox4x32(cr, k0, k1);
    const int rot = (int)(cr[0] % (unsigned int)W);
    if (mixed) {
        const int mi = ens_pick_move(mv, cr);
        mkind = mv.kind[mi]; mp0 = mv.p0[mi]; mp1 = mv.p1[mi];
    }
    return rot;
}

// the accept step of slot t, whose walker is s
template <int DPAD>
__device__ __forceinline__ void ens_accept(const int t, const int s, double (*cs)[DPAD], double* lp, int* nacc,
                                           const double (*qs)[DPAD], const double* lpq, const double* fac, const double* uacc,
                                           const int* qok) {
    const double diff = fac[t] + lpq[t] - lp[s];
    if (qok[t] && lpq[t] == lpq[t] && log(uacc[t]) < diff) {
#pragma unroll
        for (int d = 0; d < DPAD; ++d) cs[s][d] = qs[t][d];
        lp[s] = lpq[t];
        nacc[s] += 1;
    }
}

// Result writes.  The walkers in plain coordinates, elements first, first + stride, ... of a W x D block:
template <int DPAD>
__device__ __forceinline__ void ens_store_walkers(const EnsArgs& a, const double (*cs)[DPAD], double* out, const int W,
                                                  const int D, const int first, const int stride) {
    for (int e = first; e < W * D; e += stride) {
        const int w = e / D, d = e % D;
        out[e] = cs[w][d] / a.sc[d];
    }
}

// fills mv from the caller's table (NULL with nmoves == 0: the stretch move at a_stretch alone) or returns the failed check
static const char* ens_move_table(EnsMoves& mv, const apgp_ens_move_t* moves, int32_t nmoves, double a_stretch,
                                  int ndim, int nwalkers) {
    apgp_ens_move_t one = {APGP_ENS_MOVE_STRETCH, 1.0, a_stretch, 0.0};
    if (moves == nullptr) {
        if (nmoves != 0) return "moves is NULL but nmoves is not 0";
        moves = &one;
        nmoves = 1;
    }
    if (!(nmoves >= 1 && nmoves <= APGP_ENS_MAX_MOVES)) return "1 <= nmoves <= APGP_ENS_MAX_MOVES required";
    double total = 0.0;
    for (int m = 0; m < nmoves; ++m) {
        if (!(std::isfinite(moves[m].weight) && moves[m].weight > 0.0)) return "move weights must be finite and > 0";
        total = total + moves[m].weight;
    }
    if (!std::isfinite(total)) return "move weights must have a finite sum";
    double acc = 0.0;
    for (int m = 0; m < APGP_ENS_MAX_MOVES; ++m) {
        mv.kind[m] = APGP_ENS_MOVE_STRETCH;
        mv.cum[m] = 1.0;
        mv.p0[m] = 2.0;
        mv.p1[m] = 0.0;
        if (m >= nmoves) continue;
        const double u = moves[m].p0, v = moves[m].p1;
        acc = acc + moves[m].weight;
        mv.kind[m] = moves[m].kind;
        mv.cum[m] = acc / total;
        mv.p0[m] = u;
        switch (moves[m].kind) {
            case APGP_ENS_MOVE_STRETCH:
                if (!(u > 1.0)) return "stretch scale a must be > 1";
                break;
            case APGP_ENS_MOVE_DE:
                if (!(std::isfinite(u) && u >= 0.0)) return "DE sigma must be finite and >= 0";
                if (!(std::isfinite(v) && v >= 0.0)) return "DE gamma0 must be finite and > 0 (0: the default)";
                if (nwalkers < 4) return "the DE move needs at least 4 walkers";
                mv.p1[m] = v > 0.0 ? v : 2.38 / std::sqrt(2.0 * ndim);
                break;
            case APGP_ENS_MOVE_SNOOKER:
                if (!(std::isfinite(u) && u > 0.0)) return "snooker gammas must be finite and > 0";
                if (nwalkers < 6) return "the snooker move needs at least 6 walkers";
                break;
            default:
                return "unknown move kind";
        }
    }
    mv.n = nmoves;
    return nullptr;
}

// the kernels' arguments from the checked ones: the walkers live in scaled coordinates x * sc
static EnsArgs ens_args(const double* xs, int64_t n, const KernConst& kc, double mean, const double* lo, const double* hi,
                        int32_t nwalkers, int64_t iterations, uint64_t seed, double* coords, double* logp, double* chain,
                        double* logp_chain, int64_t* naccept, const EnsMoves& mv) {
    EnsArgs a;
    a.xs = xs; a.coords = coords; a.logp = logp; a.chain = chain; a.logp_chain = logp_chain;
    a.naccept = (long long*)naccept; a.n = apgp_npad(n); a.iterations = iterations;
    a.ndim = kc.ndim; a.nwalkers = nwalkers; a.seed = seed; a.mean = mean; a.amp = kc.amp;
    a.mv = mv;
    a.lin_coef = kc.lin_coef; a.lin_order = kc.lin_order;
    for (int d = 0; d < APGP_MAX_DIM; ++d) {
        a.lw[d] = kc.lw[d];
        a.sc[d] = d < kc.ndim ? kc.sc[d] : 1.0;
        a.lo[d] = d < kc.ndim ? lo[d] * kc.sc[d] : 0.0;     // bounds in scaled coordinates
        a.hi[d] = d < kc.ndim ? hi[d] * kc.sc[d] : 0.0;
    }
    return a;
}
