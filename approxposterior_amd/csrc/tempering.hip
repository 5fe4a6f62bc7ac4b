// Parallel tempering of the on-device ensemble sampler (include/apgp.h: apgp_tempered_sample).  A ladder is T ensembles
// ("rungs") of one problem; rung k targets exp(beta_k mu) on the box, beta_0 = 1 >= beta_1 >= ... >= 0, and neighbouring
// rungs exchange walkers every swap_every iterations.  A multimodal surrogate is what this is for: the red/blue moves build
// proposals from the walkers' own positions, so a cold ensemble that starts in one mode stays there; a hot rung crosses the
// barrier and hands its walkers down the ladder.
//
// Rung k of ladder l is ensemble e = l T + k of ensemble_kernel: the same keys, the same counters with the GLOBAL iteration
// number, the same ens_propose, the sampler body of ens_body.h.  It keeps two values per walker: mu, and the tempered
// value beta mu that ens_accept -- unchanged -- is fed (-inf wherever mu is not finite, at every beta).  beta = 1
// multiplies exactly: a beta = 1 rung makes the decisions ensemble_kernel makes, bit for bit.
//
// The schedule has no hand-off inside a launch: one launch per segment of swap_every iterations, a workgroup per rung, no
// waiting between workgroups.  State ping-pongs between two buffers in `work` (scaled coordinates as the kernel holds
// them, and mu), so no launch reads what it writes.  A workgroup opens a segment by reading its own mu row and its
// partner's from the previous segment's output, recomputes the pair's exchange decisions -- pure functions of those rows
// and of (seed, ladder, pair, round, walker), so both partners agree -- and loads each walker from whichever rung the
// decision says; only the lower rung of a pair writes the pair's log and counters.
#include "apgp_common.h"
#include "scratch.h"
#include "ens_moves.h"
#include "ens_body.h"

struct PtArgs {
    EnsArgs e;                 // e.iterations: the iterations of THIS segment; coords / logp: read by the first, written by the last
    const double* src;         // the previous segment's state: E x W x DPAD scaled coordinates | E x W mu
    double* dst;               // this segment's
    long long it0;             // global number of the segment's first iteration
    long long round;           // the exchange round that opens the segment (segment number - 1)
    long long* swap_prop;      // L x (T - 1)
    long long* swap_acc;
    unsigned char* swap_log;   // rounds x L x (T - 1) x W or NULL
    int ntemps, nstore, first, last;
    double beta[APGP_PT_MAX_TEMPS];
};

// the tempered value of a log-probability m: beta m, -inf wherever m is not finite (beta = 0 included)
__device__ __forceinline__ double pt_temper(const double beta, const double m) { return isfinite(m) ? beta * m : -INFINITY; }

// One workgroup of 1024 threads per rung, scheduled as ensemble_kernel: slot t proposes and accepts; wavefront wv takes
// proposals wv and wv + 16 through one pass over the training stream (one proposal per pass for D > 8).
template <int DPAD, bool XLDS, bool ALLMOVES>
__global__ __launch_bounds__(1024) void tempered_kernel(PtArgs q) {
    const EnsArgs& a = q.e;
    extern __shared__ __attribute__((aligned(16))) double xsl[];
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double cs[ENS_MAXW][DPAD];      // scaled walker coordinates
    __shared__ double lp[ENS_MAXW];            // mu
    __shared__ double lt[ENS_MAXW];            // beta mu: what the accept step compares
    __shared__ double qs[ENS_MAXW / 2][DPAD];  // scaled proposals of the active half
    __shared__ double lpq[ENS_MAXW / 2];
    __shared__ double ltq[ENS_MAXW / 2];
    __shared__ double fac[ENS_MAXW / 2];
    __shared__ double uacc[ENS_MAXW / 2];
    __shared__ int qok[ENS_MAXW / 2];
    __shared__ int nacc[ENS_MAXW];
    __shared__ int from[ENS_MAXW];             // the ensemble walker i is loaded from
    __shared__ int cnt[2];                     // proposed, accepted exchanges of the pair this rung is the lower one of
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int W = a.nwalkers, H = W / 2, D = a.ndim, T = q.ntemps;
    const long long ens = blockIdx.x, E = gridDim.x;
    const long long lad = ens / T, L = E / T;
    const int k = (int)(ens % T);
    const double beta = q.beta[k];
    apgp_exp_tab_load(etab);
    double* gc = a.coords + ens * W * D;

    // GP means of two points and of one by one wavefront, its lanes striding the training rows
    auto gp_mean2 = [&](const double* p0, const double* p1, double& m0, double& m1) {
        double t0[DPAD], t1[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) { t0[d] = p0[d]; t1[d] = p1[d]; }
        double acc0, acc1;
        ens_rows2<DPAD>(a, XLDS ? (const double*)xsl : a.xs, etab, t0, t1, lane, 64, acc0, acc1);
        m0 = acc0 + a.mean;
        m1 = acc1 + a.mean;
    };
    auto gp_mean = [&](const double* p) { return ens_rows1<DPAD>(a, XLDS ? (const double*)xsl : a.xs, etab, p, lane, 64) + a.mean; };

    if (q.first) {
        // the caller's walkers: scaled once, here; mu is computed from coordinates in this segment only
        ens_load<DPAD, XLDS, 1024>(a, gc, cs, nacc, xsl, t);
        __syncthreads();
        for (int w = wv; w < W; w += 16) {
            double m = gp_mean(cs[w]);
            m = ens_gate(a, cs[w], m);
            if (lane == 0) lp[w] = m;
        }
    } else {
        // exchange round q.round pairs rungs (j, j + 1), j = round (mod 2); this rung's partner, or none
        const double* smu = q.src + E * W * DPAD;
        int kp = -1;
        if ((k & 1) == (int)(q.round & 1)) { if (k + 1 < T) kp = k + 1; }
        else if (k >= 1) kp = k - 1;
        if (t < 2) cnt[t] = 0;
        __syncthreads();
        if (t < W) {
            long long se = ens;
            if (kp >= 0) {
                const int kl = kp > k ? k : kp;                 // the pair's lower rung: its keys, its log
                const long long el = lad * T + kl;
                const double ml = smu[el * W + t], mh = smu[(el + 1) * W + t];
                int dec = 0;
                if (isfinite(ml) && isfinite(mh)) {
                    unsigned int c[4] = {(unsigned int)q.round, (unsigned int)(q.round >> 32), (unsigned int)t, 0x7u};
                    philox4x32(c, (unsigned int)a.seed, (unsigned int)(a.seed >> 32) ^ (unsigned int)(el * 0x9E3779B9u));
                    dec = log(u01(c[0], c[1])) < (q.beta[kl] - q.beta[kl + 1]) * (mh - ml) ? 2 : 1;
                }
                if (dec == 2) se = lad * T + kp;
                if (kl == k) {
                    if (q.swap_log) q.swap_log[((q.round * L + lad) * (T - 1) + kl) * W + t] = (unsigned char)dec;
                    if (dec >= 1) atomicAdd(&cnt[0], 1);
                    if (dec == 2) atomicAdd(&cnt[1], 1);
                }
            }
            from[t] = (int)se;
            lp[t] = smu[se * W + t];
            nacc[t] = 0;
        }
        __syncthreads();
        for (int e = t; e < W * DPAD; e += 1024) {
            const int w = e / DPAD;
            cs[w][e % DPAD] = q.src[((long long)from[w] * W) * DPAD + e];
        }
        if (XLDS) {
            for (long long e = t; e < a.n * (DPAD + 2); e += 1024) xsl[e] = a.xs[e];
        }
        if (t == 0 && kp > k) {
            q.swap_prop[lad * (T - 1) + k] += cnt[0];
            q.swap_acc[lad * (T - 1) + k] += cnt[1];
        }
    }
    __syncthreads();
    if (t < W) lt[t] = pt_temper(beta, lp[t]);
    __syncthreads();

    const unsigned int k0 = (unsigned int)a.seed, k1 = (unsigned int)(a.seed >> 32) ^ (unsigned int)(ens * 0x9E3779B9u);
    const bool mixed = a.mv.n > 1;
    int mkind = a.mv.kind[0];
    double mp0 = a.mv.p0[0], mp1 = a.mv.p1[0];
    for (long long it = q.it0; it < q.it0 + a.iterations; ++it) {
        const int rot = ens_iteration(a.mv, mixed, it, k0, k1, W, mkind, mp0, mp1);
        for (int split = 0; split < 2; ++split) {
            auto s_idx = [&](int i) { return ens_slot(i, split, H, rot, W); };
            auto c_idx = [&](int i) { return ens_slot(i, 1 - split, H, rot, W); };
            if (t < H) {
                qok[t] = ens_propose<DPAD, ALLMOVES>(mkind, mp0, mp1, cs, s_idx(t), c_idx, H, D, a.lo, a.hi, it, split, t, k0, k1, qs[t],
                                           fac[t], uacc[t]) ? 1 : 0;
            }
            __syncthreads();
            if constexpr (DPAD > 8) {
                for (int i = wv; i < H; i += 16) {
                    double m = -INFINITY;
                    if (qok[i]) m = gp_mean(qs[i]);         // wave-uniform branch
                    if (lane == 0) { lpq[i] = m; ltq[i] = pt_temper(beta, m); }
                }
            } else
            for (int i = wv; i < H; i += 32) {
                // proposals i and i + 16 of this wavefront in one pass over the training stream
                const int i1 = i + 16;
                const bool ok0 = qok[i] != 0, ok1 = i1 < H && qok[i1] != 0;     // wave-uniform
                double m0 = -INFINITY, m1 = -INFINITY;
                if (ok0 && ok1) gp_mean2(qs[i], qs[i1], m0, m1);
                else if (ok0) m0 = gp_mean(qs[i]);
                else if (ok1) m1 = gp_mean(qs[i1]);
                if (lane == 0) {
                    lpq[i] = m0; ltq[i] = pt_temper(beta, m0);
                    if (i1 < H) { lpq[i1] = m1; ltq[i1] = pt_temper(beta, m1); }
                }
            }
            __syncthreads();
            if (t < H) {
                // ens_accept on the tempered values; mu follows an accepted move
                const int s = s_idx(t), n0 = nacc[s];
                ens_accept<DPAD>(t, s, cs, lt, nacc, qs, ltq, fac, uacc, qok);
                if (nacc[s] != n0) lp[s] = lpq[t];
            }
            __syncthreads();
        }
        if (a.chain && k < q.nstore) ens_store_walkers<DPAD>(a, cs, a.chain + (((it * L + lad) * q.nstore + k) * W) * D, W, D, t, 1024);
        if (a.logp_chain && t < W) a.logp_chain[(it * E + ens) * W + t] = lp[t];
    }
    if (q.last) {
        ens_store_walkers<DPAD>(a, cs, gc, W, D, t, 1024);
        if (t < W) a.logp[ens * W + t] = lp[t];
    } else {
        // the next segment's input: the scaled coordinates as they are held here (a round trip through plain coordinates
        // would perturb the walkers), and mu
        for (int e = t; e < W * DPAD; e += 1024) q.dst[(ens * W) * DPAD + e] = cs[e / DPAD][e % DPAD];
        if (t < W) q.dst[E * W * DPAD + ens * W + t] = lp[t];
    }
    // the accept counters stay with the rung
    if (t < W) a.naccept[ens * W + t] = (q.first ? 0ll : a.naccept[ens * W + t]) + nacc[t];
}

extern "C" int64_t apgp_tempered_work_len(int32_t nwalkers, int32_t ntemps, int32_t nladders, int32_t ndim) {
    if (nwalkers < 2 || nwalkers > ENS_MAXW || ntemps < 1 || ntemps > APGP_PT_MAX_TEMPS || nladders < 1 || ndim < 1 ||
        ndim > APGP_MAX_DIM || (int64_t)nladders * ntemps > 0x7fffffffll)
        return -1;
    return 2 * (int64_t)nladders * ntemps * nwalkers * (apgp_dpad(ndim) + 1);
}

// One segment's launch in one instantiation (as ens_launch of ensemble.hip): the LDS-resident form needs > 64 KiB of dynamic
// LDS, a per-device attribute set and checked once per device and instantiation, keyed by the STREAM's device.
template <int DP, bool AM>
static int pt_launch(const PtArgs& q, dim3 grid, size_t xbytes, bool xlds, int dev, hipStream_t s) {
    static ApgpLdsOnce once;
    void (*kl)(PtArgs) = tempered_kernel<DP, true, AM>;
    void (*kg)(PtArgs) = tempered_kernel<DP, false, AM>;
    if (xlds && apgp_raise_lds(once, "apgp_tempered_sample", dev, 96 * 1024, {(const void*)kl}) != 0) return -2;
    hipLaunchKernelGGL(xlds ? kl : kg, grid, dim3(1024), xlds ? xbytes : 0, s, q);
    return 0;
}

extern "C" int apgp_tempered_sample(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean, const double* lo,
                                    const double* hi, int32_t nwalkers, int32_t ntemps, int32_t nladders,
                                    const double* betas, int64_t iterations, int64_t swap_every, uint64_t seed,
                                    double* coords, double* logp, double* chain, int32_t nstore, double* logp_chain,
                                    int64_t* naccept, int64_t* swap_prop, int64_t* swap_acc, uint8_t* swap_log,
                                    const apgp_ens_move_t* moves, int32_t nmoves, double* work, void* stream) {
    APGP_CHECK_ARG(xs && kern && lo && hi && betas && coords && logp && naccept && work, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N && iterations >= 0 && nladders >= 1, "n, iterations, nladders");
    APGP_CHECK_ARG(ntemps >= 1 && ntemps <= APGP_PT_MAX_TEMPS, "1 <= ntemps <= APGP_PT_MAX_TEMPS required");
    APGP_CHECK_ARG((int64_t)nladders * ntemps <= 0x7fffffffll, "nladders * ntemps exceeds the grid limit");
    APGP_CHECK_ARG(swap_every >= 1, "swap_every must be >= 1");
    APGP_CHECK_ARG(nstore >= 0 && nstore <= ntemps, "0 <= nstore <= ntemps required");
    APGP_CHECK_ARG(ntemps == 1 || (swap_prop && swap_acc), "swap_prop and swap_acc are NULL");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(nwalkers >= 2 && nwalkers % 2 == 0 && nwalkers <= ENS_MAXW, "nwalkers must be even and <= 256");
    APGP_CHECK_ARG(nwalkers >= 2 * kc.ndim, "nwalkers must be at least twice the dimension");
    for (int k = 0; k < ntemps; ++k) {
        APGP_CHECK_ARG(std::isfinite(betas[k]) && betas[k] >= 0.0 && betas[k] <= 1.0, "betas must be finite and in [0, 1]");
        APGP_CHECK_ARG(k == 0 || betas[k] <= betas[k - 1], "betas must not increase");
    }
    if (betas[ntemps - 1] == 0.0)
        for (int d = 0; d < kc.ndim; ++d)
            APGP_CHECK_ARG(std::isfinite(lo[d]) && std::isfinite(hi[d]), "betas: beta = 0 samples the box, lo and hi must be finite");
    EnsMoves mv;
    const char* bad = ens_move_table(mv, moves, nmoves, 2.0, kc.ndim, nwalkers);
    APGP_CHECK_ARG(bad == nullptr, bad);
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(kc.sc[d] > 0.0, "inverse metric must be positive");
    bool allmoves = false;
    for (int m = 0; m < mv.n; ++m) allmoves = allmoves || mv.kind[m] != APGP_ENS_MOVE_STRETCH;

    hipStream_t s = (hipStream_t)stream;
    const int dev = apgp_stream_device(s);
    if (dev < 0 || dev >= 64) {
        apgp_set_error("apgp_tempered_sample: the stream's device is outside 0 .. 63");
        return -2;
    }
    PtArgs q;
    q.e = ens_args(xs, n, kc, mean, lo, hi, nwalkers, iterations, seed, coords, logp, nstore > 0 ? chain : nullptr, logp_chain,
                   naccept, mv);
    q.swap_prop = (long long*)swap_prop; q.swap_acc = (long long*)swap_acc; q.swap_log = swap_log;
    q.ntemps = ntemps; q.nstore = nstore;
    for (int k = 0; k < APGP_PT_MAX_TEMPS; ++k) q.beta[k] = k < ntemps ? betas[k] : 0.0;
    const long long E = (long long)nladders * ntemps;
    const long long nseg = iterations > 0 ? (iterations + swap_every - 1) / swap_every : 1;
    const size_t half = (size_t)E * nwalkers * (kc.dpad + 1);
    const size_t pairs = (size_t)nladders * (ntemps - 1);
    if (pairs > 0) {
        hipError_t e = hipMemsetAsync(swap_prop, 0, pairs * sizeof(int64_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(swap_acc, 0, pairs * sizeof(int64_t), s);
        if (e == hipSuccess && swap_log && nseg > 1) e = hipMemsetAsync(swap_log, 0, (size_t)(nseg - 1) * pairs * nwalkers, s);
        if (e != hipSuccess) {
            apgp_set_error("apgp_tempered_sample: hipMemsetAsync: %s", hipGetErrorString(e));
            return -2;
        }
    }
    const dim3 grid((unsigned)E);
    const size_t xbytes = (size_t)q.e.n * (kc.dpad + 2) * sizeof(double);
    const bool xlds = xbytes <= 96 * 1024 && kc.dpad <= 16;       // the policy of apgp_ensemble_sample_moves
    // every segment is enqueued here, nothing is waited for
    for (long long g = 0; g < nseg; ++g) {
        q.first = g == 0; q.last = g == nseg - 1;
        q.it0 = g * swap_every;
        q.e.iterations = iterations - q.it0 < swap_every ? iterations - q.it0 : swap_every;
        q.round = g - 1;
        q.src = work + (size_t)((g + 1) & 1) * half;
        q.dst = work + (size_t)(g & 1) * half;
        const int rc = allmoves
            ? apgp_by_dpad(kc.dpad, [&](auto dp) { return pt_launch<decltype(dp)::value, true>(q, grid, xbytes, xlds, dev, s); })
            : apgp_by_dpad(kc.dpad, [&](auto dp) { return pt_launch<decltype(dp)::value, false>(q, grid, xbytes, xlds, dev, s); });
        if (rc != 0) return rc;
    }
    APGP_CHECK_LAUNCH();
    return 0;
}
