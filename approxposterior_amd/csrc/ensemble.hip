// On-device affine-invariant ensemble sampler over the GP-mean surrogate: the
// whole MCMC loop of ApproxPosterior.runMCMC (approx.py:839-846) -- emcee's
// stretch move (Goodman & Weare 2010; red/blue split, a = 2) calling
// ApproxPosterior._gpll (approx.py:148-189: log-probability = GP predictive
// mean, -inf outside the prior) once per walker per half-step -- as ONE
// persistent kernel.  The chain is sequential (every half-step depends on the
// previous one) and a half-step is only W/2 mean-only predictions, so on a GPU
// the reference's structure is pure launch/sync latency (~0.1 ms per half-step
// from the host, 4e4 half-steps for the README example); here proposal, RNG
// (Philox4x32-10), prior gate, GP mean and accept test all stay on the device.
// One workgroup = one independent ensemble (grid.x ensembles = replicas, the
// only way this path shards); a wavefront evaluates one
// walker's GP mean with its lanes striding the training points.
// _gpll's lnprior only GATES the chain (a walker is rejected where it is not
// finite; its value rides along as a blob), so the kernels need the prior's
// support alone: an axis-aligned box [lo, hi] whose edges may be infinite.
// Arbitrary Python priors cannot be evaluated here: the caller either asserts
// lnprior == const inside [lo, hi], -inf outside, or passes a product of
// Uniform and Gaussian factors (priors.JointPrior), whose support is the box and
// whose log-density prior_lnprior_kernel below computes over the stored chain.
#include "apgp_common.h"
#include "scratch.h"
#include "ens_moves.h"
#include "draws.h"         // the box's and the prior's argument records and transforms, shared with sobol.hip
#include "ens_body.h"     // EnsArgs and the sampler body the kernels below share with tempering.hip
#include <atomic>
#include <mutex>

// One workgroup of 1024 threads per ensemble: slot t proposes and accepts; wavefront wv takes proposals wv and wv + 16
// through one pass over the training stream (one proposal per pass for D > 8), its lanes striding the rows.
template <int DPAD, bool XLDS, bool ALLMOVES>
__global__ __launch_bounds__(1024) void ensemble_kernel(EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double xsl[];
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double cs[ENS_MAXW][DPAD];      // scaled walker coordinates
    __shared__ double lp[ENS_MAXW];
    __shared__ double qs[ENS_MAXW / 2][DPAD];  // scaled proposals of the active half
    __shared__ double lpq[ENS_MAXW / 2];
    __shared__ double fac[ENS_MAXW / 2];       // log proposal factor of the move
    __shared__ double uacc[ENS_MAXW / 2];
    __shared__ int qok[ENS_MAXW / 2];
    __shared__ int nacc[ENS_MAXW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int W = a.nwalkers, H = W / 2, D = a.ndim;
    const long long ens = blockIdx.x;
    apgp_exp_tab_load(etab);
    double* gc = a.coords + ens * W * D;
    ens_load<DPAD, XLDS, 1024>(a, gc, cs, nacc, xsl, t);
    __syncthreads();

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

    for (int w = wv; w < W; w += 16) {
        double m = gp_mean(cs[w]);
        m = ens_gate(a, cs[w], m);
        if (lane == 0) lp[w] = m;
    }
    __syncthreads();

    const unsigned int k0 = (unsigned int)a.seed, k1 = (unsigned int)(a.seed >> 32) ^ (unsigned int)(ens * 0x9E3779B9u);
    const bool mixed = a.mv.n > 1;
    int mkind = a.mv.kind[0];
    double mp0 = a.mv.p0[0], mp1 = a.mv.p1[0];
    for (long long it = 0; it < a.iterations; ++it) {
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
                    if (lane == 0) lpq[i] = m;
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
                    lpq[i] = m0;
                    if (i1 < H) lpq[i1] = m1;
                }
            }
            __syncthreads();
            if (t < H) ens_accept<DPAD>(t, s_idx(t), cs, lp, nacc, qs, lpq, fac, uacc, qok);
            __syncthreads();
        }
        if (a.chain) ens_store_walkers<DPAD>(a, cs, a.chain + ((it * gridDim.x + ens) * W) * D, W, D, t, 1024);
        if (a.logp_chain && t < W) a.logp_chain[(it * gridDim.x + ens) * W + t] = lp[t];
    }
    ens_store_walkers<DPAD>(a, cs, gc, W, D, t, 1024);
    if (t < W) {
        a.logp[ens * W + t] = lp[t];
        a.naccept[ens * W + t] = nacc[t];
    }
}

// ---------------------------------------------------------------------------
// Round 5: ONE ensemble over SEVERAL workgroups.  The single-workgroup kernel above keeps 255 of 256 compute units idle for
// a lone ensemble (BASELINE config 5: 64 walkers x 2e4 iterations at N = 1152 took 1.4 s, 35 us per half-step, all of it the
// 32 GP means of the half-step on one CU).  Here G workgroups (256 threads = 4 wavefronts each, one per SIMD) share an
// ensemble: every workgroup keeps the whole sampler state and draws the same proposals (the RNG is counter-based: pure
// functions of (seed, iteration, walker)), evaluates the GP mean of ITS proposals (g, g + G, ...; rows split over its four
// wavefronts, partial sums added in a fixed order), publishes them as data-tagged granules ({low word, tag, high word, tag},
// tag = half-step number + 1, write-through stores, two buffers by half-step parity) and reads everybody else's; the accept
// step then runs identically in every workgroup.  One exchange of H doubles per half-step, no flag, no fence.
// All G x E workgroups must be resident at once (the host limits G x E to the device's CUs); every poll is bounded: on
// timeout the workgroup writes NaN log-probabilities and leaves -- the host wrapper re-runs on the single-workgroup kernel.
// ---------------------------------------------------------------------------
struct EnsMwArgs {
    EnsArgs e;
    unsigned long long* xchg;      // [E][2][ENS_MAXW / 2] granules of 2 x 8 bytes
    unsigned long long* status;    // sticky "a workgroup gave up" word of this launch (zeroed with xchg)
    unsigned long long timeout;    // 100 MHz ticks
    int G;
};
typedef unsigned int ens_u32x4 __attribute__((ext_vector_type(4)));

template <int DPAD, bool XLDS, bool ALLMOVES>
__global__ __launch_bounds__(256) void ensemble_mw_kernel(EnsMwArgs q) {
    const EnsArgs& a = q.e;
    extern __shared__ __attribute__((aligned(16))) double xsl[];
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double cs[ENS_MAXW][DPAD];
    __shared__ double lp[ENS_MAXW];
    __shared__ double qs[ENS_MAXW / 2][DPAD];
    __shared__ double lpq[ENS_MAXW / 2];
    __shared__ double fac[ENS_MAXW / 2];
    __shared__ double uacc[ENS_MAXW / 2];
    __shared__ double part[4][2];              // partial sums of the (at most two) proposals in flight, per wavefront
    __shared__ int qok[ENS_MAXW / 2];
    __shared__ int nacc[ENS_MAXW];
    __shared__ int gaveup;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int W = a.nwalkers, H = W / 2, D = a.ndim, G = q.G;
    const long long ens = blockIdx.x / G;
    const int g = (int)(blockIdx.x % G);
    apgp_exp_tab_load(etab);
    double* gc = a.coords + ens * W * D;
    ens_load<DPAD, XLDS, 256>(a, gc, cs, nacc, xsl, t);
    if (t == 0) gaveup = 0;
    __syncthreads();
    // GP means of one or two points by the WHOLE workgroup: row k goes to thread k mod 256 (wavefront (k / 64) mod 4), each
    // wavefront butterflies its lanes, the four partial sums are added 0 + 1 + 2 + 3
    auto gp_mean_wg = [&](const double* p0, const double* p1, const bool two, double& m0, double& m1) {
        double t0[DPAD], t1[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) { t0[d] = p0[d]; t1[d] = two ? p1[d] : p0[d]; }
        double acc0, acc1;
        ens_rows2<DPAD>(a, XLDS ? (const double*)xsl : a.xs, etab, t0, t1, t, 256, acc0, acc1);
        if (lane == 0) { part[wv][0] = acc0; part[wv][1] = acc1; }
        __syncthreads();
        m0 = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0] + a.mean;
        m1 = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1] + a.mean;
        __syncthreads();
    };
    // start-up: every workgroup evaluates every walker (once per launch; keeps the state replicated without an exchange)
    for (int w = 0; w < W; w += 2) {
        double m0, m1;
        gp_mean_wg(cs[w], cs[w + 1 < W ? w + 1 : w], w + 1 < W, m0, m1);
        if (t == 0) {
            lp[w] = ens_gate(a, cs[w], m0);
            if (w + 1 < W) lp[w + 1] = ens_gate(a, cs[w + 1], m1);
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)(q.xchg + ens * 2 * (ENS_MAXW / 2) * 2), 0,
                                                                          2 * (ENS_MAXW / 2) * 16, 0x00020000);
    const unsigned int k0 = (unsigned int)a.seed, k1 = (unsigned int)(a.seed >> 32) ^ (unsigned int)(ens * 0x9E3779B9u);
    const bool mixed = a.mv.n > 1;
    int mkind = a.mv.kind[0];
    double mp0 = a.mv.p0[0], mp1 = a.mv.p1[0];
    bool dead = false;
    for (long long it = 0; it < a.iterations && !dead; ++it) {
        const int rot = ens_iteration(a.mv, mixed, it, k0, k1, W, mkind, mp0, mp1);
        for (int split = 0; split < 2; ++split) {
            auto s_idx = [&](int i) { return ens_slot(i, split, H, rot, W); };
            auto c_idx = [&](int i) { return ens_slot(i, 1 - split, H, rot, W); };
            if (t < H) {
                qok[t] = ens_propose<DPAD, ALLMOVES>(mkind, mp0, mp1, cs, s_idx(t), c_idx, H, D, a.lo, a.hi, it, split, t, k0, k1, qs[t],
                                           fac[t], uacc[t]) ? 1 : 0;
            }
            __syncthreads();
            // this workgroup's proposals g, g + G, ... (two per pass over the training stream), published as they are done
            const unsigned step = (unsigned)(2 * it + split);
            const unsigned tag = step + 1u;
            const unsigned par = step & 1u;
            for (int i = g; i < H; i += 2 * G) {
                const int i1 = i + G;
                const bool ok0 = qok[i] != 0, ok1 = i1 < H && qok[i1] != 0;
                double m0 = -INFINITY, m1 = -INFINITY;
                if (ok0 || ok1) {
                    double r0, r1;
                    gp_mean_wg(qs[ok0 ? i : i1], qs[ok1 ? i1 : i], ok0 && ok1, r0, r1);
                    if (ok0) m0 = r0;
                    if (ok1) m1 = ok0 ? r1 : r0;
                }
                if (t < 2 && (t == 0 || i1 < H)) {
                    const double mv = t == 0 ? m0 : m1;
                    const int slot = t == 0 ? i : i1;
                    const ens_u32x4 gr = {(unsigned)__double2loint(mv), tag, (unsigned)__double2hiint(mv), tag};
                    APGP_STORE16(gr, rs_x, (unsigned)((par * (ENS_MAXW / 2) + slot) * 16), 0, 16);
                }
            }
            // everybody's values (one granule per thread, polled until its tag is this half-step's)
            if (t < H) {
                ens_u32x4 gr;
                unsigned long long t0 = 0;
                unsigned itn = 0;
                for (;;) {
                    gr = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((par * (ENS_MAXW / 2) + t) * 16), 0, 16);
                    if (gr.y == tag && gr.w == tag) break;
                    if ((++itn & 63u) == 0) {
                        if (*(volatile int*)&gaveup) break;
                        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                        if (t0 == 0) t0 = now;
                        else if (now - t0 > q.timeout) { gaveup = 1; break; }
                    }
                }
                lpq[t] = __hiloint2double((int)gr.z, (int)gr.x);
            }
            __syncthreads();
            if (gaveup) { dead = true; break; }
            if (t < H) ens_accept<DPAD>(t, s_idx(t), cs, lp, nacc, qs, lpq, fac, uacc, qok);
            __syncthreads();
        }
        if (dead) break;
        // the chain: every workgroup writes its share of the walkers
        const long long E_ = gridDim.x / G;
        if (a.chain) ens_store_walkers<DPAD>(a, cs, a.chain + ((it * E_ + ens) * W) * D, W, D, g * 256 + t, G * 256);
        if (a.logp_chain && g == 0 && t < W) a.logp_chain[(it * E_ + ens) * W + t] = lp[t];
    }
    // A workgroup that gave up raises the launch's sticky word: its NaN marker in logp alone could be overwritten by the
    // ensemble's workgroup 0 finishing normally a moment later (it has every granule it needs) while part of the last chain
    // rows was never written; ens_mark_failed_kernel, behind this launch on the stream, turns the word
    // into NaN log-probabilities for every ensemble -- the marker the host looks at can no longer be lost.
    if (dead && t == 0) atomicOr(q.status, 1ull);
    if (g == 0 || dead) {
        ens_store_walkers<DPAD>(a, cs, gc, W, D, t, 256);
        if (t < W) {
            a.logp[ens * W + t] = dead ? __longlong_as_double(0x7ff8000000000000ll) : lp[t];
            a.naccept[ens * W + t] = nacc[t];
        }
    }
}

__global__ __launch_bounds__(256) void ens_mark_failed_kernel(const unsigned long long* status, double* logp, int count) {
    if (*status == 0ull) return;
    for (int i = threadIdx.x; i < count; i += 256) logp[i] = __longlong_as_double(0x7ff8000000000000ll);
}

// 0 = several workgroups per ensemble where that helps and fits (default) | 1 = the single-workgroup kernel only.
// A test / profiling switch, not read from the environment.  Returns the previous value.
static std::atomic<int> g_ens_mode{0};
extern "C" int apgp_ensemble_mode(int mode) {
    if (mode < 0) return g_ens_mode.load();
    return g_ens_mode.exchange(mode ? 1 : 0);
}

// The launch of one kernel (MW: the multi-workgroup one) in one instantiation: per padded dimension and, AM, per "holds
// every move" / "stretch only".  The LDS-resident form (xlds) needs > 64 KiB of dynamic LDS: a per-device attribute, set and
// CHECKED once per device and instantiation.  (The kernels land in the code object in the order they are first named:
// LDS-resident form first here, AM = true first in ens_dispatch, the multi-workgroup kernel first in its caller.)
template <bool MW, int DP, bool AM, class Args>
static int ens_launch(const Args& q, dim3 grid, size_t xbytes, bool xlds, int dev, hipStream_t s) {
    static ApgpLdsOnce once;
    void (*kl)(Args), (*kg)(Args);
    if constexpr (MW) { kl = ensemble_mw_kernel<DP, true, AM>; kg = ensemble_mw_kernel<DP, false, AM>; }
    else { kl = ensemble_kernel<DP, true, AM>; kg = ensemble_kernel<DP, false, AM>; }
    if (xlds && apgp_raise_lds(once, "apgp_ensemble_sample_moves", dev, 96 * 1024, {(const void*)kl}) != 0) return -2;
    hipLaunchKernelGGL(xlds ? kl : kg, grid, dim3(MW ? 256 : 1024), xlds ? xbytes : 0, s, q);
    return 0;
}
template <bool MW, class Args>
static int ens_dispatch(int dpad, bool allmoves, const Args& q, dim3 grid, size_t xbytes, bool xlds, int dev, hipStream_t s) {
    return allmoves
        ? apgp_by_dpad(dpad, [&](auto dp) { return ens_launch<MW, decltype(dp)::value, true>(q, grid, xbytes, xlds, dev, s); })
        : apgp_by_dpad(dpad, [&](auto dp) { return ens_launch<MW, decltype(dp)::value, false>(q, grid, xbytes, xlds, dev, s); });
}

extern "C" int apgp_ensemble_sample_moves(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                          const double* lo, const double* hi, int32_t nwalkers,
                                          int32_t nensembles, int64_t iterations, double a_stretch,
                                          uint64_t seed, double* coords, double* logp, double* chain,
                                          double* logp_chain, int64_t* naccept, int mode,
                                          const apgp_ens_move_t* moves, int32_t nmoves, void* stream) {
    APGP_CHECK_ARG(xs && kern && lo && hi && coords && logp && naccept, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N && iterations >= 0 && nensembles >= 1, "n, iterations, nensembles");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(nwalkers >= 2 && nwalkers % 2 == 0 && nwalkers <= ENS_MAXW, "nwalkers must be even and <= 256");
    APGP_CHECK_ARG(nwalkers >= 2 * kc.ndim, "nwalkers must be at least twice the dimension");
    EnsMoves mv;
    const char* bad = ens_move_table(mv, moves, nmoves, a_stretch, kc.ndim, nwalkers);
    APGP_CHECK_ARG(bad == nullptr, bad);
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(kc.sc[d] > 0.0, "inverse metric must be positive");
    // the kernel for THIS call (mode 0: several workgroups per ensemble where that helps, 1: the single-workgroup kernel,
    // < 0: the process-wide switch apgp_ensemble_mode)
    // a table of stretch entries only runs the kernels that hold no other move
    bool allmoves = false;
    for (int m = 0; m < mv.n; ++m) allmoves = allmoves || mv.kind[m] != APGP_ENS_MOVE_STRETCH;
    const int ens_mode = mode < 0 ? g_ens_mode.load() : (mode ? 1 : 0);
    const EnsArgs a = ens_args(xs, n, kc, mean, lo, hi, nwalkers, iterations, seed, coords, logp, chain, logp_chain, naccept, mv);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nensembles);
    const size_t xbytes = (size_t)a.n * (kc.dpad + 2) * sizeof(double);
    // (D > 16: the sampler state alone takes 100 KB of LDS -- the training stream stays in L2)
    const bool xlds = xbytes <= 96 * 1024 && kc.dpad <= 16;
    {
        // several workgroups per ensemble (ensemble_mw_kernel) when the ensembles alone leave compute units idle: G = the
        // proposals of a half-step, at most (CUs / ensembles), at least 2; every workgroup must be resident (one per CU
        // with the training stream in LDS)
        int devn = 0, cus = 0;
        if (ens_mode == 0 && hipGetDevice(&devn) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devn) == hipSuccess && devn >= 0 && devn < 64) {
            int G = nwalkers / 2;
            if ((long long)G * nensembles > cus) G = cus / nensembles;
            if (G >= 2 && iterations > 0) {
                std::lock_guard<std::mutex> lock(apgp_stream_lock(s));
                const size_t words = (size_t)nensembles * 2 * (ENS_MAXW / 2) * 2 + 8;      // (+ the status word)
                unsigned long long* xchg = (unsigned long long*)apgp_stream_scratch(4, s, words);
                if (!xchg || hipMemsetAsync(xchg, 0, words * 8, s) != hipSuccess) {
                    apgp_set_error("apgp_ensemble_sample_moves: exchange buffer");
                    return -2;
                }
                EnsMwArgs q;
                q.e = a; q.xchg = xchg; q.status = xchg + (words - 8); q.timeout = 5000000ull; q.G = G;      // 50 ms of the 100 MHz clock
                const dim3 gridm((unsigned)(nensembles * G));
                const int rc = ens_dispatch<true>(kc.dpad, allmoves, q, gridm, xbytes, xlds, devn, s);
                if (rc != 0) return rc;
                hipLaunchKernelGGL(ens_mark_failed_kernel, dim3(1), dim3(256), 0, s, q.status, logp, (int)(nensembles * nwalkers));
                APGP_CHECK_LAUNCH();
                return 0;
            }
        }
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        apgp_set_error("apgp_ensemble_sample_moves: hipGetDevice failed");
        return -2;
    }
    const int rc = ens_dispatch<false>(kc.dpad, allmoves, a, grid, xbytes, xlds, dev, s);
    if (rc != 0) return rc;
    APGP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// Candidate matrix of the acquisition sweep drawn ON the device (round 5; opt-in, ApproxPosterior(deviceCandidates)):
// the reference's point search starts from ``priorSample`` draws (utility.py:334-338); the batched counterpart
// sweeps M of them, and drawing 1e6 x 8 uniforms with NumPy + the H2D copy cost more than the sweep itself at
// C5's sizes (26 ms vs 18 ms).  Row i of the GLOBAL matrix is a pure function of (seed, i): counter-based
// Philox4x32-10, counter = (i low, i high, d / 2, 0x43414e44 "CAND"), key = seed -- so rank r of a sharded sweep
// generates exactly its rows [lo, hi) with idx_offset = lo, and anybody can regenerate the winning row alone.
//   T[i][d] = lo[d] + (hi[d] - lo[d]) * u,  u = 53-bit uniform in (0, 1) (u01 above).
// (BoxArgs and the bounds' checks: draws.h, shared with the Sobol generator of sobol.hip)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void box_candidates_kernel(BoxArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const unsigned long long g = (unsigned long long)(a.idx_offset + i);
    double* row = a.T + i * a.ndim;
    for (int d = 0; d < a.ndim; d += 2) {
        unsigned int c[4] = {(unsigned int)g, (unsigned int)(g >> 32), (unsigned int)(d >> 1), 0x43414e44u};
        philox4x32(c, (unsigned int)a.seed, (unsigned int)(a.seed >> 32));
        row[d] = fma(a.span[d], u01(c[0], c[1]), a.lo[d]);
        if (d + 1 < a.ndim) row[d + 1] = fma(a.span[d + 1], u01(c[2], c[3]), a.lo[d + 1]);
    }
}

extern "C" int apgp_box_candidates(double* T, int64_t m, int32_t ndim, const double* lo, const double* hi,
                                   uint64_t seed, int64_t idx_offset, void* stream) {
    APGP_CHECK_ARG(T && lo && hi, "null pointer");
    APGP_CHECK_ARG(m >= 0 && idx_offset >= 0, "m >= 0 and idx_offset >= 0 required");
    APGP_CHECK_ARG(ndim >= 1 && ndim <= APGP_MAX_DIM, "1 <= ndim <= APGP_MAX_DIM required");
    if (m == 0) return 0;
    BoxArgs a;
    const char* bad = box_args(a, ndim, lo, hi);
    APGP_CHECK_ARG(bad == nullptr, bad);
    a.T = T; a.m = m; a.idx_offset = idx_offset; a.seed = seed;
    hipLaunchKernelGGL(box_candidates_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    APGP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// Candidates drawn from a product prior of Uniform and Gaussian factors (priors.JointPrior), and its log-density.
// The stream is box_candidates_kernel's: the same counter (row low, row high, d / 2, "CAND"), key and pairing of
// dimensions, so a Uniform dimension is bit-identical to the box draw of the same row and sharding by idx_offset is
// unchanged.  A Gaussian dimension turns the same u into the reference's inverse-CDF expression (priors.py
// GaussianPrior.transform_uniform), evaluated with explicit roundings in the order NumPy evaluates it:
//   x = mu + (sigma * sqrt(2)) * erfcinv(2 * (1 - u)).
// prior_lnprior_kernel is JointPrior.batch on the device: per row, sum over d of lc[d] (= -log(high - low), or
// -log(sigma) - log(2 pi) / 2) minus z^2 / 2 for Gaussian dimensions, z = (x - mu) / sigma; -inf for a non-finite
// coordinate or one outside a Uniform factor's [low, high].
// ---------------------------------------------------------------------------
// (PriorArgs, prior_draw and the factors' checks prior_args: draws.h, shared with the Sobol generator of sobol.hip)
__global__ __launch_bounds__(256) void prior_candidates_kernel(PriorArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.m; i += (long long)gridDim.x * 256) {
        const unsigned long long g = (unsigned long long)(a.idx_offset + i);
        double* row = a.T + i * a.ndim;
        for (int d = 0; d < a.ndim; d += 2) {
            unsigned int c[4] = {(unsigned int)g, (unsigned int)(g >> 32), (unsigned int)(d >> 1), 0x43414e44u};
            philox4x32(c, (unsigned int)a.seed, (unsigned int)(a.seed >> 32));
            row[d] = prior_draw(a, d, u01(c[0], c[1]));
            if (d + 1 < a.ndim) row[d + 1] = prior_draw(a, d + 1, u01(c[2], c[3]));
        }
    }
}

__global__ __launch_bounds__(256) void prior_lnprior_kernel(PriorArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.m; i += (long long)gridDim.x * 256) {
        const double* row = a.T + i * a.ndim;
        double s = 0.0;
        bool in = true;
        for (int d = 0; d < a.ndim; ++d) {
            const double x = row[d];
            if (!isfinite(x)) in = false;
            if (a.kind[d] == APGP_PRIOR_UNIFORM) {
                if (!(x >= a.p0[d] && x <= a.p1[d])) in = false;
                s += a.lc[d];
            } else {
                const double z = (x - a.p0[d]) / a.p1[d];
                s += a.lc[d] - 0.5 * z * z;
            }
        }
        a.out[i] = in ? s : -INFINITY;
    }
}

static inline unsigned prior_grid(long long m) {
    const long long b = (m + 255) / 256;
    return (unsigned)(b < 65536 ? b : 65536);
}

extern "C" int apgp_prior_candidates(double* T, int64_t m, int32_t ndim, const int32_t* kind, const double* p0,
                                     const double* p1, uint64_t seed, int64_t idx_offset, void* stream) {
    APGP_CHECK_ARG(T && kind && p0 && p1, "null pointer");
    APGP_CHECK_ARG(m >= 0 && idx_offset >= 0, "m >= 0 and idx_offset >= 0 required");
    PriorArgs a;
    const char* bad = prior_args(a, ndim, kind, p0, p1, true);
    APGP_CHECK_ARG(bad == nullptr, bad);
    if (m == 0) return 0;
    a.T = T; a.out = nullptr; a.m = m; a.idx_offset = idx_offset; a.seed = seed;
    hipLaunchKernelGGL(prior_candidates_kernel, dim3(prior_grid(m)), dim3(256), 0, (hipStream_t)stream, a);
    APGP_CHECK_LAUNCH();
    return 0;
}

extern "C" int apgp_prior_lnprior(const double* X, int64_t m, int32_t ndim, const int32_t* kind, const double* p0,
                                  const double* p1, double* out, void* stream) {
    APGP_CHECK_ARG(X && kind && p0 && p1 && out, "null pointer");
    APGP_CHECK_ARG(m >= 0, "m >= 0 required");
    PriorArgs a;
    const char* bad = prior_args(a, ndim, kind, p0, p1, false);
    APGP_CHECK_ARG(bad == nullptr, bad);
    if (m == 0) return 0;
    a.T = (double*)X; a.out = out; a.m = m; a.idx_offset = 0; a.seed = 0;
    hipLaunchKernelGGL(prior_lnprior_kernel, dim3(prior_grid(m)), dim3(256), 0, (hipStream_t)stream, a);
    APGP_CHECK_LAUNCH();
    return 0;
}

// apgp_ensemble_sample with the kernel chosen PER CALL (mode 0: several workgroups per ensemble where that helps, 1: the
// single-workgroup kernel, < 0: the process-wide switch apgp_ensemble_mode): the re-run after a give-up (NaN in logp) does
// not change what other threads' calls get.  Both are apgp_ensemble_sample_moves with the stretch move alone.
extern "C" int apgp_ensemble_sample_ex(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                       const double* lo, const double* hi, int32_t nwalkers,
                                       int32_t nensembles, int64_t iterations, double a_stretch,
                                       uint64_t seed, double* coords, double* logp, double* chain,
                                       double* logp_chain, int64_t* naccept, int mode, void* stream) {
    const apgp_ens_move_t one = {APGP_ENS_MOVE_STRETCH, 1.0, a_stretch, 0.0};
    return apgp_ensemble_sample_moves(xs, n, kern, mean, lo, hi, nwalkers, nensembles, iterations, a_stretch, seed, coords,
                                      logp, chain, logp_chain, naccept, mode, &one, 1, stream);
}

extern "C" int apgp_ensemble_sample(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                    const double* lo, const double* hi, int32_t nwalkers,
                                    int32_t nensembles, int64_t iterations, double a_stretch,
                                    uint64_t seed, double* coords, double* logp, double* chain,
                                    double* logp_chain, int64_t* naccept, void* stream) {
    return apgp_ensemble_sample_ex(xs, n, kern, mean, lo, hi, nwalkers, nensembles, iterations, a_stretch, seed, coords,
                                   logp, chain, logp_chain, naccept, -1, stream);
}
