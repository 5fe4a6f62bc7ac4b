// Nested sampling (Skilling 2006) over the GP-mean surrogate, whole runs on the device: the evidence counterpart of
// ensemble.hip / tempering.hip / hmc.hip.  The likelihood is L = exp(mu), the prior measure is uniform on the finite box
// [lo, hi] (the measure of evidence(proposal="box")), and a run compresses from the box towards the modes wherever they
// are: no proposal, no temperature ladder and no step size come from outside.  A run is a long sequential chain of
// constrained moves, each costing one GP mean (N kernel values): driven from the host it would be a launch and a round
// trip per replaced point; here the ordering, the deaths, the constrained walks and the running evidence stay in one kernel.
//
// include/apgp.h (apgp_nested_sample) fixes the algorithm and tests/nested_ref.py restates it; this file implements that
// text.  In short, for run r (Philox keys (seed, seed >> 32 ^ r 0x9E3779B9), so a run does not depend on nruns):
//   start    nlive points th = min(fma(hi - lo, u, lo), hi), u from tag 11; logL = mu(th sc) in ensemble_kernel's
//            gp_mean order (ens_rows1 with the lanes of one wavefront striding the rows): the bits that
//            apgp_ensemble_sample(iterations = 0, mode = 1) writes for the same coordinates
//   batch b  order the live points by (logL, slot); the first `batch` die (written out with their logL and birth
//            threshold), L* = the largest logL among them; walker i refills the slot of dead point i: it starts at
//            survivor (tag 12) and takes nsteps steps q' = q + gamma0 (1 + sigma n)(c_a - c_b), a != b survivors (tag
//            13), n normal (tag 14), made canonical (th' = q' / sc, q'' = th' sc: what is stored gives back the
//            evaluated point exactly), accepted iff th' is finite, inside the box and mu(q'') > L*
//   stop     before batch b >= 1 if logaddexp(logZ, Lmax + logX) - logZ < dlogz (dlogz > 0), and at max_batches; the
//            live points are then written out in (logL, slot) order, marked final.
//
// Schedule.  One workgroup of 16 wavefronts per run, a wavefront per walker (1 <= batch <= 16).  Lane d of a walker's
// wavefront keeps dimension d of its position; the proposal goes through LDS to ens_rows1, whose lanes stride the
// training rows.  The survivors are frozen for a batch: walkers read survivors' slots and write dead slots only.
// The live coordinates and birth thresholds sit in the run's slice of `work` (L2: 3 rows are read per step against N
// training rows), logL and the order in LDS: 48 KiB for the 4096 slots allowed, under 55 KiB with the rest of the
// state, beside up to 96 KiB of training stream (ens_load's rule): within the 160 KiB of a gfx950 compute unit.
// The order is a bitonic sort of slot indices under the strict total order (logL, slot), padding last: fixed order, no
// atomics, the same inputs give the same bits.
//
// Safety.  No spin, no poll, no wait on another workgroup: nothing is exchanged between runs.  Every loop is bounded by
// max_batches, batch, nsteps, nlive (the sort: log2^2 of nlive rounded up to a power of two) or the training rows.  Every
// barrier is reached by all 1024 threads: the stop decision is one LDS word read by all after a barrier.  logL never
// holds a NaN (a NaN start value is stored as -inf, a NaN proposal is never accepted), so the order is total and the
// first nlive entries of the sorted index are real slots: every index into the live set is below nlive.
#include "apgp_common.h"
#include "scratch.h"
#include "ens_moves.h"
#include "ens_body.h"

#define NEST_MAXLIVE 4096
#define NEST_NW 16
#define NEST_TAG_START 11u
#define NEST_TAG_WALKER 12u
#define NEST_TAG_PAIR 13u
#define NEST_TAG_NORMAL 14u

struct NestArgs {
    EnsArgs e;             // the training stream and the kernel's constants (ens_rows1's arguments)
    double* work;          // nruns x nlive x (D + 1): the live points (caller's coordinates), then their birth thresholds
    double* points;        // nruns x cap x D, cap = nlive + batch max_batches
    double* logl;          // nruns x cap
    double* birth;         // nruns x cap
    int* rec;              // nruns x cap: batch of death, -1 for the final live points
    long long* counts;     // nruns x 4: batches done, likelihood calls, accepted steps, stuck walkers
    double* logz;          // nruns x 2: the run's own logZ over its dead points, and logX, when it stopped
    double* trace;         // nruns x max_batches x batch x nsteps x (D + 2) or NULL: every step's th', mu (NaN: not
                           // evaluated, th' left the box) and 1 / 0 for accepted / not
    int nlive, n2, batch, nsteps, max_batches;
    double dlogz, sigma, gamma0;
    double ulo[APGP_MAX_DIM], uhi[APGP_MAX_DIM];      // the box in the caller's coordinates
};

// arr[i] for i < DPAD without indexing the kernel arguments by a register (hmc_pick's reason)
template <int DPAD>
__device__ __forceinline__ double nest_pick(const double (&arr)[APGP_MAX_DIM], const int i) {
    double v = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; ++d) v = i == d ? arr[d] : v;
    return v;
}

// a walker's proposal in dimension `lane`: the canonical scaled coordinate (qn) and the caller's (thp).  Contraction is
// off so that every operation rounds once, as tests/nested_ref.py charges it.
__device__ __forceinline__ void nest_propose(const double gam, const double tha, const double thb, const double qc, const double sc,
                                             double& thp, double& qn) {
#pragma clang fp contract(off)
    const double ca = tha * sc, cb = thb * sc;
    const double qv = fma(gam, ca - cb, qc);
    thp = qv / sc;
    qn = thp * sc;
}

template <int DPAD, bool XLDS>
__global__ __launch_bounds__(NEST_NW * 64) void nested_kernel(NestArgs q) {
    const EnsArgs& a = q.e;
    extern __shared__ __attribute__((aligned(16))) double xsl[];
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double lv[NEST_MAXLIVE];        // logL of the live points
    __shared__ int idx[NEST_MAXLIVE];          // slots in (logL, slot) order
    __shared__ double pq[NEST_NW][DPAD];       // the point a wavefront evaluates (scaled)
    __shared__ double ssc[DPAD], slo[DPAD], shi[DPAD];
    __shared__ long long cnt[NEST_NW][3];
    __shared__ int stop;
    const int NT = NEST_NW * 64;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int D = a.ndim, nl = q.nlive, n2 = q.n2, B = q.batch, ns = nl - B;
    const long long run = blockIdx.x;
    const long long cap = (long long)nl + (long long)B * q.max_batches;
    double* live = q.work + run * nl * (D + 1);
    double* lbirth = live + (long long)nl * D;
    double* pts = q.points + run * cap * D;
    double* ol = q.logl + run * cap;
    double* ob = q.birth + run * cap;
    int* orec = q.rec + run * cap;
    apgp_exp_tab_load(etab);
    if (t < DPAD) {
        ssc[t] = nest_pick<DPAD>(a.sc, t);
        slo[t] = nest_pick<DPAD>(q.ulo, t);
        shi[t] = nest_pick<DPAD>(q.uhi, t);
    }
    if (XLDS) {
        for (long long e = t; e < a.n * (DPAD + 2); e += NT) xsl[e] = a.xs[e];
    }
    const double* xs = XLDS ? (const double*)xsl : a.xs;
    for (int i = t; i < n2; i += NT) idx[i] = i;
    __syncthreads();

    const unsigned int k0 = (unsigned int)a.seed, k1 = (unsigned int)(a.seed >> 32) ^ (unsigned int)(run * 0x9E3779B9u);
    // the start: uniform in the box, two dimensions per counter (as box_candidates_kernel pairs them)
    for (int e = t; e < nl * D; e += NT) {
        const int w = e / D, d = e - w * D;
        unsigned int c[4] = {(unsigned int)w, (unsigned int)(d >> 1), 0u, NEST_TAG_START};
        philox4x32(c, k0, k1);
        const double u = (d & 1) ? u01(c[2], c[3]) : u01(c[0], c[1]);
        live[e] = fmin(fma(shi[d] - slo[d], u, slo[d]), shi[d]);
    }
    for (int i = t; i < nl; i += NT) lbirth[i] = -INFINITY;
    __syncthreads();
    // GP mean of the point in pq[wv], by this wavefront (ensemble_kernel's gp_mean)
    auto gp_mean = [&]() { return ens_rows1<DPAD>(a, xs, etab, pq[wv], lane, 64) + a.mean; };
    const double sc = lane < DPAD ? ssc[lane] : 0.0;
    for (int w = wv; w < nl; w += NEST_NW) {
        if (lane < DPAD) pq[wv][lane] = lane < D ? live[(long long)w * D + lane] * sc : 0.0;
        __builtin_amdgcn_wave_barrier();
        double m = gp_mean();
        if (!(m == m)) m = -INFINITY;
        if (lane == 0) lv[w] = m;
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    // strict total order of slots by (logL, slot); the padding of the power of two comes last
    auto before = [&](const int x, const int y) {
        if (x >= nl || y >= nl) return x < y;
        const double lx = lv[x], ly = lv[y];
        return lx < ly || (lx == ly && x < y);
    };
    const double lo = lane < DPAD ? slo[lane] : 0.0, hi = lane < DPAD ? shi[lane] : 0.0;
    long long ncall = 0, nacc = 0, nstuck = 0;      // of this wavefront's walkers (wave-uniform)
    double logZ = -INFINITY, logX = 0.0;            // thread 0's running sums
    int nb = 0;
    for (;;) {
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < n2; i += NT) {
                    const int p = i ^ j;
                    if (p > i) {
                        const int x = idx[i], y = idx[p];
                        const bool sw = (i & k) == 0 ? before(y, x) : before(x, y);
                        if (sw) { idx[i] = y; idx[p] = x; }
                    }
                }
                __syncthreads();
            }
        }
        if (t == 0) {
            int s = nb >= q.max_batches ? 1 : 0;
            if (!s && nb > 0 && q.dlogz > 0.0) {
                const double r = lv[idx[nl - 1]] + logX;
                const double m = fmax(logZ, r);
                const double lae = m == -INFINITY ? m : m + log(exp(logZ - m) + exp(r - m));
                if (lae - logZ < q.dlogz) s = 1;
            }
            stop = s;
        }
        __syncthreads();
        if (stop) break;
        const double Lstar = lv[idx[B - 1]];
        const long long base = (long long)nb * B;
        for (int e = t; e < B * D; e += NT) {
            const int i = e / D, d = e - i * D;
            pts[(base + i) * D + d] = live[(long long)idx[i] * D + d];
        }
        if (t < B) {
            const int s = idx[t];
            ol[base + t] = lv[s];
            ob[base + t] = lbirth[s];
            orec[base + t] = nb;
        }
        if (t == 0) {
            for (int i = 0; i < B; ++i) {
                const double inv = 1.0 / (double)(nl - i);
                const double lw = lv[idx[i]] + (logX + log(-expm1(-inv)));
                const double m = fmax(logZ, lw);
                logZ = m == -INFINITY ? m : m + log(exp(logZ - m) + exp(lw - m));
                logX -= inv;
            }
        }
        __syncthreads();      // the dead are out before their slots are refilled
        if (wv < B) {
            const int slot = idx[wv];
            unsigned int cw[4] = {(unsigned int)nb, 0xFFFFFFFFu, (unsigned int)wv, NEST_TAG_WALKER};
            philox4x32(cw, k0, k1);
            const int s0 = idx[B + (int)(cw[0] % (unsigned int)ns)];
            double th = lane < D ? live[(long long)s0 * D + lane] : 0.0;
            double qc = th * sc, lc = lv[s0];
            int acc = 0;
            for (int step = 0; step < q.nsteps; ++step) {
                unsigned int cp[4] = {(unsigned int)nb, (unsigned int)step, (unsigned int)wv, NEST_TAG_PAIR};
                philox4x32(cp, k0, k1);
                const int ja = (int)(cp[0] % (unsigned int)ns);
                int jb = (int)(cp[1] % (unsigned int)(ns - 1));
                if (jb >= ja) ++jb;
                const int sa = idx[B + ja], sb = idx[B + jb];
                unsigned int cn[4] = {(unsigned int)nb, (unsigned int)step, (unsigned int)wv, NEST_TAG_NORMAL};
                philox4x32(cn, k0, k1);
                const double nrm = ens_normal(u01(cn[0], cn[1]), u01(cn[2], cn[3]));
                const double gam = __dmul_rn(q.gamma0, __dadd_rn(1.0, __dmul_rn(q.sigma, nrm)));
                double thp = 0.0, qn = 0.0;
                bool bad = false;
                if (lane < D) {
                    nest_propose(gam, live[(long long)sa * D + lane], live[(long long)sb * D + lane], qc, sc, thp, qn);
                    bad = !(isfinite(thp) && thp >= lo && thp <= hi);
                }
                double* tr = q.trace ? q.trace + ((((run * q.max_batches + nb) * B + wv) * q.nsteps + step) * (D + 2)) : nullptr;
                if (tr && lane < D) tr[lane] = thp;
                if (__ballot(bad) != 0ull) {               // wave-uniform
                    if (tr && lane == 0) { tr[D] = __longlong_as_double(0x7ff8000000000000ll); tr[D + 1] = 0.0; }
                    continue;
                }
                if (lane < DPAD) pq[wv][lane] = qn;
                __builtin_amdgcn_wave_barrier();
                const double m = gp_mean();
                __builtin_amdgcn_wave_barrier();
                ++ncall;
                const bool take = m > Lstar;
                if (tr && lane == 0) { tr[D] = m; tr[D + 1] = take ? 1.0 : 0.0; }
                if (take) { qc = qn; th = thp; lc = m; ++acc; }
            }
            if (lane < D) live[(long long)slot * D + lane] = th;
            if (lane == 0) { lv[slot] = lc; lbirth[slot] = Lstar; }
            nacc += acc;
            if (acc == 0) ++nstuck;
        }
        __syncthreads();
        ++nb;
    }
    // the final live points, in order
    const long long base = (long long)nb * B;
    for (int e = t; e < nl * D; e += NT) {
        const int i = e / D, d = e - i * D;
        pts[(base + i) * D + d] = live[(long long)idx[i] * D + d];
    }
    for (int i = t; i < nl; i += NT) {
        const int s = idx[i];
        ol[base + i] = lv[s];
        ob[base + i] = lbirth[s];
        orec[base + i] = -1;
    }
    if (lane == 0) { cnt[wv][0] = ncall; cnt[wv][1] = nacc; cnt[wv][2] = nstuck; }
    __syncthreads();
    if (t == 0) {
        long long s0 = nl, s1 = 0, s2 = 0;
        for (int w = 0; w < NEST_NW; ++w) { s0 += cnt[w][0]; s1 += cnt[w][1]; s2 += cnt[w][2]; }
        q.counts[run * 4 + 0] = nb;
        q.counts[run * 4 + 1] = s0;
        q.counts[run * 4 + 2] = s1;
        q.counts[run * 4 + 3] = s2;
        q.logz[run * 2 + 0] = logZ;
        q.logz[run * 2 + 1] = logX;
    }
}

// the training stream is staged in LDS when it fits beside the sampler state (ens_load's rule)
static inline bool nest_xlds(int64_t n, int dpad) { return (size_t)apgp_npad(n) * (dpad + 2) * sizeof(double) <= 96 * 1024; }

template <int DP>
static int nest_launch(const NestArgs& q, dim3 grid, size_t xbytes, bool xlds, int dev, hipStream_t s) {
    static ApgpLdsOnce once;
    void (*kl)(NestArgs) = nested_kernel<DP, true>;
    void (*kg)(NestArgs) = nested_kernel<DP, false>;
    if (xlds && apgp_raise_lds(once, "apgp_nested_sample", dev, 96 * 1024, {(const void*)kl}) != 0) return -2;
    hipLaunchKernelGGL(xlds ? kl : kg, grid, dim3(NEST_NW * 64), xlds ? xbytes : 0, s, q);
    return 0;
}

static inline bool nest_sizes_ok(int32_t ndim, int32_t nlive, int32_t nruns) {
    return ndim >= 1 && ndim <= APGP_MAX_DIM && nlive >= 4 && nlive <= NEST_MAXLIVE && nruns >= 1 && nruns <= (1 << 20);
}

extern "C" int64_t apgp_nested_work_len(int32_t ndim, int32_t nlive, int32_t nruns) {
    if (!nest_sizes_ok(ndim, nlive, nruns)) return -1;
    return (int64_t)nruns * nlive * (ndim + 1);
}

extern "C" int apgp_nested_xlds(int64_t n, int32_t ndim) {
    if (n < 1 || n > APGP_MAX_N || ndim < 1 || ndim > APGP_MAX_DIM) return -1;
    return nest_xlds(n, apgp_dpad(ndim)) ? 1 : 0;
}

extern "C" int apgp_nested_sample(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean, const double* lo,
                                  const double* hi, int32_t nlive, int32_t batch, int32_t nsteps, int32_t max_batches,
                                  double dlogz, double sigma, double gamma0, int32_t nruns, uint64_t seed, double* work,
                                  double* points, double* logl, double* birth, int32_t* rec, int64_t* counts, double* logz,
                                  double* trace, void* stream) {
    APGP_CHECK_ARG(xs && kern && lo && hi && work && points && logl && birth && rec && counts && logz, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(kc.sc[d] > 0.0 && std::isfinite(kc.sc[d]), "inverse metric must be positive");
    APGP_CHECK_ARG(nest_sizes_ok(kc.ndim, nlive, nruns), "4 <= nlive <= 4096 and 1 <= nruns <= 2^20 required");
    APGP_CHECK_ARG(batch >= 1 && batch <= NEST_NW, "1 <= batch <= 16 required");
    APGP_CHECK_ARG(nlive >= 2 * batch, "nlive >= 2 batch required");
    APGP_CHECK_ARG(nsteps >= 1 && nsteps <= (1 << 20), "1 <= nsteps <= 2^20 required");
    APGP_CHECK_ARG(max_batches >= 1 && max_batches <= (1 << 24), "1 <= max_batches <= 2^24 required");
    APGP_CHECK_ARG(std::isfinite(dlogz) && dlogz >= 0.0, "dlogz must be finite and >= 0");
    APGP_CHECK_ARG(std::isfinite(sigma) && sigma >= 0.0, "sigma must be finite and >= 0");
    APGP_CHECK_ARG(std::isfinite(gamma0) && gamma0 >= 0.0, "gamma0 must be finite and >= 0 (0: the default)");
    for (int d = 0; d < kc.ndim; ++d)
        APGP_CHECK_ARG(std::isfinite(lo[d]) && std::isfinite(hi[d]) && lo[d] < hi[d] && std::isfinite(hi[d] - lo[d]),
                       "the box must be finite and not empty");
    const double cap = (double)nlive + (double)batch * max_batches;
    APGP_CHECK_ARG(cap * nruns * kc.ndim * 8.0 < 9.0e18, "the output is too large");
    APGP_CHECK_ARG(!trace || (double)nruns * max_batches * batch * nsteps * (kc.ndim + 2.0) * 8.0 < 9.0e18, "trace is too large");

    hipStream_t s = (hipStream_t)stream;
    const int dev = apgp_stream_device(s);
    if (dev < 0 || dev >= 64) {
        apgp_set_error("apgp_nested_sample: the stream's device is outside 0 .. 63 or does not answer");
        return -2;
    }
    NestArgs q;
    EnsMoves mv = {};
    (void)&ens_move_table;      // (ens_body.h's table check: this entry has one fixed move)
    q.e = ens_args(xs, n, kc, mean, lo, hi, 0, 0, seed, nullptr, nullptr, nullptr, nullptr, nullptr, mv);
    q.work = work; q.points = points; q.logl = logl; q.birth = birth; q.rec = rec;
    q.counts = (long long*)counts; q.logz = logz; q.trace = trace;
    q.nlive = nlive; q.batch = batch; q.nsteps = nsteps; q.max_batches = max_batches;
    q.n2 = 1;
    while (q.n2 < nlive) q.n2 <<= 1;
    q.dlogz = dlogz; q.sigma = sigma;
    q.gamma0 = gamma0 > 0.0 ? gamma0 : 2.38 / std::sqrt(2.0 * kc.ndim);
    for (int d = 0; d < APGP_MAX_DIM; ++d) {
        q.ulo[d] = d < kc.ndim ? lo[d] : 0.0;
        q.uhi[d] = d < kc.ndim ? hi[d] : 0.0;
    }
    const size_t xbytes = (size_t)q.e.n * (kc.dpad + 2) * sizeof(double);
    const bool xlds = nest_xlds(n, kc.dpad);
    const dim3 grid((unsigned)nruns);
    const int rc = apgp_by_dpad(kc.dpad, [&](auto dp) { return nest_launch<decltype(dp)::value>(q, grid, xbytes, xlds, dev, s); });
    if (rc != 0) return rc;
    APGP_CHECK_LAUNCH();
    return 0;
}
