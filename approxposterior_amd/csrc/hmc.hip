// Hamiltonian Monte Carlo over the GP-mean surrogate, whole chains on the device: the gradient-based counterpart of
// ensemble.hip.  The target is the one the ensemble sampler has -- density exp(mu(theta)) on the box [lo, hi] whose edges
// may be infinite, the prior only gating (ApproxPosterior._gpll) -- and the gradient is nearly free here:
//   d mu / d t_d = sum_n alpha_n d k(t, x_n) / d t_d
// reuses the N kernel values of the mean and adds D FMAs per training row, no factor and no solve.  Driven from the host
// one gradient is a launch and a synchronisation (GP.predict_grad); here momentum draw, L leapfrog steps, reflection at
// the box and the accept test of every iteration stay in one kernel.
//
// Everything is in the kernel's scaled coordinates q = theta * sc (EnsArgs' convention), where the squared-exponential
// term is amp exp(-|q - x_n|^2) and its derivative k_n (-2) (q_d - x_nd); the linear term adds
// lin_coef P (q_d x_d lw_d)^(P - 1) x_d lw_d (predgrad.hip pg_finish_kernel, without its chain-rule factor sc_d).
//
// One iteration of a chain (tests/hmc_ref.py states the recipe; this file implements that text):
//   p_d = ens_normal(u, u') sqrt(m_d)                      Philox tag 8, one counter per dimension
//   eps_it = eps (1 + jitter (2 u - 1))                    tag 9, chain 0's keys: the same for every chain
//   L times:  p += (eps_it / 2) g(q);  q += eps_it p / m;  reflect;  p += (eps_it / 2) g(q)
//             (the kick between two steps is applied as two half kicks, so that a step is a function of (q, p) alone:
//              that is what lets the trace be replayed step by step; g(q) is evaluated once per step)
//   the last drift's end point is made canonical before its gradient: th = clamp(q / sc), q = th sc (see the kernel)
//   reflect:  while q_d is outside a FINITE face: q_d = 2 face - q_d, p_d = -p_d, at most HMC_MAX_REFLECT times;
//             still outside after that, or a non-finite q or p: the trajectory is a divergence
//   dH = (K(p_L) - mu(q_L)) - (K(p_0) - mu(q_0)),  K = sum_d p_d^2 (0.5 / m_d)
//   accept iff log u < -dH (tag 10); non-finite dH or dH > 1000: rejected and counted as a divergence;
//   a start outside the box has mu = -inf (ens_gate's rule): that chain never moves, accepts and diverges never.
//
// Schedule.  A workgroup is HMC_NW wavefronts, a chain belongs to a group of G of them (HMC_NW / G chains per workgroup, grid =
// ceil(C / chains per workgroup)); no workgroup waits for another.  Every wavefront of a group keeps the chain's state,
// dimension d in lane d (q, p, gradient, mass, faces: a handful of registers whatever D), and all of them update it with
// the same operations.  For a gradient the group's G * 64 lanes stride the training rows with D + 1 running sums each
// (mean and D derivatives; two-accumulator distance sum and apgp_exp as everywhere), a butterfly reduces within the
// wavefront, lane 0 writes the D + 1 sums to LDS, one workgroup barrier, and every wavefront adds its group's partials
// in the order 0, 1, ..., G - 1 (two LDS buffers by parity: one barrier per gradient).  The barrier is uniform: every
// chain of a call takes the same L, and a chain past the end of the list does the arithmetic of the last chain and
// stores nothing.  No atomics, every sum in a fixed order: the same (inputs, G) give the same bits.
// HMC_NW is 4 and G is 1 or 4 at every dimension, which leaves a lane 512 registers: the row loop needs 159 at DPAD 2 and 256
// plus accumulation registers at DPAD 32.  G = 16 would take a 16-wavefront workgroup and its 128 registers a lane; built
// that way the kernel spilled to scratch at every width, DPAD 2 included, so it is not offered
// (profiles/hmc_kernel_resources.txt).
#include "apgp_common.h"
#include "scratch.h"
#include "ens_moves.h"

#define HMC_MAX_REFLECT 8

struct HmcArgs {
    const double* xs;      // packed training stream: Npad x (DPAD+2): scaled x | alpha | 0
    double* coords;        // C x D (in: start, out: final state of the chains that moved)
    double* logp;          // C
    double* chain;         // iterations x C x D or NULL
    double* logp_chain;    // iterations x C or NULL
    long long* naccept;    // C
    double* accprob;       // C
    long long* ndiverge;   // C
    double* prop;          // iterations x C x D or NULL
    double* dH;            // iterations x C or NULL
    double* trace;         // iterations x C x nleap x 2 D or NULL (scaled coordinates)
    long long n, iterations, it0;
    int ndim, lin_order, nchains, nleap, G, has_box;      // (has_box: apgp_fill_box writes it; the call always has a box)
    unsigned long long seed;
    double mean, amp, lin_coef, eps, jitter;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
    double sqm[APGP_MAX_DIM], minv[APGP_MAX_DIM];      // sqrt(m_d), 1 / m_d (scaled coordinates)
};

// arr[lane] for lane < DPAD without indexing the kernel arguments by a register (that would copy them to scratch)
template <int DPAD>
__device__ __forceinline__ double hmc_pick(const double (&arr)[APGP_MAX_DIM], const int lane, const double other) {
    double v = other;
#pragma unroll
    for (int d = 0; d < DPAD; ++d) v = lane == d ? arr[d] : v;
    return v;
}

__device__ __forceinline__ double hmc_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

#define HMC_NW 4
template <int DPAD, bool XLDS, bool LIN>
__global__ __launch_bounds__(HMC_NW * 64) void hmc_kernel(HmcArgs a) {
    extern __shared__ __attribute__((aligned(16))) double xsl[];
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ double part[2][HMC_NW][DPAD + 1];
    __shared__ double slw[DPAD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int D = a.ndim, G = a.G, L = a.nleap, P = a.lin_order;
    const int cl = wv / G, gw = wv - cl * G;               // chain of the workgroup, wavefront of the group
    const long long C = a.nchains;
    const long long cfull = (long long)blockIdx.x * (HMC_NW / G) + cl;
    const bool live = cfull < C;
    const long long c = live ? cfull : C - 1;
    const bool writer = live && gw == 0 && lane < D;        // lane d of the group's first wavefront stores dimension d
    const bool head = live && gw == 0 && lane == 0;
    apgp_exp_tab_load(etab);
    if (t < DPAD) slw[t] = hmc_pick<DPAD>(a.lw, t, 0.0);
    if (XLDS) {
        for (long long e = t; e < a.n * (DPAD + 2); e += HMC_NW * 64) xsl[e] = a.xs[e];
    }
    const double* xs = XLDS ? (const double*)xsl : a.xs;

    const double sc = hmc_pick<DPAD>(a.sc, lane, 0.0);
    const double lo = hmc_pick<DPAD>(a.lo, lane, 0.0) * sc, hi = hmc_pick<DPAD>(a.hi, lane, 0.0) * sc;   // scaled faces
    const double sqm = hmc_pick<DPAD>(a.sqm, lane, 1.0), minv = hmc_pick<DPAD>(a.minv, lane, 1.0);
    const double hm = 0.5 * minv;
    const bool dim = lane < D;
    // The state is kept twice: th in the caller's coordinates and q = th * sc.  The end point of a trajectory is made
    // canonical -- th = q / sc clamped to the box, q = th * sc -- BEFORE its mean and gradient are evaluated, so that
    // what is stored is exactly what the next call starts from: a run cut into calls is the uncut run, bit for bit.
    const double ulo = hmc_pick<DPAD>(a.lo, lane, 0.0), uhi = hmc_pick<DPAD>(a.hi, lane, 0.0);
    double th = dim ? a.coords[c * D + lane] : 0.0;
    double q = th * sc;
    double p = 0.0;
    __syncthreads();

    int par = 0;
    // mu(q) (every lane) and d mu / d q_d (lane d) of the group's chain; one workgroup barrier
    auto eval = [&](const double qv, double& mu, double& gd) {
        double tt[DPAD], acc[DPAD + 1];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) { tt[d] = __shfl(qv, d); acc[d + 1] = 0.0; }
        acc[0] = 0.0;
        const int nn = (int)a.n;
        for (int k = gw * 64 + lane; k < nn; k += G * 64) {
            const double* xr = xs + k * (DPAD + 2);
            double xv[DPAD];
#pragma unroll
            for (int d = 0; d < DPAD; ++d) xv[d] = xr[d];
            const double al = xr[DPAD];
            double s = 0.0, s3 = 0.0;
#pragma unroll
            for (int d = 0; d < DPAD; d += 2) {
                const double df0 = tt[d] - xv[d], df1 = tt[d + 1] - xv[d + 1];
                s = fma(df0, df0, s);
                s3 = fma(df1, df1, s3);
            }
            const double kse = a.amp * apgp_exp(-(s + s3), etab);
            // the linear term's mean part sum_d (p_d)^P, p_d = t_d x_d lw_d, is summed in the derivative loop below, which
            // needs (p_d)^(P - 1) anyway (a pass of its own, as APGP_LIN_SUM, kept 32 products live and spilled at DPAD 32)
            double ls = P == 0 ? (double)D : 0.0;
            const double m2k = -2.0 * kse;
#pragma unroll
            for (int d = 0; d < DPAD; ++d) {
                double J = m2k * (tt[d] - xv[d]);
                if (LIN && P > 0) {
                    const double xl = xv[d] * slw[d], pd = tt[d] * xl;
                    double pw = 1.0;
                    for (int e = 1; e < P; ++e) pw *= pd;
                    ls = fma(pw, pd, ls);
                    J = fma(a.lin_coef * (double)P * pw, xl, J);
                }
                acc[d + 1] = fma(al, J, acc[d + 1]);
            }
            const double kv = LIN ? fma(a.lin_coef, ls, kse) : kse;
            acc[0] = fma(kv, al, acc[0]);
        }
#pragma unroll
        for (int j = 0; j <= DPAD; ++j) acc[j] = hmc_wave_sum(acc[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j <= DPAD; ++j) part[par][wv][j] = acc[j];
        }
        __syncthreads();
        const double(*pp)[DPAD + 1] = part[par] + cl * G;
        const int j = lane < DPAD ? lane + 1 : 0;
        double sm = pp[0][0], sg = pp[0][j];
        for (int g = 1; g < G; ++g) { sm += pp[g][0]; sg += pp[g][j]; }
        mu = sm + a.mean;
        gd = lane < DPAD ? sg : 0.0;
        par ^= 1;
    };
    auto inside = [&](const double qv) { return __ballot(dim && !(qv >= lo && qv <= hi)) == 0ull; };

    double mu, g;
    eval(q, mu, g);
    if (!inside(q)) mu = -INFINITY;

    const unsigned int k0 = (unsigned int)a.seed, kj = (unsigned int)(a.seed >> 32);
    const unsigned int k1 = kj ^ (unsigned int)((unsigned long long)c * 0x9E3779B9u);
    long long nacc = 0, ndiv = 0;
    double apsum = 0.0;
    for (long long it = 0; it < a.iterations; ++it) {
        const long long gi = a.it0 + it;
        const unsigned int w0 = (unsigned int)gi, w1 = (unsigned int)((unsigned long long)gi >> 32);
        p = 0.0;
        if (dim) {
            unsigned int c8[4] = {w0, w1, (unsigned int)lane, 0x8u};
            philox4x32(c8, k0, k1);
            p = ens_normal(u01(c8[0], c8[1]), u01(c8[2], c8[3])) * sqm;
        }
        unsigned int c9[4] = {w0, w1, 0xFFFFFFFFu, 0x9u};
        philox4x32(c9, k0, kj);
        const double eps = a.eps * (1.0 + a.jitter * (2.0 * u01(c9[0], c9[1]) - 1.0));
        const double he = 0.5 * eps, em = eps * minv;
        const double q0 = q, th0 = th, mu0 = mu, g0 = g;
        const double H0 = hmc_wave_sum((p * p) * hm) - mu0;
        bool bad = false;
        for (int l = 0; l < L; ++l) {
            p = fma(he, g, p);
            q = fma(em, p, q);
            bool out = false;
            if (dim) {
                int r = 0;
                for (; r < HMC_MAX_REFLECT; ++r) {
                    if (q > hi) { q = 2.0 * hi - q; p = -p; }
                    else if (q < lo) { q = 2.0 * lo - q; p = -p; }
                    else break;
                }
                out = !(q >= lo && q <= hi) || !isfinite(p);      // (also a NaN q, and an overflow of the count)
            }
            if (__ballot(out) != 0ull) bad = true;
            if (l == L - 1 && dim) {
                th = fmin(fmax(q / sc, ulo), uhi);
                q = th * sc;
            }
            eval(q, mu, g);
            p = fma(he, g, p);
            if (a.trace && writer) {
                double* tr = a.trace + (((it * C + c) * L + l) * 2) * D;
                tr[lane] = q;
                tr[D + lane] = p;
            }
        }
        const double H1 = hmc_wave_sum((p * p) * hm) - mu;
        const double dH = H1 - H0;
        unsigned int ca[4] = {w0, w1, 0xFFFFFFFEu, 0xAu};
        philox4x32(ca, k0, k1);
        const double lu = log(u01(ca[0], ca[1]));
        const bool gated = mu0 == -INFINITY;
        const bool div = !gated && (bad || !isfinite(dH) || dH > 1000.0);
        const bool acc = !gated && !div && lu < -dH;
        if (a.prop && writer) a.prop[(it * C + c) * D + lane] = bad ? __longlong_as_double(0x7ff8000000000000ll) : th;   // (no end point to show)
        if (a.dH && head) a.dH[it * C + c] = dH;
        if (!gated && !div) apsum += dH <= 0.0 ? 1.0 : exp(-dH);
        if (div) ++ndiv;
        if (acc) ++nacc;
        else { q = q0; th = th0; mu = mu0; g = g0; }
        if (a.chain && writer) a.chain[(it * C + c) * D + lane] = th;
        if (a.logp_chain && head) a.logp_chain[it * C + c] = mu;
    }
    if (writer && a.iterations > 0) a.coords[c * D + lane] = th;       // (a chain that never moved: the caller's own bits)
    if (head) {
        a.logp[c] = mu;
        a.naccept[c] = nacc;
        a.accprob[c] = apsum;
        a.ndiverge[c] = ndiv;
    }
}

// wavefronts per chain the call takes
static inline bool hmc_offered(int g) { return g == 1 || g == 4; }

// The rule for g_rows == 0, from profiles/hmc_timing.json (DESIGN.md "Hamiltonian Monte Carlo"): with one workgroup per
// chain fitting the compute units at once, G = 4 took 0.42x (D = 8, N = 1152, 64 chains), 0.41x (D = 32, N = 1152, 64
// chains) and 0.64x (D = 2, N = 90, 20 chains) the time per leapfrog step of G = 1 -- at every measured size, the smallest
// included -- so the whole workgroup goes to one chain whenever the chains are no more than the compute units.  Beyond
// that a call was NOT measured: G = 1 there keeps the workgroups at a quarter of the count (four chains each).
static int hmc_rule(int64_t nchains, int cus) {
    return nchains <= cus ? 4 : 1;
}

template <int DP, bool LIN>
static int hmc_launch(const HmcArgs& a, dim3 grid, size_t xbytes, bool xlds, int dev, hipStream_t s) {
    static ApgpLdsOnce once;
    void (*kl)(HmcArgs) = hmc_kernel<DP, true, LIN>;
    void (*kg)(HmcArgs) = hmc_kernel<DP, false, LIN>;
    if (xlds && apgp_raise_lds(once, "apgp_hmc_sample", dev, 96 * 1024, {(const void*)kl}) != 0) return -2;
    hipLaunchKernelGGL(xlds ? kl : kg, grid, dim3(HMC_NW * 64), xlds ? xbytes : 0, s, a);
    return 0;
}

extern "C" int apgp_hmc_sample(const double* xs, int64_t n, const apgp_kernel_t* kern, double mean, const double* lo,
                               const double* hi, int32_t nchains, int64_t iterations, const apgp_hmc_options_t* opt,
                               uint64_t seed, double* coords, double* logp, double* chain, double* logp_chain,
                               int64_t* naccept, double* accprob, int64_t* ndiverge, double* prop, double* dH,
                               double* trace, void* stream) {
    APGP_CHECK_ARG(xs && kern && lo && hi && opt && coords && logp && naccept && accprob && ndiverge, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "1 <= n <= APGP_MAX_N required");
    APGP_CHECK_ARG(nchains >= 1 && nchains <= APGP_MAX_N, "1 <= nchains <= 2^24 required");
    APGP_CHECK_ARG(iterations >= 0 && iterations <= APGP_MAX_M, "0 <= iterations <= 2^40 required");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    for (int d = 0; d < kc.ndim; ++d) APGP_CHECK_ARG(kc.sc[d] > 0.0 && std::isfinite(kc.sc[d]), "inverse metric must be positive");
    APGP_CHECK_ARG(std::isfinite(opt->eps) && opt->eps > 0.0, "eps must be finite and > 0");
    APGP_CHECK_ARG(opt->jitter >= 0.0 && opt->jitter < 1.0, "0 <= jitter < 1 required");
    APGP_CHECK_ARG(opt->nleap >= 1 && opt->nleap <= APGP_HMC_MAX_LEAP, "1 <= nleap <= APGP_HMC_MAX_LEAP required");
    APGP_CHECK_ARG(opt->g_rows == 0 || hmc_offered(opt->g_rows), "g_rows must be 0, 1 or 4");
    APGP_CHECK_ARG(opt->iteration0 >= 0 && opt->iteration0 <= (int64_t)1 << 62, "iteration0 must be >= 0");
    for (int d = 0; d < kc.ndim; ++d) {
        APGP_CHECK_ARG(std::isfinite(opt->mass[d]) && opt->mass[d] > 0.0, "mass must be finite and > 0");
        APGP_CHECK_ARG(lo[d] <= hi[d], "lo <= hi required (NaN is refused)");
    }
    // (trace is the largest output: the byte offset of its last element, iterations x C x nleap x 2 D x 8, must stay below 2^63)
    APGP_CHECK_ARG(!trace || (double)iterations * nchains * opt->nleap * 2.0 * kc.ndim * 8.0 < 9.0e18, "trace is too large");

    hipStream_t s = (hipStream_t)stream;
    const int dev = apgp_stream_device(s);
    int cus = 0;
    if (dev < 0 || dev >= 64 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        apgp_set_error("apgp_hmc_sample: the stream's device is outside 0 .. 63 or does not answer");
        return -2;
    }
    HmcArgs a;
    a.xs = xs; a.coords = coords; a.logp = logp; a.chain = chain; a.logp_chain = logp_chain;
    a.naccept = (long long*)naccept; a.accprob = accprob; a.ndiverge = (long long*)ndiverge;
    a.prop = prop; a.dH = dH; a.trace = trace;
    a.n = apgp_npad(n); a.iterations = iterations; a.it0 = opt->iteration0;
    a.nchains = nchains; a.nleap = opt->nleap; a.seed = seed; a.mean = mean; a.eps = opt->eps; a.jitter = opt->jitter;
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    for (int d = 0; d < APGP_MAX_DIM; ++d) {
        a.sqm[d] = d < kc.ndim ? std::sqrt(opt->mass[d]) : 1.0;
        a.minv[d] = d < kc.ndim ? 1.0 / opt->mass[d] : 1.0;
    }
    a.G = opt->g_rows ? opt->g_rows : hmc_rule(nchains, cus);
    const int cpw = HMC_NW / a.G;
    const dim3 grid((unsigned)((nchains + cpw - 1) / cpw));
    const size_t xbytes = (size_t)a.n * (kc.dpad + 2) * sizeof(double);
    const bool xlds = xbytes <= 96 * 1024;                  // ens_load's rule; the state beside it is under 3 KiB
    // (a kernel without a linear term runs the instantiation that holds none: with it compiled in, the products it shares
    // between the mean and the derivatives stay live through the row loop and the DPAD 32 kernel spills)
    const int rc = kc.lin_coef != 0.0
        ? apgp_by_dpad(kc.dpad, [&](auto dp) { return hmc_launch<decltype(dp)::value, true>(a, grid, xbytes, xlds, dev, s); })
        : apgp_by_dpad(kc.dpad, [&](auto dp) { return hmc_launch<decltype(dp)::value, false>(a, grid, xbytes, xlds, dev, s); });
    if (rc != 0) return rc;
    APGP_CHECK_LAUNCH();
    return 0;
}

// the group width apgp_hmc_sample's rule picks for a call of these sizes on the current device (what g_rows = 0 runs)
extern "C" int apgp_hmc_rule(int32_t nchains, int64_t n, int32_t ndim) {
    int dev = 0, cus = 0;
    if (nchains < 1 || n < 1 || n > APGP_MAX_N || ndim < 1 || ndim > APGP_MAX_DIM) return -1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return -2;
    return hmc_rule(nchains, cus);
}
