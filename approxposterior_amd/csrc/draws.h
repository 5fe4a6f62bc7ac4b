// What turns a uniform into a draw, shared by the generators that differ only in where the uniform comes from: the
// Philox streams of ensemble.hip (box, prior) and evidence.hip (mixture) and the Sobol sequence of sobol.hip.  One copy of
// the argument records, of the checks the entry points make before any launch and of the per-row arithmetic, so that a
// Sobol draw is its Philox sibling's transform of another uniform and the two cannot drift apart.
//   box:      T[i][d] = fma(span[d], u, lo[d])
//   prior:    a Uniform factor as the box; a Gaussian factor prior_gauss(mu, sigma, u) (ens_moves.h)
//   mixture:  the first k with u < cumw[k]; z_d = prior_gauss(0, 1, u_d); t = c_k + A_k z; ln q at the stored t
#pragma once
#include "apgp_common.h"
#include "ens_moves.h"
#include "gmm_logpdf.h"
#include "scratch.h"
#include <cmath>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------------
// box
// ---------------------------------------------------------------------------------------------------------------------
struct BoxArgs {
    double* T;
    long long m, idx_offset;
    int ndim;
    unsigned long long seed;
    double lo[APGP_MAX_DIM], span[APGP_MAX_DIM];
};

// the bounds of a box draw; fills lo and span or returns the failed check's message
static inline const char* box_args(BoxArgs& a, int32_t ndim, const double* lo, const double* hi) {
    if (!(ndim >= 1 && ndim <= APGP_MAX_DIM)) return "1 <= ndim <= APGP_MAX_DIM required";
    a.ndim = ndim;
    for (int d = 0; d < APGP_MAX_DIM; ++d) {
        a.lo[d] = d < ndim ? lo[d] : 0.0;
        a.span[d] = d < ndim ? hi[d] - lo[d] : 0.0;
        if (!(d >= ndim || (a.span[d] >= 0.0 && a.span[d] < INFINITY))) return "bounds must be finite with lo <= hi";
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// product prior of Uniform and Gaussian factors
// ---------------------------------------------------------------------------------------------------------------------
#define APGP_PRIOR_UNIFORM 0
#define APGP_PRIOR_GAUSSIAN 1

struct PriorArgs {
    double* T;                 // candidates out (m x ndim) | rows in for the log-density
    double* out;               // log-density out (m), NULL for candidates
    long long m, idx_offset;
    int ndim;
    unsigned long long seed;
    int kind[APGP_MAX_DIM];
    double p0[APGP_MAX_DIM];   // low | mu
    double p1[APGP_MAX_DIM];   // candidates: span | sigma;  log-density: high | sigma
    double lc[APGP_MAX_DIM];   // log-density constant of the factor
};

// (prior_gauss: csrc/ens_moves.h)
__device__ __forceinline__ double prior_draw(const PriorArgs& a, int d, double u) {
    if (a.kind[d] == APGP_PRIOR_UNIFORM) return fma(a.p1[d], u, a.p0[d]);
    return prior_gauss(a.p0[d], a.p1[d], u);
}

// the checks the prior's entries share; fills a (kinds and parameters) or returns the failed check's message
static inline const char* prior_args(PriorArgs& a, int32_t ndim, const int32_t* kind, const double* p0, const double* p1,
                                     bool span) {
    if (!(ndim >= 1 && ndim <= APGP_MAX_DIM)) return "1 <= ndim <= APGP_MAX_DIM required";
    a.ndim = ndim;
    for (int d = 0; d < APGP_MAX_DIM; ++d) {
        a.kind[d] = APGP_PRIOR_UNIFORM;
        a.p0[d] = a.p1[d] = a.lc[d] = 0.0;
        if (d >= ndim) continue;
        const double u = p0[d], v = p1[d];
        if (kind[d] == APGP_PRIOR_UNIFORM) {
            if (!(std::isfinite(u) && std::isfinite(v) && u < v && std::isfinite(v - u)))
                return "a Uniform factor needs finite low < high";
            a.p0[d] = u;
            a.p1[d] = span ? v - u : v;
            a.lc[d] = -std::log(v - u);
        } else if (kind[d] == APGP_PRIOR_GAUSSIAN) {
            if (!(std::isfinite(u) && std::isfinite(v) && v > 0.0)) return "a Gaussian factor needs finite mu and sigma > 0";
            a.kind[d] = APGP_PRIOR_GAUSSIAN;
            a.p0[d] = u;
            a.p1[d] = v;
            a.lc[d] = -std::log(v) - 0.5 * std::log(2.0 * M_PI);
        } else {
            return "kind must be 0 (Uniform) or 1 (Gaussian)";
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian mixture.  Device image of the parameters (DP = the padded dimension):
//   [cumw (MIX_MAX_K)] [per component: log w, log det U, c (DP), U packed in DP columns (gmm_logpdf's layout)]
//   [per component: A packed lower triangle row by row, A[i][j] at i (i + 1) / 2 + j, D (D + 1) / 2 entries]
// ---------------------------------------------------------------------------------------------------------------------
#define MIX_MAX_K 16
#define MIX_SCRATCH_SLOT 6             // the device image of the mixture parameters

constexpr int ev_tri(int d) { return d * (d + 1) / 2; }

struct MixArgs {
    double* T;
    double* lnq;
    const double* P;
    long long m, idx_offset;
    int D, K;
    unsigned long long seed;
};

// the component of the uniform uc: the first k with uc < cumw[k], the last one otherwise
__device__ __forceinline__ int mix_pick(const MixArgs& a, double uc) {
    const double* cumw = a.P;
    int k = a.K - 1;
    for (int j = a.K - 2; j >= 0; --j)
        if (uc < cumw[j]) k = j;
    return k;
}

// Row i of the call from its component k and its standard normals z (zeros past D): t_r = c_r + sum_{j <= r} A_rj z_j (an
// fma chain in ascending j, then one addition), stored; then ln q at the stored t: logsumexp_k(gmm_logpdf(t | k)), the
// arithmetic of gmm_pass_kernel's score.  slp: the workgroup's MIX_MAX_K x 256 doubles of LDS, a column per thread.
template <int DP>
__device__ __forceinline__ void mix_row(const MixArgs& a, long long i, int tid, int k, const double (&z)[DP],
                                        double (*slp)[256]) {
    constexpr int QP = 2 + DP + ev_tri(DP);
    const double* G = a.P + MIX_MAX_K;
    const int triD = ev_tri(a.D);
    const double* A = G + a.K * QP;
    const double* ck = G + k * QP + 2;
    const double* Ak = A + (long long)k * triD;
    double t[DP];
#pragma unroll
    for (int r = 0; r < DP; ++r) {
        t[r] = 0.0;
        if (r < a.D) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j <= r; ++j) acc = fma(Ak[r * (r + 1) / 2 + j], z[j], acc);
            t[r] = __dadd_rn(ck[r], acc);
        }
    }
    double* row = a.T + i * a.D;
#pragma unroll
    for (int d = 0; d < DP; ++d)
        if (d < a.D) row[d] = t[d];
    if (a.lnq) {
        double mx = -INFINITY;
        for (int kk = 0; kk < a.K; ++kk) {
            const double lp = gmm_logpdf<DP>(t, G + kk * QP, a.D);
            slp[kk][tid] = lp;
            if (lp > mx) mx = lp;
        }
        double s = 0.0;
        for (int kk = 0; kk < a.K; ++kk) s += exp(slp[kk][tid] - mx);
        a.lnq[i] = mx + log(s);
    }
}

static inline long long mix_user_len(int D) { return 3 + D + 2 * ev_tri(D); }

// The host side of a mixture draw, for the entry point `fn`: the argument checks (-1 before anything reaches the device),
// the upload of the parameters' device image into per-stream scratch, and launch(MixArgs, DP, grid blocks of 256 rows,
// stream) under the stream's lock.  m == 0 returns 0 after the checks with nothing done.
template <class Launch>
static inline int mix_draw_call(const char* fn, double* T, double* lnq, int64_t m, int32_t ndim, int32_t ncomp,
                                const double* params, uint64_t seed, int64_t idx_offset, void* stream, Launch&& launch) {
#define MIX_CHECK_ARG(cond, msg)                                \
    do {                                                        \
        if (!(cond)) {                                          \
            apgp_set_error("%s: bad argument: %s", fn, msg);    \
            return -1;                                          \
        }                                                       \
    } while (0)
    MIX_CHECK_ARG(T && params, "null pointer");
    MIX_CHECK_ARG(m >= 0 && m <= APGP_MAX_M && idx_offset >= 0, "0 <= m <= APGP_MAX_M and idx_offset >= 0 required");
    MIX_CHECK_ARG(ndim >= 1 && ndim <= APGP_MAX_DIM, "1 <= ndim <= APGP_MAX_DIM required");
    MIX_CHECK_ARG(ncomp >= 1 && ncomp <= MIX_MAX_K, "1 <= ncomp <= 16 required");
    const int D = ndim, K = ncomp, DP = apgp_dpad(ndim), tri = ev_tri(D);
    const int QP = 2 + DP + ev_tri(DP);
    const long long R = mix_user_len(D);
    std::vector<double> img((size_t)MIX_MAX_K + (size_t)K * QP + (size_t)K * tri, 0.0);
    double prev = 0.0;
    for (int k = 0; k < K; ++k) {
        const double* p = params + k * R;
        const double cw = p[0], lw = p[1], ld = p[2];
        MIX_CHECK_ARG(cw >= 0.0 && cw <= 1.0 && cw >= prev, "cumulative weights must not fall and lie in [0, 1]");
        MIX_CHECK_ARG(lw <= 0.0 && std::isfinite(ld), "log weights must be <= 0 and log-determinants finite");
        prev = cw;
        img[k] = cw;
        double* g = img.data() + MIX_MAX_K + (size_t)k * QP;
        g[0] = lw; g[1] = ld;
        for (int d = 0; d < D; ++d) {
            MIX_CHECK_ARG(std::isfinite(p[3 + d]), "centres must be finite");
            g[2 + d] = p[3 + d];
        }
        for (int e = 0; e < tri; ++e) {
            MIX_CHECK_ARG(std::isfinite(p[3 + D + e]) && std::isfinite(p[3 + D + tri + e]), "factors must be finite");
            g[2 + DP + e] = p[3 + D + e];           // (the first D columns of the DP-column packing sit at the same offsets)
            img[(size_t)MIX_MAX_K + (size_t)K * QP + (size_t)k * tri + e] = p[3 + D + tri + e];
        }
        for (int d = 0; d < D; ++d)
            MIX_CHECK_ARG(p[3 + D + tri + ev_tri(d) + d] > 0.0, "the diagonal of a Cholesky factor must be positive");
    }
    MIX_CHECK_ARG(prev == 1.0, "the last cumulative weight must be 1.0");
#undef MIX_CHECK_ARG
    for (int k = K; k < MIX_MAX_K; ++k) img[k] = 1.0;
    if (m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(apgp_stream_lock(s));
    double* dev = apgp_stream_scratch(MIX_SCRATCH_SLOT, s, img.size());
    if (!dev) {
        apgp_set_error("%s: scratch allocation failed", fn);
        return -2;
    }
    // (ordered on the stream and complete on return: img is a temporary)
    if (hipMemcpyWithStream(dev, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) {
        apgp_set_error("%s: parameter upload failed", fn);
        return -2;
    }
    MixArgs a;
    a.T = T; a.lnq = lnq; a.P = dev; a.m = m; a.idx_offset = idx_offset; a.D = D; a.K = K; a.seed = seed;
    launch(a, DP, (m + 255) / 256, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        apgp_set_error("%s: HIP error: %s", fn, hipGetErrorString(e));
        return -2;
    }
    return 0;
}
