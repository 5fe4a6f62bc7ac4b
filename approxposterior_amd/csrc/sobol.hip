// Quasi-random siblings of the three candidate generators (DESIGN.md "Quasi-random draws"): the same transforms of a
// uniform (draws.h) with the uniform taken from a scrambled Sobol sequence instead of Philox.
//
//   apgp_sobol_box_candidates     apgp_box_candidates' box
//   apgp_sobol_prior_candidates   apgp_prior_candidates' product prior
//   apgp_sobol_mix_candidates     apgp_mix_candidates' mixture: dimensions 0 .. D - 1 give the normals, dimension D the component
//   apgp_sobol_direction          the compiled direction numbers, read on the host
//
// Point g (0 <= g < 2^30), dimension d: x = XOR over the set bits b of gray = g ^ (g >> 1) of V32[d][b] (sobol_table.h: the
// Joe-Kuo numbers as torch holds them, so x / 2^32 is row g of torch's SobolEngine).  Direct evaluation, no recurrence: row
// g is a function of (seed, replicate, g) alone, so a rank generates its own rows by idx_offset and anybody regenerates
// one row.  Scramble (nested uniform, hash-based: Laine-Karras as in Burley 2020), per dimension:
//   x <- rev32(lk(rev32(x), h_d)),  h_d = word 0 of Philox4x32-10 with counter (d, replicate, 0, "SOBL"), key = seed.
// Uniform: u = (x + 0.5) 2^-32, exact in fp64 and strictly inside (0, 1).
//
// One thread per row.  The table is read with wave-uniform indices (d and b are the same in every lane: scalar loads) and
// a word is XORed in under the lane's bit.  The loop over b runs in steps of ten words and stops past the bit length of the
// call's last row, found on the host.
#include "apgp_common.h"
#include "draws.h"
#include "sobol_table.h"

#define SOBOL_TAG 0x534f424cu              // "SOBL": the scramble seeds' Philox counter tag
#define SOBOL_MAX_ROWS (1ll << APGP_SOBOL_BITS)
#define SOBOL_STEP 10                      // table words per step of the XOR loop
static_assert(APGP_SOBOL_BITS % SOBOL_STEP == 0, "the XOR loop reads whole steps of a table row");

namespace {

struct SobolKey {
    int nbits;                             // bits of gray that any row of the call sets
    int scramble;
    unsigned int h[APGP_SOBOL_DIMS];       // the per-dimension scramble seeds
};

__device__ __forceinline__ unsigned int sobol_lk(unsigned int v, unsigned int h) {
    v += h;
    v ^= v * 0x6c50b47cu;
    v ^= v * 0xb82f1e52u;
    v ^= v * 0xc7afe638u;
    v ^= v * 0x8d22f6e6u;
    return v;
}

__device__ __forceinline__ unsigned int sobol_gray(long long g) {
    const unsigned int v = (unsigned int)g;
    return v ^ (v >> 1);
}

// the uniform of dimension d at the point whose Gray code is gray (d is wave-uniform)
__device__ __forceinline__ double sobol_u(const SobolKey& s, unsigned int gray, int d) {
    // ten words of the row per step (three steps cover the 30): their loads are issued together, and the words past the
    // call's last set bit meet a zero bit of gray
    unsigned int x = 0u;
    for (int b0 = 0; b0 < s.nbits; b0 += SOBOL_STEP) {
        const unsigned int gb = gray >> b0;
#pragma unroll
        for (int j = 0; j < SOBOL_STEP; ++j) x ^= sobol_v32[d][b0 + j] & (0u - ((gb >> j) & 1u));
    }
    if (s.scramble) x = __brev(sobol_lk(__brev(x), s.h[d]));
    return ((double)x + 0.5) * (1.0 / 4294967296.0);
}

__global__ __launch_bounds__(256) void sobol_box_kernel(BoxArgs a, SobolKey s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const unsigned int gray = sobol_gray(a.idx_offset + i);
    double* row = a.T + i * a.ndim;
    for (int d = 0; d < a.ndim; ++d) row[d] = fma(a.span[d], sobol_u(s, gray, d), a.lo[d]);
}

__global__ __launch_bounds__(256) void sobol_prior_kernel(PriorArgs a, SobolKey s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const unsigned int gray = sobol_gray(a.idx_offset + i);
    double* row = a.T + i * a.ndim;
    for (int d = 0; d < a.ndim; ++d) row[d] = prior_draw(a, d, sobol_u(s, gray, d));
}

template <int DP>
__global__ __launch_bounds__(256) void sobol_mix_kernel(MixArgs a, SobolKey s) {
    __shared__ double slp[MIX_MAX_K][256];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    if (i >= a.m) return;
    const unsigned int gray = sobol_gray(a.idx_offset + i);
    const int k = mix_pick(a, sobol_u(s, gray, a.D));
    double z[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        z[d] = 0.0;
        if (d < a.D) z[d] = prior_gauss(0.0, 1.0, sobol_u(s, gray, d));
    }
    mix_row<DP>(a, i, tid, k, z, slp);
}

// the checks the three draws add to their siblings'; fills s or returns the failed check's message
const char* sobol_key(SobolKey& s, int64_t m, int64_t idx_offset, uint64_t seed, int32_t replicate, int32_t scramble) {
    if (!(m >= 0 && idx_offset >= 0)) return "m >= 0 and idx_offset >= 0 required";
    if (!(m <= SOBOL_MAX_ROWS && idx_offset <= SOBOL_MAX_ROWS && idx_offset + m <= SOBOL_MAX_ROWS))
        return "idx_offset + m <= 2^30 required: the sequence has 2^30 points";
    if (replicate < 0) return "replicate >= 0 required";
    if (!(scramble == 0 || scramble == 1)) return "scramble must be 0 or 1";
    s.scramble = scramble;
    s.nbits = 0;
    for (int64_t last = idx_offset + m - 1; last > 0; last >>= 1) ++s.nbits;
    for (int d = 0; d < APGP_SOBOL_DIMS; ++d) {
        unsigned int c[4] = {(unsigned int)d, (unsigned int)replicate, 0u, SOBOL_TAG};
        philox4x32(c, (unsigned int)seed, (unsigned int)(seed >> 32));
        s.h[d] = c[0];
    }
    return nullptr;
}

}  // namespace

extern "C" int32_t apgp_sobol_direction(int32_t d, int32_t b) {
    if (d < 0 || d >= APGP_SOBOL_DIMS || b < 0 || b >= APGP_SOBOL_BITS) return -1;
    return (int32_t)(sobol_v32_host[d][b] >> 2);
}

extern "C" int apgp_sobol_box_candidates(double* T, int64_t m, int32_t ndim, const double* lo, const double* hi,
                                         uint64_t seed, int32_t replicate, int32_t scramble, int64_t idx_offset,
                                         void* stream) {
    APGP_CHECK_ARG(T && lo && hi, "null pointer");
    SobolKey s;
    const char* bad = sobol_key(s, m, idx_offset, seed, replicate, scramble);
    APGP_CHECK_ARG(bad == nullptr, bad);
    APGP_CHECK_ARG(ndim >= 1 && ndim <= APGP_MAX_DIM, "1 <= ndim <= APGP_MAX_DIM required");
    if (m == 0) return 0;
    BoxArgs a;
    bad = box_args(a, ndim, lo, hi);
    APGP_CHECK_ARG(bad == nullptr, bad);
    a.T = T; a.m = m; a.idx_offset = idx_offset; a.seed = seed;
    hipLaunchKernelGGL(sobol_box_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, s);
    APGP_CHECK_LAUNCH();
    return 0;
}

extern "C" int apgp_sobol_prior_candidates(double* T, int64_t m, int32_t ndim, const int32_t* kind, const double* p0,
                                           const double* p1, uint64_t seed, int32_t replicate, int32_t scramble,
                                           int64_t idx_offset, void* stream) {
    APGP_CHECK_ARG(T && kind && p0 && p1, "null pointer");
    SobolKey s;
    const char* bad = sobol_key(s, m, idx_offset, seed, replicate, scramble);
    APGP_CHECK_ARG(bad == nullptr, bad);
    PriorArgs a;
    bad = prior_args(a, ndim, kind, p0, p1, true);
    APGP_CHECK_ARG(bad == nullptr, bad);
    if (m == 0) return 0;
    a.T = T; a.out = nullptr; a.m = m; a.idx_offset = idx_offset; a.seed = seed;
    hipLaunchKernelGGL(sobol_prior_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, s);
    APGP_CHECK_LAUNCH();
    return 0;
}

extern "C" int apgp_sobol_mix_candidates(double* T, double* lnq, int64_t m, int32_t ndim, int32_t ncomp,
                                         const double* params, uint64_t seed, int32_t replicate, int32_t scramble,
                                         int64_t idx_offset, void* stream) {
    APGP_CHECK_ARG(T && params, "null pointer");
    SobolKey s;
    const char* bad = sobol_key(s, m, idx_offset, seed, replicate, scramble);
    APGP_CHECK_ARG(bad == nullptr, bad);
    return mix_draw_call(__func__, T, lnq, m, ndim, ncomp, params, seed, idx_offset, stream,
                         [&s](const MixArgs& a, int DP, long long blocks, hipStream_t st) {
                             apgp_by_dpad(DP, [&](auto dp) {
                                 hipLaunchKernelGGL(sobol_mix_kernel<decltype(dp)::value>, dim3((unsigned)blocks), dim3(256), 0,
                                                    st, a, s);
                             });
                         });
}
