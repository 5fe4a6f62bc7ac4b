// Proposals of the on-device ensemble sampler and the counter-based RNG they draw from.  ensemble_kernel and
// ensemble_mw_kernel (ensemble.hip) and tempered_kernel (tempering.hip) share one sampler body so that they cannot drift
// apart: ens_propose here, and in ens_body.h the walker load, the GP-mean row loops, the start gate, the iteration prologue,
// the slot index, the accept step and the walker store.  tests/ensemble_moves_ref.py states the recipe; this file implements
// that text.
//
// A half-step moves slot t of the active half S (walker s) against the complement C (H = W / 2 slots), all slots in
// parallel against the positions at its start, which are the kernel's scaled coordinates x * sc.  Every draw is a pure
// function of (seed, ensemble, iteration, split, slot): Philox4x32-10 with counter (it low, it high, split * 256 + t, tag).
//   tag 5 (word 2 = 0xffffffff): per iteration -- word 0 % W is the offset of the red/blue partition; with more than one
//          move listed, u01(word 1, word 2) picks the iteration's move from the cumulative weights (the first m with
//          u < cum[m], the last one otherwise);
//   tag 1: stretch -- u01(words 0, 1) is the stretch uniform, word 2 % H the partner;
//   tag 2: the acceptance uniform (all moves);
//   tag 3: differential evolution -- j = word 0 % H, k = word 1 % (H - 1), k += (k >= j): an ordered pair j != k;
//   tag 4: differential evolution -- n = sqrt(-2 log u01(words 0, 1)) cospi(2 u01(words 2, 3)): Box-Muller, the cosine
//          with its argument reduced exactly (2 u is exact);
//   tag 6: snooker -- j, k as tag 3, l = word 2 % (H - 2), l += (l >= min(j, k)), l += (l >= max(j, k));
//   tag 7: parallel tempering (tempering.hip) -- counter (round low, round high, walker, 7) under the keys of the pair's
//          lower rung: u01(words 0, 1) is the exchange uniform.
// Hamiltonian Monte Carlo (hmc.hip) draws under the keys (seed, seed >> 32 ^ chain * 0x9E3779B9) with the GLOBAL iteration
// number in words 0 and 1:
//   tag 8: momentum -- counter (it low, it high, d, 8): ens_normal(u01(words 0, 1), u01(words 2, 3)) sqrt(m_d) is p_d
//          (one counter per dimension: ens_normal turns four words into one normal);
//   tag 9: step jitter -- counter (it low, it high, 0xffffffff, 9) under chain 0's keys, so every chain of the call
//          has the iteration's eps (1 + jitter (2 u01(words 0, 1) - 1));
//   tag 10: the acceptance uniform -- counter (it low, it high, 0xfffffffe, 10): u01(words 0, 1).
// Moves:
//   stretch(a):           z = (a - 1) u + 1, zz = z z / a, q = c_j - (c_j - s) zz, factor (D - 1) log zz;
//   DE(sigma, g0):        gamma = g0 (1 + sigma n), q = s + gamma (c_j - c_k), factor 0;
//   snooker(gammas):      v = s - c_j, n2 = |v|^2, coef = gammas (v . (c_k - c_l)) / n2, q = s + coef v
//                         (= s + gammas (e . (z1 - z2)) e with e = v / |v|), nq2 = |q - c_j|^2,
//                         factor ((D - 1) / 2) log(nq2 / n2); s = c_j gives 0 / 0: q is NaN and the slot is rejected.
// A DE or snooker proposal with a non-finite coordinate is outside whatever the box; the stretch gate is the one it was.
#pragma once
#include "apgp_common.h"

#define ENS_MAXW 256

// (host too: sobol.hip hashes its per-dimension scramble seeds on the host)
__host__ __device__ __forceinline__ void philox4x32(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0;
        const unsigned int n1 = (unsigned int)p1;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
        const unsigned int n3 = (unsigned int)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ double u01(unsigned int a, unsigned int b) {
    // 53-bit uniform in (0, 1)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// Box-Muller normal from two uniforms in (0, 1).  Not inlined (as prior_gauss in ensemble.hip): inlined, the constants of
// log and cospi are hoisted out of the iteration loop into 25 registers that stay live through the GP mean.
static inline __device__ __attribute__((noinline)) double ens_normal(double u1, double u2) {
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// The Gaussian inverse CDF of the prior draws (ensemble.hip prior_candidates_kernel) and of the mixture proposal (evidence.hip):
// mu + (sigma sqrt 2) erfcinv(2 (1 - u)), every operation rounded in NumPy's order (tests/prior_ref.py).
// (not inlined: inside the row loop the compiler hoists erfcinv's coefficients into some 400 registers)
static inline __device__ __attribute__((noinline)) double prior_gauss(double mu, double sigma, double u) {
    const double w = __dmul_rn(2.0, __dsub_rn(1.0, u));
    return __dadd_rn(mu, __dmul_rn(__dmul_rn(sigma, 1.4142135623730951), erfcinv(w)));
}

// the move table of a launch: kinds, cumulative normalised weights and the two parameters of include/apgp.h
struct EnsMoves {
    int n;
    int kind[APGP_ENS_MAX_MOVES];
    double cum[APGP_ENS_MAX_MOVES], p0[APGP_ENS_MAX_MOVES], p1[APGP_ENS_MAX_MOVES];
};

// index of the iteration's move from the offset counter's output cr (tag 5); uniform over the workgroup
__device__ __forceinline__ int ens_pick_move(const EnsMoves& mv, const unsigned int (&cr)[4]) {
    if (mv.n == 1) return 0;
    const double um = u01(cr[1], cr[2]);
    int m = 0;
    while (m < mv.n - 1 && !(um < mv.cum[m])) ++m;
    return m;
}

// Proposal of slot t (walker s of the active half) under the iteration's move (kind, p0, p1): writes q[0..DPAD), returns
// "inside the box [lo, hi] (and, for DE and snooker, finite)" and sets fac, the log proposal factor, and uacc, the
// acceptance uniform (tag 2).  cs: the scaled positions at the start of the half-step; c_idx(i): walker of complement slot i.
// The stretch branch is one basic block as it was before the other moves existed, so that its two generators and its
// logarithm can overlap; it does not share a logarithm or the acceptance draw with the other branches after a join.
// ALLMOVES = false leaves the stretch branch alone: the kernels are instantiated both ways and a table of stretch entries
// only -- the default -- runs the kernel that holds no other move.  With the others compiled in, the README chain's
// stretch time is 8 % above the parent commit's, outside its spread, though it never takes their branch
// (profiles/ensemble_moves_timing.json, "stretch, all-moves kernels"; DESIGN.md "Ensemble moves").
template <int DPAD, bool ALLMOVES, class CIdx>
__device__ __forceinline__ bool ens_propose(const int kind, const double p0, const double p1, const double (*cs)[DPAD],
                                            const int s, const CIdx& c_idx, const int H, const int D, const double* lo,
                                            const double* hi, const long long it, const int split, const int t,
                                            const unsigned int k0, const unsigned int k1, double* q, double& fac, double& uacc) {
    const unsigned int w0 = (unsigned int)it, w1 = (unsigned int)(it >> 32), w2 = (unsigned int)(split * ENS_MAXW + t);
    bool ok = true;
    if (!ALLMOVES || kind == APGP_ENS_MOVE_STRETCH) {
        unsigned int c1[4] = {w0, w1, w2, 0x1u};
        philox4x32(c1, k0, k1);
        const double u = u01(c1[0], c1[1]);
        const double z = ((p0 - 1.0) * u + 1.0);
        const double zz = z * z / p0;
        const int j = c_idx((int)(c1[2] % (unsigned int)H));
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            const double qv = cs[j][d] - (cs[j][d] - cs[s][d]) * zz;
            q[d] = qv;
            // prior gate in scaled coordinates (lo/hi were scaled on the host)
            if (d < D && !(qv >= lo[d] && qv <= hi[d])) ok = false;
        }
        fac = (D - 1.0) * log(zz);
        unsigned int c2[4] = {w0, w1, w2, 0x2u};
        philox4x32(c2, k0, k1);
        uacc = u01(c2[0], c2[1]);
        return ok;
    }
    if constexpr (!ALLMOVES) return false;      // (not reached: the host launches this instantiation for stretch tables only)
    unsigned int c2[4] = {w0, w1, w2, 0x2u};
    philox4x32(c2, k0, k1);
    uacc = u01(c2[0], c2[1]);
    if (kind == APGP_ENS_MOVE_DE) {
        unsigned int c3[4] = {w0, w1, w2, 0x3u};
        philox4x32(c3, k0, k1);
        const int js = (int)(c3[0] % (unsigned int)H);
        int ks = (int)(c3[1] % (unsigned int)(H - 1));
        if (ks >= js) ++ks;
        const int j = c_idx(js), k = c_idx(ks);
        unsigned int c4[4] = {w0, w1, w2, 0x4u};
        philox4x32(c4, k0, k1);
        const double nrm = ens_normal(u01(c4[0], c4[1]), u01(c4[2], c4[3]));
        const double gam = p1 * (1.0 + p0 * nrm);
#pragma unroll 1
        for (int d = 0; d < DPAD; ++d) {
            const double qv = fma(gam, cs[j][d] - cs[k][d], cs[s][d]);
            q[d] = qv;
            if (d < D && !(qv >= lo[d] && qv <= hi[d] && isfinite(qv))) ok = false;
        }
        fac = 0.0;
    } else {
        unsigned int c6[4] = {w0, w1, w2, 0x6u};
        philox4x32(c6, k0, k1);
        const int js = (int)(c6[0] % (unsigned int)H);
        int ks = (int)(c6[1] % (unsigned int)(H - 1));
        if (ks >= js) ++ks;
        int ls = (int)(c6[2] % (unsigned int)(H - 2));
        if (ls >= (js < ks ? js : ks)) ++ls;
        if (ls >= (js < ks ? ks : js)) ++ls;
        const int j = c_idx(js), k = c_idx(ks), l = c_idx(ls);
        double n2 = 0.0, dot = 0.0;
#pragma unroll 1
        for (int d = 0; d < DPAD; ++d) {       // (the padding coordinates are zero; rolled: these loops run once per half-step)
            const double v = cs[s][d] - cs[j][d];
            n2 = fma(v, v, n2);
            dot = fma(v, cs[k][d] - cs[l][d], dot);
        }
        const double coef = p0 * dot / n2;
        double nq2 = 0.0;
#pragma unroll 1
        for (int d = 0; d < DPAD; ++d) {
            const double qv = fma(coef, cs[s][d] - cs[j][d], cs[s][d]);
            q[d] = qv;
            const double r = qv - cs[j][d];
            nq2 = fma(r, r, nq2);
            if (d < D && !(qv >= lo[d] && qv <= hi[d] && isfinite(qv))) ok = false;
        }
        fac = (0.5 * (D - 1.0)) * log(nq2 / n2);
    }
    return ok;
}
