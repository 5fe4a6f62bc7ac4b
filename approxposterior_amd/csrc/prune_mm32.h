// Coarse bound of the pruned arg-min with the exponents formed on the fp32 matrix cores (included from sweep.hip behind
// prune_bound32_kernel; DESIGN.md section 4, "The bound in two stages").  Same PruneArgs, same outputs as
// prune_bound32_kernel: bmin, est (b without slack), the (+inf, -1) pre-fill of the arg-min partials.
//
// With a = (t sc - c) kappa and b = (x - c) kappa as there (c = the first training row, kappa^2 = log2(e)), the exponent
// of k = amp 2^-|a - b|^2 is a rank-(Dpad + 2) product,
//     -|a - b|^2 = sum_e P[row][e] Q[e][candidate],   P = (-|b|^2, 1, 2 b_1 .. 2 b_Dpad),  Q = (1, -|a|^2, a_1 .. a_Dpad),
// and v_mfma_f32_32x32x2_f32 forms it for 32 training rows x 32 candidates in (Dpad + 2) / 2 instructions: bit for bit an
// fp32 fma chain over the entries, one rounding per entry.  Only the exponential and the two products with alpha and
// |alpha| stay on the vector ALU.
//   * operands: the candidates are the N side, lane l holds candidate l % 32 of a 32-candidate group in registers for
//     the whole kernel (PMM_G groups = PMM_G / 2 candidate blocks per wavefront, which share every LDS read of a
//     training row); the training rows are the M side, converted once per workgroup into an LDS tile of PMM_ROWS rows.
//     Lane half h = l / 32 takes entries h KH .. h KH + KH - 1 (KH = Dpad / 2 + 1), stored so that a lane reads its
//     KH floats in one 16-byte read per four entries and the rest behind them.
//   * a lane's 16 accumulators are 16 training rows (r & 3) + 8 (r >> 2) + 4 h of ONE candidate: exp2 in place, the
//     alphas of four consecutive rows in one 16-byte read, fp32 partial sums over the 16 rows, then into fp64 -- the
//     accumulation error does not grow with N.  Lanes l and l + 32 hold the two halves of a candidate's sums and are
//     combined once at the end.
//   * rows past n, rows that are not live and rows with a NaN or a coordinate beyond fp32 enter the operands as 0 (a NaN
//     in a candidate's column would stay in that column, but nothing is left to that); they decide admissibility in
//     fp64 alone, as in load_candidates.
//   * exact part: admissibility, k(t,t), util_value and the slack in fp64, as in prune_bound32_kernel.
//
// Error of mu32.  u = 2^-24, eps = 2^-53, A = |t sc - c|, B = max over the training rows of |x - c| (both without kappa:
// kappa^2 ln 2 = 1, so (A + B)^2 IS the scale of the exponent in natural units), K = Dpad + 2.  In the expanded form
// the exponent's error is no longer relative to r^2 but to (A + B)^2, whatever k is:
//   * conversions.  a^ = fl32(a), b^ = fl32(b) are off by u |a_d|, u |b_d| per coordinate, so |a^ - b^| and |a - b| = r
//     differ by <= u (A + B) and the squares by <= (2 r + u (A + B)) u (A + B) <= 2.01 u (A + B)^2  (r <= A + B).
//   * norms.  |a^|^2 and |b^|^2 are summed in fp64 from the CONVERTED coordinates (so that the three parts cancel to
//     -|a^ - b^|^2 exactly before rounding) and rounded once to fp32, no low parts: u (A^2 + B^2) <= u (A + B)^2.
//     2 b^_d is exact.
//   * chain.  One rounding per entry, relative to the partial sum, and every partial sum in any order of the entries is
//     at most |a^|^2 + |b^|^2 + 2 |a^| |b^| = (|a^| + |b^|)^2 in absolute value: K u (A + B)^2 (1 + K u).  The bound
//     does not depend on the order in which the instruction adds its two entries.
//     Together (K + 3.01) u (A + B)^2, taken as (K + 4) u (A + B)^2 with room for the fp64 roundings of a, b, kappa and
//     the norms (2^-29 u each) and the factors (1 + u)^K.
//   * centring, as for prune_bound32_kernel: t sc - c may be contracted to one fma, an ABSOLUTE shift delta of a with
//     |delta| <= 1.21 eps (|c| + A); it moves the exponent by <= 2 r |delta| + |delta|^2 <= 2.5 eps (A + B) (|c| + A).
//   * so k lies in [k^ e^-eta0, k^ e^eta0] with eta0 = (K + 4) u (A + B)^2 + 2.5 eps (A + B) (|c| + A), k^ the exact
//     power of the computed exponent.  v_exp_f32 (1 ulp, allowed 4 u), alpha -> fp32 (u) and the 16 fma of one fp32
//     partial sum (16 u of sum |alpha| k^, the terms of S32 below) are relative too: with
//         eta = eta0 + 24 u       (4.1 + 1.01 + 16.1 and room)
//     |sum alpha_i (k^_i - k_i)| <= (e^eta - 1) sum |alpha_i| k^_i.  The kernel accumulates S32 = sum |alpha_i| k^_i
//     beside mu32, one v_fmac more per value; summed like mu32 it is below the exact sum by <= 17 u of it and is taken
//     times 1 + 2^-16, expm1 times 1 + 2^-20.
//   * gate: eta <= 2^-8 keeps e^eta - 1 a small multiple of eta (and k^ <= e^eta where a candidate sits on a training
//     point).  It needs B, which the staging threads carry with the tiles (max over the rows < n), so it is decided
//     after the last tile.  Gate failed: e32 = +inf, the block's bound is -inf.
//   * flushes: a kernel value, an alpha or a product below 2^-126 may become 0: 2^-120 (sum |alpha| + N), absolute, so
//     this term keeps sum |alpha|.  It is a property of the fit, not of a candidate: the staging lanes add |alpha| of
//     the row they convert, in fp64 from the fp64 alpha, once per row and workgroup (N eps relative), and the sum is
//     taken times 1 + 2^-16, which also covers |fl32(alpha)| <= |alpha| (1 + u) where the fp32 alphas are meant.
// |mu32 - mu| <= e32 = amp ((e^eta - 1) S32 + 2^-120 (sum|alpha| + N)); the slack is prune_bound_kernel's with
// S <= amp sum|alpha| plus 2 e32.  At C3 (A + B ~ 9.5, S32 <= 5e4 against sum|alpha| = 1.9e6) that is below 8, where
// sum|alpha| in the place of S32 would give several hundred and prune nothing.
//
// A block whose bound came out -inf (gate failed: data far wider than the length scale; or a NaN bound) is left to
// prune_bound32_kernel<DPAD, true>, launched behind this kernel: the -inf in bmin is the mark, no other scratch.
// Variants measured: docs/experiments.md, round 13; what the fp32 MFMA leaves to the vector ALU beside it: round 17.
#pragma once

#ifndef PMM_G
#define PMM_G 4             // 32-candidate groups per wavefront (8 measured: docs/experiments.md, round 13)
#endif
#define PMM_ROWS 128        // training rows per LDS tile: one 32-row matrix tile staged by each wavefront
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int DPAD>
struct PmmShape {
    static constexpr int K = DPAD + 2, KH = K / 2, Q4 = KH / 4, R = KH % 4;
    static constexpr int RS = (2 * KH + 3) & ~3;                  // floats per LDS row (16-byte rows)
    // where entry e of a row stands in its LDS row: per four steps the quad of half 0, the quad of half 1; the rest after
    static constexpr int pos(int e) {
        const int h = e / KH, s = e % KH;
        return s < 4 * Q4 ? (s / 4) * 8 + h * 4 + (s & 3) : Q4 * 8 + h * R + (s - 4 * Q4);
    }
};

template <int DPAD>
__global__ __launch_bounds__(PR_THREADS, PMM_G <= 4 ? 2 : 1) void prune_bound_mm32_kernel(PruneArgs a) {
    using SH = PmmShape<DPAD>;
    constexpr int XS = DPAD + 2;                         // packed stream row: scaled x | alpha | 0
    constexpr int KH = SH::KH, RS = SH::RS, G = PMM_G;
    static_assert(PMM_G % 2 == 0 && PMM_ROWS == 32 * (PR_THREADS / 64), "one 32-row tile staged per wavefront");
    const double kappa = PR32_KAPPA;                     // sqrt(log2(e))
    __shared__ __attribute__((aligned(16))) float xt[PMM_ROWS * RS];
    __shared__ __attribute__((aligned(16))) float at[PMM_ROWS];
    __shared__ double wmax[PR_THREADS / 64], wsal[PR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const long long blk0 = ((long long)blockIdx.x * (PR_THREADS / 64) + w) * (G / 2);
    double cen[DPAD], c2 = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; ++d) { cen[d] = a.xs[d]; c2 = fma(cen[d], cen[d], c2); }
    const double cn = sqrt(c2);                          // |c|
    float qop[G][KH];                                    // the candidates' side of the product, this lane half's entries
    double an[G];
    bool adm[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        // admissibility and k(t,t) exactly as the sweep's load_candidates (lin_coef == 0: k(t,t) = amp)
        const long long blk = blk0 + (g >> 1);
        const long long row = blk * SW_CAND + (g & 1) * 32 + l32;
        const bool live = blk < a.ncb && row < a.m;
        bool ok = live, has_nan = false;
        double a2 = 0.0, ce[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            double v = 0.0;
            if (live && d < a.ndim) {
                v = a.T[row * a.ndim + d];
                if (a.has_box && !(v >= a.lo[d] && v <= a.hi[d])) ok = false;
                if (v != v) has_nan = true;
            }
            ce[d] = v * a.sc[d] - cen[d];
            a2 = fma(ce[d], ce[d], a2);
        }
        if (live && a.mask && a.mask[row] == 0) ok = false;
        adm[g] = ok && !has_nan;
        an[g] = sqrt(a2);
        const bool use = live && !has_nan && a2 <= 0x1p100;      // else 0: the gate fails on an, or the row is inadmissible
        float af[DPAD];
        double n2 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            af[d] = use ? (float)(ce[d] * kappa) : 0.0f;
            n2 = fma((double)af[d], (double)af[d], n2);
        }
        const float na = -(float)n2;
#pragma unroll
        for (int s = 0; s < KH; ++s) {
            const int e0 = s, e1 = KH + s;               // entry of half 0, of half 1
            const float q0 = e0 == 0 ? 1.0f : e0 == 1 ? na : af[e0 >= 2 ? e0 - 2 : 0];
            const float q1 = af[e1 - 2];                 // (KH >= 2: half 1 holds coordinates only)
            qop[g][s] = h ? q1 : q0;
        }
    }
    double accm[G], accs[G], sal = 0.0, bm2 = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) { accm[g] = 0.0; accs[g] = 0.0; }
    const long long ntile = (a.n + PMM_ROWS - 1) / PMM_ROWS;
    // staging: lane l32 of half 0 of wavefront w converts row 32 w + l32 of the tile
    const bool stager = h == 0;
    const int srow = w * 32 + l32;
    f64x2 pre[XS / 2];
    auto fetch = [&](long long ti) {                     // (rows < ntile * PMM_ROWS <= npad: inside the packed stream)
        const f64x2* src = (const f64x2*)(a.xs + (ti * PMM_ROWS + srow) * XS);
#pragma unroll
        for (int i = 0; i < XS / 2; ++i) pre[i] = stager ? src[i] : f64x2{0.0, 0.0};
    };
    fetch(0);
    for (long long ti = 0; ti < ntile; ++ti) {
        if (stager) {
            const bool in = ti * PMM_ROWS + srow < a.n;  // rows of the padding: operands 0, alpha 0, no part in B
            float bf[DPAD];
            double n2 = 0.0, b2 = 0.0;
#pragma unroll
            for (int d = 0; d < DPAD; ++d) {
                const double x = (d & 1) ? pre[d >> 1].y : pre[d >> 1].x;
                const double df = x - cen[d];
                b2 = fma(df, df, b2);
                bf[d] = in ? (float)(df * kappa) : 0.0f;
                n2 = fma((double)bf[d], (double)bf[d], n2);
            }
            if (in) { bm2 = fmax(bm2, b2); sal += fabs(pre[DPAD / 2].x); }
            float rowv[RS];
#pragma unroll
            for (int i = 0; i < RS; ++i) rowv[i] = 0.0f;
            rowv[SH::pos(0)] = -(float)n2;
            rowv[SH::pos(1)] = 1.0f;
#pragma unroll
            for (int d = 0; d < DPAD; ++d) rowv[SH::pos(d + 2)] = 2.0f * bf[d];
#pragma unroll
            for (int i = 0; i < RS; i += 4)
                *(f32x4*)(xt + srow * RS + i) = f32x4{rowv[i], rowv[i + 1], rowv[i + 2], rowv[i + 3]};
            at[srow] = in ? (float)pre[DPAD / 2].x : 0.0f;
        }
        __syncthreads();
        if (ti + 1 < ntile) fetch(ti + 1);
#pragma unroll 1
        for (int rt = 0; rt < PMM_ROWS / 32; ++rt) {
            const float* xr = xt + (rt * 32 + l32) * RS;
            float pop[KH];                               // the training rows' side, this lane half's entries
#pragma unroll
            for (int q = 0; q < SH::Q4; ++q) {
                const f32x4 v = *(const f32x4*)(xr + q * 8 + h * 4);
                pop[4 * q] = v.x; pop[4 * q + 1] = v.y; pop[4 * q + 2] = v.z; pop[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < SH::R; ++r) pop[4 * SH::Q4 + r] = xr[SH::Q4 * 8 + h * SH::R + r];
            float al[16];                                // alpha of accumulator r's row: (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(al + 4 * q) = *(const f32x4*)(at + rt * 32 + 8 * q + 4 * h);
            auto product = [&](int g) {
                f32x16 c = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < KH; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(pop[s], qop[g][s], c, 0, 0, 0);
                return c;
            };
            // Written as a two-tile pipeline, but hipcc issues all G groups' products first and the vector work behind
            // them (64 accumulators fit), and nothing is lost by that: v_mfma_f32_32x32x2_f32 holds the vector lanes
            // for its 64 cycles, so an exponential placed between two products costs what it costs behind them
            // (tools/probes/mfma32_shadow.hip; docs/experiments.md, round 17).
            f32x16 cur = product(0);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                f32x16 nxt = cur;
                if (g + 1 < G) nxt = product(g + 1);
                float ps = 0.0f, pS = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float k = __builtin_amdgcn_exp2f(cur[r]);
                    ps = fmaf(k, al[r], ps);
                    pS = fmaf(k, fabsf(al[r]), pS);
                }
                accm[g] += (double)ps;
                accs[g] += (double)pS;
                cur = nxt;
            }
        }
        __syncthreads();                                 // the tile has been consumed
    }
    // B = max |x - c| and sum |alpha| over the training rows: the stagers' maxima and sums, over the workgroup (every
    // workgroup adds the same rows in the same order: one value of sum |alpha| per call)
    for (int o = 32; o > 0; o >>= 1) { bm2 = fmax(bm2, __shfl_xor(bm2, o)); sal += __shfl_xor(sal, o); }
    if (lane == 0) { wmax[w] = bm2; wsal[w] = sal; }
    __syncthreads();
    sal = 0.0;
#pragma unroll
    for (int i = 0; i < PR_THREADS / 64; ++i) { bm2 = fmax(bm2, wmax[i]); sal += wsal[i]; }
    const double bn = sqrt(bm2);
    const double u32 = 0x1p-24, eps = 0x1p-53;
    const double sa = sal * (1.0 + 0x1p-16);
    double bb = INFINITY, bbe = INFINITY;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double sm = accm[g] + __shfl_xor(accm[g], 32);
        const double s32 = (accs[g] + __shfl_xor(accs[g], 32)) * (1.0 + 0x1p-16);
        const double ktt = a.amp;
        const double mu = fma(a.amp, sm, a.mean);
        double b = util_value(a.kind, mu, ktt, a.zeta, a.ybest);
        const double ab = an[g] + bn;
        const double eta = (DPAD + 6.0) * u32 * ab * ab + 2.5 * eps * ab * (cn + an[g]) + 24.0 * u32;
        double e32 = a.amp * (expm1(eta) * (1.0 + 0x1p-20) * s32 + 0x1p-120 * (sa + (double)a.n));
        if (!(eta <= 0x1p-8)) e32 = INFINITY;
        // prune_bound_kernel's slack with S <= amp sum|alpha|, and the fp32 part on top
        double slack = 2.0 * e32 + 2.0 * (4.0 * (double)(a.n + 16) + 8.0 * DPAD + 32.0) * eps * (a.amp * sa) +
                       64.0 * eps * (1.0 + fabs(mu) + fabs(a.ybest) + fabs(a.zeta) + ktt + fabs(b));
        if (a.kind == APGP_UTIL_BAPE) slack += 16.0 * eps / (1.0 - exp(0.0 - ktt));
        double be = b;
        b -= slack;
        if (!(b == b)) b = -INFINITY;
        if (!(be == be)) be = -INFINITY;
        if (!adm[g]) b = be = INFINITY;
        for (int o = 16; o > 0; o >>= 1) { b = fmin(b, __shfl_xor(b, o)); be = fmin(be, __shfl_xor(be, o)); }
        bb = fmin(bb, b); bbe = fmin(bbe, be);
        if (g & 1) {                                     // both 32-candidate groups of block blk0 + g / 2 are in
            const long long blk = blk0 + (g >> 1);
            if (lane == 0 && blk < a.ncb) {
                a.bmin[blk] = bb;
                if (a.est) a.est[blk] = bbe;
                if (a.part_u) {
                    a.part_u[blk] = INFINITY;            // a pruned block's partial: never wins
                    a.part_i[blk] = -1;
                }
            }
            bb = INFINITY; bbe = INFINITY;
        }
    }
}
