// Coarse bound of the pruned arg-min with the exponents formed on the bf16 matrix cores (included from sweep.hip behind
// prune_bound32_kernel; DESIGN.md section 4, "The bound in two stages").  Same PruneArgs, same outputs as
// prune_bound32_kernel: bmin, est (b without slack), the (+inf, -1) pre-fill of the arg-min partials.
//
// With a = (t sc - c) kappa and b = (x - c) kappa as there (c = the first training row, kappa^2 = log2(e)), the exponent
// of k = amp 2^-|a - b|^2 is a rank-(Dpad + 2) product of fp32 entries,
//     -|a - b|^2 = sum_e P[row][e] Q[e][candidate],   P = (-|b|^2, 1, 2 b_1 .. 2 b_Dpad),  Q = (1, -|a|^2, a_1 .. a_Dpad).
// v_mfma_f32_32x32x2_f32 forms it at the fp32 vector rate and holds the vector lanes while it runs (docs/experiments.md,
// round 17); v_mfma_f32_32x32x16_bf16 is 16 times faster and leaves them free.  So every fp32 entry p is written as the
// EXACT sum of three bf16 numbers, h = bf16(p), m = bf16(p - h), l = p - h - m (round to nearest; |m| <= 2^-8 |p|,
// |l| <= 2^-17 |p|; tests/test_prune_mmbf16_ref.py), and P[e] Q[e] becomes nine bf16 products of which six are kept:
//     big    h h                                  one per entry: Dpad + 2
//     small  h m, m h, m m, h l, l h              five per coordinate entry; m 1, l 1 for the two norm entries (1 = h)
//     dropped  m l, l m, l l                      <= (2^-24 + 2^-34) |p q| per coordinate entry
// The k slots of the instruction are filled 16 at a time (PmmShape::slot): the small products FIRST, lowest order first
// (h l and l h, the norms' l; m m; h m and m h, the norms' m), into an accumulator that starts at 0, padded with zeros to
// a multiple of 16; the big products in the LAST instruction.  Dpad = 8: 44 small products in three instructions and ten
// big ones in the fourth; Dpad = 4: 2 + 1; Dpad = 2: 1 + 1.  Only the exponential and the two products with alpha and
// |alpha| stay on the vector ALU, and run under the next group's matrix products or the other wavefront's.
//   * operands: the candidates are the N (B) side, lane l holds candidate l % 32 of a 32-candidate group in registers
//     for the whole kernel, k slots 8 (l / 32) .. + 7 of every instruction: 4 VGPRs per instruction and group (PMM_G
//     groups = PMM_G / 2 candidate blocks per wavefront, which share every LDS read of a training row); the training
//     rows are the M (A) side, split once per fit (apgp_pack_prune_rows -> pmm_pack_rows_kernel: the stream holds every
//     tile's LDS image and the kernel copies it, PRE = true; a caller without the stream gets PRE = false, where every
//     workgroup splits the rows itself, same bits) into LDS tiles of PMM_ROWS rows of 16 NI bf16 values, of which
//     a lane reads its 8 per instruction in one 16-byte read.  The row pitch is 32 NI + 16 bytes, an ODD number of
//     16-byte units: ds_read_b128 serves 16 lanes per pass, the rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of one
//     lane half, which are 16 different rows modulo 16, so with an odd pitch their 16-byte pieces fall on 16 different
//     four-bank groups of the 64 banks: conflict-free (an even pitch, 128 bytes for Dpad = 8, would be 8-way).
//   * a lane's 16 accumulators are 16 training rows (r & 3) + 8 (r >> 2) + 4 h of ONE candidate (the C layout does not
//     depend on the operand type): exp2 in place, the alphas of four consecutive rows in one 16-byte read, fp32 partial
//     sums over the 16 rows, then into fp64 -- the accumulation error does not grow with N.  Lanes l and l + 32 hold
//     the two halves of a candidate's sums and are combined once at the end.
//   * rows past n, rows that are not live and rows with a NaN or a coordinate beyond fp32 enter with their coordinates
//     and their norm 0 in all three parts (a NaN in a candidate's column would stay in that column, but nothing is left
//     to that); the entries "1" stay 1, so a padding row's exponent is -|a|^2 <= 0 and its kernel value meets alpha = 0.
//     Such rows decide admissibility in fp64 alone, as in load_candidates.  Inside the gate below no part can be
//     infinite: eta <= 2^-8 means (A + B)^2 < 2^13, every entry of P and Q is below 2^14 in absolute value, and
//     rounding a finite fp32 number below 2^127 to bf16 stays finite; outside it (a^2 up to 2^100 is let in) an
//     infinite or NaN exponent gives a NaN bound, which is the same -inf mark.
//   * exact part: admissibility, k(t,t), util_value and the slack in fp64, as in prune_bound32_kernel.
//
// What the instruction does with its 16 products and C (tools/probes/mfma_bf16_acc.hip, profiles/r18_mfma_bf16_acc.txt;
// DESIGN.md section 2): it works in two halves, k slots 0 .. 7 and then 8 .. 15.  Per half the products (exact, 16 bits)
// are aligned to E = the largest sum of the two operands' exponents among the non-zero products (so the largest product
// lies in [2^(E-2), 2^E)) and cut TOWARD ZERO to multiples of q = 2^(E-26); the accumulator, where it has bits below q,
// is cut to a multiple of q toward -inf; the cut values are summed exactly and rounded to nearest once.  Nothing is
// flushed: bf16 subnormal operands, subnormal products, sums and C all count.  A zero product loses nothing and a half
// with no non-zero product returns its accumulator.  With pmax the largest product of the half, q <= 2^-24 pmax = u pmax:
//     per half  |error| <= (non-zero products + 1) u pmax + u |partial sum|.
//
// Error of mu32.  u = 2^-24, eps = 2^-53, A = |t sc - c|, B = max over the training rows of |x - c| (both without kappa:
// kappa^2 ln 2 = 1, so (A + B)^2 IS the scale of the exponent in natural units), K = Dpad + 2.  In the expanded form
// the exponent's error is not relative to r^2 but to (A + B)^2, whatever k is:
//   * conversions.  a^ = fl32(a), b^ = fl32(b) are off by u |a_d|, u |b_d| per coordinate, so |a^ - b^| and |a - b| = r
//     differ by <= u (A + B) and the squares by <= (2 r + u (A + B)) u (A + B) <= 2.01 u (A + B)^2  (r <= A + B).
//   * norms.  |a^|^2 and |b^|^2 are summed in fp64 from the CONVERTED coordinates (so that the three parts cancel to
//     -|a^ - b^|^2 exactly) and rounded once to fp32: u (A^2 + B^2) <= u (A + B)^2.  2 b^_d is exact, and so is the
//     split of every entry.
//   * dropped products.  (2^-24 + 2^-34) sum_d |2 b^_d a^_d| <= (2^-24 + 2^-34) (|a^| + |b^|)^2 / 2 <= 0.51 u (A + B)^2.
//   * accumulation.  The absolute values of all products of an entry sum to <= |p q| (1 + 2^-7), and sum_e |P_e Q_e| =
//     (|a^| + |b^|)^2, so every partial sum and every product is at most (1 + 2^-7) (A + B)^2 (natural units), and every
//     small product and every partial sum of the small chain at most 2^-7 of that.  Last instruction: K non-zero
//     products and two accumulator cuts at u pmax each, two roundings: (K + 4) u (A + B)^2.  Small chain: per half nine
//     cuts of <= u 2^-8 and a rounding of <= u 2^-7, 11 u 2^-8 (A + B)^2, in at most six halves: 0.26 u (A + B)^2.
//     Together (K + 4.26) u (A + B)^2: the order of the slots matters only in that the K products of full size meet
//     the accumulator once, in the last instruction.
//     With the above (K + 7.78) u (A + B)^2, taken as (K + 8) u (A + B)^2 with room for the factors (1 + 2^-7), the
//     fp64 roundings of a, b, kappa and the norms (2^-29 u each).
//   * centring, as for prune_bound32_kernel: t sc - c may be contracted to one fma, an ABSOLUTE shift delta of a with
//     |delta| <= 1.21 eps (|c| + A); it moves the exponent by <= 2 r |delta| + |delta|^2 <= 2.5 eps (A + B) (|c| + A).
//   * so k lies in [k^ e^-eta0, k^ e^eta0] with eta0 = (K + 8) u (A + B)^2 + 2.5 eps (A + B) (|c| + A), k^ the exact
//     power of the computed exponent.  v_exp_f32 (1 ulp, allowed 4 u), alpha -> fp32 (u) and the 16 fma of one fp32
//     partial sum (16 u of sum |alpha| k^, the terms of S32 below) are relative too: with
//         eta = eta0 + 24 u       (4.1 + 1.01 + 16.1 and room)
//     |sum alpha_i (k^_i - k_i)| <= (e^eta - 1) sum |alpha_i| k^_i.  The kernel accumulates S32 = sum |alpha_i| k^_i
//     beside mu32, one v_fmac more per value (none over the sign-sorted stream, SGN below: there S32 is the sum of
//     |partial sum of mu32|, the same bits); summed like mu32 it is below the exact sum by <= 17 u of it and is taken
//     times 1 + 2^-16, expm1 times 1 + 2^-20.
//   * gate: eta <= 2^-8 keeps e^eta - 1 a small multiple of eta (and k^ <= e^eta where a candidate sits on a training
//     point).  It needs B, which the staging threads carry with the tiles (max over the rows < n; the pre-split stream
//     has it in its header), so it is decided after the last tile.  Gate failed: e32 = +inf, the block's bound is -inf.
//   * flushes: a kernel value, an alpha or a product with alpha below 2^-126 may become 0: 2^-120 (sum |alpha| + N),
//     absolute, so this term keeps sum |alpha|.  The matrix instruction flushes nothing; a part of an entry below 2^-126
//     that the conversion to bf16 might flush moves the exponent by less than 2^-100, which is inside the room of the
//     24 u.  sum |alpha| is a property of the fit, not of a candidate: the staging lanes add |alpha| of the row they
//     convert, in fp64 from the fp64 alpha, once per row and workgroup (N eps relative; the pre-split stream's header
//     carries the same sum, added in the same order: the same bits), and the sum is taken times
//     1 + 2^-16, which also covers |fl32(alpha)| <= |alpha| (1 + u) where the fp32 alphas are meant.
// |mu32 - mu| <= e32 = amp ((e^eta - 1) S32 + 2^-120 (sum|alpha| + N)); the slack is prune_bound_kernel's with
// S <= amp sum|alpha| plus 2 e32 (pr_slack).  At C3 the maxima A + B ~ 9.5 and S32 <= 5e4 (against sum|alpha| = 1.9e6) put it
// below 10 (the fp32 chain's: below 8; "coarse kept 0" holds below 45); replayed on 256 of C3's candidates it is at most
// 2.6, 1.0 in the median, 1.27 times the fp32 chain's on the same candidates (profiles/r18_seeds_branch.json), where
// sum|alpha| in the place of S32 would give several hundred and prune nothing.
//
// A block whose bound came out -inf (gate failed: data far wider than the length scale; or a NaN bound) is left to
// prune_bound32_kernel<DPAD, true>, launched behind this kernel: the -inf in bmin is the mark, no other scratch.
// Variants measured: docs/experiments.md, round 13 (the fp32 form), round 17 (what the fp32 MFMA leaves to the vector
// ALU), round 18 (this form), round 19 (the rows split once per fit), round 29 (the rows sorted by alpha's sign),
// round 30 (the row loop pipelined).
#pragma once
#include <utility>

#ifndef PMM_G
#define PMM_G 4             // 32-candidate groups per wavefront (2 measured: docs/experiments.md, round 18)
#endif
#define PMM_ROWS 128        // training rows per LDS tile: one 32-row matrix tile staged by each wavefront
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct PmmSlot { int e, pp, qp; };                       // entry; part of P, part of Q (0 h, 1 m, 2 l); e < 0: a zero slot

template <int DPAD>
struct PmmShape {
    static constexpr int K = DPAD + 2;
    static constexpr int NS = 5 * DPAD + 4;              // small products
    static constexpr int NIS = (NS + 15) / 16, NI = NIS + 1;      // instructions: the small chain, and the big products
    static constexpr int PITCH = 16 * NI + 8;            // bf16 values per LDS row: an odd number of 16-byte units
    static_assert(K <= 16, "the big products stand in one instruction");
    // the pre-split stream (apgp_pack_prune_rows): a 16-byte header (bm2, sal), then per PMM_ROWS-row tile the LDS image
    // of the rows (XPIECES 16-byte pieces) and the tile's fp32 alphas (APIECES)
    static constexpr int XPIECES = PMM_ROWS * PITCH / 8, APIECES = PMM_ROWS / 4, PIECES = XPIECES + APIECES;
    // what stands in k slot i of the chain (slot i % 16 of instruction i / 16); P[1] = Q[0] = 1 have an h part only
    static constexpr PmmSlot slot(int i) {
        if (i >= 16 * NIS) return i - 16 * NIS < K ? PmmSlot{i - 16 * NIS, 0, 0} : PmmSlot{-1, 0, 0};
        if (i < 2 * DPAD) return PmmSlot{2 + i / 2, (i & 1) ? 2 : 0, (i & 1) ? 0 : 2};             // h l, l h
        i -= 2 * DPAD;
        if (i < 2) return i == 0 ? PmmSlot{0, 2, 0} : PmmSlot{1, 0, 2};                            // the norms' l
        i -= 2;
        if (i < DPAD) return PmmSlot{2 + i, 1, 1};                                                 // m m
        i -= DPAD;
        if (i < 2 * DPAD) return PmmSlot{2 + i / 2, (i & 1) ? 1 : 0, (i & 1) ? 0 : 1};             // h m, m h
        i -= 2 * DPAD;
        if (i < 2) return i == 0 ? PmmSlot{0, 1, 0} : PmmSlot{1, 0, 1};                            // the norms' m
        return PmmSlot{-1, 0, 0};
    }
};

// part 0, 1, 2 = h, m, l of p = h + m + l, each a bf16 number (p - h and p - h - m are exact in fp32)
template <int PART>
__device__ __forceinline__ float pmm_part(float p) {
    const float h = (float)(__bf16)p;
    if constexpr (PART == 0) return h;
    const float r = p - h, m = (float)(__bf16)r;
    return PART == 1 ? m : r - m;
}

// Fragment F (k slots 8 F .. 8 F + 7 of the chain) of an operand row out of its fp32 entries (SIDE 0: P, 1: Q).  The slot
// numbers are template arguments and every slot splits its entry anew (the compiler merges the repeats): with the parts
// in an array indexed by slot() the array stayed in scratch memory.
template <int DPAD, int SIDE, int I>
__device__ __forceinline__ __bf16 pmm_slot_value(const float (&entry)[DPAD + 2]) {
    constexpr PmmSlot s = PmmShape<DPAD>::slot(I);
    if constexpr (s.e < 0) return (__bf16)0.0f;
    else return (__bf16)pmm_part<SIDE ? s.qp : s.pp>(entry[s.e]);            // (exact: every part is a bf16 number)
}
template <int DPAD, int SIDE, int F, int... J>
__device__ __forceinline__ bf16x8 pmm_frag(const float (&entry)[DPAD + 2], std::integer_sequence<int, J...>) {
    return bf16x8{pmm_slot_value<DPAD, SIDE, 8 * F + J>(entry)...};
}
// a training row's 2 NI fragments into its LDS row
template <int DPAD, int... F>
__device__ __forceinline__ void pmm_store_row(__bf16* dst, const float (&entry)[DPAD + 2],
                                              std::integer_sequence<int, F...>) {
    ((*(bf16x8*)(dst + 8 * F) = pmm_frag<DPAD, 0, F>(entry, std::make_integer_sequence<int, 8>{})), ...);
}
// a candidate's fragments of lane half h: k slots 8 h .. 8 h + 7 of every instruction (both halves' fragments are formed
// and one is selected per lane: twice the split work, once per candidate and kernel, outside the row loop)
template <int DPAD, int... T>
__device__ __forceinline__ void pmm_cand(bf16x8 (&qop)[PmmShape<DPAD>::NI], const float (&entry)[DPAD + 2], int h,
                                         std::integer_sequence<int, T...>) {
    ((qop[T] = h ? pmm_frag<DPAD, 1, 2 * T + 1>(entry, std::make_integer_sequence<int, 8>{})
                 : pmm_frag<DPAD, 1, 2 * T>(entry, std::make_integer_sequence<int, 8>{})), ...);
}

// The pre-split stream of a fit (apgp_pack_prune_rows): a 16-byte header, then every tile's LDS image as the staging lanes
// of prune_bound_mm32_kernel<DPAD, false> write it (the pad of a row zeroed) and the tile's fp32 alphas.  The header holds
// bm2 = max |x - c|^2 over the rows < n and sal = sum |alpha| with the bits that kernel reduces them to: the same lanes
// add the same rows in the same order, the same shuffle tree, the wavefronts' sums in order.  One workgroup.
template <int DPAD>
__global__ __launch_bounds__(PR_THREADS) void pmm_pack_rows_kernel(const double* xs, long long n, unsigned char* rows) {
    using SH = PmmShape<DPAD>;
    constexpr int XS = DPAD + 2, PITCH = SH::PITCH;
    const double kappa = PR32_KAPPA;
    __shared__ double wmax[PR_THREADS / 64], wsal[PR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
    double cen[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) cen[d] = xs[d];
    double sal = 0.0, bm2 = 0.0;
    const long long ntile = (n + PMM_ROWS - 1) / PMM_ROWS;
    const int srow = w * 32 + l32;
    if (h == 0) {
        for (long long ti = 0; ti < ntile; ++ti) {
            const f64x2* src = (const f64x2*)(xs + (ti * PMM_ROWS + srow) * XS);
            f64x2 pre[XS / 2];
#pragma unroll
            for (int i = 0; i < XS / 2; ++i) pre[i] = src[i];
            const bool in = ti * PMM_ROWS + srow < n;
            unsigned char* tile = rows + 16 + ti * (16ll * SH::PIECES);
            __bf16* xrow = (__bf16*)tile + srow * PITCH;
            // (the conversion is the staging lanes' of prune_bound_mm32_kernel<DPAD, false>, statement for statement;
            // tests/test_gpu_prune_rows.py holds the two to the same bits.  Tried twice as one force-inlined function
            // of (row, in, centre) -> (LDS row image, fp32 alpha, bm2, sal): hipcc then packs the bf16 pairs of both
            // kernels another way (v_perm_b32 / v_alignbit_b32 for some v_cvt_pk_bf16_f32, fewer v_cndmask_b32) and this
            // kernel's VGPR count moves, 76 -> 58 at Dpad = 8: profiles/r20_bound_asm_compare.txt)
            float pe[DPAD + 2];                          // P's entries
            double n2 = 0.0, b2 = 0.0;
#pragma unroll
            for (int d = 0; d < DPAD; ++d) {
                const double x = (d & 1) ? pre[d >> 1].y : pre[d >> 1].x;
                const double df = x - cen[d];
                b2 = fma(df, df, b2);
                const float bf = in ? (float)(df * kappa) : 0.0f;
                n2 = fma((double)bf, (double)bf, n2);
                pe[d + 2] = 2.0f * bf;
            }
            if (in) { bm2 = fmax(bm2, b2); sal += fabs(pre[DPAD / 2].x); }
            pe[0] = -(float)n2;
            pe[1] = 1.0f;
            pmm_store_row<DPAD>(xrow, pe, std::make_integer_sequence<int, 2 * SH::NI>{});
            ((float*)(tile + 16 * SH::XPIECES))[srow] = in ? (float)pre[DPAD / 2].x : 0.0f;
            *(bf16x8*)(xrow + 16 * SH::NI) = bf16x8{(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f,
                                                    (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};      // the pad
        }
    }
    for (int o = 32; o > 0; o >>= 1) { bm2 = fmax(bm2, __shfl_xor(bm2, o)); sal += __shfl_xor(sal, o); }
    if (lane == 0) { wmax[w] = bm2; wsal[w] = sal; }
    __syncthreads();
    if (tid == 0) {
        sal = 0.0;
#pragma unroll
        for (int i = 0; i < PR_THREADS / 64; ++i) { bm2 = fmax(bm2, wmax[i]); sal += wsal[i]; }
        ((double*)rows)[0] = bm2;
        ((double*)rows)[1] = sal;
    }
}

// The sign-sorted stream of a fit (apgp_pack_prune_srows): the same tile images and fp32 alphas as the pre-split stream,
// behind a header of PMM_SHDR bytes (bm2, sal, nrt, 0), with the rows in another order, so that the 16 rows a lane of
// the bound kernel accumulates -- one half h of one 32-row matrix tile -- carry alphas of ONE sign:
//   * class P: the rows < n whose alpha is not below 0 (+0 and -0 among them), in their original order; class N: the
//     rows with alpha < 0, in their original order.  gP = ceil(|P| / 16), gN = ceil(|N| / 16).
//   * group q < gP holds P's rows 16 q .. 16 q + 15, group gP + q holds N's; group q is half q & 1 of matrix tile q >> 1,
//     its slot s the tile's row (s & 3) + 8 (s >> 2) + 4 (q & 1): pmm_srow.  nrt = ceil((gP + gN) / 2) matrix tiles hold a
//     row; the stream has room for pmm_stiles(n) staged tiles, enough for any split of n rows into the two classes.
//   * every slot without a row is a padding row of the pre-split stream: coordinates and norm 0, the "1" entry 1, alpha 0.
//   * bm2 is a maximum and has no order.  sal: thread t of the PR_THREADS adds |alpha| of the rows t, t + PR_THREADS, ..
//     in fp64 in that order, then the wavefront's shuffle tree (xor 32, 16, .. 1), then the wavefronts' sums in order.
// One workgroup.  A round places PR_THREADS consecutive rows: a row's rank in its class is the class's count before the
// round, plus the counts of the wavefronts before its own, plus the set bits below its lane in the class's ballot.
__host__ __device__ inline long long pmm_srow(long long q, int s) {
    return 32 * (q >> 1) + (s & 3) + 8 * (s >> 2) + 4 * (int)(q & 1);
}
__host__ __device__ inline long long pmm_stiles(long long n) {        // ceil(n / 16) + 1 groups at most, two per matrix tile
    const long long nrt_max = ((n + 15) / 16 + 2) / 2;
    return (nrt_max + PMM_ROWS / 32 - 1) / (PMM_ROWS / 32);
}
#define PMM_SHDR 32

// one row's LDS image and fp32 alpha into their place in a tile of a stream (the statements of pmm_pack_rows_kernel)
template <int DPAD>
__device__ __forceinline__ void pmm_put_row(unsigned char* tile, int srow, const float (&pe)[DPAD + 2], float alpha) {
    using SH = PmmShape<DPAD>;
    __bf16* xrow = (__bf16*)tile + srow * SH::PITCH;
    pmm_store_row<DPAD>(xrow, pe, std::make_integer_sequence<int, 2 * SH::NI>{});
    ((float*)(tile + 16 * SH::XPIECES))[srow] = alpha;
    *(bf16x8*)(xrow + 16 * SH::NI) = bf16x8{(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f,
                                            (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};              // the pad
}

template <int DPAD>
__global__ __launch_bounds__(PR_THREADS) void pmm_pack_srows_kernel(const double* xs, long long n, unsigned char* rows) {
    using SH = PmmShape<DPAD>;
    constexpr int XS = DPAD + 2, NW = PR_THREADS / 64;
    const double kappa = PR32_KAPPA;
    __shared__ int wp[2][NW], wn[2][NW];
    __shared__ double wmax[NW], wsal[NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double cen[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) cen[d] = xs[d];
    // |P|
    int cnt = 0;
    for (long long i = tid; i < n; i += PR_THREADS) cnt += xs[i * XS + DPAD] < 0.0 ? 0 : 1;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) wp[0][w] = cnt;
    __syncthreads();
    long long np = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) np += wp[0][i];
    __syncthreads();                                     // (wp[0] is written again in round 0)
    const long long nn = n - np, gp = (np + 15) / 16, gn = (nn + 15) / 16;
    unsigned char* img = rows + PMM_SHDR;
    double sal = 0.0, bm2 = 0.0;
    long long base_p = 0, base_n = 0;                    // rows of either class before this round
    const long long nround = (n + PR_THREADS - 1) / PR_THREADS;
    for (long long rd = 0; rd < nround; ++rd) {
        const long long i = rd * PR_THREADS + tid;
        const bool in = i < n;
        const f64x2* src = (const f64x2*)(xs + (in ? i : 0) * XS);
        f64x2 pre[XS / 2];
#pragma unroll
        for (int j = 0; j < XS / 2; ++j) pre[j] = src[j];
        const double alpha = pre[DPAD / 2].x;
        const bool neg = in && alpha < 0.0, pos = in && !neg;
        const unsigned long long mp = __ballot(pos), mn = __ballot(neg), below = (1ull << lane) - 1ull;
        const int b = (int)(rd & 1);                     // two sets of counts: one barrier per round
        if (lane == 0) { wp[b][w] = __popcll(mp); wn[b][w] = __popcll(mn); }
        __syncthreads();
        long long k = pos ? base_p : base_n;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if (j < w) k += pos ? wp[b][j] : wn[b][j];
            base_p += wp[b][j];
            base_n += wn[b][j];
        }
        k += __popcll((pos ? mp : mn) & below);
        if (in) {
            float pe[DPAD + 2];                          // P's entries, as pmm_pack_rows_kernel forms them
            double n2 = 0.0, b2 = 0.0;
#pragma unroll
            for (int d = 0; d < DPAD; ++d) {
                const double x = (d & 1) ? pre[d >> 1].y : pre[d >> 1].x;
                const double df = x - cen[d];
                b2 = fma(df, df, b2);
                const float bf = (float)(df * kappa);
                n2 = fma((double)bf, (double)bf, n2);
                pe[d + 2] = 2.0f * bf;
            }
            bm2 = fmax(bm2, b2);
            sal += fabs(alpha);
            pe[0] = -(float)n2;
            pe[1] = 1.0f;
            const long long r = pmm_srow((pos ? 0 : gp) + (k >> 4), (int)(k & 15));
            pmm_put_row<DPAD>(img + r / PMM_ROWS * (16ll * SH::PIECES), (int)(r % PMM_ROWS), pe, (float)alpha);
        }
    }
    // the slots without a row
    for (long long r = tid; r < pmm_stiles(n) * PMM_ROWS; r += PR_THREADS) {
        const int rr = (int)(r & 31), s = (rr & 3) + 4 * (rr >> 3);
        const long long q = 2 * (r >> 5) + ((rr >> 2) & 1);
        const bool empty = q < gp ? 16 * q + s >= np : q < gp + gn ? 16 * (q - gp) + s >= nn : true;
        if (empty) {
            float pe[DPAD + 2];
#pragma unroll
            for (int d = 0; d < DPAD; ++d) pe[d + 2] = 0.0f;
            pe[0] = -0.0f;                               // (the pre-split stream's padding row: its norm is negated)
            pe[1] = 1.0f;
            pmm_put_row<DPAD>(img + r / PMM_ROWS * (16ll * SH::PIECES), (int)(r % PMM_ROWS), pe, 0.0f);
        }
    }
    for (int o = 32; o > 0; o >>= 1) { bm2 = fmax(bm2, __shfl_xor(bm2, o)); sal += __shfl_xor(sal, o); }
    if (lane == 0) { wmax[w] = bm2; wsal[w] = sal; }
    __syncthreads();
    if (tid == 0) {
        sal = 0.0;
#pragma unroll
        for (int i = 0; i < NW; ++i) { bm2 = fmax(bm2, wmax[i]); sal += wsal[i]; }
        ((double*)rows)[0] = bm2;
        ((double*)rows)[1] = sal;
        ((long long*)rows)[2] = (gp + gn + 1) / 2;
        ((long long*)rows)[3] = 0;
    }
}

// PRE: the training rows come pre-split (PruneArgs::prune_rows, pmm_pack_rows_kernel): staging is a copy of the next
// tile's image into the other of two LDS buffers, one barrier per tile, and bm2 and sal come from the stream's header.
// SGN (with PRE): the stream is the sign-sorted one (pmm_pack_srows_kernel).  The 16 rows of a lane's fp32 partial sum
// then carry alphas of one sign, every term k alpha of the chain ps = fma(k, alpha, ps) has that sign (or is zero), and
// the chain on |alpha| is its mirror image: negating every product and the accumulator negates every rounded result
// (round to nearest is symmetric), so pS == |ps| bit for bit and the second chain is not run.  The error analysis
// above carries over term by term: each partial sum is still an fp32 chain of 16 fma, S32 is still below the exact sum
// by <= 17 u of it; only the order of the rows, which it never used, is another.  The matrix tiles are taken up to the
// header's nrt: the last staged tile may hold one to four.
// PIPE (with PRE and SGN): the same statements in a pinned order of issue, consume_pipe below; no value is formed otherwise.
template <int DPAD, bool PRE = false, bool SGN = false, bool PIPE = false>
__global__ __launch_bounds__(PR_THREADS, PMM_G <= 4 ? 2 : 1) void prune_bound_mm32_kernel(PruneArgs a) {
    static_assert(PRE || !SGN, "the sign-sorted rows come as a stream only");
    static_assert((PRE && SGN) || !PIPE, "the pipelined row loop is written for the sign-sorted stream");
    static_assert(!PIPE || (PMM_G == 4 && PMM_ROWS == 128), "consume_pipe: four groups alternate two accumulator tiles, four matrix tiles alternate two register sets");
    using SH = PmmShape<DPAD>;
    constexpr int XS = DPAD + 2;                         // packed stream row: scaled x | alpha | 0
    constexpr int K = SH::K, NI = SH::NI, PITCH = SH::PITCH, G = PMM_G;
    static_assert(PMM_G % 2 == 0 && PMM_ROWS == 32 * (PR_THREADS / 64), "one 32-row tile staged per wavefront");
    const double kappa = PR32_KAPPA;                     // sqrt(log2(e))
    static_assert(SH::XPIECES * 8 == PMM_ROWS * PITCH && SH::APIECES * 4 == PMM_ROWS, "the stream's tile is the LDS image");
    constexpr int NB = PRE ? 2 : 1;                      // LDS buffers
    __shared__ __attribute__((aligned(16))) __bf16 xt[NB * PMM_ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) float at[NB * PMM_ROWS];
    __shared__ double wmax[PR_THREADS / 64], wsal[PR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const long long blk0 = ((long long)blockIdx.x * (PR_THREADS / 64) + w) * (G / 2);
    double cen[DPAD], c2 = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; ++d) { cen[d] = a.xs[d]; c2 = fma(cen[d], cen[d], c2); }
    const double cn = sqrt(c2);                          // |c|
    bf16x8 qop[G][NI];                                   // the candidates' side of the product, this lane half's k slots
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
        float q[K];                                      // Q's entries
        double n2 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            q[d + 2] = use ? (float)(ce[d] * kappa) : 0.0f;
            n2 = fma((double)q[d + 2], (double)q[d + 2], n2);
        }
        q[0] = 1.0f;
        q[1] = -(float)n2;
        pmm_cand<DPAD>(qop[g], q, h, std::make_integer_sequence<int, NI>{});
    }
    double accm[G], accs[G], sal = 0.0, bm2 = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) { accm[g] = 0.0; accs[g] = 0.0; }
    long long nrt = 0;                                   // SGN: the matrix tiles that hold a row (wave-uniform)
    if constexpr (SGN) nrt = ((const long long*)a.prune_rows)[2];
    const long long ntile = SGN ? (nrt + PMM_ROWS / 32 - 1) / (PMM_ROWS / 32) : (a.n + PMM_ROWS - 1) / PMM_ROWS;
    // one staged tile: its first nr (SGN; else all PMM_ROWS / 32) matrix tiles against the G candidate groups
    auto consume = [&](int xo, int ao, int nr) {  // (element offsets of the LDS buffer in xt and at)
#pragma unroll 1
        for (int rt = 0; rt < (SGN ? nr : PMM_ROWS / 32); ++rt) {
            const __bf16* xr = xt + xo + (rt * 32 + l32) * PITCH + 8 * h;
            bf16x8 pop[NI];                              // the training rows' side, this lane half's k slots
#pragma unroll
            for (int t = 0; t < NI; ++t) pop[t] = *(const bf16x8*)(xr + 16 * t);
            float al[16];                                // alpha of accumulator r's row: (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(al + 4 * q) = *(const f32x4*)(at + ao + rt * 32 + 8 * q + 4 * h);
            auto product = [&](int g) {
                f32x16 c = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < NI; ++t) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pop[t], qop[g][t], c, 0, 0, 0);
                return c;
            };
            // Written as a two-tile pipeline, but hipcc issues all G groups' chains first and the vector work behind them
            // (64 accumulators fit), behind the reads of the iteration and their wait: a wavefront waits for LDS, then
            // feeds only the matrix pipe, then only the vector ALU, and overlaps nothing of its own; what overlap there
            // is comes from the SIMD's other wavefront, which belongs to another workgroup and waits at its barriers
            // (tools/probes/mfma_bf16_shadow.hip, mfma_bf16_pipe.hip; docs/experiments.md, rounds 18 and 30).  This loop
            // is kept for the instantiations without PIPE; with PIPE the order is pinned, consume_pipe below.
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
                    if constexpr (!SGN) pS = fmaf(k, fabsf(al[r]), pS);
                }
                accm[g] += (double)ps;
                accs[g] += (double)(SGN ? fabsf(ps) : pS);       // (SGN: one sign per 16 rows, |ps| IS the chain on |alpha|)
                cur = nxt;
            }
        }
    };
    // PIPE: the same statements per value, in an order of issue that sched_barrier pins (a wavefront overlaps its own
    // LDS reads, matrix products and vector work; docs/experiments.md, round 30):
    //   * a group step runs the 16 exponentials and 16 fma of group g in NI slices, and in front of every slice ONE of
    //     the NI chained matrix products of the NEXT group: the chain's next link finds its predecessor finished, and
    //     the vector lanes never stand behind a burst of products.  Two accumulator tiles live, c0 (even groups) and c1.
    //   * the next group of group G - 1 is group 0 of the next matrix tile, whose fragments and alphas go into the other
    //     of two register sets (A: even matrix tiles of a staged tile, B: odd): the fragments in front of this tile's
    //     vector work, the alphas in front of its last group step.
    //   * across the barrier: the last group of a staged tile stays pending in c1 with its alphas in set B, and runs
    //     under group 0 of the next staged tile, whose rows are read behind the barrier.  The last matrix tile of the
    //     call drains: its last group has no product in front.
    // The four matrix tiles of a full staged tile are written out, so that the register sets alternate without moves;
    // only the last staged tile can hold fewer, and takes them one at a time, each drained.
    [[maybe_unused]] f32x16 c0, c1;
    [[maybe_unused]] bf16x8 pA[NI], pB[NI];
    [[maybe_unused]] float alA[16], alB[16];
    // (first, last: the first and the last staged tile of the call; fetch_next: the global loads of the next staged tile)
    auto consume_pipe = [&](int xo, int ao, int nr, bool first, bool last, auto&& fetch_next)
                            __attribute__((always_inline)) {
        auto rdp = [&](int rt, bf16x8 (&p)[NI]) __attribute__((always_inline)) {
            const __bf16* xr = xt + xo + (rt * 32 + l32) * PITCH + 8 * h;
#pragma unroll
            for (int t = 0; t < NI; ++t) p[t] = *(const bf16x8*)(xr + 16 * t);
        };
        auto rda = [&](int rt, float (&al)[16]) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(al + 4 * q) = *(const f32x4*)(at + ao + rt * 32 + 8 * q + 4 * h);
        };
        // The vector work of group g (exponents cc, alphas al); NEXT: under the product of group gn with the rows pn -> cn
        // (else pn, gn and cn are not used).  The matrix product, the exponential and the fma have no side effect, and instruction selection orders such
        // nodes by register pressure before the scheduler ever sees a sched_barrier: written plainly, all products
        // came out in a burst again.  So every slice ties its values to its place with empty asm statements (no
        // instruction, no move: each names a register set in place), which ARE ordered against the barriers.
        auto step = [&](auto next, f32x16& cc, const float (&al)[16], int g, f32x16& cn, const bf16x8 (&pn)[NI],
                        int gn) __attribute__((always_inline)) {
            constexpr bool NEXT = decltype(next)::value;
            f32x16 c = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            float ps = 0.0f;
#pragma unroll
            for (int t = 0; t < NI; ++t) {
                if constexpr (NEXT) {
                    if (t) asm volatile("" : "+v"(c));
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pn[t], qop[gn][t], c, 0, 0, 0);
                    asm volatile("" : "+v"(c));
                    asm volatile("" : "+v"(cc));
                }
#pragma unroll
                for (int r = 16 * t / NI; r < 16 * (t + 1) / NI; ++r) {
                    const float k = __builtin_amdgcn_exp2f(cc[r]);
                    ps = fmaf(k, al[r], ps);
                }
                if constexpr (NEXT) {
                    asm volatile("" : "+v"(ps));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            accm[g] += (double)ps;
            accs[g] += (double)fabsf(ps);                // (one sign per 16 rows, |ps| IS the chain on |alpha|)
            if constexpr (NEXT) cn = c;
        };
        const std::true_type under{};
        const std::false_type alone{};
        auto product0 = [&](const bf16x8 (&p)[NI]) __attribute__((always_inline)) {
            f32x16 c = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < NI; ++t) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p[t], qop[0][t], c, 0, 0, 0);
            c0 = c;
        };
        // a matrix tile with its rows in (p, al) and group 0 in c0; MORE: the next one's rows go into (pn, aln) and its
        // group 0 into c0; else group G - 1 is left pending in c1
        auto tile = [&](auto more, int rt, const bf16x8 (&p)[NI], const float (&al)[16], bf16x8 (&pn)[NI], float (&aln)[16])
                        __attribute__((always_inline)) {
            constexpr bool MORE = decltype(more)::value;
            if constexpr (MORE) rdp(rt + 1, pn);         // a whole tile ahead of their first use, in the last group step
            step(under, c0, al, 0, c1, p, 1);
            step(under, c1, al, 1, c0, p, 2);
            step(under, c0, al, 2, c1, p, 3);
            if constexpr (MORE) {
                rda(rt + 1, aln);                        // a group step ahead: p is dead by now, no register set more
                step(under, c1, al, G - 1, c0, pn, 0);
            }
        };
        if (nr == PMM_ROWS / 32) {
            // a full staged tile, straight-line: no value has two places
            rdp(0, pA);
            rda(0, alA);
            if (first) product0(pA);
            else step(under, c1, alB, G - 1, c0, pA, 0);
            tile(under, 0, pA, alA, pB, alB);
            tile(under, 1, pB, alB, pA, alA);
            tile(under, 2, pA, alA, pB, alB);
            if (!last) fetch_next();                     // (set A is dead from here on: the copy's registers are its)
            tile(alone, 3, pB, alB, pA, alA);
            if (last) step(alone, c1, alB, G - 1, c0, pA, 0);
        } else {
            // the last staged tile where it holds fewer than four matrix tiles: one at a time, each drained
#pragma unroll 1
            for (int rt = 0; rt < nr; ++rt) {
                rdp(rt, pA);
                rda(rt, alA);
                if (rt == 0 && !first) step(under, c1, alB, G - 1, c0, pA, 0);
                else product0(pA);
                tile(alone, rt, pA, alA, pB, alB);
                step(alone, c1, alA, G - 1, c0, pA, 0);
            }
        }
    };
    if constexpr (PRE) {
        // every thread copies pieces tid, tid + 256, .. of a tile (the last round is partial: a clamped load, a guarded
        // store); loaded before the tile in LDS is consumed, written behind it.  Past the last tile the last one is copied
        // again, into the buffer nobody reads any more: no branch around the loads.
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        constexpr int NPC = SH::PIECES, NL = (NPC + PR_THREADS - 1) / PR_THREADS;
        const u32x4* img = (const u32x4*)((const unsigned char*)a.prune_rows + (SGN ? PMM_SHDR : 16));
        u32x4 pre[NL];
        auto fetch = [&](long long ti) {
            const u32x4* src = img + ti * NPC;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int e = tid + j * PR_THREADS;
                pre[j] = src[e < NPC ? e : NPC - 1];
            }
        };
        auto put = [&](int b) {
            u32x4* xd = (u32x4*)(xt + b * PMM_ROWS * PITCH);
            u32x4* ad = (u32x4*)(at + b * PMM_ROWS);
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int e = tid + j * PR_THREADS;
                if ((j + 1) * PR_THREADS <= SH::XPIECES || e < SH::XPIECES) xd[e] = pre[j];
                else if (e < NPC) ad[e - SH::XPIECES] = pre[j];
            }
        };
        fetch(0);
        put(0);
        __syncthreads();
        for (long long ti = 0; ti < ntile; ++ti) {
            const int b = (int)(ti & 1);
            if constexpr (!PIPE) fetch(ti + 1 < ntile ? ti + 1 : ntile - 1);
            const long long left = nrt - ti * (PMM_ROWS / 32);           // (SGN alone)
            if constexpr (PIPE) {
                // the next tile is loaded in front of this one's last matrix tile, where a register set is free, and
                // there is no copy behind the last staged tile
                consume_pipe(b * PMM_ROWS * PITCH, b * PMM_ROWS, left < PMM_ROWS / 32 ? (int)left : PMM_ROWS / 32, ti == 0,
                             ti + 1 == ntile, [&]() __attribute__((always_inline)) { fetch(ti + 1); });
                if (ti + 1 < ntile) put(b ^ 1);
            } else {
                consume(b * PMM_ROWS * PITCH, b * PMM_ROWS, left < PMM_ROWS / 32 ? (int)left : PMM_ROWS / 32);
                put(b ^ 1);
            }
            __syncthreads();                             // the next tile is in; this one has been consumed
        }
        bm2 = ((const double*)a.prune_rows)[0];
        sal = ((const double*)a.prune_rows)[1];
    } else {
        // staging: lane l32 of half 0 of wavefront w converts row 32 w + l32 of the tile
        const bool stager = h == 0;
        const int srow = w * 32 + l32;
        f64x2 pre[XS / 2];
        auto fetch = [&](long long ti) {                 // (rows < ntile * PMM_ROWS <= npad: inside the packed stream)
            const f64x2* src = (const f64x2*)(a.xs + (ti * PMM_ROWS + srow) * XS);
#pragma unroll
            for (int i = 0; i < XS / 2; ++i) pre[i] = stager ? src[i] : f64x2{0.0, 0.0};
        };
        fetch(0);
        for (long long ti = 0; ti < ntile; ++ti) {
            if (stager) {
                const bool in = ti * PMM_ROWS + srow < a.n;  // rows of the padding: operands 0, alpha 0, no part in B
                float pe[K];                             // P's entries
                double n2 = 0.0, b2 = 0.0;
#pragma unroll
                for (int d = 0; d < DPAD; ++d) {
                    const double x = (d & 1) ? pre[d >> 1].y : pre[d >> 1].x;
                    const double df = x - cen[d];
                    b2 = fma(df, df, b2);
                    const float bf = in ? (float)(df * kappa) : 0.0f;
                    n2 = fma((double)bf, (double)bf, n2);
                    pe[d + 2] = 2.0f * bf;
                }
                if (in) { bm2 = fmax(bm2, b2); sal += fabs(pre[DPAD / 2].x); }
                pe[0] = -(float)n2;
                pe[1] = 1.0f;
                pmm_store_row<DPAD>(xt + srow * PITCH, pe, std::make_integer_sequence<int, 2 * NI>{});
                at[srow] = in ? (float)pre[DPAD / 2].x : 0.0f;
            }
            __syncthreads();
            if (ti + 1 < ntile) fetch(ti + 1);
            consume(0, 0, PMM_ROWS / 32);
            __syncthreads();                             // the tile has been consumed
        }
        // B = max |x - c| and sum |alpha| over the training rows: the stagers' maxima and sums, over the workgroup (every
        // workgroup adds the same rows in the same order: one value of sum |alpha| per call)
        for (int o = 32; o > 0; o >>= 1) { bm2 = fmax(bm2, __shfl_xor(bm2, o)); sal += __shfl_xor(sal, o); }
        if (lane == 0) { wmax[w] = bm2; wsal[w] = sal; }
        __syncthreads();
        sal = 0.0;
#pragma unroll
        for (int i = 0; i < PR_THREADS / 64; ++i) { bm2 = fmax(bm2, wmax[i]); sal += wsal[i]; }
    }
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
        const double eta = (DPAD + 10.0) * u32 * ab * ab + 2.5 * eps * ab * (cn + an[g]) + 24.0 * u32;
        double e32 = a.amp * (expm1(eta) * (1.0 + 0x1p-20) * s32 + 0x1p-120 * (sa + (double)a.n));
        if (!(eta <= 0x1p-8)) e32 = INFINITY;
        bbe = fmin(bbe, pr_block_min<32>(b, adm[g]));
        bb = fmin(bb, pr_block_min<32>(b - pr_slack<DPAD>(a, 2.0 * e32, a.amp * sa, mu, ktt, b), adm[g]));
        if (g & 1) {                                     // both 32-candidate groups of block blk0 + g / 2 are in
            const long long blk = blk0 + (g >> 1);
            if (lane == 0 && blk < a.ncb) pr_store_block<true>(a, blk, bb, bbe);
            bb = INFINITY; bbe = INFINITY;
        }
    }
}
