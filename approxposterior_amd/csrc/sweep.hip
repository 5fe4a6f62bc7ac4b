// K5/K6 "sweep": fused candidate tile -> k* row -> mu -> L^-1 k* contraction on
// the f64 matrix cores -> predictive variance -> AGP / BAPE / Jones utility ->
// arg-min.  The batched counterpart of
//   george.GP.predict(y, t, return_var=True)        (utility.py:131,178,224)
//   utility.AGPUtility / BAPEUtility / JonesUtility (utility.py:99-250)
//   utility.minimizeObjective's arg-min             (utility.py:369-371)
//
// One kernel implements it: sweep2_kernel, the two-role kernel further down (matrix wavefronts
// + feeder wavefronts); a short last round of the persistent grid is split by row block and
// finished by sweep_finish_kernel.  In the pruned arg-min's seed launch the heavy row blocks of such a split go as two
// row-half items each, put together by sweep_fold_kernel before sweep_finish_kernel ("row-half items" below).
//
// Data flow per workgroup (512 threads = 4 matrix + 4 feeder wavefronts, 64 candidates):
//   * matrix / feeder wavefront w owns candidates [16 w, 16 w + 16) (one MFMA column block).
//   * the packed factor W = L^-1 is streamed tile by tile (the 256-row halves of the packed
//     512 rows x 16 k tiles, 32 KiB, A-fragment order) L2/MALL -> LDS by LDS-DMA (ring of
//     three slots), shared by the four matrix wavefronts.
//   * the feeder generates the k*(t_m, x_k) values the MFMA B operand needs (lane ->
//     candidate lane&15, k lane>>4) on the VALU (D sub + D fma + table-driven exp) the
//     FIRST time chunk k is visited (the diagonal row block); later row blocks need the same
//     operands again, and because the fp64 VALU shares the DP pipe with the matrix cores,
//     regenerating them costs ~12 % of a tile.  They are parked in a per-workgroup-slot
//     scratch stream instead (32 B per lane per chunk, written once, read back by LDS-DMA)
//     -- K* is still never materialised as a matrix the host sees.  The grid is persistent
//     (one workgroup per CU, candidate blocks dealt round-robin) so the scratch is SW_GRID
//     slots, not M/64.
//   * V = W K*^T is accumulated 256 rows x 16 candidates per matrix wavefront in 64
//     v_mfma_f64_4x4x4_4b_f64 accumulators; at the end of a row block the squares are folded
//     into a per-candidate sum; V is never stored.
//   * mu is a VALU by-product of the generating tiles (every k exactly once).
#include "apgp_common.h"
#include "mma16.h"
#include "scratch.h"
#include "util_value.h"             // util_value: the utilities, shared with nmsearch.hip
#include <mutex>
#include <stdlib.h>
#include <string.h>

#define SW_ROWS APGP_ROW_BLOCK       // 512 rows of W per tile
#define SW_KC APGP_K_CHUNK           // 16 k per tile
#define SW_TILE (SW_ROWS * SW_KC)    // doubles per tile (64 KiB)
#define SW_CAND 64                   // candidates per workgroup (16 per wavefront)
#define SW_GRID 256                  // persistent workgroups = K* scratch slots (one per CU)
#define SW_BCH 1024                  // doubles of parked B operands per chunk per slot (4 wavefronts x 64 lanes x 4 k)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// cache policy of the parked-operand stream (aux bits of its buffer loads / stores): 0 = default.
// Each workgroup slot is written once and read back once per later row block and 256 slots x
// 2 MB never fit the L2, so a non-temporal hint (aux 2) looked right -- measured alternating on
// one box with the two-role kernel it is 0.5 % slower than the default policy (256.5 vs 257.9 ms).
#ifndef SW_KAUX
#define SW_KAUX 0
#endif

struct SweepArgs {
    const double* T;
    const double* linv;
    const double* xs;
    const unsigned char* mask;
    double* mu;
    double* var;
    double* u;
    double* part_u;
    long long* part_i;
    double* kcache;            // parked B operands: SW_GRID slots x ncache chunks x SW_BCH
    unsigned linv_bytes, xs_bytes, kslot_bytes;   // buffer-descriptor extents
    // candidate blocks [blk_begin, blk_end) of this launch; split != 0: one workgroup per
    // (candidate block, row block), partial sums to sp_q / sp_mu (the short last round)
    long long blk_begin, blk_end;
    double* sp_q;
    double* sp_mu;
    int split;
    long long m, idx_offset;
    int ndim, nrb, kind, has_box, n, ncache, lin_order;
    double mean, amp, zeta, ybest, lin_coef;
    double sc[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM], lw[APGP_MAX_DIM];
    // pruned sweep (sweep2_kernel<.., LIST = true>, sweep_finish_kernel): "candidate block k of this launch" is
    // blk_list[k], k < *blk_count -- a count the device computed; the launch is sized for the largest count it may
    // meet and does nothing unless list_lo < *blk_count <= list_hi
    const long long* blk_list;
    const long long* blk_count;
    long long list_lo, list_hi;
};

__device__ __forceinline__ void best_merge(double& bu, long long& bi, double u, long long i) {
    // NaN and +inf (inadmissible) never win; ties resolve to the lowest global index
    if (i >= 0 && u < INFINITY && (u < bu || (u == bu && (bi < 0 || i < bi)))) { bu = u; bi = i; }
}

// Matrix-core instruction choice (measured on MI355X, tools/mfma_peak.hip and
// tools/mfma_probe.hip):
//   v_mfma_f64_16x16x4_f64     36 TF/chip  (~138 cycles, 7.4 MAC/clk/SIMD)
//   v_mfma_f64_4x4x4_4b_f64    70-75 TF    (16.5 cycles, 15.5 MAC/clk/SIMD = FP64 FMA peak)
//   v_fma_f64 (VALU)           64-70 TF, and MFMA + VALU f64 do NOT overlap: they
//                              share the DP pipes (sum stays ~70 TF for any mix).
// So the contraction uses the 4x4x4 four-block instruction.  Its blocks are
// independent (CBSZ/ABID broadcast is ignored for f64 on gfx950):
//   A lane = i + 4 b + 16 k,  B lane = j + 4 b + 16 k,  D lane = j + 4 b + 16 i.
// A 16 x 16 x 4 product is four instructions with the SAME A fragment and the B
// operand rotated by 4 r lanes inside each row of 16 lanes (DPP row_ror): block b
// then multiplies row group b with candidate group (b + r) mod 4.  The candidate
// of an accumulator depends on r, which the variance reduction (sum over rows of
// V^2 per candidate) undoes once per row block with the inverse rotation.
// (Rotating the A fragment instead keeps lane <-> candidate fixed but needs four
// times the LDS reads and A registers: it ran the LDS at 73 % of its bandwidth.)

// K6: final arg-min over the per-workgroup partials (one workgroup).
__global__ __launch_bounds__(1024) void argmin_final_kernel(const double* part_u, const long long* part_i,
                                                            long long nparts, apgp_best_t* best) {
    __shared__ double su[16];
    __shared__ long long si[16];
    double bu = INFINITY;
    long long bi = -1;
    for (long long p = threadIdx.x; p < nparts; p += 1024) best_merge(bu, bi, part_u[p], part_i[p]);
    for (int o = 32; o > 0; o >>= 1) {
        double ou = __shfl_xor(bu, o);
        long long oi = __shfl_xor(bi, o);
        best_merge(bu, bi, ou, oi);
    }
    if ((threadIdx.x & 63) == 0) { su[threadIdx.x >> 6] = bu; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) best_merge(bu, bi, su[i], si[i]);
        best->u = bu;
        best->index = bi;
    }
}

// ===========================================================================
// Two-role sweep (round 1e): 8 wavefronts per workgroup, two per SIMD.
//   wavefronts 0-3 ("matrix" role, one per SIMD): nothing but the MFMA stream, the LDS reads
//     of its operands and one barrier per tile.  256 rows x 16 candidates per wavefront
//     (64 accumulators): the 256 unified registers of a two-wave-per-SIMD kernel hold them.
//   wavefronts 4-7 ("feeder" role): everything else -- the packed-factor stream L2 -> registers
//     -> LDS, the B operands (generated on the first visit of a chunk, otherwise fetched from
//     the parked stream) written to LDS for the matrix wavefront of the same candidates, mu,
//     the candidate setup and the utility / arg-min epilogue.
// tools/mfma_pair.hip: the SIMD issues the older wavefront first, so a companion's LDS / VMEM /
// integer traffic costs the MFMA wavefront nothing (16.25 -> 16.4 cycles per MFMA), while in
// the one-wave design every such instruction's issue time is lost to the matrix pipe (~15 %).
// Only the feeder's fp64 VALU work (k* generation) still competes for the shared DP pipe.
// Tiles are the 256-row HALVES of the packed 512 x 16 tiles (same packed format): row block jb
// = half jb & 1 of packed row block jb >> 1, chunks 0 .. 16 (jb + 1) - 1.
// Synchronisation: tile i+1 (A image into slot (i+1) % 3, B operands into buffer (i+1) & 1) is
// written by the feeders between barrier i-1 and barrier i; the matrix wavefronts execute
// barrier i after the first k-step of pair 4 of tile i and read tile i+1 only after it.
// ===========================================================================
#define S2_THREADS 512
// LDS reads of the matrix role are issued one per S2_SPREAD MFMAs instead of in clusters of four
// (sched_group_barrier): clustered, the reads' issue time exceeds one MFMA's 16-cycle shadow and
// the matrix pipe idles (same box, alternating: 249.5 vs 255.0 ms at C3).  0 = compiler's order.
#ifndef S2_SPREAD
#define S2_SPREAD 1
#endif
#define S2_ROWS 256
#define S2_TILE (S2_ROWS * SW_KC)        // doubles per tile image (32 KiB)
#define S2_CPB (S2_ROWS / SW_KC)         // chunks per row-block width (16)
#define S2_NP (S2_ROWS / 32)             // sub-block pairs per tile (8)
// substitution form: the statically unrolled diagonal tiles are used up to this many 256-row blocks
// (N <= 2048), the run-time-indexed body above that (see the matrix role)
#define S2_STATIC_DIAG_NRB 8

// ---- row-half items (the seed launch of the pruned arg-min) ----------------------------------
// A split launch lasts as long as its heaviest item, candidate block x row block nrb - 1 with its 16 nrb tiles, while the
// item of row block 0 walks 16: with one workgroup per CU the chip is half idle.  The rows of a row block are
// independent, so row blocks jb >= J0 go as TWO items, sub-block pairs [4 h, 4 h + 4) each (h = 0, 1): half the image
// bytes, the four-pair tile bodies on acc[0 .. 7].  The bits stay those of the whole item because the chain
// qr[r] = fma(acc[s][r], acc[s][r], qr[r]), s = 0 .. 15, is continued, not re-associated: the h = 0 item stores its
// chain over s = 0 .. 7 (S2_HQ_PRE doubles), the h = 1 item its 32 accumulators per lane (S2_HQ_ACC doubles), and
// sweep_fold_kernel runs the chain on from the prefix through the stored values, then the same gather and
// reductions (s2_q_gather), and writes the share sweep_finish_kernel reads.  No workgroup waits for another.
// Finer row parts (the seed waves, below): a row block >= J0 goes as 2 / 4 / 8 items of 4 / 2 / 1 sub-block pairs, pairs
// [pp p, pp p + pp) for part p.  The chain is continued through all parts in s order: part 0 stores its prefix over
// s = 0 .. 2 pp - 1, every other part its 2 pp x 4 accumulators per lane at their place s of the whole item (the fold
// region holds sub-blocks 2 .. 15: part 0 covers 0 and 1 at least), and the fold runs the chain on from s = 2 pp.
#define S2_HQ_PRE (4 * 256)              // doubles per (position, row block): 4 per matrix lane
#define S2_HQ_ACC (56 * 256)             // doubles per (position, row block): sub-blocks 2 .. 15 x 4 rotations per matrix lane
// The fold inputs lie s2_fold_off doubles behind sp_q, at the end of the caller's scratch (apgp_acquire_work_len): behind
// the split shares and the pruned sweep's 3 ncb + S2_PRUNE_WORDS words, at an even offset (16-byte accesses).  A function
// of the launch's own arguments (ncb = SweepArgs::blk_end in a list launch; split = 2 + J0 there), not a pointer in
// SweepArgs: the kernel's argument block, and with it every other instantiation's code, stays what it was.
#define S2_SPLIT_MAX 184                 // blocks of a last round that are split by row block (see launch_sweep)
#define S2_PRUNE_WORDS 24                // PR_SEED seed block numbers + 8 counters
__host__ __device__ inline long long s2_fold_off(int nrb, long long ncb) {
    return (2ll * S2_SPLIT_MAX * SW_CAND * nrb + 3 * ncb + S2_PRUNE_WORDS + 1) & ~1ll;
}
__host__ __device__ inline double* s2_fold_item(double* sp_q, int nrb, long long ncb, long long pos, int jb) {
    return sp_q + s2_fold_off(nrb, ncb) + (pos * nrb + jb) * (S2_HQ_PRE + S2_HQ_ACC);
}
// cost of a half item's tile against a whole item's: 0.70 measured (N = 2048, one item per CU: 217 against 311 us; the
// feeders' k* and the tile's barrier do not halve with the rows), that is delta = 0.4 (docs/experiments.md, Round 22)
#define S2_HALF_COST 7
#define S2_WHOLE_COST 10
// the parked route of the seed launch (seed_park_kernel): a tile re-read from the parked stream and a generating
// (diagonal) one, per kind of item, in hundredths of a microsecond.  Measured where the launch is one item per CU and
// so lasts its heaviest item (docs/experiments.md, Round 26): whole items, N = 2048 and 1152 at J0 = nrb, 112 + 16 and
// 48 + 16 tiles in 291.4 and 142.9 us: 2.32 re-read, 1.97 generating (a diagonal tile is half empty); half items,
// N = 2048 at J0 = 0 and N = 1152 at J0 = 2, the same tile counts in 184.4 and 110.1 us: 1.16 re-read, 3.40 generating
// (the item's fixed part -- prologue, the upper half's idle last diagonal tiles -- falls to this term).  With them the
// model gives 588 / 457 / 387 us for J0 = 16 / 8 / 0 at N = 4096 (measured 592-602 / 468 / 397).
#define S2P_HALF_GEN 340
#define S2P_HALF_PARK 116
#define S2P_WHOLE_GEN 197
#define S2P_WHOLE_PARK 232
// the two-pair and one-pair items of the parked route, measured the same way (docs/experiments.md, Round 27): a wave
// of fewer items than CUs lasts its heaviest item.  Two pairs: N = 4096 and 2048, 240 + 16 and 112 + 16 tiles in 265.0
// and 139.6 us: 0.98 re-read, 1.87 generating (N = 1024, 48 + 16 tiles: 77.0 modelled, 77.2 measured).  One pair (the
// predicated two-pair body with its second pair off): 221.1 and 116.9 us: 0.81 and 1.61 (N = 1024: 64.8, 65.4 measured).
// Halving an item's rows takes only a sixth off its re-read tile (half: 1.16): the tile waits for its barrier and the
// feeders' fetch, not for its MFMAs (0.22 us per pair).
#define S2P_PAIR2_GEN 187
#define S2P_PAIR2_PARK 98
#define S2P_PAIR1_GEN 161
#define S2P_PAIR1_PARK 81
// the same items through the stage-ring loop (sweep2_kernel<.., DEEP>; docs/experiments.md, Round 31), measured the same
// way (tools/seed_tile_prices.py: first waves of no more items than CUs, every row block split, N = 4096 and 2048,
// checked at N = 1024; profiles/r31_seed_tile_prices.json).  Whole items of that launch keep S2P_WHOLE_*.
#define S2Q_HALF_GEN 220
#define S2Q_HALF_PARK 101
#define S2Q_PAIR2_GEN 183
#define S2Q_PAIR2_PARK 54
#define S2Q_PAIR1_GEN 183
#define S2Q_PAIR1_PARK 45
// what a second wave costs when none of its seeds is swept: four launches that leave at once (4.7 - 5.4 us each)
#define S2P_WAVE2 2000
// ---- the seed waves' launch word (SweepArgs::split of the seed route's launches) -----------------------------------------
// The PR_SEED seeds are swept in two waves, list positions [0, K) and [K, PR_SEED) (launch_sweep_list).  A wave's launches
// carry J0, lg = log2(parts of a split row block) and the wave's positions [P0, P1) in SweepArgs::split: the argument block
// stays what it was.  P0 > 0 marks the second wave, whose K is P0.  (A plain split launch has split = 1: J0 < 0 is never
// read there, lg = P0 = P1 = 0.)  S2W_SEED: the seed route's sweep_finish_kernel, which resets the wave counter.
#define S2W_WORD(j0, lg, p0, p1) ((2 + (j0)) | ((lg) << 8) | ((p0) << 12) | ((p1) << 20))
#define S2W_J0(sp) (((sp) & 0xff) - 2)
#define S2W_LG(sp) (((sp) >> 8) & 3)
#define S2W_P0(sp) (((sp) >> 12) & 31)
#define S2W_P1(sp) (((sp) >> 20) & 31)
#define S2W_SEED (1 << 28)
// ---- the stage ring of a part item (sweep2_kernel<.., DEEP>) ---------------------------------------
// A part item of pp sub-block pairs fills pp of the 8 pieces of a tile slot, and its re-read tiles wait for their fetch,
// not for their MFMAs.  In the DEEP instantiation such an item keeps its tiles in a ring of stages inside the three tile
// slots: stage = the tile's pp image pieces (4 KiB each) followed by its B operands (8 KiB); tile i lies in stage
// i mod R, R = 4 / 6 / 8 for pp = 4 / 2 / 1.  The feeders request the re-read tiles D <= R - 2 tiles ahead (live stages:
// i - 1, read by the matrix wavefronts until their barrier i, to i + D, being filled); the launch carries D in
// bits 25 .. 27 of SweepArgs::split.
#define S2W_PF(sp) (((sp) >> 25) & 7)
#define S2_STAGE(pp) ((pp) * 512 + 2 * 4 * 128)          // doubles per stage
#define S2_NRING(pp) (3 * S2_TILE / S2_STAGE(pp))        // stages in the three tile slots
static_assert(S2_NRING(4) == 4 && S2_NRING(2) == 6 && S2_NRING(1) == 8, "the stage ring fits the three tile slots");
static_assert(S2_NRING(4) * S2_STAGE(4) <= 3 * S2_TILE && S2_NRING(2) * S2_STAGE(2) <= 3 * S2_TILE &&
              S2_NRING(1) * S2_STAGE(1) <= 3 * S2_TILE, "the stage ring fits the three tile slots");
// The counts the loop's wait can ask for are (pp + 2) requests per tile x the tiles requested beyond i+1, at most
// D - 1 <= S2_NRING(pp) - 3 of them: {6} for pp = 4, {4, 8, 12} for pp = 2, {3, 6, 9, 12, 15} for pp = 1, and 1 or 2 behind
// the x fetch of a generating iteration.  These are the cases of the loop's switch; a count it does not list waits
// with vmcnt(0), which is correct but gives the depth away -- a change of the ring must change the switch with it.
static_assert(S2_NRING(4) - 3 == 1 && S2_NRING(2) - 3 == 3 && S2_NRING(1) - 3 == 5, "the DEEP loop's vmcnt cases follow the ring");
__host__ __device__ inline int s2_nkc_of(int jb, int n) {
    const int v = S2_CPB * (jb + 1), lim = (n + SW_KC - 1) / SW_KC;
    return v < lim ? v : lim;
}
// items of row block jb: 2^lg at or above J0, fewer where its rows end sooner (lg = 1: two halves if it has rows in its
// lower half), one (a whole item) otherwise
__host__ __device__ inline int s2_nparts(int jb, int j0, int n, int lg) {
    if (jb < j0 || lg == 0) return 1;
    const int per = S2_ROWS >> lg, c = (n - S2_ROWS * jb + per - 1) / per;
    return c > (1 << lg) ? (1 << lg) : (c < 1 ? 1 : c);
}
// items of one candidate block
__host__ __device__ inline int s2_nitems(int nrb, int j0, int n, int lg) {
    int c = 0;
    for (int jb = 0; jb < nrb; ++jb) c += s2_nparts(jb, j0, n, lg);
    return c;
}
// cost of a tile of an item of 8 >> lg pairs, for the order of the items (lg 0, 1: S2_WHOLE_COST, S2_HALF_COST)
__host__ __device__ inline int s2_part_cost(int lg) { return lg == 0 ? S2_WHOLE_COST : lg == 1 ? S2_HALF_COST : lg == 2 ? 5 : 4; }
// Row item idx of s2_nitems(..), heaviest first by the cost model: the merge of two descending runs -- the row
// blocks >= J0 from the last down (their parts, the last first: its diagonal tiles are the fuller ones; a last block
// with the rows of one part only as one whole item) and the whole row blocks below J0.  h = -1: a whole item.
__host__ __device__ inline void s2_row_item(int idx, int nrb, int j0, int n, int lg, int& jb, int& h) {
    int hj = nrb - 1, hh = hj >= 0 ? s2_nparts(hj, j0, n, lg) - 1 : 0, wj = (j0 < nrb ? j0 : nrb) - 1;
    const int pc = s2_part_cost(lg);
    for (int i = 0;; ++i) {
        if (hj >= j0 && (wj < 0 || pc * s2_nkc_of(hj, n) >= S2_WHOLE_COST * s2_nkc_of(wj, n))) {
            const int np = s2_nparts(hj, j0, n, lg);
            if (i == idx) { jb = hj; h = np > 1 ? hh : -1; return; }
            if (hh > 0) --hh; else { --hj; hh = hj >= 0 ? s2_nparts(hj, j0, n, lg) - 1 : 0; }
        } else {
            if (i == idx || wj < 0) { jb = wj < 0 ? 0 : wj; h = -1; return; }    // (wj < 0: idx past the last item)
            --wj;
        }
    }
}
// gather of the four rotations' sums of squares back to their candidates and the reduction over the 4 row-lanes
// (rotation r's accumulators belong to the candidate of lane (lane & 48) | ((lane + 4 r) & 15)): the fold's copy of the
// lines at the end of the kernel's row block.  (The kernel keeps its own text: called from there, this function moved
// instructions in every instantiation.)
__device__ __forceinline__ double s2_q_gather(const double (&qr)[4], int lane) {
    double qs = qr[0];
#pragma unroll
    for (int r = 1; r < 4; ++r) qs += __shfl(qr[r], (lane & 48) | ((lane - 4 * r) & 15));
    qs += __shfl_xor(qs, 16);
    qs += __shfl_xor(qs, 32);
    return qs;
}
// Second wave (p0 = K > 0): tau_1 = the smallest utility the first wave's seeds found; the seed at `pos` is left alone
// if its bound says it can neither win nor tie.  bmin lies behind the two row-block share tables that start at sp_q.
// Uniform over the workgroup, before its first barrier.
__device__ __forceinline__ bool s2_wave_skip(const SweepArgs& a, int nrb, int p0, long long pos) {
    if (p0 == 0) return false;
    const double* bmin = a.sp_q + 2ll * S2_SPLIT_MAX * SW_CAND * nrb;
    double tau = INFINITY;
    for (int i = 0; i < p0; ++i) tau = fmin(tau, a.part_u[a.blk_list[i]]);       // (fmin: as prune_select_kernel)
    return !(bmin[a.blk_list[pos]] <= tau);
}

// which form of the feeder loop an instantiation gets (see the feeder role)
// (Dpad = 32, round 5: the plain feeder -- an x chunk is 4352 bytes there, more than the four feeder wavefronts' four 1 KiB
// LDS-DMA pieces of the structured form, whose hand-counted vmcnt waits assume exactly one piece per wavefront)
static constexpr bool s2_structured_feeder(int dpad, bool solve) { return dpad == 32 ? false : (solve ? dpad == 2 : dpad != 8); }

// MODE 0: inverse form (A = packed L^-1); 1: substitution form; 2: substitution form with the statically
// unrolled diagonal tiles (N <= 256 S2_STATIC_DIAG_NRB) -- a separate instantiation: the 65 KiB of
// unrolled code slowed the run-time-indexed path of the SAME kernel by 20 % at N = 4096 (333 vs 276 ms;
// identical hot loops, only their placement differs), so large N run the kernel that does not contain it.
// LIST: the candidate blocks of the launch come from a device list (SweepArgs::blk_list) -- an instantiation of its own,
// so that the full sweep's code is what it was before the list existed (this kernel's speed hangs on how hipcc
// allocates its scalars: DESIGN.md section 6, the NaN-refusal episode).  The indirection sits where a block's
// candidates are loaded; the tile loop never sees it.
// RHALF (MODE 0, LIST, split launches only): row blocks >= J0 = a.split - 2 go as two row-half items (above).  Again an
// instantiation of its own: every other one keeps its code.
// DEEP (RHALF without a LinearKernel term; the parked seed launch at apgp_set_seed_prefetch > 0): a part item keeps its tiles
// in a ring of stages and requests its re-read tiles several tiles ahead (S2_STAGE above; the loop at the head of the feeder
// role).  Once more an instantiation of its own.
template <int DPAD, bool LIN, int MODE, bool LIST = false, bool RHALF = false, bool DEEP = false>
__global__ __launch_bounds__(S2_THREADS, 1) void sweep2_kernel(SweepArgs a) {
    static_assert(!RHALF || (MODE == 0 && LIST), "row-half items: inverse form, list launches");
    static_assert(!DEEP || (RHALF && !LIN), "stage ring: the parked seed route");
    constexpr bool SOLVE = MODE != 0;
    // the seed launch of a pure squared-exponential kernel may read its blocks' parked stream (seed_park_kernel):
    // a.ncache > 0 there means "read slot blk0, never store"; with a LinearKernel term the instantiation is what it was
    constexpr bool SPARK = RHALF && !LIN;
    constexpr bool STATIC_DIAG = MODE == 2;
    constexpr int XS = DPAD + 2;
    constexpr int NKK = SW_KC / 4;
    constexpr int NP = S2_NP;
    constexpr int XCHUNK16 = SW_KC * XS / 2;
    // doubles between two x buffers: the chunk itself, or (structured feeder: whole-wavefront LDS-DMA
    // pieces of 1 KiB, ring of three buffers) the chunk rounded up to 1 KiB
    constexpr bool SF = s2_structured_feeder(DPAD, SOLVE);
    constexpr int XSTRIDE = SF ? (SW_KC * XS * 8 + 1023) / 1024 * 128 : SW_KC * XS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* Aring = smem;                         // 3 tile images
    double* Bbuf = Aring + 3 * S2_TILE;           // 2 x 4 wavefronts x [2][64] x 16 B
    double* Xbuf = Bbuf + 2 * 4 * 256;            // 2 x SW_KC x XS
    double* Etab = Xbuf + (SF ? 3 : 2) * XSTRIDE;
    double* Shq = Etab + APGP_EXP_TAB_N;          // sum V^2 per candidate (matrix -> feeder)
    double* red_u = Shq + SW_CAND;
    long long* red_i = (long long*)(red_u + 4);
    double* Cst = red_u + 8;                      // sc | lo | hi | lw (4 x APGP_MAX_DIM), feeder only
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int cl = lane & 15, kq = lane >> 4;
    // blocks [S2_BLK_BEGIN, S2_BLK_END) of this launch; LIST: positions 0 .. count - 1 in the list.  (Macros, not
    // variables: the full sweep's instantiation reads a.blk_begin / a.blk_end where it always did -- loaded once at
    // the top instead, hipcc allocated the feeders' scalars differently.)
    long long lst_end = 0;
    [[maybe_unused]] int wv_n = 0;                // RHALF: positions of this seed wave
    if constexpr (LIST) {
        lst_end = *a.blk_count;
        if (lst_end <= a.list_lo || lst_end > a.list_hi) return;    // (the whole grid: another launch has this count)
        long long nwg = a.split ? lst_end * ((a.n + S2_ROWS - 1) / S2_ROWS) : lst_end;
        if constexpr (RHALF) {
            // a seed wave: the positions [P0, P1) below the count, each with its row items
            const int p0 = S2W_P0(a.split), p1 = S2W_P1(a.split);
            wv_n = (int)((lst_end < p1 ? lst_end : p1) - p0);
            if (wv_n <= 0) return;
            nwg = (long long)wv_n * s2_nitems((a.n + S2_ROWS - 1) / S2_ROWS, S2W_J0(a.split), a.n, S2W_LG(a.split));
        }
        if ((long long)blockIdx.x >= nwg) return;                   // (before the first barrier, the whole workgroup)
        if constexpr (RHALF) {
            if (s2_wave_skip(a, (a.n + S2_ROWS - 1) / S2_ROWS, S2W_P0(a.split), S2W_P0(a.split) + (int)blockIdx.x % wv_n)) return;
        }
    }
#define S2_BLK_BEGIN (LIST ? 0ll : a.blk_begin)
#define S2_BLK_END (LIST ? lst_end : a.blk_end)
    apgp_exp_tab_load(Etab);
    if (t == 256) {
#pragma unroll
        for (int d = 0; d < APGP_MAX_DIM; ++d) {
            Cst[d] = a.sc[d];
            Cst[APGP_MAX_DIM + d] = a.lo[d];
            Cst[2 * APGP_MAX_DIM + d] = a.hi[d];
            Cst[3 * APGP_MAX_DIM + d] = a.lw[d];
        }
    }

    const int kc_lim = (a.n + SW_KC - 1) / SW_KC;
    const int nrb2 = (a.n + S2_ROWS - 1) / S2_ROWS;
    auto nkc_of = [&](int jb) { const int v = S2_CPB * (jb + 1); return v < kc_lim ? v : kc_lim; };
    // byte offset of tile (jb, kc) in the packed factor: half jb & 1 of packed tile (jb >> 1, kc)
    auto tile_off = [&](int jb, int kc) {
        const int ib = jb >> 1;
        const unsigned tile = (unsigned)((SW_ROWS / SW_KC) * ib * (ib + 1) / 2 + kc);
        return tile * (unsigned)(SW_TILE * 8) + (unsigned)((jb & 1) * S2_TILE * 8);
    };
    // (jb, kc, block) -> successor in the stream: next chunk, next row block, next candidate block
    // work of this workgroup: row blocks jb_lo .. jb_hi-1 of candidate blocks blk0, blk0 +
    // blk_step, ...  Persistent mode: every row block of every gridDim-th candidate block.
    // Split mode (short last round / small launches): ONE (candidate block, row block) item,
    // heaviest row blocks first; the shares go to sp_q / sp_mu and sweep_finish_kernel.
    int jb_lo = 0, jb_hi = nrb2;
    int rh = -1;                                  // RHALF: part h of row block jb_lo (pairs [pp h, pp h + pp)); -1: a whole item
    long long blk0 = S2_BLK_BEGIN + blockIdx.x, blk_step = gridDim.x;
    if (a.split) {
        const int nsplit = RHALF ? wv_n : (int)(S2_BLK_END - S2_BLK_BEGIN);
        blk0 = S2_BLK_BEGIN + (int)blockIdx.x % nsplit;
        if constexpr (RHALF) {
            blk0 += S2W_P0(a.split);
            s2_row_item((int)blockIdx.x / nsplit, nrb2, S2W_J0(a.split), a.n, S2W_LG(a.split), jb_lo, rh);
        } else jb_lo = nrb2 - 1 - (int)blockIdx.x / nsplit;
        jb_hi = jb_lo + 1;
        blk_step = S2_BLK_END;
    }
    const int rpp = RHALF ? S2_NP >> S2W_LG(a.split) : S2_NP;     // RHALF: sub-block pairs of a part item (4, 2 or 1)
    const int rsh = rh > 0 ? rh * rpp : 0;        // RHALF: first sub-block pair of this item
    // DEEP: a part item that reads the parked stream keeps its tiles in the stage ring (both roles agree on this)
    [[maybe_unused]] const bool deep = DEEP && rh >= 0 && a.ncache > 0;
    [[maybe_unused]] const int sstr = deep ? S2_STAGE(rpp) : S2_TILE;      // doubles between two stages / tile slots
    [[maybe_unused]] const int nring = deep ? (rpp == 4 ? S2_NRING(4) : rpp == 2 ? S2_NRING(2) : S2_NRING(1)) : 3;
    auto successor = [&](int& jb, int& kc, long long& blk) {
        ++kc;
        if (kc >= nkc_of(jb)) { ++jb; kc = 0; }
        if (jb >= jb_hi) { jb = jb_lo; blk += blk_step; }
    };

    if (w < 4) {
        // =============================== matrix role ===============================
        // lane whose B value this lane multiplies in rotation r (block b meets candidate
        // group b + r): the rotation is an LDS read address, not a register move
        int lr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) lr[r] = (lane & 48) | ((lane + 4 * r) & 15);
        f64x2 av[2][2][2];
        auto load_a = [&](f64x2 (&dst)[2][2], int slot, int p) {
            const f64x2* A2 = (const f64x2*)(Aring + slot * (DEEP ? sstr : S2_TILE)) + lane;     // (DEEP: slot = stage)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) dst[h][kp] = A2[((p * 2 + h) * 2 + kp) * 64];
        };
        __syncthreads();                          // C : constants staged
        __syncthreads();                          // P0: x chunks staged (feeders)
        __syncthreads();                          // P : tile 0 published
        int slot = 0, bpar = 0;
        // B operands of the current tile in all four rotations; half 0 = k-steps 0-1, 1 = 2-3
        double brot[4][NKK];
        auto load_b = [&](int buf, int half, [[maybe_unused]] int stg = 0) {
            const f64x2* Bw = (const f64x2*)(Bbuf + buf * 1024 + w * 256) + half * 64;
            // (a part item of the stage ring: the operands lie behind the image pieces of the tile's stage)
            if constexpr (DEEP) { if (deep) Bw = (const f64x2*)(Aring + stg * sstr + rpp * 512 + w * 256) + half * 64; }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f64x2 bv = Bw[lr[r]];
                brot[r][2 * half] = bv.x; brot[r][2 * half + 1] = bv.y;
            }
        };
        load_a(av[0], 0, 0);
        load_b(0, 0);
        // SOLVE: the solved blocks V are parked by the matrix wavefronts themselves (same slot
        // layout the feeders of the inverse form write: [half][wavefront][lane] x 16 B)
        const __amdgpu_buffer_rsrc_t rs_kv = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.kcache + (long long)blockIdx.x * a.ncache * SW_BCH), 0, (int)a.kslot_bytes, 0x00020000);
        for (long long blk = blk0; blk < S2_BLK_END; blk += blk_step) {
            double qtot = 0.0;
            for (int jb = jb_lo; jb < jb_hi; ++jb) {
                const int nkc = nkc_of(jb);
                const int ndiag0 = S2_CPB * jb;
                double qmic = 0.0;                // SOLVE: sum V^2 of the 16-row blocks solved on the diagonal
                double acc[2 * NP][4];
#pragma unroll
                for (int s_ = 0; s_ < 2 * NP; ++s_)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[s_][r] = 0.0;
                int kc = 0;
                auto do_tile_n = [&](auto pred_tag, auto npa_tag) {
                    constexpr bool PRED = decltype(pred_tag)::value;
                    // NPA: sub-block pairs this body works through (8 = the whole tile; 4 / 6: the straight tiles
                    // of a partial last row block, whose remaining rows are zero in the packed factor; even,
                    // so that the last pair's prefetch of the next tile lands in the free fragment buffer)
                    constexpr int NPA = decltype(npa_tag)::value;
                    const int nslot = slot == (DEEP ? nring - 1 : 2) ? 0 : slot + 1;
                    auto mfma_pair = [&](int pr, int kk) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            acc[2 * pr][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(
                                av[pr & 1][0][kk >> 1][kk & 1], brot[r][kk], acc[2 * pr][r], 0, 0, 0);
                            acc[2 * pr + 1][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(
                                av[pr & 1][1][kk >> 1][kk & 1], brot[r][kk], acc[2 * pr + 1][r], 0, 0, 0);
                        }
                    };
                    int p0 = (kc - ndiag0) >> 1;
                    if constexpr (RHALF) p0 -= rsh;     // (a half item's pairs sit in pieces 0 .. 3 and acc[0 .. 7])
                    if (p0 < 0) p0 = 0;
                    int p1 = (a.n - S2_ROWS * jb + 31) >> 5;
                    if constexpr (RHALF) {
                        p1 -= rsh;
                        if (rh >= 0 && p1 > rpp) p1 = rpp;      // (a one-pair item runs the two-pair body: its second pair is off)
                    }
                    if (p1 > NP) p1 = NP;
#pragma unroll
                    for (int pr = 0; pr < NPA; ++pr) {
                        const bool act = !PRED || (pr >= p0 && pr < p1);
                        if (act) mfma_pair(pr, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        if (pr == NPA / 2) {
                            // (SOLVE: the park stores of the last diagonal tile are acknowledged before this
                            // wavefront arrives -- their readers request them >= 14 barriers later)
                            if constexpr (SOLVE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            __syncthreads();                    // barrier i: tile i+1 is complete
                        }
                        if (pr + 1 < NPA) {
                            // (first pair: the k-step 2-3 half of this tile's B operands; its
                            // registers were still in use when the 0-1 half was prefetched)
                            if (pr == 0) load_b(bpar, 1, slot);
                            load_a(av[(pr + 1) & 1], slot, pr + 1);
                            if (act) {
                                mfma_pair(pr, 1);
                                mfma_pair(pr, 2);
                                mfma_pair(pr, 3);
                            }
#if S2_SPREAD > 0
                            if (!PRED) {
#pragma unroll
                                for (int q_ = 0; q_ < (pr == 0 ? 8 : 4); ++q_) {
                                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                                    __builtin_amdgcn_sched_group_barrier(0x008, S2_SPREAD, 0);
                                }
                            }
#endif
                        } else {
                            // last pair: the next tile's first A fragments and, as soon as this
                            // tile's k-step 0-1 B registers fall free, that half of the next
                            // tile's B operands (published by this tile's barrier): their LDS
                            // latency hides behind the 16 MFMAs of k-steps 2-3
                            load_a(av[0], nslot, 0);
                            if (act) mfma_pair(pr, 1);
                            __builtin_amdgcn_sched_barrier(0);
                            load_b(bpar ^ 1, 0, nslot);
                            if (act) {
                                mfma_pair(pr, 2);
                                mfma_pair(pr, 3);
                            }
#if S2_SPREAD > 0
                            if (!PRED) {
#pragma unroll
                                for (int q_ = 0; q_ < 4; ++q_) {
                                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                                    __builtin_amdgcn_sched_group_barrier(0x008, S2_SPREAD, 0);
                                }
                            }
#endif
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    slot = nslot;
                    bpar ^= 1;
                };
                auto do_tile = [&](auto pred_tag) { do_tile_n(pred_tag, std::integral_constant<int, NP>{}); };
                if constexpr (RHALF) {
                    // a half item: its straight tiles with the four-pair body (rows past the end are zero in the
                    // packed factor), its diagonal tiles with the predicated four-pair body; kc == nkc after them, and
                    // none of the loops below runs.  (Plain loops in sequence, as there.)
                    const int nhalf4 = (rh >= 0 && rpp == 4) ? ndiag0 : 0;
                    for (; kc < nhalf4; ++kc) do_tile_n(std::false_type{}, std::integral_constant<int, 4>{});
                    const int nhalfp = (rh >= 0 && rpp == 4) ? nkc : 0;
                    for (; kc < nhalfp; ++kc) do_tile_n(std::true_type{}, std::integral_constant<int, 4>{});
                    // a two-pair item: the same with the two-pair bodies on acc[0 .. 3]; a one-pair item: every tile
                    // with the predicated two-pair body, whose second pair p1 = 1 switches off
                    const int npair2 = (rh >= 0 && rpp == 2) ? ndiag0 : 0;
                    for (; kc < npair2; ++kc) do_tile_n(std::false_type{}, std::integral_constant<int, 2>{});
                    const int npair2p = (rh >= 0 && rpp <= 2) ? nkc : 0;
                    for (; kc < npair2p; ++kc) do_tile_n(std::true_type{}, std::integral_constant<int, 2>{});
                }
                const int nstraight = (a.n - S2_ROWS * jb >= S2_ROWS) ? ndiag0 : 0;
                for (; kc < nstraight; ++kc) do_tile(std::false_type{});
                if constexpr (!SOLVE) {
                    // partial last row block of <= 128 / <= 192 rows: its straight tiles with four / six pairs at
                    // compile time (the predicated body costs 3.4 k cycles for four pairs' 2.05 k of MFMAs,
                    // profiles/r03aa; N = 1152: 23.9 -> 22.8 ms, bit-identical).  Plain loops in sequence: as
                    // if / else alternatives that join with the 128 accumulators live, hipcc spilled them.
                    const int npart4 = (nstraight == 0 && a.n - S2_ROWS * jb <= 128) ? ndiag0 : 0;      // (kc == nkc after a half item)
                    for (; kc < npart4; ++kc) do_tile_n(std::false_type{}, std::integral_constant<int, 4>{});
                    const int npart6 = (nstraight == 0 && a.n - S2_ROWS * jb <= 192) ? ndiag0 : 0;
                    for (; kc < npart6; ++kc) do_tile_n(std::false_type{}, std::integral_constant<int, 6>{});
                    for (; kc < nkc; ++kc) do_tile(std::true_type{});
                } else {
                    for (; kc < ndiag0 && kc < nkc; ++kc) do_tile(std::true_type{});   // (partial last row block)
                    // ---- diagonal tiles of the substitution form ---------------------------------
                    // Tile (jb, 16 jb + c): the image holds -L (rows below the 16 x 16 diagonal block c) and,
                    // in sub-block slot c, that block prepared for a 4 x 4-blocked solve (pack_lsolve_kernel):
                    //   Ts[(4 q + q') 16 + 4 i + k] = -L_c[4q+i][4q'+k] (q' < q), inverse of the 4 x 4 diagonal
                    //   block (q' = q).  With acc[c] = -sum_{j<c} L_cj V_j from the tiles so far,
                    //   V_c = L_cc^-1 (K*_c + acc[c]) is solved in registers, four rows at a time, on the
                    //   four-block MFMA with the blocks used as CANDIDATE groups (A replicated, B/D lane
                    //   = cand + 16 row): the D fragment of one step is the B fragment of the next, and
                    //   V_c in that layout is, lane for lane, the tile's B operand (rotation 0) -- the other
                    //   three rotations are DPP moves, the parked copy two 16-byte stores.  No LDS round trip.
                    auto do_diag = [&]() {
                        const int nslot = slot == 2 ? 0 : slot + 1;
                        const int c = kc - ndiag0;
                        int s1 = (a.n - S2_ROWS * jb + 15) >> 4;
                        if (s1 > 2 * NP) s1 = 2 * NP;
                        load_b(bpar, 1);                        // K*_c, k-steps 2-3 (0-1: prefetched)
                        double ta[10];
                        {
                            const double* Ts = Aring + slot * S2_TILE + c * 256 + (lane & 3) * 4 + (lane >> 4);
                            int e = 0;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
#pragma unroll
                                for (int q2 = 0; q2 <= q; ++q2) ta[e++] = Ts[(q * 4 + q2) * 16];
                        }
                        const bool park_now = a.ncache > 0 && jb + 1 < nrb2;
                        auto half = [&](int pr, int h, int kk) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                acc[2 * pr + h][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(
                                    av[pr & 1][h][kk >> 1][kk & 1], brot[r][kk], acc[2 * pr + h][r], 0, 0, 0);
                        };
                        auto micro = [&](int S) {     // (S is a constant after the pair loop is unrolled)
                            // rows 4 q + i of sub-block S sit in lane block q of the four rotation registers
                            // (candidate group (q + r) & 3): ror 4 r brings group b' to lane block b'
                            double rot[4];
                            rot[0] = acc[S][0];
                            rot[1] = apgp_row_ror4<1>(acc[S][1]);
                            rot[2] = apgp_row_ror4<2>(acc[S][2]);
                            rot[3] = apgp_row_ror4<3>(acc[S][3]);
                            const int bb = (lane >> 2) & 3;
                            double R[4], V[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int rr = (bb - q) & 3;
                                R[q] = (rr == 0 ? rot[0] : rr == 1 ? rot[1] : rr == 2 ? rot[2] : rot[3]) + brot[0][q];
                            }
                            V[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[0], R[0], 0.0, 0, 0, 0);
                            R[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[1], V[0], R[1], 0, 0, 0);
                            R[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[3], V[0], R[2], 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[6], V[0], R[3], 0, 0, 0);
                            V[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[2], R[1], 0.0, 0, 0, 0);
                            R[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[4], V[1], R[2], 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[7], V[1], R[3], 0, 0, 0);
                            V[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[5], R[2], 0.0, 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[8], V[2], R[3], 0, 0, 0);
                            V[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[9], R[3], 0.0, 0, 0, 0);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                brot[0][q] = V[q];
                                brot[1][q] = apgp_row_ror4<3>(V[q]);     // lane l <- lane l + 4
                                brot[2][q] = apgp_row_ror4<2>(V[q]);
                                brot[3][q] = apgp_row_ror4<1>(V[q]);
                                qmic = fma(V[q], V[q], qmic);
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) acc[S][r] = 0.0;    // (counted through qmic)
                            if (park_now) {
                                const unsigned soff = (unsigned)kc * (unsigned)(SW_BCH * 8);
                                const unsigned voff = (unsigned)(w * 64 + lane) * 16u;
                                f64x2 q0, q1;
                                q0.x = V[0]; q0.y = V[1]; q1.x = V[2]; q1.y = V[3];
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q0), rs_kv, voff, soff, 0);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q1), rs_kv, voff, soff + 4096u, 0);
                            }
                        };
#pragma unroll
                        for (int pr = 0; pr < NP; ++pr) {
                            if (2 * pr == c) micro(2 * pr);
                            if (2 * pr + 1 == c) micro(2 * pr + 1);
                            const bool a0 = 2 * pr > c && 2 * pr < s1, a1 = 2 * pr + 1 > c && 2 * pr + 1 < s1;
                            if (a0) half(pr, 0, 0);
                            if (a1) half(pr, 1, 0);
                            __builtin_amdgcn_sched_barrier(0);
                            if (pr == 4) {
                                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                                __syncthreads();                // barrier i: tile i+1 is complete
                            }
                            if (pr + 1 < NP) {
                                load_a(av[(pr + 1) & 1], slot, pr + 1);
                                if (a0) { half(pr, 0, 1); half(pr, 0, 2); half(pr, 0, 3); }
                                if (a1) { half(pr, 1, 1); half(pr, 1, 2); half(pr, 1, 3); }
                            } else {
                                load_a(av[0], nslot, 0);
                                if (a0) half(pr, 0, 1);
                                if (a1) half(pr, 1, 1);
                                __builtin_amdgcn_sched_barrier(0);
                                load_b(bpar ^ 1, 0);
                                if (a0) { half(pr, 0, 2); half(pr, 0, 3); }
                                if (a1) { half(pr, 1, 2); half(pr, 1, 3); }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        slot = nslot;
                        bpar ^= 1;
                    };
                    // The same tile with the chunk index C a compile-time constant, for a complete row block (its
                    // sixteen diagonal tiles always come in order): only the sub-blocks below the diagonal block
                    // are touched -- no predicated pairs, no A-fragment reads or joins for the inactive ones, acc[C]
                    // indexed statically --, the first active pair's fragments land during the in-register solve.
                    // Generic form above: ~123 k cycles per row block (the inverse form's diagonal phase: 66 k) --
                    // the substitution form's whole deficit; static form: ~75 k at N = 512.  But the sixteen bodies
                    // are 65 KiB of straight-line code executed once per row block: once the workgroups have
                    // drifted apart and stop sharing instruction-cache lines the phase is fetch-bound (N = 4096:
                    // 310 ms against 276 ms for the generic form; N = 2048: 74 vs 77 ms; N = 1152: 27 vs 31 ms;
                    // N = 512: 5.9 vs 8.5 ms), so it is used up to S2_STATIC_DIAG_NRB row blocks.  (A version
                    // templated on the pair index only, parity as a uniform branch -- a third of the code --
                    // made hipcc spill the accumulators at the join: 2,900 scratch accesses.)
                    auto diag_c = [&](auto c_) {
                        constexpr int C = decltype(c_)::value;
                        constexpr int PF = (C + 1) >> 1;            // first pair with a sub-block below block C
                        const int nslot = slot == 2 ? 0 : slot + 1;
                        load_b(bpar, 1);                            // K*_C, k-steps 2-3 (0-1: prefetched)
                        double ta[10];
                        {
                            const double* Ts = Aring + slot * S2_TILE + C * 256 + (lane & 3) * 4 + (lane >> 4);
                            int e = 0;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
#pragma unroll
                                for (int q2 = 0; q2 <= q; ++q2) ta[e++] = Ts[(q * 4 + q2) * 16];
                        }
                        if constexpr (C < 15) load_a(av[PF & 1], slot, PF);
                        {
                            double rot[4];
                            rot[0] = acc[C][0];
                            rot[1] = apgp_row_ror4<1>(acc[C][1]);
                            rot[2] = apgp_row_ror4<2>(acc[C][2]);
                            rot[3] = apgp_row_ror4<3>(acc[C][3]);
                            const int bb = (lane >> 2) & 3;
                            double R[4], V[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int rr = (bb - q) & 3;
                                R[q] = (rr == 0 ? rot[0] : rr == 1 ? rot[1] : rr == 2 ? rot[2] : rot[3]) + brot[0][q];
                            }
                            V[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[0], R[0], 0.0, 0, 0, 0);
                            R[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[1], V[0], R[1], 0, 0, 0);
                            R[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[3], V[0], R[2], 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[6], V[0], R[3], 0, 0, 0);
                            V[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[2], R[1], 0.0, 0, 0, 0);
                            R[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[4], V[1], R[2], 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[7], V[1], R[3], 0, 0, 0);
                            V[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[5], R[2], 0.0, 0, 0, 0);
                            R[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[8], V[2], R[3], 0, 0, 0);
                            V[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ta[9], R[3], 0.0, 0, 0, 0);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                brot[0][q] = V[q];
                                brot[1][q] = apgp_row_ror4<3>(V[q]);
                                brot[2][q] = apgp_row_ror4<2>(V[q]);
                                brot[3][q] = apgp_row_ror4<1>(V[q]);
                                qmic = fma(V[q], V[q], qmic);
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) acc[C][r] = 0.0;
                            if (jb + 1 < nrb2) {
                                const unsigned soff = (unsigned)kc * (unsigned)(SW_BCH * 8);
                                const unsigned voff = (unsigned)(w * 64 + lane) * 16u;
                                f64x2 q0, q1;
                                q0.x = V[0]; q0.y = V[1]; q1.x = V[2]; q1.y = V[3];
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q0), rs_kv, voff, soff, 0);
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q1), rs_kv, voff, soff + 4096u, 0);
                            }
                        }
                        auto half = [&](int pr, int h, int kk) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                acc[2 * pr + h][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(
                                    av[pr & 1][h][kk >> 1][kk & 1], brot[r][kk], acc[2 * pr + h][r], 0, 0, 0);
                        };
                        // (the two park stores of THIS tile may stay in flight at its barrier -- VMEM completes in
                        // issue order, "at most two outstanding" = the previous tile's are acknowledged; their
                        // readers request them >= 14 barriers later)
                        constexpr int PBAR = PF > 4 ? PF : 4;       // pair after whose first k-step the tile's barrier stands
                        if constexpr (C == 15) {
                            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                            __syncthreads();                        // barrier i: tile i+1 is complete
                            load_a(av[0], nslot, 0);
                            load_b(bpar ^ 1, 0);
                        }
                        static_for<NP>([&](auto pr_) {
                            constexpr int pr = decltype(pr_)::value;
                            if constexpr (pr >= PF && C < 15) {
                                constexpr bool a0 = 2 * pr > C;
                                if constexpr (a0) half(pr, 0, 0);
                                half(pr, 1, 0);
                                __builtin_amdgcn_sched_barrier(0);
                                if constexpr (pr == PBAR) {
                                    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                                    __syncthreads();                // barrier i: tile i+1 is complete
                                }
                                if constexpr (pr + 1 < NP) {
                                    load_a(av[(pr + 1) & 1], slot, pr + 1);
                                    if constexpr (a0) { half(pr, 0, 1); half(pr, 0, 2); half(pr, 0, 3); }
                                    half(pr, 1, 1); half(pr, 1, 2); half(pr, 1, 3);
                                } else {
                                    load_a(av[0], nslot, 0);
                                    if constexpr (a0) half(pr, 0, 1);
                                    half(pr, 1, 1);
                                    __builtin_amdgcn_sched_barrier(0);
                                    load_b(bpar ^ 1, 0);
                                    if constexpr (a0) { half(pr, 0, 2); half(pr, 0, 3); }
                                    half(pr, 1, 2); half(pr, 1, 3);
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        });
                        slot = nslot;
                        bpar ^= 1;
                        ++kc;
                    };
                    if constexpr (STATIC_DIAG) {
                        if (a.n - S2_ROWS * jb >= S2_ROWS) static_for<S2_CPB>(diag_c);
                    }
                    for (; kc < nkc; ++kc) do_diag();
                }
                // this row block's share of sum V^2: rotation r's accumulators belong to the
                // candidate of lane lr[r]; gather them back, reduce over the 4 row-lanes
                double qr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    qr[r] = 0.0;
#pragma unroll
                    for (int s_ = 0; s_ < 2 * NP; ++s_) qr[r] = fma(acc[s_][r], acc[s_][r], qr[r]);
                }
                if constexpr (RHALF) {
                    if (rh >= 0) {
                        // the fold's inputs instead of a share (acc[2 pp ..] are zero: qr is the chain over s = 0 .. 2 pp - 1);
                        // [16-byte piece][matrix thread]: a wavefront's store is 1 KiB in one piece
                        double* item = s2_fold_item(a.sp_q, nrb2, a.blk_end, blk0, jb);
                        if (rh == 0) {
                            f64x2* P = (f64x2*)item + t;
                            f64x2 v0, v1;
                            v0.x = qr[0]; v0.y = qr[1]; v1.x = qr[2]; v1.y = qr[3];
                            P[0] = v0; P[256] = v1;
                        } else {
                            // (sub-block s of the whole item at piece pair s - 2: S2_HQ_ACC)
                            f64x2* A = (f64x2*)(item + S2_HQ_PRE) + (2 * (2 * rsh - 2)) * 256 + t;
#pragma unroll
                            for (int s_ = 0; s_ < NP; ++s_) {
                                if (s_ < 2 * rpp) {
                                    f64x2 v0, v1;
                                    v0.x = acc[s_][0]; v0.y = acc[s_][1]; v1.x = acc[s_][2]; v1.y = acc[s_][3];
                                    A[(2 * s_) * 256] = v0; A[(2 * s_ + 1) * 256] = v1;
                                }
                            }
                        }
                    }
                }
                double qs = qr[0];
#pragma unroll
                for (int r = 1; r < 4; ++r) qs += __shfl(qr[r], (lane & 48) | ((lane - 4 * r) & 15));
                if constexpr (SOLVE) qs += qmic;  // (lane = candidate + 16 row there as well)
                qs += __shfl_xor(qs, 16);
                qs += __shfl_xor(qs, 32);
                qtot += qs;
            }
            if (kq == 0) Shq[w * 16 + cl] = qtot;
            __syncthreads();                      // E1: sums visible to the feeders
            __syncthreads();                      // E2: block result written
        }
        return;
    }

    // ================================= feeder role =================================
    const int hw = w - 4, ht = t - 256;
    const unsigned hoff = (unsigned)ht * 16u;
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.linv, 0, (int)a.linv_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)a.xs, 0, (int)a.xs_bytes, 0x00020000);
    // (SPARK, the seed launch: the slot seed_park_kernel filled for this item's block, its position in the list; every
    // item of the block reads it and none writes it)
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.kcache + (SPARK ? blk0 : (long long)blockIdx.x) * a.ncache * SW_BCH), 0, (int)a.kslot_bytes, 0x00020000);
    // an x chunk is XCHUNK16 16-byte pieces, one per feeder thread -- two for the first threads when Dpad = 32 (272 pieces,
    // 256 threads): XQ carries the second piece, dead code for the other instantiations
    constexpr bool X2 = XCHUNK16 > 256;
    struct XQ { f64x2 a, b; };
    const unsigned xoff = ht < XCHUNK16 ? hoff : 0u;
    const unsigned xoff2 = (X2 && ht + 256 < XCHUNK16) ? hoff + 256u * 16u : 0u;
    auto x_fetch = [&](int kc) {
        XQ q;
        q.a = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff, (unsigned)kc * (unsigned)(SW_KC * XS * 8), 0));
        if constexpr (X2) q.b = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff2, (unsigned)kc * (unsigned)(SW_KC * XS * 8), 0));
        return q;
    };
    auto x_put = [&](int xb, const XQ& v) {
        if (ht < XCHUNK16) {
            if (xb == 0) *((f64x2*)Xbuf + ht) = v.a;
            else *((f64x2*)(Xbuf + XSTRIDE) + ht) = v.a;
        }
        if constexpr (X2) {
            if (ht + 256 < XCHUNK16) {
                if (xb == 0) *((f64x2*)Xbuf + ht + 256) = v.b;
                else *((f64x2*)(Xbuf + XSTRIDE) + ht + 256) = v.b;
            }
        }
    };
    const bool park = a.ncache > 0;
    // per-candidate state of the block being fed (cur) and of the finished one (fin)
    double tt[DPAD];
    double ktt_cur = a.amp, ktt_fin = a.amp, mu_cur = 0.0, mu_tot = 0.0, mu_fin = 0.0;
    int fl_cur = 0, fl_fin = 0;
    long long blk_cur = -1, blk_fin = -1;
    auto load_candidates = [&](long long blk) {
        // snapshot the finished block, then set up the new one
        mu_fin = mu_tot; ktt_fin = ktt_cur; fl_fin = fl_cur; blk_fin = blk_cur;
        if constexpr (LIST) {                     // position in the list -> the block's number in the candidate matrix
            const bool live = blk < S2_BLK_END;
            blk = live ? a.blk_list[blk] : a.blk_end;
        }
        blk_cur = blk; mu_cur = 0.0; mu_tot = 0.0;
        const long long crow = blk * SW_CAND + hw * 16 + cl;
        const bool inb = blk < a.blk_end && crow < a.m;
        bool adm = inb, has_nan = false;
        double ktl = (LIN && a.lin_order == 0) ? (double)a.ndim : 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            double v = 0.0;
            if (inb && d < a.ndim) {
                v = a.T[crow * a.ndim + d];
                if (a.has_box && !(v >= Cst[APGP_MAX_DIM + d] && v <= Cst[2 * APGP_MAX_DIM + d])) adm = false;
                if (v != v) has_nan = true;
            }
            tt[d] = v * Cst[d];
            if (LIN && a.lin_order > 0) {
                const double p = v * v;
                double q = p;
                for (int e = 1; e < a.lin_order; ++e) q *= p;
                ktl += q;
            }
        }
        if (inb && a.mask && a.mask[crow] == 0) adm = false;
        // a row with a NaN coordinate is inadmissible with or without a box: Jones would give it 0.0 (sqrt(var) > 0 is false),
        // which ties with an underflowed tail and, at the lowest index, would win
        fl_cur = ((adm && !has_nan) ? 1 : 0) | (has_nan ? 2 : 0) | (inb ? 4 : 0);
        ktt_cur = LIN ? fma(a.lin_coef, ktl, a.amp) : a.amp;
    };
    // generate the B operands of tile (jb, kc) of the current block -> LDS buffer bb (and, on
    // the chunk's first visit, the parked stream and this row block's share of mu)
    auto produce_b = [&](int jb, int kc, int bb, int xb, [[maybe_unused]] int stg = -1) {
        double bfv[NKK];
        {
            const double* Xb = Xbuf + xb * XSTRIDE;
            double s2[NKK], s3[NKK], al[NKK], lsum[NKK];
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                s2[kk] = 0.0; s3[kk] = 0.0;
                lsum[kk] = (LIN && a.lin_order == 0) ? (double)a.ndim : 0.0;
                al[kk] = Xb[(kk * 4 + kq) * XS + DPAD];
            }
#pragma unroll
            for (int d = 0; d < DPAD; d += 2)
#pragma unroll
                for (int kk = 0; kk < NKK; ++kk) {
                    const f64x2 xa = *(const f64x2*)(Xb + (kk * 4 + kq) * XS + d);
                    const double df0 = tt[d] - xa.x, df1 = tt[d + 1] - xa.y;
                    s2[kk] = fma(df0, df0, s2[kk]);
                    s3[kk] = fma(df1, df1, s3[kk]);
                    if (LIN && a.lin_order > 0) {
                        const double p0_ = tt[d] * xa.x * Cst[3 * APGP_MAX_DIM + d], p1_ = tt[d + 1] * xa.y * Cst[3 * APGP_MAX_DIM + d + 1];
                        double q0 = p0_, q1 = p1_;
                        for (int e = 1; e < a.lin_order; ++e) { q0 *= p0_; q1 *= p1_; }
                        lsum[kk] += q0 + q1;
                    }
                }
            double ex[NKK];
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) ex[kk] = -(s2[kk] + s3[kk]);
            apgp_exp4(ex, bfv, Etab);
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) bfv[kk] = LIN ? fma(a.lin_coef, lsum[kk], bfv[kk] * a.amp) : bfv[kk] * a.amp;
            if (kc >= S2_CPB * jb) {
#pragma unroll
                for (int kk = 0; kk < NKK; ++kk) mu_cur = fma(bfv[kk], al[kk], mu_cur);
                if (kc == nkc_of(jb) - 1) {
                    // row block complete: its share of mu, reduced over the 4 k-lanes, joins the
                    // total in row-block order (the order sweep_finish_kernel adds split shares)
                    double m = mu_cur;
                    m += __shfl_xor(m, 16);
                    m += __shfl_xor(m, 32);
                    mu_tot += m;
                    mu_cur = 0.0;
                }
                if (!SOLVE && !SPARK && park && jb + 1 < nrb2) {      // (SPARK: the slot is read-only, see rs_k)
                    const unsigned soff = (unsigned)kc * (unsigned)(SW_BCH * 8);
                    f64x2 q0, q1;
                    q0.x = bfv[0]; q0.y = bfv[1]; q1.x = bfv[2]; q1.y = bfv[3];
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q0), rs_k, hoff, soff, SW_KAUX);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q1), rs_k, hoff, soff + 256 * 16, SW_KAUX);
                }
            }
            f64x2 o0, o1;
            o0.x = bfv[0]; o0.y = bfv[1]; o1.x = bfv[2]; o1.y = bfv[3];
            if constexpr (DEEP) {                 // (stg >= 0: into stage stg of a part item's ring)
                if (stg >= 0) { f64x2* Bw = (f64x2*)(Aring + stg * sstr + rpp * 512 + hw * 256); Bw[lane] = o0; Bw[64 + lane] = o1; return; }
            }
            if (bb == 0) { f64x2* Bw = (f64x2*)(Bbuf + hw * 256); Bw[lane] = o0; Bw[64 + lane] = o1; }
            else { f64x2* Bw = (f64x2*)(Bbuf + 1024 + hw * 256); Bw[lane] = o0; Bw[64 + lane] = o1; }
        }
    };
    auto epilogue = [&]() {
        __syncthreads();                          // E1
        if (a.split) {
            if (kq == 0) {
                // (LIST: the shares are indexed by the block's position in the list -- a split workgroup has one block)
                const long long e = ((LIST ? blk0 : blk_fin - a.blk_begin) * SW_CAND + hw * 16 + cl) * nrb2 + jb_lo;
                // (RHALF: a half item's share of sum V^2 comes from sweep_fold_kernel; both halves hold the same share of
                // mu, the upper one stores it)
                if (!RHALF || rh < 0) a.sp_q[e] = Shq[hw * 16 + cl];
                if (!RHALF || rh <= 0) a.sp_mu[e] = mu_fin;
            }
            __syncthreads();                      // E2
            return;
        }
        double bu = INFINITY;
        long long bi = -1;
        const long long crow = blk_fin * SW_CAND + hw * 16 + cl;
        if (kq == 0 && (fl_fin & 4)) {
            double mu = mu_fin + a.mean;
            double var = ktt_fin - Shq[hw * 16 + cl];
            if (fl_fin & 2) { mu = NAN; var = NAN; }
            if (a.mu) a.mu[crow] = mu;
            if (a.var) a.var[crow] = var;
            if (a.kind != APGP_UTIL_NONE) {
                const double uu = (fl_fin & 1) ? util_value(a.kind, mu, var, a.zeta, a.ybest) : INFINITY;
                if (a.u) a.u[crow] = uu;
                best_merge(bu, bi, uu, a.idx_offset + crow);
            }
        }
        for (int o = 8; o > 0; o >>= 1) {
            double ou = __shfl_xor(bu, o);
            long long oi = __shfl_xor(bi, o);
            best_merge(bu, bi, ou, oi);
        }
        if (lane == 0) { red_u[hw] = bu; red_i[hw] = bi; }
        __syncthreads();                          // E2
        if (ht == 0 && a.kind != APGP_UTIL_NONE) {
            for (int i = 1; i < 4; ++i) best_merge(bu, bi, red_u[i], red_i[i]);
            a.part_u[blk_fin] = bu;
            a.part_i[blk_fin] = bi;
        }
    };

    // ---- the feeder loop -------------------------------------------------------------------
    // Next to a saturated MFMA stream every feeder instruction waits for an issue slot (~10
    // cycles for a scalar one, ~100 for one that reads or writes VGPRs; tools/mfma_pair.hip),
    // so the per-tile work is a handful of LDS-DMA requests (buffer_load ... lds: no data
    // VGPRs, no ds_write) and scalar bookkeeping.  Tile i+1's image and parked operands are
    // requested right after barrier i-1 into slot (i+1) % 3 / buffer (i+1) & 1 -- both free
    // since barrier i-1 -- and the vmcnt(0) hipcc places in front of barrier i publishes them.
    // Two forms of the feeder loop, chosen per instantiation by same-box A/B (profiles/r03g): next to a
    // saturated MFMA stream the feeder's cost is a matter of how hipcc allocates this loop's scalars (a
    // spilled one read back with v_readlane costs 30-100 cycles), and that differs between the DPAD
    // instantiations.  Structured: +8-13 % at N = 1024-2048 for DPAD 2 / 4 / 16 (inverse form) and for
    // DPAD 2 (substitution form); the single loop is 1.5-2.5 % faster for DPAD 8 (C3, C5).
    // DEEP, a part item of the stage ring: one item is one run of tiles of one row block -- tile 0 (generated, the
    // prologue's), the re-read tiles [1, nd0) and the generating tiles [nd0, nt) --, so its loop needs none of the stream
    // bookkeeping below, and one form serves every Dpad.  After barrier i-1 the feeders request the re-read tiles up to
    // i + dist into their stages (free since the matrix wavefronts passed barrier i-1: tile i-2 and older are read out)
    // and wait, in front of barrier i, until at most the requests of the tiles newer than i+1 are outstanding: every
    // feeder wavefront issues rpp + 2 requests per tile, VMEM completes in issue order, so tile i+1 has landed.  No
    // __syncthreads() in this loop (hipcc would drain the queue in front of it).  The generating tiles follow at distance
    // one as in the forms below; by then the run's last request has been waited for.
    if constexpr (DEEP) {
        if (deep) {
            const int hw_s = __builtin_amdgcn_readfirstlane(hw);
            typedef __attribute__((address_space(3))) void lds_void;
            const int jb = jb_lo, nt = nkc_of(jb);
            const int nd0 = S2_CPB * jb < nt ? S2_CPB * jb : nt;
            int dist = S2W_PF(a.split);
            dist = dist < 1 ? 1 : (dist > nring - 2 ? nring - 2 : dist);
            const int nreq = rpp + 2;
            auto dma_stage = [&](int stg, int kc) {
                double* dst = Aring + stg * sstr + hw_s * 128;
                const unsigned toffs = tile_off(jb, kc);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < rpp)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(dst + q * 512), 16, (unsigned)lane * 16u,
                                                                 toffs + (unsigned)((q + rsh) * 4096) + (unsigned)hw_s * 1024u, 0, 0);
            };
            auto dma_stage_b = [&](int stg, int c) {
                double* dst = Aring + stg * sstr + rpp * 512 + hw_s * 256;
                const unsigned soff = (unsigned)c * (unsigned)(SW_BCH * 8) + (unsigned)hw_s * 1024u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)dst, 16, (unsigned)lane * 16u, soff, 0, SW_KAUX);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)(dst + 128), 16, (unsigned)lane * 16u, soff + 4096u, 0, SW_KAUX);
            };
            // generating tiles: 0, then g1, g1 + 1, ...; the g-th of them reads x buffer g & 1
            const int g1 = nd0 > 1 ? nd0 : 1;
            __syncthreads();                          // C : constants visible
            load_candidates(blk0);
            dma_stage(0, 0);
            x_put(0, x_fetch(0));
            x_put(1, x_fetch(g1 < nt ? g1 : 0));
            __syncthreads();                          // P0
            produce_b(jb, 0, 0, 0, 0);
            XQ xq = x_fetch(g1 + 1 < nt ? g1 + 1 : 0);
            __syncthreads();                          // P
            int nx = 1, stx = 1;                      // next re-read tile to request, its stage
            int st1 = 1, g = 1;                       // stage of tile i+1; generating tiles so far
            for (int i = 0; i < nt; ++i) {
                // the matrix wavefronts have just passed barrier i-1
                const int t1 = i + 1;
                int n_pend = 0;
                if (t1 >= nd0) {
                    if (t1 < nt) {
                        __builtin_amdgcn_s_setprio(3);
                        dma_stage(st1, t1);
                        produce_b(jb, t1, 0, g & 1, st1);
                        x_put((g & 1) ^ 1, xq);       // x chunk of the generating tile after this one
                        if (t1 + 2 < nt) { xq = x_fetch(t1 + 2); n_pend = X2 ? 2 : 1; }
                        ++g;
                        __builtin_amdgcn_s_setprio(0);
                    }
                } else {
                    while (nx < nd0 && nx <= i + dist) {
                        dma_stage(stx, nx);
                        dma_stage_b(stx, nx);
                        ++nx;
                        stx = stx + 1 == nring ? 0 : stx + 1;
                    }
                    n_pend = (nx - 1 - t1) * nreq;    // requests of the tiles newer than i+1
                }
                st1 = st1 + 1 == nring ? 0 : st1 + 1;
                // barrier i (the counts: the comment at S2_NRING; one not listed: vmcnt(0), which waits for more than it must)
#define S2_DEEP_BARRIER(n) asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)\n\ts_barrier" ::: "memory")
                switch (n_pend) {
                    case 1: S2_DEEP_BARRIER(1); break;
                    case 2: S2_DEEP_BARRIER(2); break;
                    case 3: S2_DEEP_BARRIER(3); break;
                    case 4: S2_DEEP_BARRIER(4); break;
                    case 6: S2_DEEP_BARRIER(6); break;
                    case 8: S2_DEEP_BARRIER(8); break;
                    case 9: S2_DEEP_BARRIER(9); break;
                    case 12: S2_DEEP_BARRIER(12); break;
                    case 15: S2_DEEP_BARRIER(15); break;
                    default: S2_DEEP_BARRIER(0); break;
                }
#undef S2_DEEP_BARRIER
            }
            load_candidates(S2_BLK_END);              // (no next block: only snapshots the finished one)
            epilogue();
            return;
        }
    }
    if constexpr (SF) {
        const int hw_s = __builtin_amdgcn_readfirstlane(hw);
        typedef __attribute__((address_space(3))) void lds_void;
        // image of tile (jb, kc): 8 pieces of 4 KiB = the 8 sub-block pairs (32 rows each), a quarter
        // of each piece per feeder wavefront.  (Requesting only the non-zero pairs q >= (kc - 16 jb) / 2
        // of a lower-triangular diagonal tile -- 288 instead of 512 KiB per row block -- changes
        // nothing, 248.9 vs 247.4 ms: the diagonal tiles do not wait for the image stream.)
        auto dma_tile = [&](int slot, int jb, int kc) {
            double* dst = Aring + slot * S2_TILE + hw_s * 128;
            const unsigned toffs = tile_off(jb, kc);
            if constexpr (RHALF) {
                // a part item: pieces pp h .. pp h + pp - 1 of the image into pieces 0 .. pp - 1 of the slot
                if (rh >= 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < rpp)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(dst + q * 512), 16, (unsigned)lane * 16u,
                                                                     toffs + (unsigned)((q + rsh) * 4096) + (unsigned)hw_s * 1024u, 0, 0);
                    return;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(dst + q * 512), 16, (unsigned)lane * 16u,
                                                         toffs + (unsigned)(q * 4096) + (unsigned)hw_s * 1024u, 0, 0);
        };
        auto dma_parked = [&](int par, int c) {
            double* dst = Bbuf + par * 1024 + hw_s * 256;
            const unsigned soff = (unsigned)c * (unsigned)(SW_BCH * 8) + (unsigned)hw_s * 1024u;
            // (SOLVE: the parked blocks were stored by the matrix wavefronts of this workgroup: sc1 = served by
            // the L2, never by a line this CU's vector cache kept from the previous candidate block)
            constexpr int kaux = SOLVE ? 16 : SW_KAUX;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)dst, 16, (unsigned)lane * 16u, soff, 0, kaux);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)(dst + 128), 16, (unsigned)lane * 16u, soff + 4096u, 0, kaux);
        };
        // x chunk kc of the packed training stream straight into x buffer xb by LDS-DMA (whole wavefronts
        // only: the chunk is rounded up to 1 KiB pieces, the extra lanes fetch the bytes that follow it in
        // the stream -- zeros past its end -- into the buffer's padding)
        auto x_dma = [&](int xb, int kc) {
            if (hw_s * 128 < XSTRIDE)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void*)(Xbuf + xb * XSTRIDE + hw_s * 128), 16,
                                                         (unsigned)ht * 16u, (unsigned)kc * (unsigned)(SW_KC * XS * 8), 0, 0);
        };
        auto nd0_of = [&](int jb) { const int v = S2_CPB * jb, n = nkc_of(jb); return park ? (v < n ? v : n) : 0; };
        auto next_gen = [&](int& jb, int& kc) {
            if (kc + 1 < nkc_of(jb)) {
                ++kc;
                // (SPARK with the parked stream: the prologue generates chunk 0 of any row block, and the next
                // generating tile is the row block's first diagonal one)
                if constexpr (SPARK) { if (kc < nd0_of(jb)) kc = nd0_of(jb); }
                return;
            }
            jb = jb + 1 < jb_hi ? jb + 1 : jb_lo;
            kc = nd0_of(jb);
        };
        const bool xw = hw_s * 128 < XSTRIDE;
#define S2_BARRIER(n) asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)\n\ts_barrier" ::: "memory")
        __syncthreads();                              // C : constants visible
        load_candidates(blk0);
        dma_tile(0, jb_lo, 0);
        {
            int gj = jb_lo, gk = 0;
            x_dma(0, gk);
            next_gen(gj, gk);
            x_dma(1, gk);
            next_gen(gj, gk);
            x_dma(2, gk);
            __syncthreads();                          // P0 (vmcnt(0): image 0 and the x chunks have landed)
            produce_b(jb_lo, 0, 0, 0);
        }
        __syncthreads();                              // P
        int slot = 1, par = 1, gpar = 1;
        bool first_tile = true;
        for (long long blk = blk0; blk < S2_BLK_END; blk += blk_step) {
            for (int jb = jb_lo; jb < jb_hi; ++jb) {
                const int nkc = nkc_of(jb), nd0 = nd0_of(jb);
                // ---- run of parked tiles: image + parked operands by LDS-DMA, nothing else ----
                for (int kc = 0; kc < nd0; ++kc) {
                    if constexpr (SPARK) {            // (an item of a row block > 0: T_0, the prologue's, is of this run)
                        if (first_tile) { first_tile = false; continue; }
                    }
                    dma_tile(slot, jb, kc);
                    dma_parked(par, kc);
                    slot = slot == 2 ? 0 : slot + 1;
                    par ^= 1;
                    S2_BARRIER(0);
                }
                // ---- run of generating tiles ----
                for (int kc = nd0; kc < nkc; ++kc) {
                    if (first_tile) { first_tile = false; continue; }      // T_0: the prologue's
                    const bool newblk = (jb == jb_lo && kc == 0);
                    __builtin_amdgcn_s_setprio(3);
                    dma_tile(slot, jb, kc);
                    if (newblk) load_candidates(blk);
                    int xk = kc;                      // chunk of the generating tile after next
                    {
                        int gj = jb;
                        next_gen(gj, xk);
                        next_gen(gj, xk);
                    }
                    const bool stores = !SOLVE && !SPARK && park && kc >= S2_CPB * jb && jb + 1 < nrb2;
                    produce_b(jb, kc, par, gpar);
                    x_dma(gpar == 0 ? 2 : gpar - 1, xk);
                    slot = slot == 2 ? 0 : slot + 1;
                    par ^= 1;
                    gpar = gpar == 2 ? 0 : gpar + 1;
                    __builtin_amdgcn_s_setprio(0);
                    if (stores) { if (xw) S2_BARRIER(3); else S2_BARRIER(2); }
                    else { if (xw) S2_BARRIER(1); else S2_BARRIER(0); }
                    // the matrix wavefronts have passed the barrier of the previous block's last tile
                    if (newblk) epilogue();
                }
            }
        }
        load_candidates(S2_BLK_END);                  // (no next block: only snapshots the finished one)
        S2_BARRIER(0);                                // barrier of the last tile
        epilogue();
#undef S2_BARRIER
    } else {
        struct Pos { int jb, kc; long long bl; };
        Pos p0 = {jb_lo, 0, blk0}, p1, p2, p3;
        auto next_of = [&](const Pos& p) { Pos q = p; successor(q.jb, q.kc, q.bl); return q; };
        p1 = next_of(p0); p2 = next_of(p1); p3 = next_of(p2);
        const int hw_s = __builtin_amdgcn_readfirstlane(hw);
        typedef __attribute__((address_space(3))) void lds_void;
        // image of tile (jb, kc): 8 pieces of 4 KiB = the 8 sub-block pairs (32 rows each), a quarter
        // of each piece per feeder wavefront.  (Requesting only the non-zero pairs q >= (kc - 16 jb) / 2
        // of a lower-triangular diagonal tile -- 288 instead of 512 KiB per row block -- changes
        // nothing, 248.9 vs 247.4 ms: the diagonal tiles do not wait for the image stream.)
        auto dma_tile = [&](int slot, int jb, int kc) {
            double* dst = Aring + slot * S2_TILE + hw_s * 128;
            const unsigned toffs = tile_off(jb, kc);
            if constexpr (RHALF) {
                // a part item: pieces pp h .. pp h + pp - 1 of the image into pieces 0 .. pp - 1 of the slot
                if (rh >= 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < rpp)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(dst + q * 512), 16, (unsigned)lane * 16u,
                                                                     toffs + (unsigned)((q + rsh) * 4096) + (unsigned)hw_s * 1024u, 0, 0);
                    return;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(dst + q * 512), 16, (unsigned)lane * 16u,
                                                         toffs + (unsigned)(q * 4096) + (unsigned)hw_s * 1024u, 0, 0);
        };
        auto dma_parked = [&](int par, int c) {
            double* dst = Bbuf + par * 1024 + hw_s * 256;
            const unsigned soff = (unsigned)c * (unsigned)(SW_BCH * 8) + (unsigned)hw_s * 1024u;
            // (SOLVE: the parked blocks were stored by the matrix wavefronts of this workgroup: sc1 = served by
            // the L2, never by a line this CU's vector cache kept from the previous candidate block)
            constexpr int kaux = SOLVE ? 16 : SW_KAUX;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)dst, 16, (unsigned)lane * 16u, soff, 0, kaux);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_void*)(dst + 128), 16, (unsigned)lane * 16u, soff + 4096u, 0, kaux);
        };
        auto is_gen = [&](const Pos& p) { return !park || p.kc >= S2_CPB * p.jb; };
        // ---- prologue: tile 0 and its operands, x chunks of tiles 0 and 1, requests for tile 1 ----
        __syncthreads();                              // C : constants visible
        load_candidates(p0.bl);
        dma_tile(0, p0.jb, p0.kc);
        x_put(0, x_fetch(p0.kc));
        x_put(1, x_fetch(p1.kc));
        __syncthreads();                              // P0
        produce_b(p0.jb, p0.kc, 0, 0);
        XQ xq = x_fetch(p2.kc);
        __syncthreads();                              // P
        // total tiles of this workgroup
        long long ntile_blk = 0;
        for (int jb = jb_lo; jb < jb_hi; ++jb) ntile_blk += nkc_of(jb);
        long long nblk_mine = 0;
        for (long long b = blk0; b < S2_BLK_END; b += blk_step) ++nblk_mine;
        const long long ntot = ntile_blk * nblk_mine;
        bool last_m1 = (ntile_blk == 1), last_m2 = false;
        int slot = 1, par = 1;
        for (long long i = 0;; ++i) {
            // the matrix wavefronts have just passed barrier i-1: if tile i-1 closed a candidate
            // block, finish that block
            if (last_m2) epilogue();
            if (i == ntot) break;
            // ---- produce tile i+1 = p1 ----
            // (a generating iteration is what the matrix wavefronts wait for on the diagonal tiles: it
            // runs at raised priority -- same box, alternating, 244.4 vs 245.5 ms; raising it for the
            // image requests only is neutral)
            if (is_gen(p1)) __builtin_amdgcn_s_setprio(3);
            dma_tile(slot, p1.jb, p1.kc);
            if (p1.jb == jb_lo && p1.kc == 0) load_candidates(p1.bl);
            if (is_gen(p1)) produce_b(p1.jb, p1.kc, par, par);
            else dma_parked(par, p1.kc);
            x_put(par ^ 1, xq);                       // x chunk of tile i+2
            // VMEM requests of this iteration that barrier i need NOT wait for: the park stores of a
            // first-visit tile (read back a row block later) and the x chunk fetched for tile i+3 (a
            // register load hipcc tracks itself).  They are the LAST requests issued, and gfx9 VMEM
            // completes in issue order, so "at most n outstanding" still means the images and parked
            // operands of tile i+1 have landed -- without the ~1-2 k cycles of store acknowledgement.
            int n_pend = (!SOLVE && !SPARK && is_gen(p1) && park && p1.kc >= S2_CPB * p1.jb && p1.jb + 1 < nrb2) ? 2 : 0;
            if (is_gen(p3)) { xq = x_fetch(p3.kc); n_pend += X2 ? 2 : 1; }
            last_m2 = last_m1;
            last_m1 = (p1.jb == jb_hi - 1 && p1.kc == nkc_of(p1.jb) - 1);
            p0 = p1; p1 = p2; p2 = p3; p3 = next_of(p3);
            slot = slot == 2 ? 0 : slot + 1;
            par ^= 1;
            __builtin_amdgcn_s_setprio(0);
            // barrier i
            if (n_pend == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else if (n_pend == 1) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else if (n_pend == 2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else if (n_pend == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    }
}

#undef S2_BLK_BEGIN
#undef S2_BLK_END

// The short last round of the persistent grid (and every launch with fewer candidate blocks
// than CUs) is split by ROW BLOCK: one workgroup per (candidate block, row block) writes its
// share of sum V^2 and of mu, this kernel adds the shares in row-block order (deterministic)
// and finishes mu / sigma^2 / utility / block arg-min exactly like the sweep's own epilogue.
// A candidate block is a serial stream of all its tiles otherwise: 9 blocks left over for
// 256 CUs would keep 247 of them idle for a whole block time.
__global__ __launch_bounds__(64) void sweep_finish_kernel(SweepArgs a) {
    const int c = threadIdx.x;
    long long blk = a.blk_begin + blockIdx.x;
    const int pos = S2W_P0(a.split) + (int)blockIdx.x;        // (a seed wave starts at list position P0; 0 otherwise)
    if (a.blk_list) {                             // pruned sweep: the split launch's blocks come from the device list
        const long long cnt = *a.blk_count;
        // (the seed route's first wave: no second-wave seed swept yet -- the word behind the counters the select steps write)
        if ((a.split & S2W_SEED) && pos == 0 && c == 0) ((long long*)a.blk_count)[4] = 0;
        if (cnt <= a.list_lo || cnt > a.list_hi || pos >= cnt) return;
        if (s2_wave_skip(a, a.nrb, S2W_P0(a.split), pos)) return;
        if (S2W_P0(a.split) > 0 && c == 0) atomicAdd((unsigned long long*)a.blk_count + 4, 1ull);
        blk = a.blk_list[pos];
    }
    const long long crow = blk * SW_CAND + c;
    double bu = INFINITY;
    long long bi = -1;
    if (crow < a.m) {
        bool adm = true, has_nan = false;
        double ktl = a.lin_order == 0 ? (double)a.ndim : 0.0;
        for (int d = 0; d < a.ndim; ++d) {
            const double v = a.T[crow * a.ndim + d];
            if (a.has_box && !(v >= a.lo[d] && v <= a.hi[d])) adm = false;
            if (v != v) has_nan = true;
            if (a.lin_coef != 0.0 && a.lin_order > 0) {
                const double p = v * v;
                double q = p;
                for (int e = 1; e < a.lin_order; ++e) q *= p;
                ktl += q;
            }
        }
        if (a.mask && a.mask[crow] == 0) adm = false;
        const long long e0 = ((long long)pos * SW_CAND + c) * a.nrb;
        double q = 0.0, mup = 0.0;
        for (int ib = 0; ib < a.nrb; ++ib) { q += a.sp_q[e0 + ib]; mup += a.sp_mu[e0 + ib]; }
        double mu = mup + a.mean;
        double var = fma(a.lin_coef, ktl, a.amp) - q;
        if (has_nan) { mu = NAN; var = NAN; }
        if (a.mu) a.mu[crow] = mu;
        if (a.var) a.var[crow] = var;
        if (a.kind != APGP_UTIL_NONE) {
            const double uu = (adm && !has_nan) ? util_value(a.kind, mu, var, a.zeta, a.ybest) : INFINITY;   // (as the sweep)
            if (a.u) a.u[crow] = uu;
            best_merge(bu, bi, uu, a.idx_offset + crow);
        }
    }
    if (a.kind == APGP_UTIL_NONE) return;
    for (int o = 32; o > 0; o >>= 1) {
        double ou = __shfl_xor(bu, o);
        long long oi = __shfl_xor(bi, o);
        best_merge(bu, bi, ou, oi);
    }
    if (c == 0) { a.part_u[blk] = bu; a.part_i[blk] = bi; }
}

// The fold of the row-half items (between the seed launch and sweep_finish_kernel): one workgroup per (list position,
// row block), its 256 threads the matrix threads of the item.  For a row block that went as two halves it runs the
// chain of squares on from the upper half's prefix through the lower half's 32 stored accumulators, in the whole
// item's order, and writes the share the whole item would have written.  Sized for the cap; leaves on the device count.
__global__ __launch_bounds__(256) void sweep_fold_kernel(SweepArgs a) {
    const long long cnt = *a.blk_count;
    const int pos = S2W_P0(a.split) + (int)blockIdx.x / a.nrb, jb = (int)blockIdx.x % a.nrb;
    const int lg = S2W_LG(a.split), np = s2_nparts(jb, S2W_J0(a.split), a.n, lg);
    if (cnt <= a.list_lo || cnt > a.list_hi || pos >= cnt || np < 2) return;
    if (s2_wave_skip(a, a.nrb, S2W_P0(a.split), pos)) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const double* base = s2_fold_item(a.sp_q, a.nrb, a.blk_end, pos, jb);
    const f64x2* P = (const f64x2*)base + t;
    const f64x2* A = (const f64x2*)(base + S2_HQ_PRE) + t;
    double qr[4];
    {
        const f64x2 v0 = P[0], v1 = P[256];
        qr[0] = v0.x; qr[1] = v0.y; qr[2] = v1.x; qr[3] = v1.y;
    }
    // sub-blocks 2 pp .. 2 pp np - 1 of the whole item, the parts after the first (sub-block s at piece pair s - 2)
    const int s_lo = 2 * (S2_NP >> lg) - 2, s_hi = 2 * (S2_NP >> lg) * np - 2;
    for (int s_ = s_lo; s_ < s_hi; ++s_) {
        const f64x2 v0 = A[(2 * s_) * 256], v1 = A[(2 * s_ + 1) * 256];
        qr[0] = fma(v0.x, v0.x, qr[0]);
        qr[1] = fma(v0.y, v0.y, qr[1]);
        qr[2] = fma(v1.x, v1.x, qr[2]);
        qr[3] = fma(v1.y, v1.y, qr[3]);
    }
    double qtot = 0.0;
    qtot += s2_q_gather(qr, lane);                // (as the kernel: the share is 0 + the row block's sum)
    if ((lane >> 4) == 0) a.sp_q[((long long)pos * SW_CAND + w * 16 + (lane & 15)) * a.nrb + jb] = qtot;
}

// The parked stream of the seed blocks (before the seed launch): one workgroup per (list position, SP_NCH chunks
// kc < ncache), its 256 threads the feeder threads of the block.  It writes the 1024 operands a feeder of the persistent
// sweep would have parked for each chunk kc, into slot `position` of the k* scratch, so that the seed launch's 2 nrb
// items per block read the chunks left of their diagonal instead of generating them once each.  The bits are those of
// produce_b, said explicitly with contraction off (tests/kvalue_ref.py, site "sweep"): chunk 0 is the tile an item
// generates in its prologue, where hipcc contracts the scaling into the subtraction, df = fma(t, sc, -xs); every other
// chunk takes the rounded tt = t sc.  Rows past m enter as t = 0, as in load_candidates.  Pure squared-exponential
// kernels only.  Sized for the cap; a workgroup whose position is at or past the device count leaves at once.
#define SP_NCH 4                         // chunks per workgroup
template <int DPAD>
__global__ __launch_bounds__(256) void seed_park_kernel(SweepArgs a) {
#pragma clang fp contract(off)
    constexpr int XS = DPAD + 2;
    constexpr int NKK = SW_KC / 4;
    __shared__ double Etab[APGP_EXP_TAB_N];
    const int ngrp = a.ncache / SP_NCH;           // (ncache is a multiple of S2_CPB)
    const int pos = S2W_P0(a.split) + (int)blockIdx.x / ngrp, kc0 = (int)blockIdx.x % ngrp * SP_NCH;
    const long long cnt = *a.blk_count;
    if (cnt <= a.list_lo || cnt > a.list_hi || pos >= cnt) return;
    if (s2_wave_skip(a, a.nrb, S2W_P0(a.split), pos)) return;
    apgp_exp_tab_load(Etab);
    __syncthreads();
    const int ht = threadIdx.x, lane = ht & 63, hw = ht >> 6;
    const int cl = lane & 15, kq = lane >> 4;
    const long long blk = a.blk_list[pos];
    const long long crow = blk * SW_CAND + hw * 16 + cl;
    const bool inb = blk < a.blk_end && crow < a.m;
    double tv[DPAD], tt[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) {
        double v = 0.0;
        if (inb && d < a.ndim) v = a.T[crow * a.ndim + d];
        tv[d] = v;
        tt[d] = v * a.sc[d];
    }
    for (int kc = kc0; kc < kc0 + SP_NCH; ++kc) {
        const double* Xb = a.xs + (long long)kc * (SW_KC * XS);
        double s2[NKK], s3[NKK];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) { s2[kk] = 0.0; s3[kk] = 0.0; }
#pragma unroll
        for (int d = 0; d < DPAD; d += 2)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const f64x2 xa = *(const f64x2*)(Xb + (kk * 4 + kq) * XS + d);
                double df0, df1;
                if (kc == 0) { df0 = fma(tv[d], a.sc[d], -xa.x); df1 = fma(tv[d + 1], a.sc[d + 1], -xa.y); }
                else { df0 = tt[d] - xa.x; df1 = tt[d + 1] - xa.y; }
                s2[kk] = fma(df0, df0, s2[kk]);
                s3[kk] = fma(df1, df1, s3[kk]);
            }
        double ex[NKK], bfv[NKK];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) ex[kk] = -(s2[kk] + s3[kk]);
        apgp_exp4(ex, bfv, Etab);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) bfv[kk] = bfv[kk] * a.amp;
        // the layout produce_b stores: thread ht's q0 at byte 16 ht, q1 at 16 ht + 4096, chunk stride SW_BCH * 8
        f64x2* dst = (f64x2*)(a.kcache + ((long long)pos * a.ncache + kc) * SW_BCH) + ht;
        f64x2 q0, q1;
        q0.x = bfv[0]; q0.y = bfv[1]; q1.x = bfv[2]; q1.y = bfv[3];
        dst[0] = q0; dst[256] = q1;
    }
}

// blocks of the last round that are split by row block (measured break-even at N = 4096:
// ~190 of 256 -- the split launch regenerates every k* and its largest item is 1/nrb of a block): S2_SPLIT_MAX, above

static inline int s2_nrb(int64_t n) { return (int)((n + S2_ROWS - 1) / S2_ROWS); }
// chunks per workgroup slot whose B operands are revisited by a later 256-row block
static inline long long s2_ncache(int64_t n) { return (long long)S2_CPB * (s2_nrb(n) - 1); }

// dynamic LDS of sweep2_kernel<DPAD, *>
template <int DPAD>
static constexpr size_t s2_lds_bytes() {      // (the larger of the two feeder forms' x staging)
    return (3 * S2_TILE + 2 * 4 * 256 + 3 * ((SW_KC * (DPAD + 2) * 8 + 1023) / 1024 * 128) + APGP_EXP_TAB_N + SW_CAND + 8 +
            4 * APGP_MAX_DIM) * sizeof(double);
}

// The kernel needs > 64 KiB of dynamic LDS: the attribute is per device (and per kernel
// instantiation), so it is set -- and its result checked -- once for each device this process
// launches on.
template <int DPAD>
static int s2_prepare_device() {
    static ApgpLdsOnce once;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        apgp_set_error("apgp_acquire: hipGetDevice failed");
        return -2;
    }
    return apgp_raise_lds(once, "apgp_acquire", dev, (int)s2_lds_bytes<DPAD>(),
                          {(const void*)sweep2_kernel<DPAD, false, 0>, (const void*)sweep2_kernel<DPAD, true, 0>,
                           (const void*)sweep2_kernel<DPAD, false, 1>, (const void*)sweep2_kernel<DPAD, true, 1>,
                           (const void*)sweep2_kernel<DPAD, false, 2>, (const void*)sweep2_kernel<DPAD, true, 2>,
                           (const void*)sweep2_kernel<DPAD, false, 0, true>, (const void*)sweep2_kernel<DPAD, true, 0, true>,
                           (const void*)sweep2_kernel<DPAD, false, 1, true>, (const void*)sweep2_kernel<DPAD, true, 1, true>,
                           (const void*)sweep2_kernel<DPAD, false, 2, true>, (const void*)sweep2_kernel<DPAD, true, 2, true>,
                           (const void*)sweep2_kernel<DPAD, false, 0, true, true>, (const void*)sweep2_kernel<DPAD, true, 0, true, true>,
                           (const void*)sweep2_kernel<DPAD, false, 0, true, true, true>});
}

// one launch of the kernel that fits (form, N, LinearKernel term); LIST: its blocks come from a.blk_list
template <int DPAD, bool LIST>
static void s2_launch(const SweepArgs& a, hipStream_t s, bool solve, unsigned grid) {
    const size_t lds = s2_lds_bytes<DPAD>();
    if (solve && a.nrb <= S2_STATIC_DIAG_NRB) {
        if (a.lin_coef != 0.0)
            hipLaunchKernelGGL((sweep2_kernel<DPAD, true, 2, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
        else
            hipLaunchKernelGGL((sweep2_kernel<DPAD, false, 2, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
    } else if (solve) {
        if (a.lin_coef != 0.0)
            hipLaunchKernelGGL((sweep2_kernel<DPAD, true, 1, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
        else
            hipLaunchKernelGGL((sweep2_kernel<DPAD, false, 1, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
    } else if (a.lin_coef != 0.0)
        hipLaunchKernelGGL((sweep2_kernel<DPAD, true, 0, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
    else
        hipLaunchKernelGGL((sweep2_kernel<DPAD, false, 0, LIST>), dim3(grid), dim3(S2_THREADS), lds, s, a);
}

template <int DPAD>
static int launch_sweep(const SweepArgs& a0, hipStream_t s, bool solve) {
    const int rc = s2_prepare_device<DPAD>();
    if (rc != 0) return rc;
    SweepArgs a = a0;
    const long long ncb = (a.m + SW_CAND - 1) / SW_CAND;
    const int nrb2 = s2_nrb(a.n);
    a.nrb = nrb2;
    // full rounds on the persistent grid, then the remainder split by row block (the substitution
    // form cannot split: its row blocks depend on each other -- the last round just runs short)
    long long rest = ncb % SW_GRID;
    if (solve || nrb2 < 2 || rest > S2_SPLIT_MAX || a.sp_q == NULL) rest = 0;
    const long long full = ncb - rest;
    if (full > 0) {
        a.blk_begin = 0; a.blk_end = full; a.split = 0;
        s2_launch<DPAD, false>(a, s, solve, (unsigned)(full < SW_GRID ? full : SW_GRID));
    }
    if (rest > 0) {
        a.blk_begin = full; a.blk_end = ncb; a.split = 1;
        a.ncache = 0;                             // no parking across workgroups
        a.kslot_bytes = SW_BCH * 8;
        s2_launch<DPAD, false>(a, s, solve, (unsigned)(rest * nrb2));
        hipLaunchKernelGGL(sweep_finish_kernel, dim3((unsigned)rest), dim3(64), 0, s, a);
    }
    return 0;
}

// The blocks blk_list[0 .. *blk_count) (count <= max_count, known to the device only) through the same kernel.  No host
// round trip: up to `cap` blocks (inverse form, N > 256) go split by row block -- a grid sized for cap blocks whose
// surplus workgroups leave at once --, more than cap over the persistent grid; both launches are enqueued and the
// count decides on the device which of them works.
// ---- which row blocks of the seed launch go as two halves ----
// -1: the rule below; v >= 0: J0 = v (0: every row block with a lower half, v >= nrb: none -- the launch without halves)
static int g_seed_rowsplit = -1;

extern "C" int apgp_set_seed_rowsplit(int v) {
    return __atomic_exchange_n(&g_seed_rowsplit, v < 0 ? -1 : v, __ATOMIC_RELAXED);
}

extern "C" int apgp_get_seed_rowsplit(void) { return __atomic_load_n(&g_seed_rowsplit, __ATOMIC_RELAXED); }

// ---- whether the seed launch reads its blocks' k* from the parked stream (seed_park_kernel) ----
// 1 (default): yes, for pure squared-exponential kernels; 0: every item generates every tile, the launch as it was
static int g_seed_park = 1;

extern "C" int apgp_set_seed_park(int v) { return __atomic_exchange_n(&g_seed_park, v != 0 ? 1 : 0, __ATOMIC_RELAXED); }

extern "C" int apgp_get_seed_park(void) { return __atomic_load_n(&g_seed_park, __ATOMIC_RELAXED); }

// ---- whether the coarse bound over the sign-sorted rows runs its pipelined row loop (prune_mm32.h, PIPE) ----
// 1 (default): yes; 0: the loop as hipcc orders it, the kernel as it was.  The same bits either way.
static int g_prune_pipe = 1;

extern "C" int apgp_set_prune_pipe(int v) { return __atomic_exchange_n(&g_prune_pipe, v != 0 ? 1 : 0, __ATOMIC_RELAXED); }

extern "C" int apgp_get_prune_pipe(void) { return __atomic_load_n(&g_prune_pipe, __ATOMIC_RELAXED); }

// ---- how far ahead the parked seed launch requests the re-read tiles of its part items (sweep2_kernel, DEEP) ----
// 0: one tile ahead, the launch as it was; d > 0: the stage-ring instantiation, up to d tiles ahead (at most what the ring
// of the item's part size holds: 2 / 4 / 6 for four / two / one pair).  The same bits either way.
#define S2_PREFETCH_MAX 6
static_assert(S2_PREFETCH_MAX == S2_NRING(1) - 2 && S2_PREFETCH_MAX <= 7, "the deepest ring's distance, in three bits of split");
static int g_seed_prefetch = S2_PREFETCH_MAX;

extern "C" int apgp_set_seed_prefetch(int v) {
    return __atomic_exchange_n(&g_seed_prefetch, v < 0 ? 0 : (v > S2_PREFETCH_MAX ? S2_PREFETCH_MAX : v), __ATOMIC_RELAXED);
}

extern "C" int apgp_get_seed_prefetch(void) { return __atomic_load_n(&g_seed_prefetch, __ATOMIC_RELAXED); }

// ---- how many of the PR_SEED seeds the first seed wave sweeps ----
// -1: the rule (S2_SEED_FIRST where the split seed route applies, all of them elsewhere); 1 .. 16: that many (16: one wave)
#define S2_SEED_FIRST 4
static int g_seed_first = -1;

extern "C" int apgp_set_seed_first(int v) {
    return __atomic_exchange_n(&g_seed_first, v < 1 ? -1 : (v > 16 ? 16 : v), __ATOMIC_RELAXED);
}

extern "C" int apgp_get_seed_first(void) { return __atomic_load_n(&g_seed_first, __ATOMIC_RELAXED); }

// ---- sub-block pairs per item of a split row block of the seed launches ----
// -1: the rule (seed_plan); 8 / 4 / 2 / 1: whole items, halves, two-pair, one-pair items
static int g_seed_parts = -1;

extern "C" int apgp_set_seed_parts(int v) {
    return __atomic_exchange_n(&g_seed_parts, (v == 8 || v == 4 || v == 2 || v == 1) ? v : -1, __ATOMIC_RELAXED);
}

extern "C" int apgp_get_seed_parts(void) { return __atomic_load_n(&g_seed_parts, __ATOMIC_RELAXED); }

// Time of a launch of cap x (row items for J0) workgroups on SW_GRID CUs, one at a time per CU, in the order the
// kernel numbers them (s2_row_item: heaviest first), each to the CU that falls free first; in units of the cost model
// (S2_WHOLE_COST per tile of a whole item, S2_HALF_COST per tile of a half item or of a last block of <= 128 rows).
// `parked`: the launch reads the chunks left of an item's diagonal from the parked stream; a re-read tile and a
// generating (diagonal) tile then have prices of their own (S2P_*), in units that only compare with each other.
// `lg`: a split row block goes as 2^lg parts; a part of two pairs or of one has its own prices on the parked route.
// `route`: S2R_PLAIN (nothing parked), S2R_PARKED, or S2R_RING: the parked route whose part items run the stage-ring loop
// (apgp_set_seed_prefetch > 0) and have the S2Q_* prices; its whole items run the other loop and keep S2P_*.
enum { S2R_PLAIN = 0, S2R_PARKED = 1, S2R_RING = 2 };
static long long seed_launch_cost(int nrb, int cap, int n, int j0, int lg, int route) {
    static const int gen[4] = {S2P_WHOLE_GEN, S2P_HALF_GEN, S2P_PAIR2_GEN, S2P_PAIR1_GEN};
    static const int park[4] = {S2P_WHOLE_PARK, S2P_HALF_PARK, S2P_PAIR2_PARK, S2P_PAIR1_PARK};
    static const int gen_ring[4] = {S2P_WHOLE_GEN, S2Q_HALF_GEN, S2Q_PAIR2_GEN, S2Q_PAIR1_GEN};
    static const int park_ring[4] = {S2P_WHOLE_PARK, S2Q_HALF_PARK, S2Q_PAIR2_PARK, S2Q_PAIR1_PARK};
    const bool parked = route != S2R_PLAIN;
    long long load[SW_GRID] = {0};
    const int nitem = s2_nitems(nrb, j0, n, lg);
    long long last = 0;
    for (int i = 0; i < nitem; ++i) {
        int jb = 0, h = -1;
        s2_row_item(i, nrb, j0, n, lg, jb, h);
        const int kind = h >= 0 ? lg : (n - S2_ROWS * jb <= S2_ROWS / 2 ? 1 : 0);     // (a last block of <= 128 rows: a half's prices)
        const int nkc = s2_nkc_of(jb, n), nre = S2_CPB * jb < nkc ? S2_CPB * jb : nkc;
        const bool ring = route == S2R_RING && h >= 0;
        const long long c = parked ? (long long)(ring ? gen_ring : gen)[kind] * (nkc - nre) + (long long)(ring ? park_ring : park)[kind] * nre
                                   : (long long)s2_part_cost(kind) * nkc;
        for (int k = 0; k < cap; ++k) {
            int best = 0;
            for (int q = 1; q < SW_GRID; ++q)
                if (load[q] < load[best]) best = q;
            load[best] += c;
            if (load[best] > last) last = load[best];
        }
    }
    return last;
}

// The rule: J0 of {0, nrb / 2, nrb} with the shortest modelled launch (ties: the fewest items).  Remembered for the last
// (nrb, cap, n): a fit's calls repeat them.
// The parts of a split row block follow the same rule: halves, or (parked route) two-pair items where the model says
// they shorten the launch; one-pair items only when forced, or (stage-ring route, whose prices make them the shortest
// around N = 1152) where the model says so.  Remembered for the last few (nrb, blocks, n, route, forced values): a call's
// two waves and a fit's calls repeat them.
struct SeedPlan { int j0, lg; long long cost; };
static SeedPlan seed_plan(int nrb, int cap, int n, int route) {
    const int v = apgp_get_seed_rowsplit(), fp = apgp_get_seed_parts();
    const int flg = fp == 8 ? 0 : fp == 4 ? 1 : fp == 2 ? 2 : fp == 1 ? 3 : -1;
    struct Memo { int nrb, cap, n, route, v, flg; SeedPlan plan; };
    static std::mutex mu;
    static Memo memo[8];
    static int nmemo = 0, next = 0;
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < nmemo; ++i) {
        const Memo& e = memo[i];
        if (e.nrb == nrb && e.cap == cap && e.n == n && e.route == route && e.v == v && e.flg == flg) return e.plan;
    }
    SeedPlan best = {nrb, 1, 0};
    long long best_c = -1;
    for (int lg = 1; lg <= (route == S2R_RING ? 3 : route == S2R_PARKED ? 2 : 1); ++lg) {
        if (flg >= 0 && lg != 1) continue;         // (forced parts: one pass, with them)
        const int l = flg >= 0 ? flg : lg;
        for (int j0 : {nrb, nrb / 2, 0}) {
            if (v >= 0 && j0 != nrb) continue;     // (forced J0: one pass, with it)
            const int j = v >= 0 ? (v < nrb ? v : nrb) : j0;
            if (lg > 1 && j == nrb) continue;
            const long long c = seed_launch_cost(nrb, cap, n, j, l, route);
            if (best_c < 0 || c < best_c) { best = {j, l, c}; best_c = c; }
        }
    }
    memo[next] = {nrb, cap, n, route, v, flg, best};
    next = (next + 1) % 8;
    if (nmemo < 8) ++nmemo;
    return best;
}

// `rowsplit` (the seed launches): row blocks from seed_plan's J0 on go as 2, 4 or 8 row-part items each, folded by
// sweep_fold_kernel, and the seeds go in two waves.
template <int DPAD>
static void launch_sweep_list(const SweepArgs& a0, hipStream_t s, bool solve, const long long* list,
                              const long long* count, long long max_count, long long cap, bool rowsplit = false) {
    SweepArgs a = a0;
    const int nrb2 = s2_nrb(a.n);
    a.nrb = nrb2;
    a.blk_list = list; a.blk_count = count;
    a.blk_begin = 0; a.blk_end = (a.m + SW_CAND - 1) / SW_CAND;     // (LIST: one past the largest block NUMBER)
    const bool can_split = !solve && nrb2 >= 2 && a.sp_q != NULL;
    if (cap > max_count) cap = max_count;
    if (can_split) {
        SweepArgs b = a;
        b.split = 1; b.ncache = 0; b.kslot_bytes = SW_BCH * 8;
        b.list_lo = 0; b.list_hi = cap;
        // the seed launch of a pure squared-exponential kernel reads the chunks left of an item's diagonal from the
        // parked stream: seed_park_kernel fills slot `position` of the k* scratch, idle until the survivors' persistent
        // launch later on this stream (slots >= the seed count), and the launch goes through the RHALF instantiation
        // whether a row block is halved or not (it runs whole items with rh = -1)
        const bool parked = rowsplit && b.lin_coef == 0.0 && apgp_get_seed_park() != 0;
        // Two seed waves (pure squared-exponential kernels): the first K seeds, then -- each workgroup on its own, from
        // tau_1 of the first wave and the seed's bound (s2_wave_skip) -- those of the other seeds that could still win or
        // tie.  At the benchmark's sizes none can: the seeds' bounds lie further apart than the bound's slack, and the
        // first wave is all the exact work tau needs.  Both waves are the same four launches over their positions.
        // (the prices of the loop the part items run: the stage ring's at apgp_set_seed_prefetch > 0)
        const int kroute = apgp_get_seed_prefetch() > 0 ? S2R_RING : S2R_PARKED;
        int first = (int)cap;
        if (rowsplit && b.lin_coef == 0.0) {
            const int v = apgp_get_seed_first();
            // the rule: S2_SEED_FIRST where the model says the shorter first wave pays for the second one's launches
            // (from N ~ 2048 on; below, 16 blocks' items are about one per CU and a wave lasts its heaviest item either
            // way).  By the parked route's prices with the stream on or off: the same seeds are swept.  (K may differ
            // between the two values of apgp_set_seed_prefetch; tau and the winner depend on neither.)
            first = v > 0 ? v : S2_SEED_FIRST;
            if (first > (int)cap) first = (int)cap;
            if (v <= 0 && first < (int)cap &&
                seed_plan(nrb2, (int)cap, b.n, kroute).cost - seed_plan(nrb2, first, b.n, kroute).cost <= S2P_WAVE2)
                first = (int)cap;
        }
        for (int wave = 0; wave < (first < (int)cap ? 2 : 1); ++wave) {
            const int p0 = wave ? first : 0, p1 = wave ? (int)cap : first, nw = p1 - p0;
            const SeedPlan plan = rowsplit ? seed_plan(nrb2, nw, b.n, parked ? kroute : S2R_PLAIN) : SeedPlan{nrb2, 0, 0};
            const int nitem = s2_nitems(nrb2, plan.j0, b.n, plan.lg);
            b.split = S2W_WORD(plan.j0, plan.lg, p0, p1);
            if (parked) {
                b.ncache = (int)s2_ncache(b.n);
                b.kslot_bytes = (unsigned)(b.ncache * (SW_BCH * 8));
                hipLaunchKernelGGL(seed_park_kernel<DPAD>, dim3((unsigned)(nw * (b.ncache / SP_NCH))), dim3(256), 0, s, b);
            }
            if (nitem > nrb2 || parked || first < (int)cap) {
                const size_t lds = s2_lds_bytes<DPAD>();
                const unsigned grid = (unsigned)(nw * nitem);
                const int pf = parked ? apgp_get_seed_prefetch() : 0;
                if (b.lin_coef != 0.0)
                    hipLaunchKernelGGL((sweep2_kernel<DPAD, true, 0, true, true>), dim3(grid), dim3(S2_THREADS), lds, s, b);
                else if (pf > 0) {                // (the part items' stage ring; whole items run as in the other instantiation)
                    SweepArgs d = b;
                    d.split |= pf << 25;
                    hipLaunchKernelGGL((sweep2_kernel<DPAD, false, 0, true, true, true>), dim3(grid), dim3(S2_THREADS), lds, s, d);
                } else
                    hipLaunchKernelGGL((sweep2_kernel<DPAD, false, 0, true, true>), dim3(grid), dim3(S2_THREADS), lds, s, b);
                if (nitem > nrb2) hipLaunchKernelGGL(sweep_fold_kernel, dim3((unsigned)(nw * nrb2)), dim3(256), 0, s, b);
            } else {
                b.split = 1;
                s2_launch<DPAD, true>(b, s, solve, (unsigned)(cap * nrb2));
            }
            SweepArgs f = b;
            f.split = rowsplit ? (S2W_WORD(plan.j0, plan.lg, p0, p1) | S2W_SEED) : 1;
            hipLaunchKernelGGL(sweep_finish_kernel, dim3((unsigned)nw), dim3(64), 0, s, f);
        }
    }
    if (!can_split || max_count > cap) {
        a.split = 0;
        a.list_lo = can_split ? cap : 0; a.list_hi = APGP_MAX_M;
        s2_launch<DPAD, true>(a, s, solve, (unsigned)(max_count < SW_GRID ? max_count : SW_GRID));
    }
}

// ---------------------------------------------------------------------------
// Pruned arg-min ("Branch and bound on the arg-min").  acquire returns ONE row.  For every
// candidate var = k(t,t) - |L^-1 k*|^2 <= k(t,t), and the three utilities do not increase with var at fixed mu, so
//   b_i = util(mu_i, k(t_i,t_i)) <= u_i,
// at the price of a mean-only prediction (N (3D + 4) flops against N^2).  A candidate whose bound lies above the
// utility tau of ANY fully evaluated admissible candidate can neither be the arg-min nor tie it.  Whole 64-row blocks
// are pruned, never rows: a surviving row keeps its block, lane and global index and goes through the sweep's own
// kernel, so its utility has the bits the full sweep gives it.
//   1. prune_bound_kernel   bmin[blk] = min_i (b_i - slack_i) (+inf: no admissible row); part_u/part_i = (+inf, -1)
//   2. prune_seed_kernel    the PR_SEED blocks with the smallest bmin
//   3. sweep on the seeds   -> their part_u / part_i
//   4. prune_select_kernel  tau = min part_u of the seeds; the blocks with bmin <= tau that are not seeds, in
//                           ascending order, and their count
//   5. sweep on that list; argmin_final_kernel over all partials as ever.
// slack_i (prune_bound_kernel) covers every rounding between b_i as computed there and u_i as the sweep computes it,
// so "bmin <= tau" keeps every row that could win or TIE: the lowest global index still wins.
// tau = +inf (no seed row with a finite utility): every block with an admissible row survives.
// ---------------------------------------------------------------------------
#define PR_THREADS 256
#define PR_CPT 2            // candidates per thread: two blocks per wavefront, half the LDS reads per kernel value
#define PR_ROWS 128         // training rows per LDS tile (divides the packed stream's 512-row padding)
#define PR_SEED 16          // seed blocks: the SELECTION -- tau is the minimum over all 16, and all 16 stay out of the lists;
                            // the first wave sweeps K of them (apgp_set_seed_first), the second those of the rest
                            // whose bound does not lie above the first wave's tau_1 (launch_sweep_list)
// candidates below which the full sweep is taken (apgp_set_sweep_prune(1)).  The pruned call costs about one block's
// time whatever m is (the seeds), the full sweep m N^2.  Re-measured with the fp32 bound pass (docs/experiments.md,
// round 9): pruned / full = 0.95 at m = 4096 and 0.29 at 16384 for N = 4096; 0.94 at 16384 and 0.27 at 65536 for
// N = 1152 -- level at the lower neighbours, against 1.27x when nothing prunes: the thresholds stay
static inline int64_t pr_min_m(int64_t n) { return n >= 4096 ? 16384 : 65536; }

struct PruneArgs {
    const double* T;
    const double* xs;
    const unsigned char* mask;
    double* bmin;
    double* part_u;
    long long* part_i;
    long long m, ncb, n;
    int ndim, kind, has_box, lin_order;
    double mean, amp, lin_coef, zeta, ybest;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
    // refine stage (prune_bound_kernel<.., LIST = true>): the blocks blk_list[0 .. *blk_count), a count the device computed
    const long long* blk_list;
    const long long* blk_count;
    // coarse stage: per block the smallest b WITHOUT the slack (NULL: not wanted) -- where the minimum probably lies,
    // which is what the seeds are chosen by; a seed need not come from a valid bound
    double* est;
    // coarse stage up to Dpad = 8: the training rows split into bf16 parts once per fit (apgp_pack_prune_rows), or NULL:
    // every workgroup splits them itself
    const void* prune_rows;
    // which stream prune_rows is (host side only: launch_bound picks the kernel by it): APGP_PRUNE_ROWS_SPLIT, or
    // APGP_PRUNE_ROWS_SIGNED: the rows sorted by alpha's sign (apgp_pack_prune_srows), the one-chain route
    int rows_kind;
};

// Slack of a coarse bound: prune_bound_kernel's (derived there) with S <= amp sum|alpha| for its S, added in that
// kernel's order onto base = 2 e32, what the coarse mu may be off by times |du/dmu| <= 2.
template <int DPAD>
__device__ __forceinline__ double pr_slack(const PruneArgs& a, double base, double S, double mu, double ktt, double b) {
    const double eps = 0x1p-53;
    double slack = base + 2.0 * (4.0 * (double)(a.n + 16) + 8.0 * DPAD + 32.0) * eps * S +
                   64.0 * eps * (1.0 + fabs(mu) + fabs(a.ybest) + fabs(a.zeta) + ktt + fabs(b));
    if (a.kind == APGP_UTIL_BAPE) slack += 16.0 * eps / (1.0 - exp(0.0 - ktt));
    return slack;
}

// The end of a bound: a row's b (with or without its slack) -> the minimum over the W lanes that hold a block's rows (64)
// or half of them (32).  A bound that is NaN bounds nothing: -inf, the block is evaluated; a row that is not admissible
// cannot win: +inf.
template <int W>
__device__ __forceinline__ double pr_block_min(double b, bool adm) {
    if (!(b == b)) b = -INFINITY;
    if (!adm) b = INFINITY;
    for (int o = W / 2; o > 0; o >>= 1) b = fmin(b, __shfl_xor(b, o));
    return b;
}

// a block's arg-min partial before any sweep has seen the block: a pruned block's never wins
__device__ __forceinline__ void pr_prefill(const PruneArgs& a, long long blk) {
    if (a.part_u) {
        a.part_u[blk] = INFINITY;
        a.part_i[blk] = -1;
    }
}

// what one lane writes for block blk of a coarse stage: the block minimum of the bounds, of the b without slack where
// asked for (PruneArgs::est), and with PREFILL the partial
template <bool PREFILL>
__device__ __forceinline__ void pr_store_block(const PruneArgs& a, long long blk, double b, double be) {
    a.bmin[blk] = b;
    if (a.est) a.est[blk] = be;
    if (PREFILL) pr_prefill(a, blk);
}

// LIST: the refine stage of a call that bounded coarsely first (prune_bound32_kernel): only the blocks of a device list,
// bmin[blk] = max(coarse, this bound) -- both are valid, the larger prunes more --, and no pre-fill of the partials.  The
// launch is sized for the longest list; a workgroup beyond the count leaves before its first barrier.
template <int DPAD, bool LIST = false>
__global__ __launch_bounds__(PR_THREADS) void prune_bound_kernel(PruneArgs a) {
    constexpr int XS = DPAD + 2;                 // packed stream row: scaled x | alpha | 0
    constexpr int PIECES = PR_ROWS * XS / 2;     // 16-byte pieces per tile
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double tile[PR_ROWS * XS];
    long long lst_count = 0;
    if (LIST) {
        lst_count = *a.blk_count;
        if ((long long)blockIdx.x * (PR_THREADS / 64) * PR_CPT >= lst_count) return;
    }
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // wavefront w: candidate blocks blk0, blk0 + 1 (the sweep's SW_CAND blocks, same numbering), lane = row in block
    const long long blk0 = ((long long)blockIdx.x * (PR_THREADS / 64) + w) * PR_CPT;
    long long blk[PR_CPT];
#pragma unroll
    for (int c = 0; c < PR_CPT; ++c) blk[c] = !LIST ? blk0 + c : (blk0 + c < lst_count ? a.blk_list[blk0 + c] : a.ncb);
    double tt[PR_CPT][DPAD], ktt[PR_CPT];
    bool adm[PR_CPT];
#pragma unroll
    for (int c = 0; c < PR_CPT; ++c) {
        // admissibility and k(t,t) exactly as the sweep's load_candidates.  (The three bound kernels each write this load
        // out: as one force-inlined function -- coordinates returned in an array or handed to a callback, the arguments by
        // reference, value or pointer -- hipcc reads the whole PruneArgs up front, keeps it in SGPRs that spill into VGPR
        // lanes, and the VGPR counts move: docs/experiments.md, round 20.)
        const long long row = blk[c] * SW_CAND + lane;
        const bool live = blk[c] < a.ncb && row < a.m;
        bool ok = live, has_nan = false;
        double ktl = a.lin_order == 0 ? (double)a.ndim : 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            double v = 0.0;
            if (live && d < a.ndim) {
                v = a.T[row * a.ndim + d];
                if (a.has_box && !(v >= a.lo[d] && v <= a.hi[d])) ok = false;
                if (v != v) has_nan = true;
            }
            tt[c][d] = v * a.sc[d];
            if (a.lin_coef != 0.0 && a.lin_order > 0) {
                const double p = v * v;
                double q = p;
                for (int e = 1; e < a.lin_order; ++e) q *= p;
                ktl += q;
            }
        }
        if (live && a.mask && a.mask[row] == 0) ok = false;
        adm[c] = ok && !has_nan;
        ktt[c] = a.lin_coef != 0.0 ? fma(a.lin_coef, ktl, a.amp) : a.amp;
    }
    // mu - mean = sum_k k(t, x_k) alpha_k in four partial sums, and S = sum_k |k(t, x_k)| |alpha_k| for the slack
    double acc[PR_CPT][4], sab[PR_CPT][4];
#pragma unroll
    for (int c = 0; c < PR_CPT; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc[c][q] = 0.0; sab[c][q] = 0.0; }
    const long long ntile = (a.n + PR_ROWS - 1) / PR_ROWS;
    for (long long ti = 0; ti < ntile; ++ti) {
        __syncthreads();                         // the previous tile has been consumed
        const double* src = a.xs + ti * (PR_ROWS * XS);      // (rows < ntile * PR_ROWS <= npad: inside the packed stream)
        for (int e = tid; e < PIECES; e += PR_THREADS) *((f64x2*)tile + e) = *((const f64x2*)src + e);
        __syncthreads();
        for (int r = 0; r < PR_ROWS; r += 4) {
#pragma unroll
            for (int c = 0; c < PR_CPT; ++c) {
                double ex[4], kv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double* xr = tile + (r + q) * XS;
                    double s2 = 0.0, s3 = 0.0;
#pragma unroll
                    for (int d = 0; d < DPAD; d += 2) {
                        const double df0 = tt[c][d] - xr[d];
                        const double df1 = tt[c][d + 1] - xr[d + 1];
                        s2 = fma(df0, df0, s2);
                        s3 = fma(df1, df1, s3);
                    }
                    ex[q] = -(s2 + s3);
                }
                apgp_exp4(ex, kv, etab);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double* xr = tile + (r + q) * XS;
                    double k = kv[q] * a.amp, kabs = k;
                    if (a.lin_coef != 0.0) {
                        // the sweep's LinearKernel sum (produce_b: pairs of dimensions), and the sum of its |terms|
                        double ls = a.lin_order == 0 ? (double)a.ndim : 0.0, la = ls;
                        if (a.lin_order > 0)
#pragma unroll
                            for (int d = 0; d < DPAD; d += 2) {
                                const double p0 = tt[c][d] * xr[d] * a.lw[d], p1 = tt[c][d + 1] * xr[d + 1] * a.lw[d + 1];
                                double q0 = p0, q1 = p1;
                                for (int e = 1; e < a.lin_order; ++e) { q0 *= p0; q1 *= p1; }
                                ls += q0 + q1;
                                la += fabs(q0) + fabs(q1);
                            }
                        kabs = fma(a.lin_coef, la, k);
                        k = fma(a.lin_coef, ls, k);
                    }
                    acc[c][q] = fma(k, xr[DPAD], acc[c][q]);
                    sab[c][q] = fma(kabs, fabs(xr[DPAD]), sab[c][q]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < PR_CPT; ++c) {
        const double mu = ((acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3])) + a.mean;
        const double S = (sab[c][0] + sab[c][1]) + (sab[c][2] + sab[c][3]);
        double b = util_value(a.kind, mu, ktt[c], a.zeta, a.ybest);
        // slack: what the sweep's u_i, evaluated at var_i <= k(t,t), may lie below this b_i through rounding alone,
        // with eps = 2^-53.
        //  * mu.  Both passes add the same N products k alpha (the kernel values come from the same expressions) in
        //    different orders: each sum is within gamma_N S, gamma_N <~ (N + 2) eps, of the exact one, so the two
        //    differ by <= 2 (N + 2) eps S; doubled, plus (8 Dpad + 32) eps S should hipcc contract a kernel value's
        //    expressions differently in the two kernels (Dpad + 4 operations, S counts the LinearKernel terms by
        //    their absolute values).  |du/dmu| is 1 (AGP), 2 (BAPE), Phi(z) <= 1 (Jones): factor 2.
        //  * util_value at equal mu.  Its terms are each within a few eps of |mu|, |ybest| + |zeta|, k(t,t), |b| or 1
        //    (log, erfc, exp to ~1 ulp; z = imp / sd to eps, and z^2 phi(z) <= 0.3), so two evaluations that are
        //    ordered exactly are ordered to 64 eps (1 + |mu| + |ybest| + |zeta| + k(t,t) + |b|) as computed.  Where
        //    var_i is so small that ITS evaluation is worse conditioned than that (AGP: log var; BAPE: log(1 - exp(-var)),
        //    absolute error eps / (1 - exp(-var))), u_i exceeds b_i by more than it loses; BAPE at a tiny k(t,t)
        //    itself gets the term 16 eps / (1 - exp(-k(t,t))).
        //    (Jones with var_i <= 0 or NaN is 0.0: b_i = -EI <= 0 up to the same rounding.)
        // The expression stands here and in pr_slack (the coarse kernels'): here hipcc contracts the two products into ONE
        // fma; through pr_slack with base 0.0 it rounds the first product on its own (fma(.., S, 0.0), then the second
        // fma), which moves the last bit of the slack and, where b is as small as the slack (Jones), of bmin.
        const double eps = 0x1p-53;
        double slack = 2.0 * (4.0 * (double)(a.n + 16) + 8.0 * DPAD + 32.0) * eps * S +
                       64.0 * eps * (1.0 + fabs(mu) + fabs(a.ybest) + fabs(a.zeta) + ktt[c] + fabs(b));
        if (a.kind == APGP_UTIL_BAPE) slack += 16.0 * eps / (1.0 - exp(0.0 - ktt[c]));
        b -= slack;
        b = pr_block_min<64>(b, adm[c]);
        if (lane == 0 && blk[c] < a.ncb) {
            if (LIST) {
                a.bmin[blk[c]] = fmax(a.bmin[blk[c]], b);
            } else {
                a.bmin[blk[c]] = b;
                if (a.part_u) {                      // pr_prefill, written out: behind the call hipcc forms this
                    a.part_u[blk[c]] = INFINITY;     // kernel's slack with other instructions (docs/experiments.md,
                    a.part_i[blk[c]] = -1;           // round 20)
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Coarse bound in single precision (pure squared-exponential kernels: lin_coef == 0).  A bound has to lie below the
// row's utility, not to be tight: the N kernel values per candidate are computed in fp32 with the hardware exponential
// (about 11 issue slots per value with packed fp32 arithmetic, against ~38 fp64 operations), everything the slack rests
// on stays in fp64.  Same outputs as prune_bound_kernel.
//   * exact part: admissibility (box, mask, NaN) and k(t,t) as in load_candidates; util_value in fp64 on (mu32, k(t,t)).
//   * coordinates: a = (t sc - c) kappa and b = (x - c) kappa are formed in fp64 and then converted, c = the first
//     training row, kappa^2 = log2(e): a data set far from the origin keeps its differences, and
//     k = amp 2^-|a - b|^2 needs no multiply in front of v_exp_f32.
//   * PR32_CPT candidate blocks per wavefront share every LDS read of a training row (16-byte reads of fp32 rows; the
//     alphas of PR32_FLUSH rows in 16-byte reads): 2.25 reads per row against 11 PR32_CPT issue slots of arithmetic.
//   * sums: fp32 over PR32_FLUSH rows, then added into fp64 -- the accumulation error does not grow with N.
//   * the next tile's 16-byte pieces of the packed fp64 stream are loaded into registers before the current tile is
//     consumed, converted and stored after it.
// Error of mu32 against the exact sum over the fp64 inputs (t sc, x, alpha), u = 2^-24, r = |t sc - x|,
// A = |t sc - c|, per training row, in units of amp |alpha|:
//   * distance.  a_d, b_d convert with relative error u each and their fp32 difference rounds once more:
//     |d^_d - d_d| <= 2 u (1 + u) (|a_d| + |b_d|); over the dimensions (Cauchy-Schwarz, |b| <= A + r) the sum of squares
//     is off by <= u (8 A r + 4 r^2) + 32 u^2 A^2 + ..., the two fma chains and their sum add (Dpad / 2 + 1) u r^2:
//     eta(r) <= u (8 A r + C r^2) + 32 u^2 A^2 with C = Dpad / 2 + 5 in the exponent.  Behind the gate
//     u (8 A + Dpad + 8) <= 2^-8 (else the slack is +inf), eta <= (r + r^2) / 256 and
//     |k^ - k| <= e^-r^2 (e^eta - 1) <= u (8 A max_r(r e^(-r^2 + eta)) + C max_r(r^2 e^(-r^2 + eta))) + 32 u^2 A^2
//              <= u (3.52 A + 0.38 C) + u A / 64          (the maxima are 0.431 and 0.371)
//              <= u (4 A + Dpad / 2 + 4)                  (with room for the fp64 roundings of a, b, kappa: 2^-29 u each)
//   * centring.  x - c rounds once (relative, above), but t sc - c may be contracted to one fma, which differs from the
//     sweep's rounded t sc less c by eps |t sc| <= eps (|c| + A) per coordinate, eps = 2^-53: an ABSOLUTE shift delta
//     of a, |delta| <= 1.21 eps (|c| + A) with kappa, that no relative term covers once |c| >~ 2^29.  It moves the
//     exponent by <= 2 r |delta| + |delta|^2 and k by <= max_r(2 r e^-r^2) |delta| (1 + ...) <= 2 eps (|c| + A); the
//     gate takes eps (|c| + A) into its sum, so the linearisation holds as for eta.
//   * exponential: v_exp_f32 is good to 1 ulp, allowed 4 u;  alpha -> fp32: u;  PR32_FLUSH = 8 fma into one fp32 sum:
//     8 u (k^ <= 1);  one u to spare: 18 u together with the constant above.
//   * flushes: a kernel value, an alpha or a product below 2^-126 may become 0: 2^-120 (sum |alpha| + N).
//   * sum |alpha| itself is summed the same way (fp32 over 8 rows, then fp64): below the true one by <= 2^-20 of it;
//     it is taken times 1 + 2^-16.
// |mu32 - mu| <= e32 = amp ((u (4 A + Dpad / 2 + 18) + 2 eps (|c| + A)) sum|alpha| + 2^-120 (sum|alpha| + N)); the slack is
// prune_bound_kernel's with S <= amp sum|alpha| plus 2 e32 (pr_slack; |du/dmu| <= 2).  Not finite: -inf, the block goes on to
// the fp64 bound.
// Variants measured: docs/experiments.md, round 9.
// ---------------------------------------------------------------------------
#define PR32_CPT 4          // candidate blocks per wavefront (2 and 8 measured: docs/experiments.md, round 9)
#define PR32_ROWS 128       // training rows per LDS tile
#define PR32_FLUSH 8        // rows per fp32 partial sum
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// (the candidates' coordinates stay in registers: Dpad / 2 x blocks packed pairs)
// sqrt(log2(e)) to the last bit: kappa^2 ln 2 - 1 = 6e-17 is inside the derivation's "room" (the constant that stood here
// until round 13 was 3.5e-5 too small, a relative error of 7e-5 r^2 in every kernel value that no term covered)
static constexpr double PR32_KAPPA = 0x1.337cc2183b050p+0;
static constexpr int pr32_cpt(int dpad) { return dpad <= 8 ? PR32_CPT : dpad == 16 ? 2 : 1; }

// REDO: behind prune_bound_mm32_kernel (prune_mm32.h), for the blocks it left at -inf alone (its gate failed where this
// kernel's need not); the others keep its bound.  A workgroup without such a block leaves before its first barrier.
template <int DPAD, bool REDO = false>
__global__ __launch_bounds__(PR_THREADS) void prune_bound32_kernel(PruneArgs a) {
    constexpr int XS = DPAD + 2;                         // packed stream row: scaled x | alpha | 0
    constexpr int PIECES = PR32_ROWS * XS / 2;           // 16-byte pieces per tile
    constexpr int NP = (PIECES + PR_THREADS - 1) / PR_THREADS;
    constexpr int HD = DPAD / 2;
    constexpr int CPT = pr32_cpt(DPAD);
    if (REDO) {                                          // (every thread reads the same words: one decision per workgroup)
        const long long wg0 = (long long)blockIdx.x * (PR_THREADS / 64) * CPT;
        bool any = false;
        for (int i = 0; i < (PR_THREADS / 64) * CPT; ++i) any |= wg0 + i < a.ncb && a.bmin[wg0 + i] == -INFINITY;
        if (!any) return;
    }
    const double kappa = PR32_KAPPA;
    __shared__ __attribute__((aligned(16))) float xt[PR32_ROWS * DPAD];
    __shared__ __attribute__((aligned(16))) float at[PR32_ROWS];
    __shared__ double cen[DPAD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < DPAD) cen[tid] = a.xs[tid];
    const long long blk0 = ((long long)blockIdx.x * (PR_THREADS / 64) + w) * CPT;
    f32x2 tt[CPT][HD];
    double ktt[CPT], an[CPT];
    bool adm[CPT], redo[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        // admissibility and k(t,t) exactly as the sweep's load_candidates (lin_coef == 0: k(t,t) = amp)
        const long long row = (blk0 + c) * SW_CAND + lane;
        const bool live = blk0 + c < a.ncb && row < a.m;
        redo[c] = !REDO || (blk0 + c < a.ncb && a.bmin[blk0 + c] == -INFINITY);
        bool ok = live, has_nan = false;
        double a2 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; ++d) {
            double v = 0.0;
            if (live && d < a.ndim) {
                v = a.T[row * a.ndim + d];
                if (a.has_box && !(v >= a.lo[d] && v <= a.hi[d])) ok = false;
                if (v != v) has_nan = true;
            }
            const double ce = v * a.sc[d] - a.xs[d];
            a2 = fma(ce, ce, a2);
            tt[c][d >> 1][d & 1] = (float)(ce * kappa);
        }
        if (live && a.mask && a.mask[row] == 0) ok = false;
        adm[c] = ok && !has_nan;
        ktt[c] = a.amp;
        an[c] = sqrt(a2);
    }
    double acc[CPT], sal = 0.0, c2 = 0.0;
#pragma unroll
    for (int c = 0; c < CPT; ++c) acc[c] = 0.0;
#pragma unroll
    for (int d = 0; d < DPAD; ++d) c2 = fma(a.xs[d], a.xs[d], c2);
    const double cn = sqrt(c2);                          // |c|
    const long long ntile = (a.n + PR32_ROWS - 1) / PR32_ROWS;
    f64x2 pre[NP];
    auto fetch = [&](long long ti) {                     // (rows < ntile * PR32_ROWS <= npad: inside the packed stream)
        const f64x2* src = (const f64x2*)(a.xs + ti * (PR32_ROWS * XS));
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int e = tid + i * PR_THREADS;
            pre[i] = e < PIECES ? src[e] : f64x2{0.0, 0.0};
        }
    };
    fetch(0);
    __syncthreads();                                     // cen
    for (long long ti = 0; ti < ntile; ++ti) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int e = tid + i * PR_THREADS;
            if (e < PIECES) {
                const int r = (2 * e) / XS, col = (2 * e) % XS;      // (XS is even: a piece never straddles two rows)
                if (col < DPAD)
                    *(f32x2*)(xt + r * DPAD + col) = f32x2{(float)((pre[i].x - cen[col]) * kappa),
                                                           (float)((pre[i].y - cen[col + 1]) * kappa)};
                else
                    at[r] = (float)pre[i].x;
            }
        }
        __syncthreads();
        if (ti + 1 < ntile) fetch(ti + 1);
        for (int r0 = 0; r0 < PR32_ROWS; r0 += PR32_FLUSH) {
            float al[PR32_FLUSH], ps[CPT], pa = 0.0f;
#pragma unroll
            for (int q = 0; q < PR32_FLUSH; q += 4) *(f32x4*)(al + q) = *(const f32x4*)(at + r0 + q);
#pragma unroll
            for (int c = 0; c < CPT; ++c) ps[c] = 0.0f;
#pragma unroll
            for (int q = 0; q < PR32_FLUSH; ++q) {
                f32x2 xr[HD];
                if constexpr (DPAD >= 4) {
#pragma unroll
                    for (int h = 0; h < HD; h += 2) {
                        const f32x4 v = *(const f32x4*)(xt + (r0 + q) * DPAD + 2 * h);
                        xr[h] = f32x2{v.x, v.y};
                        xr[h + 1] = f32x2{v.z, v.w};
                    }
                } else {
                    xr[0] = *(const f32x2*)(xt + (r0 + q) * DPAD);
                }
                pa += fabsf(al[q]);
#pragma unroll
                for (int c = 0; c < CPT; ++c) {
                    f32x2 s2 = f32x2{0.0f, 0.0f};
#pragma unroll
                    for (int h = 0; h < HD; ++h) {
                        const f32x2 df = tt[c][h] - xr[h];
                        s2 = __builtin_elementwise_fma(df, df, s2);
                    }
                    const float k = __builtin_amdgcn_exp2f(-(s2.x + s2.y));
                    ps[c] = fmaf(k, al[q], ps[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < CPT; ++c) acc[c] += (double)ps[c];
            sal += (double)pa;
        }
        __syncthreads();                                 // the tile has been consumed
    }
    const double u32 = 0x1p-24, eps = 0x1p-53;
    const double sa = sal * (1.0 + 0x1p-16);
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        const double mu = fma(a.amp, acc[c], a.mean);
        double b = util_value(a.kind, mu, ktt[c], a.zeta, a.ybest);
        double e32 = a.amp * ((u32 * (4.0 * an[c] + 0.5 * DPAD + 18.0) + 2.0 * eps * (cn + an[c])) * sa +
                              0x1p-120 * (sa + (double)a.n));
        if (!(u32 * (8.0 * an[c] + DPAD + 8.0) + eps * (cn + an[c]) <= 0x1p-8)) e32 = INFINITY;
        const double be = pr_block_min<64>(b, adm[c]);
        b = pr_block_min<64>(b - pr_slack<DPAD>(a, 2.0 * e32, a.amp * sa, mu, ktt[c], b), adm[c]);
        // (REDO: the partials were pre-filled by the kernel in front)
        if (lane == 0 && blk0 + c < a.ncb && redo[c]) pr_store_block<!REDO>(a, blk0 + c, b, be);
    }
}

#include "prune_mm32.h"

// (value, block) pairs in ascending order: by value, then by block number
__device__ __forceinline__ bool pr_less(double v, long long i, double w, long long j) { return v < w || (v == w && i < j); }

#define PR_NONE 0x7fffffffffffffffll                     // block number of an empty shortlist entry, value +inf

// The PR_SEED smallest of the E pairs that each lane of a wavefront holds, in order: lane r < PR_SEED returns the r-th
// (PR_NONE if there are fewer).  PR_SEED rounds: every lane offers its smallest pair, the smallest offer wins and its
// lane drops it.  The pairs stay where they are (every index is a compile-time constant), so nothing is sorted or moved
// and nothing spills; block numbers are distinct, which makes the winner unique.
template <int E>
__device__ __forceinline__ void pr_wave_select(double (&lv)[E], long long (&li)[E], double& mv, long long& mi) {
    const int lane = threadIdx.x & 63;
    mv = INFINITY; mi = PR_NONE;
    for (int r = 0; r < PR_SEED; ++r) {
        double hv = lv[0];
        long long hi = li[0];
#pragma unroll
        for (int j = 1; j < E; ++j)
            if (pr_less(lv[j], li[j], hv, hi)) { hv = lv[j]; hi = li[j]; }
        double bv = hv;
        long long bi = hi;
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const long long oi = __shfl_xor(bi, o);
            if (pr_less(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (bi == PR_NONE) break;                        // (the same in every lane) nothing is left
        if (lane == r) { mv = bv; mi = bi; }
        if (hi == bi) {
#pragma unroll
            for (int j = 0; j < E; ++j)
                if (li[j] == bi) { lv[j] = INFINITY; li[j] = PR_NONE; }
        }
    }
}

#define PR_SEED_E 16                                     // values per thread and chunk: C3's 15,625 blocks are one chunk
#define PR_LIST (16 * PR_SEED)                           // pairs in the workgroup's list

// The PR_SEED blocks with the smallest bmin below +inf (fewer if fewer have an admissible row), ascending by (value,
// block number).  One workgroup, one pass over bmin in chunks of PR_SEED_E x 1024 values, a thread's strided share of a
// chunk in registers, nothing sorted, no scratch:
//   * filter.  The smallest pair of each of the 16 wavefronts are 16 different pairs, so the PR_SEED-th smallest of all
//     is not above the largest of them, tau (+inf while a wavefront has no value below +inf); tau only falls from chunk
//     to chunk.  The pairs <= tau go to a list in LDS: about 50 of C3's 15,625 values.
//   * rank.  A pair's place in the result is the number of listed pairs below it; thread t counts for pair t.
//   * a list that overflows (values in an order that defeats the filter; a wavefront's whole share at +inf) is
//     dropped: every wavefront selects the PR_SEED smallest of what its lanes hold, chunk after chunk (from the second
//     on only values below its PR_SEED-th so far enter), and the list is the 16 wavefronts' results.
__global__ __launch_bounds__(1024) void prune_seed_kernel(const double* bmin, long long ncb, long long* seeds,
                                                          long long* counts) {
    __shared__ double sv[PR_LIST], wv[16];
    __shared__ long long si[PR_LIST], wi[16];
    __shared__ int cnt, nsel;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) { cnt = 0; nsel = 0; }
    double tv = INFINITY;                                // tau: (+inf, PR_NONE) is above every pair
    long long ti = PR_NONE;
    for (long long base = 0; base < ncb; base += PR_SEED_E * 1024) {
        double lv[PR_SEED_E], hv = INFINITY;
        long long hp = PR_NONE;
#pragma unroll
        for (int j = 0; j < PR_SEED_E; ++j) {
            const long long p = base + tid + 1024 * j;
            const double v = p < ncb ? bmin[p] : INFINITY;
            lv[j] = v < INFINITY ? v : INFINITY;         // (a NaN is not below +inf)
            if (lv[j] < hv) { hv = lv[j]; hp = p; }      // p ascends with j: the lowest block number on ties
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(hv, o);
            const long long op = __shfl_xor(hp, o);
            if (pr_less(ov, op, hv, hp)) { hv = ov; hp = op; }
        }
        __syncthreads();                                 // (the previous chunk's minima have been read)
        if (lane == 0) { wv[w] = hv; wi[w] = hp; }
        __syncthreads();
        double cv = wv[0];
        long long ci = wi[0];
#pragma unroll
        for (int i = 1; i < 16; ++i)
            if (pr_less(cv, ci, wv[i], wi[i])) { cv = wv[i]; ci = wi[i]; }
        if (pr_less(cv, ci, tv, ti)) { tv = cv; ti = ci; }
#pragma unroll
        for (int j = 0; j < PR_SEED_E; ++j) {
            const long long p = base + tid + 1024 * j;
            if (lv[j] < INFINITY && !pr_less(tv, ti, lv[j], p)) {
                const int slot = atomicAdd(&cnt, 1);
                if (slot < PR_LIST) { sv[slot] = lv[j]; si[slot] = p; }
            }
        }
    }
    __syncthreads();
    int n = cnt;
    if (n > PR_LIST) {
        double lv[PR_SEED_E + 1], mv = INFINITY;
        long long li[PR_SEED_E + 1], mi = PR_NONE;
        for (long long base = 0; base < ncb; base += PR_SEED_E * 1024) {
            const double qv = __shfl(mv, PR_SEED - 1);   // the wavefront's PR_SEED-th so far (+inf, PR_NONE: none yet)
            const long long qi = __shfl(mi, PR_SEED - 1);
            bool any = false;
#pragma unroll
            for (int j = 0; j < PR_SEED_E; ++j) {
                const long long p = base + tid + 1024 * j;
                const double v = p < ncb ? bmin[p] : INFINITY;
                const bool in = v < INFINITY && pr_less(v, p, qv, qi);
                lv[j] = in ? v : INFINITY; li[j] = in ? p : PR_NONE;
                any |= in;
            }
            if (!__any(any)) continue;
            lv[PR_SEED_E] = mv; li[PR_SEED_E] = mi;
            pr_wave_select(lv, li, mv, mi);
        }
        if (lane < PR_SEED) { sv[w * PR_SEED + lane] = mv; si[w * PR_SEED + lane] = mi; }
        n = PR_LIST;
        __syncthreads();
    }
    if (tid < n && si[tid] != PR_NONE) {
        const double v = sv[tid];
        const long long p = si[tid];
        int rank = 0;
        for (int e = 0; e < n; ++e) rank += pr_less(sv[e], si[e], v, p) ? 1 : 0;
        if (rank < PR_SEED) { seeds[rank] = p; atomicAdd(&nsel, 1); }
    }
    __syncthreads();
    if (tid == 0) { counts[0] = nsel; counts[1] = 0; counts[3] = 0; }
}

// tau = the smallest utility the seed blocks found (part_u of the seeds; tau_in if part_u == NULL: a planted
// value, apgp_sweep_prune_select); survivors = blocks with an admissible row (bmin < +inf), bmin <= tau, not a seed --
// written in ascending order (each thread a contiguous range, a scan over the threads' counts), count to counts[1] and,
// if given, to *count2.
__global__ __launch_bounds__(1024) void prune_select_kernel(const double* bmin, long long ncb, const long long* seeds,
                                                            long long* counts, const double* part_u, double tau_in,
                                                            long long* list, long long* count2) {
    __shared__ long long sd[PR_SEED];
    __shared__ long long cnt[1024];
    const int t = threadIdx.x;
    const int ns = (int)counts[0];
    if (t < PR_SEED) sd[t] = t < ns ? seeds[t] : -1;
    __syncthreads();
    double tau = tau_in;
    if (part_u) {
        tau = INFINITY;
        for (int i = 0; i < ns; ++i) tau = fmin(tau, part_u[sd[i]]);      // (fmin: a NaN partial never lowers tau)
    }
    auto keep = [&](long long p) {
        const double v = bmin[p];
        if (!(v < INFINITY && v <= tau)) return false;
        for (int i = 0; i < ns; ++i)
            if (sd[i] == p) return false;
        return true;
    };
    const long long per = (ncb + 1023) / 1024;
    const long long p0 = (long long)t * per, p1 = p0 + per < ncb ? p0 + per : ncb;
    long long c = 0;
    for (long long p = p0; p < p1; ++p) c += keep(p) ? 1 : 0;
    cnt[t] = c;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // inclusive scan
        const long long add = t >= o ? cnt[t - o] : 0;
        __syncthreads();
        cnt[t] += add;
        __syncthreads();
    }
    long long pos = cnt[t] - c;
    for (long long p = p0; p < p1; ++p)
        if (keep(p)) list[pos++] = p;
    if (t == 1023) {
        counts[1] = cnt[1023];
        counts[2] = __double_as_longlong(tau);
        if (count2) *count2 = cnt[1023];
    }
}

static int g_sweep_prune = 1;

extern "C" int apgp_set_sweep_prune(int v) {
    const int old = __atomic_exchange_n(&g_sweep_prune, v < 0 ? 0 : v, __ATOMIC_RELAXED);
    return old;
}

extern "C" int apgp_get_sweep_prune(void) { return __atomic_load_n(&g_sweep_prune, __ATOMIC_RELAXED); }

static inline long long pr_ncb(int64_t m) { return (m + SW_CAND - 1) / SW_CAND; }
// doubles of the full sweep's scratch (the layout below up to the row-block shares)
static inline long long s2_work_len(int64_t m, int64_t n) {
    const long long ncb = pr_ncb(m);
    const long long slots = ncb < SW_GRID ? ncb : SW_GRID;
    return 2 * ncb + slots * s2_ncache(n) * SW_BCH + 2 * (long long)S2_SPLIT_MAX * SW_CAND * s2_nrb(n);
}

extern "C" int64_t apgp_sweep_prune_counts_offset(int64_t m, int64_t n) {
    if (m < 1 || n < 1 || m > APGP_MAX_M || n > APGP_MAX_N) return -1;
    return s2_work_len(m, n) + 2 * pr_ncb(m) + PR_SEED;
}

extern "C" int apgp_sweep_prune_select(const double* bmin, int64_t ncb, const int64_t* seeds, int64_t* counts,
                                       double tau, int64_t* list, void* stream) {
    APGP_CHECK_ARG(bmin && seeds && counts && list, "null pointer");
    APGP_CHECK_ARG(ncb >= 1 && ncb <= APGP_MAX_M / SW_CAND, "ncb >= 1 required");
    hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, bmin, (long long)ncb,
                       (const long long*)seeds, (long long*)counts, (const double*)NULL, tau, (long long*)list,
                       (long long*)NULL);
    APGP_CHECK_LAUNCH();
    return 0;
}

// the kinds of stream the entry points take: the sign-sorted one cannot be left out (no kernel sorts rows per call)
static inline bool pr_rows_kind_ok(const void* prune_rows, int rows_kind) {
    return rows_kind == APGP_PRUNE_ROWS_SPLIT || (rows_kind == APGP_PRUNE_ROWS_SIGNED && prune_rows != NULL);
}

// the one place that fills a PruneArgs.  Kern: a KernConst, or an argument struct that apgp_fill_kernel has filled;
// lo, hi: the box in the caller's coordinates, or NULL both
template <class Kern>
static PruneArgs pr_args(const double* T, int64_t m, const double* xs, int64_t n, const uint8_t* mask, const Kern& kern,
                         double mean, int32_t kind, const double* lo, const double* hi, double zeta, double ybest,
                         double* bmin, double* part_u, long long* part_i, const void* prune_rows, int rows_kind) {
    PruneArgs p;
    p.T = T; p.xs = xs; p.mask = mask; p.bmin = bmin; p.part_u = part_u; p.part_i = part_i;
    p.m = m; p.ncb = pr_ncb(m); p.n = n;
    p.kind = kind; p.mean = mean; p.zeta = zeta; p.ybest = ybest;
    apgp_fill_kernel(p, kern);
    apgp_fill_box(p, p.ndim, lo, hi);
    p.blk_list = NULL; p.blk_count = NULL; p.est = NULL; p.prune_rows = prune_rows; p.rows_kind = rows_kind;
    return p;
}

// the bound pass over all blocks: coarse (fp32 kernel values; pure squared-exponential kernels only) or fp64.  Coarse up to
// Dpad = 8: the exponents on the matrix cores (prune_mm32.h), and the vector-ALU kernel behind it for the blocks whose
// gate failed there -- as a rule none, and its workgroups leave at once.  Dpad 16 and 32 keep the vector-ALU kernel.
// With PruneArgs::prune_rows the matrix-core kernel copies the pre-split rows instead of splitting them (same bits), or,
// with rows_kind = APGP_PRUNE_ROWS_SIGNED, the sign-sorted rows, and runs one chain per kernel value (other last bits).
// With PruneArgs::blk_list (fp64 only): the refine stage, over the blocks of that list; the launch is sized for all blocks.
template <int DPAD>
static void launch_bound(const PruneArgs& p, hipStream_t s, bool coarse) {
    // cpt candidate blocks per wavefront
    auto grid_of = [&](int cpt) { return dim3((unsigned)((p.ncb + (PR_THREADS / 64) * cpt - 1) / ((PR_THREADS / 64) * cpt))); };
    const dim3 grid = grid_of(coarse ? pr32_cpt(DPAD) : PR_CPT);
    if (coarse) {
        if constexpr (DPAD <= 8) {
            const dim3 mm_grid = grid_of(PMM_G / 2);
            if (p.prune_rows && p.rows_kind == APGP_PRUNE_ROWS_SIGNED && apgp_get_prune_pipe())
                hipLaunchKernelGGL((prune_bound_mm32_kernel<DPAD, true, true, true>), mm_grid, dim3(PR_THREADS), 0, s, p);
            else if (p.prune_rows && p.rows_kind == APGP_PRUNE_ROWS_SIGNED)
                hipLaunchKernelGGL((prune_bound_mm32_kernel<DPAD, true, true>), mm_grid, dim3(PR_THREADS), 0, s, p);
            else if (p.prune_rows)
                hipLaunchKernelGGL((prune_bound_mm32_kernel<DPAD, true>), mm_grid, dim3(PR_THREADS), 0, s, p);
            else
                hipLaunchKernelGGL((prune_bound_mm32_kernel<DPAD, false>), mm_grid, dim3(PR_THREADS), 0, s, p);
            hipLaunchKernelGGL((prune_bound32_kernel<DPAD, true>), grid, dim3(PR_THREADS), 0, s, p);
        } else {
            hipLaunchKernelGGL((prune_bound32_kernel<DPAD, false>), grid, dim3(PR_THREADS), 0, s, p);
        }
    } else if (p.blk_list)
        hipLaunchKernelGGL((prune_bound_kernel<DPAD, true>), grid, dim3(PR_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL((prune_bound_kernel<DPAD, false>), grid, dim3(PR_THREADS), 0, s, p);
}

// 1. bound over all blocks (coarse if the kernel allows)  2. seeds  3. sweep on the seeds -> tau  4. select: list A
// (counts[3])  5. fp64 bound on list A, bmin = max of the two  6. select again: list B (counts[1]), written over list A
// 7. sweep on list B.  With a LinearKernel term steps 5 and 6 fall away: list A is list B.
// After a coarse stage the seeds are the blocks with the smallest b WITHOUT slack (PruneArgs::est): where the fp32 slack
// exceeds the spread of the bounds (an ill-conditioned fit: sum |alpha| is huge against the spread of mu) the bounds
// themselves order the blocks by little more than |t - c|, the seeds would be arbitrary and tau prune nothing.
template <int DPAD>
static int launch_pruned(const SweepArgs& a, hipStream_t s, bool solve, void* part, const void* prune_rows,
                         int rows_kind) {
    const int rc = s2_prepare_device<DPAD>();
    if (rc != 0) return rc;
    const long long ncb = pr_ncb(a.m);
    double* bmin = (double*)part + s2_work_len(a.m, a.n);
    long long* list = (long long*)(bmin + ncb);
    long long* seeds = list + ncb;
    long long* counts = seeds + PR_SEED;
    const bool coarse = a.lin_coef == 0.0;
    PruneArgs p = pr_args(a.T, a.m, a.xs, a.n, a.mask, a, a.mean, a.kind, a.has_box ? a.lo : NULL, a.has_box ? a.hi : NULL,
                          a.zeta, a.ybest, bmin, a.part_u, a.part_i, prune_rows, rows_kind);
    if (coarse) p.est = (double*)(counts + 8);
    launch_bound<DPAD>(p, s, coarse);
    hipLaunchKernelGGL(prune_seed_kernel, dim3(1), dim3(1024), 0, s, coarse ? (const double*)p.est : (const double*)bmin, ncb,
                       seeds, counts);
    // (counts[4], the second-wave seeds swept: the split seed route's first finish resets it; no waves elsewhere)
    if (solve || s2_nrb(a.n) < 2 || a.sp_q == NULL) (void)hipMemsetAsync(counts + 4, 0, sizeof(long long), s);
    launch_sweep_list<DPAD>(a, s, solve, seeds, counts, ncb < PR_SEED ? ncb : PR_SEED, PR_SEED, true);
    hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(1024), 0, s, bmin, ncb, seeds, counts, a.part_u, 0.0, list,
                       counts + 3);
    if (coarse) {
        p.blk_list = list; p.blk_count = counts + 3;
        launch_bound<DPAD>(p, s, false);
        hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(1024), 0, s, bmin, ncb, seeds, counts, a.part_u, 0.0, list,
                           (long long*)NULL);
    }
    launch_sweep_list<DPAD>(a, s, solve, list, counts + 1, ncb, S2_SPLIT_MAX);
    return 0;
}

// Layout of the caller's scratch (doubles): [2 ncb arg-min partials | slots x ncache x SW_BCH
// parked operands | 2 x S2_SPLIT_MAX x SW_CAND x nrb row-block shares of the split last round (s2_work_len up to
// here) | pruned sweep: ncb block bounds bmin | ncb surviving block numbers | PR_SEED seed block numbers | 8 words:
// seed count, survivor count, bit pattern of tau, blocks the coarse bound kept (list A; list B is written over it),
// second-wave seeds swept | ncb block minima of the coarse stage's b without slack | PR_SEED x nrb x (S2_HQ_PRE +
// S2_HQ_ACC) fold inputs of the seed launches' row-part items (from pr_work_len, an even offset: 16-byte accesses;
// n > S2_ROWS only)]
static_assert(S2_PRUNE_WORDS == PR_SEED + 8, "the fold inputs start behind the seed numbers and the counters");
static inline long long pr_work_len(int64_t m, int64_t n) {       // (sp_q lies 2 S2_SPLIT_MAX SW_CAND nrb before s2_work_len)
    return s2_work_len(m, n) - 2ll * S2_SPLIT_MAX * SW_CAND * s2_nrb(n) + s2_fold_off(s2_nrb(n), pr_ncb(m));
}

extern "C" int64_t apgp_acquire_work_len(int64_t m, int64_t n) {
    if (m < 1 || n < 1) return 0;
    if (m > APGP_MAX_M || n > APGP_MAX_N) return -1;
    return pr_work_len(m, n) + (s2_nrb(n) >= 2 ? (long long)PR_SEED * s2_nrb(n) * (S2_HQ_PRE + S2_HQ_ACC) : 0);
}

static int acquire_impl(bool solve, const double* T, int64_t m, int64_t idx_offset, const double* packed_linv,
                        const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                        int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                        double zeta, double ybest, double* mu, double* var, double* u, void* part,
                        apgp_best_t* best, const void* prune_rows, int rows_kind, void* stream) {
    APGP_CHECK_ARG(T && packed_linv && xs && kern, "null pointer");
    APGP_CHECK_ARG(pr_rows_kind_ok(prune_rows, rows_kind), "rows_kind: SPLIT, or SIGNED with its stream");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M && n >= 1 && n <= APGP_MAX_N, "m >= 1 and n >= 1 required");
    APGP_CHECK_ARG(kind >= APGP_UTIL_AGP && kind <= APGP_UTIL_NONE, "unknown utility kind");
    APGP_CHECK_ARG(kind == APGP_UTIL_NONE || best, "best required for an acquisition");
    APGP_CHECK_ARG(part || (kind == APGP_UTIL_NONE && n <= S2_ROWS),
                   "part (apgp_acquire_work_len doubles) required");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    SweepArgs a;
    a.T = T; a.linv = packed_linv; a.xs = xs; a.mask = mask;
    a.mu = mu; a.var = var; a.u = u;
    const long long nblk = (m + SW_CAND - 1) / SW_CAND;
    const long long slots = nblk < SW_GRID ? nblk : SW_GRID;
    a.part_u = (double*)part;
    a.part_i = part ? (long long*)((double*)part + nblk) : NULL;
    a.ncache = (int)s2_ncache(n);
    // N <= 256: nothing is parked; the descriptor then points at the factor (never dereferenced)
    a.kcache = a.ncache > 0 ? (double*)part + 2 * nblk : (double*)packed_linv;
    // row-block shares of the split last round (after the parked-operand slots)
    a.sp_q = part ? (double*)part + 2 * nblk + slots * s2_ncache(n) * SW_BCH : NULL;
    a.sp_mu = a.sp_q ? a.sp_q + (long long)S2_SPLIT_MAX * SW_CAND * s2_nrb(n) : NULL;
    a.blk_begin = 0; a.blk_end = nblk; a.split = 0;
    {
        const long long wb = apgp_packed_linv_len(n) * 8, xb = apgp_packed_train_len(n, kc.ndim) * 8;
        const long long kb = (long long)(a.ncache > 0 ? a.ncache : 1) * SW_BCH * 8;
        APGP_CHECK_ARG(wb < (1ll << 31) && kb < (1ll << 31), "n too large for the sweep's 32-bit stream offsets");
        a.linv_bytes = (unsigned)wb; a.xs_bytes = (unsigned)xb; a.kslot_bytes = (unsigned)kb;
    }
    a.m = m; a.idx_offset = idx_offset;
    a.nrb = s2_nrb(n); a.kind = kind; a.n = (int)n;
    a.mean = mean; a.zeta = zeta; a.ybest = ybest;
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    a.blk_list = NULL; a.blk_count = NULL; a.list_lo = 0; a.list_hi = 0;
    hipStream_t s = (hipStream_t)stream;
    // the pruned arg-min: only the winner is asked for (mu / var / u per candidate need the full sweep), the switch
    // is on and m is large enough to pay for the bound pass (switch value >= 2: that value is the threshold)
    const int pr_mode = apgp_get_sweep_prune();
    const bool prune = pr_mode > 0 && kind != APGP_UTIL_NONE && !mu && !var && !u && part &&
                       m >= (pr_mode == 1 ? pr_min_m(n) : (int64_t)pr_mode);
    const int rc = apgp_by_dpad(kc.dpad, [&](auto dp) {
        return prune ? launch_pruned<decltype(dp)::value>(a, s, solve, part, prune_rows, rows_kind)
                     : launch_sweep<decltype(dp)::value>(a, s, solve);
    });
    if (rc != 0) return rc;
    if (kind != APGP_UTIL_NONE)
        hipLaunchKernelGGL(argmin_final_kernel, dim3(1), dim3(1024), 0, s, a.part_u, a.part_i, nblk, best);
    APGP_CHECK_LAUNCH();
    return 0;
}

extern "C" int apgp_acquire(const double* T, int64_t m, int64_t idx_offset, const double* packed_linv,
                            const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                            int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                            double zeta, double ybest, double* mu, double* var, double* u, void* part,
                            apgp_best_t* best, void* stream) {
    return acquire_impl(false, T, m, idx_offset, packed_linv, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, NULL, APGP_PRUNE_ROWS_SPLIT, stream);
}

// apgp_acquire with the fit's pre-split rows of the coarse bound (apgp_pack_prune_rows; NULL: apgp_acquire itself)
extern "C" int apgp_acquire_rows(const double* T, int64_t m, int64_t idx_offset, const double* packed_linv,
                                 const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                 int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                 double zeta, double ybest, double* mu, double* var, double* u, void* part,
                                 apgp_best_t* best, const void* prune_rows, void* stream) {
    return acquire_impl(false, T, m, idx_offset, packed_linv, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, prune_rows, APGP_PRUNE_ROWS_SPLIT, stream);
}

// apgp_acquire_rows with the kind of its stream (APGP_PRUNE_ROWS_*)
extern "C" int apgp_acquire_rows2(const double* T, int64_t m, int64_t idx_offset, const double* packed_linv,
                                  const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                  int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                  double zeta, double ybest, double* mu, double* var, double* u, void* part,
                                  apgp_best_t* best, const void* prune_rows, int32_t rows_kind, void* stream) {
    return acquire_impl(false, T, m, idx_offset, packed_linv, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, prune_rows, rows_kind, stream);
}

// Test hooks of the pruned arg-min (include/apgp.h): one bound pass over all blocks into the caller's buffer, and the
// seed step alone.
// The coarse bound's training rows split into bf16 parts, once per fit (prune_mm32.h: pmm_pack_rows_kernel).  Doubles:
// the 16-byte header and per PMM_ROWS-row tile the LDS image and the alphas; 0 where the coarse bound does not use it.
extern "C" int64_t apgp_prune_rows_len(int64_t n, int32_t ndim) {
    if (n < 0 || n > APGP_MAX_N || ndim < 1 || ndim > APGP_MAX_DIM) return -1;
    const int dpad = apgp_dpad(ndim);
    if (n == 0 || dpad > 8) return 0;
    const int64_t ntile = (n + PMM_ROWS - 1) / PMM_ROWS;
    return apgp_by_dpad(dpad, [&](auto dp) -> int64_t {
        if constexpr (decltype(dp)::value <= 8) return 2 + ntile * 2 * PmmShape<decltype(dp)::value>::PIECES;
        else return 0;
    });
}

extern "C" int apgp_pack_prune_rows(const double* xs, int64_t n, const apgp_kernel_t* kern, void* rows, void* stream) {
    APGP_CHECK_ARG(xs && kern && rows, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "n >= 1 required");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(kc.dpad <= 8, "no pre-split rows beyond 8 dimensions (apgp_prune_rows_len is 0)");
    apgp_by_dpad(kc.dpad, [&](auto dp) {
        if constexpr (decltype(dp)::value <= 8)
            hipLaunchKernelGGL(pmm_pack_rows_kernel<decltype(dp)::value>, dim3(1), dim3(PR_THREADS), 0, (hipStream_t)stream,
                               xs, (long long)n, (unsigned char*)rows);
    });
    APGP_CHECK_LAUNCH();
    return 0;
}

// The same rows sorted by alpha's sign (prune_mm32.h: pmm_pack_srows_kernel).  Doubles: the 32-byte header and
// pmm_stiles(n) tiles, room for any split of the n rows into the two classes.
extern "C" int64_t apgp_prune_srows_len(int64_t n, int32_t ndim) {
    if (n < 0 || n > APGP_MAX_N || ndim < 1 || ndim > APGP_MAX_DIM) return -1;
    const int dpad = apgp_dpad(ndim);
    if (n == 0 || dpad > 8) return 0;
    return apgp_by_dpad(dpad, [&](auto dp) -> int64_t {
        if constexpr (decltype(dp)::value <= 8)
            return PMM_SHDR / 8 + pmm_stiles(n) * 2 * PmmShape<decltype(dp)::value>::PIECES;
        else return 0;
    });
}

extern "C" int apgp_pack_prune_srows(const double* xs, int64_t n, const apgp_kernel_t* kern, void* rows, void* stream) {
    APGP_CHECK_ARG(xs && kern && rows, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N, "n >= 1 required");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    APGP_CHECK_ARG(kc.dpad <= 8, "no sign-sorted rows beyond 8 dimensions (apgp_prune_srows_len is 0)");
    apgp_by_dpad(kc.dpad, [&](auto dp) {
        if constexpr (decltype(dp)::value <= 8)
            hipLaunchKernelGGL(pmm_pack_srows_kernel<decltype(dp)::value>, dim3(1), dim3(PR_THREADS), 0, (hipStream_t)stream,
                               xs, (long long)n, (unsigned char*)rows);
    });
    APGP_CHECK_LAUNCH();
    return 0;
}

// (who: the entry point's name, which the refusals of apgp_prune_bounds have always carried)
static int prune_bounds_impl(const char* who, const double* T, int64_t m, const double* xs, int64_t n,
                             const apgp_kernel_t* kern, double mean, int32_t kind, const double* lo, const double* hi,
                             const uint8_t* mask, double zeta, double ybest, int coarse, double* bmin_out,
                             const void* prune_rows, int rows_kind, double* est_out, void* stream) {
#define PB_CHECK_ARG(cond, msg)                                     \
    do {                                                            \
        if (!(cond)) {                                              \
            apgp_set_error("%s: bad argument: %s", who, msg);       \
            return -1;                                              \
        }                                                           \
    } while (0)
    PB_CHECK_ARG(T && xs && kern && bmin_out, "null pointer");
    PB_CHECK_ARG(m >= 1 && m <= APGP_MAX_M && n >= 1 && n <= APGP_MAX_N, "m >= 1 and n >= 1 required");
    PB_CHECK_ARG(kind >= APGP_UTIL_AGP && kind < APGP_UTIL_NONE, "unknown utility kind");
    PB_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    PB_CHECK_ARG(pr_rows_kind_ok(prune_rows, rows_kind), "rows_kind: SPLIT, or SIGNED with its stream");
    KernConst kc;
    PB_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    PB_CHECK_ARG(!coarse || kc.lin_coef == 0.0, "the coarse bound takes pure squared-exponential kernels only");
#undef PB_CHECK_ARG
    PruneArgs p = pr_args(T, m, xs, n, mask, kc, mean, kind, lo, hi, zeta, ybest, bmin_out, NULL, NULL, prune_rows, rows_kind);
    if (coarse) p.est = est_out;                         // (the fp64 bound has no use for it)
    hipStream_t s = (hipStream_t)stream;
    apgp_by_dpad(kc.dpad, [&](auto dp) { launch_bound<decltype(dp)::value>(p, s, coarse != 0); });
    APGP_CHECK_LAUNCH();
    return 0;
}

extern "C" int apgp_prune_bounds(const double* T, int64_t m, const double* xs, int64_t n, const apgp_kernel_t* kern,
                                 double mean, int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                 double zeta, double ybest, int coarse, double* bmin_out, void* stream) {
    return prune_bounds_impl(__func__, T, m, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest, coarse, bmin_out, NULL,
                             APGP_PRUNE_ROWS_SPLIT, NULL, stream);
}

extern "C" int apgp_prune_bounds_rows(const double* T, int64_t m, const double* xs, int64_t n, const apgp_kernel_t* kern,
                                      double mean, int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                      double zeta, double ybest, int coarse, double* bmin_out, const void* prune_rows,
                                      void* stream) {
    return prune_bounds_impl(__func__, T, m, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest, coarse, bmin_out,
                             prune_rows, APGP_PRUNE_ROWS_SPLIT, NULL, stream);
}

extern "C" int apgp_prune_bounds_rows2(const double* T, int64_t m, const double* xs, int64_t n, const apgp_kernel_t* kern,
                                       double mean, int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                       double zeta, double ybest, int coarse, double* bmin_out, const void* prune_rows,
                                       int32_t rows_kind, double* est_out, void* stream) {
    return prune_bounds_impl(__func__, T, m, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest, coarse, bmin_out,
                             prune_rows, rows_kind, est_out, stream);
}

extern "C" int apgp_sweep_prune_seeds(const double* bmin, int64_t ncb, int64_t* seeds, int64_t* counts, void* stream) {
    APGP_CHECK_ARG(bmin && seeds && counts, "null pointer");
    APGP_CHECK_ARG(ncb >= 1 && ncb <= APGP_MAX_M / SW_CAND, "ncb >= 1 required");
    hipLaunchKernelGGL(prune_seed_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, bmin, (long long)ncb,
                       (long long*)seeds, (long long*)counts);
    APGP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// Substitution form of the sweep: sigma^2 = amp - |v|^2 with v = L^-1 k* by BLOCKED FORWARD
// SUBSTITUTION against the factor itself (what george's cho_solve does, utility.py:131,178,224)
// instead of a product with the explicit inverse -- the only trustworthy formulation once
// cond(K) approaches 1e16 (the reference's own fitAmp=True optimum), and
// the same matrix-core stream otherwise: sweep2_kernel<.., SOLVE = true> reads the tiles of
// apgp_pack_lsolve (-L off the diagonal 16 x 16 blocks, those blocks prepared for a 4 x 4-blocked
// in-register solve), its B operands are the solved blocks V_j parked by the matrix wavefronts,
// and k* enters once per 16-row block.  No n limit beyond the inverse form's.
// ---------------------------------------------------------------------------
extern "C" int apgp_acquire_solve(const double* T, int64_t m, int64_t idx_offset, const double* packed_lsolve,
                                  const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                  int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                  double zeta, double ybest, double* mu, double* var, double* u, void* part,
                                  apgp_best_t* best, void* stream) {
    return acquire_impl(true, T, m, idx_offset, packed_lsolve, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, NULL, APGP_PRUNE_ROWS_SPLIT, stream);
}

extern "C" int apgp_acquire_solve_rows(const double* T, int64_t m, int64_t idx_offset, const double* packed_lsolve,
                                       const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                       int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                       double zeta, double ybest, double* mu, double* var, double* u, void* part,
                                       apgp_best_t* best, const void* prune_rows, void* stream) {
    return acquire_impl(true, T, m, idx_offset, packed_lsolve, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, prune_rows, APGP_PRUNE_ROWS_SPLIT, stream);
}

extern "C" int apgp_acquire_solve_rows2(const double* T, int64_t m, int64_t idx_offset, const double* packed_lsolve,
                                        const double* xs, int64_t n, const apgp_kernel_t* kern, double mean,
                                        int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                        double zeta, double ybest, double* mu, double* var, double* u, void* part,
                                        apgp_best_t* best, const void* prune_rows, int32_t rows_kind, void* stream) {
    return acquire_impl(true, T, m, idx_offset, packed_lsolve, xs, n, kern, mean, kind, lo, hi, mask, zeta, ybest,
                        mu, var, u, part, best, prune_rows, rows_kind, stream);
}

// ---------------------------------------------------------------------------
// Fantasy pass of a batch (apgp_acquire_fantasy; DESIGN.md "Batch design points").  Conditioning on
// x_j at y = mu(x_j) lowers every candidate's variance by C_j(t)^2 with
//   C_j(t) = (k(t, x_j) - k(t, X).beta_j - sum_{i<j} C_i(t) C_i(x_j)) / sqrt(s_j),
// which costs what a mean-only prediction costs (beta_j in place of alpha): O(N D) per candidate
// against the sweep's O(N^2).
// One thread per candidate, FT_THREADS candidates per workgroup: the candidate's scaled coordinates
// and its running k(t, X).beta stay in registers; the training rows and beta are staged through LDS
// in tiles of FT_ROWS rows shared by the workgroup (all lanes of a wavefront read the same LDS words:
// broadcasts, no bank conflicts).  Four rows per step feed apgp_exp4 (four independent fp64 chains)
// into four partial sums.  The epilogue holds k(t, x_j), the downdate by the earlier columns, the
// column store, v_j, the sweep's utility and gate, and the workgroup's arg-min partial.
// ---------------------------------------------------------------------------
#define FT_THREADS 256
#define FT_ROWS 128        // training rows per LDS tile (divides the packed stream's 512-row padding)

struct FantasyArgs {
    const double* T;
    const double* xs;
    const double* beta;
    double* C;
    const double* mu;
    const double* var_in;
    double* var_out;
    double* u;
    const unsigned char* mask;
    double* part_u;
    long long* part_i;
    long long m, idx_offset, ldc, pick_row, n;
    int ndim, j, kind, has_box, lin_order;
    double amp, diag_add, lin_coef, zeta, ybest;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM], lo[APGP_MAX_DIM], hi[APGP_MAX_DIM];
};

template <int DPAD>
__global__ __launch_bounds__(FT_THREADS) void fantasy_kernel(FantasyArgs a) {
    constexpr int XS = DPAD + 2;                 // packed stream row: scaled x | alpha | 0
    constexpr int PIECES = FT_ROWS * XS / 2;     // 16-byte pieces per tile
    __shared__ double etab[APGP_EXP_TAB_N];
    __shared__ __attribute__((aligned(16))) double tile[FT_ROWS * XS];   // scaled x | beta | 0
    __shared__ double cx[APGP_MAX_FANTASY];      // C_i(x_j), i < j
    __shared__ double su[FT_THREADS / 64];
    __shared__ long long si[FT_THREADS / 64];
    apgp_exp_tab_load(etab);
    const int tid = threadIdx.x;
    if (tid < a.j - 1) cx[tid] = a.C[(long long)tid * a.ldc + a.pick_row];
    const long long row = (long long)blockIdx.x * FT_THREADS + tid;
    const bool live = row < a.m;
    double tt[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) tt[d] = (live && d < a.ndim) ? a.T[row * a.ndim + d] * a.sc[d] : 0.0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const long long ntile = (a.n + FT_ROWS - 1) / FT_ROWS;
    for (long long ti = 0; ti < ntile; ++ti) {
        __syncthreads();                         // the previous tile has been consumed
        const long long r0 = ti * FT_ROWS;       // (rows < ntile * FT_ROWS <= npad: inside the packed stream)
        for (int e = tid; e < PIECES; e += FT_THREADS) {
            const int r = e / (XS / 2), p = e - r * (XS / 2);
            f64x2 v;
            if (p == DPAD / 2) {                 // the alpha slot carries beta; 0 on the padding rows
                v.x = (r0 + r < a.n) ? a.beta[r0 + r] : 0.0;
                v.y = 0.0;
            } else {
                v = *(const f64x2*)(a.xs + (r0 + r) * XS + 2 * p);
            }
            *(f64x2*)(tile + r * XS + 2 * p) = v;
        }
        __syncthreads();
        for (int r = 0; r < FT_ROWS; r += 4) {
            double ex[4], kv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* xr = tile + (r + q) * XS;
                double s = 0.0, s3 = 0.0;
#pragma unroll
                for (int d = 0; d < DPAD; d += 2) {
                    const double df0 = tt[d] - xr[d];
                    const double df1 = tt[d + 1] - xr[d + 1];
                    s = fma(df0, df0, s);
                    s3 = fma(df1, df1, s3);
                }
                ex[q] = -(s + s3);
            }
            apgp_exp4(ex, kv, etab);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* xr = tile + (r + q) * XS;
                double k = a.amp * kv[q];
                if (a.lin_coef != 0.0) {
                    double ls;
                    APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xr[d_] * a.lw[d_]);
                    k = fma(a.lin_coef, ls, k);
                }
                acc[q] = fma(k, xr[DPAD], acc[q]);
            }
        }
    }
    double bu = INFINITY;
    long long bi = -1;
    if (live) {
        double xj[DPAD];
#pragma unroll
        for (int d = 0; d < DPAD; ++d) xj[d] = d < a.ndim ? a.T[a.pick_row * a.ndim + d] * a.sc[d] : 0.0;
        double s = 0.0, s3 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            const double df0 = tt[d] - xj[d];
            const double df1 = tt[d + 1] - xj[d + 1];
            s = fma(df0, df0, s);
            s3 = fma(df1, df1, s3);
        }
        double kx = a.amp * apgp_exp(-(s + s3), etab);
        if (a.lin_coef != 0.0) {
            double ls;
            APGP_LIN_SUM(ls, DPAD, a.ndim, a.lin_order, tt[d_] * xj[d_] * a.lw[d_]);
            kx = fma(a.lin_coef, ls, kx);
        }
        double c = kx - ((acc[0] + acc[1]) + (acc[2] + acc[3]));
        for (int i = 0; i < a.j - 1; ++i) c = fma(-a.C[(long long)i * a.ldc + row], cx[i], c);
        const double ch = c / sqrt(a.var_in[a.pick_row] + a.diag_add);
        a.C[(long long)(a.j - 1) * a.ldc + row] = ch;
        const double v = fma(-ch, ch, a.var_in[row]);
        a.var_out[row] = v;
        bool adm = !(a.mask && a.mask[row] == 0);
        if (a.has_box)
            for (int d = 0; d < a.ndim; ++d) {
                const double x = a.T[row * a.ndim + d];
                if (!(x >= a.lo[d] && x <= a.hi[d])) adm = false;
            }
        // a row with a NaN coordinate is inadmissible, as in the sweep (a scaled coordinate is NaN where the coordinate is)
#pragma unroll
        for (int d = 0; d < DPAD; ++d)
            if (tt[d] != tt[d]) adm = false;
        const double uu = adm ? util_value(a.kind, a.mu[row], v, a.zeta, a.ybest) : INFINITY;
        if (a.u) a.u[row] = uu;
        best_merge(bu, bi, uu, a.idx_offset + row);
    }
    for (int o = 32; o > 0; o >>= 1) {
        double ou = __shfl_xor(bu, o);
        long long oi = __shfl_xor(bi, o);
        best_merge(bu, bi, ou, oi);
    }
    if ((tid & 63) == 0) { su[tid >> 6] = bu; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < FT_THREADS / 64; ++w) best_merge(bu, bi, su[w], si[w]);
        a.part_u[blockIdx.x] = bu;
        a.part_i[blockIdx.x] = bi;
    }
}

// Scratch: the arg-min partials of the fantasy pass's workgroups (value, index) -- 2 doubles each.
extern "C" int64_t apgp_acquire_fantasy_work_len(int64_t m) {
    if (m < 1) return 0;
    if (m > APGP_MAX_M) return -1;
    return 2 * ((m + FT_THREADS - 1) / FT_THREADS);
}

extern "C" int apgp_acquire_fantasy(const double* T, int64_t m, int64_t idx_offset, const double* xs, int64_t n,
                                    const apgp_kernel_t* kern, const double* beta, int64_t pick_row, int32_t j,
                                    double* C, int64_t ldc, const double* mu, const double* var_in, double* var_out,
                                    int32_t kind, const double* lo, const double* hi, const uint8_t* mask,
                                    double zeta, double ybest, double* u, void* part, apgp_best_t* best,
                                    void* stream) {
    APGP_CHECK_ARG(T && xs && kern && beta && C && mu && var_in && var_out && part && best, "null pointer");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M && n >= 1 && n <= APGP_MAX_N, "m >= 1 and n >= 1 required");
    APGP_CHECK_ARG((m + FT_THREADS - 1) / FT_THREADS < (1ll << 31), "m too large for one grid");
    APGP_CHECK_ARG(j >= 1 && j < APGP_MAX_FANTASY, "1 <= j < APGP_MAX_FANTASY required");
    APGP_CHECK_ARG(pick_row >= 0 && pick_row < m, "0 <= pick_row < m required");
    APGP_CHECK_ARG(ldc >= m, "ldc >= m required");
    APGP_CHECK_ARG(var_in + m <= var_out || var_out + m <= var_in, "var_in and var_out must not overlap");
    APGP_CHECK_ARG(kind >= APGP_UTIL_AGP && kind <= APGP_UTIL_JONES, "kind must be AGP, BAPE or JONES");
    APGP_CHECK_ARG((lo == NULL) == (hi == NULL), "lo and hi must be given together");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    FantasyArgs a;
    a.T = T; a.xs = xs; a.beta = beta; a.C = C; a.mu = mu; a.var_in = var_in; a.var_out = var_out; a.u = u;
    a.mask = mask;
    const long long nblk = (m + FT_THREADS - 1) / FT_THREADS;
    a.part_u = (double*)part;
    a.part_i = (long long*)((double*)part + nblk);
    a.m = m; a.idx_offset = idx_offset; a.ldc = ldc; a.pick_row = pick_row; a.n = n;
    a.j = j; a.kind = kind; a.diag_add = kc.diag_add; a.zeta = zeta; a.ybest = ybest;
    apgp_fill_kernel(a, kc);
    apgp_fill_box(a, kc.ndim, lo, hi);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(FT_THREADS);
    apgp_by_dpad(kc.dpad, [&](auto dp) { hipLaunchKernelGGL(fantasy_kernel<decltype(dp)::value>, grid, block, 0, s, a); });
    hipLaunchKernelGGL(argmin_final_kernel, dim3(1), dim3(1024), 0, s, a.part_u, a.part_i, nblk, best);
    APGP_CHECK_LAUNCH();
    return 0;
}

// Packed tiles of the substitution form, same geometry as apgp_trtri_pack's (512 x 16 tiles, MFMA
// A-fragment order, row block ib holds chunks 0 .. 32 (ib + 1) - 1):
//   * below the diagonal 16 x 16 block of a chunk: -L;
//   * sub-block slot of the diagonal block C itself (rows 16 C .. 16 C + 15 of chunk C): 256 doubles
//     Ts[(4 q + q') 16 + 4 i + k] = -L[16C+4q+i][16C+4q'+k] for q' < q, (L_qq)^-1[i][k] for q' = q, 0 above --
//     the 4 x 4 diagonal blocks are inverted by substitution with reciprocal pivots; rows / columns
//     past n are zero (so the padded rows of V are exact zeros).
// 4 x 4 is the largest diagonal block whose explicit inverse keeps the solve in cho_solve's error
// class at cond 8.5e15 (8 x 8: borderline, 16 x 16: 10-100x worse; tools/cond_blocking_study.py).
__global__ __launch_bounds__(256) void pack_lsolve_kernel(const double* L, long long ldl, long long n,
                                                          double* packed) {
    constexpr int CPB = APGP_ROW_BLOCK / APGP_K_CHUNK;
    const long long tile = blockIdx.x;
    long long ib = (long long)((sqrt(8.0 * (double)tile / CPB + 1.0) - 1.0) * 0.5);
    while (CPB * (ib + 1) * (ib + 2) / 2 <= tile) ++ib;
    while (CPB * ib * (ib + 1) / 2 > tile) --ib;
    const long long kc = tile - CPB * ib * (ib + 1) / 2;
    double* out = packed + tile * (long long)(APGP_ROW_BLOCK * APGP_K_CHUNK);
    const long long sdiag = kc - ib * CPB;                 // sub-block slot of the diagonal block (if in this tile)
    for (int e = threadIdx.x; e < APGP_ROW_BLOCK * APGP_K_CHUNK; e += 256) {
        const int s = e >> 8;
        double v = 0.0;
        if (s == sdiag) {
            const int f = e & 255, q = f >> 6, q2 = (f >> 4) & 3, i = (f >> 2) & 3, k = f & 3;
            const long long r0 = kc * APGP_K_CHUNK + 4 * q, c0 = kc * APGP_K_CHUNK + 4 * q2;
            if (q2 < q) {
                if (r0 + i < n) v = -L[(r0 + i) * ldl + c0 + k];
            } else if (q2 == q && k <= i && r0 + i < n) {
                // column k of the inverse of the 4 x 4 lower-triangular block, rows k .. i
                double x[4] = {0.0, 0.0, 0.0, 0.0};
                x[k] = 1.0 / L[(r0 + k) * ldl + r0 + k];
                for (int r = k + 1; r <= i; ++r) {
                    double sacc = 0.0;
                    for (int c = k; c < r; ++c) sacc = fma(L[(r0 + r) * ldl + r0 + c], x[c], sacc);
                    x[r] = -sacc * (1.0 / L[(r0 + r) * ldl + r0 + r]);
                }
                v = x[i];
            }
        } else {
            const int q = e & 1, lane = (e >> 1) & 63, kp = (e >> 7) & 1;
            const int kk = 2 * kp + q;
            const long long row = ib * APGP_ROW_BLOCK + 16 * s + (lane & 15);
            const long long col = kc * APGP_K_CHUNK + 4 * kk + (lane >> 4);
            if (row < n && (col >> 4) < (row >> 4)) v = -L[row * ldl + col];
        }
        out[e] = v;
    }
}

extern "C" int64_t apgp_packed_lsolve_len(int64_t n) { return apgp_packed_linv_len(n); }

extern "C" int apgp_pack_lsolve(const double* L, int64_t n, int64_t ldl, double* packed, void* stream) {
    APGP_CHECK_ARG(L && packed, "null pointer");
    APGP_CHECK_ARG(n >= 1 && n <= APGP_MAX_N && ldl >= n, "n >= 1 and ldl >= n required");
    const long long nrb = apgp_npad(n) / APGP_ROW_BLOCK;
    const long long ntiles = (APGP_ROW_BLOCK / APGP_K_CHUNK) * nrb * (nrb + 1) / 2;
    hipLaunchKernelGGL(pack_lsolve_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, L,
                       (long long)ldl, (long long)n, packed);
    APGP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// mean-only prediction: the batched ApproxPosterior._gpll (approx.py:178-180).
// One wavefront per candidate; lanes stride over the training points.
// ---------------------------------------------------------------------------
struct MeanArgs {
    const double* T;
    const double* xs;
    double* mu;
    long long m, npad;
    int ndim, lin_order;
    double mean, amp, lin_coef;
    double sc[APGP_MAX_DIM], lw[APGP_MAX_DIM];
};

template <int DPAD>
__global__ __launch_bounds__(256) void predict_mean_kernel(MeanArgs a) {
    constexpr int XS = DPAD + 2;
    __shared__ double etab[APGP_EXP_TAB_N];
    apgp_exp_tab_load(etab);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + w;
    if (row >= a.m) return;
    double tt[DPAD];
#pragma unroll
    for (int d = 0; d < DPAD; ++d) tt[d] = d < a.ndim ? a.T[row * a.ndim + d] * a.sc[d] : 0.0;
    double acc = 0.0;
    for (long long k = lane; k < a.npad; k += 64) {
        const double* xr = a.xs + k * XS;
        double s = 0.0, s3 = 0.0;
#pragma unroll
        for (int d = 0; d < DPAD; d += 2) {
            double df0 = tt[d] - xr[d];
            double df1 = tt[d + 1] - xr[d + 1];
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
    bool bad = false;
    for (int d = 0; d < DPAD; ++d) bad = bad || (tt[d] != tt[d]);
    if (lane == 0) a.mu[row] = bad ? NAN : acc + a.mean;
}

extern "C" int apgp_predict_mean(const double* T, int64_t m, const double* xs, int64_t n,
                                 const apgp_kernel_t* kern, double mean, double* mu, void* stream) {
    APGP_CHECK_ARG(T && xs && kern && mu, "null pointer");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M && n >= 1 && n <= APGP_MAX_N, "m >= 1 and n >= 1 required");
    KernConst kc;
    APGP_CHECK_ARG(apgp_make_kernconst(kern, &kc) == 0, "kernel parameters");
    MeanArgs a;
    a.T = T; a.xs = xs; a.mu = mu; a.m = m; a.npad = apgp_npad(n); a.mean = mean;
    apgp_fill_kernel(a, kc);
    dim3 grid((unsigned)((m + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    apgp_by_dpad(kc.dpad, [&](auto dp) { hipLaunchKernelGGL(predict_mean_kernel<decltype(dp)::value>, grid, block, 0, s, a); });
    APGP_CHECK_LAUNCH();
    return 0;
}

// Host-buffer form of apgp_predict_mean for the latency-bound caller: an ensemble
// sampler's half-step evaluates a few dozen points per call (approx.py:178-180 through
// emcee), 4e4 calls per chain.  One entry point; round 3: the points are staged in -- and
// the means written to -- a pinned, device-mapped area of the stream that the kernel reads
// and writes in place, and a one-thread kernel behind it posts the sequence word the host
// polls: no H2D / D2H copy, no stream synchronisation (without pinned memory: the copies
// through `work` and one synchronisation, as in round 2).
__global__ void mailbox_post_kernel(double* mail, long long seq) {
    __hip_atomic_store((long long*)(mail + 5), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" int apgp_predict_mean_host(const double* T_host, int64_t m, const double* xs, int64_t n,
                                      const apgp_kernel_t* kern, double mean, double* mu_host,
                                      double* work, void* stream) {
    APGP_CHECK_ARG(T_host && mu_host && work && kern, "null pointer");
    APGP_CHECK_ARG(m >= 1 && m <= APGP_MAX_M, "m >= 1 required");
    APGP_CHECK_ARG(kern->ndim >= 1 && kern->ndim <= APGP_MAX_DIM, "kernel parameters");   // (sizes the staging area below)
    hipStream_t s = (hipStream_t)stream;
    const size_t tn = (size_t)m * (size_t)kern->ndim;
    {
        std::lock_guard<std::mutex> lock(apgp_stream_lock(s));
        double* io_dev = nullptr;
        double* io = apgp_stream_pinned_io(s, tn + (size_t)m, &io_dev);
        ApgpMailbox* mb = io ? apgp_stream_mailbox(s) : nullptr;
        if (io && mb && mb->host) {
            memcpy(io, T_host, tn * sizeof(double));
            const int rc = apgp_predict_mean(io_dev, m, xs, n, kern, mean, io_dev + tn, stream);
            if (rc != 0) return rc;
            const long long seq = ++mb->seq;
            hipLaunchKernelGGL(mailbox_post_kernel, dim3(1), dim3(1), 0, s, mb->dev, seq);
            APGP_CHECK_LAUNCH();
            if (ApgpSeqWait(s, 400).wait(mb->host + 5, seq) != ApgpSeqWait::OK) {
                apgp_set_error("apgp_predict_mean_host: result not posted");
                return -2;
            }
            memcpy(mu_host, io + tn, (size_t)m * sizeof(double));
            return 0;
        }
    }
    const size_t tb = tn * sizeof(double);
    double* T_dev = work;
    double* mu_dev = work + tn;
    if (hipMemcpyAsync(T_dev, T_host, tb, hipMemcpyHostToDevice, s) != hipSuccess) {
        apgp_set_error("apgp_predict_mean_host: H2D copy failed");
        return -2;
    }
    const int rc = apgp_predict_mean(T_dev, m, xs, n, kern, mean, mu_dev, stream);
    if (rc != 0) return rc;
    if (hipMemcpyAsync(mu_host, mu_dev, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        apgp_set_error("apgp_predict_mean_host: D2H copy failed");
        return -2;
    }
    return 0;
}
