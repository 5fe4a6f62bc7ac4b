/*
 * apgp.h -- C ABI of the MI355X-native GP-surrogate hot path (libapgp.so).
 *
 * This is the drop-in boundary UNDER the duck-typed ``george.GP`` object that
 * dflemin3/approxposterior calls (the reference has no FFI of its own: its
 * seam is the Python object passed as ``gp=``, approx.py:77,140-144, and the
 * arithmetic lives in the third-party george wheel).  Every entry point below
 * replaces one piece of what george does for the reference's call sites; the
 * Python class ``approxposterior_amd.gp.GP`` (host side, ctypes) strings them
 * together behind george's method names.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All matrices are IEEE
 *     fp64, row-major.  Pointers are DEVICE pointers owned by the caller unless
 *     the parameter is documented as "host".  ``stream`` is a hipStream_t
 *     passed as void* (NULL = the default stream).  Calls only ENQUEUE work;
 *     they do not synchronise unless documented.
 *   - return value: 0 = OK, <0 = bad argument (-1) / HIP error (-2);
 *     apgp_last_error() gives a thread-local message.  No exceptions cross
 *     the ABI.  Not thread-safe per stream.
 *   - gfx950 (MI355X) only; there is no CPU fallback in this library.
 */
#ifndef APGP_H
#define APGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APGP_ABI_VERSION 8
#define APGP_MAX_DIM 32          /* feature dimension D supported by the kernels (instantiated for D padded to 2 / 4 / 8 / 16 / 32) */
#define APGP_ROW_BLOCK 512       /* rows per packed L^-1 row block (sweep tile)  */
#define APGP_K_CHUNK 16          /* contraction depth per packed tile            */
#define APGP_CAND_BLOCK 64       /* candidates per sweep workgroup                */

/* Acquisition kinds (utility.py:99-250). */
#define APGP_UTIL_AGP 0          /* utility.AGPUtility   utility.py:99-142  */
#define APGP_UTIL_BAPE 1         /* utility.BAPEUtility  utility.py:145-189 */
#define APGP_UTIL_JONES 2        /* utility.JonesUtility utility.py:192-250 */
#define APGP_UTIL_NONE 3         /* predict only (george.GP.predict)        */
#define APGP_UTIL_NEG_MEAN 4     /* -mu: ApproxPosterior.findMAP's objective (apgp_nm_search only) */

/*
 * ExpSquared(+Constant)(+Constant*Linear) kernel hyper-parameters in evaluated
 * form (george.kernels.ExpSquaredKernel with axis-aligned metric, optionally
 * ``c * kernel``, optionally ``+ c2 * LinearKernel(log_gamma2, order)``;
 * gpUtils.py:160-173):
 *   k(x,x') = amp * exp(-0.5 * sum_d (x_d-x'_d)^2 * inv_metric[d])
 *           + lin_coef * sum_d (x_d * x'_d)^lin_order
 *   amp        = ndim*exp(log_constant) when fitAmp, else 1
 *   inv_metric = exp(-log_M_d_d)
 *   lin_coef   = ndim*exp(log_constant2) * exp(-log_gamma2); 0 = no linear term.
 *                The per-axis sum is george's convention for non-stationary
 *                kernels; no reference test pins it for order > 1.
 *   diag_add   = yerr^2 + exp(white_noise), added to K_ii only (never to k(t,t))
 */
typedef struct apgp_kernel {
    int32_t ndim;
    int32_t lin_order;   /* integer power P >= 0 of the linear-regression term */
    double amp;
    double diag_add;
    double inv_metric[APGP_MAX_DIM];
    double lin_coef;
} apgp_kernel_t;

/* Result record of apgp_acquire (device or host memory, 16 bytes). */
typedef struct apgp_best {
    double u;        /* smallest utility found (+inf if no admissible candidate) */
    int64_t index;   /* its GLOBAL candidate index (idx_offset + row), -1 if none */
} apgp_best_t;

int apgp_abi_version(void);
const char* apgp_last_error(void);

/* ---- sizes ------------------------------------------------------------- */
/* N rounded up to the packed row block (512).                               */
int64_t apgp_npad(int64_t n);
/* doubles in the packed lower-triangular L^-1 image for N training points.  */
int64_t apgp_packed_linv_len(int64_t n);
/* doubles in the packed training stream (scaled X | alpha) for N, D.        */
int64_t apgp_packed_train_len(int64_t n, int32_t ndim);
/* doubles of scratch apgp_trtri_pack needs (two dense Np64 x Np64 panels).  */
int64_t apgp_trtri_work_len(int64_t n);

/* ---- K1: Gram matrix ------------------------------------------------------
 * Replaces george ``kernel.get_value(X)`` + the diagonal update inside
 * ``GP.compute`` (called from gpUtils.py:178,244,254; approx.py:717 and every
 * _nll evaluation, gpUtils.py:74-78).  Writes the LOWER triangle of the symmetric
 * N x N matrix K (leading dimension ldk >= N), diagonal included; nothing above the
 * diagonal is touched (allocate K zeroed if a dense lower-triangular array is wanted):
 * apgp_potrf, the only consumer, reads the lower triangle only, and half the HBM writes
 * is half the kernel's time.
 * Domain: finite coordinates; a non-finite one is not detected.  The kernels' exp clamps its
 * argument to [-700, 700] and the clamp maps NaN to -700, so a NaN or infinite coordinate
 * yields finite entries (~amp * 1e-304) where george yields NaN: the caller checks X
 * (GP.compute does, and raises as george does).                                        */
int apgp_gram(const double* X, int64_t n, const apgp_kernel_t* kern /*host*/,
              double* K, int64_t ldk, void* stream);

/* ---- cross kernel matrix ------------------------------------------------------
 * C (m x n, ld ldc) = k(X1_i, X2_j) without the diagonal term: george
 * ``kernel.get_value(x1, x2)``.  Feeds the incremental factor update when
 * ApproxPosterior.findNextPoint appends a design point (approx.py:693-717).
 * C_ij has the bits apgp_gram gives K_ij for the same two points (off the diagonal),
 * linear term included.  Domain as apgp_gram: finite coordinates; a non-finite one is
 * not detected.                                                                   */
int apgp_kernel_cross(const double* X1, int64_t m, const double* X2, int64_t n,
                      const apgp_kernel_t* kern /*host*/, double* C, int64_t ldc, void* stream);

/* ---- Cholesky factorisation (lower, row-major, in place) -------------------
 * Replaces scipy.linalg.cholesky inside george BasicSolver.compute (every
 * gpUtils._nll evaluation, gpUtils.py:74-78; GP.compute, gpUtils.py:178,
 * approx.py:717).  Only the lower triangle of A is read and written.
 * Optionally carries a right-hand side through the factorisation: with
 * y, z != NULL, z = L^-1 (y - shift) comes out of the same launches (what
 * GP.log_likelihood needs right after a refactorisation: r^T K^-1 r = z.z), so
 * an _nll evaluation needs no separate triangular solve.
 * *info_dev (device int32): 0 = OK, k > 0 = leading minor of order k is not
 * positive definite (LAPACK dpotrf convention; george/SciPy raise LinAlgError).
 * For n > 64 the library keeps a stream-ordered scratch (hipMallocAsync) of
 * (n/64) (64^2 + 64) doubles per matrix per (device, stream), grown on demand. */
int apgp_potrf(double* A, int64_t n, int64_t lda, const double* y, double shift, double* z,
               int32_t* info_dev, void* stream);

/* ---- K2: log-determinant and diagonal range of the Cholesky factor -------
 * Replaces BasicSolver.compute's ``2*sum(log(diag(U)))`` (george; feeds
 * GP._const used by gpUtils._nll, gpUtils.py:78).  L is the lower factor
 * (row-major).  out[0] = log det K = 2*sum log L_ii, out[1] = min L_ii,
 * out[2] = max L_ii (so (out[2]/out[1])^2 is a condition estimate); the buffer
 * must hold 5 doubles (out[3], out[4] are written as 0).
 * apgp_fit_summary additionally returns out[3] = z.z (if z != NULL) and
 * out[4] = *info_dev, so one 40-byte copy fetches everything an _nll needs.   */
int apgp_logdet(const double* L, int64_t n, int64_t ldl, double* out5, void* stream);
int apgp_fit_summary(const double* L, int64_t n, int64_t ldl, const double* z,
                     const int32_t* info_dev, double* out5, void* stream);

/* ---- stream scratch ------------------------------------------------------------
 * apgp_potrf / apgp_nll_eval* (n > 64) and apgp_trsv (n >= 256) keep stream-ordered
 * device scratch per (device of the stream, stream), grown with hipMallocAsync -- so
 * they must not be called while the stream is being captured into a graph.
 * apgp_release_scratch frees (stream-ordered) what `stream` holds and returns the
 * number of buffers released: call it before destroying a stream.               */
int apgp_release_scratch(void* stream);

/* ---- one gpUtils._nll evaluation (gpUtils.py:46-80) in one call ---------------
 * apgp_gram -> apgp_potrf (z = L^-1 (y - mean) riding along) -> apgp_fit_summary, and the
 * 5-value record of apgp_fit_summary in out5_host when the call returns (the call
 * synchronises with its own work only).  n <= 64: ONE single-workgroup launch (Gram block
 * in LDS, register-resident factorisation, summary; same bits as the separate calls); 64 < n <= 128
 * (with y): both block columns in one single-workgroup launch, same bits again.
 * The record travels through 64 bytes of pinned, device-mapped host memory kept per
 * (device, stream): the last kernel's last lane writes it and a sequence word, the host
 * polls the word (400 us, then an ordinary stream synchronisation) -- no D2H copy; if
 * pinned memory is unavailable the call falls back to copy + synchronisation.
 * K: n x n work (holds the factor once the stream has passed the call's work), z: n,
 * info_dev / out5_dev: device scratch (both written as before).  Only the 5-value record in
 * out5_host is host-visible when the call returns: the host stops polling as soon as the
 * record lands, which may be before the posting kernel has finished -- K, z, *info_dev and
 * out5_dev are STREAM-ordered (read them from work enqueued on `stream`, or after
 * synchronising it), not host- or other-stream-visible on return.
 * Status as the parts'; a non-PD matrix is reported in out5_host[4] (> 0), not in the status.
 * 64 < n <= 3200 (50 block columns): the Cholesky is ONE persistent launch (csrc/potrf_persist.h:
 * row workgroups chained by in-launch hand-offs instead of a launch per 64-column step); above
 * that a hybrid -- a launch per step for the first block columns, ONE persistent launch for the
 * trailing 44 x 44 blocks; all bit-identical to the multi-launch path.  The persistent launch
 * needs one compute unit per workgroup (512 threads, 160 KB of LDS each: up to all 256 CUs), all
 * resident at once; if they are not within 50 ms (a kernel of another stream or process holds
 * compute units or LDS) the launch gives up -- every expired wait inside it marks the call
 * aborted -- and the call transparently re-runs the evaluation on the multi-launch path
 * (counted by apgp_potrf_fallbacks).  LATENCY CLIFF: such a call costs the 50 ms plus the
 * re-run; after it the next 64 evaluations on that device (doubling per consecutive give-up,
 * at most 4096) go straight to the multi-launch path (counted by apgp_potrf_backoff_skips), and
 * the first persistent launch that completes ends the back-off.
 * y == NULL and z == NULL (round 5; GP.compute / recompute): the factorisation alone on the same
 * plan, out5[3] = 0.                                                                          */
int apgp_nll_eval(const double* X, int64_t n, const apgp_kernel_t* kern /*host*/,
                  const double* y, double mean, double* K, double* z,
                  int32_t* info_dev, double* out5_dev, double* out5_host /*host*/,
                  void* stream);

/* Test / profiling switch for the Cholesky inside apgp_nll_eval (not read from the
 * environment): 0 = default: ONE persistent launch for 64 < n <= 3200, above that a hybrid
 * (a launch per 64-column step for the first block columns, one persistent launch for the
 * trailing 44 x 44 blocks); 1 = a launch per step only; 2 = persistent launch that gives up
 * at once (exercises the fallback); 3 = persistent launch wherever it can run (64 < n <= 4096).
 * + 16: the launch-per-step path without its paired trailing updates (two block columns per
 * pass over a tile while the trailing matrix is large); + 32: without the deferred tiles (a paired
 * wide step leaves half of its far tiles to the narrow step after it, whose launch is a latency
 * chain on a few workgroups) -- all variants return the same bits.
 * mode < 0 only queries; setting a mode also ends any back-off.  Returns the previous mode (-1: bad argument).
 * apgp_potrf_fallbacks: evaluations re-run on the multi-launch path so far (process-wide);
 * apgp_potrf_backoff_skips: evaluations that skipped the persistent launch while backing off. */
int apgp_potrf_mode(int mode);
int64_t apgp_potrf_fallbacks(void);
int64_t apgp_potrf_backoff_skips(void);

/* ---- `batch` _nll evaluations at different hyper-parameters, one call ----------
 * (the restarts of gpUtils.optimizeGP, gpUtils.py:223-247,
 * evaluated in lock-step.)  Same training set X, y; kerns[batch] / means[batch] on the
 * host; K: batch x n x n work (the factors on return), z: batch x n, info_dev: batch
 * int32, out5_dev / out5_host: batch x 5 doubles laid out as apgp_fit_summary's record.
 * One batched Cholesky (gridDim.y = batch): values bit-identical to single calls.
 * n <= 128 and batch <= 64 (round 5; the README configuration's restarts): ONE launch of the fused
 * single-workgroup evaluation of apgp_nll_eval, a workgroup per matrix; kernel constants, shifts and
 * the records travel through the stream's pinned, device-mapped staging area (each workgroup posts
 * its own sequence word: no copy, no synchronisation).  Same bits again.
 * 128 < n <= 3200 and 2 <= batch <= 6 (round 6; the look-ahead points of a Powell line search,
 * gpUtils.py:238): the matrices' persistent factorisations run SIDE BY SIDE in one launch (gridDim.y
 * = batch; a batched Gram launch before it, the batched finish launch after it: three launches as
 * for one evaluation), each matrix on 1 / batch of the CUs with its own scratch, flags and record:
 * a batch costs little more than one evaluation (a persistent factorisation is a latency chain on a
 * quarter of the chip).  Every matrix runs the code of the single call: same bits.  A matrix that
 * gives up sends the batch to the batched launch-per-step path (as n > 3200 and batch > 6 go
 * anyway).  apgp_nll_side_batches: batches served side by side so far (process-wide).            */
int64_t apgp_nll_side_batches(void);
int apgp_nll_eval_batch(const double* X, int64_t n, int64_t batch,
                        const apgp_kernel_t* kerns /*host*/, const double* y,
                        const double* means /*host*/, double* K, double* z,
                        int32_t* info_dev, double* out5_dev, double* out5_host /*host*/,
                        void* stream);

/* ---- K3: triangular solves for z = L^-1 (b - shift), alpha = L^-T z --------
 * Replaces BasicSolver.apply_inverse / dot_solve on a vector (scipy cho_solve;
 * george GP.log_likelihood and _compute_alpha; gpUtils.py:78, utility.py:131).
 * trans = 0: solve L x = (b - shift); trans = 1: solve L^T x = (b - shift).
 * If sumsq != NULL, *sumsq = x.x (device scalar).  x may alias b.  Below n = 256: one workgroup,
 * right-hand side in LDS.  256 <= n <= 16384: ONE persistent launch (a workgroup per 64-row block,
 * solved blocks handed on as data-tagged granules; stream-ordered scratch per (device, stream):
 * slot 3 of csrc/scratch.h).  Above, or with apgp_trsv_mode(1): one launch per 256 rows with n
 * doubles of stream-ordered scratch.  All paths return the same bits.  If the persistent launch's
 * workgroups are not all resident within its timeout, x and *sumsq are written as NaN (no
 * automatic re-run: callers that may share the device re-issue with apgp_trsv_mode(1)).      */
int apgp_trsv(const double* L, int64_t n, int64_t ldl, const double* b, double shift,
              int trans, double* x, double* sumsq, void* stream);
/* Test / profiling switch (not read from the environment): 1 = the multi-launch path, 0 = default
 * (persistent launch where it applies); < 0 queries.  Returns the previous value.             */
int apgp_trsv_mode(int multi_launch);
/* apgp_trsv with the path chosen for THIS call (0: persistent launch where it applies, 1: a launch per
 * 256 rows, < 0: the process-wide switch): the re-run of one solve that came back NaN, without changing
 * what other threads' or streams' calls get (round 6).                                */
int apgp_trsv_ex(const double* L, int64_t n, int64_t ldl, const double* b, double shift,
                 int trans, double* x, double* sumsq, int mode, void* stream);

/* ---- pivot of an appended factor row -----------------------------------------
 * Incremental fit when ApproxPosterior.findNextPoint appends a design point
 * (approx.py:693-717): with l = L^-1 k(x_new, X_old) already in the new row (apgp_kernel_cross
 * + apgp_trsv, *ss = l.l on the device), writes *ljj = sqrt(kdiag - *ss), kdiag = k(x_new,
 * x_new) + diag_add.  *info_dev (device int32, caller-initialised to 0) keeps the FIRST
 * non-positive pivot's 1-based leading-minor order (LAPACK convention; rows are appended in
 * stream order) and 1.0 is stored so that later rows stay finite.                        */
int apgp_append_diag(double* ljj, const double* ss, double kdiag, int32_t* info_dev, int64_t order,
                     void* stream);

/* ---- K3 through the resident explicit inverse -------------------------------
 * x = W (b - shift) (trans = 0) or x = W^T b (trans = 1, shift must be 0) for the dense
 * lower-triangular W = L^-1 that apgp_trtri_pack leaves in the first panel of its work
 * buffer (winv, leading dimension ldw = n rounded up to 64): z and alpha of george's
 * GP._compute_alpha (behind every GP.predict, utility.py:131,178,224; approx.py:178) as two
 * HBM-rate matrix-vector products once the sweep's W exists, instead of two triangular
 * solves.  If sumsq != NULL, *sumsq = x.x (device scalar).  x must not alias b.
 * work: apgp_winv_apply_work_len(n) doubles (trans = 1 only).  Use apgp_trsv instead when the
 * condition estimate exceeds ~1e10 (same rule as apgp_acquire vs apgp_acquire_solve).     */
int64_t apgp_winv_apply_work_len(int64_t n);
int apgp_winv_apply(const double* winv, int64_t ldw, int64_t n, const double* b, double shift,
                    int trans, double* x, double* sumsq, double* work, void* stream);

/* ---- L^-1 in the sweep's packed tile layout --------------------------------
 * Computes W = L^-1 (blocked recursive triangular inversion, MFMA-f64 GEMM
 * merges) and writes it as lower-triangular 512 x 16 tiles in MFMA A-fragment
 * order (see DESIGN.md "packed factor").  This is what lets the sweep evaluate
 * BasicSolver.apply_inverse(Kxs.T) (george GP.predict, utility.py:131,178,224)
 * for millions of candidates without materialising Kxs.
 * work: apgp_trtri_work_len(n) doubles; on return its first panel holds the
 * dense row-major L^-1 with leading dimension n rounded up to 64.
 * packed: apgp_packed_linv_len(n) doubles (may be NULL).
 * If winv_dense != NULL (n x n, ld n) a compact copy of L^-1 is also stored. */
int apgp_trtri_pack(const double* L, int64_t n, int64_t ldl, double* work,
                    double* packed, double* winv_dense, void* stream);

/* ---- packed training stream ------------------------------------------------
 * rows k = 0..npad-1 of [ x_k * sqrt(inv_metric/2) (Dpad) | alpha_k | 0 ].   */
int apgp_pack_train(const double* X, const double* alpha, int64_t n,
                    const apgp_kernel_t* kern /*host*/, double* xs, void* stream);

/* ---- K5/K6: fused predict + acquisition sweep + arg-min --------------------
 * For every candidate row t of T (m x ndim):
 *   mu  = k(t,X).alpha + mean                     (george GP.predict)
 *   var = amp - || L^-1 k(t,X)^T ||^2             (return_var=True)
 *   u   = utility(kind)(mu, var)                  (utility.py:136,183,229-244)
 *   u   = +inf if t is outside [lo,hi] (box prior; utility.py:126,173,219) or
 *         mask[i] == 0
 * and the arg-min over candidates (ties -> lowest index, NaN never wins):
 * the batched counterpart of utility.minimizeObjective (utility.py:253-372).
 * A row of T with a NaN coordinate is inadmissible with or without a box or a mask (the reference
 * refuses it in its prior): mu = var = NaN, u = +inf, never the arg-min -- in apgp_acquire,
 * apgp_acquire_solve and apgp_acquire_fantasy alike.  (The reference's JONES formula alone would
 * give such a row 0.0, its ``std > 0`` being false, which ties with an underflowed tail.)
 * mu / var / u may be NULL (not stored).  lo/hi are host arrays or NULL.
 * part: scratch of apgp_acquire_work_len(m, n) doubles, 16-byte aligned: the
 *       per-block arg-min partials plus, for n > APGP_ROW_BLOCK, the stream in
 *       which each persistent workgroup parks the k* operands it generated for
 *       one row block so that later row blocks do not regenerate them, and the
 *       per-row-block shares of the candidate blocks of a short last round
 *       (those are split over one workgroup per row block), and the block
 *       bounds, block lists and counters of the pruned arg-min (below), and
 *       last, for n > 256, the fold inputs of its seed step's row-half
 *       workgroups (16 seed blocks x ceil(n / 256) row blocks x 9216 doubles:
 *       the upper half's sums so far and the lower half's accumulators).
 * best: device apgp_best_t, written by the final reduction kernel.
 * ybest = max(y) and zeta are used by JONES only.                            */
int64_t apgp_acquire_work_len(int64_t m, int64_t n);
int apgp_acquire(const double* T, int64_t m, int64_t idx_offset,
                 const double* packed_linv, const double* xs, int64_t n,
                 const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                 const double* lo /*host*/, const double* hi /*host*/,
                 const uint8_t* mask, double zeta, double ybest,
                 double* mu, double* var, double* u,
                 void* part, apgp_best_t* best, void* stream);

/* ---- substitution form of apgp_acquire (no explicit inverse) ------------------
 * Same semantics, outputs, scratch (apgp_acquire_work_len) and arg-min contract as
 * apgp_acquire, but sigma^2 = amp - |L^-1 k*|^2 comes from a BLOCKED FORWARD
 * SUBSTITUTION against the factor L itself -- what george's cho_solve does
 * (BasicSolver.apply_inverse, reached from utility.py:131,178,224) -- instead of
 * a product with the packed explicit inverse.  Use it when the condition
 * estimate of apgp_fit_summary, (out[2]/out[1])^2, exceeds ~1e10 (the reference's
 * own fitAmp=True optimum, tests/test_OptimizeGP.py:50, has cond(K) 8.5e15: the
 * explicit inverse is 200x off there, this form stays in cho_solve's error
 * class); it runs on the same matrix-core stream at about the same rate, for any n
 * the inverse form takes.
 * apgp_pack_lsolve writes the tiles it streams (apgp_packed_lsolve_len(n) doubles,
 * same geometry as the packed inverse): -L below the diagonal 16 x 16 blocks, and
 * those blocks prepared for the in-register solve (their 4 x 4 diagonal blocks
 * inverted, the rest negated).  One O(n^2) pass, no triangular inversion.     */
int64_t apgp_packed_lsolve_len(int64_t n);
int apgp_pack_lsolve(const double* L, int64_t n, int64_t ldl, double* packed, void* stream);
int apgp_acquire_solve(const double* T, int64_t m, int64_t idx_offset,
                       const double* packed_lsolve, const double* xs, int64_t n,
                       const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                       const double* lo /*host*/, const double* hi /*host*/,
                       const uint8_t* mask, double zeta, double ybest,
                       double* mu, double* var, double* u,
                       void* part, apgp_best_t* best, void* stream);

/* ---- pruned arg-min of the sweep (branch and bound) ------------------------------
 * When only the winner is asked for (kind != APGP_UTIL_NONE, mu = var = u = NULL), apgp_acquire and
 * apgp_acquire_solve skip the 64-row candidate blocks that cannot hold it: var <= k(t,t) and the
 * utilities do not increase with var, so b = utility(mu, k(t,t)) -- a mean-only prediction -- bounds
 * a row's utility from below, and a block whose smallest bound (less a rounding slack) lies above a
 * utility already found is never contracted.  Surviving blocks run through the sweep's own kernel:
 * best has the index and the bits of the full sweep, ties included.  No host synchronisation; safe
 * on a capturing stream.
 * apgp_set_sweep_prune(v): process-wide switch, returns the previous value.  0: always the full
 * sweep; 1 (default): pruned from a built-in candidate count on (16384 for n >= 4096, else 65536);
 * v >= 2: pruned whenever m >= v.
 * For a pure squared-exponential kernel (lin_coef == 0) the bound is taken in two stages: a coarse one
 * over all blocks whose kernel values are single precision (its slack covers their error), then the
 * double-precision bound on the blocks the coarse one left at or below tau; with a LinearKernel term
 * the double-precision bound alone.
 * apgp_sweep_prune_counts_offset(m, n): index into `part` (in 8-byte words) of four int64 the last
 * pruned call left there: seed blocks, surviving blocks beyond the seeds, bit pattern of tau, blocks
 * beyond the seeds the coarse bound left (equal to the second without a coarse stage).
 * apgp_sweep_prune_select: the selection step alone, for tests -- tau planted by the caller.
 * bmin: ncb block bounds; seeds: 16 int64 block numbers of which the first counts[0] are read;
 * counts: int64[3], [0] read, [1] and [2] written (survivor count, bit pattern of tau); list: ncb
 * int64, receives the blocks with bmin < +inf, bmin <= tau that are no seeds, in ascending order.
 * All pointers device memory.
 * apgp_set_seed_rowsplit(v): process-wide switch of the seed step's launch, returns the previous value.  That
 * launch is one workgroup per (seed block, 256-row block of W); a row block at or above J0 that has rows in its
 * lower half goes as TWO workgroups of 128 rows each, and a fold step puts their sums together in the whole row
 * block's order -- the bits do not depend on J0.  -1 (default): J0 by the library's rule (a model of the launch on
 * the chip's 256 CUs); v >= 0: J0 = v (0: every such row block, v >= ceil(n / 256): none).  Inverse form only;
 * apgp_acquire_solve ignores it.  Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.
 * apgp_set_seed_park(v): process-wide switch of the same launch, returns the previous value.  1 (default): the
 * k*(t, x) operands of the seed blocks are generated once, by a launch of their own, into the parked-operand
 * region of `part`, and the seed launch's workgroups read the chunks left of their diagonal from there; 0: every
 * workgroup generates every operand it needs, the launch as it was.  The bits do not depend on it.  Pure
 * squared-exponential kernels, inverse form, n > 256; everything else ignores it.  apgp_acquire_work_len is
 * unchanged; APGP_ABI_VERSION stays 8.
 * apgp_set_seed_first(v): process-wide switch of the seed step, returns the previous value.  The 16 seed blocks are
 * swept in two waves: the first K of them, then those of the others whose bound does not lie above the smallest
 * utility the first wave found (a seed that can neither win nor tie keeps the +inf partial the bound pass wrote).  tau
 * and the winner do not depend on K.  -1 (default): K = 4 for pure squared-exponential kernels, inverse form, n > 256,
 * where the library's launch model says two waves are the shorter (from n ~ 2048 on), 16 (one wave, the launches as
 * they were) elsewhere; 1 .. 16: K = v for those kernels, that form and n > 256.  A fifth int64 behind the four of
 * apgp_sweep_prune_counts_offset counts the second-wave seeds that were swept.
 * apgp_set_seed_parts(v): process-wide switch of the seed launches, returns the previous value.  A row block that
 * apgp_set_seed_rowsplit splits goes as 8 / v workgroups of v sub-block pairs (32 v rows) each: 8: whole, 4: the two
 * halves, 2 and 1: finer; -1 (default): the library's rule.  The bits do not depend on it.  apgp_acquire_work_len
 * grew with the fold inputs of the finer parts; APGP_ABI_VERSION stays 8.
 * apgp_set_prune_pipe(v): process-wide switch of the coarse bound pass over the sign-sorted rows
 * (APGP_PRUNE_ROWS_SIGNED), returns the previous value.  1 (default): the kernel whose row loop issues the next
 * group's matrix products between slices of this group's exponentials and reads the next matrix tile's rows ahead;
 * 0: the loop in the order the compiler gives it, the kernel as it was.  The bits do not depend on it.  Every other
 * kind of rows ignores it.  APGP_ABI_VERSION stays 8.
 * apgp_set_seed_prefetch(v): process-wide switch of the parked seed launch (apgp_set_seed_park on), returns the previous
 * value.  A row-part workgroup of that launch keeps its tiles in a ring of stages in LDS and requests the re-read
 * tiles up to v tiles ahead of the matrix wavefronts, at most what the ring holds for its part size (2 / 4 / 6 tiles
 * for parts of four / two / one sub-block pair).  0: one tile ahead, the launch as it was; 6 (default; larger values
 * count as 6, negative ones as 0).  The bits do not depend on it.  Everything but the parked seed launch ignores it;
 * APGP_ABI_VERSION stays 8.  */
int apgp_set_seed_prefetch(int v);
int apgp_get_seed_prefetch(void);
int apgp_set_sweep_prune(int v);
int apgp_get_sweep_prune(void);
int apgp_set_seed_rowsplit(int v);
int apgp_get_seed_rowsplit(void);
int apgp_set_seed_park(int v);
int apgp_get_seed_park(void);
int apgp_set_prune_pipe(int v);
int apgp_get_prune_pipe(void);
int apgp_set_seed_first(int v);
int apgp_get_seed_first(void);
int apgp_set_seed_parts(int v);
int apgp_get_seed_parts(void);
int64_t apgp_sweep_prune_counts_offset(int64_t m, int64_t n);
int apgp_sweep_prune_select(const double* bmin, int64_t ncb, const int64_t* seeds, int64_t* counts,
                            double tau, int64_t* list, void* stream);
/* Two more steps alone, for tests.  apgp_prune_bounds: one bound pass over all ceil(m / 64) blocks into
 * bmin_out (device), arguments as apgp_acquire's; coarse != 0: the single-precision stage (refused
 * with a LinearKernel term), 0: the double-precision bound.  apgp_sweep_prune_seeds: the seed step --
 * seeds: 16 int64, receives the blocks with the smallest bmin below +inf, ascending by (value, block
 * number); counts: int64[4], [0] = their number, [1] = [3] = 0.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.             */
int apgp_prune_bounds(const double* T, int64_t m, const double* xs, int64_t n,
                      const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                      const double* lo /*host*/, const double* hi /*host*/, const uint8_t* mask,
                      double zeta, double ybest, int coarse, double* bmin_out, void* stream);
int apgp_sweep_prune_seeds(const double* bmin, int64_t ncb, int64_t* seeds, int64_t* counts, void* stream);

/* The coarse bound's training rows, split once per fit.  Up to 8 dimensions the single-precision stage forms its
 * exponents on the bf16 matrix cores from every training row split into three bf16 parts; without the stream below
 * every workgroup of every call splits all rows itself.  The split depends on xs (apgp_pack_train) alone, not on the
 * candidates, the utility, the mean or the amplitude: pack it once per fit, behind apgp_pack_train.
 * apgp_prune_rows_len: doubles in the stream (16-byte aligned device memory); 0 beyond 8 dimensions, where the coarse
 * bound does not use it (pass NULL then).  Layout: a 16-byte header -- max |x - c|^2 over the rows (c = the first row)
 * and sum |alpha|, both fp64 with the bits the bound kernel reduces them to itself -- and per 128-row tile the kernel's
 * image of the rows (bf16) followed by the tile's 128 fp32 alphas.
 * apgp_pack_prune_rows: one launch; rows receives the stream.
 * apgp_acquire_rows, apgp_acquire_solve_rows, apgp_prune_bounds_rows: their namesakes with the stream as one more
 * argument (prune_rows; NULL: the namesake itself).  Results are the namesakes', bit for bit.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.             */
int64_t apgp_prune_rows_len(int64_t n, int32_t ndim);
int apgp_pack_prune_rows(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, void* rows, void* stream);
int apgp_acquire_rows(const double* T, int64_t m, int64_t idx_offset,
                      const double* packed_linv, const double* xs, int64_t n,
                      const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                      const double* lo /*host*/, const double* hi /*host*/,
                      const uint8_t* mask, double zeta, double ybest,
                      double* mu, double* var, double* u,
                      void* part, apgp_best_t* best, const void* prune_rows, void* stream);
int apgp_acquire_solve_rows(const double* T, int64_t m, int64_t idx_offset,
                            const double* packed_lsolve, const double* xs, int64_t n,
                            const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                            const double* lo /*host*/, const double* hi /*host*/,
                            const uint8_t* mask, double zeta, double ybest,
                            double* mu, double* var, double* u,
                            void* part, apgp_best_t* best, const void* prune_rows, void* stream);
int apgp_prune_bounds_rows(const double* T, int64_t m, const double* xs, int64_t n,
                           const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                           const double* lo /*host*/, const double* hi /*host*/, const uint8_t* mask,
                           double zeta, double ybest, int coarse, double* bmin_out, const void* prune_rows,
                           void* stream);

/* ---- the same rows sorted by the sign of alpha (the coarse bound's one-chain route) --
 * The coarse bound adds sum alpha k and sum |alpha| k per candidate in fp32 partial sums over 16 training rows.  In
 * the stream below the rows stand in an order in which every such 16 rows carry alphas of one sign; the second sum is
 * then the absolute value of the first, bit for bit, and the bound kernel runs one chain of fused multiply-adds per
 * kernel value where the route above runs two.  The bounds differ from the other routes' in their last bits (another
 * order of the rows); they are valid bounds under the same slack, and the winner does not depend on the route.
 * apgp_prune_srows_len: doubles in the stream (16-byte aligned device memory); 0 beyond 8 dimensions.  Layout: a 32-byte
 * header -- max |x - c|^2 and sum |alpha| (fp64), the number of 32-row matrix tiles that hold a row (int64), 8 bytes of
 * zero -- and per 128-row tile the image and the 128 fp32 alphas of apgp_pack_prune_rows.  Rows with alpha >= 0 come
 * first, 16 to a group, in their original order, then the rows with alpha < 0 in theirs; group q is the rows
 * (s & 3) + 8 (s >> 2) + 4 (q & 1), s = 0 .. 15, of 32-row tile q >> 1; a slot without a row has alpha 0.
 * apgp_pack_prune_srows: one launch; rows receives the stream.  It depends on xs alone: once per fit.
 * apgp_acquire_rows2, apgp_acquire_solve_rows2, apgp_prune_bounds_rows2: the entry points above with the kind of the
 * stream as one more argument: APGP_PRUNE_ROWS_SPLIT (the stream of apgp_pack_prune_rows: the entry points above
 * themselves) or APGP_PRUNE_ROWS_SIGNED (this one); any other kind, or SIGNED with a NULL stream, is refused (-1).
 * apgp_prune_bounds_rows2 also takes est_out (device, ceil(m / 64) doubles, or NULL): with coarse = 1 it receives per
 * block the smallest b WITHOUT its slack -- what the pruned arg-min chooses its seeds by; a block's bmin and est come
 * from the same row where one row of the block is admissible.  Not written with coarse = 0.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.             */
#define APGP_PRUNE_ROWS_SPLIT 0
#define APGP_PRUNE_ROWS_SIGNED 1
int64_t apgp_prune_srows_len(int64_t n, int32_t ndim);
int apgp_pack_prune_srows(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, void* rows, void* stream);
int apgp_acquire_rows2(const double* T, int64_t m, int64_t idx_offset,
                       const double* packed_linv, const double* xs, int64_t n,
                       const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                       const double* lo /*host*/, const double* hi /*host*/,
                       const uint8_t* mask, double zeta, double ybest,
                       double* mu, double* var, double* u,
                       void* part, apgp_best_t* best, const void* prune_rows, int32_t rows_kind, void* stream);
int apgp_acquire_solve_rows2(const double* T, int64_t m, int64_t idx_offset,
                             const double* packed_lsolve, const double* xs, int64_t n,
                             const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                             const double* lo /*host*/, const double* hi /*host*/,
                             const uint8_t* mask, double zeta, double ybest,
                             double* mu, double* var, double* u,
                             void* part, apgp_best_t* best, const void* prune_rows, int32_t rows_kind, void* stream);
int apgp_prune_bounds_rows2(const double* T, int64_t m, const double* xs, int64_t n,
                            const apgp_kernel_t* kern /*host*/, double mean, int32_t kind,
                            const double* lo /*host*/, const double* hi /*host*/, const uint8_t* mask,
                            double zeta, double ybest, int coarse, double* bmin_out, const void* prune_rows,
                            int32_t rows_kind, double* est_out, void* stream);

/* ---- fantasy update of a sweep (batch design points, kriging believer) -----------
 * After a sweep over T (mu, var = v_0 written) and picks x_1 .. x_j, conditioning the GP on
 * x_j = T[pick_row] observed at y = mu(x_j) (hyper-parameters unchanged) leaves mu as it is
 * and lowers every candidate's variance by a rank-one term.  One pass, for step j:
 *   s_j   = var_in[pick_row] + kern->diag_add                           (read on the device)
 *   c(t)  = k(t, x_j) - k(t, X).beta - sum_{i<j} C_i(t) C_i(x_j)        beta = K^-1 k(X, x_j)
 *   C_j   = c / sqrt(s_j)            -> column j - 1 of C (C_i lives in column i - 1)
 *   v_j   = var_in - C_j^2           -> var_out
 *   u     = utility(kind)(mu, v_j), +inf outside [lo, hi] / where mask == 0, arg-min into best
 * with the sweep's utility formulas, gate and arg-min contract (ties -> lowest index, NaN never
 * wins).  T: m x ndim; xs: packed training stream (its alpha column is not read); beta: n
 * (apgp_kernel_cross + two apgp_trsv); C: column-major, ldc >= m, at least j columns.
 * var_in and var_out must not alias (the pass reads var_in[pick_row] while it writes var_out:
 * callers ping-pong two buffers).  ybest (Jones): max(y, mu(x_1), .., mu(x_j)).  u may be NULL.
 * 1 <= j < APGP_MAX_FANTASY: a batch holds at most APGP_MAX_FANTASY points.  kind: AGP / BAPE /
 * JONES.  part: apgp_acquire_fantasy_work_len(m) doubles, 16-byte aligned.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.              */
#define APGP_MAX_FANTASY 32
int64_t apgp_acquire_fantasy_work_len(int64_t m);
int apgp_acquire_fantasy(const double* T, int64_t m, int64_t idx_offset,
                         const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/,
                         const double* beta, int64_t pick_row, int32_t j, double* C, int64_t ldc,
                         const double* mu, const double* var_in, double* var_out,
                         int32_t kind, const double* lo /*host*/, const double* hi /*host*/,
                         const uint8_t* mask, double zeta, double ybest,
                         double* u, void* part, apgp_best_t* best, void* stream);

/* ---- posterior function draws (GP.sample_paths, Thompson batches) ------------------
 * S = ndraws functions drawn from the GP posterior, evaluated at the m rows t of T (m x ndim), and the arg-max of each.
 * By Matheron's rule a posterior draw is a prior draw plus a data term; the squared-exponential part of the prior draw
 * is a sum of R = nfeat random cosines in the scaled coordinates ts_d = t_d sqrt(inv_metric_d / 2), the linear term has
 * an exact feature map of ndim features:
 *   g_s(t) = sqrt(2 amp / R) sum_{r<R} W[s,r] cos(sqrt2 Z[r,:].ts + b[r]) + sqrt(lin_coef) sum_{d<ndim} Wl[s,d] t_d^P
 *   f_s(t) = mean + g_s(t) + k(t, X).V[:,s]
 * The caller draws Z (R x ndim) ~ N(0,1), b (R) ~ U[0, 2 pi), W (S x R) ~ N(0,1), Wl (S x ndim) ~ N(0,1) (Wl may be NULL
 * without a linear term) and solves V (n x S, row-major) = K^-1 (y - mean - g_s(X) - eps_s), eps_s ~ N(0, diag_add); the
 * device only evaluates.  Only the squared-exponential part of the prior draw is approximate (O(R^-1/2) in
 * distribution); the data term is exact, so with W = Wl = 0 f_s is the predictive mean.
 * xs: the packed training stream (its alpha column is not read).  V == NULL: the data term is skipped (xs and n are not
 * read) -- with T = X and mean = 0 the call evaluates g_s(X) for the right-hand sides above.
 * F (S x m, row-major, may be NULL) receives f_s(t).  best: S records on the device; record s holds the arg-min of
 * u = -f_s(t) over the admissible rows and its global index idx_offset + row, with the sweep's contract: ties go to the
 * lowest index; NaN never wins; a row outside [lo, hi] (host arrays or NULL), with mask[row] == 0 (device or NULL) or
 * with a NaN coordinate has u = +inf and F = NaN; no admissible row gives index -1 and u = +inf.
 * part: apgp_path_draws_work_len(m, ndraws) doubles, 16-byte aligned (-1: m or ndraws beyond the limits; 0: nothing to do).
 * 1 <= ndraws <= APGP_MAX_DRAWS, 1 <= nfeat <= APGP_MAX_FEATURES.  No atomics, a fixed order in every sum.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
#define APGP_MAX_DRAWS 32
#define APGP_MAX_FEATURES 65536
int64_t apgp_path_draws_work_len(int64_t m, int32_t ndraws);
/* Test / profiling switch (not read from the environment) for where the contraction with the S weights runs: 0 =
 * default (the faster form per shape: the matrix cores above 8 draws when ndim <= 8, else the vector units), 1 = the
 * vector units always, 2 = the matrix cores wherever that kernel exists (ndraws > 1, ndim <= 8); < 0 queries.  Both
 * forms sum in a fixed order of their own: they agree to rounding, not bit for bit.  Returns the previous value (-1:
 * bad argument).                                                                                                   */
int apgp_path_draws_mode(int mode);
int apgp_path_draws(const double* T, int64_t m, int64_t idx_offset, const double* xs, int64_t n,
                    const apgp_kernel_t* kern /*host*/, double mean, const double* V, const double* Z,
                    const double* b, const double* W, const double* Wl, int32_t nfeat, int32_t ndraws,
                    const double* lo /*host*/, const double* hi /*host*/, const uint8_t* mask, double* F,
                    void* part, apgp_best_t* best, void* stream);

/* ---- integrated acquisition (GP.acquire_integrated; DESIGN.md "Integrated acquisition") ------------------
 * The expected integrated variance of the posterior estimate exp(f) after one more evaluation at t (noise diag_add,
 * hyper-parameters unchanged), integrated over J = nref reference points r_j and reduced to what depends on t:
 *   u(t) = -log sum_j exp(a_j + c_j(t)^2 / s(t)),  c_j(t) = k(t, r_j) - sum_n k(t, x_n) B[n, j],  s(t) = var(t) + diag_add
 * for the m rows t of T (m x ndim), and its arg-min.  The caller solves B (n x nref, row-major: a training row's J
 * weights side by side) = K^-1 k(X, R) and supplies a (nref log-weights: log w_j + 2 mu(r_j) + var(r_j); -inf: the column
 * contributes nothing, not one bit) and var (m; the sweep's output).  R: nref x ndim in the caller's coordinates.
 * xs: the packed training stream (its alpha column is not read).
 * C (may be NULL): column-major, ldc >= m; column j receives c_j(t).  u (may be NULL): m values.  best: one record on the
 * device with the sweep's contract: ties go to the lowest global index idx_offset + row; NaN and +inf never win; a row
 * outside [lo, hi] (host arrays or NULL), with mask[row] == 0 (device or NULL), with a NaN coordinate or with s(t) not
 * positive or not finite has u = +inf and NaN in its row of C; no admissible row gives index -1 and u = +inf.
 * The log-sum-exp is a running (max, sum) over j ascending.  No atomics, a fixed order in every sum; a row's u and C do
 * not depend on the other rows of the call.
 * part: apgp_integrated_work_len(m, nref) doubles, 16-byte aligned (-1: m or nref beyond the limits; 0 for m = 0).
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
#define APGP_MAX_REFS 4096
#define APGP_INTEGRATED_MAX_DIM 16      /* ndim above it is refused (-1): the pass has no kernel for D padded to 32 */
int64_t apgp_integrated_work_len(int64_t m, int32_t nref);
/* Test / profiling switch (not read from the environment) for where the contraction with the columns of B runs: 0 =
 * default (the matrix cores when ndim <= 8, else the vector units), 1 = the vector units always; < 0 queries.  The two
 * forms sum in a fixed order of their own: they agree to rounding, not bit for bit.  Returns the previous value (-1:
 * bad argument).                                                                                                   */
int apgp_integrated_mode(int mode);
int apgp_acquire_integrated(const double* T, int64_t m, int64_t idx_offset,
                            const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/,
                            const double* R, int32_t nref, const double* B, const double* a,
                            const double* var, const double* lo /*host*/, const double* hi /*host*/,
                            const uint8_t* mask, double* C, int64_t ldc, double* u,
                            void* part, apgp_best_t* best, void* stream);

/* ---- ONE candidate: george GP.predict(y, t[1 x D], return_var=True) ----------
 * What the reference's scalar utilities evaluate once per Nelder-Mead step
 * (utility.py:131,178,224 <- minimizeObjective, utility.py:336-372; the default
 * point search of ApproxPosterior.findNextPoint).  t_host: the candidate (host,
 * ndim doubles; it travels in the kernel arguments).  xs: packed training stream
 * (with alpha).  winv / ldw: the dense L^-1 left by apgp_trtri_pack in its work
 * buffer -> sigma^2 by one matrix-vector product; or winv = NULL and L / ldl: the
 * factor -> one triangular solve (use it above the conditioning gate).  work:
 * apgp_predict1_work_len(n) doubles (device).  out2_host: mu, sigma^2 -- through the
 * stream's pinned mailbox when the call returns (no allocation, copy or stream
 * synchronisation; falls back to copy + synchronisation without pinned memory).
 * Three small launches; through winv at n <= 256 ONE single-workgroup launch (round 5,
 * same bits; apgp_potrf_mode 1 keeps the three).                                       */
int64_t apgp_predict1_work_len(int64_t n);
int apgp_predict1_host(const double* t_host /*host*/, const double* xs, int64_t n,
                       const apgp_kernel_t* kern /*host*/, double mean,
                       const double* winv, int64_t ldw, const double* L, int64_t ldl,
                       double* work, double* out2_host /*host*/, void* stream);

/* ---- restarted Nelder-Mead point search, all restarts in one launch ------------
 * The device form of utility.minimizeObjective's default search (SciPy 1.15 _minimize_neldermead, bounds=None):
 * restart r (one workgroup, no communication between workgroups) starts from row r of `starts` (R x ndim, device)
 * and minimises the objective
 *   u(x) = +inf                              if a coordinate is not finite or lies outside [lo, hi] (host arrays,
 *                                            NULL = no box), else
 *          utility(kind)(mu(x), sigma^2(x))  kind AGP / BAPE / JONES (apgp_acquire's formulas; JONES: zeta, ybest)
 *          -mu(x), +inf where mu is not finite  kind APGP_UTIL_NEG_MEAN
 * mu, sigma^2 as apgp_predict1_host: through winv / ldw (the dense L^-1 of apgp_trtri_pack; n <= 256: the
 * arithmetic of apgp_predict1_host, same bits) or, with winv = NULL, through the factor L / ldl (an in-workgroup
 * triangular solve).  The simplex arithmetic is SciPy's, uncontracted; the vertices are re-sorted after every
 * iteration by a stable sort on the previous position with NaN last.  opt->rho/chi/psi/sigma are SciPy's
 * coefficients as the host computed them.  Every loop is bounded by maxiter / maxfev.
 * Outputs (device): x_out R x ndim (the best vertex), f_out R (np.min of the final values: NaN if one is NaN),
 * stats R x 3 int32 (nfev, nit, status: 0 converged, 1 maxfev, 2 maxiter).
 * trace (device, may be NULL): R x maxfev records of ndim + 3 doubles (x, mu, sigma^2, u) in evaluation order
 * (mu = sigma^2 = NaN where the gate refused the point); steps (device, may be NULL): R x maxiter int32, the step
 * of each iteration (APGP_NM_STEP_*).  work: apgp_nm_search_work_len(R, n) doubles.
 * Limits: 1 <= ndim <= APGP_MAX_DIM, 1 <= R <= APGP_NM_MAX_RESTARTS, 1 <= maxiter, maxfev <= APGP_NM_MAX_FEV.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                               */
#define APGP_NM_MAX_RESTARTS 4096
#define APGP_NM_MAX_FEV (1 << 20)
#define APGP_NM_STEP_REFLECT 1          /* xr accepted (fsim[0] <= f(xr) < fsim[-2])                        */
#define APGP_NM_STEP_EXPAND 2           /* xe accepted                                                      */
#define APGP_NM_STEP_REFLECT_EXP 3      /* expansion tried, xr kept                                         */
#define APGP_NM_STEP_CONTRACT_OUT 4     /* outside contraction accepted                                     */
#define APGP_NM_STEP_CONTRACT_IN 5      /* inside contraction accepted                                      */
#define APGP_NM_STEP_SHRINK_OUT 6       /* outside contraction refused -> shrink                            */
#define APGP_NM_STEP_SHRINK_IN 7        /* inside contraction refused -> shrink                             */
#define APGP_NM_STEP_MAXFEV 8           /* the iteration stopped at maxfev                                  */
typedef struct apgp_nm_options {
    int32_t kind;
    int32_t maxiter;
    int32_t maxfev;
    int32_t reserved;
    double zeta, ybest;
    double xatol, fatol;
    double rho, chi, psi, sigma;
} apgp_nm_options_t;
int64_t apgp_nm_search_work_len(int64_t restarts, int64_t n);
int apgp_nm_search(const double* starts, int64_t restarts, const double* xs, int64_t n,
                   const apgp_kernel_t* kern /*host*/, double mean,
                   const double* winv, int64_t ldw, const double* L, int64_t ldl,
                   const double* lo /*host*/, const double* hi /*host*/, const apgp_nm_options_t* opt /*host*/,
                   double* x_out, double* f_out, int32_t* stats, double* trace, int32_t* steps,
                   double* work, void* stream);

/* ---- predictive gradients: mu, sigma^2, a utility and their derivatives in t ---------
 * For each of the m rows t of T (device, m x ndim), with the kernel of apgp_kernel_t exactly as defined above
 * (the linear term included):
 *   k_n = k(t, x_n)                         J_nd   = d k(t, x_n) / d t_d
 *   mu  = k.alpha + mean                    dmu_d  = sum_n alpha_n J_nd
 *   v   = L^-1 k,  w = L^-T v (= K^-1 k)
 *   var = k(t,t) - |v|^2                    dvar_d = d k(t,t) / d t_d - 2 sum_n w_n J_nd
 *   u   = utility(kind)(mu, var)            du_d   = (du/dmu) dmu_d + (du/dvar) dvar_d
 * d k(t,t) / d t_d is zero for the pure squared-exponential kernel and lin_coef 2 P t_d^(2P-1) with a linear term.
 * kind (csrc/util_grad.h): AGP du/dmu = -1, du/dvar = -1 / (2 var); BAPE -2, -(2 + 1 / expm1(var)); JONES -Phi(z),
 * -phi(z) / (2 sd) (zeta, ybest as apgp_acquire); APGP_UTIL_NEG_MEAN -1, 0; APGP_UTIL_NONE: u and du are not written.
 * Variance route as apgp_predict1_host / apgp_nm_search: winv / ldw (the dense L^-1 of apgp_trtri_pack, 16-byte
 * aligned, ldw even) -> v = W k, w = W^T v, two passes over W per block of 8 points; or winv = NULL and L / ldl -> a
 * forward and a backward substitution against the factor, a workgroup per block of 4 points (use it above the
 * conditioning gate).  xs: the packed training stream (with alpha).
 * Outputs (device, each may be NULL): mu, var, u (m); dmu, dvar, du (m x ndim, row-major).
 * A row with a non-finite coordinate or outside [lo, hi] (host arrays, NULL = no box): mu = var = dmu = dvar = NaN,
 * u = +inf, du = 0.  BAPE with var <= 0: u = +inf, du = 0.  JONES with sd not > 0: u = 0, du = 0.  NEG_MEAN with a
 * non-finite mu: u = +inf, du = 0.  AGP with var < 0: u and du NaN, as NumPy would give.
 * work: apgp_predict_grad_work_len(m, n) doubles (device, 16-byte aligned); the call works through the rows in chunks
 * of what that holds.  0 <= m <= APGP_MAX_M (2^40), 1 <= n <= 2^24, 1 <= ndim <= APGP_MAX_DIM; the *_len function
 * returns -1 outside them (and for m = 0).  No atomics and a fixed order in every sum: the same input gives the same
 * bits, and a row's results do not depend on the other rows of the call.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
int64_t apgp_predict_grad_work_len(int64_t m, int64_t n);
int apgp_predict_grad(const double* T, int64_t m, const double* xs, int64_t n,
                      const apgp_kernel_t* kern /*host*/, double mean,
                      const double* winv, int64_t ldw, const double* L, int64_t ldl,
                      int32_t kind, const double* lo /*host*/, const double* hi /*host*/, double zeta, double ybest,
                      double* mu, double* var, double* u, double* dmu, double* dvar, double* du,
                      double* work, void* stream);

/* ---- mean-only prediction (the batched ApproxPosterior._gpll path) --------
 * mu_i = k(t_i,X).alpha + mean for m candidates (approx.py:178-180).         */
int apgp_predict_mean(const double* T, int64_t m, const double* xs, int64_t n,
                      const apgp_kernel_t* kern /*host*/, double mean,
                      double* mu, void* stream);

/* Same, from / to HOST buffers in one call (H2D, kernel, D2H, one stream
 * synchronisation): the per-half-step call of an ensemble sampler
 * (approx.py:839-846 -> _gpll, approx.py:178-180) is latency-bound.
 * work: device scratch of m * (ndim + 1) doubles.                            */
int apgp_predict_mean_host(const double* T_host, int64_t m, const double* xs, int64_t n,
                           const apgp_kernel_t* kern /*host*/, double mean,
                           double* mu_host, double* work, void* stream);

/* ---- on-device ensemble MCMC over the GP-mean surrogate ---------------------
 * The whole loop of ApproxPosterior.runMCMC (approx.py:839-846): emcee's stretch
 * move (a = a_stretch, red/blue halves with a random cyclic offset per iteration)
 * with log-probability = GP predictive mean (ApproxPosterior._gpll,
 * approx.py:148-189) and a box prior [lo, hi] (host arrays, required: -inf
 * outside), as one persistent kernel; nensembles independent ensembles run as
 * one workgroup each (replicas).  coords: nensembles x nwalkers x ndim, in =
 * initial state, out = final state; logp / naccept: nensembles x nwalkers;
 * chain (iterations x nensembles x nwalkers x ndim) and logp_chain may be NULL.
 * nwalkers even, >= 2 ndim, <= 256.  RNG: Philox4x32-10 keyed by seed.         */
/* Round 5: when the ensembles alone leave compute units idle (nensembles x nwalkers / 2 <= CUs, or fewer workgroups per
 * ensemble when not), ONE ensemble runs on several workgroups: each evaluates its share of a half-step's proposals
 * and the log-probabilities are exchanged as data-tagged granules in memory (stream-ordered scratch, slot 4 of
 * csrc/scratch.h); same RNG streams and proposals as the single-workgroup kernel, GP means summed in another order
 * (chains agree to rounding, not bit for bit).  All workgroups must be resident at once; if they are not within
 * 50 ms the launch writes NaN into logp[] -- the caller re-runs with apgp_ensemble_mode(1) (the Python wrapper does).
 * apgp_ensemble_mode: 0 = default, 1 = single-workgroup kernel only; < 0 queries; returns the previous value.   */
int apgp_ensemble_mode(int mode);
/* apgp_ensemble_sample with the kernel chosen for THIS call (0: several workgroups per ensemble where
 * that helps, 1: the single-workgroup kernel, < 0: the process-wide switch).  Round 6: a workgroup
 * that gives up also raises a sticky word of the launch, and a one-workgroup kernel behind it turns
 * that word into NaN in ALL of logp[] -- the marker cannot be overwritten by a workgroup that finishes
 * normally afterwards.                                                                                */
int apgp_ensemble_sample_ex(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                            const double* lo /*host, MAX_DIM*/, const double* hi /*host, MAX_DIM*/,
                            int32_t nwalkers, int32_t nensembles, int64_t iterations, double a_stretch,
                            uint64_t seed, double* coords, double* logp, double* chain,
                            double* logp_chain, int64_t* naccept, int mode, void* stream);
int apgp_ensemble_sample(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                         const double* lo /*host*/, const double* hi /*host*/,
                         int32_t nwalkers, int32_t nensembles, int64_t iterations,
                         double a_stretch, uint64_t seed,
                         double* coords, double* logp, double* chain, double* logp_chain,
                         int64_t* naccept, void* stream);

/* Ensemble moves: the sampler with a table of red/blue moves instead of the stretch move alone.  One entry of the
 * table is chosen per iteration for the whole ensemble (both half-steps) with probability weight / sum of weights.
 *   STRETCH  p0 = a > 1:                      q = c_j - (c_j - s) zz, zz = ((a - 1) u + 1)^2 / a, factor (D - 1) log zz
 *   DE       p0 = sigma >= 0, p1 = gamma0 > 0 (0: the default 2.38 / sqrt(2 ndim)):
 *                                             q = s + gamma0 (1 + sigma n) (c_j - c_k), n ~ N(0, 1), j != k; factor 0
 *   SNOOKER  p0 = gammas > 0:                 q = s + gammas (e . (c_k - c_l)) e, e = (s - c_j) / |s - c_j|, j, k, l
 *                                             distinct; factor (ndim - 1) (log|q - c_j| - log|s - c_j|)
 * s: the walker, c_*: walkers of the other half, positions taken in the kernel's scaled coordinates; a DE or snooker
 * proposal with a non-finite coordinate is rejected.  DE needs nwalkers >= 4, the snooker nwalkers >= 6.  The random
 * numbers (csrc/ens_moves.h) are functions of (seed, ensemble, iteration, half-step, slot); an iteration that takes the
 * stretch move draws what apgp_ensemble_sample draws in that iteration.
 * apgp_ensemble_sample_moves is apgp_ensemble_sample_ex with the table moves[0..nmoves) (host, 1 <= nmoves <=
 * APGP_ENS_MAX_MOVES; weights and parameters finite and in the ranges above, else -1); moves == NULL with nmoves == 0
 * is the one-entry table {STRETCH, 1, a_stretch}, which is what apgp_ensemble_sample and _ex run; a_stretch is not
 * read otherwise.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
#define APGP_ENS_MOVE_STRETCH 0
#define APGP_ENS_MOVE_DE 1
#define APGP_ENS_MOVE_SNOOKER 2
#define APGP_ENS_MAX_MOVES 8
typedef struct apgp_ens_move {
    int32_t kind;           /* APGP_ENS_MOVE_* */
    double weight, p0, p1;
} apgp_ens_move_t;
int apgp_ensemble_sample_moves(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                               const double* lo /*host, MAX_DIM*/, const double* hi /*host, MAX_DIM*/,
                               int32_t nwalkers, int32_t nensembles, int64_t iterations, double a_stretch,
                               uint64_t seed, double* coords, double* logp, double* chain,
                               double* logp_chain, int64_t* naccept, int mode,
                               const apgp_ens_move_t* moves /*host*/, int32_t nmoves, void* stream);

/* Parallel tempering: nladders independent ladders of ntemps ensembles ("rungs") each.  Rung k of ladder l is ensemble
 * e = l ntemps + k; it targets exp(betas[k] mu) on the box, betas (host) finite, in [0, 1] and not increasing.
 *   Moves: exactly those of apgp_ensemble_sample_moves for ensemble e -- the same keys (k1 ^= e 0x9E3779B9), the same
 *     counters with the GLOBAL iteration number, the same proposals; moves == NULL with nmoves == 0 is the stretch move
 *     at a = 2.  The kernel keeps two values per walker, mu and the tempered value beta mu, which is -inf wherever mu
 *     is not finite, at every beta (0 included); the accept step is the ensemble sampler's, fed the tempered values.
 *     beta = 1 multiplies exactly: a beta = 1 rung makes the decisions apgp_ensemble_sample_moves(mode = 1) makes, bit
 *     for bit.
 *   Exchanges: round r = 0, 1, ... follows every swap_every iterations, except after the last.  It pairs rungs
 *     (k, k + 1) with k = r (mod 2); an unpaired top or bottom rung sits the round out.  Walker i of rung k is exchanged
 *     with walker i of rung k + 1 iff both mu are finite and log u < (beta_k - beta_{k+1}) (mu_{k+1,i} - mu_{k,i}), u =
 *     u01 of Philox words 0, 1 under the keys of ensemble l ntemps + k with counter (r, r >> 32, i, 7).  Coordinates and
 *     mu move together; naccept stays with the rung.
 *   Outputs: coords (L x T x W x D, in = initial state, out = final state), logp (L x T x W: the final UNtempered mu),
 *     naccept (L x T x W); chain (iterations x L x nstore x W x D, the first nstore rungs of every ladder; may be NULL,
 *     0 <= nstore <= ntemps); logp_chain (iterations x L x T x W: untempered mu of ALL rungs, may be NULL); swap_prop /
 *     swap_acc (L x (T - 1), required for ntemps > 1): exchanges proposed (both mu finite) and accepted per pair;
 *     swap_log (uint8, rounds x L x (T - 1) x W with rounds = ceil(iterations / swap_every) - 1, may be NULL): every
 *     decision, 0 = not proposed, 1 = rejected, 2 = accepted.
 *   Schedule: one launch per segment of swap_every iterations, a workgroup per (ladder, rung), nothing waits inside a
 *     launch and the call enqueues every launch without synchronising.  State passes between launches through two
 *     halves of work (device, apgp_tempered_work_len doubles; -1 for sizes the call refuses) in the kernel's scaled
 *     coordinates.  Not to be called twice at once with the same work.
 * -1 before anything reaches the device: every check of apgp_ensemble_sample_moves; ntemps outside 1 ..
 * APGP_PT_MAX_TEMPS; betas not finite, outside [0, 1] or increasing; beta = 0 with an infinite box edge; swap_every < 1;
 * nstore outside 0 .. ntemps; nladders ntemps beyond the grid limit 2^31 - 1.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
#define APGP_PT_MAX_TEMPS 64
int64_t apgp_tempered_work_len(int32_t nwalkers, int32_t ntemps, int32_t nladders, int32_t ndim);
int apgp_tempered_sample(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                         const double* lo /*host, MAX_DIM*/, const double* hi /*host, MAX_DIM*/,
                         int32_t nwalkers, int32_t ntemps, int32_t nladders, const double* betas /*host, ntemps*/,
                         int64_t iterations, int64_t swap_every, uint64_t seed, double* coords, double* logp,
                         double* chain, int32_t nstore, double* logp_chain, int64_t* naccept, int64_t* swap_prop,
                         int64_t* swap_acc, uint8_t* swap_log, const apgp_ens_move_t* moves /*host*/, int32_t nmoves,
                         double* work, void* stream);

/* ---- Hamiltonian Monte Carlo over the GP-mean surrogate, whole chains on the device (csrc/hmc.hip) ----------------
 * nchains independent chains sample the target of apgp_ensemble_sample -- density exp(mu) on the box [lo, hi], edges may
 * be infinite, the box only gates -- with the exact gradient of the predictive mean, which reuses the mean's N kernel
 * values.  All positions below are in the kernel's scaled coordinates q = theta sc, sc_d = sqrt(inv_metric_d / 2).
 *   One iteration of chain c, global number i = iteration0 + it, Philox4x32-10 under the keys
 *   (seed, seed >> 32 ^ c 0x9E3779B9):
 *     momentum  p_d = sqrt(-2 log u) cospi(2 u') sqrt(mass_d), (u, u') = u01 of words (0, 1), (2, 3) of counter
 *               (i, i >> 32, d, 8);
 *     step      eps_i = eps (1 + jitter (2 u - 1)), u = u01 of words 0, 1 of counter (i, i >> 32, 0xffffffff, 9) under
 *               the keys of chain 0: one draw per iteration, the same for all chains;
 *     nleap leapfrog steps, each  p += (eps_i / 2) g(q);  q += eps_i p / mass;  reflect;  p += (eps_i / 2) g(q),
 *               g = d mu / d q (the kick between two steps is two half kicks: a step is a function of (q, p) alone);
 *     reflect   while q_d lies outside a finite face: q_d = 2 face - q_d, p_d = -p_d, at most 8 times; still outside
 *               then, or q or p not finite: the trajectory is a divergence.  Infinite faces never reflect;
 *     accept    dH = (K(p_L) - mu(q_L)) - (K(p_0) - mu(q_0)), K = sum_d p_d^2 (0.5 / mass_d); accepted iff log u < -dH,
 *               u = u01 of words 0, 1 of counter (i, i >> 32, 0xfffffffe, 10).  dH not finite or > 1000: rejected and
 *               counted in ndiverge.  A start outside the box has mu = -inf: the chain never moves, naccept = 0.
 *   A chain's draws depend on (seed, c, i) only: not on nchains, and not on where a run was cut into calls (feed the
 *   next call the previous coords and iteration0 + iterations).
 *   mass is diagonal, in scaled coordinates; all ones makes the GP's own length scales the preconditioner.
 *   Outputs (device): coords (C x D, in = start, out = final state; a chain that accepted nothing keeps its bits), logp
 *     (C: final mu, -inf outside the box), naccept, ndiverge (C), accprob (C: sum over the iterations of
 *     min(1, exp(-dH)), 0 for a divergence); may be NULL: chain (iterations x C x D), logp_chain (iterations x C), prop
 *     (iterations x C x D: the end of every trajectory, accepted or not; NaN where the trajectory left the box for good
 *     or stopped being finite), dH (iterations x C), trace (iterations x C x
 *     nleap x 2 D: q then p after every step, in SCALED coordinates, the kernel's own bits).
 *   iterations == 0 leaves coords and writes logp.
 *   Schedule: g_rows wavefronts share a chain (their lanes stride the training rows; fixed-order sums, no atomics: the
 *     same inputs and g_rows give the same bits); offered: 1 and 4 (a workgroup is 4 wavefronts); 0 = the library's rule
 *     (apgp_hmc_rule reports it).  One launch, nothing waits, the call does not synchronise.
 * -1 before anything reaches the device: a NULL among xs, kern, lo, hi, opt, coords, logp, naccept, accprob, ndiverge;
 * n outside 1 .. 2^24; nchains outside 1 .. 2^24; iterations outside 0 .. 2^40; bad kernel parameters; eps not finite or
 * <= 0; jitter outside [0, 1); nleap outside 1 .. APGP_HMC_MAX_LEAP; g_rows not offered; iteration0 < 0; a mass not
 * finite or <= 0; lo > hi (or NaN); a trace of more than 2^63 bytes.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
#define APGP_HMC_MAX_LEAP 1024
typedef struct apgp_hmc_options {
    double eps, jitter;        /* step in scaled coordinates, > 0; 0 <= jitter < 1 */
    int32_t nleap;             /* 1 .. APGP_HMC_MAX_LEAP */
    int32_t g_rows;            /* 0 = the rule, else wavefronts per chain */
    int64_t iteration0;        /* global number of the call's first iteration */
    double mass[APGP_MAX_DIM]; /* diagonal mass, scaled coordinates, finite > 0 */
} apgp_hmc_options_t;
int apgp_hmc_sample(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                    const double* lo /*host, MAX_DIM*/, const double* hi /*host, MAX_DIM*/, int32_t nchains,
                    int64_t iterations, const apgp_hmc_options_t* opt /*host*/, uint64_t seed,
                    double* coords, double* logp, double* chain, double* logp_chain, int64_t* naccept, double* accprob,
                    int64_t* ndiverge, double* prop, double* dH, double* trace, void* stream);
/* g_rows the rule picks for these sizes on the current device; -1 for sizes the call refuses, -2 without a device */
int apgp_hmc_rule(int32_t nchains, int64_t n, int32_t ndim);

/* ---- nested sampling over the GP-mean surrogate, whole runs on the device (csrc/nested.hip) ------------------------
 * The evidence Z = V int L dU of the likelihood L = exp(mu) under the uniform measure U on the FINITE box [lo, hi] (V its
 * volume: the measure of the box proposal of apgp_importance_pass's callers), by nruns independent runs of nested
 * sampling with a constrained differential-evolution step sampler.  Nothing is tuned from outside: no proposal, no
 * ladder, no step size.  Positions are kept in the caller's coordinates th; the kernel evaluates at q = th sc,
 * sc_d = sqrt(inv_metric_d / 2).  Run r draws from Philox4x32-10 under the keys (seed, seed >> 32 ^ r 0x9E3779B9): its
 * output does not depend on nruns.  u01 is the 53-bit uniform of two words.
 *   start    live point w, dimension d: th = min(fma(hi_d - lo_d, u, lo_d), hi_d), u = u01 of words (0, 1) for even d,
 *            (2, 3) for odd d, of counter (w, d / 2, 0, 11).  logL = mu(th sc) summed in the order of the
 *            single-workgroup ensemble kernel: the bits apgp_ensemble_sample(iterations = 0, mode = 1) writes into logp
 *            for the same coordinates (a NaN would be stored as -inf).  Birth threshold -inf.
 *   batch b = 0, 1, ...: the live points are ordered ascending by (logL, slot).  The first `batch` die; L* is the logL
 *            of the last of them.  Dead point i (i = 0 .. batch - 1 in that order) is written to row b batch + i with
 *            its logL, its birth threshold and rec = b.  The survivors, j = 0 .. S - 1 in the same order (S = nlive -
 *            batch), are frozen for the batch.  Walker i refills the slot of dead point i:
 *              start  survivor word 0 % S of counter (b, 0xffffffff, i, 12);
 *              step s = 0 .. nsteps - 1: a = word 0 % S, k = word 1 % (S - 1), k += (k >= a) of counter (b, s, i, 13);
 *                     n = sqrt(-2 log u) cospi(2 u'), (u, u') = u01 of words (0, 1), (2, 3) of counter (b, s, i, 14);
 *                     gamma = gamma0 (1 + sigma n);  q' = fma(gamma, th_a sc - th_k sc, q);  th' = q' / sc;
 *                     q'' = th' sc (every operation rounded once).  Accepted iff every th'_d is finite and inside
 *                     [lo_d, hi_d] and mu(q'') > L*; then (th, q, logL) = (th', q'', mu(q'')).  mu is evaluated, and
 *                     counted in ncall, only for a proposal inside the box.  The proposal is symmetric: the walk
 *                     leaves the uniform law on {L > L*} invariant.
 *              The walker's end point takes the dead slot with birth threshold L*.  A walker that accepted nothing is
 *              a copy of its start point: it is kept and counted in nstuck.
 *            One lane keeps logX_b and logZ_b over the dead points: per dead point i of a batch, n = nlive - i,
 *            logZ = logaddexp(logZ, logL + logX + log(1 - exp(-1 / n))), logX -= 1 / n.
 *   stop     before batch b >= 1 if dlogz > 0 and logaddexp(logZ, Lmax + logX) - logZ < dlogz, Lmax the largest live
 *            logL; and at b = max_batches.  dlogz = 0: at max_batches only.  The nlive live points are then written
 *            ascending to rows nb batch ..., rec = -1 (nb = batches done).
 *   gamma0 = 0 is the default 2.38 / sqrt(2 ndim), the one of APGP_ENS_MOVE_DE.  Tags 11 - 14 are this entry's; 1 - 10
 *   and the candidate tag belong to the entries above.
 *   Outputs (device), cap = nlive + batch max_batches rows per run, rows past nb batch + nlive are not written: points
 *     (nruns x cap x ndim), logl, birth (nruns x cap), rec (int32, nruns x cap), counts (int64, nruns x 4: nb, likelihood
 *     calls with the nlive start values, accepted steps, stuck walkers), logz (nruns x 2: logZ and logX over the dead
 *     points when the run stopped; the live points' share is the host's to add); may be NULL: trace (nruns x
 *     max_batches x batch x nsteps x (ndim + 2): per step th', then mu(q'') -- NaN where th' left the box and mu was not
 *     evaluated -- then 1 for accepted, 0 for not; rows of batches not run are not written).  work (device,
 *     apgp_nested_work_len doubles, -1 for sizes the call refuses) holds the live sets; not to be shared by two calls
 *     at once.
 *   Schedule: one launch, one workgroup of 16 wavefronts per run, a wavefront per walker (so batch <= 16).  Nothing is
 *     exchanged between workgroups, nothing spins or waits; every loop is bounded by max_batches, batch, nsteps, nlive
 *     or the training rows.  The order is a fixed-sequence bitonic sort: the same inputs give the same bits.  The
 *     training stream is staged in LDS when it fits 96 KiB (apgp_nested_xlds: 1, else 0 and it is read from L2; -1 for
 *     sizes the call refuses).  The call does not synchronise.
 * -1 before anything reaches the device: a NULL pointer; n outside 1 .. 2^24; bad kernel parameters; nlive outside
 * 4 .. 4096; nlive < 2 batch; batch outside 1 .. 16; nsteps outside 1 .. 2^20; max_batches outside 1 .. 2^24; nruns
 * outside 1 .. 2^20; dlogz, sigma or gamma0 negative or not finite; a box edge not finite or lo >= hi; outputs of more
 * than 2^63 bytes.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                   */
int64_t apgp_nested_work_len(int32_t ndim, int32_t nlive, int32_t nruns);
int apgp_nested_xlds(int64_t n, int32_t ndim);
int apgp_nested_sample(const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                       const double* lo /*host, MAX_DIM*/, const double* hi /*host, MAX_DIM*/, int32_t nlive,
                       int32_t batch, int32_t nsteps, int32_t max_batches, double dlogz, double sigma, double gamma0,
                       int32_t nruns, uint64_t seed, double* work, double* points, double* logl, double* birth,
                       int32_t* rec, int64_t* counts, double* logz, double* trace, void* stream);

/* ---- candidate matrix of the sweep drawn on the device (round 5, opt-in) ------
 * The batched counterpart of the ``sampleFn`` draws utility.minimizeObjective starts from
 * (utility.py:334-338) when the prior is the box: T (m x ndim, device) row i =
 * lo + (hi - lo) * u(seed, idx_offset + i), u = 53-bit uniforms in (0, 1) from counter-based
 * Philox4x32-10 (counter = (row low, row high, d / 2, "CAND"), key = seed).  Row g of the global
 * matrix depends on (seed, g) only: a rank of a sharded sweep generates its own rows with
 * idx_offset = first row, and any rank regenerates the winning row alone.               */
int apgp_box_candidates(double* T, int64_t m, int32_t ndim, const double* lo /*host*/,
                        const double* hi /*host*/, uint64_t seed, int64_t idx_offset, void* stream);

/* ---- product prior of Uniform and Gaussian factors (priors.JointPrior) ---------
 * One record per dimension (host arrays of ndim entries, 1 <= ndim <= APGP_MAX_DIM):
 *   kind 0 (Uniform):  p0 = low, p1 = high, finite, low < high
 *   kind 1 (Gaussian): p0 = mu,  p1 = sigma, finite, sigma > 0
 * apgp_prior_candidates: T (m x ndim, device) from the stream of apgp_box_candidates -- same
 *   counter, key and pairing of dimensions, so a Uniform dimension is bit-identical to the box
 *   draw of the same row; a Gaussian dimension is mu + (sigma sqrt 2) erfcinv(2 (1 - u)).
 * apgp_prior_lnprior: out[i] (device) = sum_d log-density of row i of X (m x ndim, device);
 *   -inf for a non-finite coordinate or one outside a Uniform factor's [low, high].
 * Bad arguments are refused (-1) before anything reaches the device.                      */
int apgp_prior_candidates(double* T, int64_t m, int32_t ndim, const int32_t* kind /*host*/,
                          const double* p0 /*host*/, const double* p1 /*host*/, uint64_t seed,
                          int64_t idx_offset, void* stream);
int apgp_prior_lnprior(const double* X, int64_t m, int32_t ndim, const int32_t* kind /*host*/,
                       const double* p0 /*host*/, const double* p1 /*host*/, double* out, void* stream);

/* ---- Gaussian-mixture passes (gmmUtils.fitGMM) --------------------------------
 * One pass over X (n x ndim, row-major, device) and a fixed-order reduction into
 * stats_out (device, apgp_gmm_stats_len doubles); no atomics, same bits run to run.
 * params (device, apgp_gmm_params_len doubles): per component k, 2 + D + D(D+1)/2 doubles
 *   [log w_k, log det U_k, c_k (D), U_k packed upper triangle column by column: U[i][j] at j(j+1)/2 + i]
 * with U_k the precision Cholesky factor (precision = U U^T) and c_k the centre.
 * stats_out: [G, then per component (s0, s1 (D), S (D(D+1)/2, packed as U))]
 *   APGP_GMM_EM:     G = sum_rows log_prob_norm, s0 = sum r, s1 = sum r (x - c_k),
 *                    S = sum r (x - c_k)(x - c_k)^T, r the responsibilities of the E-step
 *   APGP_GMM_SCORE:  G only (the rest of stats_out is not written)
 *   APGP_GMM_KMEANS: r = 1 for the nearest centre c_k (lowest k on ties), else 0; G = the
 *                    sum of the squared distances to it (log w, log det and U are not read)
 * row_lp / row_label (device, n each, may be NULL): per row log_prob_norm (k-means: the
 * squared distance) and the most likely (k-means: nearest) component.
 * Limits: 1 <= n < 2^31, 1 <= ndim <= APGP_MAX_DIM, 1 <= ncomp <= 16; the *_len functions
 * return -1 outside them.  Uses per-stream scratch (apgp_release_scratch): not during capture. */
#define APGP_GMM_EM 0
#define APGP_GMM_SCORE 1
#define APGP_GMM_KMEANS 2
int64_t apgp_gmm_params_len(int32_t ndim, int32_t ncomp);
int64_t apgp_gmm_stats_len(int32_t ndim, int32_t ncomp);
int apgp_gmm_pass(const double* X, int64_t n, int32_t ndim, int32_t ncomp, const double* params, int32_t mode,
                  double* stats_out, double* row_lp, int32_t* row_label, void* stream);

/* ---- Evidence and posterior moments by importance sampling --------------------------------
 * The surrogate models the unnormalised log-posterior (y = lnlike + lnprior), so Z = int exp(mu(t)) dt over the prior's
 * support is the model evidence.  With M draws t_i from a proposal q and log w_i = mu(t_i) - ln q(t_i), one record of
 * weighted sums gives log Z, its standard error, the effective sample size and the posterior mean and covariance.
 *
 * apgp_mix_candidates: rows idx_offset .. idx_offset + m - 1 of the global matrix of draws from a Gaussian mixture into T
 * (m x ndim, device) and ln q of each STORED row into lnq (m, device, may be NULL).  params (HOST, apgp_mix_params_len
 * doubles): per component k, 3 + D + D(D+1) doubles
 *   [cumw_k, log w_k, log det U_k, c_k (D), U_k packed as apgp_gmm_pass takes it (U[i][j] at j(j+1)/2 + i, i <= j),
 *    A_k packed row by row (A[i][j] at i(i+1)/2 + j, j <= i)]
 * cumw: the cumulative weights, summed sequentially by the caller, the last one forced to 1.0; c_k the centre; A_k the
 * lower Cholesky factor of the covariance (the draw); U_k the precision Cholesky factor (precision = U U^T) and its
 * log-determinant (the density), i.e. entries 1 .. of a component are its apgp_gmm_pass record.
 * A row depends on (seed, global row) only, as in apgp_box_candidates: Philox4x32-10, key = seed, counter (row low, row
 * high, j, "MIXT"); j = 0: u = u01(words 0, 1) picks the first k with u < cumw[k]; j = 1 + d / 2: words 0, 1 / 2, 3 are
 * the uniforms of dimensions d, d + 1, each turned into a standard normal by the inverse-CDF expression of a Gaussian
 * prior factor (sqrt 2 erfcinv(2 (1 - u))); t = c_k + A_k z.  ln q = logsumexp_k(log w_k + log N(t | c_k, Sigma_k)) at the
 * stored t, by the arithmetic of apgp_gmm_pass's score.
 * 1 <= ncomp <= 16, 1 <= ndim <= APGP_MAX_DIM, 0 <= m <= APGP_MAX_M (m = 0: nothing is done); bad arguments -- among
 * them cumulative weights that fall or do not end at 1.0, a non-finite entry, a non-positive diagonal of A -- are refused
 * (-1) before anything reaches the device.  The parameters are uploaded into per-stream scratch (apgp_release_scratch;
 * not during capture) by a copy ordered on `stream` that has completed when the call returns.
 *
 * apgp_importance_pass: for the m rows t of T (m x ndim, device) and lnq (m, device; NULL: zeros), with the surrogate as
 * apgp_predict_mean takes it (xs, n, kern, mean), a gate lo / hi (host, NULL: none) and a centre c (host, ndim doubles):
 *   mu = k(t, X).alpha + mean
 *   logw = mu - lnq   if every coordinate is finite and inside [lo, hi] and mu and lnq are finite, else -inf
 * (a gated row still counts in m).  stats_out (device, apgp_importance_stats_len = 4 + D + D(D+1)/2 doubles):
 *   [lmax, S0, S2, cnt, s1 (D), S (D(D+1)/2, packed as apgp_gmm_pass packs S)]
 *   lmax = max logw (-inf if no row is admissible), e_i = exp(logw_i - lmax), S0 = sum e_i, S2 = sum e_i^2, cnt = the
 *   number of rows with finite logw, s1_d = sum e_i (t_d - c_d), S_de = sum e_i (t_d - c_d)(t_e - c_e).
 * With no admissible row the record is (-inf, 0, 0, 0, zeros).  e_i is 0 where logw_i - lmax < -700.
 * logw_out (m, device, may be NULL) receives logw.  work: apgp_importance_work_len(m) doubles (device).
 * A candidate per thread, APGP_IMP_BLOCK candidates per workgroup, at most APGP_IMP_MAX_BLOCKS workgroups: beyond
 * APGP_IMP_BLOCK * APGP_IMP_MAX_BLOCKS rows a workgroup takes further tiles of candidates.  Each k(t, x) carries the bits
 * of apgp_predict_mean's; the sum over the training rows runs in another order (four interleaved partial sums), so mu
 * agrees with apgp_predict_mean's to rounding, not bit for bit.  No atomics and a fixed order in every sum: the same
 * input gives the same bits, and the record depends on nothing but the inputs and m.
 * 1 <= m <= APGP_MAX_M, 1 <= n <= 2^24; the *_len functions return -1 outside the limits.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                      */
#define APGP_IMP_BLOCK 256
#define APGP_IMP_MAX_BLOCKS 2048
int64_t apgp_mix_params_len(int32_t ndim, int32_t ncomp);
int apgp_mix_candidates(double* T, double* lnq, int64_t m, int32_t ndim, int32_t ncomp, const double* params /*host*/,
                        uint64_t seed, int64_t idx_offset, void* stream);
int64_t apgp_importance_stats_len(int32_t ndim);
int64_t apgp_importance_work_len(int64_t m);
int apgp_importance_pass(const double* T, int64_t m, const double* lnq, const double* xs, int64_t n,
                         const apgp_kernel_t* kern /*host*/, double mean, const double* lo /*host*/,
                         const double* hi /*host*/, const double* centre /*host*/, double* logw_out,
                         double* stats_out, double* work, void* stream);

/* ---- Quasi-random siblings of the three candidate generators (DESIGN.md "Quasi-random draws") ----------------
 * Rows idx_offset .. idx_offset + m - 1 of replicate `replicate` of a scrambled Sobol sequence keyed by `seed`, pushed
 * through the sibling's transform of a uniform: fma(hi - lo, u, lo) for the box and a Uniform factor, mu + (sigma sqrt 2)
 * erfcinv(2 (1 - u)) for a Gaussian factor; for the mixture the Sobol dimensions 0 .. D - 1 give the standard normals,
 * dimension D picks the component (the first k with u < cumw[k]), t = c_k + A_k z and ln q at the stored row follow by
 * apgp_mix_candidates' arithmetic.  Every other argument is the sibling's, checked as the sibling checks it.
 * Point g (0 <= g < 2^30), dimension d: x = XOR over the set bits b of g ^ (g >> 1) of V32[d][b] = V[d][b] << 2, V the
 * Joe-Kuo direction numbers as torch.quasirandom.SobolEngine holds them: x / 2^32 is row g of SobolEngine's draw (row 0 is
 * the origin).  scramble = 1 (nested uniform, hash-based: Laine-Karras as in Burley 2020), per dimension:
 *   x <- rev32(lk(rev32(x), h_d)),  lk(v, h): v += h; v ^= v * 0x6c50b47c; v ^= v * 0xb82f1e52; v ^= v * 0xc7afe638;
 *   v ^= v * 0x8d22f6e6 (uint32),  h_d = word 0 of Philox4x32-10 with counter (d, replicate, 0, 0x534f424c "SOBL"), key = seed.
 * scramble = 0 leaves x alone (seed and replicate then change nothing).  u = (x + 0.5) 2^-32: exact, never 0 or 1.
 * A row depends on (seed, replicate, scramble, global row) only.  Refused (-1) before any launch, besides the sibling's
 * refusals: idx_offset + m > 2^30, replicate < 0, scramble outside {0, 1}.  m = 0: nothing is done.
 * apgp_sobol_direction: V[d][b] (30 bits) of the compiled table, 0 <= d <= 32, 0 <= b <= 29; -1 out of range.  Host only.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                      */
int32_t apgp_sobol_direction(int32_t d, int32_t b);
int apgp_sobol_box_candidates(double* T, int64_t m, int32_t ndim, const double* lo /*host*/, const double* hi /*host*/,
                              uint64_t seed, int32_t replicate, int32_t scramble, int64_t idx_offset, void* stream);
int apgp_sobol_prior_candidates(double* T, int64_t m, int32_t ndim, const int32_t* kind /*host*/,
                                const double* p0 /*host*/, const double* p1 /*host*/, uint64_t seed, int32_t replicate,
                                int32_t scramble, int64_t idx_offset, void* stream);
int apgp_sobol_mix_candidates(double* T, double* lnq, int64_t m, int32_t ndim, int32_t ncomp,
                              const double* params /*host*/, uint64_t seed, int32_t replicate, int32_t scramble,
                              int64_t idx_offset, void* stream);

/* ---- Evidence over posterior function draws (GP.importance_paths, ApproxPosterior.evidence(surrogateDraws=)) ----
 * apgp_importance_pass integrates exp(mu): the surrogate's mean taken for the log-posterior.  apgp_path_importance takes
 * S = ndraws posterior function draws f_s instead -- exactly apgp_path_draws' functions: the same arguments (xs, n, kern,
 * mean, V, Z, b, W, Wl, nfeat, ndraws; V == NULL allowed), the same limits, the same switch apgp_path_draws_mode -- and
 * leaves one importance record per draw, so that the scatter of the records over s is the surrogate's own error bar on
 * the evidence and the moments.  For the m rows t of T (m x ndim, device) and lnq (m, device; NULL: zeros):
 *   logw_s(row) = f_s(t_row) - lnq[row]   if every coordinate is finite and inside [lo, hi] (host, NULL: no box) and
 *                                         f_s and lnq are finite, else -inf
 * (a gated row still counts in m).  Where the row is admissible logw_s is F[s, row] - lnq[row] in one rounded subtraction,
 * F being what apgp_path_draws stores for the same inputs in the same mode, bit for bit: the two share the contraction.
 * stats_out (device, S x apgp_importance_stats_len(ndim)): record s has apgp_importance_pass's layout and definitions,
 *   [lmax, S0, S2, cnt, s1 (D), S packed],
 * about centre (host, ndim finite doubles) over draw s's log-weights: lmax their exact maximum, e = exp(logw - lmax) (0
 * below -700 and for -inf); no admissible row gives (-inf, 0, 0, 0, zeros).  logw_out (S x m row-major, device, may be
 * NULL) receives the log-weights.
 * work (device): apgp_path_importance_work_len(m, ndraws) doubles =
 *   ndraws (ceil(m / 256) + m + 1 + min(ceil(m / APGP_IMP_BLOCK), APGP_IMP_MAX_BLOCKS) (3 + 32 + 528))
 * -- per draw the maxima of the first stage's workgroups, the log-weights (not used with logw_out), the draw's maximum
 * and the partial sums of the moments; -1 beyond the limits, 0 for m < 1 or ndraws < 1.
 * Two stages: the path-draw contraction with a weights epilogue (a candidate per thread, 256 per workgroup), then the
 * moments kernels of apgp_importance_pass with the draw as a grid dimension.  No atomics; every sum runs in a fixed
 * order that depends on (m, ndraws) only: the same input gives the same bits, and a draw's record does not depend on
 * the other draws' weights.
 * Refused (-1) before anything reaches the device: a null T, kern, Z, b, W, centre, stats_out or work; xs null with V
 * not null; lo without hi; Wl null with a linear term; ndraws outside 1 .. APGP_MAX_DRAWS; nfeat outside 1 ..
 * APGP_MAX_FEATURES; m or n below 1 or beyond 2^40 / 2^24; a non-finite centre.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                      */
int64_t apgp_path_importance_work_len(int64_t m, int32_t ndraws);
int apgp_path_importance(const double* T, int64_t m, const double* lnq,
                         const double* xs, int64_t n, const apgp_kernel_t* kern /*host*/, double mean,
                         const double* V, const double* Z, const double* b, const double* W, const double* Wl,
                         int32_t nfeat, int32_t ndraws,
                         const double* lo /*host*/, const double* hi /*host*/, const double* centre /*host*/,
                         double* logw_out /* S x m row-major, may be NULL */,
                         double* stats_out /* S x apgp_importance_stats_len(ndim) */,
                         double* work, void* stream);

/* ---- Chain diagnostics: a block of the walker-averaged autocorrelation function ------------
 * (mcmc.integrated_time(onDevice=True).)  x (device, fp64) is an ensemble chain laid out (steps, n_w, n_d) row-major as
 * GP.sample_ensemble stores it; step t of the series is row row0 + t * row_stride of it (a get_chain(discard=, thin=)
 * view needs no copy), n_t steps in all.  With m_kd the mean over t of x[t,k,d] and
 *   A_kd(l) = sum_{t = 0}^{n_t - l - 1} (x[t,k,d] - m_kd) (x[t+l,k,d] - m_kd),
 * f (device, n_d x nlags row-major) receives
 *   f[d][l - lag0] = (1 / n_w) * sum_k A_kd(l) / A_kd(0)        for lag0 <= l < lag0 + nlags
 * by direct summation (no FFT); a lag l >= n_t has an empty sum, f = 0 there.  A series with A(0) = 0 makes its
 * dimension's f NaN (0/0) and no other.  Partial sums over time chunks are combined in a fixed order that depends on
 * n_t only: no atomics, the same input gives the same bits whatever blocks of lags are asked for.
 * work (device): apgp_autocorr_work_len(n_t, n_w, n_d) doubles.  reuse_stats = 0: the means and A(0) are computed and
 * left in work; reuse_stats != 0: work still holds them from an earlier call on the same x, n_t, row0 and row_stride.
 * Limits: 1 <= n_t, nlags < 2^31, 0 <= lag0, row0 < 2^31, 1 <= row_stride < 2^31, 1 <= n_w <= 2^24,
 * 1 <= n_d <= APGP_MAX_DIM, (row0 + (n_t - 1) row_stride + 1) n_w n_d <= 2^60; apgp_autocorr_work_len returns -1
 * outside them.  Bad arguments are refused (-1) before anything reaches the device.
 * Added in ABI 8 without changing anything before it: APGP_ABI_VERSION stays 8.                                      */
int64_t apgp_autocorr_work_len(int64_t n_t, int64_t n_w, int32_t n_d);
int apgp_autocorr_block(const double* x, int64_t n_t, int64_t n_w, int32_t n_d, int64_t row0, int64_t row_stride,
                        int64_t lag0, int64_t nlags, int32_t reuse_stats, double* work, double* f, void* stream);

/* ---- K4: gradient of the log-likelihood wrt kernel hyper-parameters -------
 * Replaces george GP.grad_log_likelihood (gpUtils._grad_nll, gpUtils.py:110):
 *   g_k = 0.5 * sum_ij (alpha alpha^T - K^-1)_ij dK_ij/dtheta_k.
 * winv/ldw: the dense L^-1 that apgp_trtri_pack leaves in the first panel of
 * its work buffer (ldw = n rounded up to 64).  work: apgp_grad_work_len(n)
 * doubles (K^-1 = W^T W is formed there).  out (device, 2+ndim doubles):
 *   out[0] = sum(alpha) (d/d mean), out[1] = d/d log_constant (amp part),
 *   out[2+d] = d/d log_M_d_d (d < ndim),
 *   out[2+APGP_MAX_DIM] = 0.5 * trace(alpha alpha^T - K^-1): times exp(white_noise)
 *   it is d/d white_noise (george fit_white_noise=True),
 *   out[3+APGP_MAX_DIM] = 0.5 * sum_ij (alpha alpha^T - K^-1)_ij K_lin_ij: d/d log_constant
 *   of the linear term, and minus d/d log_gamma2.  out: 4 + APGP_MAX_DIM doubles.   */
int64_t apgp_grad_work_len(int64_t n);
/* K^-1 by the SOLVE route, for factors whose explicit inverse must not be trusted (the host's
 * conditioning gate): what george does -- K^-1 = cho_solve(L, I) inside grad_log_likelihood
 * (gpUtils.py:110) -- two blocked triangular solves against the identity, no product of
 * inverses.  xwork: apgp_kinv_solve_work_len(n) doubles; kinv: n x n (ld n), the lower
 * 64 x 64 tiles are written -- pass it as apgp_grad_loglik's `work` with winv = NULL.       */
int64_t apgp_kinv_solve_work_len(int64_t n);
int apgp_kinv_solve(const double* L, int64_t n, int64_t ldl, double* xwork, double* kinv, void* stream);
/* winv == NULL: `work` already holds K^-1 (apgp_kinv_solve); otherwise K^-1 = W^T W is formed there. */
int apgp_grad_loglik(const double* X, const double* alpha, const double* winv, int64_t ldw,
                     int64_t n, const apgp_kernel_t* kern /*host*/,
                     double* work, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APGP_H */
