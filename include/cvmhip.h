/*
 * cvmhip.h -- C ABI of libcvmhip.so: the MI355X (gfx950) implementation of the cvmatrix
 * per-fold training-matrix hot path.
 *
 * The reference (sm00thix/cvmatrix v3.2.1) has no FFI of its own: its seam is the array
 * namespace chosen by `_resolve_backend` (cvmatrix/cvmatrix.py:58-96) and used through
 * `self.xp` by the private methods of `CVMatrix`.  The two entry points below replace,
 * for a backend literal "hip", exactly the two fused stages behind that seam:
 *
 *   cvm_gram_fit     <- CVMatrix.fit(): _init_weighted_mats, _init_matrix_products,
 *                       _init_stats                      (cvmatrix.py:1193-1243)
 *   cvm_fold_update  <- CVMatrix._training_matrices / training_statistics for a BATCH of
 *                       folds: _get_val_matrices, _compute_training_stats,
 *                       _training_kernel_matrix          (cvmatrix.py:589-1129)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed / torch-ROCm storage) unless it is
 *     named host_*; row-major, contiguous, no strides;
 *   - the library never allocates or frees device memory and keeps no pointer after a
 *     call returns; scratch comes from the caller's workspace `ws`;
 *   - calls enqueue work on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) and return without synchronising;
 *   - return value: CVM_OK or a CVM_E* code; cvm_last_error() gives the text for the
 *     calling thread;
 *   - dtype: CVM_F64 or CVM_F32 (the reference accepts any NumPy float; f16/f128 are not
 *     offered on the device).  Column statistics are always kept in float64.
 *   - results are deterministic: no floating-point atomics, fixed-order reductions;
 *   - threads: every entry point may be called concurrently from several host threads (one
 *     per stream / device is the intended use).  The library's only process-wide state is the
 *     optional launch-timing recorder below (mutex-guarded), once-per-device kernel
 *     attributes (atomic flags) and one 1 MiB device allocation per device, made on first use
 *     and kept (1024 work-queue blocks of the persistent Gram kernel, one per stream that uses
 *     it, handed out under a mutex and RECYCLED: when all are taken, the least recently used
 *     block whose last Gram launch is over -- by an event the library itself recorded behind
 *     that launch, once the process has used more than 64 streams on the device; never by a
 *     query of a foreign stream handle -- changes hands, so a service may create and destroy
 *     streams without bound); the optional clock-probe buffer and forced split plan are single
 *     atomic words; planning depends on the arguments alone.
 */
#ifndef CVMHIP_H
#define CVMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVM_OK 0
#define CVM_EINVAL 1   /* bad argument */
#define CVM_EWORKSPACE 2 /* workspace too small */
#define CVM_ELAUNCH 3  /* HIP launch / runtime error */

#define CVM_F32 0
#define CVM_F64 1

/* flags for cvm_fold_update (cvmatrix.py:157-163 constructor flags + what to return) */
#define CVM_RET_XTX 0x01u
#define CVM_RET_XTY 0x02u
#define CVM_CENTER_X 0x04u
#define CVM_CENTER_Y 0x08u
#define CVM_SCALE_X 0x10u
#define CVM_SCALE_Y 0x20u
/* cvm_fold_update only: `idx` and `offsets` are HOST pointers.  For one fold of at most 32 rows
 * (the reference's call pattern in leave-one-out: one training_XTX_XTY(validation_indices) per
 * sample, cvmatrix.py:451-517): the indices travel inside the kernel arguments and no device
 * copy of the index array is made. */
#define CVM_IDX_HOST 0x40u

const char *cvm_version(void);
/* sha256 (first 16 hex digits) over the source files the library was built from, as computed by
 * cvmatrix_amd/build.py; the Python loader refuses (or rebuilds) a library whose hash differs from
 * the sources lying next to it. */
const char *cvm_source_hash(void);
const char *cvm_last_error(void);

/* Number of float64 entries of the global statistics vector written by cvm_gram_fit and
 * read by cvm_fold_update:  [ sX(K) | qX(K) | sY(M) | qY(M) | sw | nz ]
 *   sX = sum_i w_i x_i   (cvmatrix.py:1231)      qX = sum_i w_i x_i^2   (1235-1236)
 *   sY = sum_i w_i y_i   (1233)                  qY = sum_i w_i y_i^2   (1240-1241)
 *   sw = sum_i w_i       (1225 / 1228)           nz = #{w_i != 0}       (1226 / 1229)
 * With w == NULL: w_i = 1, sw = nz = N. */
size_t cvm_gstats_len(int K, int M);

/* Workspace (bytes) that lets cvm_gram_fit run N rows in one launch sequence. */
size_t cvm_fit_workspace_bytes(int64_t N, int K, int M, int dtype);

/* Full-data Gram and column statistics (replaces cvmatrix.py:1193-1243).
 *   X [N,K], Y [N,M] or NULL (then M must be 0), w [N] or NULL (unweighted)
 *   G [K,K]  = X^T diag(w) X   (exactly symmetric)
 *   H [K,M]  = X^T diag(w) Y   (untouched if Y == NULL)
 *   gstats   float64[cvm_gstats_len(K,M)] as laid out above
 *   neg_flag int32[1], set to 1 if any w_i < 0 (cvmatrix.py:1188), else 0; may be NULL */
int cvm_gram_fit(const void *X, const void *Y, const void *w, int64_t N, int K, int M,
                 int dtype, void *G, void *H, double *gstats, int32_t *neg_flag,
                 void *ws, size_t ws_bytes, void *stream);

/* Workspace (bytes) recommended for a cvm_fold_update call: with it all folds are
 * processed in one batch.  A smaller workspace is legal as long as it holds one fold;
 * the call then walks the folds in several batches. */
size_t cvm_fold_workspace_bytes(int64_t n_folds, int64_t n_idx, int64_t max_fold_rows,
                                int K, int M, int dtype, unsigned flags);

/* Training-set matrices for a batch of folds (replaces, per fold, cvmatrix.py:754-896).
 *   idx      int64[n_idx]      validation row numbers of all folds, concatenated
 *                              (each in [0,N); duplicates are subtracted twice, as
 *                              NumPy fancy indexing would)
 *   offsets  int64[n_folds+1]  DEVICE: fold f owns idx[offsets[f] .. offsets[f+1])
 *   host_offsets               the same array in HOST memory (sizes the launch)
 *   G,H,gstats                 outputs of cvm_gram_fit (replicated on every GPU)
 *   ddof, resolution           cvmatrix.py:172, 187
 * outputs (any may be NULL if not wanted; *_XTX needs CVM_RET_XTX etc.):
 *   out_XTX [n_folds,K,K], out_XTY [n_folds,K,M]           dtype
 *   out_muX,out_sdX [n_folds,K], out_muY,out_sdY [n_folds,M]  dtype
 *   out_fold float64[n_folds,4] = { sw_train, nz_train, sw_val, nz_val }
 * The kernels never raise: the caller turns nz_train == 0 / nz_train <= ddof into the
 * reference's ValueErrors (cvmatrix.py:625-629, 1074-1078).  Statistics are computed
 * whenever a centre/scale flag asks for them (same conditions as cvmatrix.py:828-831);
 * un-requested statistic outputs are left untouched. */
int cvm_fold_update(const void *X, const void *Y, const void *w, const int64_t *idx,
                    const int64_t *offsets, const int64_t *host_offsets,
                    int64_t n_folds, int64_t N, int K, int M, int dtype, unsigned flags,
                    double ddof, double resolution, const void *G, const void *H,
                    const double *gstats, void *out_XTX, void *out_XTY, void *out_muX,
                    void *out_sdX, void *out_muY, void *out_sdY, double *out_fold,
                    void *ws, size_t ws_bytes, void *stream);

/* cvm_fold_update with a status word (the reference's contract is "raise or return correct numbers",
 * cvmatrix.py:625-629, 1074-1078: this is how a caller proves the second half).
 *   status   DEVICE int32[1], zeroed by the caller before the call, or NULL.
 * One route of the fold stage -- mid-size folds that form their statistics inside the Gram launch -- lets
 * work items wait for flags that other items of the same launch raise.  The wait is bounded; an item whose
 * wait gives up writes nothing and is recomputed by a second launch of the same call once every flag is up.
 * Behind the call (on `stream`):  *status == 0  nothing gave up;  2  some items were recomputed, every output
 * is valid;  1  an item gave up in the second launch too (not possible by the kernel's own logic: a fault) and
 * its outputs hold NaN.  Every other route leaves *status untouched. */
int cvm_fold_update_ex(const void *X, const void *Y, const void *w, const int64_t *idx,
                       const int64_t *offsets, const int64_t *host_offsets,
                       int64_t n_folds, int64_t N, int K, int M, int dtype, unsigned flags,
                       double ddof, double resolution, const void *G, const void *H,
                       const double *gstats, void *out_XTX, void *out_XTY, void *out_muX,
                       void *out_sdX, void *out_muY, void *out_sdY, double *out_fold,
                       void *ws, size_t ws_bytes, void *stream, int32_t *status);

/* One-sweep cross-validation (no counterpart in the reference).  When the
 * folds PARTITION the rows -- every row of X in exactly one fold, as the reference's own
 * benchmark and README build them (benchmarks/benchmark.py:232, README.md:120-141) -- the
 * full-data matrices of cvm_gram_fit are the sum of the folds' validation matrices.
 *   cvm_sweep_fit    runs the Gram kernel once over all folds (rows gathered by idx), writes
 *                    G, H, gstats, neg_flag like cvm_gram_fit (as the sum over the folds of each
 *                    fold's own sum over its row splits) and leaves the per-fold partials in ws; *splits_out receives an
 *                    opaque token (the row-split plan) to be handed back to cvm_sweep_folds
 *   cvm_sweep_folds  = the finalize half of cvm_fold_update on those partials (same outputs),
 *                    valid while ws is untouched; `weighted` = 1 if cvm_sweep_fit got w != NULL
 * Together they do half the arithmetic of cvm_gram_fit + cvm_fold_update.  The caller
 * checks the partition property; ws must hold all folds (cvm_sweep_workspace_bytes). */
size_t cvm_sweep_workspace_bytes(int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype);
int cvm_sweep_fit(const void *X, const void *Y, const void *w, const int64_t *idx,
                  const int64_t *offsets, const int64_t *host_offsets, int64_t n_folds, int64_t N,
                  int K, int M, int dtype, void *G, void *H, double *gstats, int32_t *neg_flag,
                  void *ws, size_t ws_bytes, void *stream, int64_t *splits_out);
int cvm_sweep_folds(const int64_t *offsets, int64_t n_folds, int K, int M, int dtype, unsigned flags,
                    double ddof, double resolution, int weighted, const void *G, const void *H,
                    const double *gstats, void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX,
                    void *out_muY, void *out_sdY, double *out_fold, void *ws, size_t ws_bytes,
                    int64_t splits, void *stream);

/* cvm_sweep_fit followed by cvm_sweep_folds over all folds, as one call (same arguments, same
 * results to the bit, the partials stay in ws for cvm_sweep_fold_range).  With at most 16 folds
 * and 16-byte aligned rows the finalize half runs as one launch that reads every partial once:
 * a fold's update stays on chip while the full-data matrix is formed as the sum of the
 * folds' updates. */
int cvm_sweep_all(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                  const int64_t *host_offsets, int64_t n_folds, int64_t N, int K, int M, int dtype, unsigned flags,
                  double ddof, double resolution, void *G, void *H, double *gstats, int32_t *neg_flag,
                  void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX, void *out_muY, void *out_sdY,
                  double *out_fold, void *ws, size_t ws_bytes, void *stream, int64_t *splits_out);

/* The same for folds [fold0, fold0 + n_folds) of the n_total folds of the sweep; outputs are written
 * from index 0.  Serves the reference's one-call-per-fold loop (README.md:120-141) from the sweep's
 * partials: training_XTX_XTY(p.get_validation_indices(fold)) then costs two small finalize kernels. */
int cvm_sweep_fold_range(const int64_t *offsets, int64_t n_total, int64_t fold0, int64_t n_folds, int K, int M,
                         int dtype, unsigned flags, double ddof, double resolution, int weighted, const void *G,
                         const void *H, const double *gstats, void *out_XTX, void *out_XTY, void *out_muX,
                         void *out_sdX, void *out_muY, void *out_sdY, double *out_fold, void *ws, size_t ws_bytes,
                         int64_t splits, void *stream);

/* Training matrices of the complements of UNIONS of folds of the sweep (nested cross-validation,
 * repeated leave-several-groups-out): output u is what cvm_fold_update gives for the concatenated
 * validation indices of the folds of union u (cvmatrix.py:754-896), formed from the partials the sweep
 * left in sweep_ws as  G - sum_{f in S_u} U_f  -- no row of X is read again.
 *   fold_offsets, n_total, weighted, sweep_ws, splits   as in cvm_sweep_fold_range; sweep_ws is only
 *               read: the call may run any number of times after one sweep, between calls of
 *               cvm_sweep_fold_range
 *   union_folds        device int64[host_union_offsets[n_unions]]: union u owns
 *                      union_folds[union_offsets[u] .. union_offsets[u+1]), fold numbers in
 *                      [0, n_total), strictly ascending inside a union (the caller guarantees it)
 *   union_offsets      device int64[n_unions+1]; host_union_offsets: the same array on the host
 *   outputs            as in cvm_sweep_fold_range, leading axis = union;
 *                      out_fold[u] = {sw_train, nz_train, sw_val, nz_val} of the union
 *   ws                 this call's own scratch (cvm_sweep_unions_workspace_bytes): the unions'
 *                      statistics vectors; what it held before does not matter
 * The folds of a union are summed in ascending order, each fold's own ordered sum over its row splits
 * first: the bits of a union's outputs depend on its folds, the partials and the token alone, and a
 * union of one fold has the bits cvm_sweep_fold_range gives that fold.  No atomics.  CVM_EINVAL (bad
 * token, missing pointer, n_unions < 0, negative / decreasing host_union_offsets, a union of no fold)
 * and CVM_EWORKSPACE (ws or sweep_ws too short) are decided before the device is touched; n_unions == 0
 * launches nothing. */
size_t cvm_sweep_unions_workspace_bytes(int64_t n_unions, int K, int M);
int cvm_sweep_unions(const int64_t *fold_offsets, int64_t n_total,
                     const int64_t *union_folds, const int64_t *union_offsets,
                     const int64_t *host_union_offsets, int64_t n_unions,
                     int K, int M, int dtype, unsigned flags, double ddof, double resolution, int weighted,
                     const void *G, const void *H, const double *gstats,
                     void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX, void *out_muY, void *out_sdY,
                     double *out_fold, const void *sweep_ws, size_t sweep_ws_bytes, int64_t splits,
                     void *ws, size_t ws_bytes, void *stream);

/* Streaming cross-validation: the folds' raw updates accumulated over ROW CHUNKS, for data that is larger
 * than device memory or arrives in batches (no reference counterpart: cvmatrix.py's fit takes all rows at
 * once, :207-328).  Every quantity the fold stage reads -- U_f = X_f^T W X_f | X_f^T W Y_f, the column
 * sums, sw_f, nz_f -- is a sum over rows, hence over chunks.
 *   accumulator   device, cvm_stream_workspace_bytes(CVM_STREAM_ACCUMULATOR, ..) bytes, 16-byte aligned:
 *                 one float64 unit per fold (both dtypes) and behind the units the statistics region
 *                 cvm_sweep_fold_range carves
 *   state         host int64[CVM_STREAM_STATE_LEN]: the stream's header (shape it was reset with, chunks
 *                 and rows added); the caller keeps it next to the accumulator and does not edit it
 * cvm_stream_reset  zeroes the accumulator and fills the header.
 * cvm_stream_add    one chunk: X, Y (NULL iff M == 0), w (NULL: unweighted; the same for every chunk of a
 *                 stream) hold n_rows rows; idx / offsets (device) / host_offsets group the chunk's rows by
 *                 fold as in cvm_sweep_fit -- chunk-local row numbers, fold position = label, empty folds
 *                 allowed.  Launches the Gram kernel exactly as cvm_sweep_fit does, into `ws`
 *                 (cvm_stream_workspace_bytes(CVM_STREAM_SCRATCH, n_folds, the chunk's longest fold, ..);
 *                 contents before and after do not matter), and one kernel that adds every fold's chunk
 *                 update -- the ordered float64 sum of its row-split slots -- to the accumulator.  A fold
 *                 without rows in the chunk is skipped; n_rows == 0 launches nothing.  info (host, NULL or
 *                 int64[2]): the chunk's plan token (s_off | s_diag << 20) and the bytes the accumulate
 *                 kernel moves.
 * cvm_stream_close  makes the accumulated state readable: G, H, gstats = the fold-ordered sum of the units
 *                 (as cvm_sweep_fit forms them), neg_flag as there; *units_out / *units_bytes_out /
 *                 *splits_out are the workspace, its size and the plan token (one slot per fold) that
 *                 cvm_sweep_fold_range and cvm_sweep_unions accept as they are.  float64: the workspace is
 *                 the accumulator itself (ws may be NULL).  float32: every accumulated element is rounded
 *                 once into `ws` (cvm_stream_workspace_bytes(CVM_STREAM_CLOSE, ..)).  The units of the
 *                 accumulator are not written: more chunks may follow, and a later close sees them all.
 *                 Those two entry points read `offsets` only for the row counts of unweighted folds: pass
 *                 the cumulative totals of the accumulated fold sizes.
 * The bits depend on the chunks and their order alone; a stream of ONE chunk gives the bits of
 * cvm_sweep_fit + cvm_sweep_folds over the same folds.  No atomics.  CVM_EINVAL (negative sizes, decreasing
 * offsets, offsets that do not add up to n_rows, n_folds / K / M / dtype other than the header's, weights in
 * some chunks only) and CVM_EWORKSPACE (accumulator or workspace too small) are decided before the device is
 * touched. */
#define CVM_STREAM_ACCUMULATOR 0
#define CVM_STREAM_SCRATCH 1
#define CVM_STREAM_CLOSE 2
#define CVM_STREAM_STATE_LEN 8
size_t cvm_stream_workspace_bytes(int what, int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype);
int cvm_stream_reset(void *acc, size_t acc_bytes, int64_t n_folds, int K, int M, int dtype, int64_t *state,
                     void *stream);
int cvm_stream_add(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                   const int64_t *host_offsets, int64_t n_folds, int64_t n_rows, int K, int M, int dtype,
                   void *acc, size_t acc_bytes, int64_t *state, void *ws, size_t ws_bytes, void *stream,
                   int64_t *info);
int cvm_stream_close(void *acc, size_t acc_bytes, const int64_t *state, int64_t n_folds, int K, int M, int dtype,
                     void *G, void *H, double *gstats, int32_t *neg_flag, void *ws, size_t ws_bytes, void *stream,
                     void **units_out, size_t *units_bytes_out, int64_t *splits_out);

/* Device-side Partitioner (replaces cvmatrix/partitioner.py:89-107 for integer labels):
 *   labels      int64[N], one fold label per row, each in [0, n_labels) (up to 4096 labels: one
 *               stable counting sort; more, e.g. leave-one-out with a label per row: the same
 *               sort over 12-bit digits of the label, least significant first)
 *   idx_out     int64[N]           row numbers grouped by label, ascending inside a group
 *   offsets_out int64[n_labels+1]  label l owns idx_out[offsets_out[l] .. offsets_out[l+1])
 *   first_out   int64[n_labels]    first row of each label (N if the label does not occur): the
 *                                  reference orders its folds by first appearance
 *   err_flag    int32[1]           set to 1 if some label is outside [0, n_labels), else 0
 * The output is exactly the idx / offsets pair cvm_fold_update takes. */
size_t cvm_partition_workspace_bytes(int64_t N, int64_t n_labels);
int cvm_partition_labels(const int64_t *labels, int64_t N, int64_t n_labels, int64_t *idx_out,
                         int64_t *offsets_out, int64_t *first_out, int32_t *err_flag, void *ws,
                         size_t ws_bytes, void *stream);

/* The fit stage's weight validation for weights that live on the device -- cvmatrix/cvmatrix.py:1188-1189
 * (`any(weights < 0)` -> ValueError("Weights must be non-negative.")) and :1226 (`count_nonzero(weights)`):
 * out2 (device, int64[2]) receives [#(w < 0), #(w != 0)] as exact integer counts, by one small launch on
 * `stream`.  The host class copies the two words to pinned memory asynchronously and reads them when a
 * result of that fit is first handed out, so fit() neither reads the weights back nor waits for the device
 * (the reference's own JAX backend defers its data-dependent raises the same way, cvmatrix.py:621-625,
 * 1071-1074). */
int cvm_weights_check(const void *w, int64_t N, int dtype, int64_t *out2, void *stream);

/* Labels that are arange(N) % n_labels (the reference benchmark's folds, benchmarks/benchmark.py:232;
 * n_labels == N: leave-one-out) need no sort.  One launch: checks the labels (not_periodic[0] = 1 if
 * they are anything else -- the outputs are then garbage and the caller runs cvm_partition_labels),
 * writes idx_out int64[N] (fold-major, rows ascending inside a fold), offsets_out int64[n_labels + 1]
 * and, if nz_out is not NULL, every fold's number of rows with a non-zero weight (w NULL: its row
 * count) -- what cvm_fold_update's host-side checks need (cvmatrix.py:612-630).  Replaces
 * Partitioner._init_folds_dict (partitioner.py:89-107) for such labels. */
int cvm_partition_periodic(const int64_t *labels, int64_t N, int64_t n_labels, const void *w, int dtype,
                           int64_t *idx_out, int64_t *offsets_out, int64_t *nz_out, int32_t *not_periodic,
                           void *stream);

/* The step after the path: Improved Kernel PLS, algorithm #2 of Dayal &
 * MacGregor (1997), on the training matrices of a batch of folds where cvm_fold_update left them.
 * It is what the out-of-tree consumer named by the reference runs per fold (reference
 * README.md:23, cvmatrix/partitioner.py:27-31: `ikpls`, fast cross-validation); the reference
 * itself holds no PLS code, so there is no reference line to cite beyond those.
 *   XTX [n_folds][K][K], XTY [n_folds][K][M]   the out_XTX / out_XTY of cvm_fold_update (not modified)
 *   A                    components, 1 <= A <= 512;  M <= 64
 *   B   [n_folds][A][K][M]   B[f][a] = regression coefficients with a+1 components (required)
 *   W, P, R [n_folds][K][A], Q [n_folds][M][A]      weights / loadings / rotations (each may be NULL)
 *   n_fit  int32[n_folds]    components extracted (< A only if XTY deflated to zero: the rest stay 0)
 *   status int32[1]          0; the routes that cut a fold into slices need an otherwise idle device (the
 *                            slices wait for each other): if a slice found no place to run, every fold is
 *                            recomputed in the same call by one workgroup per fold and status is 2 (outputs
 *                            valid); 1 only where a fold does not fit one workgroup's LDS -- the outputs are
 *                            then NaN and n_fit -1, never half-written
 * Component signs are those of the dominant eigenvector found by repeated squaring of XTY^T XTY;
 * B does not depend on them.  Arithmetic in float64 for both dtypes.
 * Non-finite input: a fold with a NaN or an infinity anywhere in its XTX or XTY has B, W, P, Q, R all NaN
 * for every component and n_fit -1 (never zeros or other finite numbers: a fold that cvm_fold_update
 * handed over as NaN stays NaN through cvm_pls_validation_sse); status stays 0 and every other fold has
 * the bits it has when that fold is clean.  A fold of finite numbers whose arithmetic overflows ends the
 * same way.  A fold's bits depend on its own matrices and on the plan (cvm_pls_plan), not on its place
 * in the batch or on what the workspace held. */
size_t cvm_pls_workspace_bytes(int64_t n_folds, int K, int M, int A, int dtype);
int cvm_pls_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype,
                void *B, void *W, void *P, void *Q, void *R, int32_t *n_fit, int32_t *status,
                void *ws, size_t ws_bytes, void *stream);
/* Validation errors of the folds' PLS models -- the last step of the cross-validation the reference's
 * README describes (README.md:23), which its consumer ikpls leaves to the caller: for fold f, the model
 * with a+1 components and response m
 *   sse[f][a][m] = sum over the fold's validation rows i (idx / offsets as in cvm_fold_update) of
 *                  w_i * ( ((x_i - muX[f]) / sdX[f]) . B[f][a][:, m] * sdY[f][m] + muY[f][m] - y_im )^2
 *   wsum[f]      = sum w_i    (w NULL: the row count)
 * muX, sdX [n_folds][K], muY, sdY [n_folds][M] in `dtype`: the statistics outputs of cvm_fold_update
 * (NULL: no centring / no scaling).  B as cvm_pls_fit wrote it.  sse float64[n_folds][A][M], wsum
 * float64[n_folds].  MFMA in `dtype`, errors accumulated in float64 in a fixed order (no atomics).
 * RMSE of the cross-validation with a+1 components: sqrt(sum_f sse[f][a][m] / sum_f wsum[f]).
 * Limits: at most 65535 folds per call (one more: CVM_EINVAL, cvm_last_error names the limit; cut a longer
 * batch into several calls); max_fold_rows is the longest fold or any upper bound of it.  ws_bytes below
 * cvm_pls_sse_workspace_bytes: CVM_EWORKSPACE.  A refused call writes nothing; n_folds == 0 launches nothing.
 * An empty fold, and a fold whose weights are all zero, has sse exactly 0 and wsum exactly 0; without
 * weights wsum[f] is the fold's row count exactly.  A row may lie in several folds, or several times in one.
 * Bits: sse[f][a][m] depends on the fold's rows (their x, y, w and their order in idx), the fold's statistics,
 * its column B[f][a][:, m] and on where the plan keeps the fold's statistics (cvm_cv_predict_plan, info[7]) --
 * not on the other folds or the fold's place in the batch, the other columns of B, max_fold_rows, the
 * alignment of the arrays, what the workspace held, or the stream; the same call again gives the same bits.
 * The two places of the statistics form 1 / sdX differently (a division; the reciprocal instruction with one
 * Newton step, within a unit of it) and may differ in the last places: so may two calls whose K, M, A or
 * alignment lead to different info[7].
 * Non-finite input stays where it belongs and never becomes a finite number: an sdX[f][k] that is 0, infinite
 * or NaN, or a muX[f][k] that is infinite or NaN, makes every sse[f][a][m] of that fold non-finite on both
 * routes; a NaN in the column B[f][a][:, m] makes that one sum NaN; a NaN in y_im makes sse[f][:, m] NaN (with
 * the row's weight 0 too: 0 * NaN is NaN); a NaN in a row of X makes the sums of the folds that hold the row
 * NaN.  Every other sum keeps the bits it has when the input is clean. */
size_t cvm_pls_sse_workspace_bytes(int64_t n_folds, int64_t max_fold_rows, int M, int A);
int cvm_pls_validation_sse(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                           int64_t n_folds, int64_t max_fold_rows, int K, int M, int A, int dtype, const void *muX,
                           const void *sdX, const void *muY, const void *sdY, const void *B, double *sse,
                           double *wsum, void *ws, size_t ws_bytes, void *stream);
/* Ridge regression over a grid of penalties for every fold (no counterpart in the reference; the other
 * model people fit on the training matrices and tune by cross-validation): for fold f and penalty l
 *   (XTX[f] + lambdas[l] I) B[f][l] = XTY[f]
 * by a Cholesky factorisation, one workgroup per (fold, penalty) problem.
 *   XTX [n_folds][K][K], XTY [n_folds][K][M]   the out_XTX / out_XTY of cvm_fold_update (not modified;
 *                        XTX is taken as symmetric), 1 <= K <= 4096, 1 <= M <= 64
 *   lambdas  HOST float64[L], 1 <= L <= 256, each finite and >= 0 (copied into the launch: the caller may
 *            free it when the call returns)
 *   B    [n_folds][L][K][M] in `dtype`: the layout cvm_pls_validation_sse scores, penalties in place of
 *        components
 *   info int32[n_folds][L]: 0, or j > 0 where the j-th pivot (1-based, as LAPACK potrf) was not finite or
 *        not > 0: that problem's B is all NaN (never half-written); the other problems are unaffected.
 *        A NaN in XTY alone is no failure: info stays 0, the columns of that problem's B whose
 *        right-hand side held it are NaN, its other columns and the other problems are unaffected
 *   ws   cvm_ridge_workspace_bytes(n_folds, K, M, L) for every problem in flight at once (host arithmetic,
 *        no device query); any smaller workspace that holds one problem runs fewer problems at a time with
 *        the same results to the bit.  Less than one problem: CVM_EWORKSPACE.  Bad pointers, shapes,
 *        penalties or dtype: CVM_EINVAL.  n_folds == 0: nothing is launched.
 * Arithmetic in float64 for both dtypes (float32 inputs widened on load, B rounded once on store); a
 * problem's bits depend on its inputs alone, not on the batch around it or on the workspace size. */
size_t cvm_ridge_workspace_bytes(int64_t n_folds, int K, int M, int L);
int cvm_ridge_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, const double *lambdas, int L,
                  int dtype, void *B, int32_t *info, void *ws, size_t ws_bytes, void *stream);
/* Linear discriminant analysis with shrinkage for every fold (the classifier of the family; no counterpart in
 * the reference), from the training matrices alone.  With h_c = XTY[f][:, c], n_c = class_w[f][c], n = sum_c n_c
 * and m_c = h_c / n_c:
 *   S_w = XTX[f] - sum_c h_c h_c' / n_c,   Sigma_g = (1 - g) S_w / n + g (tr S_w / (n K)) I
 *   coef[f][l][:, c] = Sigma_g^-1 m_c,     intercept[f][l][c] = -1/2 m_c' coef[f][l][:, c] + log(n_c / n)
 * for g = shrinkage[l]: scikit-learn's LinearDiscriminantAnalysis(solver="lsqr", shrinkage=g) up to a term common
 * to all classes, PROVIDED that X is centred on the training set (CVM_CENTER_X) and Y is the unscaled 0/1 class
 * indicator with one 1 per row, which the call cannot see.  The discriminant of a row z standardised by the
 * fold's statistics is z' coef + intercept (cvm_cv_predict with muY = sdY = NULL, plus the intercept).
 * Three stages: S' = (K / tr S_w) S_w and the m_c into the workspace (lda_moments_kernel, lda_scatter_kernel);
 * (S' + g / (1 - g) I) x = m_c by the solver of cvm_ridge_fit for every g < 1; scaling and intercepts
 * (lda_finish_kernel; g = 1 takes x = m_c with no solve).
 *   XTX, XTY   [n_folds][K][K] and [n_folds][K][C] in `dtype`, 1 <= K <= 4096, 2 <= C <= 64 (not modified; the
 *              upper triangle of XTX is the one used, both are checked for values that are not finite)
 *   class_w    float64[n_folds][C]: the training weight of every class (its row count when unweighted)
 *   shrinkage  HOST float64[L], 1 <= L <= 256, each in [0, 1] (copied into the launches)
 *   coef       [n_folds][L][K][C] in `dtype`: the layout cvm_cv_predict takes, g in place of components
 *   intercept  [n_folds][L][C] in `dtype`
 *   info       int32[n_folds][L]: 0; j > 0 where the j-th pivot of the factorisation was not positive (a
 *              singular S_w at g = 0); -1 where the fold holds a value of XTX, XTY or class_w that is not finite,
 *              a negative class_w, or n or tr S_w that is not > 0.  Where info != 0 every coef and intercept
 *              of that (fold, g) is NaN (never half-written); the fold's other g keep the bits they have
 *              without the failure.  A class with n_c == 0 is absent from the fold: coef 0, intercept -inf
 *   ws         cvm_lda_workspace_bytes(n_folds, K, C, L): the fold records (S', m, x: (K + C + L C) K float64
 *              a fold and a few words) plus cvm_ridge_workspace_bytes(n_folds, K, C, L).  The smallest that
 *              runs is one fold record and one factorisation,
 *                cvm_lda_workspace_bytes(1, K, C, L) - cvm_ridge_workspace_bytes(1, K, C, L)
 *                                                    + cvm_ridge_workspace_bytes(1, K, C, 1);
 *              anything between runs fewer folds or factorisations at a time with the same results to the
 *              bit.  Less: CVM_EWORKSPACE.  Bad pointers, shapes, shrinkage (NaN included) or dtype: CVM_EINVAL,
 *              decided before the device is touched (cvm_lda_workspace_bytes: 0).  n_folds == 0: nothing is
 *              launched.
 * Arithmetic in float64 for both dtypes (float32 inputs widened on load, outputs rounded once on store), no
 * float atomics, every sum in a fixed order, S' symmetric to the bit: a fold's bits depend on its own XTX, XTY,
 * class_w and the grid alone, not on the batch around it or on the workspace size. */
size_t cvm_lda_workspace_bytes(int64_t n_folds, int K, int C, int L);
int cvm_lda_fit(const void *XTX, const void *XTY, const double *class_w /* [F][C] */, int64_t n_folds, int K, int C,
                const double *shrinkage, int L, int dtype, void *coef /* [F][L][K][C] */, void *intercept /* [F][L][C] */,
                int32_t *info /* [F][L] */, void *ws, size_t ws_bytes, void *stream);
/* PCA-LDA for every fold (the count-tuned classifier of the family; no counterpart in the reference): linear
 * discriminant analysis on the scores of the first 1, 2, .., A principal components, from the eigenpairs that
 * cvm_pcr_fit or cvm_pcr_blocked_fit return, the class sums and the class weights.  With h_c = XTY[f][:, c],
 * n_c = class_w[f][c], n = sum_c n_c, V = V[f] (K x A) and lambda = eigenvalues[f]:
 *   P = V' H,  m~_c = p_c / n_c (0 for an absent class),  S = diag(lambda) - sum_c p_c p_c' / n_c
 *   S = L L' column by column; the path ends before component j (counted from 0) when j >= n_comp[f] or the pivot
 *       d_j^2 = S_jj - sum_{i<j} L_ji^2 is not > pivot_tol lambda_j: n_fit[f] = j
 *   Z = L^-1 M~,  W = V L^-T
 *   coef[f][a] = coef[f][a-1] + w_a (n z_a)',   intercept[f][a] = intercept[f][a-1] - 1/2 (n z_a) o z_a,
 *   coef[f][-1] = 0,  intercept[f][-1][c] = log(n_c / n)
 * coef[f][a], intercept[f][a] are the discriminants on a+1 components, scikit-learn's Pipeline(PCA(a+1),
 * LinearDiscriminantAnalysis(solver="lsqr")) up to a term common to all classes, PROVIDED that X is centred on the
 * training set (CVM_CENTER_X) and Y is the unscaled 0/1 class indicator, which the call cannot see.  The
 * discriminant of a row z standardised by the fold's statistics is z' coef + intercept (cvm_cv_predict with
 * muY = sdY = NULL, plus the intercept).
 *   V          [n_folds][K][A] in `dtype`, eigenvalues float64[n_folds][A] descending, n_comp int32[n_folds]: the
 *              V, eigenvalues and n_fit of cvm_pcr_fit; 1 <= K <= 4096, 1 <= A <= min(K, 64): the factor lies in
 *              LDS with one row per lane.  n_comp above A counts as A
 *   XTY        [n_folds][K][C] in `dtype`, 2 <= C <= 64;  class_w float64[n_folds][C]
 *   pivot_tol  below 1; <= 0: the default 2^-26.  d_j^2 / lambda_j is the within-class share of component j's
 *              variance: below the square root of the unit roundoff the classes are separated along it as well as
 *              the arithmetic can tell
 *   coef       [n_folds][A][K][C] in `dtype`: the layout cvm_cv_predict takes;  intercept [n_folds][A][C] in `dtype`.
 *              For a >= n_fit[f] both have the bits of a = n_fit[f] - 1 (n_fit 0: coef 0, intercept the log priors).
 *              A class with n_c == 0 is absent from the fold: coef 0, intercept -inf
 *   n_fit      int32[n_folds]: the models that exist, 0 .. A; -1 for a flagged fold
 *   info       int32[n_folds]: 0 all A models exist; 1 the path ended at n_comp[f] < A; 2 it ended at a pivot; -1
 *              the fold is flagged: n_comp[f] < 0, a value of V or eigenvalues in a component < n_comp[f], of XTY or
 *              of class_w that is not finite (or a pivot, by overflow), a negative class_w, or n not > 0.  Every
 *              coef and intercept of a flagged fold is NaN (written in the same pass as the others: never
 *              half-written); other folds keep their bits
 *   ws         cvm_pcalda_workspace_bytes(n_folds, K, C, A): a record per fold (the shares of P of the
 *              ceil(K / 128) row slices, L^-1, n Z: (ceil(K / 128) C + A + C) A float64 and a few words).  The
 *              smallest that runs is cvm_pcalda_workspace_bytes(1, K, C, A); anything between takes as many folds
 *              at a time as fit, with the same results to the bit.  Less: CVM_EWORKSPACE.  Shapes outside the
 *              limits, a pivot_tol that is NaN or >= 1, a dtype that is none, or a null pointer with
 *              n_folds > 0: CVM_EINVAL, decided before the device is touched (cvm_pcalda_workspace_bytes: 0).
 *              n_folds == 0: nothing is launched.
 * Three launches per chunk of folds: P by row slices of K (pcalda_project_kernel; the slices are added in
 * ascending order, no float atomics), the factorisation, Z, L^-1 and the intercepts by one workgroup per fold
 * (pcalda_factor_kernel), coef by one workgroup per (fold, tile of rows) (pcalda_expand_kernel).  Arithmetic in
 * float64 for both dtypes (float32 inputs widened on load, outputs rounded once on store), every sum in a fixed
 * order: a fold's bits depend on its own V, eigenvalues, n_comp, XTY, class_w, A and pivot_tol alone, not on the
 * batch around it, the workspace size or the chunking. */
size_t cvm_pcalda_workspace_bytes(int64_t n_folds, int K, int C, int A);
int cvm_pcalda_fit(const void *V /* [F][K][A] */, const double *eigenvalues /* [F][A] */, const int32_t *n_comp /* [F] */,
                   const void *XTY /* [F][K][C] */, const double *class_w /* [F][C] */, int64_t n_folds, int K, int C,
                   int A, int dtype, double pivot_tol, void *coef /* [F][A][K][C] */, void *intercept /* [F][A][C] */,
                   int32_t *n_fit /* [F] */, int32_t *info /* [F] */, void *ws, size_t ws_bytes, void *stream);
/* PCA and principal component regression for every fold (the two consumers of the training matrices that
 * the reference's CVMatrix docstring names next to PLS and OLS): the A leading eigenpairs of XTX[f],
 *   XTX[f] v_j = lambda_j v_j,  lambda_0 >= lambda_1 >= ...,
 * and the regression coefficients on the first a+1 components
 *   B[f][a] = sum over j <= a of v_j (v_j^T XTY[f]) / lambda_j
 * by a cyclic two-sided Jacobi iteration in a fixed round-robin order, one workgroup per fold.
 *   XTX [n_folds][K][K], XTY [n_folds][K][M]   the out_XTX / out_XTY of cvm_fold_update (not modified;
 *                        XTX is taken as symmetric), 1 <= K <= 512, 1 <= A <= K, 0 <= M <= 64;
 *                        M == 0 with XTY == NULL and B == NULL: PCA only
 *   rank_tol     components with lambda_j <= rank_tol * lambda_0 do not exist; <= 0: the default
 *                32 K 2^-52 (the backward error of the method, below which an eigenvalue cannot be told
 *                from zero); NaN or >= 1: CVM_EINVAL
 *   B    [n_folds][A][K][M] in `dtype`: the layout cvm_pls_validation_sse scores.  Summed in the order
 *        j = 0, 1, ...; for a >= n_fit[f], B[f][a] has the bits of B[f][n_fit[f] - 1] (all zeros if
 *        n_fit[f] == 0): the model with more components than exist is the model with all that exist
 *   eigenvalues  float64 [n_folds][A] for both dtypes, as computed (may be tiny or slightly negative)
 *   V    [n_folds][K][A] in `dtype` (may be NULL): the components; in each the entry of largest magnitude
 *        is positive (the lowest index among equals); components a >= n_fit[f] are exactly zero
 *   n_fit  int32[n_folds]: min(A, number of lambda_j > rank_tol * lambda_0)
 *   sweeps int32[n_folds]: Jacobi sweeps run (the last one made no rotation), 1 .. 60
 *   ws   cvm_pcr_workspace_bytes(n_folds, K, M, A) for min(n_folds, 512) folds in flight (host arithmetic,
 *        no device query): slots of 2 K ld float64, ld = max(K, M) rounded up to 4, each 256-byte aligned;
 *        any smaller workspace that holds one slot runs fewer folds at a time with the same results to
 *        the bit.  Less than one slot: CVM_EWORKSPACE.  Bad pointers, shapes, rank_tol or dtype:
 *        CVM_EINVAL (cvm_pcr_workspace_bytes: 0).  n_folds == 0: nothing is launched.
 * Non-finite input: a fold with a NaN or an infinity anywhere in its XTX or XTY (or whose Frobenius norm
 * overflows) has B, V and eigenvalues all NaN, n_fit -1 and sweeps 0, as cvm_pls_fit has it: a fold that
 * cvm_fold_update handed over as NaN stays NaN through cvm_pls_validation_sse.  A fold that has not
 * converged after 60 sweeps: the same outputs with sweeps -1.  Every other fold is unaffected.
 * Arithmetic in float64 for both dtypes (float32 inputs widened on load, outputs rounded once on store),
 * no float atomics, every sum in a fixed order; a fold's bits depend on its own matrices alone, not on its
 * place in the batch, the batch size, the workspace size or what the workspace held. */
size_t cvm_pcr_workspace_bytes(int64_t n_folds, int K, int M, int A);
int cvm_pcr_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype,
                double rank_tol, void *B, double *eigenvalues, void *V, int32_t *n_fit, int32_t *sweeps,
                void *ws, size_t ws_bytes, void *stream);
/* The same PCA / PCR with a second eigensolver, for 1 <= K <= 4096: a cyclic two-sided BLOCK Jacobi method
 * (blocks of 32 indices, the round-robin order above applied to blocks), many workgroups per fold.  A round is
 * two launches: one workgroup per pair of blocks runs one scalar Jacobi sweep (the rotation formulas and the
 * rule of cvm_pcr_fit: pair (p,q) rotates iff |S_pq| > 2^-52 ||XTX[f]||_F) on the pair's 64 x 64 diagonal tile
 * and keeps the product Q of its rotations; then one workgroup per off-diagonal tile of S and per tile of V
 * applies Q^T . Q and . Q by 64 x 64 x 64 float64 matrix-core products, writing the mirror tile of S as the
 * transpose of the same numbers.  No workgroup waits for another; the launches are ordered by the stream.
 *   XTX, XTY, rank_tol, B, eigenvalues, V, n_fit: as cvm_pcr_fit, word for word (eigenvalues descending by
 *        counting rank, ties by index; in every component the entry of largest magnitude positive; n_fit =
 *        min(A, number of lambda_j > rank_tol * lambda_0), default rank_tol 32 K 2^-52; B[f][a] for a >= n_fit
 *        has the bits of B[f][n_fit - 1]; components a >= n_fit are exactly zero), with 1 <= K <= 4096
 *   max_sweeps  1 .. 60: a fold that has not converged after that many sweeps is NaN throughout, sweeps -1
 *   sweeps int32[n_folds]: block sweeps run (the last one made no rotation), 1 .. max_sweeps; 0 with n_fit -1
 *        for a fold with a NaN or an infinity in its XTX or XTY (NaN throughout, no rotation run)
 *   ws   cvm_pcr_blocked_workspace_bytes(n_folds, K, M, A) for min(n_folds, 512) folds in flight (host
 *        arithmetic, no device query).  A slot holds S and V padded to Kp = 32 * (ceil(K / 32) rounded up to
 *        even), Kp / 64 matrices Q, the flag words and the running sum of the coefficients, 256-byte aligned
 *        (about 270 MB at K = 4096).  Any workspace that holds one slot gives the same bits; less:
 *        CVM_EWORKSPACE.  Bad pointers, shapes, rank_tol, max_sweeps or dtype: CVM_EINVAL
 *        (cvm_pcr_blocked_workspace_bytes: 0).  n_folds == 0: nothing is launched.
 * THIS ENTRY WAITS FOR THE DEVICE ONCE PER SWEEP, unlike cvm_pcr_fit: after every sweep it copies one status
 * word per fold of the batch on `stream` and waits for the copy; converged folds are finished and drop out,
 * the rest get another sweep.  It therefore cannot be captured into a graph: on a capturing stream it returns
 * CVM_EINVAL without launching or synchronising anything.
 * Arithmetic in float64 for both dtypes, no float atomics, every sum in a fixed order; a fold's bits depend on
 * its own matrices, rank_tol and max_sweeps alone, not on its place in the batch, the batch size, the
 * workspace size, which other folds have finished or what the workspace held. */
size_t cvm_pcr_blocked_workspace_bytes(int64_t n_folds, int K, int M, int A);
int cvm_pcr_blocked_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype,
                        double rank_tol, int max_sweeps, void *B, double *eigenvalues, void *V,
                        int32_t *n_fit, int32_t *sweeps, void *ws, size_t ws_bytes, void *stream);
/* Elastic net and lasso over a grid of penalties for every fold (the sparse member of the family; no
 * counterpart in the reference): for fold f, response m and penalty l, with G = XTX[f], h = XTY[f][:, m],
 *   B[f][l][:, m] = argmin over beta of
 *                   1/2 beta' G beta - h' beta + lambdas[l] (l1_ratio |beta|_1 + 1/2 (1 - l1_ratio) |beta|_2^2)
 * on the training matrices as they are.  For unweighted, centred data of n training rows this is scikit-learn's
 * ElasticNet(alpha = lambda / n, l1_ratio, fit_intercept=False); with weights, the sum of weights in place of n.
 * Cyclic coordinate descent with covariance updates, one wavefront per (fold, response): the penalties of a
 * path are walked from the largest down, each warm-started from the one before; B is in the caller's order.
 *   XTX, XTY, B, lambdas, ws   as cvm_ridge_fit has them, but every penalty finite and > 0
 *   l1_ratio   0 < l1_ratio <= 1 (1: the lasso; 0 is cvm_ridge_fit)
 *   tol        1e-12 <= tol < 1.  A problem is converged when, with g = h - G beta formed afresh and
 *              r = g - lambda (1 - l1_ratio) beta, the largest over all K coordinates of
 *                |r_j - lambda l1_ratio sign(beta_j)|      where beta_j != 0
 *                max(0, |r_j| - lambda l1_ratio)           where beta_j == 0
 *              is <= tol max_j |h_j|.  Nothing else counts as converged.
 *   max_sweeps >= 1: passes over the coordinates plus certificate passes a problem may take
 *   info   int32[n_folds][L][M]: 0 converged; 1 max_sweeps reached: B holds the last iterate, finite, and
 *          sweeps == max_sweeps; 2 a value that is not finite met in the diagonal of G, in h, in a coefficient
 *          or in the violation: B[f][l][:, m] is all NaN (never half-written), and the next penalty of that
 *          path starts from zero.  A NaN in one response's column of XTY affects that response only.
 *   sweeps int32[n_folds][L][M]: the passes taken (1 where lambda >= max|h| / l1_ratio: B is exactly zero)
 *   ws     cvm_enet_workspace_bytes(n_folds, K, M, L) for min(n_folds M, 1024) paths in flight (host
 *          arithmetic, no device query): one slot of K float64, 256-byte aligned, per path; any smaller
 *          workspace that holds one slot runs fewer paths at a time with the same results to the bit.  Less
 *          than one slot: CVM_EWORKSPACE.  Bad pointers, shapes, penalties, l1_ratio, tol, max_sweeps or
 *          dtype: CVM_EINVAL.  n_folds == 0: nothing is launched.
 * A coordinate whose denominator G_jj + lambda (1 - l1_ratio) is not > 0 stays at zero.  Arithmetic in float64
 * for both dtypes (float32 inputs widened on load, B rounded once on store), no atomics, every sum and every
 * admission to the active set in a fixed order: a path's bits depend on its own inputs and the penalty grid
 * alone. */
size_t cvm_enet_workspace_bytes(int64_t n_folds, int K, int M, int L);
int cvm_enet_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, const double *lambdas, int L,
                 double l1_ratio, double tol, int max_sweeps, int dtype, void *B, int32_t *info, int32_t *sweeps,
                 void *ws, size_t ws_bytes, void *stream);
/* Orthogonal matching pursuit (greedy forward variable selection; scikit-learn's orthogonal_mp_gram; no
 * counterpart in the reference) for every fold: for fold f and response m, with G = XTX[f], h = XTY[f][:, m]
 * and S the ordered list of selected indices (empty at first), step a = 0 .. A - 1 is
 *   1. alpha = h - G[:, S] gamma, gamma the least-squares coefficients on S (alpha = h while S is empty)
 *   2. score_k = |alpha_k| (normalize == 0, scikit-learn's rule) or |alpha_k| / sqrt(G_kk) (normalize == 1, the
 *      correlation with the residual; a column whose G_kk is not > 0 is never selected) for every k not in S
 *   3. j = the index of the largest score; among equal scores the lowest index.  A largest score that is not
 *      > 0 (no column may be selected, or every remaining alpha is exactly zero, as with h = 0) ends the path
 *      with n_fit = a
 *   4. the Cholesky factor L of G_SS gains the row w = L^-1 G[S, j] and the pivot d^2 = G_jj - w'w;
 *      d^2 <= rank_tol G_jj ends the path with n_fit = a: the best remaining candidate depends on S
 *   5. L L' gamma = h_S;  B[f][a][:, m] = gamma scattered to S, exactly 0 elsewhere.
 * Each response selects its own variables.  One wavefront per (fold, response).
 *   XTX, XTY   [n_folds][K][K] and [n_folds][K][M] in `dtype`, 1 <= K <= 4096, 1 <= M <= 64
 *   A          steps = selected variables at most, 1 <= A <= min(K, 64)
 *   normalize  0 or 1
 *   rank_tol   below 1; <= 0: the default 32 A 2^-52
 *   B          [n_folds][A][K][M] in `dtype`: for a >= n_fit[f][m], B[f][a][:, m] has the bits of
 *              B[f][n_fit - 1][:, m] (all zeros if n_fit == 0), as cvm_pcr_fit pads
 *   support    int32[n_folds][A][M]: the index selected at step a; -1 for a >= n_fit
 *   n_fit      int32[n_folds][M]: 0 .. A, or -1 where a value that is not finite was met in the diagonal of G,
 *              in h, in alpha or a score, in a pivot or in a coefficient: B[f][:][:, m] is then all NaN (written
 *              once, after the status is known: never half-written) and support[f][:][m] all -1.  A NaN in one
 *              response's column of XTY affects that response only, a NaN fold that fold only.
 *   ws         cvm_omp_workspace_bytes(n_folds, K, M, A) for min(n_folds M, 1024) paths in flight (host
 *              arithmetic, no device query): one slot of K float64, 256-byte aligned, per path; any smaller
 *              workspace that holds one slot runs fewer paths at a time with the same results to the bit.  Less
 *              than one slot: CVM_EWORKSPACE.  Bad pointers, shapes, A, normalize, rank_tol (NaN or >= 1) or
 *              dtype: CVM_EINVAL, decided before the device is touched (cvm_omp_workspace_bytes: 0).
 *              n_folds == 0: nothing is launched.
 * Arithmetic in float64 for both dtypes (float32 inputs widened on load, which is exact: the selection on float32
 * inputs is the float64 selection on those inputs; B rounded once on store), no atomics, every sum and every
 * comparison in a fixed order: a path's bits depend on its own G, h, A, normalize and rank_tol alone, not on the
 * batch around it, the workspace size or scheduling. */
size_t cvm_omp_workspace_bytes(int64_t n_folds, int K, int M, int A);
int cvm_omp_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int normalize,
                double rank_tol, int dtype, void *B, int32_t *support, int32_t *n_fit,
                void *ws, size_t ws_bytes, void *stream);
/* Out-of-fold predictions of every fold's linear models, and predictions for new rows -- what the scorer
 * above forms and reduces to one number, stored whole (scikit-learn's cross_val_predict; no counterpart in
 * the reference, whose consumers predict fold by fold on the host): for fold f, row i of the fold, model a
 * and response m
 *   out[r][a][m] = ((x_i - muX[f]) / sdX[f]) . B[f][a][:, m] * sdY[f][m] + muY[f][m]
 *   X    rows of K elements with a row pitch of ldX >= K elements (a padded model: its pitch)
 *   idx, offsets  device arrays as in cvm_pls_validation_sse; idx == NULL: the fold's rows are the rows
 *        offsets[f] .. offsets[f+1]-1 of X themselves (new data: one fold, offsets {0, n})
 *   max_fold_rows  the longest fold, from the host (the device offsets are not read back)
 *   muX, sdX [n_folds][K], muY, sdY [n_folds][M] in `dtype`; each may be NULL: 0 for a mean, 1 for a
 *        standard deviation
 *   B    [n_folds][A][K][M] in `dtype`, 1 <= A <= 512, 1 <= M <= 64, K >= 1
 *   out  [rows][A][M] in `dtype`, contiguous: the A M predictions of a row lie together.  by_row == 0: r is
 *        the position in idx (offsets[f] + i); by_row == 1: r is the row number (the idx value) -- the caller
 *        guarantees that no row occurs twice, and rows in no fold are not written
 * No workspace, no atomics, any number of folds of any length (cvm_cv_predict_plan: how a call is cut into
 * launches).  n_folds == 0: nothing is launched.  Bad pointers, shapes,
 * by_row or dtype: CVM_EINVAL, decided before the device is touched.
 * MFMA in `dtype`, the standardisation and the scale-and-shift in float64, one rounding to `dtype` at the
 * store.  The sum over k runs in ONE order (stages of 16, steps of 4) on every route, and the reciprocal of
 * sdX is formed by one formula: the bits of one prediction depend on its row of X, its fold's statistics and
 * its column B[f][a][:, m] alone -- not on the fold's other rows, the row's place in the fold, the other
 * folds, A, the other columns of B, ldX, by_row, the alignment of the arrays or the stream.  A NaN stays
 * where it belongs: in the rows of X that hold it, in the folds whose B or statistics hold it. */
int cvm_cv_predict(const void *X, int64_t ldX, const int64_t *idx, const int64_t *offsets, int64_t n_folds,
                   int64_t max_fold_rows, int K, int M, int A, int dtype,
                   const void *muX, const void *sdX, const void *muY, const void *sdY,
                   const void *B, void *out, int by_row, void *stream);
/* How cvm_cv_predict cuts a call into launches -- host arithmetic, no device: info[0] = column tiles of 16 per
 * wave (a workgroup owns 64 rows x 64 info[0] columns), [1] = column groups, [2] = row chunks of 64 in the longest
 * fold, [3] = workgroups in all = n_folds x [1] x [2], [4] = launches, [5] = workgroups of the largest launch,
 * [6] = LDS bytes per workgroup, [7] = 1 if the fold's statistics are kept in LDS, [8] = 1 if rows and coefficients
 * are read in 16-byte pieces.  `aligned`: X, B, muX and sdX are 16-byte aligned.  The HIP runtime refuses a launch
 * of 2^32 threads or more in x, so a launch has at most 2^24 - 1 workgroups of 256 threads; the flat list of
 * workgroups is cut wherever that falls, inside a fold too: neither the number of folds nor the length of a fold is
 * limited by it (beyond 2^40 each, and 2^61 workgroups in all: CVM_EINVAL).
 * info[0], [1], [6], [7] and [8] are cvm_pls_validation_sse's choices too, for ldX = K: the two calls share the
 * kernel variants and the rule that picks one. */
int cvm_cv_predict_plan(int64_t n_folds, int64_t max_fold_rows, int64_t ldX, int K, int M, int A, int dtype,
                        int aligned, int64_t *info);
/* info[0]=row slices per fold, [1]=rows per slice, [2]=folds per launch, [3]=1 if the slice of XTX
 * stays in LDS, 0 if it is streamed, 2: few folds -- the kernel that keeps the small state of a fold
 * (deflated XTY, P, R) whole in every slice and passes ONE per-fold barrier per component, XTX
 * streamed from L2, the slices of a fold on one XCD; [4]=LDS bytes per workgroup */
int cvm_pls_plan(int64_t n_folds, int K, int M, int A, int dtype, int64_t *info);

/* Benchmark support: when enabled, a hipEvent pair is recorded on the launch stream around
 * every launch of the Gram kernel (at most 8192 pairs between reads).  cvm_timing_read
 * waits for the recorded events, returns the summed kernel milliseconds and launch counts
 * of the fit stage and of the fold stage since the last read, and resets the list.
 * One recorder per process (all streams, all threads; slots are handed out under a mutex):
 * meant for bench.py. */
int cvm_timing_enable(int on);
int cvm_timing_read(double *ms_fit, int64_t *n_fit, double *ms_fold, int64_t *n_fold);
/* The same list by kind: ms4 / n4 [0] Gram launches of the fit stage, [1] of the fold stage, [2] the
 * statistics kernel of the small-fold route (small_stats_kernel), [3] its update kernels (everything
 * a call launches after the statistics: tile / whole-rows kernel and the XTY panels). */
int cvm_timing_read_kinds(double *ms4, int64_t *n4);
/* The same for a stream: the Gram launches (kind 1) and the accumulate kernels of cvm_stream_add. */
int cvm_timing_read_stream(double *ms_gram, int64_t *n_gram, double *ms_acc, int64_t *n_acc);

/* Benchmark support: the write ceiling of this device, measured with the product's own kind of store --
 * one launch that fills `bytes` (a multiple of 16) from `buf` (16-byte aligned) with zeros by nontemporal
 * 16-byte stores in linear order.  bench.py times it on the output buffer of the HBM-regime shapes, in the
 * same run, so that a measured rate can be read against what THIS box's memory system takes
 * (`frac_of_fill` next to `frac`).  No reference counterpart: the reference has no device. */
int cvm_fill_probe(void *buf, size_t bytes, void *stream);

/* Benchmark support: the shader clock the chip holds UNDER the product's LDS-DMA Gram kernel (the kernel of
 * cvm_gram_fit / cvm_sweep_* / cvm_fold_update), read inside the shipped kernel itself.  While a caller-owned
 * device buffer is set (8-byte aligned; NULL switches the probe off, the default), every such launch of the
 * process makes workgroup b < bytes / 32 store four 64-bit words at buf + 32 b:
 *   [0] s_memtime, [1] s_memrealtime when the workgroup starts;  [2], [3] the same pair when it has run out of
 *   work items
 * -- two scalar clock reads per workgroup lifetime, nothing inside the item loop; results are unchanged.
 * ([2] - [0]) / ([3] - [1]) x 100 MHz is the average shader clock over that workgroup's life (s_memrealtime
 * ticks at 100 MHz whatever the chip does; MI355X_MICROARCH.md "DVFS give-back" item 6), ([3] - [1]) its
 * duration in 10 ns units.  bench.py reports the median over the workgroups of the last timed launch as
 * roofline.effective_clock_mhz.  The caller synchronises before it reads the buffer, and clears the probe
 * before it frees it.  No reference counterpart: the reference has no device. */
int cvm_clock_probe(void *device_buf, size_t bytes);

/* Experiments and tests: pin the row-split plan of every later call of this process to (s_off, s_diag) row
 * splits of the off-diagonal / diagonal tile items (clamped to what the problem allows); (0, 0) hands the
 * decision back to the planner.  Stored in one atomic word; the environment variable CVM_FORCE_SPLITS="a,b" is
 * read once, as its initial value.  Results stay within the parity bar under any plan (float32: one more
 * rounding per extra partial, cvmatrix_amd/fp32_gate.py).  No reference counterpart. */
int cvm_debug_force_splits(int s_off, int s_diag);

/* Experiments and tests: where float32 XTX batches of folds of at most 32 rows, K a multiple of 1024, take the round-6
 * "resident" kernel (csrc/resident.hpp: G in the register files of the whole chip, every tile computed directly, no
 * mirrored store).  mode 2 (the default): K = 2048 or a multiple of 4096 and at least 16 folds per workgroup set (16 folds per
 * batch from K = 4096 on, 64 at K = 2048), where it measures 6-13 % faster than the tile kernel; 1: wherever the shape allows (slower below K = 4096 and for few folds); 0: never.  The environment
 * variable CVM_RESIDENT=0|1|2 is read once, as the initial value.  Results stay within the float32 parity bar and exactly
 * symmetric on either route; size the workspace with cvm_fold_workspace_bytes AFTER changing the mode (the route keeps an
 * operand block per fold there; with a smaller workspace the folds are walked in smaller batches or take the tile
 * kernel).  No reference counterpart. */
int cvm_debug_resident(int mode);

/* Introspection for benchmarks/profiles: geometry chosen for a problem (info: int64[8]).
 * info[0]=row splits per fold of the off-diagonal 128x128 tiles, [6]=row splits of the diagonal
 * tiles (which also produce XTY and the column sums and cost less per row: the two kinds are cut
 * differently so that all workgroups of a launch take about the same time), [7]=partial slots per
 * fold in the workspace (the larger of the two), [1]=workgroups of the Gram kernel per batch,
 * [2]=column panels, [3]=work items per (fold, split) if both kinds were cut alike, [4]=folds per
 * batch, [5]=MFMA instructions the kernel issues per 4 rows of one fold (executed work, 2048 flop
 * each).  Bit 31 of `flags` set: plan the fit stage instead.  Same decision procedure as the real
 * calls. */
int cvm_plan_fold(int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype,
                  unsigned flags, size_t ws_bytes, int64_t *info);

#ifdef __cplusplus
}
#endif
#endif /* CVMHIP_H */
