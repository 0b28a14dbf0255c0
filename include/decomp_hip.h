/*
 * decomp_hip.h -- C ABI of libdecomp_hip.so, the MI355X (gfx950) implementation of
 * deComP's iterative-update hot path.
 *
 * The reference (fujii-team/deComP) has no FFI: its "device layer" is the NumPy/CuPy
 * array-module handle `xp` (decomp/utils/cp_compat.py:9-24) threaded through every
 * solver.  This header is what replaces `xp` + the L1/L2 solver bodies for the hot
 * path; each entry point cites the reference function it stands in for.  The
 * reference-side binding (a ctypes stub) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handle, raw DEVICE pointers, sizes; no C++ or torch types.
 *   - every function returns an int status (DCP_OK = 0, negative = error); no C++
 *     exception crosses the ABI.  dcp_last_error_string() gives the message.
 *   - arrays are C-contiguous row-major, exactly as the reference's NumPy arrays:
 *       y[N,F]  x[N,K]  D[K,F]  mask[N,F]   (N samples, F features/channels, K atoms)
 *   - dtype suffixes: f32, f64 (real), c64, c128 (interleaved re,im pairs).
 *   - work is enqueued on the handle's stream (dcp_set_stream); functions that
 *     return host scalars (iteration counts, max|dD|) synchronise that stream
 *     before returning, the *_async step functions do not.
 *   - a handle is bound to one device and is not re-entrant.
 */
#ifndef DECOMP_HIP_H
#define DECOMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcp_handle dcp_handle;

enum {
    DCP_OK = 0,
    DCP_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, bad enum) */
    DCP_ERR_HIP = -2,       /* a HIP runtime call failed */
    DCP_ERR_NOMEM = -3,     /* workspace allocation failed */
    DCP_ERR_INTERNAL = -4,  /* library bug (workspace plan mismatch, ...) */
    DCP_ERR_UNSUPPORTED = -5,
    DCP_ERR_REF_TYPEERROR = -6, /* the reference raises TypeError on this input (lasso.py:509) */
    DCP_ERR_COMM = -7       /* librccl missing, no communicator on the handle, or an RCCL call failed */
};

/* likelihood codes: decomp/nmf_methods/grads.py:7-14, and the beta-divergence family (Fevotte & Idier 2011;
 * beta = 0 is Itakura-Saito).  DCP_LIK_BETA takes its beta from the handle (dcp_set_nmf_beta). */
enum { DCP_LIK_L2 = 0, DCP_LIK_KL = 1, DCP_LIK_BETA = 2 };

/* LASSO solver codes: decomp/lasso.py:13 */
enum { DCP_LASSO_ISTA = 0, DCP_LASSO_ACC_ISTA = 1, DCP_LASSO_FISTA = 2, DCP_LASSO_CD = 3,
       DCP_LASSO_PARALLEL_CD = 4, DCP_LASSO_ADMM = 5 };
/* dcp_dict_* only: orthogonal matching pursuit as the inner coder (dcp_omp_*).  lasso_iter is the sparsity
 * n_nonzero, lasso_tol the residual tolerance (< 0: none); alpha and the warm start X are not read; with
 * DCP_LASSO_POSITIVE, with a mask or with n_nonzero outside [1, min(K, cap)] the call is DCP_ERR_INVALID. */
enum { DCP_LASSO_OMP = 6 };
/* dcp_dict_*: OR this into lasso_method for the '_pos' (non-negative) solvers */
enum { DCP_LASSO_POSITIVE = 0x100 };

/* ---- lifetime ----------------------------------------------------------------- */
int dcp_create(dcp_handle** out, int device);
int dcp_destroy(dcp_handle* h);
/* hipStream_t passed as void*; NULL = the device's default stream.  Cheap (no HIP call): the library's
 * workspace is ordered between the old and the new stream by the next call that uses workspace (an event
 * recorded on the OLD stream and waited for on the new one, no host synchronisation); the row movers use none
 * and are never ordered against other streams' work.
 * LIFETIME (hard rule): a stream handed to the handle must stay alive until the next workspace-using call has
 * been issued through this handle on another stream (that call still records an event on the old stream), or
 * until the handle is destroyed.  Destroying it earlier is a use-after-free inside the HIP runtime, not an
 * error the library can detect or recover from. */
int dcp_set_stream(dcp_handle* h, void* hip_stream);
const char* dcp_last_error_string(dcp_handle* h);
/* compile-time facts, for the loader's sanity check */
const char* dcp_build_info(void);

/* ---- multi-GPU: the handle's RCCL communicator ---------------------------------- */
/* The reference has no multi-device path; the data-parallel form of its loops (rows of y / x / mask
 * sharded over one process per GPU, D replicated) needs exactly ONE exchange per outer iteration: the
 * sum over ranks of the D-side statistics (grads.py:117-125 / dictionary_learning.py:147-152 are sums over
 * rows).  That all-reduce runs INSIDE the library, on the handle's own stream, through RCCL over xGMI:
 *   dcp_comm_unique_id : rank 0 draws the 128-byte id (ncclGetUniqueId) into HOST memory; the launcher's
 *                        own channel (decomp_amd.sharded: torch.distributed's store) carries it to the
 *                        other ranks -- the only thing that channel is used for.
 *   dcp_comm_init      : collective over all ranks (ncclCommInitRank on the handle's device).
 *   dcp_comm_allreduce_sum_* : in-place sum of buf[count] over the ranks, asynchronous on the handle's
 *                        stream (complex data: pass the interleaved (re, im) floats, count doubled).
 * librccl is bound at run time (the copy the process already holds, else the system one); without it
 * these calls return DCP_ERR_COMM and everything else of the library works.
 *   dcp_comm_set_external : instead of RCCL, the caller's own exchange (MPI, gloo, a test double): fn(buf, count,
 *                        dtype (0 = float32, 1 = float64), hip_stream, user) must leave the element-wise sum over
 *                        all ranks in the DEVICE array buf[count], ordered before anything enqueued on hip_stream
 *                        afterwards (e.g. synchronise the stream, exchange through the host, copy back on the same
 *                        stream), and return 0.  The sharded loops call it exactly where they would call
 *                        ncclAllReduce; decomp_amd.sharded uses it for process groups RCCL cannot serve (gloo with
 *                        several ranks on one GPU), so the SAME in-library loop runs in the two-rank tests.
 *   dcp_memcpy         : hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault) on the handle's stream (what such a
 *                        callback needs to stage through pinned host memory). */
enum { DCP_COMM_ID_BYTES = 128 };
typedef int (*dcp_allreduce_fn)(void* buf, int64_t count, int dtype, void* hip_stream, void* user);
int dcp_comm_set_external(dcp_handle* h, dcp_allreduce_fn fn, void* user, int rank, int world);
int dcp_memcpy(dcp_handle* h, void* dst, const void* src, int64_t bytes);
int dcp_comm_unique_id(void* id_out, int64_t id_bytes);
int dcp_comm_init(dcp_handle* h, const void* unique_id, int rank, int world);
int dcp_comm_destroy(dcp_handle* h);
/* *world = 0 when the handle has no communicator */
int dcp_comm_info(dcp_handle* h, int* rank, int* world);
int dcp_comm_allreduce_sum_f32(dcp_handle* h, float* buf, int64_t count);
int dcp_comm_allreduce_sum_f64(dcp_handle* h, double* buf, int64_t count);

/* ---- per-kernel timing (measurement aid, used by bench.py) ---------------------- */
/* While enabled, every labelled kernel group of the solvers is bracketed by hipEvents on
 * the handle's stream.  dcp_profile_read synchronises the stream, folds the pending
 * event pairs into per-label totals and returns total milliseconds and launch count. */
enum {
    DCP_PROF_GRAM = 0,        /* D D^T (split-K) + slab sum                      */
    DCP_PROF_XNEG = 1,        /* negative part of the x gradient: x G, f D^T, M D^T */
    DCP_PROF_XUPDATE = 2,     /* Y D^T GEMM with the fused MU quotient epilogue  */
    DCP_PROF_FWD = 3,         /* (x D) o M / KL ratio: the [N,F] intermediate     */
    DCP_PROF_STATS = 4,       /* x^T [Y | x] split-K GEMM                         */
    DCP_PROF_STATS_SUM = 5,   /* slab sum of the statistics                       */
    DCP_PROF_DUPDATE = 6,     /* (x^T x) D GEMM + quotient (or elementwise quotient) */
    DCP_PROF_DNORM = 7,       /* l2_strict + max|dD|                              */
    DCP_PROF_MISC = 8,
    DCP_PROF_EXCHANGE = 9,    /* the all-reduce of the statistics (sharded loops)  */
    DCP_PROF_NLABELS = 10
};
int dcp_profile_enable(dcp_handle* h, int on);
/* restrict the brackets to the labels whose bit is set (each bracket costs ~4 us of stream time:
 * bench.py times only the dominant kernel inside its timed steps) */
int dcp_profile_select(dcp_handle* h, unsigned label_mask);
int dcp_profile_reset(dcp_handle* h);
int dcp_profile_read(dcp_handle* h, int label, double* total_ms, int64_t* count);
const char* dcp_profile_label_name(int label);

/* ---- utilities ---------------------------------------------------------------- */
/* utils/normalize.py:2-21.  Rows of U[K,F] divided by sqrt(sum|u|^2) (strict != 0)
 * or by sqrt(max(sum|u|^2, 1)) (strict == 0), in place. */
int dcp_l2_normalize_f32(dcp_handle* h, float* U, int64_t K, int64_t F, int strict);
int dcp_l2_normalize_f64(dcp_handle* h, double* U, int64_t K, int64_t F, int strict);
int dcp_l2_normalize_c64(dcp_handle* h, void* U, int64_t K, int64_t F, int strict);
int dcp_l2_normalize_c128(dcp_handle* h, void* U, int64_t K, int64_t F, int strict);

/* utils/assertion.py:95-100 (assert_nonnegative): number of elements for which
 * `x >= 0` is false (negative values and NaNs), written to the HOST integer *count. */
int dcp_count_negative_f32(dcp_handle* h, const float* x, int64_t n, int64_t* count);
int dcp_count_negative_f64(dcp_handle* h, const double* x, int64_t n, int64_t* count);

/* math_utils/eigen.py:9-20 (spectral_radius_Gershgorin): for a batch X[batch, n, n],
 * out[b] = max_j sum_i |X[b, i, j]| (DEVICE array of the real dtype, length batch).
 * Asynchronous on the handle's stream. */
int dcp_gershgorin_f32(dcp_handle* h, const float* X, int64_t batch, int64_t n, float* out);
int dcp_gershgorin_f64(dcp_handle* h, const double* X, int64_t batch, int64_t n, double* out);
int dcp_gershgorin_c64(dcp_handle* h, const void* X, int64_t batch, int64_t n, float* out);
int dcp_gershgorin_c128(dcp_handle* h, const void* X, int64_t batch, int64_t n, double* out);

/* math_utils/linalg.py:9-38 (inv, "batch version of np.linalg.inv"): out[b] = X[b]^-1 for a batch
 * X[batch, n, n]; Gauss-Jordan with partial pivoting, computed in double precision (complex double) whatever
 * the storage dtype, one workgroup per matrix.  A singular matrix yields inf / nan entries (NumPy raises
 * LinAlgError).  X and out must not overlap.  Asynchronous on the handle's stream. */
int dcp_inv_f32(dcp_handle* h, const float* X, int64_t batch, int64_t n, float* out);
int dcp_inv_f64(dcp_handle* h, const double* X, int64_t batch, int64_t n, double* out);
int dcp_inv_c64(dcp_handle* h, const void* X, int64_t batch, int64_t n, void* out);
int dcp_inv_c128(dcp_handle* h, const void* X, int64_t batch, int64_t n, void* out);

/* Test hook (not a reference interface): C[M,N] = op(A) . op(B) through the same GEMM
 * cores the solvers use.  form: 0 = NT (A[M,K], B[N,K]), 1 = NN (A[M,K], B[K,N]),
 * 2 = TN (A[K,M], B[K,N]).  ksplits >= 1 selects split-K (partials summed in order).
 * tile: 0 = auto, 1 = large tile, 2 = small tile. */
int dcp_gemm_f32(dcp_handle* h, int form, const float* A, const float* B, float* C,
                 int64_t M, int64_t N, int64_t K, int ksplits, int tile);
int dcp_gemm_f64(dcp_handle* h, int form, const double* A, const double* B, double* C,
                 int64_t M, int64_t N, int64_t K, int ksplits, int tile);
/* complex64: form 0 = A B^H, 1 = A B, 2 = A^H B (the conjugations the solvers use) */
int dcp_gemm_c64(dcp_handle* h, int form, const void* A, const void* B, void* C,
                 int64_t M, int64_t N, int64_t K, int ksplits, int tile);
int dcp_gemm_c128(dcp_handle* h, int form, const void* A, const void* B, void* C,
                  int64_t M, int64_t N, int64_t K, int ksplits, int tile);

/* Test hook (not a reference interface): C[M,N] = op(A) . op(B) on the split-bf16 core ("bf16x6": each
 * float32 operand split into three bf16 planes, six bf16 MFMA products per K block, fp32 accumulation; error of
 * the fp32 core's size).  form: 0 = NT, 2 = TN, as dcp_gemm_f32; ksplits >= 1 as there.  Only whole 128 x 128
 * (or 256 x 256) tiles, K % 16 == 0 and 16-byte aligned operands: other shapes return DCP_ERR_INVALID. */
int dcp_gemm_bf16x6_f32(dcp_handle* h, int form, const float* A, const float* B, float* C,
                        int64_t M, int64_t N, int64_t K, int ksplits);

/* Test hooks: the same product with B in two column segments, as the NMF statistics x^T [Y | x] has it: columns
 * < n_b1 from B, the others from B2, each segment a dense array of its own (NT: [n_b1, K] and [N - n_b1, K]; TN:
 * [K, n_b1] and [K, N - n_b1]).  B2 == NULL with n_b1 == N is dcp_gemm_bf16x6_f32.  dcp_gemm_bf16x6_tier says, from
 * the shape alone (16-byte aligned operands taken for granted; n_b1 == N: one segment), which tile that call would
 * run on: 1 = 256 x 256, 0 = 128 x 128, -1 = none (the call fails). */
int dcp_gemm_bf16x6_seg_f32(dcp_handle* h, int form, const float* A, const float* B, const float* B2, float* C,
                            int64_t M, int64_t N, int64_t n_b1, int64_t K, int ksplits);
int dcp_gemm_bf16x6_tier(int form, int64_t M, int64_t N, int64_t n_b1, int64_t K, int ksplits);

/* How the float32 NMF multiplicative-update step (l2 loss, no mask) forms its two large products, Y.D^T and
 * x^T [Y | x], on this handle: mode 0 (default) = split-bf16 core (bf16x6, see dcp_gemm_bf16x6_f32), mode 1 =
 * the exact fp32 MFMA core.  Every other product, dtype and loss always uses its usual core.  mode < 0 only
 * queries.  Returns the previous mode, or a negative error code. */
int dcp_set_f32_product_mode(dcp_handle* h, int mode);

/* Test hook (not a reference interface): the reduction-over-samples products (form 2) run the "pair" LDS schedule
 * of the fp32 MFMA core unless DCP_TN_PLAIN is set in the environment (read once); on != 0 selects the plain
 * schedule, on == 0 the pair schedule, on < 0 only queries.  Returns the previous setting (1 = plain).  Process-wide;
 * tests/test_gpu_gemm.py runs the same products both ways so that a toolchain change that breaks the hand-placed
 * LDS waits of the pair schedule is caught. */
int dcp_debug_tn_plain(int on);

/* Test hook (not a reference interface): how the GEMM front end routes one product.  Pure host arithmetic, no
 * handle and no GPU.  dtype: 0 = float32, 1 = float64, 2 = complex64, 3 = complex128; form, tile and the
 * conjugations as dcp_gemm_*; n_b1 > 0: B in two column segments, the first n_b1 wide; flags: bit 0 = an
 * extended-operand scratch is present (complex), bit 1 = a second row segment of A is present.  target_wgs > 0
 * plans the split-K first (plan_splits(target_wgs, max_splits, min_blocks)); 0 routes one un-planned split.
 * out[13] = core (0 fp32 MFMA, 1 fp64 MFMA, 2 generic), complex image (0 none, 1 ext(B), 2 TN views, 3 rows(A)),
 * the launched tile BM, BN, BK, WM, WN, PIPE, the product as the core sees it M, N, K, and klen, ksplits as the
 * core receives them. */
int dcp_debug_gemm_route(int dtype, int form, int64_t M, int64_t N, int64_t K, int64_t n_b1, int tile, int flags,
                         int target_wgs, int max_splits, int min_blocks, int32_t* out);

/* PMC calibration aid (not a reference interface): reads p[rows, cols] exactly once with the
 * global-load shape of the GEMM panel loaders (pattern 0: 16 rows x 64 B per wave instruction;
 * pattern 1: 512-B row segments), so that rocprofv3 FETCH_SIZE can be compared with a known
 * byte count (tools/calib_fetch.py). */
int dcp_calib_read_f32(dcp_handle* h, const float* p, int64_t rows, int64_t cols, int pattern,
                       float* out);

/* ---- NMF, multiplicative update ------------------------------------------------ */
/* decomp/nmf_methods/batch_mu.py:8-26 (whole loop).  D must already be l2_strict
 * normalised (nmf.py:70).  mask may be NULL.  On return X and D hold what the
 * reference returns: (it, D_new, x) when max|D - D_new| < tol at iteration it,
 * else (maxiter, D, x) after maxiter-1 iterations.  last_maxdiff (host, nullable)
 * receives the last max|D - D_new|; resid_trace (host, nullable, length >= maxiter)
 * receives ||(Y - X D_new) o mask||_F after every iteration (parity metric; costs one
 * extra N.K.F product per iteration, so leave it NULL when timing). */
int dcp_nmf_mu_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D,
                   int64_t N, int64_t F, int64_t K, int likelihood, float tol, int maxiter,
                   int* it_out, float* last_maxdiff, float* resid_trace);
int dcp_nmf_mu_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D,
                   int64_t N, int64_t F, int64_t K, int likelihood, double tol, int maxiter,
                   int* it_out, double* last_maxdiff, double* resid_trace);

/* ---- NMF, HALS (exact block coordinate descent, squared loss, no mask) ------------- */
/* One iteration from (X, D), D with unit-norm rows:
 *   X <- sweep(X, Y D^T, D D^T)                      (N vectors, the rows of X)
 *   D^T <- sweep(D^T, (X^T Y)^T, X^T X)              (F vectors, the columns of D; with the new X)
 *   n_k = ||D_k||_2; where n_k > 0: D_k /= n_k, X[:,k] *= n_k (X D unchanged); where n_k = 0 both stay
 * with sweep() as dcp_nn_cd_sweep_*.  The stop rule, the return convention, last_maxdiff and resid_trace are
 * those of dcp_nmf_mu_*: (it, D_new, X) at the first iteration with max|D - D_new| < tol, else (maxiter, D, X)
 * after maxiter-1 iterations; the test of iteration it-1 is made while iteration it runs, with no host round
 * trip per iteration.  float: Y D^T and X^T [Y | X] follow dcp_set_f32_product_mode. */
int dcp_nmf_hals_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                     float tol, int maxiter, int* it_out, float* last_maxdiff, float* resid_trace);
int dcp_nmf_hals_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                     double tol, int maxiter, int* it_out, double* last_maxdiff, double* resid_trace);
/* HALS for a problem whose ROWS are sharded over the ranks of the handle's communicator (dcp_comm_init or
 * dcp_comm_set_external): Y and X are this rank's rows, D is replicated.  Every iteration runs
 *   D D^T, Y D^T, the x sweep and [x^T Y | x^T x] with the new x on this rank's rows
 *   -> all-reduce(sum) of the [K, F+K] statistics on the handle's stream          (the ONLY exchange)
 *   -> the replicated D sweep and normalisation (identical on every rank), X[:,k] *= n_k on this rank's rows
 * with the stop rule of dcp_nmf_hals_*: no host synchronisation and no second stream inside a step.  Every rank
 * must call it with the same F, K, tol and maxiter; N >= 1 may differ per rank.  it_out, last_maxdiff and D are
 * identical on all ranks.  DCP_ERR_COMM without a communicator. */
int dcp_nmf_hals_sharded_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                             float tol, int maxiter, int* it_out, float* last_maxdiff);
int dcp_nmf_hals_sharded_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                             double tol, int maxiter, int* it_out, double* last_maxdiff);
/* One HALS iteration split at the exchange point, asynchronous on the handle's stream (the HALS counterpart of
 * dcp_nmf_mu_stats_* / dcp_nmf_mu_update_*; run in this order they reproduce dcp_nmf_hals_* bit for bit):
 *   dcp_nmf_hals_stats_*  : G = D D^T, C = Y D^T, X_out = sweep(X, C, G) (X_out may alias X), then this rank's
 *                           stats[K, F+K] = [ X_out^T Y | X_out^T X_out ]  (the caller sums stats over ranks)
 *   dcp_nmf_hals_update_* : U = sweep(D^T, (stats[:, :F])^T, stats[:, F:]) (coordinate-major), D_new = U with
 *                           each row of positive norm n_k scaled to unit norm, X[:,k] *= n_k (X [N, K] in place,
 *                           columns with n_k = 0 unchanged), max|D - D_new| to the DEVICE scalar maxdiff_dev,
 *                           with the maxdiff_next protocol of dcp_nmf_mu_update_* (NULL: maxdiff_dev is set). */
int dcp_nmf_hals_stats_f32(dcp_handle* h, const float* Y, const float* X, float* X_out, const float* D, int64_t N,
                           int64_t F, int64_t K, float* stats);
int dcp_nmf_hals_stats_f64(dcp_handle* h, const double* Y, const double* X, double* X_out, const double* D,
                           int64_t N, int64_t F, int64_t K, double* stats);
int dcp_nmf_hals_update_f32(dcp_handle* h, const float* stats, const float* D, float* D_new, float* X, int64_t N,
                            int64_t F, int64_t K, float* maxdiff_dev, float* maxdiff_next);
int dcp_nmf_hals_update_f64(dcp_handle* h, const double* stats, const double* D, double* D_new, double* X,
                            int64_t N, int64_t F, int64_t K, double* maxdiff_dev, double* maxdiff_next);
/* ---- NMF, em-hals: HALS for data with missing entries (weights mask in [0, 1]) ------------------------ */
/* Y_out[N, F] = mask o Y + (1 - mask) o (X D): the data with its missing part filled in from the model (the E
 * step of EM for weighted low-rank factorisation, Srebro & Jaakkola 2003).  One X D product with the imputation
 * in its epilogue, formed as  fma(w, y, (1 - w) * acc): for finite operands an entry with w == 1 is y and one
 * with w == 0 is (X D) bit for bit.  mask values outside [0, 1] are not checked here.  Y_out must not overlap an
 * input.  Nothing outside Y_out[N, F] is written.  Deterministic.  Asynchronous on the handle's stream. */
int dcp_nmf_impute_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D, int64_t N,
                       int64_t F, int64_t K, float* Y_out);
int dcp_nmf_impute_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                       int64_t N, int64_t F, int64_t K, double* Y_out);
/* em-hals minimises  1/2 sum mask o (Y - X D)^2  (plus the penalty of dcp_set_nmf_penalty).  One iteration from
 * (X, D):  Yi = impute(Y, mask, X, D)  as dcp_nmf_impute_*, then ONE iteration of dcp_nmf_hals_* on Yi (both
 * half-steps read the same Yi).  1/2 |Yi - X' D'|^2 majorises the masked objective and equals it at (X, D), and
 * the HALS iteration does not increase it, so no iteration increases the masked objective; the fewer entries are
 * observed, the slower the convergence.  mask == NULL: exactly dcp_nmf_hals_* (the same kernels).  The stop rule,
 * the return convention, last_maxdiff and the product modes are those of dcp_nmf_hals_*; resid_trace reports
 * ||(Y - X D_new) o mask||_F.  Workspace: N F elements more than dcp_nmf_hals_*.
 * The sharded entries are dcp_nmf_hals_sharded_* with this iteration (Y, mask, X: this rank's rows; the
 * imputation is local to a row, so the exchange is unchanged); DCP_ERR_COMM without a communicator.
 * The split step needs no entry of its own: dcp_nmf_impute_* into a caller's buffer, dcp_nmf_hals_stats_* on
 * that buffer and dcp_nmf_hals_update_* reproduce the loop bit for bit. */
int dcp_nmf_emhals_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N, int64_t F,
                       int64_t K, float tol, int maxiter, int* it_out, float* last_maxdiff, float* resid_trace);
int dcp_nmf_emhals_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D, int64_t N,
                       int64_t F, int64_t K, double tol, int maxiter, int* it_out, double* last_maxdiff,
                       double* resid_trace);
int dcp_nmf_emhals_sharded_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N,
                               int64_t F, int64_t K, float tol, int maxiter, int* it_out, float* last_maxdiff);
int dcp_nmf_emhals_sharded_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D, int64_t N,
                               int64_t F, int64_t K, double tol, int maxiter, int* it_out, double* last_maxdiff);
/* The non-negative coordinate sweep of HALS on R independent vectors: for k = 0 .. K-1 in order, with the
 * current V (coordinates < k already updated),
 *   if G[k,k] > 0:  V[:,k] = max(0, V[:,k] - (V G[:,k] - C[:,k]) / G[k,k])      (else V[:,k] unchanged)
 * G [K, K] symmetric, row-major.  coord_major == 0: V and C are [R, K] (vector r is row r); != 0: they are
 * [K, R] (vector r is column r).  Reads V_in, writes V_out (they may be the same array).  Deterministic. */
int dcp_nn_cd_sweep_f32(dcp_handle* h, const float* V_in, float* V_out, const float* C, const float* G,
                        int64_t R, int64_t K, int coord_major);
int dcp_nn_cd_sweep_f64(dcp_handle* h, const double* V_in, double* V_out, const double* C, const double* G,
                        int64_t R, int64_t K, int coord_major);

/* The same loop for a problem whose ROWS are sharded over the ranks of the handle's communicator
 * (dcp_comm_init): Y, mask, X are this rank's rows, D is replicated.  Every iteration runs
 *   local x update + [x^T Y | x^T x] (or [num | den]) on this rank's rows
 *   -> ncclAllReduce(sum) of the [K, W] statistics on the handle's stream        (the ONLY exchange)
 *   -> the replicated D update, l2_strict and max|D - D_new| (identical on every rank)
 * with the stop test of iteration i read after iteration i+1 has been enqueued, exactly as in
 * dcp_nmf_mu_*: no host synchronisation and no second stream inside a step.  Every rank must call it
 * with the same F, K, likelihood, tol, maxiter and masked-ness; N may differ per rank.  it_out,
 * last_maxdiff and D are identical on all ranks.  DCP_ERR_COMM without a communicator. */
int dcp_nmf_mu_sharded_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D,
                           int64_t N, int64_t F, int64_t K, int likelihood, float tol, int maxiter,
                           int* it_out, float* last_maxdiff);
int dcp_nmf_mu_sharded_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D,
                           int64_t N, int64_t F, int64_t K, int likelihood, double tol, int maxiter,
                           int* it_out, double* last_maxdiff);

/* One iteration split at the data-parallel exchange point, asynchronous:
 *   dcp_nmf_mu_stats_*  : X_out <- update_x(X) (grads.py:77-84; X_out may alias X, or be a
 *                         second buffer so that the caller can overlap the stop test of the
 *                         previous iteration), then this rank's share of the D-side sums
 *                         (grads.py:117-125, with the NEW x) into stats:
 *                           l2, no mask : stats[K, F+K] = [ x^T Y | x^T x ]
 *                           otherwise   : stats[K, 2F]  = [ numerator | denominator ]
 *                         (the caller all-reduces stats over ranks: sums over rows)
 *   dcp_nmf_mu_update_* : D_new <- l2_strict(D o max(num,0) / max(den,1e-15))
 *                         (grads.py:86-93, batch_mu.py:21) written to D_new, and
 *                         max|D - D_new| written to the DEVICE scalar maxdiff_dev.
 *                         maxdiff_next (nullable): when given, *maxdiff_dev must be 0 on
 *                         entry, the max is formed by one atomic per row (no extra launch)
 *                         and *maxdiff_next is cleared for the following iteration.
 * stats width: dcp_nmf_mu_stats_width(). */
int64_t dcp_nmf_mu_stats_width(int64_t F, int64_t K, int likelihood, int masked);
int dcp_nmf_mu_stats_f32(dcp_handle* h, const float* Y, const float* mask, const float* X,
                         float* X_out, const float* D, int64_t N, int64_t F, int64_t K,
                         int likelihood, float* stats);
int dcp_nmf_mu_stats_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                         double* X_out, const double* D, int64_t N, int64_t F, int64_t K,
                         int likelihood, double* stats);
/* Loop-invariant mask work of a masked run, done ONCE instead of in every dcp_nmf_mu_stats_* call
 * (grads.py:114,124 recompute y * mask per gradient): Ym[N,F] = Y o mask, and -- float32 only, `bits`
 * non-NULL -- the row-bit image of the mask (dcp_nmf_mask_bits_words(N, F) uint32 words: word
 * (row / 32, col) holds mask[32 (row/32) + b, col] != 0 in bit b).  *binary (HOST) = 1 when every mask
 * entry is exactly 0 or 1, i.e. when `bits` may be passed to dcp_nmf_mu_stats_prepared_* (otherwise pass
 * NULL there).  dcp_nmf_mu_stats_prepared_*: dcp_nmf_mu_stats_* on (Ym, mask[, bits]); with bits the
 * (x D) o M products multiply by bits fetched ahead of the GEMM main loop instead of loading the float
 * mask in the epilogue.  Results are identical with and without bits. */
int64_t dcp_nmf_mask_bits_words(int64_t N, int64_t F);
int dcp_nmf_mask_prepare_f32(dcp_handle* h, const float* Y, const float* mask, int64_t N, int64_t F,
                             float* Ym, uint32_t* bits, int* binary);
int dcp_nmf_mask_prepare_f64(dcp_handle* h, const double* Y, const double* mask, int64_t N, int64_t F,
                             double* Ym, uint32_t* bits, int* binary);
int dcp_nmf_mu_stats_prepared_f32(dcp_handle* h, const float* Ym, const float* mask, const uint32_t* bits,
                                  const float* X, float* X_out, const float* D, int64_t N, int64_t F,
                                  int64_t K, int likelihood, float* stats);
int dcp_nmf_mu_stats_prepared_f64(dcp_handle* h, const double* Ym, const double* mask, const uint32_t* bits,
                                  const double* X, double* X_out, const double* D, int64_t N, int64_t F,
                                  int64_t K, int likelihood, double* stats);
int dcp_nmf_mu_update_f32(dcp_handle* h, const float* stats, const float* D, float* D_new,
                          int64_t F, int64_t K, int likelihood, int masked,
                          float* maxdiff_dev, float* maxdiff_next);
int dcp_nmf_mu_update_f64(dcp_handle* h, const double* stats, const double* D, double* D_new,
                          int64_t F, int64_t K, int likelihood, int masked,
                          double* maxdiff_dev, double* maxdiff_next);

/* Building blocks of the stochastic MU variants (decomp/nmf_methods/serizel.py:36-165,
 * kasai.py:36-88), which are host loops over minibatches around the same gradients:
 *   dcp_nmf_grads_*: n_x_updates times  x_mb <- x_mb o max(gx+,0)/max(gx-,1e-15)  in place
 *                    (serizel.py:46-49, kasai.py:63-67), then the two parts of the D gradient
 *                    (grads.py:117-125, 152-160) of that minibatch into grad_pos / grad_neg [K,F].
 *   dcp_nmf_apply_*: D_new = l2_strict(rule) and max|D - D_new| to the host:
 *                    alpha <  0: D o max(P,0)/max(Q,1e-15)                 (serizel.py:54-57)
 *                    alpha >= 0: max(D o ((1-alpha) + alpha P/max(Q,1e-15)), 0)  (kasai.py:77-78)
 *   dcp_axpby_*    : y = a x + b y  (gradient averaging serizel.py:95-96, kasai.py:74-75); a zero
 *                    coefficient means its operand is not read (y may be uninitialised when b = 0);
 *                    x may alias y. */
int dcp_nmf_grads_f32(dcp_handle* h, const float* Y, const float* mask, float* X, const float* D,
                      int64_t N, int64_t F, int64_t K, int likelihood, int n_x_updates,
                      float* grad_pos, float* grad_neg);
int dcp_nmf_grads_f64(dcp_handle* h, const double* Y, const double* mask, double* X, const double* D,
                      int64_t N, int64_t F, int64_t K, int likelihood, int n_x_updates,
                      double* grad_pos, double* grad_neg);
/* Gaussian.grad_x / Poisson.grad_x (decomp/nmf_methods/grads.py:108-115, 143-150), the plugin surface a
 * user subclass reaches through super(): grad_pos, grad_neg [N, K].  Without a mask the l2 negative part
 * is x (D D^T) (the Gram identity of (x D) D^T) and the kl negative part -- the reference's [1, K] row
 * d.T.sum(axis=0) -- is repeated on every row.  X is not modified.  Asynchronous. */
int dcp_nmf_grad_x_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                       int64_t N, int64_t F, int64_t K, int likelihood, float* grad_pos, float* grad_neg);
int dcp_nmf_grad_x_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                       int64_t N, int64_t F, int64_t K, int likelihood, double* grad_pos, double* grad_neg);
/* Gaussian.logp (grads.py:127-135): sum((-0.5 ((y - x d) / scale)^2 - log(scale) - pi / 2) [* mask]) to the
 * HOST double (accumulated in double precision).  Synchronises. */
int dcp_nmf_gauss_logp_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                           int64_t N, int64_t F, int64_t K, double scale, double* out);
int dcp_nmf_gauss_logp_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                           int64_t N, int64_t F, int64_t K, double scale, double* out);
/* beta of DCP_LIK_BETA on this handle (default 0, Itakura-Saito).  Handle state like the stream and
 * dcp_set_f32_product_mode: read when a call that passes DCP_LIK_BETA is enqueued, so set it before each such
 * call when several betas share a handle.  DCP_ERR_INVALID for a NULL handle or a non-finite beta.
 * With DCP_LIK_BETA every NMF entry that takes `likelihood` runs the beta-divergence MU rule (Fevotte & Idier
 * 2011, the reference's update_x / update_d applied to these parts), V = X D + 1e-15, M = mask or 1:
 *   R1 = (Y o M) o V^(beta-2),  R2 = M o V^(beta-1)
 *   x: pos = R1 D^T, neg = R2 D^T  [N, K]      D: pos = X^T R1, neg = X^T R2  [K, F]
 * statistics width 2F ([X^T R1 | X^T R2]), mask or not.  No Gram identity applies. */
int dcp_set_nmf_beta(dcp_handle* h, double beta);
/* L1 / L2 penalty on the NMF codes on this handle (default 0, 0): the objective gains  l1 sum X + l2/2 |X|^2
 * (no 1/N scaling; D stays unpenalised, its rows unit norm).  Handle state like dcp_set_nmf_beta, read when a
 * call is enqueued by exactly these entries:
 *   dcp_nmf_mu_*, dcp_nmf_mu_sharded_*, dcp_nmf_mu_stats_*, dcp_nmf_mu_stats_prepared_*   the MU x update
 *       x <- x * max(pos, 0) / max(neg + l1 + l2 x, 1e-15)    (x before the update; pos / neg as without it)
 *   dcp_nmf_hals_*, dcp_nmf_hals_sharded_*, dcp_nmf_hals_stats_*                           the HALS x sweep
 *   dcp_nmf_emhals_*, dcp_nmf_emhals_sharded_*                                  (the same sweep, on the imputed data)
 *       the exact coordinate minimiser: the sweep on C = Y D^T - l1 and G = D D^T + l2 I, i.e. where
 *       G[k,k] + l2 > 0:  X[:,k] = max(0, X[:,k] - (X G[:,k] + l2 X[:,k] - C[:,k] + l1) / (G[k,k] + l2))
 * Every other entry ignores it (dcp_nmf_grads_*, dcp_nmf_grad_x_*, dcp_nn_cd_sweep_*, the D updates, the
 * dictionary and lasso entries).  The D side, the statistics and the stop rule are unchanged; with both
 * penalties 0 the unpenalised kernels run.  DCP_ERR_INVALID for a NULL handle or a negative or non-finite value. */
int dcp_set_nmf_penalty(dcp_handle* h, double l1, double l2);
/* sum over entries with mask != 0 of mask * d_beta(Y | X D + 1e-15) with the handle's beta, to the HOST double
 * (per-element divergence and accumulation in double, ordered second-stage sum: deterministic).  d_0 = y/v -
 * log(y/v) - 1, d_1 = y log(y/v) - y + v (0 log 0 = 0), else (y^b + (b-1) v^b - b y v^(b-1)) / (b (b-1)).
 * Valid for every beta.  Synchronises. */
int dcp_nmf_beta_divergence_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                                int64_t N, int64_t F, int64_t K, double* out);
int dcp_nmf_beta_divergence_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                                const double* D, int64_t N, int64_t F, int64_t K, double* out);
int dcp_nmf_apply_f32(dcp_handle* h, const float* D, const float* P, const float* Q, double alpha,
                      float* D_new, int64_t K, int64_t F, double* maxdiff);
int dcp_nmf_apply_f64(dcp_handle* h, const double* D, const double* P, const double* Q, double alpha,
                      double* D_new, int64_t K, int64_t F, double* maxdiff);
int dcp_axpby_f32(dcp_handle* h, int64_t n, double a, const float* x, double b, float* y);
int dcp_axpby_f64(dcp_handle* h, int64_t n, double a, const double* x, double b, double* y);

/* Likelihood.update_x / update_d (decomp/nmf_methods/grads.py:77-93), the multiplicative rule a
 * user-supplied Likelihood subclass inherits:  out = cur o max(pos, 0) / max(neg, 1e-15), all
 * [rows, cols] contiguous (out may alias cur).  Asynchronous on the handle's stream. */
int dcp_mu_quotient_f32(dcp_handle* h, const float* cur, const float* pos, const float* neg,
                        int64_t rows, int64_t cols, float* out);
int dcp_mu_quotient_f64(dcp_handle* h, const double* cur, const double* pos, const double* neg,
                        int64_t rows, int64_t cols, double* out);
/* The tail of one MU iteration for a caller-produced U (batch_mu.py:21-22 with a user Likelihood):
 * out = l2_strict(U) (strict != 0) or l2(U), *maxdiff (HOST) = max |ref - out|.  Synchronises. */
int dcp_l2_normalize_diff_f32(dcp_handle* h, const float* U, const float* ref, float* out, int64_t K,
                              int64_t F, int strict, double* maxdiff);
int dcp_l2_normalize_diff_f64(dcp_handle* h, const double* U, const double* ref, double* out, int64_t K,
                              int64_t F, int strict, double* maxdiff);

/* ||(Y - X D) o mask||_F (parity metric of SURVEY 8d; mask nullable). */
int dcp_nmf_residual_f32(dcp_handle* h, const float* Y, const float* mask, const float* X,
                         const float* D, int64_t N, int64_t F, int64_t K, double* out);
int dcp_nmf_residual_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                         const double* D, int64_t N, int64_t F, int64_t K, double* out);

/* ---- batched LASSO / NNLS ---------------------------------------------------------- */
/* decomp/lasso.py:97-189 (solve_fastpath, everything after validation):
 *   argmin_x 1/(2n) |y - x A|^2 + alpha |x|_1  for every row of Y[N,F] (batch dims
 *   flattened by the caller), A[K,F], X[N,K] in: initial estimate, out: solution.
 * mask: NULL (mask_ndim 0), [F] (mask_ndim 1, lasso.py:120-122) or [N,F] (mask_ndim 2,
 * lasso.py:160-186), real dtype of the problem.  method: DCP_LASSO_*; positive != 0 selects
 * the `_pos` (NNLS) proximal operator (real dtypes only, lasso.py:92).
 * *it_out (host) is the reference's iteration count: the index of the first iteration
 * i % 10 == 0 at which max(|dx| - tol) < 0, else maxiter - 1 (with the reference's
 * choice of returned iterate per method, lasso.py:297,357,415).  Coordinate descent has no size
 * limit (K <= 2048: a row's coefficients live in one wave's registers; wider: in that row's memory).
 * Synchronises the stream before returning. */
int dcp_lasso_f32(dcp_handle* h, const float* Y, const float* mask, int mask_ndim, const float* A,
                  float* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                  int method, int positive, int* it_out);
int dcp_lasso_f64(dcp_handle* h, const double* Y, const double* mask, int mask_ndim, const double* A,
                  double* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                  int method, int positive, int* it_out);
int dcp_lasso_c64(dcp_handle* h, const void* Y, const float* mask, int mask_ndim, const void* A,
                  void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                  int method, int positive, int* it_out);
int dcp_lasso_c128(dcp_handle* h, const void* Y, const double* mask, int mask_ndim, const void* A,
                   void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                   int method, int positive, int* it_out);

/* decomp/lasso.py:448-523 `_solve_parallel_cd(_mask)`: every iteration evaluates the unit-step
 * proximal update of all coordinates and commits it on p = int(K / Gershgorin(A A^H)) of them,
 * chosen by a 0/1 vector that the reference re-shuffles with np.random.RandomState(0) each
 * iteration.  The RNG stream is host state, so the caller supplies it: `order` is a DEVICE
 * int32 [order_rows, K] table, row i = arange(K) after i + 1 cumulative RandomState(0).shuffle
 * calls (a shuffle's swap sequence does not depend on the array's content); coordinate k is
 * committed in iteration i iff order[i, k] < p.  order_rows >= maxiter.  p <= 1: the library
 * runs plain coordinate descent as the reference does (lasso.py:469-470); with a 2-D mask the
 * reference's fallback call is broken (lasso.py:509) and DCP_ERR_REF_TYPEERROR is returned. */
int dcp_lasso_pcd_f32(dcp_handle* h, const float* Y, const float* mask, int mask_ndim, const float* A,
                      float* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                      int positive, const int32_t* order, int64_t order_rows, int* it_out);
int dcp_lasso_pcd_f64(dcp_handle* h, const double* Y, const double* mask, int mask_ndim, const double* A,
                      double* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                      int positive, const int32_t* order, int64_t order_rows, int* it_out);
int dcp_lasso_pcd_c64(dcp_handle* h, const void* Y, const float* mask, int mask_ndim, const void* A,
                      void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                      int positive, const int32_t* order, int64_t order_rows, int* it_out);
int dcp_lasso_pcd_c128(dcp_handle* h, const void* Y, const double* mask, int mask_ndim, const void* A,
                       void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                       int positive, const int32_t* order, int64_t order_rows, int* it_out);

/* decomp/lasso.py:586-657 `_solve_admm(_mask)` with penalty rho (dcp_lasso_* with
 * DCP_LASSO_ADMM uses rho = 1.0 like solve_fastpath).  (A A^H + rho I)^-1 is formed on the
 * device in double precision (math_utils/linalg.py:9-16); a 2-D mask needs one K x K system
 * per row (N K^2 workspace, as the reference's lasso.py:643; K <= 10240 real / 5120 complex). */
int dcp_lasso_admm_f32(dcp_handle* h, const float* Y, const float* mask, int mask_ndim, const float* A,
                       float* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                       int positive, double rho, int* it_out);
int dcp_lasso_admm_f64(dcp_handle* h, const double* Y, const double* mask, int mask_ndim, const double* A,
                       double* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                       int positive, double rho, int* it_out);
int dcp_lasso_admm_c64(dcp_handle* h, const void* Y, const float* mask, int mask_ndim, const void* A,
                       void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                       int positive, double rho, int* it_out);
int dcp_lasso_admm_c128(dcp_handle* h, const void* Y, const double* mask, int mask_ndim, const void* A,
                        void* X, int64_t N, int64_t F, int64_t K, double alpha, double tol, int maxiter,
                        int positive, double rho, int* it_out);

/* ---- orthogonal matching pursuit (not in the reference; csrc/omp.hpp) ------------------------ */
/* argmin_x |y - x A|^2  s.t.  |x|_0 <= n_nonzero  for every row of Y[N,F], A[K,F], greedily (batch OMP in Gram
 * form, Rubinstein, Zibulevsky & Elad 2008): at most n_nonzero times, stop when tol >= 0 and |r|^2 <= tol; pick the
 * atom k outside the support with the largest |r . a_k^H| / |a_k| (lowest index on ties; zero atoms never; stop when
 * that maximum is <= 0); stop when its Cholesky pivot d = G_kk - |w|^2 <= 4096 eps G_kk (the atom is numerically in
 * the span of the support: the previous solution is kept); else add it and solve the least squares on the support
 * through the extended Cholesky factor.  X[N,K] is written in full (zeros off the support; the coefficients are
 * those for the caller's A); no initial estimate is read.  tol < 0: no residual stop.  n_nonzero in
 * [1, min(K, cap)], cap = 64 for real and 32 for complex dtypes, else DCP_ERR_INVALID.  *it_out (host) = the
 * largest number of atoms any row selected.  Bitwise reproducible.  Synchronises the stream before returning.
 *   dcp_omp_*      : alpha0 = Y A^H and G = A A^H on the GEMM cores, then the greedy kernel.
 *   dcp_omp_gram_* : the greedy kernel alone on the caller's alpha0[N,K] (= Y A^H), G[K,K] (= A A^H, Hermitian)
 *                    and ynorm2[N] (= |y|^2 per row, real; may be NULL when tol < 0). */
int dcp_omp_f32(dcp_handle* h, const float* Y, const float* A, float* X, int64_t N, int64_t F, int64_t K,
                int n_nonzero, double tol, int* it_out);
int dcp_omp_f64(dcp_handle* h, const double* Y, const double* A, double* X, int64_t N, int64_t F, int64_t K,
                int n_nonzero, double tol, int* it_out);
int dcp_omp_c64(dcp_handle* h, const void* Y, const void* A, void* X, int64_t N, int64_t F, int64_t K,
                int n_nonzero, double tol, int* it_out);
int dcp_omp_c128(dcp_handle* h, const void* Y, const void* A, void* X, int64_t N, int64_t F, int64_t K,
                 int n_nonzero, double tol, int* it_out);
int dcp_omp_gram_f32(dcp_handle* h, const float* alpha0, const float* G, const float* ynorm2, float* X,
                     int64_t N, int64_t K, int n_nonzero, double tol, int* it_out);
int dcp_omp_gram_f64(dcp_handle* h, const double* alpha0, const double* G, const double* ynorm2, double* X,
                     int64_t N, int64_t K, int n_nonzero, double tol, int* it_out);
int dcp_omp_gram_c64(dcp_handle* h, const void* alpha0, const void* G, const float* ynorm2, void* X,
                     int64_t N, int64_t K, int n_nonzero, double tol, int* it_out);
int dcp_omp_gram_c128(dcp_handle* h, const void* alpha0, const void* G, const double* ynorm2, void* X,
                      int64_t N, int64_t K, int n_nonzero, double tol, int* it_out);

/* ---- masked orthogonal matching pursuit (not in the reference; csrc/omp_mask.hpp) ------------- */
/* argmin_x sum_f m_f |y_f - (x A)_f|^2  s.t.  |x|_0 <= n_nonzero  for every row of Y[N,F], A[K,F], with non-negative
 * weights M in the real type: [F] (mask_ndim 1, shared by all rows) or [N,F] (mask_ndim 2, a row of its own for every
 * row of Y), as in dcp_lasso_*.  The weights enter linearly (m, not m^2).  The algorithm is that of dcp_omp_* with
 * every inner product weighted, <u, v>_m = sum_f m_f u_f conj(v_f): the residual stop is sum m |r|^2 <= tol, the
 * selection score |<r, a_k>_m| / n_k with n_k^2 = sum_f m_f |a_kf|^2 of THAT row (an atom whose observed part vanishes
 * in a row is never selected there; a row whose weights are all zero gets x = 0 and takes no step), the pivot test
 * d <= 4096 eps n_k*^2.  n_nonzero, tol, the sizes, X, *it_out and the error codes are those of dcp_omp_*; mask_ndim
 * other than 1 or 2, a negative rows_per_pass or a null M: DCP_ERR_INVALID.
 *   mask_ndim 1 : Y and A are scaled by sqrt(m) into workspace and dcp_omp_* runs on them.
 *   mask_ndim 2 : the residual form, in passes of rows_per_pass rows (0: the library chooses the fewest equal passes
 *                 whose per-row workspace -- the packed Cholesky factor, alpha, the weighted norms and the residual
 *                 image -- stays within 1 GiB).  Per pass the weighted squared norms M (|A|^2)^T, then n_nonzero
 *                 times: alpha = (m o r) A^H on the GEMM cores and one step kernel (selection, the weighted dot
 *                 products of the pivot, the factor's new row, both substitutions, r rebuilt from y).  No host round
 *                 trip between the steps.
 * Bitwise reproducible; the rows are independent, so the result does not depend on rows_per_pass as long as the
 * products of every pass take the same GEMM tile.  Synchronises the stream before returning.  With dcp_profile_*
 * on, the products of the steps are timed under DCP_PROF_GRAM, the step kernels under DCP_PROF_XUPDATE and the rest
 * under DCP_PROF_MISC. */
int dcp_omp_mask_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, const float* A, float* X,
                     int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass, int* it_out);
int dcp_omp_mask_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, const double* A, double* X,
                     int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass, int* it_out);
int dcp_omp_mask_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, const void* A, void* X,
                     int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass, int* it_out);
int dcp_omp_mask_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, const void* A, void* X,
                      int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass, int* it_out);

/* ---- approximate K-SVD (not in the reference; csrc/ksvd.hpp) ---------------------------------- */
/* min |Y - X D|^2  s.t.  |x_i|_0 <= s, |d_k| = 1  for Y[N,F], X[N,K], D[K,F] (Rubinstein, Zibulevsky & Elad 2008).
 * The atom sweep, on R = Y - X D formed once on the GEMM cores: for k = 0 .. K-1 in order, with I the rows where
 * X[i,k] != 0 (ascending, fixed for the sweep), g = X[I,k], d = D[k]:  u = g^H R[I,:] + |g|^2 d;  d' = u / |u| (d is
 * kept where !(|u| > 0));  g' = R[I,:] d'^H + g (d . d'^H);  R[I,:] += g d - g' d';  X[I,k] = g';  D[k] = d'.  An atom
 * no row uses is left as it is.  The sweep never increases |Y - X D|^2.  *maxdiff_out (host) = max |D_new - D_old|
 * over all entries.  Bitwise reproducible.  Both families synchronise the stream before returning.
 *   dcp_ksvd_sweep_* : the residual and the sweep on the caller's X and D, both updated in place.  row_nnz_max in
 *                      [1, K] bounds the non-zeros of a row of X (it sizes the lists): a row with more gives
 *                      DCP_ERR_INVALID before X or D is written.
 *   dcp_ksvd_step_*  : X = dcp_omp_*(Y, D, n_nonzero, coef_tol) (X is written in full; the limits on n_nonzero and
 *                      coef_tol are those of dcp_omp_*; *it_out = its step count), then the residual and the sweep.
 *                      D should have unit rows on entry. */
int dcp_ksvd_sweep_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                       int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_sweep_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                       int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_sweep_c64(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                       int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_sweep_c128(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                        int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_step_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                      int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out);
int dcp_ksvd_step_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                      int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out);
int dcp_ksvd_step_c64(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                      int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out);
int dcp_ksvd_step_c128(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                       int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out);

/* ---- masked approximate K-SVD (not in the reference; csrc/ksvd_mask.hpp) ------------------------ */
/* min sum_if M_if |Y_if - (X D)_if|^2  s.t.  |x_i|_0 <= s, |d_k| = 1: dcp_ksvd_* for data with holes.  M: non-negative
 * weights in the real type, [F] (mask_ndim 1) or [N,F] (mask_ndim 2), entering linearly, as in dcp_omp_mask_*.  Y must
 * be finite at hidden entries (M = 0) too; its values there do not influence the result.  The atom sweep, on
 * R = Y - X D formed once: for k = 0 .. K-1 in order, I the rows where X[i,k] != 0, g = X[I,k], d = D[k], m_i = M[i,:]:
 *   c_f = sum_I m_if |g_i|^2;  n_f = sum_I m_if conj(g_i) R_if + c_f d_f;  u_f = n_f / c_f (d_f where !(c_f > 0));
 *   d' = u / |u| (d where !(|u| > 0));  q_i = sum_f m_if |d'_f|^2;
 *   g'_i = (sum_f m_if R_if conj(d'_f) + g_i sum_f m_if d_f conj(d'_f)) / q_i (0 where !(q_i > 0));
 *   R[I,:] += g d - g' d';  X[I,k] = g';  D[k] = d'.
 * u minimises the weighted objective over the atom for fixed g, the normalisation leaves it unchanged and g' minimises
 * it over the coefficients for d', so the sweep never increases it.  With M = 1 this is the sweep of dcp_ksvd_sweep_*
 * up to rounding.  A 1-D mask and its [N,F] broadcast give the same bits.  Bitwise reproducible; both families
 * synchronise the stream before returning.  *maxdiff_out, row_nnz_max, n_nonzero, coef_tol and *it_out are those of
 * dcp_ksvd_*; rows_per_pass and the coder are those of dcp_omp_mask_* (coef_tol bounds the weighted residual).
 * A null pointer, sizes outside [1, 2^31-1], mask_ndim other than 1 or 2, a negative rows_per_pass, a NaN coef_tol, a
 * sparsity beyond the cap or K, row_nnz_max outside [1, K] or below a row's count: DCP_ERR_INVALID with a message,
 * before anything is written. */
int dcp_ksvd_mask_sweep_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X, float* D,
                            int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_mask_sweep_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X, double* D,
                            int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_mask_sweep_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                            int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_mask_sweep_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X, void* D,
                             int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out);
int dcp_ksvd_mask_step_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X, float* D,
                           int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                           double* maxdiff_out, int* it_out);
int dcp_ksvd_mask_step_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X, double* D,
                           int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                           double* maxdiff_out, int* it_out);
int dcp_ksvd_mask_step_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                           int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                           double* maxdiff_out, int* it_out);
int dcp_ksvd_mask_step_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X, void* D,
                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                            double* maxdiff_out, int* it_out);

/* ---- K-SVD: replacement of unused and duplicate atoms (not in the reference; csrc/ksvd_clean.hpp) ---------- */
/* One cleaning pass on what a sweep leaves behind: X, D, R = Y - X D, the mask M (1 without one: M null with
 * mask_ndim 0) and cnt_k, the non-zeros of column k of X.
 *   marking      k = 0 .. K-1 in order, G = D D^H in the working dtype: atom k is marked if cnt_k == 0, or if
 *                max_coherence > 0 and there is a j < k, itself not marked, with |G_kj| > max_coherence.  A marked
 *                atom never marks another; of a coherent pair the lower index survives.
 *   ranking      e_i = sum_f M_if |R_if|^2 (0 where !(e_i > 0)); rows by e descending, ties to the lower row.
 *   replacement  the j-th marked atom (ascending) takes the j-th row i: z_f = Y_if where M_if > 0, elsewhere
 *                sum_k X_ik D_kf from the row's non-zeros and the given D (never Y - R: Y at hidden entries does not
 *                influence the result).  D[k] = z / |z| if e_i > 0 and |z| > 0, otherwise (NaN included, or no row
 *                left) the atom is kept.  Every z is formed before any atom is written.  X is not touched.
 * Bitwise reproducible.
 *   dcp_ksvd_clean_*      : forms R = Y - X D as dcp_ksvd_sweep_* does and runs one pass on the caller's X and D
 *                           (D updated in place); *n_marked_out, *n_replaced_out (host): atoms marked / replaced.
 *                           Synchronises the stream before returning.
 *   dcp_ksvd_clean_step_* : dcp_ksvd_mask_step_* (or, with M null and mask_ndim 0, dcp_ksvd_step_*; rows_per_pass is
 *                           then ignored), then the pass on the sweep's own R.  The marking always runs and
 *                           *n_marked_out comes back in the synchronisation that reads *maxdiff_out; the replacement
 *                           is enqueued only if *n_marked_out > 0 and *maxdiff_out >= stop_tol (stop_tol = +inf:
 *                           never; a NaN maxdiff: never) and may still be in flight on the handle's stream on return.
 *                           *maxdiff_out is that of the sweep: the jump of a replaced atom does not enter it.
 * DCP_ERR_INVALID with a message, before X or D is written: what the step entries refuse, a null pointer (M aside),
 * mask_ndim outside {0, 1, 2} or not matching M, a NaN max_coherence or stop_tol. */
int dcp_ksvd_clean_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, const float* X, float* D,
                       int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out, int* n_replaced_out);
int dcp_ksvd_clean_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, const double* X, double* D,
                       int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out, int* n_replaced_out);
int dcp_ksvd_clean_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, const void* X, void* D, int64_t N,
                       int64_t F, int64_t K, double max_coherence, int* n_marked_out, int* n_replaced_out);
int dcp_ksvd_clean_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, const void* X, void* D, int64_t N,
                       int64_t F, int64_t K, double max_coherence, int* n_marked_out, int* n_replaced_out);
int dcp_ksvd_clean_step_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X, float* D,
                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                            double* maxdiff_out, int* it_out, double max_coherence, double stop_tol,
                            int* n_marked_out);
int dcp_ksvd_clean_step_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X, double* D,
                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                            double* maxdiff_out, int* it_out, double max_coherence, double stop_tol,
                            int* n_marked_out);
int dcp_ksvd_clean_step_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                            double* maxdiff_out, int* it_out, double max_coherence, double stop_tol,
                            int* n_marked_out);
int dcp_ksvd_clean_step_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X, void* D,
                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                            double* maxdiff_out, int* it_out, double max_coherence, double stop_tol,
                            int* n_marked_out);

/* ---- row movers of the minibatch containers (decomp/utils/data.py:124-156, 214-313) ------ */
/* gather : out[i, :] = in[index[i], :]      scatter: out[index[i], :] = in[i, :]      i < rows
 * Rows are row_bytes long (any dtype); index: int64 in DEVICE memory.  `in` / `out` may be
 * device memory or PINNED host memory (hipHostMalloc; mapped into the device's address space):
 * the out-of-core container gathers each shuffled minibatch straight out of the host array over
 * PCIe and scatters updated rows back, so no shuffle pass over the host data is ever needed.
 * Asynchronous on the handle's stream. */
int dcp_gather_rows_bytes(dcp_handle* h, const void* in, const int64_t* index, int64_t rows,
                          int64_t row_bytes, void* out);
int dcp_scatter_rows_bytes(dcp_handle* h, const void* in, const int64_t* index, int64_t rows,
                           int64_t row_bytes, void* out);

/* Registers ONE row gather (out[i, :] = in[index[i], :], as dcp_gather_rows_bytes) that the NEXT dcp_dict_step_*
 * / dcp_dict_step_async_* call on this handle runs on the library's side stream beside its atom sweep (after its
 * statistics product, joined before the step's last kernel): the rows of minibatch s + 1 are staged while step s
 * leaves the chip and its HBM nearly idle (decomp/utils/data.py:152-156 gathers all of y once per epoch instead).
 * Use a second staging block for `out`.  Everything enqueued on the
 * handle's stream after that step sees the gathered rows.  rows = 0 clears a pending registration. */
int dcp_dict_prefetch_rows_bytes(dcp_handle* h, const void* in, const int64_t* index, int64_t rows,
                                 int64_t row_bytes, void* out);

/* parallel_cd as the inner solver of the dictionary step (dcp_dict_*): the shuffle table of
 * dcp_lasso_pcd_* (DEVICE int32 [rows, K], rows >= lasso_iter), remembered by the handle until
 * replaced or cleared with order = NULL.  The reference restarts RandomState(0) in every call of the
 * solver (lasso.py:463), so one table serves every minibatch.  The memory stays owned by the caller. */
int dcp_dict_set_pcd_order(dcp_handle* h, const int32_t* order, int64_t rows, int64_t K);

/* ---- online dictionary learning (block coordinate descent) -------------------------- */
/* One minibatch step of decomp/dictionary_learning.py:135-164 (solve_cd), split at the
 * data-parallel exchange point like the NMF step:
 *   dcp_dict_stats_*  : x_mb <- lasso.solve_fastpath(y_mb, D, alpha, x_mb, lasso_tol,
 *                       lasso_iter, lasso_method) (in place), then this rank's
 *                       stats[K, F+K] = x_mb^H [ y_mb | x_mb ]   (lines 137-152)
 *   dcp_dict_update_* : A <- beta A + stats[:, F:], B <- beta B + stats[:, :F] (147-152),
 *                       the sequential atom sweep into D_new (154-159), and max|D - D_new|
 *                       into the DEVICE scalar maxdiff_dev (161).  Asynchronous.
 *   dcp_dict_step_*   : both on one GPU; max|D - D_new| returned to the HOST double.
 *   dcp_dict_step_async_* : the same step with max|D - D_new| left in the DEVICE scalar maxdiff_dev and no
 *                       wait for the GPU: the caller evaluates the stop test (line 161-162) one step late,
 *                       when the next minibatch is already enqueued (decomp_amd.dictionary_learning).
 *                       maxdiff_dev may be device memory or pinned, device-mapped host memory (hipHostMalloc): the
 *                       step's last kernel stores the value with a plain store, so a caller that puts a sentinel
 *                       (-1; max|.| >= 0 or NaN) into a pinned word before the call can poll it instead of
 *                       recording an event -- a recorded event is a barrier packet that idles the stream ~6 us.
 *                       *lasso_it (host) is final when the call returns (a coordinate-descent solve settles it at the
 *                       end of the step, when its stop flag has landed in pinned memory; nothing waits mid-step).
 * D [K,F] must be l2_strict-normalised by the caller on entry of the run (line 126); A [K,K]
 * and B [K,F] are the running statistics (zero before the first step). */
int dcp_dict_stats_f32(dcp_handle* h, const float* Y, float* X, const float* D, int64_t Nb, int64_t F,
                        int64_t K, double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                        float* stats, int* lasso_it);
int dcp_dict_update_f32(dcp_handle* h, const float* stats, double beta, float* A, float* B, const float* D,
                         float* D_new, int64_t F, int64_t K, float* maxdiff_dev);
int dcp_dict_step_f32(dcp_handle* h, const float* Y, float* X, const float* D, float* D_new, float* A, float* B,
                       int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                       int lasso_iter, double lasso_tol, double* maxdiff, int* lasso_it);
int dcp_dict_step_async_f32(dcp_handle* h, const float* Y, float* X, const float* D, float* D_new, float* A, float* B,
                             int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                             int lasso_iter, double lasso_tol, float* maxdiff_dev, int* lasso_it);
/* out[i, :] = in[index[i], :]  (MinibatchData.shuffle / .array, decomp/utils/data.py:147-156);
 * index: int64 on the device. */
int dcp_gather_rows_f32(dcp_handle* h, const float* in, const int64_t* index, int64_t rows,
                         int64_t cols, float* out);
int dcp_dict_stats_f64(dcp_handle* h, const double* Y, double* X, const double* D, int64_t Nb, int64_t F,
                        int64_t K, double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                        double* stats, int* lasso_it);
int dcp_dict_update_f64(dcp_handle* h, const double* stats, double beta, double* A, double* B, const double* D,
                         double* D_new, int64_t F, int64_t K, double* maxdiff_dev);
int dcp_dict_step_f64(dcp_handle* h, const double* Y, double* X, const double* D, double* D_new, double* A, double* B,
                       int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                       int lasso_iter, double lasso_tol, double* maxdiff, int* lasso_it);
int dcp_dict_step_async_f64(dcp_handle* h, const double* Y, double* X, const double* D, double* D_new, double* A, double* B,
                             int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                             int lasso_iter, double lasso_tol, double* maxdiff_dev, int* lasso_it);
/* out[i, :] = in[index[i], :]  (MinibatchData.shuffle / .array, decomp/utils/data.py:147-156);
 * index: int64 on the device. */
int dcp_gather_rows_f64(dcp_handle* h, const double* in, const int64_t* index, int64_t rows,
                         int64_t cols, double* out);
int dcp_dict_stats_c64(dcp_handle* h, const void* Y, void* X, const void* D, int64_t Nb, int64_t F,
                        int64_t K, double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                        void* stats, int* lasso_it);
int dcp_dict_update_c64(dcp_handle* h, const void* stats, double beta, void* A, void* B, const void* D,
                         void* D_new, int64_t F, int64_t K, float* maxdiff_dev);
int dcp_dict_step_c64(dcp_handle* h, const void* Y, void* X, const void* D, void* D_new, void* A, void* B,
                       int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                       int lasso_iter, double lasso_tol, double* maxdiff, int* lasso_it);
int dcp_dict_step_async_c64(dcp_handle* h, const void* Y, void* X, const void* D, void* D_new, void* A, void* B,
                             int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                             int lasso_iter, double lasso_tol, float* maxdiff_dev, int* lasso_it);
/* out[i, :] = in[index[i], :]  (MinibatchData.shuffle / .array, decomp/utils/data.py:147-156);
 * index: int64 on the device. */
int dcp_gather_rows_c64(dcp_handle* h, const void* in, const int64_t* index, int64_t rows,
                         int64_t cols, void* out);
int dcp_dict_stats_c128(dcp_handle* h, const void* Y, void* X, const void* D, int64_t Nb, int64_t F,
                        int64_t K, double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                        void* stats, int* lasso_it);
int dcp_dict_update_c128(dcp_handle* h, const void* stats, double beta, void* A, void* B, const void* D,
                         void* D_new, int64_t F, int64_t K, double* maxdiff_dev);
int dcp_dict_step_c128(dcp_handle* h, const void* Y, void* X, const void* D, void* D_new, void* A, void* B,
                       int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                       int lasso_iter, double lasso_tol, double* maxdiff, int* lasso_it);
int dcp_dict_step_async_c128(dcp_handle* h, const void* Y, void* X, const void* D, void* D_new, void* A, void* B,
                             int64_t Nb, int64_t F, int64_t K, double beta, double alpha, int lasso_method,
                             int lasso_iter, double lasso_tol, double* maxdiff_dev, int* lasso_it);
/* out[i, :] = in[index[i], :]  (MinibatchData.shuffle / .array, decomp/utils/data.py:147-156);
 * index: int64 on the device. */
int dcp_gather_rows_c128(dcp_handle* h, const void* in, const int64_t* index, int64_t rows,
                         int64_t cols, void* out);
/* One minibatch step of the MASKED variant, decomp/dictionary_learning.py:192-225
 * (solve_cd_mask): lasso with the 2-D mask, A3[K,F,K] <- beta A3 + x^H (x (x) m) (per-channel
 * Gram, :209-213), B <- beta B + x^H (y o m), the atom update against the OLD dictionary
 * (:218-223) and max|D - D_new| to the host.  A parity path (O(F K^2 Nb) statistic as in the
 * reference), single GPU. */
int dcp_dict_mask_step_f32(dcp_handle* h, const float* Y, const float* mask, float* X, const float* D,
                            float* D_new, float* A3, float* B, int64_t Nb, int64_t F, int64_t K, double beta,
                            double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                            double* maxdiff, int* lasso_it);
int dcp_dict_mask_step_f64(dcp_handle* h, const double* Y, const double* mask, double* X, const double* D,
                            double* D_new, double* A3, double* B, int64_t Nb, int64_t F, int64_t K, double beta,
                            double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                            double* maxdiff, int* lasso_it);
int dcp_dict_mask_step_c64(dcp_handle* h, const void* Y, const float* mask, void* X, const void* D,
                            void* D_new, void* A3, void* B, int64_t Nb, int64_t F, int64_t K, double beta,
                            double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                            double* maxdiff, int* lasso_it);
int dcp_dict_mask_step_c128(dcp_handle* h, const void* Y, const double* mask, void* X, const void* D,
                            void* D_new, void* A3, void* B, int64_t Nb, int64_t F, int64_t K, double beta,
                            double alpha, int lasso_method, int lasso_iter, double lasso_tol,
                            double* maxdiff, int* lasso_it);

/* ---- template matching (decomp/template_matching.py) ------------------------------------- */
/* 1-D convolutional templates D [T, S] over signals Y [B, N]; coefficients X [B, T, C] with
 * C = floor((S + 2 pad - N) / stride) + 1, pad = N - 1 (padding = 1, 'SAME') or N - S (padding = 0,
 * 'VALID'); 0 < S <= N.  Device pointers in the problem dtype (complex: interleaved pairs).  The
 * im2col operator A [T C, N] (A[(t, c), n] = D[t, n - stride c + Q], Q = stride (C - 1) - pad) is never
 * formed except by dcp_tm_temp2mat_*.  Enqueued on the handle's stream; lasso and dstep synchronise it.
 *   temp2mat:  out [T, C, N] = _temp2mat(D)           coef2mat: out [B, T, S, N] = _coef2mat(X)
 *   predict:   out [B, N] = X . A
 *   lasso:     solve_fastpath (lasso.py:97-189) of Y on A for method DCP_LASSO_ISTA / _ACC_ISTA / _FISTA
 *              (+ positive, real dtypes), X in: initial estimate, out: solution; *it_out as dcp_lasso_*.
 *   dstep:     the statistics XXt [T S, T S], yX [T S] of (Y, X) (template_matching.py:177-182),
 *              written (acc_it == 0) or added as stat / acc_it to XXt / yX (the running sums, :238-239),
 *              then D <- l2(D + (yX - XXt D) / (Gershgorin(XXt) + 1e-15)) in place; *maxdiff = max|dD|.
 *   gather_windows:  Yw [m, w] = Y[idx_b[j], idx_n[j] : + w], Xw [m, T, cw] = X[idx_b[j], :, idx_n[j] : + cw]
 *              (cw = coefficients of a w-sample window; the caller keeps idx_n[j] + cw <= C, idx_n[j] + w <= N)
 *   scatter_windows: X[idx_b[j], :, idx_n[j] : + cw] = Xw[j] in order j = 0 .. m - 1 (the last window wins).
 *   pursuit:   matching pursuit of every signal on A (decomp_amd/csrc/template_pursuit.hpp states the algorithm): at
 *              most n_steps (in [1, T C]) greedy steps, each taking the atom of the largest |alpha|^2 / rho2 (lowest
 *              flat index t C + c on ties; positive != 0, real dtypes: only atoms with alpha > 0) and adding
 *              alpha / rho2 to its coefficient; a signal stops once its residual energy is <= tol (tol < 0: no such
 *              stop) or no atom scores > 0.  D is used as given.  X [B, T, C] is written entirely (the caller does not
 *              zero it); *it_out = the largest number of steps a signal took.  Synchronises the stream.
 *   pursuit_lds_atoms: the largest T C for which pursuit keeps the correlations in LDS (above: global workspace).
 *   omp:       orthogonal matching pursuit of every signal on A (decomp_amd/csrc/template_omp.hpp states the
 *              algorithm): at most n_steps (in [1, min(T C, cap)], cap = 64 real, 32 complex) atoms per signal, each
 *              the atom outside the support with the largest |alpha|^2 / rho2 (lowest flat index on ties), followed by
 *              the least-squares re-fit of the signal on the support through a Cholesky factor of the support's Gram
 *              matrix, whose entries are read from the lag correlations of the templates.  A signal stops once its
 *              residual energy is <= tol (tol < 0: no such stop), no atom scores > 0, or the best atom is numerically
 *              dependent on the support.  X [B, T, C] is written entirely; *it_out = the largest support a signal
 *              reached.  Synchronises the stream.
 *   omp_lds_atoms: the largest T C for which omp keeps the correlations in LDS (above: global workspace). */
int dcp_tm_temp2mat_f32(dcp_handle* h, const void* D, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_temp2mat_f64(dcp_handle* h, const void* D, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_temp2mat_c64(dcp_handle* h, const void* D, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_temp2mat_c128(dcp_handle* h, const void* D, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_coef2mat_f32(dcp_handle* h, const void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_coef2mat_f64(dcp_handle* h, const void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_coef2mat_c64(dcp_handle* h, const void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_coef2mat_c128(dcp_handle* h, const void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_predict_f32(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_predict_f64(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_predict_c64(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_predict_c128(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_lasso_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_lasso_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_lasso_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_lasso_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_dstep_f32(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, double* maxdiff);
int dcp_tm_dstep_f64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, double* maxdiff);
int dcp_tm_dstep_c64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, double* maxdiff);
int dcp_tm_dstep_c128(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, double* maxdiff);
/* dcp_tm_dstep_* for sparse X (the codes of dcp_tm_pursuit_* / dcp_tm_omp_*): same outputs, same acc_it, same single
 * synchronisation, bit for bit the same result; the statistics are summed over per-row lists of the non-zeros of X.
 * max_events >= 1 bounds the list of a (signal, template) row; a row with more non-zeros is walked in full, so the
 * bound decides the speed, never the result.  X and Y must be finite.  With dcp_profile_* on, both steps time their
 * statistics kernels under DCP_PROF_STATS and, inside that, the partial sums the lists replace under DCP_PROF_MISC. */
int dcp_tm_dstep_events_f32(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_dstep_events_f64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_dstep_events_c64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_dstep_events_c128(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_gather_windows_f32(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_gather_windows_f64(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_gather_windows_c64(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_gather_windows_c128(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_scatter_windows_f32(dcp_handle* h, const void* Xw, void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding);
int dcp_tm_scatter_windows_f64(dcp_handle* h, const void* Xw, void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding);
int dcp_tm_scatter_windows_c64(dcp_handle* h, const void* Xw, void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding);
int dcp_tm_scatter_windows_c128(dcp_handle* h, const void* Xw, void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t S, int64_t N, int64_t w, int64_t stride, int padding);
int dcp_tm_pursuit_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_pursuit_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_pursuit_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_pursuit_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_pursuit_lds_atoms_f32(void);
int dcp_tm_pursuit_lds_atoms_f64(void);
int dcp_tm_pursuit_lds_atoms_c64(void);
int dcp_tm_pursuit_lds_atoms_c128(void);
int dcp_tm_omp_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_omp_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_omp_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_omp_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_omp_lds_atoms_f32(void);
int dcp_tm_omp_lds_atoms_f64(void);
int dcp_tm_omp_lds_atoms_c64(void);
int dcp_tm_omp_lds_atoms_c128(void);
/* Multichannel templates for the greedy coders: D [T, Ch, S], Y [B, Ch, N], one coefficient X [B, T, C] per event for
 * all Ch channels: y[b, ch, n] ~ sum_(t, c) x[b, t, c] D[t, ch, n - stride c + Q].  The geometry (C, Q), the steps, the
 * stop rules, the caps and the argument checks are those of dcp_tm_pursuit_* / dcp_tm_omp_* / dcp_tm_predict_*, with
 * every correlation, rho2 and |y|^2 (hence tol) summed over the channels; Ch < 1 gives DCP_ERR_INVALID.  Ch = 1 runs
 * these kernels too.
 * With dcp_profile_* on, the correlation pass alpha0 = y A^H of dcp_tm_pursuit_*, dcp_tm_omp_* and their mc forms is
 * timed under DCP_PROF_XUPDATE.
 *   mc_predict:           out [B, Ch, N].
 *   mc_template_block:    templates per thread of the correlation kernel.
 *   mc_channels_per_pass: channels of y that kernel stages in LDS per pass for templates of S taps at this stride
 *                         (0: one channel's window does not fit and the kernel reads global memory). */
int dcp_tm_mc_pursuit_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_mc_pursuit_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_mc_pursuit_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_mc_pursuit_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int positive, int* it_out);
int dcp_tm_mc_omp_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_mc_omp_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_mc_omp_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_mc_omp_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol /* < 0: none */, int* it_out);
int dcp_tm_mc_predict_f32(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_mc_predict_f64(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_mc_predict_c64(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_mc_predict_c128(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, void* out);
int dcp_tm_mc_template_block_f32(void);
int dcp_tm_mc_template_block_f64(void);
int dcp_tm_mc_template_block_c64(void);
int dcp_tm_mc_template_block_c128(void);
int dcp_tm_mc_channels_per_pass_f32(int64_t S, int64_t stride);
int dcp_tm_mc_channels_per_pass_f64(int64_t S, int64_t stride);
int dcp_tm_mc_channels_per_pass_c64(int64_t S, int64_t stride);
int dcp_tm_mc_channels_per_pass_c128(int64_t S, int64_t stride);
/* Learning multichannel templates: dcp_tm_dstep_events_* for D [T, Ch, S] (updated in place), Y [B, Ch, N],
 * X [B, T, C], yX [T Ch S]; XXt [T S, T S] is that of one channel, since X is shared by the channels.
 *   U[t, ch, k] = D[t, ch, k] + (yX[t, ch, k] - sum_(t', k') XXt[(t, k), (t', k')] D[t', ch, k']) / L,
 *   L = Gershgorin(XXt) + 1e-15,   D <- U / |U_t| with the norm over the Ch S entries of a template;
 * *maxdiff = max|dD| over all T Ch S entries.  acc_it, max_events, the single synchronisation, the argument checks and
 * the profile scopes are those of dcp_tm_dstep_events_*; Ch < 1 gives DCP_ERR_INVALID.  Channel by channel the sums
 * are the one-channel step's: with Ch = 1 the outputs are dcp_tm_dstep_events_*'s bit for bit.
 *   mc_gather_windows: Yw [m, Ch, w] = Y[idx_b[j], :, idx_n[j] : + w], Xw as dcp_tm_gather_windows_*; the codes go
 *              back with dcp_tm_scatter_windows_*. */
int dcp_tm_mc_dstep_events_f32(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_mc_dstep_events_f64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_mc_dstep_events_c64(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_mc_dstep_events_c128(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, int64_t max_events, double* maxdiff);
int dcp_tm_mc_gather_windows_f32(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_mc_gather_windows_f64(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_mc_gather_windows_c64(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
int dcp_tm_mc_gather_windows_c128(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t w, int64_t stride, int padding, void* Yw, void* Xw);
/* dcp_tm_lasso_* for multichannel templates: Y [B, Ch, N], D [T, Ch, S], X [B, T, C] (in: the initial estimate, out: the
 * solution), i.e. lasso.solve on the dense operator A [T C, Ch N], A[(t, c), (ch, n)] = D[t, ch, n - stride c + Q].
 * method, positive, the scaled variables, the stop test, it_out and the argument checks are those of dcp_tm_lasso_*; the
 * threshold is alpha Ch N / rho.  Proximal gradient in Gram form: one correlation pass over Y per call, then one kernel
 * per iteration on the lag correlations of the templates, whose cost does not depend on Ch.  The Gram entries of pairs
 * of atoms that both reach outside the signal are tabulated once per call (none with VALID padding); a table above
 * 1 GiB gives DCP_ERR_INVALID before anything is launched.  Ch = 1 runs these kernels too. */
int dcp_tm_mc_lasso_f32(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_mc_lasso_f64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_mc_lasso_c64(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);
int dcp_tm_mc_lasso_c128(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol, int maxiter, int method, int positive, int* it_out);

#ifdef __cplusplus
}
#endif
#endif /* DECOMP_HIP_H */
