/*
 * include/spp_hip.h -- C ABI of libspp_hip.so, the MI355X (gfx950) block-sparse Lambda solver
 * that drops in behind SLAM++'s duck-typed CLinearSolver_* concept.
 *
 * The reference has NO C ABI for this path: a linear solver is a C++ template concept
 * (reference: include/slam/LinearSolverTags.h:38,54,64-135; the native model is
 * include/slam/LinearSolver_UberBlock.h:44-427, the Schur wrapper include/slam/LinearSolver_Schur.h:1423-2392).
 * include/spp_adapter.h implements that concept on top of these entry points; INTEGRATION.md
 * shows how the reference is recompiled against it without source edits.
 *
 * Conventions
 *   - every function returns SPP_OK (0), SPP_NOT_POSDEF (1: the adapter maps it to `return false`,
 *     reference: BlockMatrix.cpp:9765-9771 / NonlinearSolver_Lambda.h:628-664), or a negative
 *     SPP_E_* code (the adapter throws std::runtime_error / std::bad_alloc, reference:
 *     LinearSolver_Schur_GPU.cpp:734-797); spp_last_error() returns the message.
 *   - plain pointers and sizes only; int64 block indices / offsets, int32 block dims, fp64 values.
 *   - pointers named h_* are host memory, d_* are device (HBM) memory of the ctx's device.
 *   - one ctx = one device + one stream, used from one thread (reference threading contract:
 *     LinearSolver_Schur.h:1187 binds one context per solver instance).
 *   - there is NO CPU fallback: every compute entry point fails with SPP_E_NO_DEVICE if HIP
 *     cannot run on the selected device.
 *
 * Matrix layout (the flattening of CUberBlockMatrix, reference BlockMatrixBase.h:380-503):
 *   upper-triangular block-CSC; nb block columns; dim[nb] widths; col_ptr[nb+1]; row_idx[nnzb]
 *   ascending per column with the diagonal block last; blk_off[nnzb] = offset in doubles of block
 *   p inside `vals`; a block is dim[row] x dim[col], column-major (the element order
 *   t_Block_AtColumn(...).data() yields, BlockMatrix.h:343-485).
 */
#ifndef SPP_HIP_H
#define SPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPP_OK            0
#define SPP_NOT_POSDEF    1
#define SPP_E_BADARG     -1
#define SPP_E_NOMEM      -2
#define SPP_E_HIP        -3
#define SPP_E_NO_DEVICE  -4
#define SPP_E_STATE      -5   /* call order violated (e.g. solve before analyze) */
#define SPP_E_UNSUPPORTED -6

/* spp_analyze modes */
#define SPP_MODE_AUTO     0   /* Schur if two block widths with a block-diagonal landmark part, else sparse */
#define SPP_MODE_SPARSE   1   /* ordering + supernodal block Cholesky on the whole Lambda */
#define SPP_MODE_SCHUR    2   /* guided Schur complement (landmarks = smaller width) + dense reduced solve; block widths
                                   {6,3} (SE(3) cameras / poses + points), {3,2} (2D poses + landmarks), {7,3} (Sim(3)
                                   cameras + points); anything else SPP_E_UNSUPPORTED */
#define SPP_MODE_SCHUR_SPARSE 3 /* guided Schur complement, the reduced camera system kept sparse (block-CSC) and
                                   solved by the supernodal path: CLinearSolver_Schur with a sparse inner solver,
                                   include/slam/LinearSolver_Schur.h:1844-1853. AUTO picks it beyond 16384 reduced
                                   scalars (BASELINE config 5: 10k cameras). Shards over landmarks like SPP_MODE_SCHUR: every
                                   rank holds the union block structure of S, the all-reduced buffer is the block value
                                   array followed by the reduced rhs */

/* spp_create flags */
#define SPP_FLAG_PROFILE  1   /* record hipEvents around the phases of each solve */
#define SPP_FLAG_SCHUR_PARTIAL 2 /* multi-GPU: spp_schur_form() leaves the partial S / rhs for an external all-reduce */

typedef struct spp_ctx spp_ctx;

/* ---- lifetime ---------------------------------------------------------------------------------
 * replaces: CLinearSolver_UberBlock ctor / dtor / Free_Memory (LinearSolver_UberBlock.h:69-121) */
spp_ctx *spp_create(int device, int flags);
void spp_destroy(spp_ctx *ctx);
/* drops factor/workspaces but keeps the ctx usable (Free_Memory, LinearSolver_UberBlock.h:88-121) */
int spp_free_memory(spp_ctx *ctx);
int spp_last_error(const spp_ctx *ctx, char *buf, size_t buf_size);
/* Page-locked host buffer of at least n_doubles doubles, owned by the ctx (grows, freed by spp_destroy), or NULL
 * when it cannot be had. The adapter flattens Lambda's blocks straight into it (the role of the m_vals vector) so
 * that the host-pointer entry spp_factor_solve() copies to the device at the DMA rate of the link instead of through
 * the runtime's pageable bounce buffers: the reference's own workspace reuse, LinearSolver_UberBlock.h:332-348. */
double *spp_host_staging(spp_ctx *ctx, int64_t n_doubles);
/* run all work of this ctx on an externally owned hipStream_t (e.g. torch's current stream). Drains the old stream and
 * the ctx's side stream first. The results of spp_factor_solve_device and spp_schur_finish are ordered on this stream
 * (see there): work the caller enqueues on it sees them complete; work on any OTHER stream needs spp_synchronize or an
 * event of the caller's behind the call. */
int spp_set_stream(spp_ctx *ctx, void *hip_stream);
/* waits for everything enqueued on the ctx stream; reports (SPP_E_HIP) a backward substitution that timed out in a solve
 * which had returned before it ended */
int spp_synchronize(spp_ctx *ctx);

/* ---- symbolic -----------------------------------------------------------------------------------
 * replaces: SymbolicDecomposition_Blocky (LinearSolver_UberBlock.h:272-296: block AMD ordering via
 * OrderingMagic.cpp:701; LinearSolver_Schur.h:1566-1606: guided ordering) plus the structure-only
 * work the reference redoes inside every Solve_PosDef_Blocky: Permute_UpperTriangular_To
 * (BlockMatrix.cpp:8183), Build_EliminationTree (:9403), ereach (:9453), SliceTo/TransposeTo
 * (LinearSolver_Schur.h:1699-1709). Call again whenever the block structure changes
 * (Clear_SymbolicDecomposition, LinearSolver_UberBlock.h:260-264). */
int spp_analyze(spp_ctx *ctx, int64_t nb, const int64_t *h_col_ptr, const int64_t *h_row_idx,
	const int64_t *h_blk_off, const int32_t *h_dim, int mode);

/* multi-GPU landmark sharding: this rank keeps only landmarks p with
 * shard_of_landmark == rank; cameras and A are replicated. Call before spp_analyze. */
int spp_set_shard(spp_ctx *ctx, int rank, int world_size);

/* facts about the analyzed system; unknown keys give SPP_E_BADARG */
#define SPP_MODE_SCHUR_MIS 4  /* Schur complement over a maximal independent set of a ONE-width graph (3 or 6: pose
                                 graphs): the general ordering of CSchurOrdering (src/slam/LinearSolver_Schur.cpp:690-769,
                                 1235-1340); reduced system sparse, supernodal solve. Never chosen by AUTO */

#define SPP_INFO_MODE           0  /* SPP_MODE_SPARSE, SPP_MODE_SCHUR or SPP_MODE_SCHUR_SPARSE actually chosen */
#define SPP_INFO_N              1  /* scalar dimension */
#define SPP_INFO_NNZB           2  /* stored blocks of Lambda (upper incl. diagonal) */
#define SPP_INFO_NVALS          3  /* doubles in vals */
#define SPP_INFO_FACTOR_NNZ     4  /* scalar nonzeros of the factor (sparse) or n_reduced^2 storage (Schur dense) */
#define SPP_INFO_FACTOR_FLOPS   5  /* flops of the numeric factorization */
#define SPP_INFO_N_REDUCED      6  /* Schur: dimension of the reduced camera system */
#define SPP_INFO_N_POSES        7
#define SPP_INFO_N_LANDMARKS    8  /* landmarks owned by this shard */
#define SPP_INFO_SCHUR_PAIRS    9  /* sum_p k_p (k_p+1)/2 block products of the S accumulation */
#define SPP_INFO_N_OBS          10 /* pose-landmark blocks owned by this shard */
#define SPP_INFO_SOLVE_BYTES    11 /* algorithmic HBM bytes of one numeric solve */
#define SPP_INFO_N_SUPERNODES   12
#define SPP_INFO_N_LEVELS       13
#define SPP_INFO_S_LD           14 /* leading dimension of the dense S buffer (padded); 0 when S is sparse */
#define SPP_INFO_S_NNZB         15 /* Schur: stored blocks of the reduced camera system (upper incl. diagonal) */
#define SPP_INFO_DENSE_STREAMED 16 /* tile rows (of 128) the last dense factorization handed to the streamed launch (spp_dense_tail.h); 0: none */
#define SPP_INFO_LM_STREAM      17 /* landmark-side Schur kernels the last spp_schur_form / solve launched: 0 one lane per block, 1 / 2 the streamed forms (SPP_LM_STREAM) */
#define SPP_INFO_BS_GROUPS      18 /* Schur: landmark groups of the fused back-substitution; 0: a landmark has more than 256 observations, two launches */
#define SPP_INFO_SCHUR_SIDE     19 /* the last spp_schur_form / solve ran the reduced right-hand side on the side stream (SPP_SCHUR_SIDE): 1, else 0 */
#define SPP_INFO_S_CLEAR        20 /* what the last spp_schur_form / solve cleared of its S buffer: 0 all of it, 1 the tiles of the filled mask, 2 the right-hand side and padding columns (every block of S is written) */
#define SPP_INFO_S_DEVICE_PTR   21 /* diagnostics, tests: device address of the S | rhs buffer spp_factor_solve owns (0: none yet) */
#define SPP_INFO_ASM_HUB_CHUNK   22 /* assembly of ternary edges: edges one workgroup of the hub reduction sums (C); a constant, needs no analysis */
#define SPP_INFO_SOLVE_ASYNC    23 /* what the last spp_factor_solve_device / spp_schur_finish did (SPP_SOLVE_ASYNC): 1 it returned when the factor's status was known, the solves and the back-substitution still running on the stream; 0 it drained the stream (profiling on, stream capture, sparse reduced system, sparse mode, the switch at 0) */
#define SPP_INFO_FACTOR_KEPT    24 /* 1: the ctx holds a factor spp_solve_device / spp_marginals_device may use: the last spp_factor_solve_device returned SPP_OK in SPP_MODE_SCHUR with a dense reduced system, unsharded, and nothing has rewritten it since; 0 otherwise (needs no analysis) */
#define SPP_INFO_SPARSE_FACTOR_KEPT 25 /* 1: the ctx holds a sparse factor spp_sparse_solve_device / spp_sparse_marginals_device may use: the last spp_factor_solve_device returned SPP_OK in SPP_MODE_SPARSE, unsharded, and no call that drops it has been entered since; 0 otherwise (needs no analysis). SPP_INFO_FACTOR_KEPT stays 0 in the sparse mode */
#define SPP_INFO_SCHUR_SPARSE_FACTOR_KEPT 26 /* 1: the ctx holds a factor spp_schur_sparse_solve_device / spp_schur_sparse_marginals_device / spp_schur_sparse_sigma_device may use: the last spp_factor_solve_device returned SPP_OK in SPP_MODE_SCHUR_SPARSE, unsharded, and no call that drops it has been entered since; 0 otherwise (needs no analysis). The two words above stay 0 in this mode */
int spp_get_info(const spp_ctx *ctx, int what, int64_t *out);
/* elimination order chosen by the analysis: order[k] = source block column eliminated k-th */
int spp_get_ordering(const spp_ctx *ctx, int64_t *h_order);
/* The front table of the sparse plan (diagnostics and tests; host copies only, nothing is launched). Returns the number
 * of fronts (supernodes), 0 when the analysis built no sparse plan, and fills the first min(capacity, fronts) entries of
 * every array that is not NULL, fronts in elimination (post-) order:
 *   h, w     scalar height (right-hand-side slot included: a root has h = w + 1) and pivot width
 *   pad      identity padding behind the pivot block in the front's HBM image (class 3: to 16, class 4: to 128, else 0)
 *   cls      size class 0..4: LDS image of 32 / 64 / 128 rows, one workgroup in place in HBM, 128-padded big front
 *   level    level in the assembly tree (leaves 0);  parent: front index, -1 for a root
 *   team     workgroups of a big front inside the dependency-driven launch (1: none, or the front is host-driven) */
int64_t spp_sparse_fronts(const spp_ctx *ctx, int64_t capacity, int32_t *h, int32_t *w, int32_t *pad, int32_t *cls, int32_t *level,
	int32_t *parent, int32_t *team);

/* Fill-reducing block ordering of an upper block pattern, host only (no context, no GPU): the job of
 * CMatrixOrdering::p_BlockOrdering (reference src/slam/OrderingMagic.cpp:701, live path :900-1031:
 * A + A^T block pattern -> AMD). order[k] = block column eliminated k-th (the reference returns the
 * inverse of this). SPP_ORDER_AMD: approximate minimum degree (quotient graph); SPP_ORDER_ND: nested
 * dissection on BFS level structures with minimum-degree leaves (logarithmic tree height on
 * chain-like graphs). The analysis picks between the two itself (ordering). */
#define SPP_ORDER_AMD 0
#define SPP_ORDER_ND  1
int spp_block_ordering(int64_t nb, const int64_t *col_ptr, const int64_t *row_idx, int method, int64_t *h_order);

/* The symbolic Schur plan of an upper block pattern, host only (no context, no GPU): what the reference recomputes
 * structurally in every CLinearSolver_Schur::Solve_PosDef_Blocky call (guided ordering LinearSolver_Schur.cpp:771-838,
 * the slices LinearSolver_Schur.h:1699-1709, the symbolic part of MultiplyToWith BlockMatrixFBS.inl:1147-1304) as
 * observation lists, the block pattern of S and its per-block lists of block products. Runs on up to 16 host threads
 * (SPP_PLAN_THREADS); the result does not depend on their number. out holds NINE values: out[0..6] = poses, landmarks
 * of this shard, observations, block products, blocks of S, work items, split blocks; out[7] = a 64-bit checksum of the
 * pair lists, the block list of S, the item records and the XCD ranges; out[8] = a 64-bit checksum of every list and
 * scalar of the plan that the device plan uploads or keeps (out[7] and the scalars mixed in). *seconds = wall clock of
 * the plan. sparse_S: bit 0 = sparse reduced system, bit 1 = the MIS cut of SPP_MODE_SCHUR_MIS (one block
 * width; its reduced system is always sparse). For tests and for timing the analysis phase without a device. */
int spp_schur_plan_host(int64_t nb, const int32_t *dim, const int64_t *col_ptr, const int64_t *row_idx, int shard_rank,
	int shard_world, int sparse_S, int64_t *out, double *seconds);

/* ---- numeric: host-pointer entry points (what the header adapter calls) ----------------------------
 * replaces: Solve_PosDef_Blocky (LinearSolver_UberBlock.h:312-426; LinearSolver_Schur.h:1623-1935)
 * and Solve_PosDef (LinearSolver_UberBlock.h:143-258). h_vals holds the blocks at the blk_off
 * given to spp_analyze; h_rhs (length n) is overwritten with the solution. */
int spp_factor_solve(spp_ctx *ctx, const double *h_vals, double *h_rhs_inout);

/* ---- numeric: device-resident entry points (Lambda lives in HBM across GN iterations) ------------
 * d_vals: nvals doubles in the layout given to spp_analyze; d_rhs: n doubles, in/out (contents unspecified after
 * SPP_NOT_POSDEF: the status is fetched once, after the solves have run).
 * STREAM-ORDERED RESULT: with a dense reduced camera system (SPP_MODE_SCHUR; SPP_INFO_SOLVE_ASYNC tells) the call returns
 * as soon as the factorization's status is known -- the return code is final -- while the triangular solves and the
 * back-substitution may still be running on the ctx stream. d_rhs_inout is complete for any later work on the ctx
 * stream (the next solve, spp_memcpy_d2d, the update kernels), for spp_memcpy_d2h and behind spp_synchronize; d_vals and
 * d_rhs_inout must stay allocated until then (spp_device_free waits for the stream). Not so -- the call drains the stream
 * as before -- with profiling on, under stream capture, for the sparse reduced system and the sparse mode, and with
 * SPP_SOLVE_ASYNC=0. */
int spp_factor_solve_device(spp_ctx *ctx, const double *d_vals, double *d_rhs_inout);

/* ---- solve again on the kept factor -----------------------------------------
 * Lambda X = B for nrhs further right-hand sides against the factor the last successful spp_factor_solve_device of this
 * ctx left behind (SPP_INFO_FACTOR_KEPT): no S accumulation, no factorization. d_B: n x nrhs, column-major, leading
 * dimension ldb >= n, rows in Lambda's numbering, overwritten by X; nothing outside its n rows and nrhs columns is touched.
 * CONTRACT: d_vals must hold the values that call factored, unchanged -- the landmark side reads U and C from them, and the
 * library cannot tell whether they are the same. Column j of the result has the same bits whatever the other columns hold
 * and wherever it stands; two runs give the same bits.
 * STREAM-ORDERED: the call enqueues on the ctx stream and returns; d_B is complete for later work on that stream, for
 * spp_memcpy_d2h and behind spp_synchronize -- also behind a solve that returned early (SPP_SOLVE_ASYNC). d_vals and d_B
 * must stay allocated until then.
 * The factor is kept by SPP_OK of spp_factor_solve_device in SPP_MODE_SCHUR (dense reduced system, unsharded) and dropped
 * on entry of every call that rewrites S, the dense workspaces or the plan: any factor / solve, spp_schur_form /
 * spp_schur_finish (whatever their buffer: the block inverses are the ctx's), spp_dense_*, spp_analyze and the
 * spp_assemble_analyze* calls, spp_set_shard, spp_free_memory. The two calls below keep it.
 * SPP_E_STATE: no kept factor. SPP_E_UNSUPPORTED: a sparse reduced system (SPP_MODE_SCHUR_SPARSE, SPP_MODE_SCHUR_MIS), the
 * sparse mode, a sharded ctx. SPP_E_BADARG: a null pointer, nrhs < 1, ldb < n. */
int spp_solve_device(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs);
/* Joint covariance of chosen vertices: d_cov (m x m, column-major, m = sum of their widths) <- E^T Lambda^-1 E, E the unit
 * block columns of the n_sel vertices h_vertices (block columns of Lambda: cameras and landmarks in any mix and order, each
 * at most once) -- one solve with m columns on the kept factor, as the reference's Schur_Marginals solves against the
 * factor of S block column by block column (include/slam/BAMarginals.h). Rows and columns follow h_vertices. The upper
 * triangle is computed and mirrored: exactly symmetric. Workspace: n x m doubles. Contract, ordering and errors as above;
 * SPP_E_BADARG also for n_sel < 1, a vertex out of range or listed twice. Which damping Lambda carries is the caller's
 * choice (a bundle adjustment without a scale prior has a gauge direction only damping makes definite). */
int spp_marginals_device(spp_ctx *ctx, const double *d_vals, int64_t n_sel, const int64_t *h_vertices, double *d_cov);

/* ---- solve again on the kept SPARSE factor: pose graphs ------------------------
 * Lambda X = B for nrhs further right-hand sides against the multifrontal factor the last successful
 * spp_factor_solve_device / spp_factor_solve of this ctx left in the fronts of its sparse plan
 * (SPP_INFO_SPARSE_FACTOR_KEPT): a forward and a backward multifrontal substitution, no factorization. d_B: n x nrhs,
 * column-major, leading dimension ldb >= n, rows in Lambda's numbering, overwritten by X; nothing outside its n rows and
 * nrhs columns is written. There is no d_vals: the fronts hold all of R, so nothing is asked of Lambda's values.
 * Column j of the result has the same bits whatever the other columns hold, wherever it stands and however many columns
 * the call carries; two runs give the same bits. (They are not the bits of spp_factor_solve_device on that column: its
 * forward substitution rides inside the factorization and sums in another order.)
 * STREAM-ORDERED: the call enqueues on the ctx stream and returns; d_B is complete for later work on that stream, for
 * spp_memcpy_d2h and behind spp_synchronize. d_B must stay allocated until then.
 * The factor is kept by SPP_OK of spp_factor_solve_device / spp_factor_solve when the ctx's mode is SPP_MODE_SPARSE (also
 * SPP_MODE_AUTO resolving to it, and the repeated enqueue after a timed-out dependency-driven launch), unsharded. It is
 * dropped on entry of every call that drops the dense Schur factor above: any factor / solve, spp_schur_form /
 * spp_schur_finish, spp_dense_*, spp_analyze and the spp_assemble_analyze* calls, spp_set_shard, spp_free_memory. The two
 * calls below keep it, and so do spp_solve_device / spp_marginals_device (which answer SPP_E_UNSUPPORTED in this mode).
 * Refusals, each checked before anything is touched (the ctx stays usable):
 * SPP_E_STATE: no kept factor -- never solved, the last solve returned SPP_NOT_POSDEF, or a later call dropped it.
 * SPP_E_UNSUPPORTED: SPP_MODE_SCHUR, SPP_MODE_SCHUR_SPARSE, SPP_MODE_SCHUR_MIS, a sharded ctx.
 * SPP_E_BADARG: a null pointer, nrhs < 1, ldb < n. */
int spp_sparse_solve_device(spp_ctx *ctx, double *d_B, int64_t ldb, int64_t nrhs);
/* Joint covariance of chosen vertices of a pose graph, the job of the reference's CMarginals (include/slam/Marginals.h):
 * d_cov (m x m, column-major, m = sum of their widths) <- E^T Lambda^-1 E, E the unit block columns of the n_sel vertices
 * h_vertices (block columns of Lambda of any widths, in any order, each at most once). Rows and columns follow h_vertices.
 * One m-column spp_sparse_solve_device of unit columns built on the device; the upper triangle is computed and mirrored:
 * exactly symmetric. Workspace: n x m doubles in the ctx. Ordering, keeping and refusals as above; SPP_E_BADARG also for
 * n_sel < 1, a vertex out of range or listed twice. NOT FOR STREAM CAPTURE: the call waits for the ctx stream once on entry
 * (the list of rows is staged in host memory of the ctx) and may reallocate its n x m workspace when m grows. */
int spp_sparse_marginals_device(spp_ctx *ctx, int64_t n_sel, const int64_t *h_vertices, double *d_cov);
/* Blocks of Sigma = Lambda^-1 on the stored pattern of Lambda, from the kept sparse factor
 * (SPP_INFO_SPARSE_FACTOR_KEPT), the job of the reference's CMarginals::Calculate_DenseMarginals_Recurrent_FBS.
 * d_sigma: SPP_INFO_NVALS doubles in the layout of vals: the block of Sigma at (i, j) stands where Lambda's stored
 * block (i, j) stands (upper incl. diagonal, each block column-major). Diagonal blocks exactly symmetric.
 * Selected inversion down the assembly tree on the kept fronts: work of the order of the factorization's, no solve per
 * column. It takes no d_vals (the fronts hold all of R), keeps the factor and writes nothing into it.
 * STREAM-ORDERED on the ctx stream; no host synchronisation after the first call, which allocates the workspace (as many
 * doubles as the fronts hold; spp_free_memory frees it). Keeping and refusals as for spp_sparse_solve_device, each checked
 * before anything is touched: SPP_E_STATE without a kept factor, SPP_E_UNSUPPORTED in the three Schur modes and on a
 * sharded ctx, SPP_E_BADARG for a null pointer. */
int spp_sparse_sigma_device(spp_ctx *ctx, double *d_sigma);

/* ---- covariance blocks on Lambda's pattern from the kept DENSE SCHUR factor: bundle adjustment ----
 * Blocks of Sigma = Lambda^-1 on the stored pattern of Lambda from the factor spp_factor_solve_device left in
 * SPP_MODE_SCHUR (SPP_INFO_FACTOR_KEPT): a covariance per camera and per point and the cross block of every observation,
 * the job of the reference's CSchurComplement_Marginals::Schur_Marginals (include/slam/BAMarginals.h:563-583, "block
 * diagonal of the covariance matrix from a Schur-complemented system").
 * d_sigma: SPP_INFO_NVALS doubles in the layout of vals: the block of Sigma at (i, j) stands where Lambda's stored block
 * (i, j) stands (each block column-major; an observation block stored landmark row first holds Sigma[l, c]). Diagonal
 * blocks are exactly symmetric. Every double of d_sigma is written exactly once.
 * Z = S^-1 is formed whole from R and the block inverses (three launches per 128-row block row, about two thirds of a
 * factorization's flops per n^3), then Sigma[c, l] = -(sum_j Z[c, c_j] U_j) C_l^-1 and
 * Sigma[l, l] = C_l^-1 - C_l^-1 sum_i U_i^T Sigma[c_i, l] per landmark; no solve per column.
 * d_vals: the contract of spp_solve_device (the values the factor was made from: U and C are read from them).
 * STREAM-ORDERED on the ctx stream; no host synchronisation after the first call, which allocates the workspace (ld x ld
 * doubles for Z; spp_free_memory frees it) and lists the camera-camera blocks. It keeps the factor and writes nothing into
 * S or the block inverses. Refusals, each checked by the test of spp_solve_device before anything is touched (the ctx
 * stays usable): SPP_E_STATE without a kept factor; SPP_E_UNSUPPORTED in the sparse mode, SPP_MODE_SCHUR_SPARSE,
 * SPP_MODE_SCHUR_MIS, on a sharded ctx and for cameras of more than one width; SPP_E_BADARG for a null pointer.
 * (spp_sparse_sigma_device keeps answering SPP_E_UNSUPPORTED in the Schur modes.) */
int spp_schur_sigma_device(spp_ctx *ctx, const double *d_vals, double *d_sigma);

/* ---- the same three jobs on the kept factor of a SPARSE reduced system: SPP_MODE_SCHUR_SPARSE ----
 * The mode SPP_MODE_AUTO picks beyond 16384 reduced rows, and long landmark-SLAM trajectories analyzed in it. After SPP_OK
 * of spp_factor_solve_device R (S = R^T R) sits in the fronts of the sparse plan made from S's pattern
 * (SPP_INFO_SCHUR_SPARSE_FACTOR_KEPT); Lambda's values are the caller's. The six calls above keep answering
 * SPP_E_UNSUPPORTED in this mode, and keep this factor.
 * spp_schur_sparse_solve_device: Lambda X = B for nrhs further right-hand sides, the steps of spp_solve_device with the
 * camera panel solved by the multifrontal substitutions of spp_sparse_solve_device. d_B: n x nrhs, column-major, leading
 * dimension ldb >= n, rows in Lambda's numbering, overwritten by X; nothing outside its n rows and nrhs columns is
 * written. CONTRACT: d_vals must hold the values that were factored, unchanged (U and C are read from them). Column j of
 * the result has the same bits whatever the other columns hold, wherever it stands and however many columns the call
 * carries; two runs give the same bits.
 * STREAM-ORDERED on the ctx stream; no host synchronisation after the first call, which allocates the panels. d_vals and
 * d_B must stay allocated until the stream has passed the call.
 * The factor is kept by SPP_OK of spp_factor_solve_device / spp_factor_solve in SPP_MODE_SCHUR_SPARSE (also SPP_MODE_AUTO
 * resolving to it), unsharded, and dropped on entry of every call that drops the two factors above: any factor / solve,
 * spp_schur_form / spp_schur_finish, spp_dense_*, spp_analyze and the spp_assemble_analyze* calls, spp_set_shard,
 * spp_free_memory. The three calls here keep it.
 * Refusals, each checked before anything is touched (the ctx stays usable):
 * SPP_E_STATE: no kept factor -- never solved, the last solve returned SPP_NOT_POSDEF, or a later call dropped it.
 * SPP_E_UNSUPPORTED: SPP_MODE_SPARSE, SPP_MODE_SCHUR with a dense reduced system, SPP_MODE_SCHUR_MIS, a sharded ctx, block
 * widths other than {6,3}, {3,2}, {7,3}.
 * SPP_E_BADARG: a null pointer, nrhs < 1, ldb < n. */
int spp_schur_sparse_solve_device(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs);
/* Joint covariance of chosen vertices, worded as spp_marginals_device: d_cov (m x m, column-major, m = sum of their widths)
 * <- E^T Lambda^-1 E of the n_sel vertices h_vertices (cameras and landmarks in any mix and order, each at most once); one
 * m-column spp_schur_sparse_solve_device of unit columns built on the device, the upper triangle computed and mirrored:
 * exactly symmetric. Workspace: n x m doubles. Keeping and refusals as above; SPP_E_BADARG also for n_sel < 1, a vertex out
 * of range or listed twice. NOT FOR STREAM CAPTURE: the call waits for the ctx stream once on entry. */
int spp_schur_sparse_marginals_device(spp_ctx *ctx, const double *d_vals, int64_t n_sel, const int64_t *h_vertices, double *d_cov);
/* Blocks of Sigma = Lambda^-1 on the stored pattern of Lambda, worded as spp_schur_sigma_device. d_sigma: SPP_INFO_NVALS
 * doubles in the layout of vals; every double is written exactly once; diagonal blocks are exactly symmetric; an observation
 * block stored landmark row first holds Sigma[l, c].
 * The blocks of Z = S^-1 on the stored pattern of S come from the selected inversion of spp_sparse_sigma_device on the
 * kept fronts -- that pattern holds a block for every two cameras that share a landmark, which is every block the landmark
 * formulas of spp_schur_sigma_device read -- then Sigma[c, l] = -(sum_j Z[c, c_j] U_j) C_l^-1 and Sigma[l, l] as there; the
 * camera blocks are copies of Z's. No solve per column, no dense n_red x n_red array.
 * STREAM-ORDERED on the ctx stream; no host synchronisation after the first call, which allocates the workspaces (as many
 * doubles as the fronts hold, and as many as S's value array; spp_free_memory frees them). It keeps the factor and writes
 * nothing into S's buffer, the fronts or the plan. Keeping and refusals as for spp_schur_sparse_solve_device;
 * SPP_E_BADARG for a null pointer. */
int spp_schur_sparse_sigma_device(spp_ctx *ctx, const double *d_vals, double *d_sigma);

/* split form for multi-GPU: (1) each rank forms its partial Schur complement and
 * reduced rhs into d_S_rhs = [S (ld x ld, column-major, upper blocks) | rhs (ld)] ; (2) the caller
 * all-reduces that buffer (RCCL); (3) every rank factors S, solves and back-substitutes its own
 * landmarks. With world_size == 1 step (2) is a no-op. rank 0 alone adds A and the pose rhs. */
int spp_schur_buffer_size(const spp_ctx *ctx, int64_t *n_doubles);
int spp_schur_form(spp_ctx *ctx, const double *d_vals, const double *d_rhs, double *d_S_rhs);
/* spp_schur_finish returns like spp_factor_solve_device: with a dense S, once the status is known, d_rhs_inout ordered
 * on the ctx stream (d_S_rhs is still being read until then). */
int spp_schur_finish(spp_ctx *ctx, const double *d_vals, double *d_S_rhs, double *d_rhs_inout);
/* Only the upper block-trapezoid of S carries data: pack it (128-column panels, rows 0 .. end of the
 * panel's diagonal block; 128^2 nblk (nblk + 1) / 2 doubles, about half of the square buffer) before
 * the all-reduce and unpack afterwards -- halves the bytes that cross xGMI. */
int spp_schur_packed_size(const spp_ctx *ctx, int64_t *n_doubles);
int spp_schur_pack(spp_ctx *ctx, const double *d_S_rhs, double *d_packed);
int spp_schur_unpack(spp_ctx *ctx, const double *d_packed, double *d_S_rhs);

/* ---- Lambda / eta assembly ------------------------------------------------------------------------
 * replaces: CLambdaOps2::AddEntriesInSparseSystem + Alloc_HessianBlocks_v2 (symbolic;
 * NonlinearSolver_Lambda_Base.h:1852-1931, BaseTypes_Binary.h:525-660) and Refresh_Lambda =
 * Calculate_Hessians_v2 over all edges + ReduceAll (numeric; _Lambda_Base.h:1658-1688,
 * BaseTypes_Binary.h:759-848, _Lambda_Base.h:563-607,152-197).
 * One homogeneous binary-edge group (several: spp_assemble_analyze_groups below): residual dimension rd, vertex 0 width d0, vertex 1 width d1.
 * J0: ne x (rd x d0) col-major, J1: ne x (rd x d1), Omega: ne x (rd x rd), r: ne x rd.
 * Instantiated shapes (d0, d1, rd): (6,3,2) projections, (3,3,3) 2D odometry, (6,6,6) 3D odometry, (3,2,2) 2D landmark
 * observations, (6,3,3) 3D landmark (XYZ) observations, (6,3,1) ranges from a position-velocity vertex to a landmark
 * (CEdgePosVel_Landmark3D, include/slam/ROCV_Types.h:77-223: J0 ne x (1x6), J1 ne x (1x3), Omega ne x 1, r ne x 1), (7,3,2)
 * projections into Sim(3) cameras (CEdgeP2C_XYZ_Sim3_G, include/slam/Sim3_Types.h:492-595: J0 ne x (2x7) belongs to the
 * camera, J1 ne x (2x3) to the point -- the library's order is camera first, as for (6,3,2); the reference's typelist is
 * (XYZ, CamSim3)); any other is SPP_E_UNSUPPORTED. (7,3,2) is the ONLY group of its plan: through this entry point, or as the
 * one group of spp_assemble_analyze_groups (bit-equal); beside any other group, unary ones included, SPP_E_UNSUPPORTED.
 * The unary factor (identity, FlatSystem.h:441,467) is added to the diagonal block of vertex
 * `unary_vertex` (pass -1 for none). The reference's default build puts it on vertex 0 whatever its type
 * (__AUTO_UNARY_FACTOR_ON_VERTEX_ZERO, FlatSystem.h:331-337, _Lambda_Base.h:1903-1924; without that macro: on the
 * first vertex of the first edge). `damping` is added to every diagonal entry of Lambda
 * (Levenberg-Marquardt, NonlinearSolver_Lambda_LM.h:228-239; 0 for Gauss-Newton). */
int spp_assemble_analyze(spp_ctx *ctx, int64_t nv, const int32_t *h_dim,
	int64_t ne, const int64_t *h_v0, const int64_t *h_v1, int d0, int d1, int rd,
	int64_t unary_vertex);
/* structure produced by spp_assemble_analyze (sizes via spp_get_info NNZB / NVALS) */
int spp_assemble_get_structure(const spp_ctx *ctx, int64_t *h_col_ptr, int64_t *h_row_idx,
	int64_t *h_blk_off);
int spp_assemble_device(spp_ctx *ctx, const double *d_J0, const double *d_J1,
	const double *d_Omega, const double *d_r, double damping, double *d_vals_out, double *d_eta_out);
/* Robust edges (the reference's b_is_robust_edge branch of Calculate_Hessians_v2, include/slam/BaseTypes_Binary.h:768-848;
 * kernels and mix-ins include/slam/RobustUtils.h): d_w holds ONE weight per edge -- the value of the edge's
 * f_RobustWeight(r), evaluated by the caller -- and every following spp_assemble_device applies it exactly where the
 * reference does: H01 and H00 carry w once (T = J0^T Omega w), the first vertex's right-hand side w TWICE (T r w),
 * H11 and the second vertex's right-hand side once. The array is NOT copied (it must stay valid); NULL restores plain
 * edges; spp_assemble_analyze resets it. On a (7,3,2) plan a non-NULL array is SPP_E_UNSUPPORTED (and so from
 * spp_assemble_set_group_edge_weights): the "first vertex twice" rule would attach to the landmark there. */
int spp_assemble_set_edge_weights(spp_ctx *ctx, const double *d_w);
/* Several edge groups in one Lambda: odometry (3,3,3) beside landmark observations (3,2,2), camera-camera constraints
 * (6,6,6) beside projections (6,3,2) -- the reference's AddEntriesInSparseSystem / Refresh_Lambda run over an edge pool of
 * several types alike (NonlinearSolver_Lambda_Base.h:1852-1931, 1658-1688; the reduction plan sums a destination's sources
 * in the order the edges were added, whatever their types: :563-607, 152-197; BaseTypes_Binary.h:759-848 per edge).
 * Group g: h_ne[g] edges h_v0[g] -> h_v1[g] of shape (h_d0[g], h_d1[g], h_rd[g]), one of the six above; two groups may
 * share a shape, but no two of (6,3,1), (6,3,2) and (6,3,3) may appear in one plan: they share their widths, so one
 * off-diagonal block could be fed by both, and a block is summed by the kernel of ONE shape (SPP_E_UNSUPPORTED).
 * UNARY edges (priors: GPS fixes, anchors, surveyed beacons; CBaseEdgeImpl with ONE vertex, include/slam/BaseTypes_Unary.h,
 * e.g. CEdgeLandmark3DPrior, ROCV_Types.h:228-320): a group with h_d1[g] == 0 and h_v1[g] == NULL holds unary edges on
 * h_v0[g], of shape (d0, rd) = (3,3) or (6,6) (anything else SPP_E_UNSUPPORTED). Per edge H00 = J0^T Omega J0 is added to the
 * vertex's diagonal block and g0 = J0^T (Omega r) to its eta segment (Calculate_Hessians_v2, BaseTypes_Unary.h:547-587);
 * there is no off-diagonal block, the structure does not change, d_J1[g] is ignored and may be NULL, and no self-edge check
 * applies. A unary edge takes its place among the sources of its vertex by its h_seq position like any other edge. Robust
 * weights on a unary group: the reference HAS the branch (:554-569) -- H00 and g0 carry w ONCE each (g0 = J0^T (Omega r w)),
 * and so they do here. The built-in identity factor `unary_vertex` is independent of these groups (ROCV passes -1,
 * CNullUnaryFactorFactory, src/slam_app/SolveROCVImpl.cpp:42-43). A plan holding a unary group is assembled by
 * spp_assemble_groups_device (spp_assemble_device: SPP_E_STATE), also when it is the only group. h_seq[g][e]: position of that edge in the graph's global edge order (all of them a permutation of
 * 0 .. sum(ne) - 1; h_seq, or h_seq[g], NULL: the position in the concatenation of the groups). Every destination -- diagonal
 * block, eta segment, off-diagonal block, also one fed by several groups -- sums its contributions in ascending position,
 * first assigned, rest added (vertices of degree > 24: the fixed butterfly of the wave kernel over that order). The
 * structure (spp_assemble_get_structure, NNZB / NVALS) is the union: every diagonal block and one upper block per
 * connected pair. With one group and no h_seq this IS spp_assemble_analyze, and spp_assemble_device accepts the plan;
 * spp_assemble_groups_device (host arrays of n_groups device pointers) accepts any plan and gives the same bits on a
 * one-group plan.
 * Unary factor and damping as above; robust weights per group (NULL: plain), reset by either analyze call.
 * SPP_E_UNSUPPORTED: a shape not instantiated, two of (6,3,1) (6,3,2) (6,3,3) side by side, a (7,3,2) group beside any other group, more than SPP_MAX_EDGE_GROUPS groups. SPP_E_BADARG: a vertex width that does
 * not match its group, a bad index, a self edge, h_seq not a permutation; the ctx then holds no assembly plan.
 * SPP_E_STATE: spp_assemble_device on a plan of several groups, spp_assemble_groups_device without a plan. */
#define SPP_MAX_EDGE_GROUPS 4
int spp_assemble_analyze_groups(spp_ctx *ctx, int64_t nv, const int32_t *h_dim, int n_groups,
	const int64_t *h_ne, const int64_t *const *h_v0, const int64_t *const *h_v1, const int64_t *const *h_seq,
	const int32_t *h_d0, const int32_t *h_d1, const int32_t *h_rd, int64_t unary_vertex);
int spp_assemble_groups_device(spp_ctx *ctx, const double *const *d_J0, const double *const *d_J1,
	const double *const *d_Omega, const double *const *d_r, double damping, double *d_vals_out, double *d_eta_out);
int spp_assemble_set_group_edge_weights(spp_ctx *ctx, int group, const double *d_w);
/* Ternary edges: self-calibrating bundle adjustment, one residual of CEdgeP2CI3D (include/slam/BA_Types.h:562-700) feeding
 * a camera v0 (6), a point v1 (3) and an intrinsics vertex v2 (CVertexIntrinsics, :141-206: 5 coordinates fx fy cx cy kappa).
 * replaces, for an n-ary edge: Alloc_HessianBlocks_v2 (symbolic; include/slam/BaseTypes.h:1540-1767: one upper block per
 * pair of the edge's vertices, transposed when the ids are reversed) and Calculate_Hessians_v2 (numeric; :1981-2130) + the
 * reduction plan (NonlinearSolver_Lambda_Base.h:563-607, 152-197).
 * Inside this library an intrinsics vertex is d2 = 6 WIDE with live2 = 5 live coordinates and one inert one: h_dim[v2] is 6,
 * J2 is ne x (2x6) column-major with a zero last column, the assembly puts 1.0 on the inert diagonal entry (before the
 * damping), its row and column are otherwise exact zeros and its eta entry is 0 -- the solution's inert entry is exactly
 * +-0, and Lambda keeps the two widths {6, 3} of the guided Schur mode, with "poses" = cameras + intrinsics.
 * One instantiated shape: (d0, d1, d2, rd) = (6,3,6,2) with live2 = 5; anything else is SPP_E_UNSUPPORTED. SPP_E_BADARG: a
 * bad index, a vertex width that does not match, two equal vertices in one edge, a vertex that is the camera of one edge
 * and the intrinsics of another; the ctx then holds no assembly plan. Structure (spp_assemble_get_structure): every
 * diagonal block and one upper block per connected pair among (v0, v1), (v0, v2), (v1, v2). Every destination is summed
 * in edge order: H00, H01, H11, g0, g1 by the kernels of spp_assemble_device on the (6,3,2) edges (v0, v1), bit for bit;
 * what touches an intrinsics vertex -- H02, H12, H22, g2 -- sequentially (first assigned, rest added) up to 24 edges, beyond
 * that by a two-stage reduction over chunks of SPP_INFO_ASM_HUB_CHUNK edges whose result depends on that constant alone
 * (DESIGN section 20). The unary factor is the identity on the LIVE coordinates of unary_vertex when that is an
 * intrinsics vertex; `damping` is added to every diagonal entry. Robust weights: SPP_E_UNSUPPORTED on such a plan.
 * SPP_E_STATE: spp_assemble_ternary_device without a ternary plan, spp_assemble_device / _groups_device on one. */
int spp_assemble_analyze_ternary(spp_ctx *ctx, int64_t nv, const int32_t *h_dim, int64_t ne, const int64_t *h_v0,
	const int64_t *h_v1, const int64_t *h_v2, int d0, int d1, int d2, int live2, int rd, int64_t unary_vertex);
int spp_assemble_ternary_device(spp_ctx *ctx, const double *d_J0, const double *d_J1, const double *d_J2,
	const double *d_Omega, const double *d_r, double damping, double *d_vals_out, double *d_eta_out);
/* the weights themselves, on the device: w_e = kernel(||r_e|| / scale) -- CRobustify_ErrorNorm_Default::f_RobustWeight
 * (include/slam/RobustUtils.h:396-400) with kind 0 = Huber, w = 1 for x <= param, param / x beyond (CHuberLoss::operator (),
 * include/geometry/RobustLoss.h:100-104; the reference's default param is 1.345). Asynchronous on the ctx stream. */
int spp_edge_robust_weights_device(spp_ctx *ctx, int64_t n_edges, int rd, int kind, double scale, double param,
	const double *d_r, double *d_w_out);

/* ---- device memory helpers for hosts without a HIP runtime of their own ---------------------------- */
/* ---- on-device geometry of 2D pose graphs (CEdgePose2D) --------------------------
 * spp_se2_linearize_device: per edge (pose v0 -> pose v1, measurement z = dx dy dtheta in the frame of
 * v0) the Jacobians of the expectation and the error r = z - h(x), exactly the quantities of
 * C2DJacobians::Absolute_to_Relative (include/slam/2DSolverBase.h:373-418) and CEdgePose2D (angle error
 * wrapped by f_ClampAngularError_2Pi, :90-94), written in the layout spp_assemble_device reads
 * (J0, J1: ne x 3x3 column-major, r: ne x 3). All pointers are device pointers; v0 / v1 are int32.
 * spp_se2_update_device: ||dx||^2 -> *h_dx_norm2 (deterministic two-stage sum) and, if `apply`,
 * x <- x (+) dx with the angle clamped (CVertexPose2D::Operator_Plus, include/slam/SE2_Types.h:70-74).
 * It synchronizes the stream: the stopping test of the Gauss-Newton loop needs the norm on the host
 * (NonlinearSolver_Lambda.h:638-650). */
int spp_se2_linearize_device(spp_ctx *ctx, int64_t n_edges, const int32_t *d_v0, const int32_t *d_v1,
	const double *d_poses, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_se2_update_device(spp_ctx *ctx, int64_t n_vertices, double *d_poses, const double *d_dx, int apply,
	double *h_dx_norm2);

/* ---- on-device geometry of 2D landmark SLAM (CEdgePose2D + CEdgePoseLandmark2D) ----------------------
 * Poses (x y theta) and landmarks (x y) live in ONE flat state laid out like eta (in 2D the increment has the state's
 * layout); vertices are addressed by scalar offset (int64), so 2-wide vertices may sit between the poses.
 * spp_se2_linearize_at_device: spp_se2_linearize_device with the two pose offsets given per edge (3 * id reproduces it).
 * spp_se2_rb_linearize_device: per observation the expectation (||l - p||, clamp(atan2(dn, de) - theta)) and the 2x3 / 2x2
 * Jacobians of C2DJacobians::Observation2D_RangeBearing (include/slam/2DSolverBase.h:443-496; the range is floored at 1e-5
 * before the Jacobians are formed), r = z - h with the bearing error wrapped (CEdgePoseLandmark2D::
 * Calculate_Jacobians_Expectation_Error, include/slam/SE2_Types.h:562-573); layout of the (3,2,2) group: J0 ne x (2x3)
 * column-major, J1 ne x (2x2), r ne x 2.
 * spp_slam2d_update_device: ||dx||^2 over the n state entries (two-stage sum) and, if `apply`, x += dx, the n_pose_angles
 * entries at d_angle_off clamped afterwards (CVertexPose2D::Operator_Plus, SE2_Types.h:70-74); landmarks are plain sums
 * (CVertexLandmark2D::Operator_Plus, :89). Synchronizes the stream. */
int spp_se2_linearize_at_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_off0, const int64_t *d_off1,
	const double *d_state, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_se2_rb_linearize_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_pose_off, const int64_t *d_lm_off,
	const double *d_state, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_slam2d_update_device(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_pose_angles,
	const int64_t *d_angle_off, int apply, double *h_dx_norm2);

/* ---- on-device geometry of 3D pose graphs (CEdgePose3D) ---------------------------
 * Poses: 6 doubles [t | axis-angle]. Expectation = C3DJacobians::Absolute_to_Relative(v0, v1), error
 * [z_t - e_t ; log(R(z_r) R(e_r)^T)] (include/slam/SE3_Types.h:264-286), Jacobians w.r.t. the increments of
 * Relative_to_Absolute (3DSolverBase.h:807-850) -- analytic here, forward differences with delta = 1e-9 in
 * the reference (:1331-1371). J0, J1: ne x (6x6) column-major, r: ne x 6 (the (6,6,6) group of
 * spp_assemble_device). spp_se3_update_device: ||dx||^2 and x <- x (+) dx (CVertexPose3D::Operator_Plus). */
int spp_se3_linearize_device(spp_ctx *ctx, int64_t n_edges, const int32_t *d_v0, const int32_t *d_v1,
	const double *d_poses, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_se3_update_device(spp_ctx *ctx, int64_t n_vertices, double *d_poses, const double *d_dx, int apply,
	double *h_dx_norm2);

/* ---- on-device geometry of 3D landmark SLAM (CEdgePose3D + CEdgePoseLandmark3D) ----------------------
 * Poses [t | axis-angle] (6) and landmarks XYZ (3) live in ONE flat state laid out like eta (in 3D, too, the increment
 * has the state's layout); vertices are addressed by scalar offset (int64), so landmarks may sit between the poses.
 * spp_se3_linearize_at_device: spp_se3_linearize_device with the two pose offsets given per edge (6 * id reproduces it,
 * bit for bit).
 * spp_se3_xyz_linearize_device: per observation the expectation e = R(a)^T (l - t) of C3DJacobians::
 * Absolute_to_Relative_Landmark (include/slam/3DSolverBase.h:1528-1539), r = z - e, nothing wrapped (CEdgePoseLandmark3D::
 * Calculate_Jacobians_Expectation_Error, include/slam/SE3_Types.h:568-586), and the Jacobians w.r.t. the pose increment of
 * Relative_to_Absolute (t' = t + R dt, R' = R exp(dr), 3DSolverBase.h:807-850) and w.r.t. the landmark -- analytic here,
 * d e / d pose = [-I | [e]x], d e / d l = R^T, forward differences with delta = 1e-9 in the reference (:1602-1637). Layout
 * of the (6,3,3) group: J0 ne x (3x6) column-major, J1 ne x (3x3), r ne x 3.
 * spp_slam3d_update_device: ||dx||^2 over the n state entries (two-stage sum) and, if `apply`, the 6 entries at each of
 * the n_poses offsets d_pose_off <- pose (+) dx (CVertexPose3D::Operator_Plus, the composition spp_se3_update_device
 * applies, same bits), every other entry a plain sum (CVertexLandmark3D::Operator_Plus, SE3_Types.h:110-113).
 * Synchronizes the stream. */
int spp_se3_linearize_at_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_off0, const int64_t *d_off1,
	const double *d_state, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_se3_xyz_linearize_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_pose_off, const int64_t *d_lm_off,
	const double *d_state, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_slam3d_update_device(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_poses,
	const int64_t *d_pose_off, int apply, double *h_dx_norm2);

/* ---- on-device geometry of range-only constant-velocity SLAM (ROCV, include/slam/ROCV_Types.h) ---------
 * Receivers [p | v] (6, CVertexPositionVelocity3D :31-72) and transmitters XYZ (3, CVertexLandmark3D) live in ONE flat state
 * laid out like eta; vertices are addressed by scalar offset (int64), as in spp_se3_xyz_linearize_device.
 * spp_rocv_range_linearize_device: CEdgePosVel_Landmark3D<false>::Calculate_Jacobians_Expectation_Error (:163-205):
 * e = |p - l|, r = z - e, J0 = [(p - l)^T / e | 0 0 0], J1 = -J0[0:3]; layout of the (6,3,1) group. The distance is formed
 * from the differences, where the reference writes the expanded polynomial (which cancels). DEVIATION: at e = 0 the
 * reference divides 0 by 0; here both Jacobians are exact zeros and r = z -- nothing is divided by e.
 * spp_rocv_cv_linearize_device: CEdgeConstVelocity3D<false> (:543-614), d_dt the measured time step per edge: expectation
 * (p0 + v0 dt, v0), r = -(x1 - expectation) -- the reversed sign the reference chose (:608) --, J0 = -[I, dt I; 0, I], J1 = I;
 * layout of the (6,6,6) group (Omega: the upper-left 6x6 of the parsed matrix, :394).
 * The transmitter prior CEdgeLandmark3DPrior (:228-320) needs no kernel: J = I, r = 0 whatever the state (:302-310), chi2 0;
 * a unary (3,3) group whose constants are uploaded once. Both vertex types add plainly (:60-63): the update is
 * spp_slam2d_update_device with n_pose_angles = 0; chi2: spp_edge_chi2_device with rd 1 and rd 6. */
int spp_rocv_range_linearize_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_recv_off, const int64_t *d_lm_off,
	const double *d_state, const double *d_measurements, double *d_J0, double *d_J1, double *d_r);
int spp_rocv_cv_linearize_device(spp_ctx *ctx, int64_t n_edges, const int64_t *d_off0, const int64_t *d_off1,
	const double *d_state, const double *d_dt, double *d_J0, double *d_J1, double *d_r);

/* ---- on-device geometry of bundle adjustment (CEdgeP2C3D) -------------------------
 * Cameras: 6 doubles each [t | axis-angle], world -> camera, and 5 constant intrinsics each (fx fy cx cy k:
 * CVertexCam, include/slam/BA_Types.h); points: XYZ. spp_ba_linearize_device evaluates per observation the
 * projection of CBAJacobians::Project_P2C (include/slam/BASolverBase.h:260-325), r = z - uv, and its
 * Jacobians w.r.t. the camera increment of C3DJacobians::Relative_to_Absolute (t' = t + R dt,
 * R' = R exp(dr), include/slam/3DSolverBase.h:807-850) and w.r.t. the point -- analytically, where the
 * reference takes forward differences with delta = 1e-9 (BASolverBase.h:559-620): agreement to ~1e-7
 * relative, the noise of the difference quotients. Output layout = input of spp_assemble_device for the
 * (6,3,2) edge group: J0 no x (2x6) column-major, J1 no x (2x3), r no x 2. cam_of / pt_of: int32 indices
 * into the camera / point arrays.
 * spp_ba_update_device: ||dx||^2 over the n_dx entries of dx -> *h_dx_norm2, and if `apply` camera i
 * <- camera i (+) dx[cam_dxoff[i] .. +6) (the composition above), point j += dx[pt_dxoff[j] .. +3)
 * (CVertexCam / CVertexXYZ::Operator_Plus). Synchronizes the stream. */
int spp_ba_linearize_device(spp_ctx *ctx, int64_t n_obs, const int32_t *d_cam_of, const int32_t *d_pt_of,
	const double *d_cams, const double *d_intrinsics, const double *d_points, const double *d_measurements,
	double *d_J0, double *d_J1, double *d_r);
int spp_ba_update_device(spp_ctx *ctx, int64_t n_cams, double *d_cams, const int64_t *d_cam_dxoff,
	int64_t n_points, double *d_points, const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, int apply,
	double *h_dx_norm2);

/* ---- on-device geometry of Sim(3) bundle adjustment (CEdgeP2C_XYZ_Sim3_G, include/slam/Sim3_Types.h:492-595) ----
 * Cameras: 7 doubles each, v = [t | w | s] in sim(3) (CVertexCamSim3, Sim3_Types.h:178-238), and 5 constant intrinsics
 * each (fx fy cx cy d); points: XYZ. The camera is T = Exp(v) (CSim3Jacobians::t_Exp, include/slam/Sim3SolverBase.h:
 * 3829-3905): rotation exp([w]x), scale e^s, translation tau = a t + b (w x t) + c w x (w x t), with a, b, c the
 * coefficients of V there. spp_sim3_ba_linearize_device evaluates per observation CSim3Jacobians::Project_P2C_XYZ
 * (:630-681): x = T^-1 X = e^-s R^T (X - tau), p - c = (fx x0/x2, fy x1/x2), k = d / (0.5 fx fy) -- the PRODUCT of the focal
 * lengths, not the mono BA form --, uv = c + (1 + |p - c|^2 k)(p - c), residual z - uv; and its Jacobians w.r.t. the
 * POST-multiplicative camera increment T Exp(delta) of Relative_to_Absolute (:435-452) and w.r.t. the point --
 * analytically (d x / d delta = [-I | [x]x | -x], d x / d X = e^-s R^T), where the reference takes forward differences
 * with delta = 1e-9 (:1043-1062). The scale column of J0 is identically zero (the projection does not see the scale of
 * the camera frame) and is written as zeros; nothing is divided by |p - c|, a point on the optical axis gives finite
 * Jacobians. a, b, c are evaluated by a Taylor series for s^2 + |w|^2 < 1 and in closed form beyond (the reference: four
 * cells at 1e-6, whose truncated series approximate the same functions); both match the exact Exp to rounding.
 * Output layout = input of spp_assemble_device for the (7,3,2) edge group: J0 no x (2x7) column-major, J1 no x (2x3),
 * r no x 2. cam_of / pt_of: int32 indices into the camera / point arrays.
 * spp_sim3_update_device has the signature of spp_ba_update_device: ||dx||^2 over the n_dx entries of dx -> *h_dx_norm2,
 * and if `apply` camera i <- Log(Exp(camera i) Exp(dx[cam_dxoff[i] .. +7))) (CVertexCamSim3::Operator_Plus; v_Log
 * :3740-3819, with V^-1 in closed form instead of the reference's QR; the composite rotation through unit quaternions,
 * the composite scale as s1 + s2), point j += dx[pt_dxoff[j] .. +3). Synchronizes the stream. */
int spp_sim3_ba_linearize_device(spp_ctx *ctx, int64_t n_obs, const int32_t *d_cam_of, const int32_t *d_pt_of,
	const double *d_cams, const double *d_intrinsics, const double *d_points, const double *d_measurements,
	double *d_J0, double *d_J1, double *d_r);
int spp_sim3_update_device(spp_ctx *ctx, int64_t n_cams, double *d_cams, const int64_t *d_cam_dxoff,
	int64_t n_points, double *d_points, const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, int apply,
	double *h_dx_norm2);

/* ---- on-device geometry of stereo bundle adjustment (CEdgeP2SC3D, include/slam/BA_Types.h:705-811) ----
 * Cameras: 6 doubles each [t | axis-angle], world -> left camera, and 6 constant intrinsics each (fx fy cx cy d b, b the
 * baseline: CVertexSCam, BA_Types.h:211-290); points: XYZ; measurements: 3 per observation (u v u_right).
 * spp_ba_stereo_linearize_device replaces CBAJacobians::Project_P2SC (include/slam/BASolverBase.h:462-537, with Jacobians
 * :781-841) as CEdgeP2SC3D::Calculate_Jacobians_Expectation_Error calls it: x = R X + t, p = (fx x0/x2 + cx,
 * fy x1/x2 + cy), k = d / (0.5 (fx + fy)), rho = |p - c|, uv = c + (1 + rho k)(p - c); the right camera sees the point
 * moved by -b (row 0 of R)^T, i.e. x - b e0 in the camera frame (the form evaluated), through the same projection and
 * distortion with its own rho; expectation e = (uv0, uv1, uv_right0), r = z - e. Jacobians w.r.t. the camera increment of
 * C3DJacobians::Relative_to_Absolute (t' = t + R dt, R' = R exp(dr), include/slam/3DSolverBase.h:807-850) and w.r.t. the
 * point -- analytic, where the reference takes forward differences with delta = 1e-9; the distortion's derivative
 * (1 + rho k) I + k (p - c)(p - c)^T / rho is evaluated with (p - c) / rho := 0 at rho = 0, so a point on the optical
 * axis gives finite Jacobians. Output layout = input of spp_assemble_device for the (6,3,3) edge group: J0 no x (3x6)
 * column-major, J1 no x (3x3), r no x 3. cam_of / pt_of: int32 indices into the camera / point arrays. The vertex update
 * is spp_ba_update_device (CVertexSCam::Operator_Plus is the same Relative_to_Absolute). */
int spp_ba_stereo_linearize_device(spp_ctx *ctx, int64_t n_obs, const int32_t *d_cam_of, const int32_t *d_pt_of,
	const double *d_cams, const double *d_intrinsics, const double *d_points, const double *d_measurements,
	double *d_J0, double *d_J1, double *d_r);

/* ---- on-device geometry of self-calibrating bundle adjustment (CEdgeP2CI3D, include/slam/BA_Types.h:562-700) ----
 * Cameras: 6 doubles each [t | axis-angle], world -> camera; intrinsics VERTICES: 5 doubles each (fx fy cx cy kappa:
 * CVertexIntrinsics, BA_Types.h:141-206), observation e uses d_intrinsics + 5 intr_of[e]; points: XYZ.
 * spp_ba_intrinsics_linearize_device evaluates CBAJacobians::Project_P2C (include/slam/BASolverBase.h:260-327): p - c =
 * (fx x0/x2, fy x1/x2), k = kappa / (0.5 (fx + fy)), uv = c + (1 + r^2 k)(p - c), r = |p - c|; residual z - uv. J0, J1 and
 * the residual come from the device function of spp_ba_linearize_device and are bit-identical to its output for the
 * gathered per-camera intrinsics. J2 (no x (2x6) column-major, last column zeros: the inert coordinate) is analytic
 * w.r.t. the plain increment of Relative_to_Absolute_Intrinsics (BASolverBase.h:204-212), where the reference takes
 * forward differences with delta = 1e-9 (:690-759); nothing is divided by r, a point on the optical axis gives finite
 * Jacobians. Output = input of spp_assemble_ternary_device.
 * spp_ba_intrinsics_update_device: ||dx||^2 over the 5 LIVE entries dx[intr_dxoff[i] .. +5) of every intrinsics vertex ->
 * *h_dx_norm2 and, if `apply`, CVertexIntrinsics::Operator_Plus AS WRITTEN (BA_Types.h:170-185): fx fy cx cy plain sums,
 * kappa' = (kappa + dkappa) / (0.5 fx fy) * (0.5 fx' fy') -- renormalised through the PRODUCT of the focal lengths of the old
 * and of the new state. Cameras and points keep spp_ba_update_device (whose norm over the padded dx already holds the
 * intrinsics' share: the inert entries are zero). Synchronizes the stream. */
int spp_ba_intrinsics_linearize_device(spp_ctx *ctx, int64_t n_obs, const int32_t *d_cam_of, const int32_t *d_pt_of,
	const int32_t *d_intr_of, const double *d_cams, const double *d_intrinsics, const double *d_points,
	const double *d_measurements, double *d_J0, double *d_J1, double *d_J2, double *d_r);
int spp_ba_intrinsics_update_device(spp_ctx *ctx, int64_t n_intrinsics, double *d_intrinsics, const int64_t *d_intr_dxoff,
	const double *d_dx, int apply, double *h_dx_norm2);

/* ---- scalars of the Levenberg-Marquardt control (include/slam/NonlinearSolver_Lambda_LM.h) ----------
 * chi2 = sum_e r_e^T Omega_e r_e (f_Error, :1078-1095); the largest diagonal entry of any vertex Hessian
 * J_i^T Omega J_i over all edges (f_InitialDamping multiplies it by tau = 1e-3, :151-199); the denominator
 * dx . (alpha dx + eta) of the gain ratio (Aftermath, :204-222). Device inputs, host outputs, deterministic
 * reductions; each call synchronizes the stream. rd / (d0, d1): the edge group of spp_assemble_analyze (chi2: rd 1, 2, 3
 * or 6; max diagonal: (rd, d0, d1) = (2,6,3), (3,3,3), (6,6,6), (3,6,3), the XYZ observations, (1,6,3), the ranges, or (2,7,3), the
 * projections into Sim(3) cameras). */
int spp_edge_chi2_device(spp_ctx *ctx, int64_t n_edges, int rd, const double *d_r, const double *d_Omega, double *h_chi2);
int spp_edge_hessian_maxdiag_device(spp_ctx *ctx, int64_t n_edges, int rd, int d0, int d1, const double *d_J0,
	const double *d_J1, const double *d_Omega, double *h_max);
int spp_lm_gain_denominator_device(spp_ctx *ctx, int64_t n, const double *d_dx, const double *d_eta, double alpha,
	double *h_out);

int spp_device_malloc(spp_ctx *ctx, size_t bytes, void **d_ptr);
int spp_device_free(spp_ctx *ctx, void *d_ptr);
int spp_memcpy_h2d(spp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int spp_memcpy_d2h(spp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* asynchronous on the ctx stream */
int spp_memcpy_d2d(spp_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);

/* switch SPP_FLAG_PROFILE on / off for the following solves (the hipEvents around phases and around the
 * dominant kernel cost microseconds per solve; a benchmark times with profiling off and reads the
 * breakdown from a separate profiled pass) */
int spp_set_profiling(spp_ctx *ctx, int on);

/* ---- profiling (SPP_FLAG_PROFILE) ------------------------------------------------------------------
 * phase names follow the reference's __SCHUR_PROFILING / Dump() vocabulary
 * (LinearSolver_Schur.h:1889-1912, NonlinearSolver_Lambda.h:250-276). */
#define SPP_PHASE_PERMUTE   0
#define SPP_PHASE_SCHUR_INV 1  /* C^-1 and W = -U C^-1 */
#define SPP_PHASE_SCHUR_GEMM 2 /* S = A + W U^T */
#define SPP_PHASE_SCHUR_RHS 3
#define SPP_PHASE_FACTOR    4  /* numeric Cholesky (dense or sparse) */
#define SPP_PHASE_TRISOLVE  5
#define SPP_PHASE_BACKSUBST 6  /* landmark back-substitution */
#define SPP_PHASE_ASSEMBLE  7
#define SPP_PHASE_TOTAL     8
#define SPP_N_PHASES        9
/* milliseconds of each phase of the LAST solve / assemble call (hipEvent elapsed on the ctx stream) */
int spp_get_phase_ms(spp_ctx *ctx, double *ms_out /* [SPP_N_PHASES] */);
/* hipEvent-timed average duration (ms) of the dominant kernel family of the last solve:
 * the MFMA trailing-update GEMM launches of the dense factor; n_launches/flops are totals */
int spp_get_dominant_kernel(spp_ctx *ctx, double *ms_total, int64_t *n_launches, double *flops);

/* ---- micro-benchmarks used by bench.py to report measured peaks beside the spec peaks ------------ */
int spp_microbench_copy(spp_ctx *ctx, size_t bytes, int iters, double *gb_per_s);
int spp_microbench_mfma_f64(spp_ctx *ctx, int iters, double *tflops);
/* read-negate-write of an n x n fp64 matrix (n % 128 == 0) in the trailing-update kernel's C-tile lane
   pattern; a known byte count (2 * 8 * n * n per launch) to calibrate the PMC traffic counters with */
int spp_microbench_ctile(spp_ctx *ctx, int n, int iters, double *gb_per_s);
/* the bulk trailing update of ONE dense factorization step, stand-alone: an m x (m + 1) trailing matrix (upper
 * tiles) receives a rank-128 update `iters` times back to back; *ms_per_launch = hipEvent time per launch.
 * Useful flops per launch = 128 m (m + 1) + 256 m (what bench.py's roofline counts for the same launch). */
int spp_microbench_update(spp_ctx *ctx, int64_t m, int iters, double *ms_per_launch);

/* direct access to the dense kernels for unit tests (device pointers; A is n x n col-major, ld) */
int spp_dense_potrf_upper(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld);
/* A x = b by the dense path (upper triangle of A read; A <- R, b <- x) */
int spp_dense_posv(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, double *d_b);
/* A X = B for nrhs columns: A is factored as by spp_dense_potrf_upper (no right-hand side rides along; A <- R with the
 * same bits), then B (n x nrhs, column-major, ldb >= n) <- X by the multi-column solves of the kept-factor path
 * (spp_solve_device); returns the factor's status (B untouched after SPP_NOT_POSDEF) */
int spp_dense_posv_multi(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, double *d_B, int64_t ldb, int64_t nrhs);
/* the inverse from the factor: A is factored as by spp_dense_potrf_upper (A <- R with the same bits), then Z (n x n,
 * column-major, ldz >= n) <- A^-1, whole and exactly symmetric, by the block recursion of spp_schur_sigma_device on the
 * kept upper factor; nothing of Z outside its n x n is written. Returns the factor's status (Z untouched after
 * SPP_NOT_POSDEF) */
int spp_dense_potri(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, double *d_Z, int64_t ldz);
/* NOT FOR USERS -- a timing entry (tools/schur_sigma_time.py): the first step of spp_schur_sigma_device alone, Z = S^-1
 * into the ctx's workspace, nothing else written; needs the kept factor and refuses as spp_schur_sigma_device does */
int spp_schur_sigma_dense_device(spp_ctx *ctx);
/* NOT FOR USERS -- a timing entry (tools/schur_sparse_again_time.py): the first step of spp_schur_sparse_sigma_device alone,
 * the blocks of Z = S^-1 on S's stored pattern into the ctx's workspace, nothing else written; needs the kept factor and
 * refuses as spp_schur_sparse_sigma_device does */
int spp_schur_sparse_sigma_inverse_device(spp_ctx *ctx);
/* the same with the tile structure of A given: words[i], bit j set = the 128 x 128 tile (i, j), i <= j, of A may be nonzero
 * (nwords = ceil(n / 128); nwords = 0: every tile). The call adds the diagonal tiles and the right-hand side's tile column
 * and closes the pattern under elimination; the streamed factorization then skips the tiles that stay zero. A tile
 * outside the closed pattern must hold exact zeros. Results equal those of spp_dense_posv. */
int spp_dense_posv_masked(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, double *d_b, const uint64_t *words, int64_t nwords);
/* host only: the tile mask of an n x n matrix of bs x bs blocks (i1[q], i2[q]), q < nblk, at rows / columns bs * index:
 * words[i], bit j = tile (i, j) of 128 x 128 touched by a block (upper triangle); diagonal tiles always, with has_rhs the
 * tile column of column n in every row; with fill the pattern is closed under elimination. *n_updates (may be NULL):
 * rank-128 tile updates of a factorization on the pattern. Returns the number of words written (tile rows, at most 64),
 * 0 when the matrix has more than 64 tile columns (no mask: every tile), or a negative error. */
int spp_tile_mask_host(int64_t n, int bs, int64_t nblk, const int32_t *i1, const int32_t *i2, int has_rhs, int fill,
	uint64_t *words, int64_t *n_updates);
/* host only: the filled tile mask the dense Schur plan of a block pattern (as spp_schur_plan_host takes it) hands to the
 * factorization of S; it covers the landmarks of every shard whatever shard_rank is. Returns the number of words, 0 for
 * "every tile", or a negative error. The mask is that of the natural camera order. */
int spp_schur_tile_mask_host(int64_t nb, const int32_t *dim, const int64_t *col_ptr, const int64_t *row_idx, int shard_rank,
	int shard_world, uint64_t *words);
/* host only: the camera order the Schur plan of a block pattern uses for landmark shard shard_rank of shard_world (read
 * back from that plan; every shard chooses the same) and the cost model of the streamed factor behind it. flags: 1 = sparse S, 2 = MIS (both keep the natural order). cam_order[position] = camera in
 * natural numbering (room for every pose). figures (8 entries): listed tiles, rank-128 tile updates, critical path of
 * diagonal tiles and modelled launch cost in microseconds of the NATURAL order, then the same four of the order used.
 * order_in (may be NULL): a permutation of the cameras -- nothing is chosen, figures[4..7] are those of order_in.
 * spp_schur_tile_mask_host keeps reporting the mask of the natural order. Returns 1 when the order used differs from the
 * natural one, 0 when it does not, or a negative error. */
int spp_schur_cam_order_host(int64_t nb, const int32_t *dim, const int64_t *col_ptr, const int64_t *row_idx, int shard_rank,
	int shard_world, int flags, const int64_t *order_in, int64_t *cam_order, double *figures);
/* host only: the workgroup order of the streamed dense factor for an n x n matrix (+ right-hand side column with has_rhs)
 * whose FILLED tile mask is words[0 .. nwords) (nwords = ceil(n / 128), or 0: no mask, every tile): table[q] = (i << 16) | j,
 * the tile workgroup q owns (room for 64 * 65 / 2 + 64 entries). resident: workgroups the device holds at once; early:
 * the value of SPP_TAIL_EARLY to apply; beta: the order key i + beta j (SPP_TAIL_ORDER_BETA, 0 = row by row). With a mask,
 * early != 0 and the conditions of DESIGN section 11 met, the tiles of the trailing tile rows r* .. go first; otherwise
 * the table is the sorted one. info (may be NULL, 5 entries): tiles in front, r* (tile rows when none), whole rows
 * resident D, live demand of the other tiles, tiles of the widest row. Returns the number of entries or a negative error.
 * Bit 1 of early (early = 3): the table the launch uses under the depth order of the mask (spp_tail_step_order_host) where
 * that is not k ascending (SPP_TAIL_EARLY_LEAD) -- a trailing run too large to go first whole has its
 * leading rows r* .. r2 in front, then the rows < r* by the depth of their diagonal tile, then the rows > r2; info as above
 * with the tiles and r* of those rows. The call is spp_tail_plan_host with nothing in front and no limit on the tile rows. */
int spp_tail_order_host(int64_t n, int has_rhs, const uint64_t *words, int64_t nwords, int resident, int early, double beta,
	int32_t *table, int32_t *info);
/* host only: everything the host decides for the streamed launch that takes the region behind the
 * first `front` tile rows (0: the whole factorization) of an n x n matrix (+ right-hand side column with has_rhs), computed
 * by the function the launch itself calls. words[0 .. nwords): the FILLED tile mask of the whole matrix (nwords =
 * ceil(n / 128), or 0: no mask); step_order[0 .. norder) (norder = 0: none): the caller's step order, used where it has one
 * entry per tile row and front = 0; tail_rows: SPP_TAIL_ROWS; resident, beta: as above; early: bit 0 SPP_TAIL_EARLY, bit 1
 * SPP_TAIL_EARLY_LEAD, bit 2 set = SPP_TAIL_MASK off. Out (each may be NULL but table): rowbits (65 words) -- word i + 1 the
 * listed tiles of the region's tile row i in region indices, word 0 the row panel in front of the region --, steps (72
 * entries): the launch's step list as the kernel unpacks it, -1 = the row panel in front, 127 behind the last step,
 * table and info as above. Returns the number of table entries, 0 where the region is not one streamed launch (nothing
 * is written), SPP_E_BADARG for a step order that is no permutation, or another negative error. */
int spp_tail_plan_host(int64_t n, int has_rhs, const uint64_t *words, int64_t nwords, const int32_t *step_order, int64_t norder,
	int front, int tail_rows, int resident, int early, double beta, uint64_t *rowbits, int32_t *steps, int32_t *table, int32_t *info);
/* spp_dense_posv_masked with the order in which a tile of the streamed factorization applies its steps given:
 * step_order[0 .. nwords), a permutation of the tile rows 0 .. nwords - 1 (anything else: SPP_E_BADARG; nwords > 0). A tile
 * applies the steps its mask selects in that order instead of k ascending -- a different summation order, the same
 * factor up to rounding; the identity gives the bits of spp_dense_posv_masked. It takes effect where the whole
 * factorization is one streamed launch (up to SPP_TAIL_ROWS tile rows) and is ignored elsewhere. */
int spp_dense_posv_ordered(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, double *d_b, const uint64_t *words, int64_t nwords,
	const int32_t *step_order);
/* host only: the depth order of the steps for the tile mask words[0 .. nwords) (nwords = ceil(n / 128); closed under
 * elimination by the call, right-hand side column included): steps sorted by the depth of their diagonal tile in the tile
 * DAG -- depth(k) = 1 + max depth(j) over j < k with tile (j, k) listed, as in the cost model --, ties by k. Returns the
 * number of entries or a negative error. (The Schur plan uses it under a dissected camera order only: DESIGN section 25.) */
int spp_tail_step_order_host(int64_t n, const uint64_t *words, int64_t nwords, int32_t *step_order);
/* host only: the step order the Schur plan of a block pattern hands to the streamed factor for landmark shard shard_rank
 * of shard_world, read back from that plan (flags as spp_schur_cam_order_host): one entry per tile row of S (room for 64),
 * the identity for every camera order but a dissected one and with SPP_TAIL_STEP_ORDER=0. Returns the number of entries
 * (0 without a tile mask) or a negative error. */
int spp_schur_step_order_host(int64_t nb, const int32_t *dim, const int64_t *col_ptr, const int64_t *row_idx, int shard_rank,
	int shard_world, int flags, int32_t *step_order);
/* C (m x n, ldc) -= A^T B with A: k x m (lda), B: k x n (ldb): the MFMA trailing-update kernel */
int spp_dense_gemm_tn_sub(spp_ctx *ctx, int64_t m, int64_t n, int64_t k,
	const double *d_A, int64_t lda, const double *d_B, int64_t ldb, double *d_C, int64_t ldc);
/* the same update as the factorization makes it: only the 128 x 128 tiles of C that reach the diagonal or lie above it
 * are written (whole: their entries below the diagonal may change); tiles below them and rows >= m keep what they held */
int spp_dense_gemm_tn_sub_upper(spp_ctx *ctx, int64_t m, int64_t n, int64_t k,
	const double *d_A, int64_t lda, const double *d_B, int64_t ldb, double *d_C, int64_t ldc);
/* the partial factorization of a big front of the sparse path: F (h x h, ld, upper triangle read) is laid out with
 * pad = roundup(w, 128) - w identity rows / columns after its w pivots, as the sparse path lays out a front, and factored by
 * the same call: R11, R12 and the contribution block S = A22 - R12^T R12 (upper triangle) come back in F. d_image (may be
 * NULL) receives the padded image, hp = h + pad columns of (hp + 1) & ~1 doubles. SPP_NOT_POSDEF: a pivot of A11 failed. */
int spp_dense_front_factor(spp_ctx *ctx, double *d_F, int64_t ld, int64_t w, int64_t h, double *d_image);

const char *spp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPP_HIP_H */
