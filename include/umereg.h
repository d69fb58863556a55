/*
 * umereg.h -- C ABI of the MI355X-native (gfx950) UMERegRobust registration hot path.
 *
 * The reference (yuvalH9/UMERegRobust) is pure Python: its "operator interface" for this
 * path is the function level of evaluate.py / utils/loc_utils.py / utils/eval_utils.py, with
 * the arithmetic living in un-vendored CUDA libraries (pytorch3d, torch).  Each entry point
 * below is what a ctypes/cffi binding written for that function would bind; the reference
 * statement it replaces is cited as file:line relative to the reference tree.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer (HIP global memory) unless the name ends in _host;
 *     tensors are dense, row-major, batch-first, fp32 values / int64 indices, exactly the
 *     layouts the reference's torch tensors have;
 *   - the library never allocates or frees device memory: outputs and workspaces are caller
 *     owned (size queries: *_workspace_bytes); the only mutable state is the thread-local
 *     last-error string -- options are per-call arguments (umereg_match_opts, the `flags` of the
 *     *_ex entry points), never process-wide settings;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); calls are asynchronous
 *     with respect to the host and re-entrant;
 *   - return value: UMEREG_OK (0) or a negative UMEREG_E* code; umereg_last_error() gives the
 *     text for the calling thread;
 *   - there is NO CPU fallback: without a HIP device every compute entry point returns
 *     UMEREG_ENODEV.
 */
#ifndef UMEREG_H
#define UMEREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_ABI_VERSION 2 /* 2: per-call umereg_match_opts replace the process-wide matcher setters of version 1 */
#define UMEREG_FEAT_DIM 32 /* evaluate.py:55 hard-codes 32 */

enum {
    UMEREG_OK = 0,
    UMEREG_EINVAL = -1, /* bad argument (null pointer, size, unsupported feature dim) */
    UMEREG_ENODEV = -2, /* no HIP device / wrong architecture */
    UMEREG_EWORKSPACE = -3, /* workspace too small */
    UMEREG_ELAUNCH = -4 /* HIP launch / runtime error */
};

/* Q-basis layouts written by umereg_ume_orthobasis_f32 */
enum {
    UMEREG_QLAYOUT_PLAIN = 0, /* [n,32,4] row-major, like torch.linalg.qr(...).Q */
    UMEREG_QLAYOUT_ROWS = 1,  /* MFMA A-fragment order: source side of the distance GEMM */
    UMEREG_QLAYOUT_COLS = 2,  /* MFMA B-fragment order: target side of the distance GEMM */
    /* split-f16 operands for the fast GEMM: every basis entry is stored as hi = f16(q) and
     * lo = f16(q - hi): |q| <= 1, so the pair carries q to an absolute error <= 2^-25 */
    UMEREG_QLAYOUT_ROWS_F16X2 = 3, /* source side; pads n to a multiple of 128 */
    UMEREG_QLAYOUT_COLS_F16X2 = 4  /* target side; pads n to a multiple of 32 */
};

int umereg_abi_version(void);
/* sha256 (64 hex digits) of the HIP sources, headers and compiler flags this library was compiled from; the build
 * recipe (umeregrobust_amd/_build.py) rebuilds an in-tree library whose hash differs from the tree's */
const char* umereg_build_source_hash(void);
const char* umereg_last_error(void);
/* number of visible HIP devices; fills name (may be NULL) with device 0's gcnArchName */
int umereg_device_count(char* arch_name, size_t arch_name_len);

/* Do two HIP streams of this process run SIDE BY SIDE?  (Runtime plumbing of the loops that keep several pairs in flight,
 * evaluate.py:175: the HIP runtime multiplexes streams onto a few hardware queues by a rule a caller cannot read back; two streams on
 * one queue execute one after the other.)  A spin kernel of spin_ms on stream_a, a one-thread kernel on stream_b, both timed by
 * events: *side_by_side_host = 1 if b's kernel completed while a's was still spinning.  Synchronises both streams; host outputs. */
int umereg_streams_run_side_by_side(void* stream_a, void* stream_b, float spin_ms, int* side_by_side_host, float* waited_ms_host);

/* ---------------------------------------------------------------------------------------------
 * a1  pytorch3d.ops.ball_query(p1, p2, lengths1, lengths2, K, radius, return_nn)
 *     reference call sites: evaluate.py:51, utils/loc_utils.py:38,72,100,114,167,184,383-384.
 * For every query p1[b,i] (i < lengths1[b]) the FIRST K points of p2[b] IN INDEX ORDER with
 * |p1-p2|^2 < radius^2 (strict; fp32, one rounding per operation, no FMA contraction).
 *   p1 [B,n1,3]  p2 [B,n2,3]  lengths1/lengths2 int64 [B] or NULL (= full)
 *   idx   int64 [B,n1,K]  padded with -1
 *   dists f32   [B,n1,K]  squared distances, padded with 0      (may be NULL)
 *   nn    f32   [B,n1,K,3] neighbour coordinates, padded with 0 (may be NULL; return_nn)
 * workspace: umereg_ball_query_workspace_bytes(B, n2).
 * ------------------------------------------------------------------------------------------- */
size_t umereg_ball_query_workspace_bytes(int B, int n2);
int umereg_ball_query_f32(const float* p1, const float* p2, const int64_t* lengths1,
                          const int64_t* lengths2, int B, int n1, int n2, int K, float radius,
                          int64_t* idx, float* dists, float* nn, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The same with flags.  UMEREG_BALL_FMA (opt-in): the squared distance contracted the way nvcc compiles pytorch3d's CUDA kernel
 * (`dist2 += diff * diff` under the default -fmad=true): d2 = fma(dz, dz, fma(dy, dy, dx * dx)) -- one rounding less per term than the
 * CPU kernel's ((dx dx) + (dy dy)) + (dz dz), which is the default here and what the task's "bit-exact neighbourhood indices"
 * refers to.  The reference's published numbers were produced by the CUDA build: a maintainer who has it can reproduce its
 * neighbourhoods bit for bit with this flag (the two forms differ in one neighbour of one ball in ~1e5 on off-lattice clouds). */
#define UMEREG_BALL_FMA 1
int umereg_ball_query_ex_f32(const float* p1, const float* p2, const int64_t* lengths1,
                             const int64_t* lengths2, int B, int n1, int n2, int K, float radius, int flags,
                             int64_t* idx, float* dists, float* nn, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1+a2  evaluate.my_ume_generation(pts, kpts, feat, args)            evaluate.py:50-60
 *        (the same moment matrix as ume_kp_layer.ume_mat, utils/loc_utils.py:365-372)
 * Fused ball query (K = args.ume_max_nn, radius = args.ume_r_nn) + feature gather + UME moment
 * matrix:  F = [sum f, sum f p^T] / (sum_c sum f_c + 1e-6)   ->  F f32 [B,n_kp,32,4].
 * The 960 MB gathered intermediate of the reference (evaluate.py:54-55) is never formed.
 * Moments are accumulated in fp64 (on the matrix pipe: v_mfma_f64_4x4x4_4b_f64) and rounded once to fp32.
 *   pts [B,N,3]  kpts [B,n_kp,3]  feat [B,N,32]
 *   nn_count int32 [B,n_kp]   neighbours used per keypoint (0 => F row is exactly 0)  (may be NULL)
 *   nn_idx   int64 [B,n_kp,K] the neighbourhood actually used, -1 padded              (may be NULL)
 * ------------------------------------------------------------------------------------------- */
size_t umereg_ume_moments_workspace_bytes(int B, int N);
/* layered form of the same call, so a caller can time the moment kernel alone:
 * (1) umereg_pack_points_f32 builds the search structure for `radius` in `packed` (size =
 *     umereg_ume_moments_workspace_bytes(B,N)): packed {x,y,z} table, bounding box, uniform grid
 *     with cell edge >= radius, points counting-sorted by cell (stable, deterministic);
 * (2) umereg_ume_moments_packed_f32 runs the fused search + gather + moments kernel on it (same
 *     radius). */
int umereg_pack_points_f32(const float* pts, int B, int N, float radius, void* packed,
                           size_t packed_bytes, void* stream);
int umereg_ume_moments_packed_f32(const void* packed, const float* kpts, const int64_t* kp_index,
                                  const float* feat, int B, int N, int n_kp, int feat_dim, int K,
                                  float radius, int flags, float* F, int32_t* nn_count,
                                  int64_t* nn_idx, void* stream);
/*   flags & UMEREG_MOMENTS_ORDERED: process keypoints in the cell-sorted, XCD-sliced order that
 *   umereg_ume_keypoint_order wrote into `packed` for these same keypoints (results are unchanged;
 *   only cache locality differs).  Requires n_kp <= N rounded up to 256.
 *   flags & UMEREG_MOMENTS_RAW: F = [sum f, sum f p^T] without the normaliser -- the matrix of
 *   generate_ume_from_keypoints2(normalized_ume=False), utils/loc_utils.py:160-162. */
#define UMEREG_MOMENTS_ORDERED 1
#define UMEREG_MOMENTS_RAW 2
/*   flags & UMEREG_MOMENTS_ACC_F32 (opt-in, measurement): neighbour sums in packed fp32 on keypoint-centred coordinates, the
 *   centre, slot fold, normaliser and division in fp64.  9 % faster on MI355X, but 2.6e-5 (row-relative maximum) from the fp64
 *   evaluation instead of correctly rounded (see ume_moments_kernel); the default accumulates every term in fp64. */
#define UMEREG_MOMENTS_ACC_F32 4
/*   flags & UMEREG_MOMENTS_ACC_VALU (measurement / A-B): the fp64 sums on the vector pipe (16 v_fma_f64 per lane and neighbour
 *   slot: the kernel of rounds 1-3) instead of the matrix pipe (v_mfma_f64_4x4x4_4b_f64, the default: exact fp32 x fp32 products,
 *   fp64 accumulation -- the same arithmetic in another order, bit-identical results on every input tried, 13 % faster). */
#define UMEREG_MOMENTS_ACC_VALU 8
/*   flags & UMEREG_MOMENTS_FMA_DIST (opt-in; default accumulation only): the ball search with the contracted squared distance of
 *   UMEREG_BALL_FMA (pytorch3d's CUDA kernel) instead of the uncontracted CPU form. */
#define UMEREG_MOMENTS_FMA_DIST 16
int umereg_ume_keypoint_order(void* packed, const float* kpts, const int64_t* kp_index, int B, int N,
                              int n_kp, float radius, void* stream);
/*   kp_index int64 [B,n_kp] (optional): keypoints given as indices into pts -- fuses the gathers
 *   `src_pts[0, src_inds]` of evaluate.py:201-202; when non-NULL, kpts may be NULL. */
int umereg_ume_moments_f32(const float* pts, const float* kpts, const float* feat, int B, int N,
                           int n_kp, int feat_dim, int K, float radius, float* F,
                           int32_t* nn_count, int64_t* nn_idx, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a3 (first half)  torch.linalg.qr(ume, mode='reduced').Q           utils/loc_utils.py:9,11
 * Householder orthonormal basis of each 32x4 UME matrix (LAPACK geqr2/org2r conventions,
 * computed in fp64, stored fp32).  The projector QQ^T -- all the reference uses -- is
 * invariant to QR sign conventions.
 *   ume [n,32,4] -> Q in `layout`; ROWS pads n to a multiple of 16, COLS to 32, ROWS_F16X2 to 128
 *   (padding is written as zeros): size = umereg_qbasis_bytes(n, layout).
 * ------------------------------------------------------------------------------------------- */
size_t umereg_qbasis_bytes(int n, int layout);
int umereg_ume_orthobasis_f32(const float* ume, int n, int layout, float* Q, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a3  utils.loc_utils.ume_cdist(ume1, ume2)                          utils/loc_utils.py:8-15
 * D[b,i,j] = |Q1 Q1^T - Q2 Q2^T|_F / sqrt(2), evaluated as sqrt(max(4 - |Q1^T Q2|_F^2, 0)) by
 * an fp32 MFMA GEMM over the 4-column bases (no 1024-wide projector is materialised).
 *   ume1 [B,n1,32,4]  ume2 [B,n2,32,4]  ->  D f32 [B,n1,n2]
 * ------------------------------------------------------------------------------------------- */
size_t umereg_ume_cdist_workspace_bytes(int B, int n1, int n2);
int umereg_ume_cdist_f32(const float* ume1, const float* ume2, int B, int n1, int n2, float* D,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a3+a4  D = ume_cdist(...); m = D.min(dim=-1)[1]; ume_d = D[i, m_i]   evaluate.py:215,224,234
 * Same GEMM with the row arg-min fused into the epilogue: D is never written.
 *   match_idx int64 [B,n1] (lowest index on ties), match_dist f32 [B,n1]
 * ------------------------------------------------------------------------------------------- */
size_t umereg_ume_match_workspace_bytes(int B, int n1, int n2);
/* layered form: bases already orthonormalised by umereg_ume_orthobasis_f32 (Q1 in ROWS layout,
 * Q2 in COLS layout), one batch element.  D may be NULL (no distance matrix written); match_idx
 * may be NULL (no arg-min); `keys` is n1 x 8 bytes of scratch, required when match_idx != NULL. */
int umereg_ume_dist_q_f32(const float* Q1_rows, const float* Q2_cols, int n1, int n2, float* D,
                          int64_t* match_idx, float* match_dist, void* keys, void* stream);
int umereg_ume_match_f32(const float* ume1, const float* ume2, int B, int n1, int n2,
                         int64_t* match_idx, float* match_dist, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same two calls on the f16 MFMA pipe (16x the fp32-MFMA rate): operands in the *_F16X2
 * layouts, products hi*hi + hi*lo + lo*hi accumulated in fp32 by v_mfma_f32_32x32x16_f16 --
 * an fp32-class result (operand error <= 2^-25 absolute) several times faster. */
int umereg_ume_dist_q_f16x2(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, float* D,
                            int64_t* match_idx, float* match_dist, void* keys, void* stream);
int umereg_ume_match_f16x2(const float* ume1, const float* ume2, int B, int n1, int n2,
                           int64_t* match_idx, float* match_dist, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Filter + refine matching ("f16r"): a coarse pass with the hi planes only (ONE f16 MFMA product)
 * collects, per source row, every target whose coarse score is within a proven error margin of the
 * row's best; the candidates (~15 per row) are re-evaluated in fp64 from hi+lo and the arg-min taken
 * (lowest index among candidates whose squared distances agree to fp32).  The result is the arg-min of
 * the fp64-evaluated distance over ALL targets -- deterministic, and more accurate than either scan
 * variant -- at a third of the MFMA work.
 * Operands in the *_F16X2 layouts; scratch from umereg_ume_match_q_scratch_bytes(n1, n2). */
size_t umereg_ume_match_q_scratch_bytes(int n1, int n2);
int umereg_ume_match_q_f16r(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                            int64_t* match_idx, float* match_dist, void* scratch, size_t scratch_bytes,
                            void* stream);
/* Per-call options of the filter + refine matcher (tuning, experiments, parity tests).  A NULL pointer -- and every entry
 * point without the _ex suffix -- means the defaults.  The scratch / workspace size depends on `variant` and `splits`: query it
 * with the same options (the *_bytes_ex functions).  Nothing here is process-wide: two pipelines in one process may use
 * different options concurrently.
 *   variant          0 (default) = the Q-form coarse kernel (16 basis-column products per pair, squared and summed in the
 *                    epilogue), 1 = the P-form kernel (one inner product of the packed 32 x 32 projectors per pair, K = 528; it
 *                    keeps its packed operands in the scratch).  Same results bit for bit.
 *   splits           target splits of the coarse pass (0 = automatic)
 *   share_mask       limit-sharing schedule of the coarse pass, bit k = share after tile k of a split (< 0 = default)
 *   force_exhaustive != 0: refine every block of rows exhaustively (a parity test uses it) */
typedef struct umereg_match_opts {
    int32_t variant;
    int32_t splits;
    int64_t share_mask;
    int32_t force_exhaustive;
    int32_t reserved; /* must be 0 */
} umereg_match_opts;
size_t umereg_ume_match_q_scratch_bytes_ex(int n1, int n2, const umereg_match_opts* opts);
int umereg_ume_match_q_f16r_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                               int64_t* match_idx, float* match_dist, void* scratch, size_t scratch_bytes,
                               const umereg_match_opts* opts, void* stream);

/* the stages of umereg_ume_match_q_f16r on their own (same scratch, same stream, same options, in this order): reset
 * zeroes the per-row limits (a 4 n1 byte memset at the head of the scratch, whatever the options), coarse is the MFMA
 * filter, refine the fp64 arg-min over the candidates */
int umereg_ume_match_reset_f16(void* scratch, size_t scratch_bytes, int n1, int n2, void* stream);
int umereg_ume_match_coarse_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, void* scratch,
                                size_t scratch_bytes, void* stream);
int umereg_ume_match_refine_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                const void* scratch, size_t scratch_bytes, int64_t* match_idx,
                                float* match_dist, void* stream);
int umereg_ume_match_coarse_f16_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, void* scratch,
                                   size_t scratch_bytes, const umereg_match_opts* opts, void* stream);
int umereg_ume_match_refine_f16_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                   const void* scratch, size_t scratch_bytes, int64_t* match_idx,
                                   float* match_dist, const umereg_match_opts* opts, void* stream);
int umereg_ume_match_f16r(const float* ume1, const float* ume2, int B, int n1, int n2,
                          int64_t* match_idx, float* match_dist, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t umereg_ume_match_workspace_bytes_ex(int B, int n1, int n2, const umereg_match_opts* opts);
int umereg_ume_match_f16r_ex(const float* ume1, const float* ume2, int B, int n1, int n2,
                             int64_t* match_idx, float* match_dist, void* workspace,
                             size_t workspace_bytes, const umereg_match_opts* opts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1..a5 of one registration pair in one call                          evaluate.py:206-236
 * (my_ume_generation x2, ume_cdist + arg-min + match distances, match probabilities: everything up
 * to the host RNG draw).  Pure composition of the entry points above -- same kernels, same results.
 *   pts f32 [2,N,3], feat f32 [2,N,32] (row 0 = source cloud, row 1 = target cloud),
 *   kp_index int64 [2,n_kp] keypoints as indices into their cloud (evaluate.py:199-202)
 *   -> F f32 [2,n_kp,32,4], match_idx int64 [n_kp], match_dist f32 [n_kp],
 *      prob f32 [n_kp] (NULL to skip: configs without filter_by_ume_dist_cond)
 * ------------------------------------------------------------------------------------------- */
size_t umereg_pair_match_workspace_bytes(int N, int n_kp);
int umereg_pair_match_f32(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                          float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                          float* prob, void* workspace, size_t workspace_bytes, void* stream);
/* the same with explicit matcher options (workspace from umereg_pair_match_workspace_bytes_ex with the same options) */
size_t umereg_pair_match_workspace_bytes_ex(int N, int n_kp, const umereg_match_opts* opts);
int umereg_pair_match_ex_f32(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                             float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                             float* prob, void* workspace, size_t workspace_bytes, const umereg_match_opts* opts,
                             void* stream);

/* The same for a pair whose clouds DIFFER in size and live in separate buffers -- the shape real data has: the reference's
 * collate dilutes source and target independently (datasets/kitti/kitti_dataset.py:568-569: src_num_pts = min(len(src),
 * max_pc_size), tgt_num_pts = min(len(tgt), max_pc_size)), the loop takes num_init_sel = min(10000, N_src, N_tgt) keypoints from
 * each (evaluate.py:195-204).  So N_src != N_tgt, both varying from pair to pair, with ONE keypoint count n_kp.
 *   src_pts f32 [N_src,3], tgt_pts f32 [N_tgt,3], src_feat f32 [N_src,32], tgt_feat f32 [N_tgt,32] (16-byte aligned),
 *   src_kp / tgt_kp int64 [n_kp]: keypoints as indices into their own cloud
 *   -> F f32 [2,n_kp,32,4] (row 0 = source), match_idx, match_dist, prob as in umereg_pair_match_f32.
 * Nothing is copied or stacked: the kernels read each cloud where it lies, through a 64-byte device record at the tail of the
 * workspace.  Results are those of the per-cloud calls, bit for bit.
 * workspace: umereg_pair_match_workspace_bytes_ex(max(N_src, N_tgt), n_kp, opts). */
int umereg_pair_match_ragged_f32(const float* src_pts, const float* tgt_pts, const float* src_feat, const float* tgt_feat,
                                 const int64_t* src_kp, const int64_t* tgt_kp, int N_src, int N_tgt, int n_kp, int K,
                                 float radius, float tau, float* F, int64_t* match_idx, float* match_dist, float* prob,
                                 void* workspace, size_t workspace_bytes, const umereg_match_opts* opts, void* stream);

/* The same chain as ONE executable hipGraph, for callers that process many pairs out of the same buffers (an evaluation
 * loop with resident or double-buffered inputs): captured once on `stream` (a non-default stream; nothing is executed by
 * the capture), replayed with a single launch per pair -- ~0.015 ms of host time instead of ~0.10 ms for the 12
 * launches.  The handle owns only the graph: every buffer (inputs, outputs, workspace) stays the caller's and must stay
 * at the same address with the same contents contract as in umereg_pair_match_f32 while the handle is used.  Launching
 * on any stream is allowed; launches of one handle must not overlap (they share the workspace). */
int umereg_pair_match_graph_create(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                   float radius, float tau, float* F, int64_t* match_idx, float* match_dist, float* prob,
                                   void* workspace, size_t workspace_bytes, void* stream, void** graph_out);
int umereg_pair_match_graph_create_ex(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                      float radius, float tau, float* F, int64_t* match_idx, float* match_dist, float* prob,
                                      void* workspace, size_t workspace_bytes, const umereg_match_opts* opts, void* stream,
                                      void** graph_out);
/* Both replays below are for a graph over fixed buffers.  On a handle made by umereg_pair_match_graph_create_cap they
 * return UMEREG_EINVAL and launch nothing (the captured kernels read their clouds through a record that only
 * umereg_pair_match_graph_launch_ragged writes): replay a capacity graph with that entry. */
int umereg_pair_match_graph_launch(void* graph, void* stream);
/* Replay + the device -> host copy of the match probabilities (the operand of the host draw, evaluate.py:238; prob_host:
 * pinned host memory, n_kp floats, or NULL) in one call. */
int umereg_pair_match_graph_launch_ex(void* graph, float* prob_host, void* stream);
/* Replay for ANOTHER pair of the same shape -- the loop of evaluate.py:175 runs over distinct pairs: pts [2,N,3], feat [2,N,32],
 * kp_index [2,n_kp] of the new pair (device pointers) are first copied device to device into the buffers the graph was captured
 * over (which must therefore be the caller's to overwrite: a pipeline slot's persistent staging buffers), then the graph is
 * replayed and the probabilities downloaded as in _launch_ex.  NULL, or the captured pointer itself, skips that copy. */
int umereg_pair_match_graph_launch_from(void* graph, const float* pts, const float* feat, const int64_t* kp_index,
                                        float* prob_host, void* stream);
/* ONE graph for every pair that fits a capacity (the loop of evaluate.py:175 over pairs of varying size): the chain is captured
 * with its kernels reading the clouds through the device record in the workspace, sized for clouds of up to N_cap points.
 * umereg_pair_match_graph_launch_ragged replays it for ANY pair with N_src, N_tgt <= N_cap (arguments as in
 * umereg_pair_match_ragged_f32): the record is rewritten by a one-thread kernel on `stream`, then the graph is launched and the
 * probabilities downloaded as in _launch_ex.  A change of shape therefore costs a 64-byte record -- no staging copy of the
 * clouds, no re-capture.  Baked in: N_cap, n_kp (10 000 for every pair of the KITTI benchmarks), K, radius, tau, the options.
 * workspace (caller-owned, as are F / match_idx / match_dist / prob): umereg_pair_match_workspace_bytes_ex(N_cap, n_kp, opts).
 * The clouds of a launch must stay valid until that launch has completed. */
int umereg_pair_match_graph_create_cap(int N_cap, int n_kp, int K, float radius, float tau, float* F, int64_t* match_idx,
                                       float* match_dist, float* prob, void* workspace, size_t workspace_bytes,
                                       const umereg_match_opts* opts, void* stream, void** graph_out);
int umereg_pair_match_graph_launch_ragged(void* graph, const float* src_pts, const float* tgt_pts, const float* src_feat,
                                          const float* tgt_feat, const int64_t* src_kp, const int64_t* tgt_kp, int N_src,
                                          int N_tgt, float* prob_host, void* stream);
/* The continuation after the host draw (evaluate.py:238-254): upload the kept match indices (cond_host int64 [n_cond], pinned
 * host memory; NULL = every match) and solve one SE(3) per kept match from the graph's own outputs:
 * T_out[k] from (F_src[cond[k]], F_tgt[match[cond[k]]]).  cond_dev int64 [n_cond], T_out f32 [n_cond,4,4]: device buffers. */
int umereg_pair_match_graph_solve(void* graph, const int64_t* cond_host, int n_cond, int64_t* cond_dev, float* T_out,
                                  void* stream);
int umereg_pair_match_graph_destroy(void* graph);

/* ---------------------------------------------------------------------------------------------
 * a5  a = exp((1 - ume_d)/tau); prob = a / a.sum()                   evaluate.py:235-236
 *   ume_d f32 [n] -> prob f32 [n].  (The draw itself, np.random.choice(..., p=prob) at
 *   evaluate.py:238, consumes the HOST numpy RNG and stays on the host.)
 * ------------------------------------------------------------------------------------------- */
int umereg_match_prob_f32(const float* ume_d, int n, float tau, float* prob, void* stream);

/* HOST helper (host pointers, no device work) for the draw itself -- evaluate.py:238,
 * np.random.choice(n, size, replace=False, p=prob): one round of numpy's legacy weighted
 * sampling-without-replacement algorithm, bit-identical to numpy given the same uniforms (which the
 * caller keeps drawing from its RandomState).  See csrc/api.hip for the argument contract. */
int umereg_host_choice_round(double* p_host, int n, const double* x_host, int k, int64_t* found_host,
                             int n_uniq, double* cdf_scratch_host, unsigned char* seen_scratch_host);
/* numpy's pre-draw argument checks in one pass: out[0] = Kahan sum, out[1] = #(p > 0), out[2] = any NaN/negative */
int umereg_host_choice_check(const double* p_host, int n, double* out3_host);
/* the whole draw in one call: numpy's legacy RandomState is MT19937, so given its state
 * (RandomState.get_state(): key[624], pos) the uniforms are generated here exactly as random_sample()
 * would and the advanced state is handed back (set_state) -- indices, order and the RNG stream stay
 * bit-identical to np.random.choice.  p: f32 or f64 [n]; work: 2n + size doubles; seen: n bytes.
 * returns 0, or 1 / 2 / 3 for numpy's argument errors (NaN or negative entries / sum != 1 / fewer
 * non-zero entries than size), -1 for bad arguments. */
int umereg_host_choice_mt19937(uint32_t* mt_key_host, int* mt_pos_host, const void* p_host, int p_is_f32, int n,
                               int size, int64_t* found_host, double* work_host, unsigned char* seen_host,
                               int* rounds_out_host);

/* np.random.choice(n, size, replace=False) without p -- the keypoint draws of evaluate.py:199-200 and the correlation
 * sub-sampling of :280, :284 -- on the caller's MT19937 state (numpy's legacy RandomState): permutation(n)[:size] by
 * numpy's own shuffle (legacy random_interval, 32-bit words).  Bit-identical indices and generator state.
 *   mt_key uint32[624], mt_pos: the generator state (BitGenerator.ctypes.state_address); perm: int64 [n] scratch;
 *   out: int64 [size].  Host-only: runs without a device. */
int umereg_host_permutation_mt19937(uint32_t* mt_key, int* mt_pos, int64_t n, int64_t size, int64_t* perm, int64_t* out);

/* ---------------------------------------------------------------------------------------------
 * f1 (raw-cloud prep)  ME.utils.sparse_quantize(coordinates, return_index=True, quantization_size)
 *                      evaluate.py:261-264, datasets/kitti/kitti_dataset.py:416-419
 * One representative per occupied voxel of edge `voxel`: the FIRST point (lowest index) of every voxel
 * floor(p / voxel), indices ascending (MinkowskiEngine 0.5.4 not installable: restated, parity unpinned).
 *   pts [n,3] f32; out_idx int64 [n] (the first out_count[0] entries are written);
 *   out_count int32 [2] (device): [0] = number of voxels, [1] != 0 if a coordinate was NaN / inf / outside
 *   |floor(p / voxel)| < 2^20 (such points are left out; callers should treat it as an error).
 * Asynchronous like every entry point: read out_count after synchronising the stream. */
size_t umereg_voxel_first_index_workspace_bytes(int n);
int umereg_voxel_first_index_f32(const float* pts, int n, float voxel, int64_t* out_idx, int* out_count, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a6  utils.loc_utils.batch_estimate_transform_ume_old(G, H)         utils/loc_utils.py:292-350
 * Closed-form SE(3) from a (source G, target H) UME pair; T maps source -> target.
 *   G_all [nG,32,4], H_all [nH,32,4]; g_index/h_index int64 [n] select the rows used by
 *   hypothesis k (NULL = identity), which fuses the gathers of evaluate.py:230-231,243-244;
 *   h_of_g int64 [nG] (optional, instead of h_index): the match table m[:,1] of evaluate.py:224,
 *   hypothesis k then pairs G row g = g_index[k] with H row h_of_g[g];
 *   T f32 [n,4,4];  dist f32 [n] = 0.707 |P_H - P_G|_F (utils/loc_utils.py:338-344; NULL to
 *   skip -- every live caller discards it).
 * ------------------------------------------------------------------------------------------- */
int umereg_rtume_solve_f32(const float* G_all, const float* H_all, const int64_t* g_index,
                           const int64_t* h_index, const int64_t* h_of_g, int nG, int nH, int n,
                           float* T, float* dist, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a7  utils.eval_utils.relative_rotation_error(R, R_hat)             utils/eval_utils.py:60-76
 *   R, R_hat f32 [b,3,3] -> degrees f32 [b]; the trace is clamped as torch.clamp does: a NaN stays NaN
 * ------------------------------------------------------------------------------------------- */
int umereg_rre_deg_f32(const float* R, const float* R_hat, int b, float* out_deg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a7 + the recall gates of evaluate.py:304-305, batched over hypotheses and kept on the device:
 * rre[k] = relative_rotation_error(T[k][:3,:3], gt[:3,:3]) (utils/eval_utils.py:60-76),
 * rte[k] = |T[k][:3,3] - gt[:3,3]| (evaluate.py:43), and
 *   counts[0] += n
 *   counts[1] += #(rre <= 1.5 deg & rte <= 0.6 m)   "N.P" as coded   (evaluate.py:304)
 *   counts[2] += #(rre <= 1.5 deg & rte <= 0.3 m)   "N.P" as the README states it
 *   counts[3] += #(rre <= 1   deg & rte <= 0.1 m)   "S.P"            (evaluate.py:305)
 * counts: uint64 [4], caller-initialised, accumulated with integer atomics (order-independent).
 *   T f32 [n,4,4], gt_tform f32 [4,4]; rre_deg / rte f32 [n] optional outputs.
 *   A row with a NaN trace reports rre_deg = NaN (never 180) and passes no gate: it counts in counts[0] only.
 * ------------------------------------------------------------------------------------------- */
int umereg_hypothesis_gates_f32(const float* T, const float* gt_tform, int n, uint64_t* counts,
                                float* rre_deg, float* rte, void* stream);

/* =============================================================================================
 * hypothesis selection (FeatureCorrelator, utils/loc_utils.py:579-681)
 * ============================================================================================= */

/* pytorch3d.ops.knn_points(p1, p2, K)   -- utils/loc_utils.py:580,623; evaluate.py:272,274
 * Exact K nearest points of p2[b] for every p1[b,i]: squared distances ascending, ties towards the
 * lower index (upstream leaves tie order unspecified).  K <= min(64, n2).
 *   p1 [B,n1,3]  p2 [B,n2,3]  ->  dists f32 [B,n1,K], idx int64 [B,n1,K]
 * K >= 2 runs one query per lane with a candidate list of K + 6 keys per lane in LDS.  Two things change with the sizes, the
 * results do not: the list holds 16-bit target indices up to n2 = 65 536 and 32-bit ones from 65 537 on (another instance of
 * the kernel), and with 32-bit indices a wavefront's list is (K + 6) * 512 bytes, so the workgroup has four wavefronts up to
 * K = 26, two up to K = 58 (exactly 64 KiB of dynamic LDS at K = 58) and a single one from K = 59 on.  Queries are taken in the
 * target grid's cell order while n1 <= n2 rounded up to a multiple of 256, in the caller's order beyond. */
size_t umereg_knn_workspace_bytes(int B, int n2);
int umereg_knn_points_f32(const float* p1, const float* p2, int B, int n1, int n2, int K, float* dists,
                          int64_t* idx, void* workspace, size_t workspace_bytes, void* stream);

/* The K = 1 feature transfer of BOTH clouds of a pair in one pass -- evaluate.py:272-275:
 *   knn_points(src_pts_raw, src_pts, K=1) and knn_points(tgt_pts_raw, tgt_pts, K=1)
 * Four clouds of four sizes on a real pair (the collate dilutes source and target independently, datasets/kitti/kitti_dataset.py:
 * 568-569; the voxel thinning keeps what it keeps): q_src [nq_src,3] searches p_src [n_src,3], q_tgt [nq_tgt,3] searches p_tgt
 * [n_tgt,3]; idx_* int64 [nq_*] (the nearest point, lower index on ties: umereg_knn_points_f32 with K = 1), dist_* f32 [nq_*]
 * squared distances (may be NULL).  One structure build and one query launch for both clouds. */
size_t umereg_nn1_pair_workspace_bytes(int n_src, int n_tgt);
int umereg_nn1_pair_f32(const float* q_src, const float* q_tgt, const float* p_src, const float* p_tgt, int nq_src, int nq_tgt,
                        int n_src, int n_tgt, int64_t* idx_src, int64_t* idx_tgt, float* dist_src, float* dist_tgt,
                        void* workspace, size_t workspace_bytes, void* stream);

/* feature_spatial_var(pts, feat, knn)   -- utils/loc_utils.py:579-585
 * out[b,i] = mean over the knn-1 nearest OTHER points j of |feat[b,i] - feat[b,j]|_2 (self-kNN,
 * idx[:, :, 1:]); fused kNN + gather + norm, nothing of size [N,knn,32] is formed.
 *   pts [B,N,3], feat [B,N,32] -> out f32 [B,N]; workspace: umereg_knn_workspace_bytes(B, N)
 * 2 <= knn <= min(64, N).  Up to N = 32 768 one wavefront serves a query; larger clouds run umereg_knn_points_f32's
 * one-query-per-lane search on themselves, with its switches: 16-bit list indices up to N = 65 536 and 32-bit ones from
 * 65 537 on, one wavefront per workgroup from knn = 59 on with 32-bit indices, and 32 instead of 64 queries per wavefront
 * while N <= 65 472.  The neighbours are the same whichever kernel runs; the two kernels sum them in different orders. */
int umereg_feature_spatial_var_f32(const float* pts, const float* feat, int B, int N, int feat_dim, int knn,
                                   float* out, void* workspace, size_t workspace_bytes, void* stream);

/* weighted features of feature_corr_hypothesis_test -- utils/loc_utils.py:661,664-665
 *   m = mean over the points of BOTH clouds;  out = (feat - m) * weight[:, None]
 * workspace >= 16 KiB (partial column sums, reduced in a fixed order). */
int umereg_corr_weighted_features_f32(const float* src_feat, const float* tgt_feat, const float* src_w,
                                      const float* tgt_w, int Ns, int Nt, float* src_out, float* tgt_out,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* pc_corr_cost_pytorch3d for all hypotheses -- utils/loc_utils.py:592-637
 *   score[h] = (1/Ns) sum_n sum_{k<K} cauchy(|R_h p_n + t_h - q_jk|, sigma) <src_wfeat[n], tgt_wfeat[jk]>
 * with jk the K nearest target points of the transformed source point and
 * cauchy(e, s) = 1 / (1 + (e/s)^2).  Fused transform + exact kNN + correlation; the reference's
 * [batch,Ns,K,32] gathered tensor is never formed.
 *   src_pts [Ns,3], tgt_pts [Nt,3], src_wfeat [Ns,32], tgt_wfeat [Nt,32], T [M,4,4] -> scores f32 [M] */
size_t umereg_corr_workspace_bytes(int Ns, int Nt, int M);
int umereg_corr_scores_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                           const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                           float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* The same with an explicit choice of the search structure (tuning / tests; results are the same sets of K
 * neighbours either way).  By default jobs of >= 2^17 queries (M x Ns) into <= 65 471 target points build a
 * per-cell candidate lattice on the target once and stream every query's cell list; smaller jobs walk the grid.
 *   UMEREG_CORR_NO_LATTICE     always walk the grid
 *   UMEREG_CORR_FORCE_LATTICE  build the lattice whatever the job size (still needs <= 65 471 target points)
 * The workspace size depends on the flags: query it with the same ones.
 *   UMEREG_CORR_NO_CONSENSUS   skip the consensus pass (by default, with the lattice on and M >= 256, every source
 *                              point first scores all hypotheses whose image of it lies near the image under the
 *                              median hypothesis from ONE staged set of target points; the rest goes to the lattice)
 *   UMEREG_CORR_FORCE_CONSENSUS  run it whatever M (needs the lattice: combine with FORCE_LATTICE on small jobs)
 *   UMEREG_CORR_NO_FLAT        serve the queries neither pass could (one wavefront per query) record by record instead of
 *                              as a flat list (the round-2 start form; bit-identical sums) */
#define UMEREG_CORR_NO_LATTICE 1
#define UMEREG_CORR_FORCE_LATTICE 2
#define UMEREG_CORR_NO_CONSENSUS 4
#define UMEREG_CORR_FORCE_CONSENSUS 8
#define UMEREG_CORR_NO_FLAT 16
#define UMEREG_CORR_CONSENSUS_V1 32 /* the consensus pass in its first form (round 2: K + 6 entry lists, images in empty regions give up) */
#define UMEREG_CORR_DEBUG_STATS 64  /* the consensus pass counts into workspace header words 16..23, 28, 29: staged near / far source points,
                                       staged target points, rank-counting steps and their zone sizes, histogram steps and their zone sizes,
                                       zoomed steps, candidate slots visited per lane by either kind of step (ops.corr_scores_profile) */
#define UMEREG_CORR_FAR_MARGIN_SHIFT 8 /* bits 8..15: margin of the stage of an image in an empty region, in eighths of a grid cell
                                          (0 = default, 255 = such source points are left to the lattice) */
#define UMEREG_CORR_SRC_ROWS 128 /* source points processed in row-major cell order (round 2) instead of Hilbert-curve order */
#define UMEREG_CORR_RECORD_STAGE (1 << 18) /* (experimental) the queries neither pass serves first go one wavefront per RECORD over a staged candidate set; what that cannot serve goes one wavefront per query as before */
#define UMEREG_CORR_LEFT_COOP (1 << 16)    /* what the consensus pass leaves goes to the one-wavefront-per-query search whatever its size */
#define UMEREG_CORR_LEFT_LATTICE (1 << 17) /* ... to the candidate lattice whatever its size (by default the count decides) */
#define UMEREG_CORR_CELL_PASS (1 << 19)    /* the cell pass (leftovers sorted by lattice cell, one wavefront per cell) also on jobs below 2^25 queries (tests, tuning) */
#define UMEREG_CORR_NO_CELL_PASS (1 << 20) /* never (the round-3-start path: list kernel + one wavefront per query) */
#define UMEREG_CORR_BOUND_OUTSIDE (1 << 21) /* arg-max mode: a listed query whose image lies outside the candidate lattice (beyond its margin around the target's bounding
                                               box: max(20 % of the x/y extent, 3 m) in x / y, max(6 %, 3 m) in z) is BOUNDED by its distance dB to that box (K w(dist to the box) |vp| max|vq|) instead of searched,
                                               and so is (round 4) a listed query of the one-wavefront-per-query search with no target point within 2.5 sigma of its image (dB = the
                                               smallest distance to a 64-point chunk box of the target, known before anything is scanned); hypotheses whose score + bound reaches the best
                                               score - bound get those queries computed exactly in a second pass.  scores[h] is then exact for every hypothesis that can be the
                                               arg-max; for the others it lacks the bounded terms (it is within the bound of the exact score, and the exact score is below the
                                               arg-max's): umereg_corr_select_best_f32 returns the same hypothesis */
/* The workspace depends on the flags (the cell pass's entry buffer, the bound's slack): query it with the flags of the call.  On jobs
 * of >= 2^25 queries (M x Ns), and with UMEREG_CORR_BOUND_OUTSIDE from 2^24 on, the cell pass is on by default: its entry buffer holds min(M x Ns, 2^26) entries of 8 bytes, the flat
 * one-wavefront-per-query list half the job's queries at 8 bytes each. */
size_t umereg_corr_workspace_bytes_ex(int Ns, int Nt, int M, int flags);
int umereg_corr_scores_ex_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                              const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                              int flags, float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* The same call with its stages timed by HIP events on the launch stream (measurement; it synchronises the stream):
 * stage_ms_host[0..5] = milliseconds of  structures + hypothesis orders | consensus pass (+ leftover queue) | lattice build + cell pass |
 * list kernel | one-wavefront-per-query / per-record leftovers | reduction,   stage_ms_host[6] = the whole call.
 * A stage the configuration skips reads 0. */
int umereg_corr_scores_profile_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                                   const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                                   int flags, float* scores, void* workspace, size_t workspace_bytes, void* stream,
                                   float* stage_ms_host);

/* FeatureCorrelator's pick (utils/loc_utils.py:676-680: argsort by score, the n_hypotheses best, the best of those =
 * the arg-max): T_best f32 [4,4] = T[argmax scores] (lowest index among equal scores; a NaN score wins, the lowest-indexed one --
 * torch.argsort(descending=True) and torch.argmax order NaN above every number, so the reference picks a NaN-scored hypothesis too),
 * best_index int64 [1] (optional).  Everything stays on the device: no host read of the index. */
int umereg_corr_select_best_f32(const float* scores, const float* T, int M, float* T_best, int64_t* best_index, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f3  torch.linalg.svdvals(ume)                                       utils/eval_utils.py:31-32
 * Singular values (descending) of each 32x4 UME matrix, one-sided Jacobi in fp64.
 *   ume f32 [n,32,4] -> sv f32 [n,4]
 * ------------------------------------------------------------------------------------------- */
int umereg_ume_svdvals_f32(const float* ume, int n, float* sv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f2  o3d.pipelines.registration.registration_icp(src, tgt, max_dist, T_init,
 *         TransformationEstimationPointToPoint(), ICPConvergenceCriteria(max_iteration=...))
 *                                                                     evaluate.py:93-96
 * Point-to-point ICP: per iteration every source point (transformed in fp64) takes its exact nearest
 * target point (ties -> lower index) if closer than max_correspondence_distance; update = Umeyama
 * without scaling on the correspondences; stops like open3d (|d fitness| < relative_fitness and
 * |d inlier_rmse| < relative_rmse, or max_iteration updates).  open3d's defaults: 1e-6, 1e-6, 30.
 *   src f32 [n_src,3], tgt f32 [n_tgt,3] on the device; T_init / T_out: HOST double[16], row major;
 *   fitness, inlier_rmse, iterations: HOST outputs (NULL to skip).  Synchronous w.r.t. `stream`.
 * ------------------------------------------------------------------------------------------- */
size_t umereg_icp_workspace_bytes(int n_src, int n_tgt);
int umereg_icp_point_to_point_f32(const float* src, const float* tgt, int n_src, int n_tgt,
                                  const double* T_init_host, float max_correspondence_distance,
                                  int max_iteration, double relative_fitness, double relative_rmse,
                                  double* T_out_host, double* fitness_host, double* inlier_rmse_host,
                                  int* iterations_host, void* workspace, size_t workspace_bytes, void* stream);
/* The same from an initial transform that lives on the DEVICE (T_init_dev f32 [4,4], row major) -- the hypothesis
 * umereg_corr_select_best_f32 wrote: it is read by the first kernel when that runs, so the ICP chain is enqueued behind the
 * selection with no host read of the hypothesis in between (evaluate.py:63-96 reads R_hat / t_hat back first). */
int umereg_icp_point_to_point_dev_f32(const float* src, const float* tgt, int n_src, int n_tgt,
                                      const float* T_init_dev, float max_correspondence_distance,
                                      int max_iteration, double relative_fitness, double relative_rmse,
                                      double* T_out_host, double* fitness_host, double* inlier_rmse_host,
                                      int* iterations_host, void* workspace, size_t workspace_bytes, void* stream);
/* The same in pieces that never wait, for a loop that keeps several pairs in flight (evaluate.py:301 refines after the loop: nothing
 * on the host needs a refined transform before the metrics).  umereg_icp_enqueue_f32 enqueues [first != 0: the target's search grid
 * and the initial state from T_init_dev] + `iterations` evaluation / update pairs (the stop test lives on the device: iterations
 * beyond it find the flag set and return) + an asynchronous copy of the state to state_host (umereg_icp_state_bytes() bytes of
 * PINNED host memory) and returns.  Once the caller has waited for the stream (an event recorded behind the call),
 * umereg_icp_state_decode reads that copy: *done_host = 0 means "enqueue more" (first = 0, same workspace, untouched in between). */
size_t umereg_icp_state_bytes(void);
int umereg_icp_enqueue_f32(const float* src, const float* tgt, int n_src, int n_tgt, const float* T_init_dev,
                           float max_correspondence_distance, int max_iteration, double relative_fitness,
                           double relative_rmse, int first, int iterations, void* state_host, void* workspace,
                           size_t workspace_bytes, void* stream);
int umereg_icp_state_decode(const void* state_host, double* T_out_host, double* fitness_host, double* inlier_rmse_host,
                            int* iterations_host, int* done_host);

#ifdef __cplusplus
}
#endif
#endif /* UMEREG_H */
