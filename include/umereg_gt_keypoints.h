/* umereg_gt_keypoints.h -- C ABI of the device-side selection of ground-truth-driven keypoints (csrc/gt_keypoints.hip): what
 * `utils.loc_utils.generate_ume_from_keypoints2(..., selection="device")` runs in place of the moment matrices of EVERY candidate, the
 * two sorts and the per-keypoint search structures of the default path.
 *
 * Same conventions as umereg.h: outputs and workspace belong to the caller, every compute entry takes a HIP stream (NULL = the
 * default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, allocates
 * nothing and never waits for the device.  The size query is host arithmetic and returns 0 for arguments the entries refuse.  The entry
 * points here are typed by their own table (umeregrobust_amd/gt_keypoints.py: GT_KEYPOINTS_SIGNATURES).
 *
 * Every output is a function of the inputs alone: same bytes in every run, whatever the workspace or the outputs held before.  No
 * word of the workspace is read that the call did not write.  The atomics of the selection (a ticket and a found-counter per batch
 * element) decide how many candidates are TESTED, never which are selected.  No kernel waits for another workgroup. */
#ifndef UMEREG_GT_KEYPOINTS_H
#define UMEREG_GT_KEYPOINTS_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest batch (one workgroup reduces the per-element candidate counts) */
#define UMEREG_GT_KEYPOINTS_MAX_B 1024
/* largest K of umereg_gt_ball_any_f32 (the ball search's limit) */
#define UMEREG_GT_BALL_ANY_MAX_K 7680
/* words per batch element of the record umereg_gt_select_f32 writes */
#define UMEREG_GT_RECORD_WORDS 2

/* bytes of workspace umereg_gt_candidates and umereg_gt_select_f32 need (the same buffer serves both, in that order);
 * 0 for B < 1, B > UMEREG_GT_KEYPOINTS_MAX_B or N < 1 */
size_t umereg_gt_keypoints_workspace_bytes(int B, int N);

/* Candidate list.  overlap_idx int64 [B][N] (the K = 1 ball query of the transformed source against the target: > -1 = overlaps),
 * non_flat uint8 [B][N] (1 = not of a flat class).  Point i of element b is a candidate iff both hold.
 * cand int32 [B][N]: the candidates of element b in DESCENDING index order, the rest of the row -1.  lengths int32 [B]: their number.
 * Three launches (count, scan, scatter: the ordered compaction of compact.h over the reversed row). */
int umereg_gt_candidates(const int64_t* overlap_idx, const uint8_t* non_flat, int B, int N, int32_t* cand, int32_t* lengths,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Selection.  packed: the search structure umereg_pack_points_f32 built for the source cloud [B][N][3] and `radius`; cand / lengths
 * as umereg_gt_candidates wrote them.  With L = min_b lengths[b] (taken on the device), hits(i) = the number of points of the cloud
 * with d2 < radius * radius (strict; the point itself counts; flags & UMEREG_BALL_FMA as in umereg_ball_query_ex_f32) and
 * dense(i) = min(hits(i), max_nn) >= min_nn:
 *     kp_index int64 [B][num_samples]: the first num_samples dense ones of the walk cand[b][L - 1], cand[b][L - 2], ... cand[b][0]
 *                                      (the reference picks dense POSITIONS in descending order), the rest of the row -1
 *     record   int32 [B][2]:           { min(#dense of cand[b][0 .. L), num_samples), lengths[b] }
 * The scan of a ball ends at its min_nn-th hit, and a worker takes no new candidate of an element once num_samples dense ones have
 * been published for it: the tested candidates are a prefix of the walk that holds the first num_samples dense ones, so the outputs
 * do not depend on how far the workers got.  tested int32 [B] (may be NULL): how many candidates were tested -- the one output that
 * depends on timing, for measurement only.  Three launches (zero the counters, test, pick). */
int umereg_gt_select_f32(const void* packed, const int32_t* cand, const int32_t* lengths, int B, int N, float radius, int max_nn,
                         int min_nn, int num_samples, int flags, int64_t* kp_index, int32_t* record, int32_t* tested,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Batched small-set existence.  q, p f32 [Bk][K][3]; hits int32 [Bk]: the number of rows of q[b] with some row of p[b] at
 * d2 < radius * radius (strict, d2 as umereg_ball_query_ex_f32 forms it for the same flags) -- the number of idx > -1 of a K = 1
 * ball query of q[b] against p[b], without a search structure per b.  1 <= K <= UMEREG_GT_BALL_ANY_MAX_K.  One launch. */
int umereg_gt_ball_any_f32(const float* q, const float* p, int Bk, int K, float radius, int flags, int32_t* hits, void* stream);

#ifdef __cplusplus
}
#endif

#endif
