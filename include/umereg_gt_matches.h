/* umereg_gt_matches.h -- C ABI of the ground-truth correspondences of a training pair: the reference's
 * one_side_ball_query_matches / mutual_ball_query_matches (utils/general_utils.py:38-59; a scipy KDTree there) on the GPU.
 *
 * Same conventions as umereg.h: outputs and workspace belong to the caller, every compute entry point takes a HIP stream
 * (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a
 * device, returns UMEREG_ENODEV where no HIP device is visible, allocates nothing and never waits for the device.  The size
 * query is host arithmetic and returns 0 for arguments the compute entries would refuse.  The entry points here are typed by
 * their own table (umeregrobust_amd/gt_matches.py: GT_MATCH_SIGNATURES).
 *
 * Semantics (exact, so that a restatement can be compared with ==):
 *   query     q_i = ((x * R[:,0] + y * R[:,1]) + z * R[:,2]) + t in fp32, in this order, no fused multiply-add; R = T[:3,:3],
 *             t = T[:3,3] of the row-major 4 x 4 fp32 matrix T (device memory).  T == NULL: the queries are used as given.
 *   distance  d2(i,j) = dx*dx + dy*dy + dz*dz, left to right, in fp64 on the fp32 values widened to double.
 *   match     j* = argmin_j d2(i,j), the lower j on an exact tie; kept iff d2(i,j*) < radius * radius (double, strict).
 *   one side  rows (i, j*) as int64 [m][2], i ascending; m -> out_count[0].
 *   mutual    the one-side rows of src -> tgt under T that the one-side rows of tgt -> src under T_inv hold as (j*, i);
 *             same order.  T_inv is the caller's (the reference forms it with torch.linalg.inv).
 * out_count[1] is set to 1 if a coordinate of either cloud (or a transformed query) is NaN or infinite, or a TARGET coordinate
 * lies beyond 2^20 m from the origin: the rows are then meaningless and the caller must refuse them.  A finite query that is
 * far from every target (outside the grid's box, in an empty cell, 1e4 m away) simply has no row.
 *
 * The search structure is the uniform grid of the ball search, built over the targets; a query visits only the cells its
 * radius can reach.  Row order comes from a scan, never from atomics; no workspace word is read that the same call did not
 * write: two runs give the same bytes whatever the workspace held. */
#ifndef UMEREG_GT_MATCHES_H
#define UMEREG_GT_MATCHES_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a target coordinate beyond this (metres) is refused through out_count[1] */
#define UMEREG_GT_MATCHES_MAX_COORD 1048576.0f

/* workspace of one call (mutual != 0: of umereg_gt_matches_mutual_f32); 16-byte aligned memory */
size_t umereg_gt_matches_workspace_bytes(int n_src, int n_tgt, int mutual);

/* src f32 [n_src][3], tgt f32 [n_tgt][3], T f32 [4][4] or NULL (all device memory); out_rows int64 [n_src][2] (the first
 * out_count[0] rows are written), out_count int32 [2] */
int umereg_gt_matches_one_side_f32(const float* src, int n_src, const float* tgt, int n_tgt, const float* T, double radius,
                                   int64_t* out_rows, int* out_count, void* workspace, size_t workspace_bytes, void* stream);

int umereg_gt_matches_mutual_f32(const float* src, int n_src, const float* tgt, int n_tgt, const float* T, const float* T_inv,
                                 double radius, int64_t* out_rows, int* out_count, void* workspace, size_t workspace_bytes,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif
