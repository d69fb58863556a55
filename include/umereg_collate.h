/* umereg_collate.h -- C ABI of the device-side collate: what the reference's batch_collate_fn_dset (datasets/kitti/
 * kitti_dataset.py:546-616) does to ONE batch element once its two random dilutions are drawn -- the index gathers of both clouds
 * into the batched tensors and the correspondences that survive the dilution -- on the GPU.  The draws themselves stay the host's
 * (numpy's `choice(n, size, replace=False)`, in the reference's order); the keep lists are uploaded as they come.
 *
 * Same conventions as umereg.h: outputs and workspace belong to the caller, the compute entry takes a HIP stream (NULL = the
 * default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, returns
 * UMEREG_ENODEV where no HIP device is visible, allocates nothing and never waits for the device.  The size query is host
 * arithmetic and returns 0 for arguments the compute entry would refuse.  The entry points here are typed by their own table
 * (umeregrobust_amd/collate.py: COLLATE_SIGNATURES).
 *
 * Semantics (exact; everything is integer work or a copy, so a restatement can be compared with ==):
 *   gather    out[j] = in[keep[j]] for the points (3 floats), the labels and the transformed source points;
 *             out_coords[j] = {b, coords[keep[j]][0..2]}: MinkowskiEngine's sparse_collate layout, batch index in column 0.
 *             The entries of one keep list are distinct (a draw without replacement).
 *   matches   the two np.intersect1d(..., return_indices=True) calls of kitti_dataset.py:585-589:
 *               1. a source point keeps only its FIRST row of `matches` (file order); its later rows are dropped;
 *               2. a source point that the dilution dropped loses its row;
 *               3. of the rows left, a target point keeps the one with the LOWEST source index;
 *               4. a target point that the dilution dropped loses its row;
 *               5. rows (position of the source in keep_src, position of the target in keep_tgt), in ASCENDING TARGET INDEX
 *                  (the index before the dilution).
 *             (1 comes before 2 and 3 before 4: a source whose first target was thinned away does not fall back to its second.)
 *             m rows are written; m -> out_count[0]; m <= min(n_matches, n_src, n_tgt).
 *   out_count[1] is set to 1 if an index of `matches` lies outside [0, ns) x [0, nt) or a keep index outside its cloud: the
 *   outputs are then meaningless and the caller must refuse them.
 *
 * Two integer atomicMin passes give the minima of 1 and 3 (their result does not depend on order); row order comes from a scan
 * over the targets, never from atomics; no workspace word is read that the same call did not write: two runs give the same bytes
 * whatever the workspace held.  Rows of out_matches beyond out_count[0] are not written. */
#ifndef UMEREG_COLLATE_H
#define UMEREG_COLLATE_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workspace of one umereg_collate_element call on clouds of ns / nt points and n_matches rows; 16-byte aligned memory.  Indices
 * are 32-bit inside: 0 unless 0 < ns, nt < 2^31 and 0 <= n_matches < 2^31. */
size_t umereg_collate_workspace_bytes(int64_t ns, int64_t nt, int64_t n_matches);

/* One batch element.  All pointers are device memory.
 *   source    src_pts f32 [ns][3], src_seg i64 [ns], src_coords i32 [ns][3], src_pts_tform f32 [ns][3]
 *   target    tgt_pts f32 [nt][3], tgt_seg i64 [nt], tgt_coords i32 [nt][3]
 *   matches   i64 [n_matches][2] (source index, target index); NULL allowed when n_matches == 0
 *   keep_src  i64 [n_src] (0 < n_src <= ns), keep_tgt i64 [n_tgt] (0 < n_tgt <= nt)
 *   b         the element's batch index (column 0 of the coordinates)
 *   outputs   THIS element's slices of the batched tensors: out_src_pts f32 [n_src][3], out_src_seg i64 [n_src], out_src_coords
 *             i32 [n_src][4], out_src_pts_tform f32 [n_src][3]; out_tgt_pts f32 [n_tgt][3], out_tgt_seg i64 [n_tgt],
 *             out_tgt_coords i32 [n_tgt][4]; out_matches i64 [min(n_matches, n_src, n_tgt)][2] (NULL allowed when that is 0);
 *             out_count i32 [2].
 * A field whose input pointer is NULL is skipped, and its output pointer must be NULL too (the caller gathers such a field
 * itself: another dtype, say); the keep lists, the counts and the workspace are always needed. */
int umereg_collate_element(const float* src_pts, const int64_t* src_seg, const int32_t* src_coords, const float* src_pts_tform,
                           int64_t ns, const float* tgt_pts, const int64_t* tgt_seg, const int32_t* tgt_coords, int64_t nt,
                           const int64_t* matches, int64_t n_matches, const int64_t* keep_src, int64_t n_src,
                           const int64_t* keep_tgt, int64_t n_tgt, int b, float* out_src_pts, int64_t* out_src_seg,
                           int32_t* out_src_coords, float* out_src_pts_tform, float* out_tgt_pts, int64_t* out_tgt_seg,
                           int32_t* out_tgt_coords, int64_t* out_matches, int* out_count, void* workspace, size_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif
