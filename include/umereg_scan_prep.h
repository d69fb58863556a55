/* umereg_scan_prep.h -- C ABI of the scan preparation: what the reference does to ONE raw lidar scan between reading it and
 * "Voxlize point clouds" (datasets/kitti/kitti_dataset.py:300-314, :407-413; datasets/nuscenes/nuscenes_dataset.py:403-421), on the
 * GPU -- the semantic half of the label word, the learning map, the ego-vehicle box, the unlabelled mask, and the compaction of what
 * is left, in scan order.
 *
 * Same conventions as umereg_collate.h: outputs and workspace belong to the caller, the compute entry takes a HIP stream (NULL =
 * the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device,
 * returns UMEREG_ENODEV where no HIP device is visible, allocates nothing and never waits for the device.  The size query is host
 * arithmetic and returns 0 for arguments the compute entry would refuse.  The entry points here are typed by their own table
 * (umeregrobust_amd/raw_scan.py: SCAN_PREP_SIGNATURES).
 *
 * Semantics (exact; integer work, comparisons and copies, so a restatement can be compared with ==).  For scan row i:
 *   sem    = labels ? labels[i] : 1;   with UMEREG_SCAN_SEM16: sem &= 0xFFFF            (SemLaserScan.set_label, :262)
 *   seg    = lut ? lut[sem] : sem                                                       (CFG['learning_map'][l], :312)
 *            a key sem >= n_lut sets UMEREG_SCAN_ERR_KEY_RANGE, an entry lut[sem] < 0 sets UMEREG_SCAN_ERR_KEY_UNMAPPED (the
 *            reference raises KeyError): on EVERY row, dropped or not, as the reference maps all labels before it masks any point
 *   ego    = ego_hx > 0 && ego_hy > 0 && |x| <= ego_hx && |y| <= ego_hy                 (inclusive, nuscenes_dataset.py:404; a NaN
 *            coordinate fails the comparison, so the point is not an ego point)
 *   keep   = !ego && (seg != 0 || UMEREG_SCAN_KEEP_UNLABELED)
 * The kept rows come out in ascending i: out_pts[r] = scan[i][0..2] (the bytes, untouched), out_seg[r] = seg, out_index[r] = i.
 * out_count = {number of kept rows, error bits}.  With an error bit set the outputs are meaningless and the caller must refuse
 * them.  Rows of the outputs beyond the count are not written.
 *
 * Three launches: per-block keep counts and error bits, one block scanning the counts, a scatter with an in-block prefix.  Row
 * order comes from the scan, never from atomics; no workspace word is read that the same call did not write: two runs give the
 * same bytes whatever the workspace held. */
#ifndef UMEREG_SCAN_PREP_H
#define UMEREG_SCAN_PREP_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags */
#define UMEREG_SCAN_SEM16 1          /* the semantic label is the low 16 bits of the word; the instance half is dropped */
#define UMEREG_SCAN_KEEP_UNLABELED 2 /* do not drop rows whose mapped label is 0 */

/* error bits of out_count[1] */
#define UMEREG_SCAN_ERR_KEY_RANGE 1    /* a label key >= n_lut */
#define UMEREG_SCAN_ERR_KEY_UNMAPPED 2 /* a label key whose entry in the map is negative (no such key) */

/* rows one workgroup compacts (one per thread); the size of the workspace and the edge sizes of the tests follow from it */
#define UMEREG_SCAN_PREP_BLOCK 1024

/* workspace of one umereg_scan_prep_f32 call on a scan of n rows; 16-byte aligned memory.  0 unless 0 < n < 2^31. */
size_t umereg_scan_prep_workspace_bytes(int64_t n);

/* One scan.  All pointers are device memory.
 *   scan       f32 [n][stride], stride 3 or 4; the first three floats of a row are x, y, z (a KITTI .bin row is x, y, z, remission)
 *   labels     u32 [n], or NULL: every row has label 1 (load_nuscenes_point_cloud without a label file, nuscenes_dataset.py:310)
 *   flags      UMEREG_SCAN_* bits
 *   lut        i32 [n_lut], or NULL with n_lut == 0 for the identity
 *   ego_hx/hy  half extents of the ego box in x and y; either <= 0 switches the filter off
 *   outputs    out_pts f32 [n][3], out_seg i64 [n], out_index i64 [n] (NULL allowed), out_count i32 [2] */
int umereg_scan_prep_f32(const float* scan, int64_t n, int stride, const uint32_t* labels, int flags, const int32_t* lut,
                         int64_t n_lut, float ego_hx, float ego_hy, float* out_pts, int64_t* out_seg, int64_t* out_index,
                         int* out_count, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
