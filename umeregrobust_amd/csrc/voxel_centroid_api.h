/* voxel_centroid_api.h -- C entry points of the voxel-centroid downsampling (csrc/voxel_centroid.hip): open3d's voxel_down_sample, one
 * centroid per occupied voxel, the coarse levels of ops.icp_multi_scale.  A private header: typed by umeregrobust_amd/icp_multiscale.py
 * (VOXEL_CENTROID_SIGNATURES, through _lib.load_typed), not under include/.
 *
 * Conventions of umereg.h: outputs and workspace belong to the caller, the compute entry takes a HIP stream (NULL = the default stream),
 * returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, allocates nothing, waits for
 * nothing and reads nothing back.
 *
 * THE CONTRACT.  pts f32 [n][3] on the device, 1 <= n <= UMEREG_VOXEL_CENTROID_MAX_POINTS, voxel > 0.
 * The voxel of a point is floorf(p / voxel) per axis, with the 63-bit key and the table of umereg_voxel_first_index_f32, which this entry
 * calls on the front of its workspace.  Output row r belongs to the voxel whose lowest point index is the r-th smallest: rows are in
 * the order umereg_voxel_first_index_f32 returns, and first_index IS its output.
 * The centroid is an integer sum (voxel_centroid_math.h): per axis q = llrint(((double)p / (double)voxel - (double)c) * 2^32), S = sum q
 * in int64 (global 64-bit integer atomics: any arrival order gives the same integers), centroid = (float)(((double)c + (double)S /
 * ((double)cnt * 2^32)) * (double)voxel).  Outputs are bit-identical from run to run.  The cap on n keeps (double)S exact: |q| <= 2^32,
 * so 2^20 points give |S| <= 2^52 < 2^53.
 * Two deviations from open3d: the grid is anchored at the ORIGIN (open3d: the cloud's minimum bound), so two clouds share it; rows come
 * in the order of their first points (open3d: hash order).
 *
 * count int32 [2] on the device: [0] = m, the number of occupied voxels; [1] != 0 if a coordinate was NaN, infinite or 2^20 voxels or more
 * from the origin (such points are left out; callers treat it as an error).  Rows at and beyond m of the three outputs are not written. */
#ifndef UMEREG_VOXEL_CENTROID_API_H
#define UMEREG_VOXEL_CENTROID_API_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_VOXEL_CENTROID_MAX_POINTS (1 << 20)

/* bytes of workspace umereg_voxel_centroid_f32 needs; 0 for an n it refuses */
size_t umereg_voxel_centroid_workspace_bytes(int n);

/* pts -> centroids f32 [n][3], first_index int64 [n], counts int32 [n] (the first count[0] rows of each are written), count int32 [2] */
int umereg_voxel_centroid_f32(const float* pts, int n, float voxel, float* centroids, int64_t* first_index, int32_t* counts, int* count,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
