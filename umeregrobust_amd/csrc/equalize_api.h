/* equalize_api.h -- C entry points of the built-in sampling equalizer (csrc/equalize.hip): this library's own stand-in for the surface half
 * of the reference's Sampling Equalizer Module (lidar_point_cloud_completion, datasets/kitti/kitti_dataset.py:511-542), which rebuilds a
 * surface with NKSR and samples it uniformly.  NKSR (a learned kernel field) is NOT rebuilt and no similarity to its samples is claimed;
 * what is built is what the module is for: undo the 1/r^2 density of a spinning lidar by resampling the scanned surfaces to uniform
 * density.  A private header: typed by umeregrobust_amd/equalizer.py (EQUALIZE_SIGNATURES, through _lib.load_typed), not under include/.
 *
 * Conventions of umereg.h: outputs and workspace belong to the caller, every compute entry takes a HIP stream (NULL = the default stream),
 * returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, allocates nothing and waits for
 * nothing.  Every output is a function of the inputs alone: no atomics, no device RNG state, fixed reduction trees, no word of the
 * workspace read that the call did not write.
 *
 * THE CONTRACT.  pts f32 [n][3] on the device, sensor at the origin.  num_points M (default 125 000), knn k in [3, 64] (16), max_radius
 * r_max in [1e-3, 1e3] m (1.0), project (on), seed uint32 (0).  The defaults are choices, not tuned on real scans.  n, M <= 2^22.
 *
 * Surfels, per point i: its K = min(k, n) nearest points, itself included (umereg_knn_points_f32: exact, ties -> lower index); normal n_i
 * from the neighbourhood's fp64 covariance about its own mean (covariance_normal, icp_plane_math.h; fewer than 3 neighbours or a zero
 * covariance: (0, 0, 1)); support r2_i = min(d2 of the K-th neighbour, r_max * r_max) in f32; integer area weight q_i = (uint32)(r2_i * s),
 * s = (float)(65536 / r_max^2) formed on the host; fewer than 3 neighbours or r2_i == 0 (duplicates): q_i = 0.  Area ~ r_k^2 is the
 * inverse of the local density, so samples allocated in proportion to q equalize it.
 *
 * Allocation (integers only): Q = inclusive 64-bit prefix sum of q, Qt = Q[n-1].  One offset per call, r = (xi_0(0) Qt) >> 24 < Qt;
 * sample j of M sits at u_j = (j Qt + r) / M, and its source is the first i with Q[i] > u_j (systematic resampling: every point gets
 * the floor or the ceiling of its share, |count_i - M q_i / Qt| < 1; a point with q = 0 is never chosen; Qt < M is legal).
 * xi_c(j), c = 0, 1, 2: the top 24 bits of the stateless integer mix of (seed, j, c) in equalize_math.h; c = 0 is read at j = 0 only.
 *
 * Placement (f32, one rounding per operation): (t1, t2) the branch-free orthonormal basis of n_i (Duff et al. 2017); a = (xi1 - 2^23) 2^-23,
 * b likewise from xi2; half side h_i = sqrtf(r2_i) * c, c = (float)(0.5 sqrt(pi / K)); x_j = p_i + h_i * ((a * t1) + (b * t2));
 * src_index[j] = i, rho2_j = r2_i.
 *
 * Projection (one moving-least-squares step per sample): neighbours are the original points p with f32 d2 = ((dx*dx)+(dy*dy))+(dz*dz) < rho2_j,
 * d = x - p; weight w = (1 - d2 / rho2)^2 in fp64; with e = p - x (exact in fp64), m = sum w e / sum w and C = sum w (e - m)(e - m)^T, two
 * passes in fp64, n = covariance_normal(C): x' = x + (m . n) n, computed in fp64 and rounded once to f32.  Fewer than 3 neighbours or a
 * zero covariance: x' = x.
 *
 * Qt == 0 (no point has an area: n < 3, or every support is zero) leaves nothing to sample.  n < 3 is refused with UMEREG_EINVAL; a
 * Qt that turns out zero on the device cannot be reported by an entry that does not wait: the sample kernel then writes src_index = -1,
 * samples = 0, rho2 = 0, and `total` (the device word that receives Qt) tells the caller, who must treat 0 as UMEREG_EINVAL. */
#ifndef UMEREG_EQUALIZE_API_H
#define UMEREG_EQUALIZE_API_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_EQUALIZE_MIN_KNN 3
#define UMEREG_EQUALIZE_MAX_KNN 64
#define UMEREG_EQUALIZE_MAX_POINTS (1 << 22)
#define UMEREG_EQUALIZE_MIN_RADIUS 1.0e-3f
#define UMEREG_EQUALIZE_MAX_RADIUS 1.0e3f

/* bytes of workspace umereg_equalize_cloud_f32 needs; 0 for arguments it refuses.  The stage entries use the front of the same carve-up,
 * which does not depend on num_points: surfels and sample need (n, 1, knn) bytes, project (n, 1, 3); the size of the whole call serves all. */
size_t umereg_equalize_workspace_bytes(int n, int num_points, int knn);

/* pts -> normals f32 [n][3], r2 f32 [n], q uint32 [n] */
int umereg_equalize_surfels_f32(const float* pts, int n, int knn, float max_radius, float* normals, float* r2, uint32_t* q,
                                void* workspace, size_t workspace_bytes, void* stream);

/* pts, normals, r2, q -> samples f32 [M][3], src_index int64 [M], rho2 f32 [M], total uint64 [1] (Qt).  The 64-bit scan of q happens
 * inside (one workgroup, fixed order).  knn: the one the surfels were made with (K enters the patch size). */
int umereg_equalize_sample_f32(const float* pts, const float* normals, const float* r2, const uint32_t* q, int n, int num_points, int knn,
                               uint32_t seed, float* samples, int64_t* src_index, float* rho2, uint64_t* total, void* workspace,
                               size_t workspace_bytes, void* stream);

/* samples, rho2, pts -> projected f32 [M][3]; nb_count int32 [M] (may be NULL): the neighbours each sample's projection used.  Builds the
 * grid of pts in the workspace (kNN mode, as the ICP does). */
int umereg_equalize_project_f32(const float* samples, const float* rho2, const float* pts, int num_points, int n, float* projected,
                                int32_t* nb_count, void* workspace, size_t workspace_bytes, void* stream);

/* the three chained on one stream: pts -> out f32 [M][3], src_index int64 [M], total uint64 [1]; project == 0 skips the projection */
int umereg_equalize_cloud_f32(const float* pts, int n, int num_points, int knn, float max_radius, int project, uint32_t seed, float* out,
                              int64_t* src_index, uint64_t* total, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
