/* umereg_icp_plane.h -- C ABI of the opt-in point-to-plane refinement: target normals (csrc/normals.hip) and the point-to-plane
 * ICP loop (csrc/icp.hip), the counterparts of open3d's
 *     tgt.estimate_normals(KDTreeSearchParamKNN(knn) | KDTreeSearchParamHybrid(radius, knn))
 *     registration_icp(src, tgt, d, T_init, TransformationEstimationPointToPlane(), ICPConvergenceCriteria(max_iteration=...))
 * open3d is not installable here: parity with it stays unpinned, as for the point-to-point loop.
 *
 * Same conventions as umereg.h: outputs and workspace belong to the caller, every compute entry takes a HIP stream (NULL = the
 * default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device and
 * allocates nothing.  The size queries are host arithmetic and return 0 for arguments the entries refuse.  Every output is a function
 * of the inputs alone: no atomics, fixed reduction trees, no word of the workspace read that the call did not write.  The entry points here
 * are typed by their own table (umeregrobust_amd/icp_plane.py: ICP_PLANE_SIGNATURES). */
#ifndef UMEREG_ICP_PLANE_H
#define UMEREG_ICP_PLANE_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_NORMALS_MIN_KNN 3
#define UMEREG_NORMALS_MAX_KNN 64

/* bytes of workspace umereg_estimate_normals_f32 needs (search structure + the neighbour lists); 0 for n < 1 or knn outside [3, 64] */
size_t umereg_normals_workspace_bytes(int n, int knn);

/* Normals.  pts f32 [n][3] (device) -> normals f32 [n][3].  The neighbourhood of a point is its min(knn, n) nearest points of the
 * cloud, itself included (umereg_knn_points_f32: exact, fp32 squared distances summed left to right, ties -> lower index); with
 * radius > 0 (open3d's hybrid search) the neighbours whose squared distance exceeds (float)radius * (float)radius are dropped.
 * The covariance is formed in fp64 about the neighbourhood's own mean; the normal is the unit eigenvector of its smallest eigenvalue
 * (fp64 Jacobi), with the component of largest magnitude positive (ties -> the lowest axis).  Fewer than 3 neighbours, or a zero
 * covariance: (0, 0, 1).  radius <= 0: no radius.  Does not wait for the device. */
int umereg_estimate_normals_f32(const float* pts, int n, int knn, float radius, float* normals, void* workspace,
                                size_t workspace_bytes, void* stream);

/* bytes of workspace the point-to-plane entries need; 0 for empty clouds */
size_t umereg_icp_plane_workspace_bytes(int n_src, int n_tgt);

/* Point-to-plane ICP with open3d's RegistrationICP loop: evaluate, update, T <- update * T, evaluate, stop on
 * |d fitness| < relative_fitness and |d inlier_rmse| < relative_rmse; fitness and inlier_rmse from Euclidean distances -- the loop
 * of umereg_icp_point_to_point_f32, arguments and outputs alike.  tgt_normals f32 [n_tgt][3] (device).  Per correspondence (p the
 * fp64-transformed source point, q its exact nearest target closer than max_correspondence_distance, n_q its normal):
 * r = (p - q) . n_q, J = [p x n_q, n_q]; the update solves (sum J J^T) x = -(sum J r) and is [Rz(x2) Ry(x1) Rx(x0) | x3..5].
 * Deviation from open3d (Eigen's LDLT): the system is solved through its eigen-decomposition, eigenvalues at or below
 * 1e-12 * lambda_max treated as zero -- the minimum-norm update where the correspondences leave directions unconstrained; the same
 * solution wherever the system has full rank.  No correspondences: the update is the identity.
 * Synchronous with respect to `stream` (the stop test lives on the device; the host polls it once per batch of iterations). */
int umereg_icp_point_to_plane_f32(const float* src, const float* tgt, const float* tgt_normals, int n_src, int n_tgt,
                                  const double* T_init_host, float max_correspondence_distance, int max_iteration,
                                  double relative_fitness, double relative_rmse, double* T_out_host, double* fitness_host,
                                  double* inlier_rmse_host, int* iterations_host, void* workspace, size_t workspace_bytes, void* stream);

/* the same from a start transform on the DEVICE (f32 [4][4] row major), read when the first kernel runs */
int umereg_icp_point_to_plane_dev_f32(const float* src, const float* tgt, const float* tgt_normals, int n_src, int n_tgt,
                                      const float* T_init_dev, float max_correspondence_distance, int max_iteration,
                                      double relative_fitness, double relative_rmse, double* T_out_host, double* fitness_host,
                                      double* inlier_rmse_host, int* iterations_host, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* enqueue only, as umereg_icp_enqueue_f32: [first: the target's grid, the initial state] + `iterations` evaluation / update pairs +
 * an asynchronous copy of the state (umereg_icp_state_bytes bytes; read it with umereg_icp_state_decode) to state_host.  Nothing is
 * waited for. */
int umereg_icp_plane_enqueue_f32(const float* src, const float* tgt, const float* tgt_normals, int n_src, int n_tgt,
                                 const float* T_init_dev, float max_correspondence_distance, int max_iteration,
                                 double relative_fitness, double relative_rmse, int first, int iterations, void* state_host,
                                 void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
