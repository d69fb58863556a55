/* umereg_icp_gicp.h -- C entries of the opt-in plane-to-plane (generalized) ICP refinement (csrc/icp.hip, csrc/icp_gicp_math.h): Segal et
 * al.'s Generalized ICP in its plane-to-plane form, the counterpart of open3d's
 *     registration_generalized_icp(src, tgt, d, T_init, TransformationEstimationForGeneralizedICP(epsilon),
 *                                  ICPConvergenceCriteria(max_iteration=...))
 * (epsilon = 1e-3 by default there, as recalled).  open3d is not installable here: parity with it stays unpinned, as for the other two
 * loops.
 *
 * The entries are typed by _lib.TABLES["umereg_icp_gicp.h"], which umeregrobust_amd/icp_gicp.py aliases as ICP_GICP_SIGNATURES.
 *
 * Same conventions as umereg_icp_plane.h: outputs and workspace belong to the caller, every compute entry takes a HIP stream (NULL =
 * the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device and
 * allocates nothing.  The size query is host arithmetic and returns 0 for arguments the entries refuse.  Every output is a function
 * of the inputs alone: no atomics, fixed reduction trees, no word of the workspace read that the call did not write. */
#ifndef UMEREG_ICP_GICP_H
#define UMEREG_ICP_GICP_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_GICP_MIN_EPSILON 1e-4f
#define UMEREG_GICP_MAX_EPSILON 1.0f

/* bytes of workspace the plane-to-plane entries need; 0 for empty clouds */
size_t umereg_icp_plane_to_plane_workspace_bytes(int n_src, int n_tgt);

/* Plane-to-plane ICP with open3d's RegistrationICP loop: evaluate, update, T <- update * T, evaluate, stop on
 * |d fitness| < relative_fitness and |d inlier_rmse| < relative_rmse; fitness and inlier_rmse from Euclidean distances -- the loop
 * of umereg_icp_point_to_plane_f32, arguments and outputs alike, with the source's normals in front of the target's and epsilon
 * behind relative_rmse.  src_normals f32 [n_src][3] (in the SOURCE's own frame: the kernel rotates them), tgt_normals f32 [n_tgt][3]
 * (device), unit vectors as umereg_estimate_normals_f32 writes them (not checked); a zero normal means an isotropic covariance for
 * that point.  Per correspondence (s a source point with normal n_s, p = T s in fp64, q its exact nearest target closer than
 * max_correspondence_distance, n_q its normal, R the rotation of the current T; epsilon widened to fp64):
 *     a = R n_s, b = n_q, M = 2 I - (1 - epsilon) (a a^T + b b^T)  (= C_q + R C_s R^T with C = I - (1 - epsilon) n n^T),
 *     W = M^-1 (closed form), d = p - q, J0 = [ -[p]x  I3 ];
 * the update solves (sum J0^T W J0) x = -(sum J0^T W d) and is [Rz(x2) Ry(x1) Rx(x0) | x3..5].  M is fixed during an update
 * (standard GICP).  The solve is umereg_icp_point_to_plane_f32's: through the eigen-decomposition, eigenvalues at or below
 * 1e-12 * lambda_max treated as zero.  epsilon in [1e-4, 1], anything else is refused; epsilon = 1 makes M = 2 I: the normals drop
 * out and the loop is Gauss-Newton point to point.  The result is even in either set of normals.  No correspondences: the update is
 * the identity.  Synchronous with respect to `stream` (the stop test lives on the device; the host polls it once per batch). */
int umereg_icp_plane_to_plane_f32(const float* src, const float* tgt, const float* src_normals, const float* tgt_normals, int n_src,
                                  int n_tgt, const double* T_init_host, float max_correspondence_distance, int max_iteration,
                                  double relative_fitness, double relative_rmse, float epsilon, double* T_out_host,
                                  double* fitness_host, double* inlier_rmse_host, int* iterations_host, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* the same from a start transform on the DEVICE (f32 [4][4] row major), read when the first kernel runs */
int umereg_icp_plane_to_plane_dev_f32(const float* src, const float* tgt, const float* src_normals, const float* tgt_normals, int n_src,
                                      int n_tgt, const float* T_init_dev, float max_correspondence_distance, int max_iteration,
                                      double relative_fitness, double relative_rmse, float epsilon, double* T_out_host,
                                      double* fitness_host, double* inlier_rmse_host, int* iterations_host, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* enqueue only, as umereg_icp_plane_enqueue_f32: [first: the target's grid, the initial state] + `iterations` evaluation / update
 * pairs + an asynchronous copy of the state (umereg_icp_state_bytes bytes; read it with umereg_icp_state_decode) to state_host.
 * Nothing is waited for. */
int umereg_icp_plane_to_plane_enqueue_f32(const float* src, const float* tgt, const float* src_normals, const float* tgt_normals,
                                          int n_src, int n_tgt, const float* T_init_dev, float max_correspondence_distance,
                                          int max_iteration, double relative_fitness, double relative_rmse, float epsilon, int first,
                                          int iterations, void* state_host, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
