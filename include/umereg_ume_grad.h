/* umereg_ume_grad.h -- C ABI of the backward passes that the UME contrastive loss needs: the gradient of the UME moment
 * matrices with respect to the point features, and the gradient of the subspace distance matrix with respect to both sets
 * of UME matrices.
 *
 * Same conventions as umereg.h / umereg_featnet.h / umereg_sparse_conv.h: outputs and scratch belong to the caller, every
 * compute entry point takes a HIP stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports
 * argument errors before it probes for a device, returns UMEREG_ENODEV where no HIP device is visible, and never waits for
 * the device.  Size queries are host arithmetic and return 0 for arguments the compute entry would refuse.  The entry points
 * here are typed by their own table (umeregrobust_amd/ume_grad.py: UME_GRAD_SIGNATURES).
 *
 * Both passes are deterministic: every sum runs in one fixed order, there is no floating-point atomic, and no result
 * depends on what the scratch held. */
#ifndef UMEREG_UME_GRAD_H
#define UMEREG_UME_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* feature channels of a UME matrix (rows of the 32 x 4 matrix) */
#define UMEREG_UME_GRAD_D 32
/* the largest neighbour list the moment kernel writes (umereg_ume_moments_packed_f32) */
#define UMEREG_UME_GRAD_MAX_K 7680
/* A pair with D_ij <= this has no gradient: it contributes nothing to either side.  The distance is not differentiable at 0
 * (torch's cdist backward gives 0 there), and the forward forms D^2 = 4 - |Q1^T Q2|_F^2 in f32, so the D of two equal
 * subspaces is the square root of that difference's rounding noise (about 1e-6: D up to about 1e-3), not 0.  4e-3 is
 * D^2 = 1.6e-5, 67 ulp of 4: above the noise, and far below the distance of any two distinct neighbourhoods. */
#define UMEREG_UME_CDIST_BWD_DMIN 4e-3f

/* ---- moments ---------------------------------------------------------------------------------------------------------
 * Forward (umereg_ume_moments_packed_f32): Fr_i[c][:] = sum_{j in N(i)} feat[j][c] * [1, p_j], and with `normalize`
 * F_i = Fr_i / (s_i + 1e-6), s_i = sum_c Fr_i[c][0].  N(i) is row i of `nn_idx` AS THE FORWARD WROTE IT: int64 [B][n][K],
 * ascending point indices, padded with -1.
 *
 * dfeat[b][j][:] = (sum over the keypoints i of b with j in N(i), in ascending i, of Gr_i) . [1, p_j]   (f32 [B][N][32])
 * Gr_i = dF_i (raw), or dF_i / (s_i + 1e-6) with <dF_i, F_i> / (s_i + 1e-6) subtracted from column 0 (`normalize`; F is the
 * forward's output then, and may be NULL otherwise).  Sums are fp64; a point in no list gets exactly 0. */
size_t umereg_ume_moments_bwd_scratch_bytes(int B, int N, int n);
int umereg_ume_moments_bwd_f32(const float* pts, const float* feat, const int64_t* nn_idx, const float* F, const float* dF, int B,
                               int N, int n, int K, int normalize, float* dfeat, void* scratch, size_t scratch_bytes, void* stream);

/* ---- subspace distance -----------------------------------------------------------------------------------------------
 * Forward: D[i][j] = |P1_i - P2_j|_F / sqrt(2), P = Q Q^T, ume = Q R (32 x 4, full rank).  One batch element per call:
 * ume1 f32 [n1][32][4], ume2 f32 [n2][32][4], D (the forward's output) and dD f32 [n1][n2].
 *
 * With w_ij = dD_ij / (2 D_ij) (0 where D_ij <= UMEREG_UME_CDIST_BWD_DMIN) and M1_i = sum_j w_ij Q2_j Q2_j^T Q1_i:
 *     dume1_i = -2 (M1_i - Q1_i Q1_i^T M1_i) R1_i^{-T},   and dume2_j the same with the roles swapped.
 * M is an f32 MFMA contraction (two chained products per 32 x 32 tile, no n1 x n2 x 16 intermediate); the bases, the sum
 * over the column splits and the per-keypoint finish are fp64.  Either output may be NULL (not both): its pass is skipped. */
size_t umereg_ume_cdist_bwd_scratch_bytes(int n1, int n2);
int umereg_ume_cdist_bwd_f32(const float* ume1, const float* ume2, const float* D, const float* dD, int n1, int n2, float* dume1,
                             float* dume2, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
