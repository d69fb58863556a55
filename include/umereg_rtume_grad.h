/* umereg_rtume_grad.h -- C ABI of the backward pass of the RTUME solve (umereg_rtume_solve_f32 of umereg.h): the gradient of the
 * closed-form SE(3) estimate with respect to both UME matrices.  It is what `cube_loss.CubeRegistrationLoss` stands on.
 *
 * Same conventions as umereg.h / umereg_ume_grad.h: outputs belong to the caller, the entry point takes a HIP stream (NULL = the
 * default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, returns
 * UMEREG_ENODEV where no HIP device is visible, and never waits for the device.  The entry point here is typed by its own table
 * (umeregrobust_amd/rtume_grad.py: RTUME_GRAD_SIGNATURES).
 *
 * The pass is deterministic: one hypothesis writes only its own rows, every sum runs in one fixed order, there is no atomic and
 * no scratch. */
#ifndef UMEREG_RTUME_GRAD_H
#define UMEREG_RTUME_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The convention at the rotation's singularity.  The solve takes R = U diag(1, 1, d) V^T from A = U S V^T, d = sign det(U V^T).
 * With the signed values s' = (s1, s2, d s3) the derivative of R has one term per pair (i, j) of singular directions, divided by
 * s'_i + s'_j.  A pair with s'_i + s'_j <= UMEREG_RTUME_BWD_MIN_GAP * s1 contributes nothing (its term is set to 0): there R is
 * not a differentiable function of the input (s2 + d s3 = 0: a reflection fits as well as the rotation), and below this relative
 * size the forward itself declares A rank 1 and completes the second singular direction arbitrarily, so that R is no function of
 * the input at all.  Where the forward returns R = I without looking at A (A zero, infinite or NaN) the gradient takes no path
 * through R: only the terms of the translation that do not pass through R remain.  Repeated singular values (s1 = s2, or
 * s2 = s3 with d = +1) are no singularity and need no convention. */
#define UMEREG_RTUME_BWD_MIN_GAP 1e-8

/* Forward (umereg_rtume_solve_f32 without index arrays): T_k = RTUME(G_k, H_k), T_k[:3,:3] = R_k^T, T_k[:3,3] = b2_k, for
 * G, H f32 [n][32][4].
 *
 * dG, dH f32 [n][32][4]: the gradients of sum_k <dT_k, T_k> for the upstream dT f32 [n][4][4], of which only rows 0-2 are read
 * (row 3 of T is constant).  The forward's quantities are recomputed from G and H in fp64, as the forward computes them; the
 * results are rounded once on output.  Either output may be NULL (not both): it is not written. */
int umereg_rtume_solve_bwd_f32(const float* G, const float* H, const float* dT, int n, float* dG, float* dH, void* stream);

#ifdef __cplusplus
}
#endif

#endif
