/* umereg_sparse_conv_f16.h -- C ABI and contract of the f16-operand TRAINING mode of the ResUNetSmall2 feature network: the
 * single sparse-convolution operators of umereg_sparse_conv.h with the operands of every matrix product rounded to f16 and
 * every sum kept in f32.  Parameters, gradients and every stored activation are f32; the mode is opt-in
 * (umeregrobust_amd: sparse_conv(..., precision="f16"), ResUNetSmall2(..., train_precision="f16")) and deterministic like the
 * f32 path.
 *
 * Same conventions as umereg_sparse_conv.h / umereg_featnet_f16.h: outputs and scratch belong to the caller, every entry
 * point takes a HIP stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument
 * errors before it probes for a device, returns UMEREG_ENODEV where no HIP device is visible, and never waits for the
 * device.  The entry point here is typed by its own table (umeregrobust_amd/sparse_conv.py: SPARSE_CONV_F16_SIGNATURES).
 *
 * The contract, in the notation of umereg_featnet_f16.h: f16() rounds an f32 value to IEEE binary16, to nearest even; sums are
 * f32; a missing neighbour contributes zeros.
 *
 *   Forward, 27-offset layers after conv1:  umereg_sparse_conv_f16 (umereg_featnet_f16.h) as it stands -- one chain over all
 *     input channels, as in the fused f16 forward, not the 32-channel slices of the f32 training path.
 *   Forward, mlp1:  the same entry with table = -1.
 *   Unchanged:  conv1, `final`, batch norm, the residual, ReLU, the concatenation and the L2 normalisation are f32; saved
 *     activations are f32 (f16 storage of activations is out of scope).
 *   Backward scaling:  the output gradient dY of a layer is scaled by a power of two before it is rounded,
 *         e = 14 - floor(log2(max |dY|)),   dYs = dY 2^e   (exact),
 *     so the largest scaled magnitude lies in [2^14, 2^15); e = 0 if max |dY| is zero or not finite.  e is computed on the
 *     device; no host synchronisation is added.  (The Python layer holds e to +-126 so that 2^e and 2^-e are normal f32
 *     numbers: below max |dY| = 2^-112 the scaled maximum stays under 2^14.)  A power-of-two scale commutes with rounding in
 *     f16's normal range, so the result is the unscaled one wherever nothing underflows.  A scaled operand below 2^-14 is at
 *     most 2^-28 of the largest
 *     operand; whether the hardware rounds it to an f16 subnormal or to zero has NOT been measured here, and no gate of the
 *     tests depends on it (they allow 2^-14 2^-e sum |x_i| for it).
 *   Input gradient:  dX[i] = 2^-e sum over (o, k) with nbr(o, k) = i of f16(dYs[o]) @ f16(W[k])^T -- umereg_sparse_conv_f16 over
 *     the adjoint table with the repacked kernel (umereg_sparse_conv.h); the epilogue's `scale` vector carries 2^-e (exact).
 *     mlp1: table = -1 with W^T.
 *   Weight gradient of a 27-offset layer with C_in >= 32:  dW[k] = 2^-e sum_o f16(X[nbr(o, k)])^T f16(dYs[o]) -- the entry
 *     below, then a multiplication by 2^-e.  f16(X) is the very operand the forward used, so dW is the exact straight-through
 *     gradient of the forward contract; the only further approximation of the backward pass is the rounding of dY.
 *     conv1's weight gradient (C_in = 1) stays f32 (umereg_sparse_conv_wgrad_f32); mlp1's and `final`'s stay f32 block sums. */
#ifndef UMEREG_SPARSE_CONV_F16_H
#define UMEREG_SPARSE_CONV_F16_H

#include <stddef.h>
#include <stdint.h>

#include "umereg_featnet_f16.h"
#include "umereg_sparse_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dW[k] = sum_o f16(in[nbr_t(o, k)])^T f16(dY[o])  ([C_in x C_out], f32): the arguments and conventions of
 * umereg_sparse_conv_wgrad_f32 -- rows are f32, the caller passes dY already scaled (and multiplies dW by 2^-e afterwards);
 * C_in and C_out multiples of 32 up to UMEREG_SPARSE_CONV_MAX_CH (C_in = 1 is refused: conv1 stays f32).  The row segmentation
 * is that of the f32 entry: umereg_sparse_conv_wgrad_scratch_bytes and umereg_sparse_conv_wgrad_segments serve both
 * precisions.  Deterministic: the chain of an (offset, tile, segment) is the segment's rows that have a neighbour at the offset,
 * ascending, in groups of 16 (one v_mfma_f32_32x32x16_f16 each; a padded group adds 0 * 0); the segments that hold rows are
 * summed in order by a second launch.  The result depends neither on what `scratch` held nor on a second run; no atomics.
 * Every argument error, a short scratch included, is reported before the device probe. */
int umereg_sparse_conv_wgrad_f16(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table,
                                 const float* in, int ld_in, int c_in, const float* dY, int ld_dy, int c_out, float* dW,
                                 void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
