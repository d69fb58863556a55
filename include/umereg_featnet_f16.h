/* umereg_featnet_f16.h -- C ABI of the f16-operand inference mode of the ResUNetSmall2 feature network: the fused forward
 * pass and the single convolution, with every operand of the matrix products rounded to f16 and every sum kept in f32.
 *
 * Same conventions as umereg_featnet.h / umereg_sparse_conv.h: outputs and workspace belong to the caller, every entry
 * point takes a HIP stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument
 * errors before it probes for a device, returns UMEREG_ENODEV where no HIP device is visible, and never waits for the
 * device.  The entry points here are typed by their own table (umeregrobust_amd/models.py: FEATNET_F16_SIGNATURES).
 *
 * The contract.  Layers 1..18 of umereg_featnet_layer_info (the seventeen 27-offset convolutions other than conv1, and
 * mlp1) compute
 *     out[o][c] = (sum over offsets k ascending, channels i ascending: f16(in[nbr_k(o)][i]) * f16(W[k][i][c])) * scale + shift
 * where f16() rounds an f32 value to IEEE binary16, to nearest even (a value beyond 65504 + 16 becomes infinity), each
 * product is exact and the sum is accumulated in f32 by v_mfma_f32_32x32x16_f16, 16 channels per instruction; a missing
 * neighbour contributes zeros.  The chain of an output element does not depend on the tile or the row order: two runs
 * agree bit for bit, a batch equals its clouds bit for bit.  The epilogue (scale, shift, residual, ReLU) and every stored
 * activation are f32; conv1 (C_in = 1) and `final` with the L2 normalisation are the f32 kernels of umereg_featnet.h.  The
 * packed parameter block is the f32 block of umereg_featnet.h (weights are rounded where a tile is staged); the workspace,
 * its size (umereg_featnet_workspace_bytes), its debug buffers (umereg_featnet_buffer) and `status` are those of
 * umereg_featnet.h and serve both precisions.
 *
 * The entry points here are inference's; the f16-operand form of the training path (umereg_sparse_conv.h) is
 * umereg_sparse_conv_f16.h. */
#ifndef UMEREG_FEATNET_F16_H
#define UMEREG_FEATNET_F16_H

#include <stddef.h>
#include <stdint.h>

#include "umereg_featnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status[0] bit of umereg_featnet_forward_f16 (beside 1 and 2 of umereg_featnet.h): an activation stored by one of layers
 * 1..17 lies outside [-65504, 65504] (or is a NaN), so a later layer's f16 operand would be infinite; the output is undefined */
#define UMEREG_FN_ERR_F16_RANGE 4

/* the forward pass with f16 operands: the arguments of umereg_featnet_forward_f32 */
int umereg_featnet_forward_f16(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out,
                               int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* the plain convolution with f16 operands: the arguments of umereg_sparse_conv_f32 (in, W, scale, shift and out are f32;
 * `accumulate` adds the slice's result to out in f32).  table -1 is the 1x1 layer over level 0: out[o] = in[o] @ W,
 * W [C_in][C_out].  No range check: an input beyond the f16 range is rounded to infinity, as the conversion does. */
int umereg_sparse_conv_f16(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table, const float* in,
                           int ld_in, const float* W, int c_in, int c_out, const float* scale, const float* shift, float* out,
                           int ld_out, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif

#endif
