/* umereg_sparse_conv_pairs.h -- C ABI and contract of the pair-compacted convolution engine of the ResUNetSmall2 feature
 * network (opt-in; umeregrobust_amd: conv_mode="pairs", the default engine is "union"): the fused forward pass and the single
 * convolution of umereg_featnet.h / umereg_featnet_f16.h / umereg_sparse_conv.h, with every 27-offset layer on kernels that feed
 * the matrix unit, for every offset k, only the rows of a tile that have a neighbour at k.
 *
 * Same conventions as those headers: outputs and workspace belong to the caller, every entry point takes a HIP stream (NULL =
 * the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device,
 * returns UMEREG_ENODEV where no HIP device is visible, and never waits for the device.  The entry points here are typed by
 * their own table (umeregrobust_amd/sparse_conv.py: SPARSE_CONV_PAIRS_SIGNATURES).
 *
 * The contract: the values of the union engine.  The union engine skips nothing: a workgroup walks every offset that some row
 * of its tile uses and, for a row without that neighbour, adds 0 * w -- which leaves a finite accumulator as it was.  The
 * kernels here use the same instructions (v_mfma_f32_32x32x2_f32; with f16 operands v_mfma_f32_32x32x16_f16), the same
 * 32-channel slices, the same order (offsets ascending, then channels ascending), round to f16 at the same point and keep the
 * same epilogue -- fmaf(acc, scale, shift), then the residual, then the ReLU, then the f16 range flag -- so every output element
 * runs the union engine's chain minus its no-op links, and the outputs are equal bit for bit.  A row whose mask is empty (the
 * stride-3 table has such rows) still gets its epilogue: shift, then the residual, then the ReLU.  Two differences are allowed:
 *   1. the sign of a zero: where the union engine's accumulator is -0 when it meets a no-op link, -0 + 0 * w = +0 there and -0
 *      here (a -0 accumulator needs a negative sum that underflows; +0 and -0 compare equal);
 *   2. non-finite WEIGHTS: 0 * inf and 0 * nan are NaN, which the union engine lets reach the rows that lack the neighbour and
 *      this engine does not.  Non-finite activations meet only rows that gather them, in both engines alike.
 * Deterministic like the union engine: no atomics on data, no host synchronisation, bit-identical from run to run, a batch equals
 * its clouds, a row permutation of the input permutes the output.  The compaction lives in LDS: the workspace, its layout, its
 * size (umereg_featnet_workspace_bytes), its debug buffers (umereg_featnet_buffer) and `status` are those of umereg_featnet.h
 * and serve both engines.  The 1x1 layers (every row is active there), conv1 and `final` run the union engine's kernels in both
 * modes.  The weight gradient (umereg_sparse_conv.h) has no mode: it is pair-compacted already. */
#ifndef UMEREG_SPARSE_CONV_PAIRS_H
#define UMEREG_SPARSE_CONV_PAIRS_H

#include <stddef.h>
#include <stdint.h>

#include "umereg_featnet_f16.h"
#include "umereg_sparse_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the forward pass on the pair-compacted engine: the arguments of umereg_featnet_forward_f32, then f16 (0: the values of
 * umereg_featnet_forward_f32; else: those of umereg_featnet_forward_f16, UMEREG_FN_ERR_F16_RANGE in status[0] included) */
int umereg_featnet_forward_pairs(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out,
                                 int32_t* status, void* workspace, size_t workspace_bytes, void* stream, int f16);

/* the plain convolution on the pair-compacted engine: the arguments of umereg_sparse_conv_f32, then f16 (0: the values and
 * argument checks of umereg_sparse_conv_f32; else: those of umereg_sparse_conv_f16, whose table -1 -- the 1x1 layer -- runs the
 * union engine's kernel) */
int umereg_sparse_conv_pairs(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table, const float* in,
                             int ld_in, const float* W, int c_in, int c_out, const float* scale, const float* shift, float* out,
                             int ld_out, int accumulate, void* stream, int f16);

#ifdef __cplusplus
}
#endif

#endif
