/* umereg_sparse_conv.h -- C ABI of the single sparse-convolution operators that training ResUNetSmall2 is made of: the plain
 * convolution over one neighbour table (forward, and with a repacked kernel every input gradient), conv1's forward, the
 * kernel repack and the weight gradient.
 *
 * Same conventions as umereg.h / umereg_featnet.h: outputs and scratch belong to the caller, every compute entry point takes
 * a HIP stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it
 * probes for a device, returns UMEREG_ENODEV where no HIP device is visible, and never waits for the device.  The entry
 * points here are typed by their own table (umeregrobust_amd/sparse_conv.py: SPARSE_CONV_SIGNATURES).
 *
 * Maps: `workspace` / `status` are what umereg_featnet_build_maps(coords, n, batch, ...) filled; n is that call's n.  A table t
 * in [0, UMEREG_SPARSE_CONV_TABLES) (self map of level l: l; strided l -> l+1: 5 + l; transposed l+1 -> l: 9 + l) has one row
 * of 27 neighbour indices per OUTPUT row: out[o] = sum_k in[nbr_t(o, k)] @ W[k] over the neighbours that exist.  The output
 * rows of table t are those of level t (t < 5), t - 4 (t < 9), t - 9 (else); the input rows those of level t, t - 5, t - 8.
 * Row counts are read from `status` on the device; every level has at most n rows.
 *
 * The adjoint of table t (d in[i] = sum over (o, k) with nbr_t(o, k) = i of d out[o] @ W[k]^T) is a plain convolution over
 * another table with the repacked kernel W'[k'] = W[k]^T (`transpose`):  self l -> the same table, k' = 26 - k (`mirror`);
 * strided 5 + l -> table 9 + l, k' = k;  transposed 9 + l -> table 5 + l, k' = k.
 *
 * Feature rows are f32 with a leading dimension in floats (a multiple of 4, >= the channel count; base pointers 16-byte
 * aligned), channel counts multiples of 32 up to UMEREG_SPARSE_CONV_MAX_CH (conv1 and the weight gradient also C_in = 1).
 * Kernels are [27][C_in][C_out], contiguous. */
#ifndef UMEREG_SPARSE_CONV_H
#define UMEREG_SPARSE_CONV_H

#include <stddef.h>
#include <stdint.h>

#include "umereg_featnet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_SPARSE_CONV_TABLES 13
#define UMEREG_SPARSE_CONV_MAX_CH 256
#define UMEREG_SPARSE_CONV_MAX_SEGMENTS 64

/* out[o][0 .. C_out) = (sum_k in[nbr_t(o, k)] @ W[k]) * scale + shift (+ out[o] as it was, if `accumulate`) for every output
 * row of `table`; scale / shift: f32 [C_out] on the device (ones / zeros for the plain convolution: acc * 1 + 0 is exact).
 * `accumulate` lets a caller cut a long contraction into channel slices (in + c0 with the full leading dimension, the slice's
 * own [27][slice][C_out] kernel block, see the repack below): every slice is one short chain, the slices are added in call
 * order -- a two-level sum whose rounding error is a fraction of one chain over all channels. */
int umereg_sparse_conv_f32(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table, const float* in,
                           int ld_in, const float* W, int c_in, int c_out, const float* scale, const float* shift, float* out,
                           int ld_out, int accumulate, void* stream);

/* conv1 (C_in = 1, C_out = 32) over the self map of level 0: out [rows of level 0, 32] in level-0 row order from feat [n, 1]
 * in INPUT row order (the kernel reads feat[perm[j]]); W [27][1][32], scale / shift [32] */
int umereg_sparse_conv1_f32(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, const float* feat,
                            const float* W, const float* scale, const float* shift, float* out, void* stream);

/* Kernel repack, W [27][C_in][C_out] -> out (27 C_in C_out floats, no overlap).  With R = C_out, C = C_in and
 * M[k][r][c] = W[k][c][r] if `transpose`, else R = C_in, C = C_out and M = W:  out[s][k'][r - s slice][c] = M[k][r][c] for
 * r in [s slice, (s + 1) slice), k' = mirror ? 26 - k : k -- R / slice blocks [27][slice][C], each the kernel of a
 * convolution over `slice` of the input channels.  slice must divide R (slice = R: one block). */
int umereg_sparse_conv_repack_f32(const float* W, int c_in, int c_out, int transpose, int mirror, int slice, float* out, void* stream);

/* scratch bytes of the weight gradient over maps of n points (host arithmetic; 0 for arguments the entry would refuse) */
size_t umereg_sparse_conv_wgrad_scratch_bytes(int n, int c_in, int c_out);
/* row segments the weight gradient cuts [0, n) into: a function of n, C_in and C_out only, at most
 * UMEREG_SPARSE_CONV_MAX_SEGMENTS; the scratch holds one [27][C_in][C_out] block per segment */
int umereg_sparse_conv_wgrad_segments(int n, int c_in, int c_out);

/* dW[k] = sum_o in[nbr_t(o, k)]^T dY[o]  ([C_in x C_out], o over the output rows of `table` in ascending order), C_in a
 * multiple of 32 or 1.  Deterministic: every (offset, tile, segment) is one fixed chain, the segments are summed in order;
 * the result does not depend on what `scratch` held. */
int umereg_sparse_conv_wgrad_f32(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table,
                                 const float* in, int ld_in, int c_in, const float* dY, int ld_dy, int c_out, float* dW,
                                 void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
