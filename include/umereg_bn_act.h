/* umereg_bn_act.h -- C ABI of the fused batch norm of the trainable ResUNetSmall2's opt-in path (`fused_norm=True`):
 *     y = act(batch_norm(x) [+ residual]),  act in {identity, ReLU},
 * forward and backward, and of the device-side gradient scale of the f16 training path (umereg_sparse_conv_f16.h).
 *
 * Same conventions as umereg.h / umereg_sparse_conv.h: outputs and scratch belong to the caller, every compute entry point takes
 * a HIP stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it
 * probes for a device, returns UMEREG_ENODEV where no HIP device is visible, and never waits for the device.  Size queries are
 * host arithmetic and return 0 for arguments the compute entry would refuse.  The entry points here are typed by their own
 * table (umeregrobust_amd/bn_act.py: BN_ACT_SIGNATURES).
 *
 * Activations and gradients are f32 [n][C] with a row stride in elements (a multiple of 4, at least C; 16-byte aligned base), C a
 * multiple of 32 up to UMEREG_BN_ACT_MAX_CH.  Per-channel vectors are contiguous f32 [C].
 *
 * Summation.  The rows are cut into slabs of S rows, S a function of (n, C) alone (csrc/bn_act_plan.h).  Inside a slab each of
 * the workgroup's row lanes adds its rows (row r, r + unit, ...) in ascending order and the lanes are added in ascending order;
 * every slab writes one fp64 partial per channel and sum to the scratch; the partials are added in ascending slab order as W runs
 * of consecutive slabs whose sums are then added in ascending order.  All of it is fp64, there is no atomic, every scratch word
 * read was written by the same call, and so every result is deterministic bit for bit and independent of what the scratch held.
 *
 * Forward statistics are taken about a pivot (row 0 of each channel): S1 = sum (x - p), S2 = sum (x - p)^2 in fp64 (the
 * differences are exact there), mean = p + S1 / n, var = S2 / n - (S1 / n)^2 (biased), invstd = 1 / sqrt(var + eps); the saved
 * mean and invstd are those fp64 values rounded once to f32. */
#ifndef UMEREG_BN_ACT_H
#define UMEREG_BN_ACT_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_BN_ACT_MAX_CH 256

/* bytes of scratch either pass needs for n rows of C channels (train mode and every backward with parameter gradients; an
 * eval-mode forward needs none); 0 for sizes the compute entries refuse */
size_t umereg_bn_act_scratch_bytes(int n, int C);

/* y = act(x scale + shift [+ residual]), scale = gamma invstd, shift = beta - mean scale (f32, one fused multiply-add each).
 * train != 0: mean / invstd are the batch's (above; n >= 2), and running_mean <- (1 - momentum) running_mean + momentum mean,
 *   running_var the same with the unbiased variance var n / (n - 1), num_batches_tracked += 1, all in place; the three may be
 *   NULL together (nothing is tracked).
 * train == 0: mean = running_mean, invstd = 1 / sqrt(running_var + eps) (both required); nothing is updated, no statistics
 *   launch, scratch may be NULL.
 * save_mean / save_invstd (f32 [C], required) receive the statistics used: what the backward reads.  residual may be NULL;
 * y may alias neither x nor residual.  relu != 0: act = max(., 0).  Two launches in train mode, one in eval mode. */
int umereg_bn_act_forward_f32(const float* x, int ld_x, const float* residual, int ld_res, int n, int C, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, int train,
                              int relu, double eps, double momentum, float* y, int ld_y, float* save_mean, float* save_invstd,
                              void* scratch, size_t scratch_bytes, void* stream);

/* With g = dy (y > 0) (relu) or g = dy, xhat = (x - save_mean) save_invstd:
 *     dbeta = sum g,  dgamma = sum g xhat   (fp64, the slab tree above; f32 [C] out),
 *     train:  dx = gamma invstd (g - dbeta / n - xhat dgamma / n);   eval:  dx = gamma invstd g;   dres = g.
 * g is never stored on its own: the reduction and the apply kernel both read dy, y and x.  y is read only with relu != 0 and may
 * be NULL otherwise; dx and dres may each be NULL (not written).  dgamma and dbeta may be NULL together in eval mode only: the
 * reduction is skipped then (one launch, no scratch).  Two launches otherwise. */
int umereg_bn_act_backward_f32(const float* dy, int ld_dy, const float* x, int ld_x, const float* y, int ld_y, int n, int C,
                               const float* gamma, const float* save_mean, const float* save_invstd, int train, int relu, float* dx,
                               int ld_dx, float* dres, int ld_dres, float* dgamma, float* dbeta, void* scratch, size_t scratch_bytes,
                               void* stream);

/* The backward scaling of umereg_sparse_conv_f16.h for an output gradient dy (f32, `count` elements, contiguous, 16-byte
 * aligned; count == 0 allowed): e = 14 - floor(log2(max |dy|)) held to [-126, 126], e = 0 if the maximum is zero or not finite
 * (a NaN anywhere counts as not finite); out_e (int32), out_up = 2^e and out_down = 2^-e (f32, made from the exponent field) are
 * device scalars.  One maximum per chunk of the tensor, then one finishing workgroup; nothing is read back to the host. */
size_t umereg_grad_scale_scratch_bytes(size_t count);
int umereg_grad_scale_f32(const float* dy, size_t count, int32_t* out_e, float* out_up, float* out_down, void* scratch,
                          size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
