/* umereg_infonce.h -- C ABI of the fused InfoNCE point-wise loss, forward and backward (csrc/infonce.hip): what
 * `pw_loss.MyInfoNCELossNoSeg` runs in place of the torch statements of the reference's loss.py:19-46 (the gathers, the cosine
 * similarity, the S x S logit matrix, the cdist mask, the two exp tensors, the concatenation, the sum, the log and the mean, and
 * everything autograd keeps of them).  No S x S tensor is formed, forward or backward.
 *
 * Same conventions as umereg.h / umereg_ume_grad.h: outputs and workspace belong to the caller, every compute entry takes a HIP
 * stream (NULL = the default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a
 * device, returns UMEREG_ENODEV where no HIP device is visible, allocates nothing and never waits for the device.  The size query is
 * host arithmetic and returns 0 for arguments the compute entries refuse.  The entry points here are typed by their own table
 * (umeregrobust_amd/infonce.py: INFONCE_SIGNATURES).
 *
 * Contract.  Per batch element b and sample s, with i = matches[b][s][0] and j = matches[b][s][1]:
 *     a_s = src_feat[b][i],  x_s = src_pts[b][i],  p_s = tgt_feat[b][j]           (32 channels only)
 *     pos_s  = <a_s, p_s> / max(|a_s| |p_s|, 1e-8)
 *     l_st   = <a_s, p_t>                         for every t, t = s included (the mask below removes it, as in the reference)
 *     far_st = (dx dx + dy dy) + dz dz > r2       f32, one rounding per operation; r2 = (float)((double)neg_dist * neg_dist)
 *     row_s  = log(exp(pos_s / tau) + sum_t far_st exp(l_st / tau)) - pos_s / tau
 *     loss   = sum_s row_s / (B S)                every sum in one fixed order
 * `far` is the reference's `cdist(x, x) > neg_dist`.  torch forms cdist through a matrix product for S > 25, so the two may
 * disagree for a pair whose distance is within rounding of neg_dist, and only for such a pair; far_ss is false by construction
 * (0 > r2 never holds).  The row sum runs under a running maximum: where the reference's exp overflows for l / tau above 88 and its
 * loss becomes inf / inf = NaN, the result here stays finite.
 * A `matches` entry outside [0, N) x [0, M) is never dereferenced.  Its sample takes no part in the other rows' sums, and its own
 * row_s is NaN, so the loss is NaN.
 *
 * Both passes are deterministic: every sum runs in one fixed order, there is no floating-point atomic, and no result depends on what
 * the workspace or the outputs held. */
#ifndef UMEREG_INFONCE_H
#define UMEREG_INFONCE_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* feature channels */
#define UMEREG_INFONCE_D 32
/* largest S (kInfoNceMaxS of csrc/infonce_plan.h) */
#define UMEREG_INFONCE_MAX_S 8192

/* bytes of workspace either compute entry needs; 0 for B, N, M < 1, S < 1 or S > UMEREG_INFONCE_MAX_S */
size_t umereg_infonce_workspace_bytes(int B, int N, int M, int S);

/* Forward.  src_feat f32 [B][N][32], src_pts f32 [B][N][3], tgt_feat f32 [B][M][32], matches int64 [B][S][2]; tau > 0,
 * neg_dist >= 0.  row_stats f32 [B][S][2]: the row's log-sum-exp  log(exp(pos_s / tau) + sum_t far_st exp(l_st / tau))  and pos_s.
 * loss f32 [1].  Two launches: the rows, then the sum of their workgroups' partial sums (fp64, in workgroup order). */
int umereg_infonce_fwd_f32(const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches, int B, int N,
                           int M, int S, float tau, float neg_dist, float* row_stats, float* loss, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Backward.  The inputs of the forward, the row_stats it wrote, and dloss f32 [1] ON THE DEVICE (the upstream gradient g; the host
 * never reads it).  With w_st = far_st exp(l_st / tau - lse_s), w_s0 = exp(pos_s / tau - lse_s) and c = g / (B S tau):
 *     dA_s = c sum_t w_st p_t + c (w_s0 - 1) d pos_s / d a_s,      dP_t = c sum_s w_st a_s + c (w_t0 - 1) d pos_t / d p_t
 * dsrc f32 [B][N][32] and dtgt f32 [B][M][32] receive dA and dP at the rows `matches` names and are zero everywhere else (the call
 * zeroes them itself); a row named twice receives the sum of its samples in ascending s.  Either may be NULL (not both): that side is
 * not computed. */
int umereg_infonce_bwd_f32(const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches, int B, int N,
                           int M, int S, float tau, float neg_dist, const float* row_stats, const float* dloss, float* dsrc,
                           float* dtgt, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
