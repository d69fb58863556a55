"""`MyInfoNCELossNoSeg` of the reference (loss.py:10-46) on the fused HIP kernels of `infonce`: a drop-in for
`loss.MyInfoNCELossNoSeg` (same constructor, same `forward` signature, same scalar to fp32 rounding), the way
`ume_loss.UMEContrastiveLoss` is for its class.

    pw_fn = MyInfoNCELossNoSeg(num_samples=512, tau=0.1, neg_euclid_dist=5)
    loss_infonce = pw_fn(velo_feat, velo_pts, ref_feat, matches)

What differs from the torch class: no [B, S, S + 1] tensor is formed or kept for autograd (two floats per sample are), the row sum
runs under a running maximum (finite where the torch form overflows), `far` is evaluated from coordinate differences instead of
torch's matrix-product cdist (the two can differ only for a pair within rounding of `neg_euclid_dist`), and CPU tensors are refused.
`train_coloring.run(..., fused_pointwise=True)` selects it; `loss.MyInfoNCELossNoSeg` stays the default."""
from torch import nn

from .infonce import infonce_loss


class MyInfoNCELossNoSeg(nn.Module):
    """forward(velo_feat [B, N, 32], velo_pts [B, N, 3], ref_feat [B, M, 32], matches int64 [B, S, 2]) -> scalar.
    `num_samples` and `match_r` are kept for the reference's constructor; the forward pass does not use them."""

    def __init__(self, num_samples=2048, tau=0.1, match_r=0.1, neg_euclid_dist=5):
        super().__init__()
        self.num_samples, self.tau, self.match_r, self.neg_euclid_dist = num_samples, tau, match_r, neg_euclid_dist

    def forward(self, velo_feat, velo_pts, ref_feat, matches):
        return infonce_loss(velo_feat, velo_pts.detach(), ref_feat, matches, self.tau, self.neg_euclid_dist)
