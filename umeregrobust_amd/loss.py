"""Training losses of the reference (loss.py) as far as this library can differentiate them.

`MyInfoNCELossNoSeg` -- the point-wise contrastive loss of the reference's trainer (train_coloring.py:44-45; loss.py:10-46) --
is plain torch on top of the feature network's differentiable output, with the reference's signature and the reference's
order of operations, so that fp32 values agree to rounding.  The working `UMEContrastiveLoss` lives in `ume_loss.py`, on the
differentiable UME moments and subspace distances of `ume_grad.py`, and the working `CubeRegistrationLoss` in `cube_loss.py`, on the
differentiable RTUME solve of `rtume_grad.py`; the two names here still refuse and point there."""
import torch
from torch import nn
from torch.nn import functional as tnf


class MyInfoNCELossNoSeg(nn.Module):
    """InfoNCE over matched points without segmentation labels.

    forward(velo_feat [B, N, d], velo_pts [B, N, 3], ref_feat [B, M, d], matches int64 [B, S, 2]) -> scalar.  Anchor s is
    source row matches[b, s, 0], its positive is target row matches[b, s, 1] (similarity: cosine); the negatives of anchor s
    are the positives of the anchors farther than `neg_euclid_dist` from it (similarity: dot product).
    loss = mean_s -log(exp(pos / tau) / (exp(pos / tau) + sum_negatives exp(dot / tau))).
    `num_samples` and `match_r` are kept for the reference's constructor; the forward pass does not use them."""

    def __init__(self, num_samples=2048, tau=0.1, match_r=0.1, neg_euclid_dist=5):
        super().__init__()
        self.num_samples, self.tau, self.match_r, self.neg_euclid_dist = num_samples, tau, match_r, neg_euclid_dist

    def forward(self, velo_feat, velo_pts, ref_feat, matches):
        d = velo_feat.shape[-1]
        src_rows, tgt_rows = matches[..., 0:1], matches[..., 1:2]
        anchors = velo_feat.gather(1, src_rows.expand(-1, -1, d))
        anchor_xyz = velo_pts.gather(1, src_rows.expand(-1, -1, 3))
        positives = ref_feat.gather(1, tgt_rows.expand(-1, -1, d))
        pos = tnf.cosine_similarity(anchors, positives, dim=-1).unsqueeze(-1)           # [B, S, 1]
        logits = torch.cat((pos, anchors @ positives.transpose(1, 2)), dim=2)           # [B, S, 1 + S]: positive first
        far = torch.cdist(anchor_xyz, anchor_xyz) > self.neg_euclid_dist                # (the diagonal is never far)
        keep = torch.cat((torch.ones_like(far[..., :1]), far), dim=-1)
        ratio = torch.exp(pos / self.tau) / (torch.exp(logits / self.tau) * keep).sum(dim=-1, keepdim=True)
        return (-torch.log(ratio)).mean()


class UMEContrastiveLoss(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("loss.UMEContrastiveLoss is out of scope of this module: the working class is "
                                  "umeregrobust_amd.ume_loss.UMEContrastiveLoss (same constructor, same return values)")


class CubeRegistrationLoss(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("loss.CubeRegistrationLoss is out of scope of this module: the working class is "
                                  "umeregrobust_amd.cube_loss.CubeRegistrationLoss (same constructor, same return values)")
