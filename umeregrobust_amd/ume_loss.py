"""`UMEContrastiveLoss` of the reference (loss.py:49-118) on the differentiable UME operators of `ume_grad`.

The trainer forms it beside the point-wise loss (train_coloring.py:47-60):

    ume_fn = UMEContrastiveLoss(num_samples=256, max_nn=750, min_nn=..., nn_r=5, flat_labels=[...])
    loss_ume, velo_kp, ref_kp, velo_ume, ref_ume, ratio, with_kpts = ume_fn(velo_pts, velo_seg, velo_feat, ref_pts, ref_feat, gt_tform)
    loss = (1 - w) * loss_infonce + w * loss_ume

Keypoint selection, the validity mask and the intersection ratio carry no gradient in the reference either (indices, counts
and comparisons); they run on `utils.loc_utils.generate_ume_from_keypoints2` and `ops.ume_svdvals`.  The UME matrices of the
selected keypoints are then formed by `ume_grad.ume_moments`, so that the graph reaches `velo_feat` and `ref_feat`, their
distances by `ume_grad.ume_cdist`, and the softmax over n_samples x n_samples is plain torch in the reference's order of
operations.  (`loss.UMEContrastiveLoss` is still the refusing stub; this module is where the working class lives.)"""
import numpy as np
import torch
from torch import nn

from . import gt_keypoints, ops, ume_grad
from .utils.loc_utils import generate_ume_from_keypoints2


class UMEContrastiveLoss(nn.Module):
    """forward(velo_pts [B, N, 3], velo_seg [B, N, 1], velo_feat [B, N, 32], ref_pts [B, M, 3], ref_feat [B, M, 32],
    gt_tform [B, 4, 4]) -> (loss, velo_keypoint_pts, ref_keypoint_pts, velo_ume, ref_ume, matched_nn_intersection_ratio,
    with_kpts_batch_cond), as the reference returns them."""

    def __init__(self, num_samples=1024, max_nn=5000, min_nn=1000, nn_r=10, tau=0.1, tau_neg=0.1, hd_labels_flag=False,
                 flat_labels=[], nn_intersection_r=0.6, svd_thr=1e-5):
        super().__init__()
        self.selection = "torch"        # the keypoint generator's engine; `with_selection` changes it (the constructor is the reference's)
        self.n_samples = num_samples
        self.max_nn = max_nn
        self.min_nn = min_nn
        self.nn_r = nn_r
        self.tau = tau
        self.tau_neg = tau_neg
        self.hd_labels_flag = hd_labels_flag
        self.flat_labels = flat_labels
        self.nn_intersection_r = nn_intersection_r
        self.svd_thr = svd_thr

    def with_selection(self, selection):
        """selection="torch" | "device": the engine of generate_ume_from_keypoints2 (same keypoints and values either way); -> self.
        Anything else is a ValueError.  Not a constructor argument: the constructor's signature stays the reference's."""
        gt_keypoints.check_selection("UMEContrastiveLoss", selection)
        self.selection = selection
        return self

    def forward(self, velo_pts, velo_seg, velo_feat, ref_pts, ref_feat, gt_tform):
        for t in (velo_pts, velo_seg, velo_feat, ref_pts, ref_feat, gt_tform):
            if t.device.type != "cuda":
                raise RuntimeError("UMEContrastiveLoss: CPU tensors given; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
        with torch.no_grad():
            F_velo, F_ref, velo_keypoint_pts, ref_keypoint_pts, matched_nn_intersection_ratio, with_kpts_batch_cond = \
                generate_ume_from_keypoints2(velo_pts, velo_seg, velo_feat.detach(), ref_pts, ref_feat.detach(), gt_tform,
                                             num_samples=self.n_samples, max_nn=self.max_nn, min_nn=self.min_nn, nn_r=self.nn_r,
                                             flat_labels=self.flat_labels, normalized_ume=True,
                                             nn_intersection_r=self.nn_intersection_r, selection=self.selection)
            # valid UME matrices (loss.py:83-97): all four singular values above the threshold, in both clouds
            valid = ((ops.ume_svdvals(F_velo) > self.svd_thr).sum(dim=-1) == 4) & ((ops.ume_svdvals(F_ref) > self.svd_thr).sum(dim=-1) == 4)
            invalid_keypoints_velo = torch.zeros_like(F_velo[0, :, 0, 0]).bool()
            invalid_keypoints_velo[torch.where(~valid)[1]] = True
            keep_kp = ~invalid_keypoints_velo
        if not bool(with_kpts_batch_cond.all()):      # batch elements without a keypoint were dropped (utils/loc_utils.py:129-141)
            keep = with_kpts_batch_cond
            velo_pts, velo_feat, ref_pts, ref_feat = velo_pts[keep], velo_feat[keep], ref_pts[keep], ref_feat[keep]
        # the same matrices again, this time with a graph behind them
        velo_ume = ume_grad.ume_moments(velo_pts.detach(), velo_keypoint_pts, velo_feat, self.max_nn, self.nn_r, normalize=True)
        ref_ume = ume_grad.ume_moments(ref_pts.detach(), ref_keypoint_pts, ref_feat, self.max_nn, self.nn_r, normalize=True)
        velo_ume = velo_ume[:, keep_kp]
        ref_ume = ref_ume[:, keep_kp]
        matched_nn_intersection_ratio = matched_nn_intersection_ratio[:, keep_kp]
        if velo_ume.shape[1] == 0:
            # no keypoint column survived: the reference's distance matrix of two empty sets is empty and its loss the mean of nothing
            # (NaN); the trainer tests `src_ume.shape[1] == 0` on what is returned here and skips the batch (train_coloring.py:50-52)
            D_ume = velo_ume.new_zeros(velo_ume.shape[0], 0, 0)
        else:
            D_ume = ume_grad.ume_cdist(velo_ume, ref_ume)                               # (bs, n_samples, n_samples)
        ume_rank = velo_ume.shape[-1]

        sim_ume = (np.sqrt(ume_rank) - 2 * D_ume) / (np.sqrt(ume_rank))
        tau_mat = self.tau_neg * torch.ones_like(sim_ume)
        pos_mask = torch.arange(D_ume.shape[-1], device=D_ume.device)[None] == \
            torch.arange(D_ume.shape[-1], device=D_ume.device)[None].T
        pos_mask = pos_mask[None].expand(D_ume.shape[0], -1, -1)
        tau_mat[pos_mask] = self.tau

        exp_sim_ume = torch.exp(sim_ume / tau_mat)
        loss = exp_sim_ume / exp_sim_ume.sum(dim=-1, keepdim=True)                      # (bs, n_samples, n_samples)
        loss = torch.diagonal(loss, dim1=-1, dim2=-2)                                   # (bs, n_samples)
        loss = -torch.log(loss)
        loss = loss.mean()
        return loss, velo_keypoint_pts, ref_keypoint_pts, velo_ume, ref_ume, matched_nn_intersection_ratio, with_kpts_batch_cond
