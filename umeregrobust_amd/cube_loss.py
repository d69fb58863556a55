"""`CubeRegistrationLoss` of the reference (loss.py:121-190) on the differentiable RTUME solve of `rtume_grad`.

The trainer forms it from what `ume_loss.UMEContrastiveLoss` returns (train_coloring.py:48-58):

    reg_fn = CubeRegistrationLoss(rtume_max_nn=750, rtume_r_nn=5)
    loss_ume, velo_kp, ref_kp, velo_ume, ref_ume, ratio, with_kpts = ume_fn(...)
    loss_reg, rre, rte = reg_fn(velo_pts, velo_ume, ref_pts, ref_ume, gt_tform, ratio, with_kpts)
    loss = PW * loss_infonce + UME * loss_ume + REG * loss_reg

Keypoint i of the source is paired with keypoint i of the target (the reference's `reshape(-1, ...)` of [bs, n, 1, 32, 4] and
[bs, 1, n, 32, 4] does not broadcast: bs * n solves, not n^2).  Each pair's SE(3) comes from `rtume_grad.rtume_solve`, so the graph
reaches both UME tensors; the eight cube corners, the threshold on the intersection ratio and the mean are plain torch in the
reference's order of operations.  `rre` is `ops.rre_deg`, `rte` plain torch, both without a graph.  (`loss.CubeRegistrationLoss` is
still the refusing stub; this module is where the working class lives.)"""
import torch
from torch import nn

from . import ops, rtume_grad


class CubeRegistrationLoss(nn.Module):
    """forward(src_pts, src_ume [bs, n, 32, 4], tgt_pts, tgt_ume [bs, n, 32, 4], gt_tform [B, 4, 4], matched_nn_intersection_ratio
    [bs, n], valid_batch_entries bool [B] with bs entries set) -> (loss, rre [bs, n] in degrees, rte [bs, n]), as the reference
    returns them.  The point tensors are not read (nor are they in the reference); `rtume_max_nn` and `rtume_r_nn` are kept for
    the reference's constructor."""

    def __init__(self, rtume_max_nn, rtume_r_nn, cube_scale=1.0, nn_inter_ratio_thr=0.75):
        super().__init__()
        self.rtume_max_nn, self.rtume_r_nn = rtume_max_nn, rtume_r_nn
        unit_cube = torch.tensor([[-1, 1, 1],
                                  [1, 1, 1],
                                  [-1, -1, 1],
                                  [1, -1, 1],
                                  [-1, 1, -1],
                                  [1, 1, -1],
                                  [-1, -1, -1],
                                  [1, -1, -1]])
        self.points_cube = unit_cube.float() * cube_scale
        self.nn_inter_ratio_thr = nn_inter_ratio_thr

    def forward(self, src_pts, src_ume, tgt_pts, tgt_ume, gt_tform, matched_nn_intersection_ratio, valid_batch_entries):
        for t in (src_ume, tgt_ume, gt_tform, matched_nn_intersection_ratio, valid_batch_entries):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                raise RuntimeError("CubeRegistrationLoss: CPU tensors given; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
        gt_tform = gt_tform[valid_batch_entries]

        bs, n_hypotheses, _, _ = src_ume.shape
        device = src_ume.device
        self.points_cube = self.points_cube.to(device)

        # one RTUME solve per keypoint pair (loss.py:147-154)
        T = rtume_grad.rtume_solve(src_ume.reshape(-1, *src_ume.shape[2:]), tgt_ume.reshape(-1, *tgt_ume.shape[2:]))
        rtume_tform = T.view(bs, n_hypotheses, *T.shape[1:])

        R_rtume = rtume_tform[..., :3, :3]                                              # (bs, n, 3, 3)
        t_rtume = rtume_tform[..., :3, 3]                                               # (bs, n, 3)
        R_gt = gt_tform[:, :3, :3]
        t_gt = gt_tform[:, :3, 3]

        # the cube's corners under the estimate and under the ground truth (loss.py:161-169)
        src_estimated_tform_pts = self.points_cube[None, None].expand(bs, n_hypotheses, -1, -1) @ R_rtume.transpose(-1, -2) + \
            t_rtume.unsqueeze(-2)                                                       # (bs, n, 8, 3)
        src_gt_tform_pts = self.points_cube @ R_gt.transpose(-1, -2) + t_gt[:, None]    # (bs, 8, 3)
        src_gt_tform_pts = src_gt_tform_pts[:, None, ...].expand(-1, n_hypotheses, -1, -1)
        loss_src_to_tgt = (src_gt_tform_pts - src_estimated_tform_pts).norm(dim=-1)     # (bs, n, 8)
        loss_src_to_tgt = loss_src_to_tgt.mean(dim=-1)                                  # (bs, n)

        # keypoints whose neighbourhoods overlap enough; none at all: those at or above the row's median (loss.py:171-178)
        intersection_cond = matched_nn_intersection_ratio >= self.nn_inter_ratio_thr
        if intersection_cond.sum() == 0:
            intersection_cond = matched_nn_intersection_ratio >= matched_nn_intersection_ratio.median(dim=-1, keepdim=True)[0]
        loss = loss_src_to_tgt[intersection_cond].mean()

        with torch.no_grad():
            rre = ops.rre_deg(R_rtume.reshape(bs * n_hypotheses, 3, 3).contiguous(),
                              R_gt.unsqueeze(1).expand(-1, n_hypotheses, -1, -1).reshape(bs * n_hypotheses, 3, 3).contiguous()
                              ).view(bs, n_hypotheses)
            rte = (t_rtume.reshape(bs * n_hypotheses, 3) - t_gt.unsqueeze(1).expand(-1, n_hypotheses, -1).reshape(
                bs * n_hypotheses, 3)).norm(dim=-1).view(bs, n_hypotheses)
        return loss, rre, rte
