"""Time the UME contrastive loss and its HIP backward kernels; one JSON line per shape.

    python tools/ume_loss_time.py [--out profiles/ume_loss/ume_loss_time.jsonl] [--iters 20] [--warmup 5]

Every figure is the median over `--iters` launches, each bracketed by its own pair of device events on the launch stream,
after `--warmup` launches of the same shape.

  * `trainer`: the shape of the reference's KITTI training config (batch 8, ume_n_samples 256, ume_max_nn 750, ume_r_nn 5) on
    synthetic 50 000-point clouds: moments forward / backward, distance forward / backward (all 8 batch elements), the
    part of the loss a gradient flows through (both moments, distance, softmax; forward + backward) on the HIP operators
    and composed from torch ops on the same GPU (gather of [B, n, K, 32], torch.linalg.qr, torch.cdist, autograd) on the
    same neighbour lists, and the whole `UMEContrastiveLoss` forward + backward including the keypoint selection.
  * `matcher`: the distance backward alone at n1 = n2 = 10 000 (both sides), with its share of the f32 matrix rate:
    4096 n1 n2 flop (two 32 x 32 x 32 products per pair of keypoint octets and side) over PEAK_FP32_MATRIX.

`--profile-steps N`: N loss steps at the trainer's shape and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats -d DIR -o ume_loss -- python tools/ume_loss_time.py --profile-steps 3`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from umeregrobust_amd import ops, ume_grad                    # noqa: E402
from umeregrobust_amd.ume_loss import UMEContrastiveLoss      # noqa: E402

PEAK_FP32_MATRIX = 155e12
TRAINER = dict(B=8, N=50000, n=256, K=750, r=5.0)


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def trainer_clouds(dev, seed=0):
    """B source clouds in a 100 x 100 x 8 m box, the target a rotated and shifted copy with 3 cm noise; features a smooth positive
    function of position plus noise"""
    g = torch.Generator().manual_seed(seed)
    B, N = TRAINER["B"], TRAINER["N"]
    src = torch.rand(B, N, 3, generator=g) * torch.tensor([100.0, 100.0, 8.0])
    a = 0.3
    R = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    t = torch.tensor([2.0, -1.0, 0.3])
    gt = torch.eye(4).repeat(B, 1, 1)
    gt[:, :3, :3], gt[:, :3, 3] = R, t
    tgt = src @ R.T + t + 0.03 * torch.randn(B, N, 3, generator=g)
    W = torch.randn(3, 32, generator=g) * 0.1
    feat = lambda p: 0.55 + 0.5 * torch.sin(p @ W + torch.arange(32.0)) + 0.02 * torch.randn(B, N, 32, generator=g)     # noqa: E731
    seg = torch.zeros(B, N, 1, dtype=torch.int64)
    return [x.to(dev) for x in (src, seg, feat(src), tgt, feat(src), gt)]


def softmax_loss(D, tau=0.1):
    sim = (2.0 - 2 * D) / 2.0
    e = torch.exp(sim / tau)
    return (-torch.log(torch.diagonal(e / e.sum(dim=-1, keepdim=True), dim1=-1, dim2=-2))).mean()


def torch_moments(pts, feat, nn_idx):
    B = pts.shape[0]
    valid = (nn_idx >= 0)[..., None].float()
    idx = nn_idx.clamp_min(0)
    bi = torch.arange(B, device=pts.device)[:, None, None]
    f = feat[bi, idx] * valid                                                   # [B, n, K, 32]
    h = torch.cat([torch.ones_like(pts[..., :1]), pts], -1)[bi, idx]            # [B, n, K, 4]
    Fr = f.transpose(-1, -2) @ h
    return Fr / (Fr[..., 0].sum(dim=-1)[..., None, None] + 1e-6)


def torch_cdist(u1, u2):
    Q1, Q2 = torch.linalg.qr(u1).Q, torch.linalg.qr(u2).Q
    return torch.cdist((Q1 @ Q1.transpose(-1, -2)).flatten(2), (Q2 @ Q2.transpose(-1, -2)).flatten(2)) / np.sqrt(2)


def run_trainer(dev, iters, warmup):
    K, r, n = TRAINER["K"], TRAINER["r"], TRAINER["n"]
    src, seg, sf, tgt, tf, gt = trainer_clouds(dev)
    g = torch.Generator().manual_seed(1)
    kp_rows = torch.stack([torch.randperm(TRAINER["N"], generator=g)[:n] for _ in range(TRAINER["B"])]).to(dev)
    kp = torch.gather(src, 1, kp_rows[..., None].expand(-1, -1, 3)).contiguous()
    kp_t = (kp @ gt[0, :3, :3].T + gt[0, :3, 3]).contiguous()
    F, nn_idx = ops.ume_moments(src, kp, sf, K, r, return_idx=True)
    F_t, nn_t = ops.ume_moments(tgt, kp_t, tf, K, r, return_idx=True)
    D = ops.ume_cdist(F, F_t)
    G, gD = torch.randn_like(F), torch.randn_like(D)
    out = dict(shape="trainer", **TRAINER, neighbours_mean=float((nn_idx >= 0).sum(-1).float().mean()), iters=iters)
    out["moments_fwd_ms"] = median_ms(lambda: ops.ume_moments(src, kp, sf, K, r, return_idx=True), iters, warmup)
    out["moments_bwd_ms"] = median_ms(lambda: ume_grad.moments_bwd_raw(src, sf, nn_idx, F, G), iters, warmup)
    out["dist_fwd_ms"] = median_ms(lambda: ops.ume_cdist(F, F_t), iters, warmup)
    out["dist_bwd_ms"] = median_ms(lambda: ume_grad.cdist_bwd_raw(F, F_t, D, gD), iters, warmup)

    def hip_part():
        a, b = sf.detach().requires_grad_(), tf.detach().requires_grad_()
        softmax_loss(ume_grad.ume_cdist(ume_grad.ume_moments(src, kp, a, K, r), ume_grad.ume_moments(tgt, kp_t, b, K, r))).backward()
        return a.grad

    def torch_part():
        a, b = sf.detach().requires_grad_(), tf.detach().requires_grad_()
        softmax_loss(torch_cdist(torch_moments(src, a, nn_idx), torch_moments(tgt, b, nn_t))).backward()
        return a.grad

    out["loss_part_hip_ms"] = median_ms(hip_part, iters, warmup)
    try:
        out["loss_part_torch_ms"] = median_ms(torch_part, max(3, iters // 4), 2)
        ga, gb = hip_part(), torch_part()
        out["loss_part_grad_rel_diff"] = float((ga - gb).abs().max() / gb.abs().max())
    except RuntimeError as e:       # (out of memory, or an op the torch build lacks): reported, not hidden
        out["loss_part_torch_ms"] = None
        out["loss_part_torch_error"] = str(e).splitlines()[0][:200]
    fn = UMEContrastiveLoss(num_samples=n, max_nn=K, min_nn=100, nn_r=r, flat_labels=[9])

    def whole():
        a, b = sf.detach().requires_grad_(), tf.detach().requires_grad_()
        res = fn(src, seg, a, tgt, b, gt)
        res[0].backward()
        return res

    res = whole()
    out["whole_loss_keypoints"] = int(res[3].shape[1])
    out["whole_loss_value"] = float(res[0].detach())
    out["whole_loss_fwd_bwd_ms"] = median_ms(whole, max(3, iters // 4), 2)
    return out


def run_matcher(dev, iters, warmup, n=10000):
    g = torch.Generator().manual_seed(2)
    u1 = (torch.randn(1, n, 32, 4, generator=g) * torch.tensor([1.0, 6.0, 6.0, 1.5])).to(dev)
    u2 = (torch.randn(1, n, 32, 4, generator=g) * torch.tensor([1.0, 6.0, 6.0, 1.5])).to(dev)
    D = ops.ume_cdist(u1, u2)
    gD = torch.randn_like(D)
    scratch = torch.empty(int(ume_grad.load_native().umereg_ume_cdist_bwd_scratch_bytes(n, n)), dtype=torch.uint8, device=dev)
    out = dict(shape="matcher", n1=n, n2=n, iters=iters, scratch_mib=scratch.numel() / 2 ** 20)
    out["dist_fwd_ms"] = median_ms(lambda: ops.ume_cdist(u1, u2), iters, warmup)
    both = median_ms(lambda: ume_grad.cdist_bwd_raw(u1, u2, D, gD, scratch=scratch), iters, warmup)
    one = median_ms(lambda: ume_grad.cdist_bwd_raw(u1, u2, D, gD, need2=False, scratch=scratch), iters, warmup)
    flop = 4096.0 * n * n
    out.update(dist_bwd_ms=both, dist_bwd_one_side_ms=one, flop=flop, tflops=flop / both / 1e9,
               share_of_f32_matrix_rate=flop / (both * 1e-3) / PEAK_FP32_MATRIX, floor_ms=flop / PEAK_FP32_MATRIX * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ume_loss",
                                                  "ume_loss_time.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ume_loss_time: no HIP device visible; a time is a measurement on the GPU")
    dev = torch.device("cuda:0")
    if args.profile_steps:
        src, seg, sf, tgt, tf, gt = trainer_clouds(dev)
        fn = UMEContrastiveLoss(num_samples=TRAINER["n"], max_nn=TRAINER["K"], min_nn=100, nn_r=TRAINER["r"], flat_labels=[9])
        for _ in range(args.profile_steps):
            a, b = sf.detach().requires_grad_(), tf.detach().requires_grad_()
            fn(src, seg, a, tgt, b, gt)[0].backward()
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for run in (run_trainer, run_matcher):
            line = json.dumps(run(dev, args.iters, args.warmup))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
