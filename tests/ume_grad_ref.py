"""Differentiable torch restatement of the UME contrastive loss (reference loss.py:49-118, utils/loc_utils.py:8-15 and
:146-162) from neighbour lists on: moments, reduced QR, projectors, cdist / sqrt(2), the softmax.  Runs in the dtype of its
inputs (fp64: the truth of the gradient tests; fp32: the yardstick of their gates); gradients come from autograd.  Nothing
here is shared with the library."""
import numpy as np
import torch


def moments(pts, feat, nn_idx, normalize=True):
    """pts [B, N, 3], feat [B, N, d], nn_idx int64 [B, n, K] (-1 padded) -> F [B, n, d, 4]:
    Fr_i[c, :] = sum_{j in N(i)} feat[j, c] * [1, p_j];  F_i = Fr_i / (sum_c Fr_i[c, 0] + 1e-6) if `normalize`."""
    B, N, d = feat.shape
    h = torch.cat([torch.ones_like(pts[..., :1]), pts], dim=-1)
    out = []
    for b in range(B):
        idx = nn_idx[b].long()
        valid = (idx >= 0).to(feat.dtype)[..., None]
        idx = idx.clamp_min(0)
        f = feat[b][idx] * valid                        # [n, K, d]
        Fr = torch.einsum("nkc,nke->nce", f, h[b][idx])
        if normalize:
            Fr = Fr / (Fr[..., 0].sum(dim=-1)[:, None, None] + 1e-6)
        out.append(Fr)
    return torch.stack(out)


def moments_grad(pts, feat, nn_idx, G, normalize=True, block=256):
    """d <moments(feat), G> / d feat by autograd, the keypoints in blocks (the sum over keypoints is additive)"""
    feat = feat.detach().clone().requires_grad_()
    n = nn_idx.shape[1]
    for i0 in range(0, n, block):
        (moments(pts, feat, nn_idx[:, i0:i0 + block], normalize) * G[:, i0:i0 + block]).sum().backward()
    return feat.grad if feat.grad is not None else torch.zeros_like(feat)


def projectors(ume):
    Q = torch.linalg.qr(ume, mode="reduced").Q
    return Q @ Q.transpose(-1, -2)


def ume_cdist(ume1, ume2):
    """the reference's ume_cdist: [B, n1, 32, 4], [B, n2, 32, 4] -> [B, n1, n2]"""
    return torch.cdist(projectors(ume1).flatten(2), projectors(ume2).flatten(2)) / np.sqrt(2)


def cdist_grads(ume1, ume2, g, drop=None):
    """(D, dume1, dume2) of <ume_cdist(ume1, ume2), g> by autograd; `drop`: bool [B, n1, n2], pairs whose terms are left out
    (their distance is replaced by a constant before the product)"""
    a, b = ume1.detach().clone().requires_grad_(), ume2.detach().clone().requires_grad_()
    D = ume_cdist(a, b)
    Dm = D if drop is None else torch.where(drop, torch.zeros_like(D), D)
    (Dm * g).sum().backward()
    return D.detach(), a.grad, b.grad


def contrastive(velo_ume, ref_ume, tau=0.1, tau_neg=0.1):
    """loss.py:98-116 on the UME matrices of the valid keypoints"""
    D = ume_cdist(velo_ume, ref_ume)
    rank = velo_ume.shape[-1]
    sim = (np.sqrt(rank) - 2 * D) / (np.sqrt(rank))
    tau_mat = tau_neg * torch.ones_like(sim)
    n = D.shape[-1]
    pos = torch.eye(n, dtype=torch.bool)[None].expand(D.shape[0], -1, -1)
    tau_mat[pos] = tau
    e = torch.exp(sim / tau_mat)
    p = e / e.sum(dim=-1, keepdim=True)
    return (-torch.log(torch.diagonal(p, dim1=-1, dim2=-2))).mean()


def loss_and_grads(velo_pts, velo_feat, velo_nn, ref_pts, ref_feat, ref_nn, tau=0.1, tau_neg=0.1):
    """(loss, d loss / d velo_feat, d loss / d ref_feat, velo_ume, ref_ume) on given neighbour lists, every keypoint valid"""
    a, b = velo_feat.detach().clone().requires_grad_(), ref_feat.detach().clone().requires_grad_()
    vu, ru = moments(velo_pts, a, velo_nn, True), moments(ref_pts, b, ref_nn, True)
    loss = contrastive(vu, ru, tau, tau_neg)
    loss.backward()
    return loss.detach(), a.grad, b.grad, vu.detach(), ru.detach()


def gate(got, truth, yard, name, log=print):
    """max |got - truth| <= 4 max |yard - truth| (got: the GPU's tensor, yard: this helper in fp32 on the CPU, truth: fp64);
    prints and returns the observed ratio"""
    truth = truth.double()
    e_gpu = float((got.detach().double().cpu() - truth).abs().max())
    e_cpu = float((yard.detach().double() - truth).abs().max())
    scale = float(truth.abs().max())
    ratio = e_gpu / e_cpu if e_cpu > 0 else (0.0 if e_gpu == 0 else float("inf"))
    log(f"[gate] {name}: max|gpu - fp64| {e_gpu:.3e}  max|fp32 cpu - fp64| {e_cpu:.3e}  ratio {ratio:.3f}  (max|truth| {scale:.3e})")
    assert np.isfinite(e_gpu), name
    assert e_gpu <= 4 * e_cpu, f"{name}: {e_gpu:.3e} > 4 x {e_cpu:.3e}"
    return ratio
