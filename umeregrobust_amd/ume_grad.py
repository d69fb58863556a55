"""UME moments and the UME subspace distance as differentiable torch ops, on the HIP backward kernels of
include/umereg_ume_grad.h: what `ume_loss.UMEContrastiveLoss` is made of.

    F = ume_moments(pts, kpts, feat, K, radius, normalize=True)     # [B, n, 32, 4]; gradient with respect to feat only
    D = ume_cdist(ume1, ume2)                                       # [B, n1, n2]; gradient with respect to both

Forward values are those of `ops.ume_moments` / `ops.ume_cdist` (the same calls).  The moments' backward reads the
neighbour lists the forward wrote (`return_idx=True`), never a second ball search; the distance's backward reads the D the
forward returned.  A pair with D <= D_MIN has no gradient and contributes nothing (torch's cdist backward gives 0 there too).
Both backward passes are deterministic bit for bit, run on the current stream and never wait for the device."""
import torch

from . import _lib, ops

UME_GRAD_SIGNATURES = _lib.TABLES["umereg_ume_grad.h"]
load_native = _lib.load
_on_gpu = _lib.on_gpu

D_MIN = 4e-3        # UMEREG_UME_CDIST_BWD_DMIN: at or below it a pair has no gradient (the forward's noise floor at D = 0)
MAX_K = 7680        # UMEREG_UME_GRAD_MAX_K


def _scratch(dev, nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def moments_bwd_raw(pts, feat, nn_idx, F, dF, normalize=True, scratch=None):
    """dfeat f32 [B, N, 32] of the moments whose forward wrote `nn_idx` (int64 [B, n, K]) and `F`; dF: f32 [B, n, 32, 4].
    `feat` and `F` are read by the normalised form only."""
    lib = _lib.load()
    _on_gpu("ume_moments backward", pts, nn_idx, dF)
    pts, dF = pts.float().contiguous(), dF.float().contiguous()
    nn_idx = nn_idx.contiguous()
    B, N, _ = pts.shape
    n, K = nn_idx.shape[1:]
    if nn_idx.dtype != torch.int64 or nn_idx.shape[0] != B or tuple(dF.shape) != (B, n, 32, 4):
        raise ValueError(f"ume_moments backward: nn_idx int64 [B, n, K] and dF [B, n, 32, 4] expected, got {nn_idx.dtype} "
                         f"{tuple(nn_idx.shape)} / {tuple(dF.shape)}")
    if normalize:
        _on_gpu("ume_moments backward", feat, F)
        feat, F = feat.float().contiguous(), F.float().contiguous()
        if tuple(feat.shape) != (B, N, 32) or F.shape != dF.shape:
            raise ValueError(f"ume_moments backward: feat [B, N, 32] and F [B, n, 32, 4] expected, got {tuple(feat.shape)} / {tuple(F.shape)}")
    dfeat = torch.empty(B, N, 32, dtype=torch.float32, device=pts.device)
    if n == 0 or N == 0 or B == 0:
        return dfeat.zero_()
    need = int(lib.umereg_ume_moments_bwd_scratch_bytes(B, N, n))
    if need == 0:
        raise ValueError(f"ume_moments backward: sizes B = {B}, N = {N}, n = {n} not supported")
    if scratch is None:
        scratch = _scratch(pts.device, need)
    _lib.call(pts.device, lib.umereg_ume_moments_bwd_f32, pts.data_ptr(), feat.data_ptr() if normalize else None, nn_idx.data_ptr(),
              F.data_ptr() if normalize else None, dF.data_ptr(), B, N, n, K, int(bool(normalize)), dfeat.data_ptr(), scratch.data_ptr(),
              scratch.numel(), _lib.stream_ptr(pts.device))
    return dfeat


def cdist_bwd_raw(ume1, ume2, D, dD, need1=True, need2=True, scratch=None):
    """(dume1, dume2) of D = ume_cdist(ume1, ume2) for upstream dD; a side that is not needed is None.  ume [B, n, 32, 4]."""
    lib = _lib.load()
    _on_gpu("ume_cdist backward", ume1, ume2, D, dD)
    ume1, ume2 = ume1.float().contiguous(), ume2.float().contiguous()
    D, dD = D.float().contiguous(), dD.float().contiguous()
    B, n1 = ume1.shape[:2]
    n2 = ume2.shape[1]
    if tuple(D.shape) != (B, n1, n2) or D.shape != dD.shape:
        raise ValueError(f"ume_cdist backward: D and dD [B, n1, n2] expected, got {tuple(D.shape)} / {tuple(dD.shape)}")
    d1 = torch.empty_like(ume1) if need1 else None
    d2 = torch.empty_like(ume2) if need2 else None
    if not (need1 or need2) or B == 0 or n1 == 0 or n2 == 0:
        return (None if d1 is None else d1.zero_()), (None if d2 is None else d2.zero_())
    need = int(lib.umereg_ume_cdist_bwd_scratch_bytes(n1, n2))
    if need == 0:
        raise ValueError(f"ume_cdist backward: sizes n1 = {n1}, n2 = {n2} not supported")
    if scratch is None:
        scratch = _scratch(ume1.device, need)
    st = _lib.stream_ptr(ume1.device)
    with torch.cuda.device(ume1.device):
        for b in range(B):      # one launch chain per batch element, like the forward; the scratch is reused in stream order
            _lib.checked(lib.umereg_ume_cdist_bwd_f32, ume1[b].data_ptr(), ume2[b].data_ptr(), D[b].data_ptr(), dD[b].data_ptr(), n1, n2,
                         d1[b].data_ptr() if need1 else None, d2[b].data_ptr() if need2 else None, scratch.data_ptr(), scratch.numel(), st)
    return d1, d2


class _Moments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, kpts, feat, K, radius, normalize):
        F, nn_idx = ops.ume_moments(pts, kpts, feat.detach(), K, radius, return_idx=True, normalize=normalize)
        ctx.normalize = bool(normalize)
        ctx.save_for_backward(pts, feat, nn_idx, F)
        return F

    @staticmethod
    def backward(ctx, dF):
        pts, feat, nn_idx, F = ctx.saved_tensors
        dfeat = moments_bwd_raw(pts, feat, nn_idx, F, dF, ctx.normalize) if ctx.needs_input_grad[2] else None
        return None, None, dfeat, None, None, None


class _Cdist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ume1, ume2):
        D = ops.ume_cdist(ume1.detach(), ume2.detach())
        ctx.save_for_backward(ume1, ume2, D)
        return D

    @staticmethod
    def backward(ctx, dD):
        ume1, ume2, D = ctx.saved_tensors
        return cdist_bwd_raw(ume1, ume2, D, dD, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def ume_moments(pts, kpts, feat, K, radius, normalize=True):
    """Differentiable `ops.ume_moments`: pts [B, N, 3], kpts [B, n, 3], feat [B, N, 32] -> F [B, n, 32, 4].  The gradient
    reaches `feat`; points and keypoints are data (a point or keypoint tensor that requires grad is refused)."""
    _on_gpu("ume_moments", pts, kpts, feat)
    if pts.requires_grad or kpts.requires_grad:
        raise RuntimeError("ume_moments: no gradient with respect to points or keypoints; detach them")
    if feat.dim() != 3 or feat.shape[2] != 32:
        raise ValueError(f"ume_moments: feat must be [B, N, 32], got {tuple(feat.shape)}")
    if not 0 < int(K) <= MAX_K:
        raise ValueError(f"ume_moments: K must be in [1, {MAX_K}], got {K}")
    return _Moments.apply(pts, kpts, feat, int(K), float(radius), bool(normalize))


def ume_cdist(ume1, ume2):
    """Differentiable `ops.ume_cdist` (reference utils/loc_utils.py:8-15): ume1 [B, n1, 32, 4], ume2 [B, n2, 32, 4] -> D [B, n1, n2]."""
    _on_gpu("ume_cdist", ume1, ume2)
    return _Cdist.apply(ume1, ume2)
