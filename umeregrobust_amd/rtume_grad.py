"""The RTUME solve as a differentiable torch op, on the HIP backward kernel of include/umereg_rtume_grad.h: what
`cube_loss.CubeRegistrationLoss` is made of.

    T = rtume_solve(G, H)       # G, H [n, 32, 4] -> T [n, 4, 4] (source -> target); gradient with respect to both

Forward values are those of `ops.rtume_solve` (the same call, the same bits).  The backward saves nothing but G and H: the kernel
forms the forward's quantities again in fp64 and differentiates the rotation itself (no 1 / (s_i^2 - s_j^2) as autograd through an
SVD has it), so repeated singular values are harmless.  A pair of singular directions whose signed values sum to no more than
MIN_GAP times the largest contributes nothing (include/umereg_rtume_grad.h states the convention).  The backward is deterministic
bit for bit, runs on the current stream and never waits for the device."""
import torch

from . import _lib, ops

RTUME_GRAD_SIGNATURES = _lib.TABLES["umereg_rtume_grad.h"]
load_native = _lib.load
_on_gpu = _lib.on_gpu

MIN_GAP = 1e-8      # UMEREG_RTUME_BWD_MIN_GAP: s'_i + s'_j <= MIN_GAP * s1 -> the pair (i, j) has no gradient


def _check_shapes(who, G, H):
    if G.dim() != 3 or tuple(G.shape[1:]) != (32, 4) or H.shape != G.shape:
        raise ValueError(f"{who}: G and H [n, 32, 4] expected, got {tuple(G.shape)} / {tuple(H.shape)}")


def rtume_bwd_raw(G, H, dT, need_g=True, need_h=True):
    """(dG, dH) of T = rtume_solve(G, H) for upstream dT [n, 4, 4]; a side that is not needed is None."""
    lib = _lib.load()
    _on_gpu("rtume_solve backward", G, H, dT)
    _check_shapes("rtume_solve backward", G, H)
    n = G.shape[0]
    if tuple(dT.shape) != (n, 4, 4):
        raise ValueError(f"rtume_solve backward: dT [n, 4, 4] expected, got {tuple(dT.shape)} for n = {n}")
    G, H, dT = G.float().contiguous(), H.float().contiguous(), dT.float().contiguous()
    dG = torch.empty_like(G) if need_g else None
    dH = torch.empty_like(H) if need_h else None
    if n == 0 or not (need_g or need_h):
        return dG, dH
    _lib.call(G.device, lib.umereg_rtume_solve_bwd_f32, G.data_ptr(), H.data_ptr(), dT.data_ptr(), n, dG.data_ptr() if need_g else None,
              dH.data_ptr() if need_h else None, _lib.stream_ptr(G.device))
    return dG, dH


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, H):
        T = ops.rtume_solve(G.detach(), H.detach())[0]
        ctx.save_for_backward(G, H)
        return T

    @staticmethod
    def backward(ctx, dT):
        G, H = ctx.saved_tensors
        return rtume_bwd_raw(G, H, dT, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def rtume_solve(G, H):
    """Differentiable `ops.rtume_solve` without index arrays (reference utils/loc_utils.py:292-350): G (source), H (target)
    [n, 32, 4] -> T [n, 4, 4].  n = 0 gives empty tensors, forward and backward, without a launch."""
    _on_gpu("rtume_solve", G, H)
    _check_shapes("rtume_solve", G, H)
    return _Solve.apply(G, H)
