"""The point-wise InfoNCE loss of the reference (loss.py:19-46) as one differentiable op on the fused HIP kernels of
include/umereg_infonce.h: what `pw_loss.MyInfoNCELossNoSeg` is made of.

    loss = infonce_loss(src_feat, src_pts, tgt_feat, matches, tau, neg_euclid_dist)      # scalar; gradient to the two feature tensors

src_feat f32 [B, N, 32], src_pts f32 [B, N, 3], tgt_feat f32 [B, M, 32], matches int64 [B, S, 2].  The forward keeps two floats per
sample (`row_stats`: the row's log-sum-exp and its cosine similarity); the backward recomputes every weight from them.  No S x S
tensor exists at any time, nothing is gathered into a copy, and both passes are deterministic bit for bit, run on the current stream
and never wait for the device.  The row sum runs under a running maximum, so logits / tau above 88 -- where the torch form returns
inf / inf = NaN -- give a finite loss.  A `matches` entry out of range is not read through: the loss is NaN."""
import torch

from . import _lib

INFONCE_SIGNATURES = _lib.TABLES["umereg_infonce.h"]
load_native = _lib.load

D = 32              # UMEREG_INFONCE_D
MAX_S = 8192        # UMEREG_INFONCE_MAX_S


def _inputs(who, src_feat, src_pts, tgt_feat, matches):
    """The four inputs as the kernels read them (contiguous; the features 16-byte aligned) and (B, N, M, S).  Shapes and types are
    judged first, then the device."""
    for t in (src_feat, src_pts, tgt_feat, matches):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: expected torch tensors, got {type(t).__name__}")
    if src_feat.dim() != 3 or tgt_feat.dim() != 3 or src_feat.shape[2] != D or tgt_feat.shape[2] != D:
        raise ValueError(f"{who}: features must be [B, N, {D}] and [B, M, {D}], got {tuple(src_feat.shape)} / {tuple(tgt_feat.shape)}")
    if src_feat.dtype != torch.float32 or tgt_feat.dtype != torch.float32 or src_pts.dtype != torch.float32:
        raise ValueError(f"{who}: features and points must be float32, got {src_feat.dtype} / {tgt_feat.dtype} / {src_pts.dtype}")
    if matches.dtype != torch.int64:
        raise ValueError(f"{who}: matches must be int64, got {matches.dtype}")
    B, N = src_feat.shape[:2]
    M = tgt_feat.shape[1]
    if tuple(src_pts.shape) != (B, N, 3) or tgt_feat.shape[0] != B or matches.dim() != 3 or matches.shape[0] != B or matches.shape[2] != 2:
        raise ValueError(f"{who}: src_pts [B, N, 3], tgt_feat [B, M, {D}] and matches [B, S, 2] expected for src_feat {tuple(src_feat.shape)}, "
                         f"got {tuple(src_pts.shape)} / {tuple(tgt_feat.shape)} / {tuple(matches.shape)}")
    S = matches.shape[1]
    if S > MAX_S:
        raise ValueError(f"{who}: S = {S} samples; at most {MAX_S} are supported")
    _lib.on_gpu(who, src_feat, src_pts, tgt_feat, matches)

    def flat(t):
        t = t.contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    return flat(src_feat), flat(src_pts), flat(tgt_feat), flat(matches), (B, N, M, S)


def _workspace(lib, dev, sizes, workspace):
    need = int(lib.umereg_infonce_workspace_bytes(*sizes))
    if need == 0:
        raise ValueError("infonce: sizes B = {}, N = {}, M = {}, S = {} not supported".format(*sizes))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    return workspace


def infonce_fwd_raw(src_feat, src_pts, tgt_feat, matches, tau, neg_euclid_dist, workspace=None):
    """(loss f32 [1], row_stats f32 [B, S, 2]) on the device.  B, N, M, S >= 1."""
    lib = load_native()
    src_feat, src_pts, tgt_feat, matches, sizes = _inputs("infonce forward", src_feat, src_pts, tgt_feat, matches)
    dev = src_feat.device
    workspace = _workspace(lib, dev, sizes, workspace)
    row_stats = torch.empty(sizes[0], sizes[3], 2, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call(dev, lib.umereg_infonce_fwd_f32, src_feat.data_ptr(), src_pts.data_ptr(), tgt_feat.data_ptr(), matches.data_ptr(), *sizes,
              float(tau), float(neg_euclid_dist), row_stats.data_ptr(), loss.data_ptr(), workspace.data_ptr(), workspace.numel(),
              _lib.stream_ptr(dev))
    return loss, row_stats


def infonce_bwd_raw(src_feat, src_pts, tgt_feat, matches, tau, neg_euclid_dist, row_stats, dloss, need_src=True, need_tgt=True,
                    workspace=None):
    """(dsrc f32 [B, N, 32], dtgt f32 [B, M, 32]) for the upstream gradient `dloss` (a device tensor of one element, never read by the
    host); a side that is not needed is None and is not computed."""
    lib = load_native()
    src_feat, src_pts, tgt_feat, matches, sizes = _inputs("infonce backward", src_feat, src_pts, tgt_feat, matches)
    _lib.on_gpu("infonce backward", row_stats, dloss)
    B, N, M, S = sizes
    if tuple(row_stats.shape) != (B, S, 2) or row_stats.dtype != torch.float32 or dloss.numel() != 1:
        raise ValueError(f"infonce backward: row_stats f32 [B, S, 2] and a one-element dloss expected, got {row_stats.dtype} "
                         f"{tuple(row_stats.shape)} / {tuple(dloss.shape)}")
    if not (need_src or need_tgt):
        return None, None
    dev = src_feat.device
    row_stats, dloss = row_stats.contiguous(), dloss.reshape(1).float().contiguous()
    workspace = _workspace(lib, dev, sizes, workspace)
    dsrc = torch.empty(B, N, D, dtype=torch.float32, device=dev) if need_src else None
    dtgt = torch.empty(B, M, D, dtype=torch.float32, device=dev) if need_tgt else None
    _lib.call(dev, lib.umereg_infonce_bwd_f32, src_feat.data_ptr(), src_pts.data_ptr(), tgt_feat.data_ptr(), matches.data_ptr(), *sizes,
              float(tau), float(neg_euclid_dist), row_stats.data_ptr(), dloss.data_ptr(), _lib.ptr(dsrc), _lib.ptr(dtgt),
              workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(dev))
    return dsrc, dtgt


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src_feat, src_pts, tgt_feat, matches, tau, neg_euclid_dist):
        loss, row_stats = infonce_fwd_raw(src_feat.detach(), src_pts, tgt_feat.detach(), matches, tau, neg_euclid_dist)
        ctx.tau, ctx.neg_euclid_dist = tau, neg_euclid_dist
        ctx.save_for_backward(src_feat, src_pts, tgt_feat, matches, row_stats)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        src_feat, src_pts, tgt_feat, matches, row_stats = ctx.saved_tensors
        dsrc, dtgt = infonce_bwd_raw(src_feat, src_pts, tgt_feat, matches, ctx.tau, ctx.neg_euclid_dist, row_stats, dloss,
                                     ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        return dsrc, None, dtgt, None, None, None


def infonce_loss(src_feat, src_pts, tgt_feat, matches, tau, neg_euclid_dist):
    """Differentiable fused InfoNCE (module docstring).  The gradient reaches `src_feat` and `tgt_feat`; points and matches are data.
    S == 0 gives NaN without a launch, as the mean of nothing does in the torch form."""
    who = "infonce_loss"
    src_feat, src_pts, tgt_feat, matches, sizes = _inputs(who, src_feat, src_pts, tgt_feat, matches)
    if src_pts.requires_grad:
        raise RuntimeError(f"{who}: no gradient with respect to the points; detach them")
    if sizes[3] == 0:
        nan = torch.full((), float("nan"), dtype=torch.float32, device=src_feat.device)
        # (an empty sum keeps the graph: zero gradients, as the torch form's gathers of nothing give)
        return nan + (src_feat[:, :0].sum() + tgt_feat[:, :0].sum())
    if min(sizes) < 1:
        raise ValueError("{}: B, N and M must be at least 1, got B = {}, N = {}, M = {}".format(who, *sizes[:3]))
    return _InfoNCE.apply(src_feat, src_pts, tgt_feat, matches, float(tau), float(neg_euclid_dist))
