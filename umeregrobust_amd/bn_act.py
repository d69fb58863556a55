"""Fused batch norm as a differentiable torch op, on the HIP kernels of include/umereg_bn_act.h: what
`ResUNetSmall2(trainable=True, fused_norm=True)` runs between its convolutions.

    y = batch_norm_act(x, bn, residual=None, relu=False)      # act(bn(x) [+ residual]), bn an nn.BatchNorm1d
    e, up, down = grad_scale_device(dy)                       # the three device scalars of sparse_conv.grad_scale

`batch_norm_act` follows `bn.training`: batch statistics over all rows of x and in-place updates of the running statistics in
train mode, the running statistics in eval mode.  Gradients reach x, the residual, `bn.weight` and `bn.bias`; the op saves x, y and
the two statistic vectors (the backward recomputes the ReLU mask from y and never stores the masked gradient).  Two launches per
forward and two per backward in train mode; every sum is fp64 over a fixed tree (deterministic bit for bit).  Everything runs on
the current stream and nothing waits for the device.  No CPU fallback: CPU tensors raise."""
import torch

from . import _lib

BN_ACT_SIGNATURES = _lib.TABLES["umereg_bn_act.h"]
load_native = _lib.load

MAX_CH = 256        # UMEREG_BN_ACT_MAX_CH


_ptr, _stream = _lib.ptr, _lib.stream_ptr


def _rows(t, what):
    return _lib.rows(t, "batch_norm_act", what)


def scratch_bytes(n, C):
    return int(_lib.load().umereg_bn_act_scratch_bytes(int(n), int(C)))


def forward_raw(x, residual, gamma, beta, running_mean, running_var, num_batches_tracked, train, relu, eps, momentum):
    """One forward through the C ABI -> (y, stats [2, C]: the mean and invstd used).  Train mode updates the running statistics
    in place (pass None for all three to track nothing)."""
    lib = _lib.load()
    n, C = x.shape
    y = torch.empty(n, C, dtype=torch.float32, device=x.device)
    stats = torch.empty(2, C, dtype=torch.float32, device=x.device)
    scratch = torch.empty(max(scratch_bytes(n, C), 16), dtype=torch.uint8, device=x.device) if train else None
    _lib.call(x.device, lib.umereg_bn_act_forward_f32, x.data_ptr(), x.stride(0), _ptr(residual),
              0 if residual is None else residual.stride(0), n, C, gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
              _ptr(num_batches_tracked), int(bool(train)), int(bool(relu)), float(eps), float(momentum), y.data_ptr(), C,
              stats[0].data_ptr(), stats[1].data_ptr(), _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream(x.device))
    return y, stats


def backward_raw(dy, x, y, gamma, stats, train, relu, need_dx=True, need_dres=False, need_params=True):
    """One backward through the C ABI -> (dx, dres, dgamma, dbeta); what is not asked for is None (train mode always forms the
    parameter sums: dx depends on them)."""
    lib = _lib.load()
    n, C = x.shape
    need_params = bool(need_params or train)
    dx = torch.empty(n, C, dtype=torch.float32, device=x.device) if need_dx else None
    dres = torch.empty(n, C, dtype=torch.float32, device=x.device) if need_dres else None
    dparams = torch.empty(2, C, dtype=torch.float32, device=x.device) if need_params else None
    scratch = torch.empty(max(scratch_bytes(n, C), 16), dtype=torch.uint8, device=x.device) if need_params else None
    _lib.call(x.device, lib.umereg_bn_act_backward_f32, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0),
              _ptr(y) if relu else None, y.stride(0) if relu else 0, n, C, gamma.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
              int(bool(train)), int(bool(relu)), _ptr(dx), C, _ptr(dres), C, dparams[0].data_ptr() if need_params else None,
              dparams[1].data_ptr() if need_params else None, _ptr(scratch), 0 if scratch is None else scratch.numel(),
              _stream(x.device))
    return dx, dres, (dparams[0] if need_params else None), (dparams[1] if need_params else None)


def _bump(*tensors):
    """the kernels wrote these through raw pointers: tell torch (version counters key the model's packed-parameter cache)"""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, bn, relu):
        train = bool(bn.training)
        xs = _rows(x, "input")
        rs = None if residual is None else _rows(residual, "residual")
        track = (bn.running_mean, bn.running_var, bn.num_batches_tracked)
        y, stats = forward_raw(xs, rs, weight.detach(), bias.detach(), *track, train, relu, bn.eps, bn.momentum)
        if train:
            _bump(*track)
        ctx.train, ctx.relu, ctx.has_res = train, bool(relu), residual is not None
        ctx.save_for_backward(xs, y, stats, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, stats, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = _rows(dy, "output gradient")
        if not (need[0] or need[2] or need[3] or (ctx.has_res and need[1])):
            return None, None, None, None, None, None
        dx, dres, dgamma, dbeta = backward_raw(dy, x, y, weight.detach(), stats, ctx.train, ctx.relu, need_dx=need[0],
                                               need_dres=ctx.has_res and need[1], need_params=need[2] or need[3])
        return dx, dres, (dgamma if need[2] else None), (dbeta if need[3] else None), None, None


def batch_norm_act(x, bn, residual=None, relu=False):
    """act(bn(x) [+ residual]) on the HIP kernels of include/umereg_bn_act.h.  x, residual: f32 [rows, C] on the GPU, C a multiple of
    32 up to 256; bn: an affine `nn.BatchNorm1d(C)` that tracks running statistics with a numeric momentum; relu: act = ReLU
    (else the identity).  Follows `bn.training`; train mode needs at least two rows."""
    if not isinstance(bn, torch.nn.BatchNorm1d):
        raise TypeError(f"batch_norm_act: bn must be an nn.BatchNorm1d, got {type(bn).__name__}")
    if bn.momentum is None:
        raise ValueError("batch_norm_act: momentum=None (the cumulative average) is not supported; give BatchNorm1d a number")
    if not bn.affine or not bn.track_running_stats:
        raise ValueError("batch_norm_act: BatchNorm1d must be affine and track its running statistics")
    _lib.on_gpu("batch_norm_act", x, bn.weight, *(() if residual is None else (residual,)))
    if x.dim() != 2 or x.shape[1] != bn.num_features or x.shape[1] % 32 or not 32 <= x.shape[1] <= MAX_CH:
        raise ValueError(f"batch_norm_act: x must be [rows, {bn.num_features}] with a channel count that is a multiple of 32 up to "
                         f"{MAX_CH}, got {tuple(x.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"batch_norm_act: residual {tuple(residual.shape)} != x {tuple(x.shape)}")
    if x.shape[0] == 0:
        raise ValueError("batch_norm_act: empty input")
    if bn.training and x.shape[0] == 1:
        raise ValueError("batch_norm_act: train mode needs more than one value per channel (one row given)")
    return _BatchNormAct.apply(x, residual, bn.weight, bn.bias, bn, bool(relu))


_unit = {}      # device -> (ones [256], zeros [256]): the identity affine map of `relu`


class _Relu(torch.autograd.Function):
    """max(x, 0) on the same kernels: the eval-mode form with scale 1 and shift 0 (x * 1 + 0 is exact), one launch each way."""

    @staticmethod
    def forward(ctx, x):
        xs = _rows(x, "input")
        if xs.device not in _unit:
            _unit[xs.device] = (torch.ones(MAX_CH, device=xs.device), torch.zeros(MAX_CH, device=xs.device))
        ones, zeros = _unit[xs.device]
        y, stats = forward_raw(xs, None, ones, zeros, zeros, ones, None, False, True, 0.0, 0.0)
        ctx.save_for_backward(xs, y, stats, ones)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, stats, ones = ctx.saved_tensors
        return backward_raw(_rows(dy, "output gradient"), x, y, ones, stats, False, True, need_params=False)[0]


def relu(x):
    """max(x, 0) for f32 [rows, C] on the GPU (C a multiple of 32 up to 256), forward and backward on the kernels of this module."""
    _lib.on_gpu("relu", x)
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] % 32 or not 32 <= x.shape[1] <= MAX_CH:
        raise ValueError(f"relu: x must be a non-empty [rows, C] with C a multiple of 32 up to {MAX_CH}, got {tuple(x.shape)}")
    return _Relu.apply(x)


def grad_scale_device(dy):
    """`sparse_conv.grad_scale` as two kernels (include/umereg_bn_act.h): -> (e, 2^e, 2^-e) as 0-dim tensors on dy's device
    (int32, f32, f32), the same contract bit for bit; one reduction of max |dy|, no host sync."""
    _lib.on_gpu("grad_scale_device", dy)
    if dy.dtype != torch.float32:
        raise ValueError(f"grad_scale_device: dy must be f32, got {dy.dtype}")
    lib = _lib.load()
    dy = dy.detach()
    dy = dy.contiguous()
    if dy.data_ptr() % 16:
        dy = dy.clone()
    count = dy.numel()
    need = int(lib.umereg_grad_scale_scratch_bytes(count))
    if need == 0:
        raise ValueError(f"grad_scale_device: {count} elements not supported")
    buf = torch.empty(4 + need // 4, dtype=torch.int32, device=dy.device)      # the three scalars, one pad word, the partials
    base = buf.data_ptr()
    _lib.call(dy.device, lib.umereg_grad_scale_f32, dy.data_ptr() if count else None, count, base, base + 4, base + 8, base + 16, need,
              _stream(dy.device))
    return buf[0], buf[1:2].view(torch.float32)[0], buf[2:3].view(torch.float32)[0]
