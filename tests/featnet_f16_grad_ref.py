"""The f16-operand TRAINING contract of include/umereg_sparse_conv_f16.h restated in torch for the tests: the convolution of
tests/featnet_grad_ref.py as a `torch.autograd.Function`, in fp64 (the contract's truth) or fp32 (the f32-sized perturbation a
correct kernel is allowed).

    forward:   out = conv(q(x), q(W))                                         q = the operand hook, sums in `dtype`
    backward:  e = 14 - floor(log2(max |dY|)) (0 if that maximum is zero or not finite),  dYs = q(dY 2^e)
               dx = 2^-e adjoint conv(dYs, q(W)),   dW[k] = 2^-e sum_o q(x)[nbr(o, k)]^T dYs[o]
    mlp1:      out = q(x) @ q(W);  dx = 2^-e dYs @ q(W)^T;  dW = x^T dY in `dtype`, unrounded (the f32 block sum)

The hook is one of tests/featnet_f16_ref.py's (`r16_op`: round to nearest even -- the contract; `t16_op`: truncation -- the
wrong rounding the gates must tell apart; `identity`): `q(array, what)` with `what` in "in", "w", "dy".  `network` is
featnet_grad_ref.network with these two operators in layers 1..18 of the packed parameter block; conv1, `final`, batch norm,
residuals, ReLU and the L2 normalisation are featnet_grad_ref's."""
import math

import numpy as np
import torch
import torch.nn.functional as tnf

import featnet_f16_ref as f16ref
import featnet_grad_ref as gref


def scale_exponent(dy):
    """e of the contract from a tensor of output gradients (host arithmetic on the exact maximum)"""
    m = float(dy.detach().abs().max()) if dy.numel() else 0.0
    if m == 0.0 or not math.isfinite(m):
        return 0
    return 14 - (math.frexp(m)[1] - 1)          # m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1


def _q(q, t, what):
    return torch.from_numpy(np.asarray(q(t.detach().numpy(), what))).to(t.dtype)


def _scaled(q, dy):
    e = scale_exponent(dy)
    return _q(q, dy * 2.0 ** e, "dy"), 2.0 ** -e


class _Conv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, tables, t, q, order):
        xq, Wq = _q(q, x, "in"), _q(q, W, "w")
        ctx.tables, ctx.t, ctx.q, ctx.order = tables, t, q, order
        ctx.save_for_backward(xq, Wq)
        return gref.conv(xq, Wq, tables, t, order)

    @staticmethod
    def backward(ctx, dy):
        xq, Wq = ctx.saved_tensors
        tables, t = ctx.tables, ctx.t
        dys, down = _scaled(ctx.q, dy)
        ta, mirror = gref.adjoint(t)
        dx = gref.conv(dys, gref.repack(Wq, mirror), tables, ta, ctx.order) * down
        dw = torch.zeros_like(Wq)
        for k in range(27):
            o, i = tables.pairs[t][k]
            if len(o):
                dw[k] = xq[i].t() @ dys[o]
        return dx, dw * down, None, None, None, None


class _Linear16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, q):
        Wq = _q(q, W, "w")
        ctx.q = q
        ctx.save_for_backward(x, Wq)
        return _q(q, x, "in") @ Wq

    @staticmethod
    def backward(ctx, dy):
        x, Wq = ctx.saved_tensors
        dys, down = _scaled(ctx.q, dy)
        return (dys @ Wq.t()) * down, x.t() @ dy, None


def conv(x, W, tables, t, q=f16ref.r16_op, order=range(27)):
    """the 27-offset convolution of the contract, differentiable (x [rows, C_in >= 32], W [27, C_in, C_out])"""
    return _Conv16.apply(x, W, tables, t, q, order)


def linear(x, W, q=f16ref.r16_op):
    """mlp1 of the contract, differentiable"""
    return _Linear16.apply(x, W, q)


def network(tables, feat, sd, train=False, masks=None, q=f16ref.r16_op, momentum=0.1, eps=1e-5, order=range(27)):
    """featnet_grad_ref.network (same arguments, same returns) with the f16-operand operators in layers 1..18"""
    dtype = feat.dtype
    pre, used = {}, {}

    def relu(v, site):
        pre[site] = v
        m = (v > 0) if masks is None else masks[site]
        used[site] = m
        return v * m.to(dtype)

    def bn(x, name):
        p = name + ".bn."
        if train:
            sd[p + "num_batches_tracked"] += 1
        return tnf.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], training=train,
                              momentum=momentum, eps=eps)

    def block(h, l, name, site):
        return relu(bn(conv(h, sd[name + ".conv1.kernel"], tables, l, q, order), name + ".norm1") + h, site)

    skips = []
    x = feat
    for l in range(5):
        i = l + 1
        if l == 0:      # conv1: f32 in the contract
            h = gref.conv(x, sd["conv1.kernel"], tables, 0, order)
        else:
            h = conv(x, sd[f"conv{i}.kernel"], tables, 5 + l - 1, q, order)
        x = block(bn(h, f"norm{i}"), l, f"block{i}", f"enc{l}")
        skips.append(x)
    inter = dict(s4=x, cat=[None] * 4)
    for l in range(3, -1, -1):
        i = l + 1
        h = bn(conv(x, sd[f"conv{i}_tr.kernel"], tables, 9 + l, q, order), f"norm{i}_tr")
        x = inter["cat"][l] = torch.cat([block(h, l, f"block{i}_tr", f"dec{l}"), skips[l]], dim=1)
    hidden = inter["hidden"] = relu(linear(x, sd["mlp1.kernel"], q), "mlp1")
    o = hidden @ sd["final.kernel"] + sd["final.bias"].reshape(1, -1)
    inter["pre"], inter["mask"] = pre, used
    return o / o.norm(dim=1, keepdim=True), inter


def rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0
