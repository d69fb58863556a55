"""Differentiable torch restatement of ResUNetSmall2 on the index tables of tests/featnet_ref.py, for the gradient tests.

Every one of the 13 neighbour tables (featnet_ref.TABLES) becomes, per kernel offset, a pair list (output rows, input rows);
a convolution is `index_add` of `x[input rows] @ W[k]` over the offsets.  dtype is a parameter: autograd through the fp64 run
is the gradient truth, the fp32 run on the CPU is the reference-precision run that the gates are set against.  Batch norm is
`torch.nn.functional.batch_norm` in train or eval mode.  ReLU decisions can be forced (`relu(v) := v * mask`): an fp32 and an
fp64 run disagree on a handful of pre-activations within rounding of zero, and one such flip moves a kernel gradient by
1e-2 of its maximum -- with the masks of the run under test forced onto the truth, the comparison is sharp.

Rows: level 0 in input order, level l >= 1 in sorted-key order (featnet_ref.levels).  The ten ReLU sites, in the order of
RELU_SITES: the encoder blocks of levels 0..4, the decoder blocks of levels 3..0, mlp1."""
import numpy as np
import torch
import torch.nn.functional as tnf

import featnet_ref as ref

CAT_TR = (64, 64, 128, 128)          # the decoder block's share of cat[l] (first columns)
RELU_SITES = [f"enc{l}" for l in range(5)] + [f"dec{l}" for l in range(3, -1, -1)] + ["mlp1"]
NORMS = ([f"norm{i}" for i in range(1, 6)] + [f"block{i}.norm1" for i in range(1, 6)]
         + [f"norm{i}_tr" for i in range(1, 5)] + [f"block{i}_tr.norm1" for i in range(1, 5)])


def out_level(t):
    return ref.TABLES[t][0]


def in_level(t):
    return ref.TABLES[t][1]


def adjoint(t):
    """(table, mirror): <conv_t(x; W), y> = <x, conv_t'(y; W')>, W'[k'] = W[k]^T with k' = 26 - k if mirror else k"""
    if t < 5:
        return t, True
    return (t + 4, False) if t < 9 else (t - 4, False)


def repack(W, mirror):
    Wt = W.transpose(1, 2)
    return Wt.flip(0) if mirror else Wt


class Tables:
    """levels + per table and offset the (output rows, input rows) pairs of a coordinate set (int [n, 4])"""

    def __init__(self, coords, tables=range(13)):
        self.levels = ref.levels(coords)
        self.sizes = [len(c) for c in self.levels]
        idx = [ref.Index(c) for c in self.levels]
        self.pairs = {}
        for t in tables:
            ql, tl, sign = ref.TABLES[t]
            ts = ref.TSTRIDES[min(ql, tl)]
            per_k = []
            for k in range(27):
                q = self.levels[ql].copy()
                q[:, 1:] += sign * ref.OFFSETS[k] * ts
                j = idx[tl].find(q)
                o = np.nonzero(j >= 0)[0]
                per_k.append((torch.from_numpy(o), torch.from_numpy(j[o])))
            self.pairs[t] = per_k


def conv(x, W, tables, t, order=range(27)):
    """out[o] = sum_k x[nbr_t(o, k)] @ W[k]; `order`: the order the offsets are accumulated in"""
    out = torch.zeros(tables.sizes[out_level(t)], W.shape[2], dtype=x.dtype)
    for k in order:
        o, i = tables.pairs[t][k]
        if len(o):
            out = out.index_add(0, o, x[i] @ W[k])
    return out


def chain_lengths(tables, t, cin):
    """products in the chain of every output element of conv over table t: existing offsets x C_in, per output row"""
    cnt = torch.zeros(tables.sizes[out_level(t)], dtype=torch.int64)
    for k in range(27):
        cnt[tables.pairs[t][k][0]] += 1
    return cnt * cin


def state(sd, dtype, requires_grad=True):
    """{name: numpy} -> {name: torch leaf tensors of `dtype`} (running statistics without grad, counters as they are)"""
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.as_tensor(np.asarray(v)).clone()
            continue
        t = torch.as_tensor(np.asarray(v)).to(dtype).clone()
        out[k] = t.requires_grad_(requires_grad and "running_" not in k)
    return out


def network(tables, feat, sd, train=False, masks=None, momentum=0.1, eps=1e-5, order=range(27)):
    """feat [n, 1] torch, sd {name: torch} (see `state`) -> (out [n, 32] in input order, inter).  inter: `cat` (l < 4), `s4`,
    `hidden` as featnet_ref.network; `pre` {site: the ReLU's input}, `mask` {site: the decisions used}.  train=True: batch
    statistics, and the running statistics / counters of `sd` are updated in place as nn.BatchNorm1d does.
    masks: {site: bool tensor} forced decisions, or None for relu's own."""
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
        return relu(bn(conv(h, sd[name + ".conv1.kernel"], tables, l, order), name + ".norm1") + h, site)

    skips = []
    x = feat
    for l in range(5):
        i = l + 1
        h = bn(conv(x, sd[f"conv{i}.kernel"], tables, 0 if l == 0 else 5 + l - 1, order), f"norm{i}")
        x = block(h, l, f"block{i}", f"enc{l}")
        skips.append(x)
    inter = dict(s4=x, cat=[None] * 4)
    for l in range(3, -1, -1):
        i = l + 1
        h = bn(conv(x, sd[f"conv{i}_tr.kernel"], tables, 9 + l, order), f"norm{i}_tr")
        x = inter["cat"][l] = torch.cat([block(h, l, f"block{i}_tr", f"dec{l}"), skips[l]], dim=1)
    hidden = inter["hidden"] = relu(x @ sd["mlp1.kernel"], "mlp1")
    o = hidden @ sd["final.kernel"] + sd["final.bias"].reshape(1, -1)
    inter["pre"], inter["mask"] = pre, used
    return o / o.norm(dim=1, keepdim=True), inter


def site_values(inter):
    """{site: the post-ReLU tensor of that site} from a network's intermediates (`cat`, `s4`, `hidden`), ours or the GPU's
    (torch tensors or numpy arrays): value > 0 is the site's mask"""
    out = {"enc4": inter["s4"], "mlp1": inter["hidden"]}
    for l in range(4):
        out[f"dec{l}"] = inter["cat"][l][:, :CAT_TR[l]]
        out[f"enc{l}"] = inter["cat"][l][:, CAT_TR[l]:]
    return out


def site_level(site):
    return 0 if site == "mlp1" else int(site[3])
