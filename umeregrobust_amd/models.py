"""`ResUNetSmall2(in_channels=1, out_channels=32)` -- the reference's feature network (models.py:392-618 with the
configuration of :691-698) on the HIP sparse convolution of csrc/sparse_map.hip + csrc/featnet.hip (C ABI:
include/umereg_featnet.h): one fused forward call in eval mode, and with `trainable=True` a layer-wise differentiable
path over csrc/sparse_wgrad.hip (include/umereg_sparse_conv.h, umeregrobust_amd/sparse_conv.py).

Drop-in for the reference's evaluation loop (evaluate.py:163-165, :178-179, :190-192):

    model = ResUNetSmall2(in_channels=1, out_channels=32).to(device)
    model.load_state_dict(checkpoint_state_dict(path))        # the reference's names and shapes
    model.eval()
    with torch.no_grad():
        feat = torch.stack(model(SparseTensor(ones, coordinates=coords, device=device)).decomposed_features, 0)

The network: channels [_, 32, 64, 64, 128, 256], transposed-conv channels [_, 64, 64, 64, 128, 128], kernel size 3,
strides [1, 2, 2, 2, 3] (tensor strides 1, 2, 4, 8, 24), blocks conv3 -> BN -> + residual -> ReLU; encoder levels conv -> BN
-> block -> ReLU, decoder levels transposed conv -> BN -> block -> ReLU -> cat(tr, skip); mlp1 (1x1, 96 -> 64) -> ReLU;
final (1x1, 64 -> 32, bias); row-wise L2 normalisation without epsilon.  Eval batch norm (eps 1e-5) is folded into a
per-channel scale and shift in fp64 before the parameters go to the device as f32.

MinkowskiEngine 0.5.4 semantics restated (parity unpinned; the kernels keep each in one place, csrc/sparse.h):
  1. strided output map: unique(floor(c / (ts s)) ts s) per axis, batch index kept;
  2. kernel offsets {-1, 0, 1} ts_in per axis, offset index k = (dx+1) + 3(dy+1) + 9(dz+1) (x fastest);
  3. kernel shapes [27, C_in, C_out], 1x1 kernels [C_in, C_out], bias [1, C_out];
  4. convolution: out[o] = sum_k in[o + off_k(ts_in)] @ W[k] over the offsets that exist;
  5. transposed convolution onto the encoder map at ts_in / s: out[f] = sum_k in[f - off_k(ts_out)] @ W[k] over the
     f - off_k that exist in the coarse map;
  6. output rows in input order (`decomposed_features` splits them by batch index).
Input coordinates must be unique per batch item (a duplicate raises); x, y, z in [-2^17, 2^17), at most 127 clouds.

No CPU fallback: CPU tensors raise.  By default (`trainable=False`) there is no autograd either: train mode and a forward
that would need gradients raise.

`ResUNetSmall2(..., trainable=True)` (reference train_coloring.py:33-73): in train mode, and in eval mode whenever gradients
are needed, the forward runs layer by layer -- every 27-offset convolution is `sparse_conv.sparse_conv` (HIP forward, HIP
input and weight gradients), batch norm is the model's own `nn.BatchNorm1d` modules (batch statistics over all rows of the
call and running-stat updates in train mode, running statistics in eval mode), residual / ReLU / concatenation / the two
1x1 layers / the L2 normalisation are torch ops.  Eval mode under `torch.no_grad()` stays the fused call, bit for bit.

`ResUNetSmall2(..., precision="f16")` (include/umereg_featnet_f16.h; the default is "f32"): the fused call with the operands of
the seventeen 27-offset convolutions after conv1 and of mlp1 rounded to f16 (round to nearest even) and every sum, the
epilogues and all stored activations in f32 -- deterministic like the f32 path.  Inference only: train mode and a forward
that needs gradients raise, there is no silent fallback to f32.  An activation beyond the f16 range raises ValueError.

`ResUNetSmall2(..., trainable=True, train_precision="f16")` (include/umereg_sparse_conv_f16.h; the default is "f32"): the
operand precision of the layer-wise path, whatever `precision` is -- the seventeen 27-offset convolutions after conv1 and mlp1
run `sparse_conv(..., precision="f16")` / `linear(..., precision="f16")`: f16 operands in the forward and in both gradients,
f32 sums, parameters, gradients and saved activations; conv1, `final`, batch norm and the rest stay f32.  Deterministic.  No
range check per layer (it would synchronise): an activation beyond +-65504 reaches the next layer as infinity and the loss as
a non-finite value, which the training driver names where it reads the loss.

`ResUNetSmall2(..., trainable=True, fused_norm=True)` (include/umereg_bn_act.h, umeregrobust_amd/bn_act.py; opt-in, the default
path and its bits are unchanged): every `bn(conv)` and every `relu(bn(conv) + h)` of the layer-wise path is one
`bn_act.batch_norm_act` (HIP statistics, apply and backward kernels; fp64 sums over a fixed tree), mlp1's ReLU is `bn_act.relu`,
and with train_precision="f16" the backward scale comes from `bn_act.grad_scale_device`.  Parameters, buffers, state-dict keys and
`packed_parameters` are the same modules' as ever: a checkpoint of either path loads into the other.

`ResUNetSmall2(..., conv_mode="pairs")` (include/umereg_sparse_conv_pairs.h, csrc/sparse_conv_pairs.hip; opt-in, the default is
"union"): the seventeen 27-offset layers after conv1 run on the pair-compacted engine, which feeds the matrix unit, per offset,
only the rows of a tile that have that neighbour -- in the fused call and in the layer-wise path (forward and input gradient; the
weight gradient has no mode).  The values are the union engine's bit for bit; the mode combines freely with `precision`,
`trainable`, `train_precision` and `fused_norm`, and leaves state dict and checkpoints alone."""
import ctypes

import torch
from torch import nn

from . import _lib
from .sparse import SparseTensor

FEATNET_SIGNATURES = _lib.TABLES["umereg_featnet.h"]
FEATNET_F16_SIGNATURES = _lib.TABLES["umereg_featnet_f16.h"]
load_native = _lib.load

# include/umereg_featnet.h
N_LAYERS, OUT_CHANNELS, N_STATUS, MAX_BATCH = 20, 32, 8, 127
BUF_COORDS0, BUF_CAT0, BUF_S4, BUF_HIDDEN, BUF_PERM, BUF_MASKS = 0, 5, 9, 10, 11, 12
ERR_RANGE, ERR_DUPLICATE = 1, 2
ERR_F16_RANGE = 4           # include/umereg_featnet_f16.h
PRECISIONS = ("f32", "f16")
CONV_MODES = ("union", "pairs")     # the engine of the 27-offset layers; "pairs": include/umereg_sparse_conv_pairs.h

# the packed parameter block's layer order (umereg_featnet_layer_info) -> (kernel, batch norm or None)
LAYERS = (
    ("conv1", "norm1"), ("block1.conv1", "block1.norm1"),
    ("conv2", "norm2"), ("block2.conv1", "block2.norm1"),
    ("conv3", "norm3"), ("block3.conv1", "block3.norm1"),
    ("conv4", "norm4"), ("block4.conv1", "block4.norm1"),
    ("conv5", "norm5"), ("block5.conv1", "block5.norm1"),
    ("conv4_tr", "norm4_tr"), ("block4_tr.conv1", "block4_tr.norm1"),
    ("conv3_tr", "norm3_tr"), ("block3_tr.conv1", "block3_tr.norm1"),
    ("conv2_tr", "norm2_tr"), ("block2_tr.conv1", "block2_tr.norm1"),
    ("conv1_tr", "norm1_tr"), ("block1_tr.conv1", "block1_tr.norm1"),
    ("mlp1", None), ("final", None))


def check_precision(precision):
    """-> `precision`, one of PRECISIONS ("f32"; "f16": f16 operands, f32 accumulation, inference only); else ValueError"""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


def check_conv_mode(conv_mode):
    """-> `conv_mode`, one of CONV_MODES ("union"; "pairs": the pair-compacted engine, the same values); else ValueError"""
    if conv_mode not in CONV_MODES:
        raise ValueError(f"conv_mode must be one of {CONV_MODES}, got {conv_mode!r}")
    return conv_mode


def layer_info():
    """[(K, C_in, C_out, offset of W, offset of scale)] of the packed parameter block, from the library."""
    lib = _lib.load()
    info = (ctypes.c_int32 * 5)()
    out = []
    for i in range(N_LAYERS):
        _lib.checked(lib.umereg_featnet_layer_info, i, ctypes.addressof(info))
        out.append(tuple(info))
    return out


def workspace_bytes(n, batch):
    return int(_lib.load().umereg_featnet_workspace_bytes(int(n), int(batch)))


def buffer_view(ws, n, batch, which, rows, dtype=torch.float32):
    """A [rows, cols] view of workspace buffer `which` (include/umereg_featnet.h, UMEREG_FN_*)."""
    off, cols = ctypes.c_size_t(), ctypes.c_int32()
    _lib.checked(_lib.load().umereg_featnet_buffer, int(n), int(batch), int(which), ctypes.addressof(off), ctypes.addressof(cols))
    esz = torch.empty(0, dtype=dtype).element_size()
    return ws[off.value:off.value + rows * cols.value * esz].view(dtype).view(rows, cols.value)


def forward_raw(coords, feat, batch, params, ws, out, status, precision="f32", conv_mode="union"):
    """One forward pass through the C ABI on the current stream; no host sync, no error check of `status`.  precision="f16":
    umereg_featnet_forward_f16 (include/umereg_featnet_f16.h), same buffers.  conv_mode="pairs": umereg_featnet_forward_pairs
    (include/umereg_sparse_conv_pairs.h) in the chosen precision, same buffers, same values."""
    check_precision(precision)
    check_conv_mode(conv_mode)
    lib = _lib.load()
    f16 = precision == "f16"
    if conv_mode == "pairs":
        fn, mode = lib.umereg_featnet_forward_pairs, (int(f16),)
    else:
        fn, mode = (lib.umereg_featnet_forward_f16 if f16 else lib.umereg_featnet_forward_f32), ()
    _lib.call(coords.device, fn, coords.data_ptr(), feat.data_ptr(), int(coords.shape[0]), int(batch), params.data_ptr(), out.data_ptr(),
              status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(coords.device), *mode)


def build_maps_raw(coords, batch, ws, status):
    """The coordinate maps alone (the first half of forward_raw), on the current stream; no host sync."""
    _lib.call(coords.device, _lib.load().umereg_featnet_build_maps, coords.data_ptr(), int(coords.shape[0]), int(batch),
              status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(coords.device))


def check_status(status, precision="f32"):
    """Raise on the error bits of a forward pass's status (one device read); -> level sizes [5]."""
    s = status.cpu().tolist()
    if s[0] & ERR_F16_RANGE and not s[0] & (ERR_DUPLICATE | ERR_RANGE):
        raise ValueError(f"ResUNetSmall2(precision={precision!r}): an activation left the f16 range (|x| > 65504) and would "
                         "reach the next layer as infinity; run this input with precision='f32'")
    if s[0] & ERR_DUPLICATE:
        raise ValueError("ResUNetSmall2: duplicate coordinates in a batch item (MinkowskiEngine would merge them; "
                         "the reference's inputs come from sparse_quantize and are unique)")
    if s[0] & ERR_RANGE:
        raise ValueError("ResUNetSmall2: a batch index outside [0, batch) or a coordinate outside [-2^17, 2^17)")
    return s[1:6]


class _Conv(nn.Module):
    """MinkowskiConvolution(Transpose)'s parameters: `kernel` [27, C_in, C_out] (1x1: [C_in, C_out]), `bias` [1, C_out]."""

    def __init__(self, cin, cout, kernel_size, bias=False):
        super().__init__()
        shape = (27, cin, cout) if kernel_size == 3 else (cin, cout)
        self.kernel = nn.Parameter(torch.empty(shape))
        self.bias = nn.Parameter(torch.zeros(1, cout)) if bias else None
        with torch.no_grad():
            bound = 1.0 / (cin * (27 if kernel_size == 3 else 1)) ** 0.5
            self.kernel.uniform_(-bound, bound)


class _Norm(nn.Module):
    """MinkowskiBatchNorm: the parameters live in `.bn` (torch.nn.BatchNorm1d, eps 1e-5)."""

    def __init__(self, c, bn_momentum=0.1):
        super().__init__()
        self.bn = nn.BatchNorm1d(c, momentum=bn_momentum)


class _Block(nn.Module):
    """BasicBlockBase2 (reference models.py:70-96): conv3 -> BN -> + residual -> ReLU."""

    def __init__(self, c, bn_momentum=0.1):
        super().__init__()
        self.conv1 = _Conv(c, c, 3)
        self.norm1 = _Norm(c, bn_momentum)


class ResUNetSmall2(nn.Module):
    CHANNELS = [None, 32, 64, 64, 128, 256]
    TR_CHANNELS = [None, 64, 64, 64, 128, 128]
    STRIDES = [1, 2, 2, 2, 3]

    def __init__(self, in_channels=1, out_channels=32, bn_momentum=0.1, normalize_feature=True, D=3, trainable=False,
                 precision="f32", train_precision="f32", fused_norm=False, conv_mode="union"):
        super().__init__()
        self.conv_mode = check_conv_mode(conv_mode)
        self.trainable = bool(trainable)
        self.fused_norm = bool(fused_norm)
        if self.fused_norm and not self.trainable:
            raise ValueError("ResUNetSmall2(fused_norm=True) selects the kernels of the layer-wise path's batch norm: it needs "
                             "trainable=True")
        self.precision = check_precision(precision)
        if train_precision not in PRECISIONS:
            raise ValueError(f"train_precision must be one of {PRECISIONS}, got {train_precision!r}")
        if train_precision != "f32" and not self.trainable:
            raise ValueError(f"ResUNetSmall2(train_precision={train_precision!r}) is the operand precision of the layer-wise path: "
                             "it needs trainable=True")
        self.train_precision = train_precision
        if (in_channels, out_channels, bool(normalize_feature), D) != (1, OUT_CHANNELS, True, 3):
            raise ValueError("the HIP network is built for in_channels=1, out_channels=32, normalize_feature=True, D=3 "
                             "(the configuration of reference evaluate.py:163)")
        ch, tr = self.CHANNELS, self.TR_CHANNELS
        for i in range(1, 6):
            setattr(self, f"conv{i}", _Conv(in_channels if i == 1 else ch[i - 1], ch[i], 3))
            setattr(self, f"norm{i}", _Norm(ch[i], bn_momentum))
            setattr(self, f"block{i}", _Block(ch[i], bn_momentum))
        for i in range(4, 0, -1):
            cin = ch[5] if i == 4 else ch[i + 1] + tr[i + 2]
            setattr(self, f"conv{i}_tr", _Conv(cin, tr[i + 1], 3))
            setattr(self, f"norm{i}_tr", _Norm(tr[i + 1], bn_momentum))
            setattr(self, f"block{i}_tr", _Block(tr[i + 1], bn_momentum))
        self.mlp1 = _Conv(tr[2] + ch[1], tr[1], 1)
        self.final = _Conv(tr[1], out_channels, 1, bias=True)
        self._packed_key = None
        self._packed = None
        self._ws = {}

    # ---- parameters ------------------------------------------------------------------------------------------------------
    def packed_parameters(self):
        """The packed f32 parameter block of include/umereg_featnet.h on the parameters' device: kernels as they are, eval
        batch norm folded in fp64 into scale = gamma / sqrt(var + eps), shift = beta - mean scale; cached until a parameter or
        buffer changes."""
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if key == self._packed_key:
            return self._packed
        info = layer_info()
        dev = self.conv1.kernel.device
        total = int(_lib.load().umereg_featnet_params_count())
        block = torch.zeros(total, dtype=torch.float64, device=dev)
        mods = dict(self.named_modules())
        with torch.no_grad():
            for (name, norm), (K, cin, cout, off_w, off_s) in zip(LAYERS, info):
                conv = mods[name]
                w = conv.kernel.detach().double()
                if tuple(w.shape) != ((K, cin, cout) if K > 1 else (cin, cout)):
                    raise ValueError(f"{name}.kernel: shape {tuple(w.shape)} != the library's {(K, cin, cout)}")
                block[off_w:off_w + K * cin * cout] = w.reshape(-1)
                if norm is not None:
                    bn = mods[norm].bn
                    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
                    shift = bn.bias.double() - bn.running_mean.double() * scale
                else:
                    scale = torch.ones(cout, dtype=torch.float64, device=dev)
                    shift = conv.bias.detach().double().reshape(-1) if conv.bias is not None else torch.zeros_like(scale)
                block[off_s:off_s + cout] = scale
                block[off_s + cout:off_s + 2 * cout] = shift
        self._packed = block.float().contiguous()
        self._packed_key = key
        return self._packed

    def _workspace(self, n, batch, dev):
        need = workspace_bytes(n, batch)
        ws = self._ws.get(dev)
        if ws is None or ws.numel() < need:
            self._ws[dev] = ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    # ---- forward ---------------------------------------------------------------------------------------------------------
    def forward(self, x, debug=False):
        """x: SparseTensor with features [N, 1] and coordinates [N, 4] on the GPU -> SparseTensor of [N, 32] unit rows on the
        same coordinates, rows in input order.  debug=True: (output, intermediates) with the per-level coordinates, both
        halves of every level's concatenation, block5's output and mlp1's output (see include/umereg_featnet.h)."""
        F, C = x.F, x.C
        needs_grad = torch.is_grad_enabled() and (F.requires_grad or any(p.requires_grad for p in self.parameters()))
        if self.precision != "f32" and self.train_precision == "f32" and (self.training or needs_grad):
            raise RuntimeError(f"ResUNetSmall2(precision={self.precision!r}) is inference only: the layer-wise path (train mode, "
                               "or a forward that needs gradients) is f32, and there is no silent fallback to it; call .eval() "
                               "under torch.no_grad(), or build the model with precision='f32' (to train with f16 operands: "
                               "trainable=True, train_precision='f16')")
        if not self.trainable:
            if self.training:
                raise RuntimeError("ResUNetSmall2 runs forward only with eval-mode batch norm: call .eval() first "
                                   "(or build it with trainable=True)")
            if needs_grad:
                raise RuntimeError("ResUNetSmall2 has no backward pass: run it under torch.no_grad() (or build it with trainable=True)")
        _lib.on_gpu("ResUNetSmall2", F, C)
        if self.training or needs_grad:
            return self._forward_layers(x, debug)
        params = self.packed_parameters()
        if params.device != F.device:
            raise RuntimeError(f"ResUNetSmall2: parameters on {params.device}, input on {F.device}")
        if F.shape[1] != 1:
            raise ValueError(f"ResUNetSmall2: in_channels is 1, got features [N, {F.shape[1]}]")
        n, batch = C.shape[0], x.batch_size
        if n == 0:
            raise ValueError("ResUNetSmall2: empty input")
        if batch > MAX_BATCH:
            raise ValueError(f"ResUNetSmall2: at most {MAX_BATCH} clouds per call, got batch index {batch - 1}")
        coords = C.to(torch.int32).contiguous()
        feat = F.to(torch.float32).contiguous()
        ws = self._workspace(n, batch, F.device)
        out = torch.empty(n, OUT_CHANNELS, dtype=torch.float32, device=F.device)
        status = torch.empty(N_STATUS, dtype=torch.int32, device=F.device)
        forward_raw(coords, feat, batch, params, ws, out, status, self.precision, self.conv_mode)
        sizes = check_status(status, self.precision)
        res = SparseTensor(out, coordinates=coords)
        res._batch_size = batch
        if not debug:
            return res
        inter = dict(levels=sizes, perm=buffer_view(ws, n, batch, BUF_PERM, n, torch.int32)[:, 0].clone(),
                     hidden=buffer_view(ws, n, batch, BUF_HIDDEN, n).clone(),
                     s4=buffer_view(ws, n, batch, BUF_S4, sizes[4]).clone())
        inter["coords"] = [buffer_view(ws, n, batch, BUF_COORDS0 + l, sizes[l], torch.int32).clone() for l in range(5)]
        inter["cat"] = [buffer_view(ws, n, batch, BUF_CAT0 + l, sizes[l]).clone() for l in range(4)]
        return res, inter

    def _forward_layers(self, x, debug):
        """The trainable path: the same network layer by layer (see the module docstring).  Rows travel in the level-0 order of
        the coordinate maps between the first and the last layer."""
        from . import sparse_conv as sc
        F, C = x.F, x.C
        if F.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("ResUNetSmall2: the input features require grad, and conv1 has no input gradient "
                               "(the reference's input features are ones); detach them")
        dev = self.conv1.kernel.device
        if dev != F.device:
            raise RuntimeError(f"ResUNetSmall2: parameters on {dev}, input on {F.device}")
        if F.shape[1] != 1:
            raise ValueError(f"ResUNetSmall2: in_channels is 1, got features [N, {F.shape[1]}]")
        n, batch = C.shape[0], x.batch_size
        if n == 0:
            raise ValueError("ResUNetSmall2: empty input")
        if batch > MAX_BATCH:
            raise ValueError(f"ResUNetSmall2: at most {MAX_BATCH} clouds per call, got batch index {batch - 1}")
        maps = sc.CoordinateMaps(C, batch)
        sizes = maps.sizes
        if self.training:
            for l, rows in enumerate(sizes):
                if rows == 1:
                    raise ValueError(f"ResUNetSmall2: level {l} of this input has a single row, and train-mode batch norm needs "
                                     "more than one value per channel (use a larger cloud or .eval())")
        relu = torch.relu
        tp = self.train_precision                     # (conv1, C_in = 1, stays f32 inside sparse_conv)

        fused = self.fused_norm                       # batch norm, residual, ReLU and the f16 scale on include/umereg_bn_act.h
        if fused:
            from . import bn_act
            relu = bn_act.relu

        def conv(h, kernel, table):
            return sc.sparse_conv(h, kernel, maps, table, precision=tp, fused_scale=fused, conv_mode=self.conv_mode)

        def bn(norm, v):
            return bn_act.batch_norm_act(v, norm.bn) if fused else norm.bn(v)

        def block(h, l, blk):
            v = conv(h, blk.conv1.kernel, l)
            if fused:
                return bn_act.batch_norm_act(v, blk.norm1.bn, residual=h, relu=True)
            return relu(blk.norm1.bn(v) + h)

        skips = []
        h = F.detach().to(torch.float32)
        for l in range(5):
            cv, norm, blk = getattr(self, f"conv{l + 1}"), getattr(self, f"norm{l + 1}"), getattr(self, f"block{l + 1}")
            h = block(bn(norm, conv(h, cv.kernel, 0 if l == 0 else 5 + l - 1)), l, blk)
            skips.append(h)
        s4 = h
        cats = [None] * 4
        for l in range(3, -1, -1):
            cv, norm, blk = getattr(self, f"conv{l + 1}_tr"), getattr(self, f"norm{l + 1}_tr"), getattr(self, f"block{l + 1}_tr")
            tr = block(bn(norm, conv(h, cv.kernel, 9 + l)), l, blk)
            h = cats[l] = torch.cat([tr, skips[l]], dim=1)
        hidden = relu(sc.linear(h, self.mlp1.kernel, precision=tp, maps=maps, fused_scale=fused))
        o = sc.linear(hidden, self.final.kernel) + self.final.bias
        o = o / o.norm(dim=1, keepdim=True)
        inv = torch.empty_like(maps.perm)
        inv[maps.perm] = torch.arange(n, device=dev)
        res = SparseTensor(o.index_select(0, inv), coordinates=maps.coords)
        res._batch_size = batch
        if not debug:
            return res
        inter = dict(levels=sizes, perm=maps.perm32.clone(), hidden=hidden.detach(), s4=s4.detach(),
                     coords=[maps.level_coords(l).clone() for l in range(5)], cat=[c.detach() for c in cats])
        return res, inter
