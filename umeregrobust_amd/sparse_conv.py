"""Sparse 3-D convolution as a differentiable torch op, on the HIP operators of include/umereg_sparse_conv.h: what
`ResUNetSmall2(trainable=True)` is made of.

    maps = CoordinateMaps(coords, batch)              # once per coordinate set: every level, all 13 neighbour tables
    y = sparse_conv(x, kernel, maps, table)           # out[o] = sum_k x[nbr_table(o, k)] @ kernel[k]

Tables (include/umereg_featnet.h): self map of level l = l, strided l -> l+1 = 5 + l, transposed l+1 -> l = 9 + l.  Rows of
every level are in the library's own order; `maps.perm[j]` is the input row of level-0 row j.

Backward: the input gradient is the same convolution kernel over the ADJOINT table with the kernel's slices transposed
(self l: the same table with the offsets mirrored, k -> 26 - k; strided 5 + l <-> transposed 9 + l, same k), skipped when
the input needs no gradient; the weight gradient dW[k] = sum_o x[nbr(o, k)]^T dY[o] is the library's deterministic
segmented MFMA kernel.  Everything runs on the current stream and nothing waits for the device.

precision="f16" (include/umereg_sparse_conv_f16.h; opt-in, the default is "f32"): the operands of the three matrix products are
rounded to f16 (to nearest even) and every sum stays f32.  Forward: `conv_raw(..., precision="f16")`.  Backward: the output
gradient is scaled by 2^e (`grad_scale`: e computed on the device, no host sync) so that its largest magnitude lies in
[2^14, 2^15) before it is rounded; the scaled gradient feeds both gradients and 2^-e is applied to the results (the input
gradient's epilogue scale, one multiplication of dW).  The saved input is the f32 the forward rounded, so dW is the exact
straight-through gradient of the forward.  Inputs, kernels, outputs and gradients are f32 tensors in both precisions."""
import torch

from . import _lib
from . import models as _models

SPARSE_CONV_SIGNATURES = _lib.TABLES["umereg_sparse_conv.h"]
SPARSE_CONV_F16_SIGNATURES = _lib.TABLES["umereg_sparse_conv_f16.h"]
SPARSE_CONV_PAIRS_SIGNATURES = _lib.TABLES["umereg_sparse_conv_pairs.h"]
load_native = _lib.load
N_TABLES, MAX_CH = 13, 256
# input channels per launch of the plain convolution: a longer contraction runs as slices accumulated in order (two-level
# summation; one chain over 27 x 256 products carries about twice the rounding error of eight chains over 27 x 32)
SLICE = 32


def out_level(table):
    """the level whose rows table `table` has one row for"""
    return table if table < 5 else table - 4 if table < 9 else table - 9


def in_level(table):
    """the level whose rows table `table`'s entries index"""
    return table if table < 5 else table - 5 if table < 9 else table - 8


def adjoint(table):
    """(table, mirror) of the adjoint convolution: <conv_t(x; W), y> = <x, conv_t'(y; repack(W, mirror))>"""
    if table < 5:
        return table, True
    return (table + 4, False) if table < 9 else (table - 4, False)


class CoordinateMaps:
    """The five levels and 13 neighbour tables of one coordinate set (int32 [n, 4]: batch index, x, y, z; on the GPU), built
    once with umereg_featnet_build_maps.  Owns the workspace the tables live in -- keep it alive until the backward pass is
    over (the autograd graph of `sparse_conv` does).  `sizes`: rows of the five levels, read once from the device (the one
    host sync; duplicate or out-of-range coordinates raise here); `perm`: int64 [n], the input row of level-0 row j."""

    def __init__(self, coords, batch):
        _lib.on_gpu("CoordinateMaps", coords)
        self.coords = coords.to(torch.int32).contiguous()
        self.n, self.batch, self.device = int(coords.shape[0]), int(batch), coords.device
        if self.n == 0:
            raise ValueError("CoordinateMaps: empty input")
        if self.batch > _models.MAX_BATCH:
            raise ValueError(f"CoordinateMaps: at most {_models.MAX_BATCH} clouds per call, got batch index {self.batch - 1}")
        self.ws = torch.empty(_models.workspace_bytes(self.n, self.batch), dtype=torch.uint8, device=self.device)
        self.status = torch.empty(_models.N_STATUS, dtype=torch.int32, device=self.device)
        _models.build_maps_raw(self.coords, self.batch, self.ws, self.status)
        self.sizes = _models.check_status(self.status)
        self.perm32 = _models.buffer_view(self.ws, self.n, self.batch, _models.BUF_PERM, self.n, torch.int32)[:, 0]
        self.perm = self.perm32.long()
        # the plain convolution's epilogue: acc * 1 + 0 (exact)
        self.ones = torch.ones(MAX_CH, dtype=torch.float32, device=self.device)
        self.zeros = torch.zeros(MAX_CH, dtype=torch.float32, device=self.device)
        self._scratch = None

    def level_coords(self, l):
        return _models.buffer_view(self.ws, self.n, self.batch, _models.BUF_COORDS0 + l, self.sizes[l], torch.int32)

    def scratch(self, nbytes):
        """weight-gradient scratch, grown on demand (one stream: the kernels of successive layers run in order)"""
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._scratch


def _launch(lib, pairs, f16, dev, *args):
    """one launch of the 27-offset convolution on the chosen engine: `args` are the sixteen arguments the three entries share"""
    if pairs:
        _lib.call(dev, lib.umereg_sparse_conv_pairs, *args, int(f16))
    else:
        _lib.call(dev, lib.umereg_sparse_conv_f16 if f16 else lib.umereg_sparse_conv_f32, *args)


def conv_raw(x, kernel, maps, table, transpose=False, mirror=False, precision="f32", scale=None, conv_mode="union"):
    """out[o] = sum_k x[nbr_table(o, k)] @ M[k], M = kernel, or with `transpose` M[k'] = kernel[k]^T (k' = 26 - k if `mirror`):
    x f32 [rows of in_level(table), C] -> [rows of out_level(table), C']; kernel [27, C, C'] ([27, C', C] with `transpose`).
    precision="f16" (include/umereg_featnet_f16.h; forward only, not differentiable): x and the kernel rounded to f16, sums in
    f32, one chain over all channels as in the fused f16 forward; table -1 with a [C, C'] kernel is the 1x1 layer over level 0
    (`transpose`: the kernel is [C', C]); `scale` (f16 only): f32 [>= C'] on the device, the epilogue's factor per output channel
    instead of ones.  conv_mode="pairs" (include/umereg_sparse_conv_pairs.h; the default is "union"): the pair-compacted engine,
    the same values bit for bit (the 1x1 layer runs the union engine's kernel either way)."""
    _models.check_precision(precision)
    pairs = _models.check_conv_mode(conv_mode) == "pairs"
    lib = _lib.load()
    x = _lib.rows(x, "sparse_conv", "input")
    if precision == "f16":
        return _conv_f16(lib, x, kernel, maps, table, transpose, mirror, scale, pairs)
    if scale is not None:
        raise ValueError("sparse_conv: `scale` goes with precision='f16'")
    K, cin, cout = kernel.shape
    if transpose:
        cin, cout = cout, cin
    rows_in, rows_out = maps.sizes[in_level(table)], maps.sizes[out_level(table)]
    if x.shape != (rows_in, cin):
        raise ValueError(f"sparse_conv: table {table} reads [{rows_in}, {cin}] rows, got {tuple(x.shape)}")
    out = torch.empty(rows_out, cout, dtype=torch.float32, device=x.device)
    step = SLICE if cin > SLICE and cin % SLICE == 0 else cin
    if transpose or step < cin:
        kernel = repack_raw(kernel, transpose, mirror, step)        # [cin / step] blocks [27, step, cout]
    else:
        kernel = kernel.contiguous()
    for s in range(cin // step):
        _launch(lib, pairs, False, x.device, maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, table,
                x.data_ptr() + 4 * s * step, x.stride(0), kernel.data_ptr() + 4 * s * 27 * step * cout, step, cout, maps.ones.data_ptr(),
                maps.zeros.data_ptr(), out.data_ptr(), cout, int(s > 0), _lib.stream_ptr(x.device))
    return out


def _conv_f16(lib, x, kernel, maps, table, transpose, mirror, scale=None, pairs=False):
    if kernel.dim() == 2:
        if table != -1:
            raise ValueError("sparse_conv: a [C_in, C_out] kernel is the 1x1 layer: table -1")
        if transpose:
            kernel = kernel.t()
        (cin, cout), rows_in = kernel.shape, maps.sizes[0]
        rows_out = rows_in
        transpose = False
    else:
        if not 0 <= table < N_TABLES:
            raise ValueError(f"sparse_conv: table {table} outside [0, {N_TABLES})")
        K, cin, cout = kernel.shape
        if transpose:
            cin, cout = cout, cin
        rows_in, rows_out = maps.sizes[in_level(table)], maps.sizes[out_level(table)]
    if x.shape != (rows_in, cin):
        raise ValueError(f"sparse_conv: table {table} reads [{rows_in}, {cin}] rows, got {tuple(x.shape)}")
    kernel = repack_raw(kernel, True, mirror, cin) if transpose else kernel.contiguous()
    out = torch.empty(rows_out, cout, dtype=torch.float32, device=x.device)
    if scale is None:
        scale = maps.ones
    elif scale.dtype != torch.float32 or scale.device != x.device or scale.dim() != 1 or scale.numel() < cout or not scale.is_contiguous():
        raise ValueError(f"sparse_conv: scale must be contiguous f32 [>= {cout}] on {x.device}")
    _launch(lib, pairs, True, x.device, maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, table, x.data_ptr(),
            x.stride(0), kernel.data_ptr(), cin, cout, scale.data_ptr(), maps.zeros.data_ptr(), out.data_ptr(), cout, 0,
            _lib.stream_ptr(x.device))
    return out


def conv1_raw(feat, kernel, maps):
    """conv1: feat f32 [n, 1] in INPUT row order, kernel [27, 1, 32] -> [rows of level 0, 32] in level-0 order"""
    lib = _lib.load()
    feat = feat.contiguous()
    if feat.shape != (maps.n, 1) or tuple(kernel.shape) != (27, 1, 32):
        raise ValueError(f"sparse_conv1: features [{maps.n}, 1] and a [27, 1, 32] kernel, got {tuple(feat.shape)} / {tuple(kernel.shape)}")
    out = torch.empty(maps.n, 32, dtype=torch.float32, device=feat.device)
    kernel = kernel.contiguous()
    _lib.call(feat.device, lib.umereg_sparse_conv1_f32, maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n,
              feat.data_ptr(), kernel.data_ptr(), maps.ones.data_ptr(), maps.zeros.data_ptr(), out.data_ptr(),
              _lib.stream_ptr(feat.device))
    return out


def repack_raw(kernel, transpose, mirror, slice):
    """[27, C_in, C_out] -> R / slice blocks [27, slice, C] of M (M[k'] = kernel[k]^T if `transpose` else kernel[k]; R, C its rows
    and columns; k' = 26 - k if `mirror`), as one flat tensor (include/umereg_sparse_conv.h)"""
    lib = _lib.load()
    K, cin, cout = kernel.shape
    kernel = kernel.contiguous()
    out = torch.empty(K * cin * cout, dtype=torch.float32, device=kernel.device)
    _lib.call(kernel.device, lib.umereg_sparse_conv_repack_f32, kernel.data_ptr(), cin, cout, int(bool(transpose)), int(bool(mirror)),
              int(slice), out.data_ptr(), _lib.stream_ptr(kernel.device))
    return out


def wgrad_raw(x, dy, maps, table, precision="f32"):
    """dW [27, C_in, C_out] = sum_o x[nbr_table(o, k)]^T dy[o]; x [rows of in_level(table), C_in] (C_in = 1 included).
    precision="f16" (include/umereg_sparse_conv_f16.h): x and dy rounded to f16, sums in f32, C_in a multiple of 32; dy as it is
    given -- the caller scales it (`grad_scale`) and unscales the result."""
    _models.check_precision(precision)
    lib = _lib.load()
    dy = _lib.rows(dy, "sparse_conv", "output gradient")
    if x.shape[1] == 1:
        x = x.contiguous()
    else:
        x = _lib.rows(x, "sparse_conv", "input")
    cin, cout = x.shape[1], dy.shape[1]
    if x.shape[0] != maps.sizes[in_level(table)] or dy.shape[0] != maps.sizes[out_level(table)]:
        raise ValueError(f"sparse_conv_wgrad: table {table}: {x.shape[0]} input rows / {dy.shape[0]} gradient rows")
    need = int(lib.umereg_sparse_conv_wgrad_scratch_bytes(maps.n, cin, cout))
    if need == 0:
        raise ValueError(f"sparse_conv_wgrad: channels {cin} -> {cout} not supported")
    scratch = maps.scratch(need)
    dw = torch.empty(27, cin, cout, dtype=torch.float32, device=x.device)
    fn = lib.umereg_sparse_conv_wgrad_f16 if precision == "f16" else lib.umereg_sparse_conv_wgrad_f32
    _lib.call(x.device, fn, maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, table, x.data_ptr(), x.stride(0), cin,
              dy.data_ptr(), dy.stride(0), cout, dw.data_ptr(), scratch.data_ptr(), scratch.numel(), _lib.stream_ptr(x.device))
    return dw


E_MAX = 126     # |e| of grad_scale is at most this: 2^e and 2^-e are normal f32 numbers


def _pow2(e):
    """2^e as f32 for an int32 tensor e in [-126, 127], by the exponent field (exact; no pow())"""
    return ((e + 127) << 23).view(torch.float32)


def grad_scale(dy):
    """The backward scaling of include/umereg_sparse_conv_f16.h for an output gradient dy (f32): -> (e, 2^e, 2^-e) as 0-dim
    tensors on dy's device (int32, f32, f32), e = 14 - floor(log2(max |dy|)) so that max |dy 2^e| lies in [2^14, 2^15); e = 0 if
    max |dy| is zero or not finite.  Nothing is read back to the host.  e is held to +-126 (it exceeds that only for
    max |dy| < 2^-112, where the scaled maximum then stays below 2^14)."""
    if dy.numel():
        lo, hi = torch.aminmax(dy.detach())          # one pass, no |dy| temporary; a NaN comes through both
        m = torch.maximum(hi, -lo)
    else:
        m = torch.zeros((), dtype=dy.dtype, device=dy.device)
    _, ex = torch.frexp(m)                           # m = mantissa 2^ex, mantissa in [0.5, 1): floor(log2 m) = ex - 1
    ok = torch.isfinite(m) & (m > 0)
    e = torch.where(ok, 15 - ex.to(torch.int32), torch.zeros_like(ex, dtype=torch.int32)).clamp(-E_MAX, E_MAX).to(torch.int32)
    return e, _pow2(e), _pow2(-e)


def _scale_of(dy, fused):
    """`grad_scale(dy)`, or with `fused` the same three scalars from the kernels of include/umereg_bn_act.h"""
    if fused:
        from . import bn_act
        return bn_act.grad_scale_device(dy)
    return grad_scale(dy)


class _SparseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, maps, table, precision="f32", fused_scale=False, conv_mode="union"):
        ctx.maps, ctx.table, ctx.precision, ctx.fused_scale, ctx.conv_mode = maps, table, precision, fused_scale, conv_mode
        ctx.save_for_backward(x, kernel)
        return conv_raw(x, kernel.detach(), maps, table, precision=precision, conv_mode=conv_mode)

    @staticmethod
    def backward(ctx, dy):
        x, kernel = ctx.saved_tensors
        maps, table = ctx.maps, ctx.table
        dy = dy.contiguous()
        dx = dw = None
        if ctx.precision == "f16":
            # include/umereg_sparse_conv_f16.h: one power-of-two scale per layer, computed on the device; dy 2^e feeds both gradients
            _, up, down = _scale_of(dy, ctx.fused_scale)
            dys = dy * up
            if ctx.needs_input_grad[0]:
                adj, mirror = adjoint(table)
                dx = conv_raw(dys, kernel.detach(), maps, adj, transpose=True, mirror=mirror, precision="f16", scale=maps.ones * down,
                              conv_mode=ctx.conv_mode)
            if ctx.needs_input_grad[1]:
                dw = wgrad_raw(x, dys, maps, table, precision="f16") * down
            return dx, dw, None, None, None, None, None
        if ctx.needs_input_grad[0]:
            adj, mirror = adjoint(table)
            dx = conv_raw(dy, kernel.detach(), maps, adj, transpose=True, mirror=mirror, conv_mode=ctx.conv_mode)
        if ctx.needs_input_grad[1]:
            dw = wgrad_raw(x, dy, maps, table)
        return dx, dw, None, None, None, None, None


class _SparseConv1(torch.autograd.Function):
    """conv1 (C_in = 1): features in input row order; no input gradient (the reference's input features are ones)."""

    @staticmethod
    def forward(ctx, feat, kernel, maps):
        ctx.maps = maps
        ctx.save_for_backward(feat, kernel)
        return conv1_raw(feat, kernel.detach(), maps)

    @staticmethod
    def backward(ctx, dy):
        feat, _ = ctx.saved_tensors
        dw = wgrad_raw(feat.index_select(0, ctx.maps.perm), dy.contiguous(), ctx.maps, 0) if ctx.needs_input_grad[1] else None
        return None, dw, None


def sparse_conv(x, kernel, maps, table, precision="f32", fused_scale=False, conv_mode="union"):
    """Differentiable sparse convolution over table `table` of `maps`.  x: f32 [rows of the table's input level, C_in] in the
    level's row order -- for a [27, 1, 32] kernel (conv1, table 0): [n, 1] in INPUT row order, and it may not require grad;
    kernel: [27, C_in, C_out].  -> f32 [rows of the table's output level, C_out].  precision="f16": f16 operands in the forward
    and in both gradients (module docstring); a C_in = 1 kernel (conv1) stays f32 either way.  fused_scale=True (f16 only): the
    backward takes its scale from `bn_act.grad_scale_device` (two kernels) instead of `grad_scale` (the same scalars bit for bit).
    conv_mode="pairs" (include/umereg_sparse_conv_pairs.h): the forward and the input gradient -- the same operator over the adjoint
    table -- run on the pair-compacted engine, bit for bit the values of the default "union"; the weight gradient has no mode, and
    neither has conv1."""
    _models.check_precision(precision)
    _models.check_conv_mode(conv_mode)
    if not 0 <= table < N_TABLES:
        raise ValueError(f"sparse_conv: table {table} outside [0, {N_TABLES})")
    _lib.on_gpu("sparse_conv", x, kernel)
    if kernel.dim() != 3 or kernel.shape[0] != 27:
        raise ValueError(f"sparse_conv: kernel must be [27, C_in, C_out], got {tuple(kernel.shape)}")
    if kernel.shape[1] == 1:
        if table != 0:
            raise ValueError("sparse_conv: a C_in = 1 kernel runs over table 0 only (conv1)")
        if x.requires_grad:
            raise RuntimeError("sparse_conv: conv1 has no input gradient (the network's input features are constants); "
                               "detach the input features")
        return _SparseConv1.apply(x, kernel, maps)
    return _SparseConv.apply(x, kernel, maps, table, precision, bool(fused_scale), conv_mode)


def _block_wgrad(x, dy):
    n, r = x.shape[0], _Linear.ROWS          # x^T dy summed in blocks of ROWS rows, then over the blocks
    pad = (-n) % r
    xp = torch.nn.functional.pad(x, (0, 0, 0, pad)).view(-1, r, x.shape[1])
    dp = torch.nn.functional.pad(dy, (0, 0, 0, pad)).view(-1, r, dy.shape[1])
    return torch.bmm(xp.transpose(1, 2), dp).sum(dim=0)


class _Linear(torch.autograd.Function):
    """x @ W for the 1x1 layers.  torch's own matmul, except that the weight gradient x^T dy -- a contraction over all rows --
    is summed in blocks of ROWS rows and then over the blocks: one chain over 10^5 rows would carry several times the rounding
    error of every other gradient of the network."""
    ROWS = 256

    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return x @ W

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dx = dy @ W.t() if ctx.needs_input_grad[0] else None
        dw = _block_wgrad(x, dy) if ctx.needs_input_grad[1] else None
        return dx, dw


class _LinearF16(torch.autograd.Function):
    """mlp1 with f16 operands (include/umereg_sparse_conv_f16.h): forward and input gradient are the HIP convolution with
    table -1 (x and W, the scaled dy and W^T rounded to f16; sums f32); the weight gradient stays `_Linear`'s f32 block sum."""

    @staticmethod
    def forward(ctx, x, W, maps, fused_scale=False):
        ctx.maps, ctx.fused_scale = maps, fused_scale
        ctx.save_for_backward(x, W)
        return conv_raw(x, W.detach(), maps, -1, precision="f16")

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            _, up, down = _scale_of(dy, ctx.fused_scale)
            dx = conv_raw(dy * up, W.detach(), ctx.maps, -1, transpose=True, precision="f16", scale=ctx.maps.ones * down)
        if ctx.needs_input_grad[1]:
            dw = _block_wgrad(x, dy)
        return dx, dw, None, None


def linear(x, W, precision="f32", maps=None, fused_scale=False):
    """x [rows, C_in] @ W [C_in, C_out] with a block-summed weight gradient (the 1x1 layers of the network).  precision="f16"
    (mlp1): x [rows of level 0 of `maps`, C_in], operands of the forward and of the input gradient rounded to f16, channel counts
    multiples of 32; the weight gradient stays the f32 block sum.  fused_scale: as in `sparse_conv` (f16 only)."""
    _models.check_precision(precision)
    if precision == "f16":
        if maps is None:
            raise ValueError("linear: precision='f16' runs on the HIP convolution and needs the CoordinateMaps of its rows (maps=...)")
        _lib.on_gpu("linear", x, W)
        return _LinearF16.apply(x, W, maps, bool(fused_scale))
    return _Linear.apply(x, W)
