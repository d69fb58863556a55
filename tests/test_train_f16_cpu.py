"""CPU: the f16-operand training mode (include/umereg_sparse_conv_f16.h) -- its restatement (tests/featnet_f16_grad_ref.py)
against fp64 autograd, the backward scaling's exponent, the host side of the new header and the Python surface, and the
derivation of the whole-network gradient margins that tests/test_train_f16_gpu.py applies.

The margins.  Per parameter, G64 = fp64 autograd of the unrounded network, G16 = fp64 autograd through the restatement, GE16 =
G16 - G64: the error the CONTRACT has, computed without the code under test.  A correct implementation differs from G16 by
f32-sized terms (its f32 sums), a wrong rounding (truncation is the mildest) has another error.  Measured here on the clouds of
the GPU test, as the worst parameter's rms(g - G64) / rms(GE16) and max |g - G64| / max |GE16|:

                                 restatement in fp32         truncated operands (fp64)
                                   rms      max                 rms      max
    small (6000), eval            1.10     1.32                 7.28    13.07
    small (6000), train           1.24     1.40                 2.29     1.99
    2 x 3000, eval                1.22     1.29                 6.68    11.04
    2 x 3000, train               1.13     1.41                 2.23     2.33

(the f32-sized terms are not negligible here: GE16 is only 1.4e-4 .. 1.5e-3 of a gradient's rms, because rounding errors
average out over thousands of rows while an f32 sum's do less so.)  M_RMS = 1.7 lies between 1.24 and 2.23, M_MAX = 1.7 between
1.41 and 1.99."""
import inspect
import os

import numpy as np
import pytest
import torch

import featnet_f16_grad_ref as g16
import featnet_f16_ref as f16ref
import featnet_grad_ref as gref
import test_featnet_gpu as fg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_RMS, M_MAX = 1.7, 1.7


def nearest(c, m):
    """the m voxels of a cloud nearest to the sensor, in the cloud's row order"""
    return c[np.sort(np.argsort((c[:, 1:] ** 2).sum(1), kind="stable")[:m])]


def small_cloud():
    return nearest(fg.voxel_cloud(0, "KT"), 6000)              # (test_sparse_grad_gpu.small_cloud)


def two_3000():
    """a batch of two 3 000-point clouds"""
    return np.concatenate([nearest(fg.voxel_cloud(3, "NS"), 3000), nearest(fg.voxel_cloud(4, "KT", batch=1), 3000)])


NET_CLOUDS = {"small": small_cloud, "two_3000": two_3000}


def gradient_errors(g, g64, G16):
    """per parameter: (rms(g - G64) / rms(GE16), max |g - G64| / max |GE16|)"""
    out = {}
    for k in g64:
        ge = G16[k] - g64[k]
        d = g[k].double().cpu() - g64[k]
        out[k] = (g16.rms(d) / g16.rms(ge), float(d.abs().max() / ge.abs().max()))
    return out


def helper_grads(net, tables, sd_np, dtype, train, masks, G, **kw):
    sd = gref.state(sd_np, dtype)
    out, _ = net(tables, torch.ones(G.shape[0], 1, dtype=dtype), sd, train=train, masks=masks, **kw)
    (out * G.to(dtype)).sum().backward()
    return {k: v.grad.double() for k, v in sd.items() if v.requires_grad}


# ---- 1: the restatement is the straight-through gradient ------------------------------------------------------------------------

def test_restatement_backward_is_fp64_autograd_of_the_rounded_forward():
    """With a dY that the scaled rounding leaves as it is (small integers), the restatement's dx and dW equal fp64 autograd of
    conv(r16(x), r16(W)) with respect to the rounded operands: nothing but the rounding of dY separates the two."""
    rng = np.random.default_rng(2)
    c = np.unique(rng.integers(-12, 12, (700, 3)), axis=0)
    c = np.concatenate([np.zeros((len(c), 1), np.int64), c[rng.permutation(len(c))]], axis=1)
    tables = gref.Tables(c)
    g = torch.Generator().manual_seed(5)
    for t, cin, cout in ((0, 32, 64), (5, 32, 64), (9, 64, 32), (2, 32, 32)):
        x = torch.randn(tables.sizes[gref.in_level(t)], cin, generator=g, dtype=torch.float64).requires_grad_()
        W = torch.randn(27, cin, cout, generator=g, dtype=torch.float64).requires_grad_()
        dy = torch.randint(-7, 8, (tables.sizes[gref.out_level(t)], cout), generator=g).double()
        y = g16.conv(x, W, tables, t)
        y.backward(dy)
        xq = torch.from_numpy(f16ref.r16(x.detach().numpy())).requires_grad_()
        Wq = torch.from_numpy(f16ref.r16(W.detach().numpy())).requires_grad_()
        assert not torch.equal(xq, x.detach())
        yq = gref.conv(xq, Wq, tables, t)
        yq.backward(dy)
        assert torch.equal(y.detach(), yq.detach())
        for got, want in ((x.grad, xq.grad), (W.grad, Wq.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), t
    # mlp1: the same for dx; dW is the unrounded x^T dY
    x = torch.randn(50, 96, generator=g, dtype=torch.float64).requires_grad_()
    W = torch.randn(96, 64, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randint(-7, 8, (50, 64), generator=g).double()
    g16.linear(x, W).backward(dy)
    Wq = torch.from_numpy(f16ref.r16(W.detach().numpy()))
    assert float((x.grad - dy @ Wq.t()).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert torch.equal(W.grad, x.detach().t() @ dy)


# ---- 2: the exponent ------------------------------------------------------------------------------------------------------------

def test_scale_exponent():
    from umeregrobust_amd import sparse_conv as sc
    cases = []
    for j in (-60, -1, 0, 15):
        for f in (1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23):
            cases.append((np.float32(2.0 ** j) * np.float32(f), 14 - (j if f >= 1.0 else j - 1)))
    for m, want in cases:
        dy = torch.zeros(5, 32)
        dy[3, 7] = -float(m)
        dy[1, 2] = float(m) / 3
        e, up, down = sc.grad_scale(dy)
        assert e.dtype == torch.int32 and up.dtype == down.dtype == torch.float32 and e.dim() == up.dim() == down.dim() == 0
        assert int(e) == want == g16.scale_exponent(dy), (m, int(e), want)
        assert float(up) == 2.0 ** want and float(down) == 2.0 ** -want
        top = float((dy * up).abs().max())
        assert 2.0 ** 14 <= top < 2.0 ** 15 and top == float(m) * 2.0 ** want, (m, top)
    for bad in (0.0, float("inf"), -float("inf"), float("nan")):
        dy = torch.ones(4, 32)
        if bad == 0.0:
            dy.zero_()
        else:
            dy[2, 2] = bad
        e, up, down = sc.grad_scale(dy)
        assert int(e) == 0 == g16.scale_exponent(dy) and float(up) == 1.0 and float(down) == 1.0, bad
    e, up, down = sc.grad_scale(torch.zeros(0, 32))
    assert int(e) == 0
    # the documented clamp: beyond 2^126 there is no normal f32 scale
    e, up, down = sc.grad_scale(torch.full((1, 32), 2.0 ** -140))
    assert int(e) == sc.E_MAX == 126 and float(up) == 2.0 ** 126 and float(down) == 2.0 ** -126


# ---- 3: the header's host side and the surface ------------------------------------------------------------------------------------

def test_f16_training_table_mirrors_its_header():
    """(keys, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import sparse_conv
    syms = ["umereg_sparse_conv_wgrad_f16"]
    assert syms == sorted(sparse_conv.SPARSE_CONV_F16_SIGNATURES)
    assert len(sparse_conv.SPARSE_CONV_F16_SIGNATURES[syms[0]][1]) == 15
    assert sparse_conv.SPARSE_CONV_F16_SIGNATURES[syms[0]] == sparse_conv.SPARSE_CONV_SIGNATURES["umereg_sparse_conv_wgrad_f32"]
    assert "umereg_sparse_conv_f16.h" in open(os.path.join(REPO, "include", "umereg_featnet_f16.h")).read()


def test_wgrad_f16_checks_arguments_before_the_device():
    from umeregrobust_amd import sparse_conv
    lib = sparse_conv.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    n = 100
    ws_bytes = lib.umereg_featnet_workspace_bytes(n, 1)
    need = lib.umereg_sparse_conv_wgrad_scratch_bytes(n, 64, 32)
    assert need == lib.umereg_sparse_conv_wgrad_segments(n, 64, 32) * 27 * 64 * 32 * 4 > 0
    call = lambda **kw: lib.umereg_sparse_conv_wgrad_f16(*[kw.get(k, d) for k, d in (          # noqa: E731
        ("ws", p), ("ws_bytes", ws_bytes), ("status", p), ("n", n), ("table", 0), ("x", p), ("ld_in", 64), ("cin", 64), ("dy", p),
        ("ld_dy", 32), ("cout", 32), ("dw", p), ("scratch", p), ("scratch_bytes", need), ("stream", None))])
    for k in ("ws", "status", "x", "dy", "dw", "scratch"):
        assert call(**{k: None}) == -1 and b"null" in lib.umereg_last_error(), k
    for kw in (dict(n=0), dict(table=13), dict(table=-1), dict(cin=1, ld_in=1), dict(cin=48), dict(cout=16), dict(cout=288, ld_dy=288),
               dict(cin=0), dict(ld_in=32), dict(ld_dy=16)):
        assert call(**kw) == -1, kw
    assert call(cin=1, ld_in=1) == -1 and b"C_in = 1 stays f32" in lib.umereg_last_error()
    assert call(scratch_bytes=need - 1) == -3 and b"scratch" in lib.umereg_last_error()          # UMEREG_EWORKSPACE
    assert call(ws_bytes=ws_bytes - 1) == -3 and call(ws=p + 16) == -3 and call(scratch=p + 4) == -3
    if lib.umereg_device_count(None, 0) == 0:
        assert call() == -2 and b"no CPU fallback" in lib.umereg_last_error()                      # UMEREG_ENODEV


def test_train_precision_surface(capsys):
    from umeregrobust_amd import models, sparse_conv, train_coloring
    from umeregrobust_amd.sparse import SparseTensor
    assert inspect.signature(models.ResUNetSmall2.__init__).parameters["train_precision"].default == "f32"
    assert inspect.signature(sparse_conv.sparse_conv).parameters["precision"].default == "f32"
    assert inspect.signature(sparse_conv.wgrad_raw).parameters["precision"].default == "f32"
    assert inspect.signature(sparse_conv.linear).parameters["precision"].default == "f32"
    assert inspect.signature(train_coloring.run).parameters["train_precision"].default == "f32"
    assert models.PRECISIONS == ("f32", "f16")
    m = models.ResUNetSmall2(trainable=True)
    assert m.train_precision == "f32" and m.precision == "f32"
    m = models.ResUNetSmall2(trainable=True, train_precision="f16")
    assert m.train_precision == "f16" and m.precision == "f32"
    assert models.ResUNetSmall2(trainable=True, train_precision="f16", precision="f16").precision == "f16"
    with pytest.raises(ValueError, match="bf16"):
        models.ResUNetSmall2(trainable=True, train_precision="bf16")
    for kw in (dict(), dict(trainable=False), dict(precision="f16")):
        with pytest.raises(ValueError, match="train_precision='f16'.*trainable=True"):
            models.ResUNetSmall2(train_precision="f16", **kw)
    x, W = torch.zeros(2, 32), torch.zeros(27, 32, 32)
    with pytest.raises(ValueError, match="bf16"):
        sparse_conv.sparse_conv(x, W, None, 0, precision="bf16")
    with pytest.raises(ValueError, match="bf16"):
        sparse_conv.wgrad_raw(x, x, None, 0, precision="bf16")
    with pytest.raises(ValueError, match="bf16"):
        sparse_conv.linear(x, W[0], precision="bf16")
    with pytest.raises(ValueError, match="maps"):
        sparse_conv.linear(x, W[0], precision="f16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_conv.sparse_conv(x, W, None, 0, precision="f16")
    # what exists keeps its behaviour: an f16 inference module with the default train_precision is still inference only,
    # and with train_precision="f16" the layer-wise path is reached (here: its refusal of CPU tensors)
    st = SparseTensor(torch.ones(2, 1), coordinates=torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="precision='f16'.*inference only"):
        models.ResUNetSmall2(precision="f16", trainable=True).train()(st)
    for precision in models.PRECISIONS:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            models.ResUNetSmall2(precision=precision, trainable=True, train_precision="f16").train()(st)
    # the driver: the command line names its choices, and a non-finite loss names the mode
    with pytest.raises(SystemExit):
        train_coloring.main(["--train-precision", "bf16"])
    err = capsys.readouterr().err
    assert "--train-precision" in err and "'f32', 'f16'" in err
    m16 = models.ResUNetSmall2(trainable=True, train_precision="f16")
    with pytest.raises(FloatingPointError, match="train_precision='f16'"):
        train_coloring.check_loss_is_finite({"total": float("nan")}, m16)
    with pytest.raises(FloatingPointError, match="train_precision='f16'"):
        train_coloring.check_loss_is_finite({"total": float("inf")}, m16)
    train_coloring.check_loss_is_finite({"total": 1.5}, m16)
    train_coloring.check_loss_is_finite({"total": float("nan")}, models.ResUNetSmall2(trainable=True))     # f32: as before


# ---- 4: where the gradient margins come from ------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(NET_CLOUDS))
def test_gradient_margins_sit_between_the_fp32_restatement_and_truncation(name, train):
    """The measurement of the module docstring: the restatement in fp32 passes the gates of tests/test_train_f16_gpu.py, the
    restatement with truncated operands does not (ReLU decisions: the unrounded fp64 run's, forced onto every run)."""
    coords = NET_CLOUDS[name]()
    tables, n = gref.Tables(coords), len(coords)
    sd_np = fg.f32_state(fg.seeded())
    G = torch.randn(n, 32, generator=torch.Generator().manual_seed(n), dtype=torch.float32)
    with torch.no_grad():
        _, it = gref.network(tables, torch.ones(n, 1, dtype=torch.float64), gref.state(sd_np, torch.float64, False), train=train)
    masks = it["mask"]
    g64 = helper_grads(gref.network, tables, sd_np, torch.float64, train, masks, G)
    G16 = helper_grads(g16.network, tables, sd_np, torch.float64, train, masks, G)
    rel = [g16.rms(G16[k] - g64[k]) / g16.rms(g64[k]) for k in g64]
    assert 5e-5 < min(rel) and max(rel) < 5e-3, (min(rel), max(rel))
    e32 = gradient_errors(helper_grads(g16.network, tables, sd_np, torch.float32, train, masks, G), g64, G16)
    et = gradient_errors(helper_grads(g16.network, tables, sd_np, torch.float64, train, masks, G, q=f16ref.t16_op), g64, G16)
    worst = lambda e: (max(v[0] for v in e.values()), max(v[1] for v in e.values()))        # noqa: E731
    (r32, m32), (rt, mt) = worst(e32), worst(et)
    print(f"[f16 training margins {name} {'train' if train else 'eval'}] GE16 / |G64| rms {min(rel):.2e} .. {max(rel):.2e}; worst parameter: "
          f"fp32 restatement rms {r32:.3f} max {m32:.3f}; truncation rms {rt:.3f} max {mt:.3f}")
    assert r32 <= M_RMS and m32 <= M_MAX, (r32, m32)
    assert rt > M_RMS and mt > M_MAX, (rt, mt)
