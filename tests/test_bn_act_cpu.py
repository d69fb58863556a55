"""CPU: the ground tests/test_bn_act_gpu.py stands on -- the fp64 restatement of include/umereg_bn_act.h (tests/bn_act_ref.py)
against torch's own batch norm and autograd in fp64, the gradient-scale restatement against `sparse_conv.grad_scale` bit for bit,
the header's symbols and the slab plan (csrc/bn_act_plan.h through tests/bn_act_plan_host.cpp), every argument refusal of the C
entries without a GPU, and the properties of the exact-data clouds."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bn_act_ref as bref
from umeregrobust_amd import bn_act         # noqa: F401  (everything here is ground for this module: without it nothing is checked)

REPO =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "umereg_bn_act.h")


# ---- 1. the restatement is torch's batch norm ---------------------------------------------------------------------------------------

def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(float(np.abs(b).max()), 1e-300))


@pytest.mark.parametrize("train,res,relu", list(itertools.product([True, False], repeat=3)))
def test_restatement_is_torch_batch_norm_in_fp64(train, res, relu):
    n, C, eps, mom = 77, 32, 1e-5, 0.1
    g = torch.Generator().manual_seed(5 + 4 * train + 2 * res + relu)
    draw = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)         # noqa: E731  (f32 inputs, as the kernels get them)
    x, r, dy = draw(n, C) * 2 + 0.5, draw(n, C), draw(n, C)
    gamma, beta, rm, rv = draw(C), draw(C), draw(C), torch.rand(C, generator=g) + 0.5
    bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=mom).double().train(train)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    xt, rt = x.double().requires_grad_(), r.double().requires_grad_()
    y = bn(xt) + rt if res else bn(xt)
    y = torch.relu(y) if relu else y
    y.backward(dy.double())
    f = bref.forward(x.numpy(), gamma.numpy(), beta.numpy(), r.numpy() if res else None, relu, train, eps, rm.numpy(), rv.numpy())
    b = bref.backward(dy.numpy(), x.numpy(), f["y"], gamma.numpy(), f["mean"], f["invstd"], train, relu)
    assert rel(f["y"], y.detach().numpy()) <= 1e-12
    assert rel(b["dx"], xt.grad.numpy()) <= 1e-12
    assert rel(b["dgamma"], bn.weight.grad.numpy()) <= 1e-12 and rel(b["dbeta"], bn.bias.grad.numpy()) <= 1e-12
    if res:
        assert rel(b["dres"], rt.grad.numpy()) <= 1e-12
    if train:
        m2, v2, t2 = bref.running_update(rm.numpy(), rv.numpy(), 0, f["mean"], f["var"], n, mom)
        assert t2 == int(bn.num_batches_tracked) == 1
    else:
        m2, v2 = rm.double().numpy(), rv.double().numpy()
        assert int(bn.num_batches_tracked) == 0
    assert rel(m2, bn.running_mean.numpy()) <= 1e-12 and rel(v2, bn.running_var.numpy()) <= 1e-12


# ---- 2. the gradient-scale restatement ----------------------------------------------------------------------------------------------

def scale_bits(t):
    e, up, down = t
    return (int(e), int(np.asarray(up, dtype=np.float32).view(np.uint32)), int(np.asarray(down, dtype=np.float32).view(np.uint32)))


@pytest.mark.parametrize("v", bref.SCALE_VALUES, ids=lambda v: f"{v:.6g}")
def test_grad_scale_restatement_is_sparse_conv_grad_scale(v):
    from umeregrobust_amd import sparse_conv as sc
    for sign in (1.0, -1.0):
        for n, at in ((1, 0), (65, 0), (65, 64), (300, 123)):
            a = np.full(n, bref.scale_background(v), np.float32)
            a[at] = sign * v
            e, up, down = sc.grad_scale(torch.from_numpy(a))
            assert e.dtype == torch.int32 and up.dtype == down.dtype == torch.float32
            assert scale_bits(bref.grad_scale(a)) == scale_bits((e, up.numpy(), down.numpy())), (v, sign, n, at)
    assert scale_bits(bref.grad_scale(np.zeros(0, np.float32))) == scale_bits([t.numpy() for t in sc.grad_scale(torch.zeros(0))])
    # the contract's corners, by hand
    want = {0.0: 0, 2.0 ** -120: 126, 2.0 ** -113: 126, 2.0 ** 14: 0, 2.0 ** 15 - 1: 0, 2.0 ** 15: -1, float(np.finfo(np.float32).max): -113}
    if v in want:
        assert int(bref.grad_scale(np.array([v], np.float32))[0]) == want[v]
    elif not np.isfinite(v):
        assert scale_bits(bref.grad_scale(np.array([1.0, v], np.float32))) == (0, 0x3f800000, 0x3f800000)


# ---- 3. export and plan ---------------------------------------------------------------------------------------------------------------

def test_every_symbol_of_the_header_is_exported():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import bn_act
    assert {"umereg_bn_act_scratch_bytes", "umereg_bn_act_forward_f32", "umereg_bn_act_backward_f32", "umereg_grad_scale_f32"} \
        <= set(bn_act.BN_ACT_SIGNATURES)
    umereg_h = open(os.path.join(REPO, "include", "umereg.h")).read()
    assert "bn_act" not in umereg_h and "grad_scale" not in umereg_h
    assert int(re.search(r"#define UMEREG_BN_ACT_MAX_CH (\d+)", open(HEADER).read()).group(1)) == bn_act.MAX_CH == bref.MAX_C


PLAN_N = sorted(set(list(range(1, 700)) + [1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 50000, 65535, 65536, 65537, 262144, 262145, 800000,
                                           8388608, 8388609, 2 ** 31 - 1]))
PLAN_C = list(range(32, 257, 32))
GS_COUNTS = [0, 1, 63, 65, 8191, 8192, 8193, 256 * 8192, 256 * 8192 + 1, 25600000, 2 ** 40]


@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's bn_plan cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("bn_act_plan") / "bn_act_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "bn_act_plan_host.cpp"), "-o", exe])
    pairs = [(n, C) for n in PLAN_N for C in PLAN_C]
    text = "".join(f"{n} {C}\n" for n, C in pairs) + "".join(f"-1 {c}\n" for c in GS_COUNTS) + "5 16\n5 48\n5 288\n"
    lines = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    head = lines[0].split()
    return {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}, pairs, [ln for ln in lines[1:] if ln]


def test_plan_restates_the_header(header_plan):
    consts, pairs, lines = header_plan
    assert consts == dict(kBnThreads=bref.THREADS, kBnMaxC=bref.MAX_C, kBnMinPasses=bref.MIN_PASSES, kBnMaxSlabs=bref.MAX_SLABS,
                          kGsChunk=bref.GS_CHUNK, kGsWidth=bref.GS_WIDTH)
    assert len(lines) == len(pairs) + len(GS_COUNTS) + 3 and lines[-3:] == ["refused"] * 3
    rows = np.array([[int(v) for v in ln.split()] for ln in lines[:len(pairs)]], np.int64)
    mine = np.array([bref.plan(n, C) + (bref.scratch_bytes(n, C),) for n, C in pairs], np.int64)
    bad = np.nonzero((mine != rows).any(axis=1))[0]
    assert bad.size == 0, ([pairs[i] for i in bad[:5]], rows[bad[:5]], mine[bad[:5]])
    assert [int(ln) for ln in lines[len(pairs):-3]] == [bref.gs_partials(c) for c in GS_COUNTS]
    # what every plan must satisfy for the kernels to cover each row once and stay inside their scratch and LDS
    n, C = np.array(pairs).T
    unit, slab, slabs, width, scratch = rows.T
    assert (unit * (C // 4) <= bref.THREADS).all() and (unit * C <= 4 * bref.THREADS).all() and (unit >= 4).all()
    assert (slab % unit == 0).all() and (slab >= bref.MIN_PASSES * unit).all()
    assert (slabs >= 1).all() and (slabs <= bref.MAX_SLABS).all() and ((slabs - 1) * slab < n).all() and (slabs * slab >= n).all()
    assert (width >= 1).all() and (width * C <= bref.THREADS).all() and (scratch == slabs * 2 * C * 8).all()
    # the slab length depends on (n, C) alone and only grows where 256 slabs no longer cover n
    for c in bref.CHANNELS:
        assert bref.plan(2, c)[1] == 4096 // c == bref.plan(1024 * (1024 // c), c)[1]
        assert bref.plan(1024 * (1024 // c) + 1, c)[1] == 5 * (1024 // c)


def test_the_library_s_scratch_query_is_the_plan():
    from umeregrobust_amd import bn_act
    lib = bn_act.load_native()
    for n in (1, 2, 127, 128, 129, 4097, 50000, 800000):
        for C in PLAN_C:
            assert lib.umereg_bn_act_scratch_bytes(n, C) == bref.scratch_bytes(n, C)
    for bad in ((0, 32), (-1, 32), (5, 0), (5, 16), (5, 48), (5, 288)):
        assert lib.umereg_bn_act_scratch_bytes(*bad) == 0
    for c in GS_COUNTS:
        assert lib.umereg_grad_scale_scratch_bytes(c) == 4 * max(1, bref.gs_partials(c))
    assert lib.umereg_grad_scale_scratch_bytes(2 ** 40 + 1) == 0


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_device_probe():
    from umeregrobust_amd import bn_act
    lib = bn_act.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    q = p + (1 << 15)                                     # a second buffer: outputs may not alias inputs
    n, C = 8, 32
    need = lib.umereg_bn_act_scratch_bytes(n, C)
    assert need == 2 * C * 8
    fwd_args = (("x", p), ("ld_x", C), ("residual", p + 4096), ("ld_res", C), ("n", n), ("C", C), ("gamma", p), ("beta", p), ("running_mean", p),
                ("running_var", p), ("num_batches_tracked", p), ("train", 1), ("relu", 1), ("eps", 1e-5), ("momentum", 0.1), ("y", q), ("ld_y", C),
                ("save_mean", q + 8192), ("save_invstd", q + 8192 + 1024), ("scratch", q + 16384), ("scratch_bytes", need), ("stream", None))
    bwd_args = (("dy", p), ("ld_dy", C), ("x", p + 4096), ("ld_x", C), ("y", p + 8192), ("ld_y", C), ("n", n), ("C", C), ("gamma", p),
                ("save_mean", p), ("save_invstd", p), ("train", 1), ("relu", 1), ("dx", q), ("ld_dx", C), ("dres", q + 4096), ("ld_dres", C),
                ("dgamma", q + 8192), ("dbeta", q + 8192 + 1024), ("scratch", q + 16384), ("scratch_bytes", need), ("stream", None))
    fwd = lambda **kw: lib.umereg_bn_act_forward_f32(*[kw.get(k, d) for k, d in fwd_args])          # noqa: E731
    bwd = lambda **kw: lib.umereg_bn_act_backward_f32(*[kw.get(k, d) for k, d in bwd_args])         # noqa: E731
    gs = lambda **kw: lib.umereg_grad_scale_f32(*[kw.get(k, d) for k, d in (                         # noqa: E731
        ("dy", p), ("count", 100), ("e", q), ("up", q + 4), ("down", q + 8), ("scratch", q + 16), ("scratch_bytes", 4), ("stream", None))])
    EINVAL, ENODEV, EWORKSPACE = -1, -2, -3
    # null pointers where one is needed
    for k in ("x", "gamma", "beta", "y", "save_mean", "save_invstd"):
        assert fwd(**{k: None}) == EINVAL, k
        assert b"null" in lib.umereg_last_error()
    for k in ("dy", "x", "y", "gamma", "save_mean", "save_invstd"):
        assert bwd(**{k: None}) == EINVAL, k
    for k in ("e", "up", "down", "dy"):
        assert gs(**{k: None}) == EINVAL, k
    # n == 0, train mode with one row, C off the list
    for f in (fwd, bwd):
        for kw in (dict(n=0), dict(n=-3), dict(n=1), dict(C=0), dict(C=16), dict(C=48), dict(C=288, ld_x=288, ld_y=288)):
            assert f(**kw) == EINVAL, kw
    assert b"more than one value" in (fwd(n=1), lib.umereg_last_error())[1]
    # a short or missing scratch
    for f in (fwd, bwd):
        assert f(scratch_bytes=need - 1) == EWORKSPACE and f(scratch=None) == EWORKSPACE and f(scratch=q + 16384 + 8) == EWORKSPACE
    assert gs(scratch_bytes=3) == EWORKSPACE and gs(scratch=None) == EWORKSPACE and gs(count=8193) == EWORKSPACE
    # rows: stride and alignment; aliasing; the running statistics go together; eval mode needs them; the sums in train mode
    for kw in (dict(ld_x=C - 4), dict(ld_x=C + 2), dict(x=p + 4), dict(y=q + 8), dict(residual=p + 4100), dict(y=p), dict(y=p + 4096),
               dict(running_mean=None), dict(num_batches_tracked=None), dict(train=0, running_var=None), dict(eps=-1.0), dict(momentum=1.5)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(ld_dy=C - 4), dict(dy=p + 8), dict(dx=p), dict(dres=p + 8192), dict(dres=q), dict(dgamma=None), dict(dbeta=None),
               dict(dgamma=None, dbeta=None), dict(train=0, dgamma=None, dbeta=None, dx=None, dres=None)):
        assert bwd(**kw) == EINVAL, kw
    assert gs(dy=p + 4) == EINVAL and gs(count=2 ** 40 + 1, scratch_bytes=1 << 30) == EINVAL
    if lib.umereg_device_count(None, 0) == 0:
        # everything in order: only now is a device looked for
        assert fwd() == ENODEV and b"no CPU fallback" in lib.umereg_last_error()
        assert fwd(residual=None) == ENODEV and fwd(train=0, scratch=None, scratch_bytes=0, num_batches_tracked=None) == ENODEV
        assert fwd(running_mean=None, running_var=None, num_batches_tracked=None) == ENODEV
        assert bwd() == ENODEV and bwd(dx=None) == ENODEV and bwd(dres=None) == ENODEV and bwd(relu=0, y=None) == ENODEV
        assert bwd(train=0, dgamma=None, dbeta=None, scratch=None, scratch_bytes=0) == ENODEV
        assert gs() == ENODEV and gs(count=0, dy=None) == ENODEV


def test_python_entry_points_refuse_cpu_tensors_and_bad_modules():
    from umeregrobust_amd import bn_act
    from umeregrobust_amd.models import ResUNetSmall2
    bn = torch.nn.BatchNorm1d(32)
    for call in (lambda: bn_act.batch_norm_act(torch.zeros(4, 32), bn), lambda: bn_act.grad_scale_device(torch.zeros(4)),
                 lambda: bn_act.relu(torch.zeros(4, 32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="momentum=None"):
        bn_act.batch_norm_act(torch.zeros(4, 32), torch.nn.BatchNorm1d(32, momentum=None))
    with pytest.raises(TypeError):
        bn_act.batch_norm_act(torch.zeros(4, 32), torch.nn.LayerNorm(32))
    with pytest.raises(ValueError, match="trainable=True"):
        ResUNetSmall2(fused_norm=True)
    m = ResUNetSmall2(trainable=True, fused_norm=True)
    assert m.fused_norm and list(m.state_dict()) == list(ResUNetSmall2(trainable=True).state_dict())
    assert not ResUNetSmall2(trainable=True).fused_norm


# ---- 5. the exact-data clouds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", bref.CHANNELS)
def test_exact_clouds_have_the_properties_their_tests_rely_on(C):
    rows = bref.edge_rows(C)
    unit, S, _, W = bref.plan(2, C)
    assert rows == sorted({2, 3, S - 1, S, S + 1, 2 * S + 1, W * S + 1}) and S == 4096 // C and W == 256 // C
    assert all(bref.plan(n, C)[1] == S for n in rows)                   # one slab length over the whole list
    assert [bref.plan(n, C)[2] for n in (S - 1, S, S + 1, 2 * S + 1, W * S + 1)] == [1, 1, 2, 3, W + 1]
    even = [n for n in rows if n % 2 == 0]
    assert 2 in even and S in even and S & (S - 1) == 0
    for n in even:
        x, m, k, sign = bref.exact_cloud(n, C, 100 + n)
        assert x.dtype == np.float32 and x.shape == (n, C)
        f = bref.forward(x, np.ones(C), np.zeros(C), eps=0.0)
        assert np.array_equal(f["mean"], m.astype(np.float64)) and np.array_equal(f["var"], 4.0 ** k)
        assert np.array_equal(f["invstd"], 2.0 ** -k) and np.array_equal(f["y"], sign)
        assert (np.abs(sign) == 1).all() and (sign.sum(axis=0) == 0).all()
        if n > 2:
            assert len({tuple(sign[:, c]) for c in range(C)}) > 1          # permuted per channel
        dy = bref.balanced_dy(sign, n)
        b = bref.backward(dy, x, f["y"], np.ones(C), f["mean"], f["invstd"])
        assert not b["dbeta"].any() and not b["dgamma"].any()
        assert n == 2 or np.abs(dy).max() > 0
