"""CPU: the ground the trainable ResUNetSmall2 stands on -- the differentiable restatement (tests/featnet_grad_ref.py) against
the fp64 forward restatement and torch's own batch norm, the adjoint-table identity on all 13 neighbour tables, the host
side of include/umereg_sparse_conv.h, `loss.MyInfoNCELossNoSeg` against the reference's own class (tests/golden/g13_infonce.npz,
tools/gen_infonce_golden.py), and the refusals of the trainable model without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import featnet_grad_ref as gref
import featnet_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SHAPES = json.load(open(os.path.join(GOLDEN, "featnet_state_dict.json")))


def small_batch(seed=0, n=700, span=16):
    rng = np.random.default_rng(seed)
    clouds = []
    for b in range(2):
        c = np.unique(rng.integers(-span, span, (n, 3)), axis=0)
        c = c[rng.permutation(len(c))] + (b * 5, 0, -3 * b)
        clouds.append(np.concatenate([np.full((len(c), 1), b), c], axis=1))
    return np.concatenate(clouds)


# ---- 1. the helper itself ------------------------------------------------------------------------------------------------

def test_helper_eval_forward_equals_the_forward_restatement():
    coords = small_batch()
    sd = ref.seeded_state_dict(3, SHAPES)
    want, want_inter = ref.network(coords, np.ones((len(coords), 1)), sd)
    tables = gref.Tables(coords)
    with torch.no_grad():
        got, inter = gref.network(tables, torch.ones(len(coords), 1, dtype=torch.float64), gref.state(sd, torch.float64), train=False)
    assert np.abs(got.numpy() - want).max() <= 1e-12
    for l in range(4):
        assert np.abs(inter["cat"][l].numpy() - want_inter["cat"][l]).max() <= 1e-12 * max(1.0, np.abs(want_inter["cat"][l]).max())
    assert np.abs(inter["s4"].numpy() - want_inter["s4"]).max() <= 1e-12 * max(1.0, np.abs(want_inter["s4"]).max())
    assert np.abs(inter["hidden"].numpy() - want_inter["hidden"]).max() <= 1e-12 * max(1.0, np.abs(want_inter["hidden"]).max())
    # the ReLU sites: the mask of a site is its value > 0, and forcing a run's own masks changes nothing
    vals = gref.site_values(inter)
    assert sorted(vals) == sorted(gref.RELU_SITES)
    for site in gref.RELU_SITES:
        assert torch.equal(vals[site] > 0, inter["mask"][site])
    with torch.no_grad():
        again, _ = gref.network(tables, torch.ones(len(coords), 1, dtype=torch.float64), gref.state(sd, torch.float64),
                                masks=inter["mask"])
    assert torch.equal(again, got)


def test_helper_train_mode_statistics_are_batch_norm1d_s():
    coords = small_batch(1)
    sd = gref.state(ref.seeded_state_dict(4, SHAPES), torch.float64)
    tables = gref.Tables(coords)
    feat = torch.ones(len(coords), 1, dtype=torch.float64)
    bn = torch.nn.BatchNorm1d(32, momentum=0.1).double()
    with torch.no_grad():
        for k in ("weight", "bias", "running_mean", "running_var"):
            getattr(bn, k).copy_(sd["norm1.bn." + k])
        x1 = gref.conv(feat, sd["conv1.kernel"], tables, 0)
        bn.train()(x1)
        out, _ = gref.network(tables, feat, sd, train=True)
    assert torch.isfinite(out).all()
    assert torch.allclose(sd["norm1.bn.running_mean"], bn.running_mean, rtol=1e-13, atol=0)
    assert torch.allclose(sd["norm1.bn.running_var"], bn.running_var, rtol=1e-13, atol=0)
    assert all(int(sd[n + ".bn.num_batches_tracked"]) == 1 for n in gref.NORMS) and int(bn.num_batches_tracked) == 1
    assert len(gref.NORMS) == 18


# ---- 2. the adjoint table ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", range(13))
def test_adjoint_table_inner_product_identity(t):
    """<conv_t(x; W), y> == <x, conv_t'(y; W')> with t' / W' of featnet_grad_ref.adjoint / repack (include/umereg_sparse_conv.h)"""
    coords = small_batch(2)
    tables = gref.Tables(coords)
    g = torch.Generator().manual_seed(t)
    cin, cout = 5, 3
    x = torch.randn(tables.sizes[gref.in_level(t)], cin, dtype=torch.float64, generator=g)
    y = torch.randn(tables.sizes[gref.out_level(t)], cout, dtype=torch.float64, generator=g)
    W = torch.randn(27, cin, cout, dtype=torch.float64, generator=g)
    ta, mirror = gref.adjoint(t)
    assert gref.out_level(ta) == gref.in_level(t) and gref.in_level(ta) == gref.out_level(t)
    lhs = (gref.conv(x, W, tables, t) * y).sum()
    rhs = (x * gref.conv(y, gref.repack(W, mirror), tables, ta)).sum()
    assert sum(len(o) for o, _ in tables.pairs[t]) > 0
    assert abs(float(lhs - rhs)) <= 1e-10 * max(abs(float(lhs)), 1.0), (float(lhs), float(rhs))
    # and autograd's input gradient of the helper is that adjoint convolution
    x.requires_grad_()
    (gref.conv(x, W, tables, t) * y).sum().backward()
    assert torch.allclose(x.grad, gref.conv(y, gref.repack(W, mirror), tables, ta), rtol=1e-12, atol=1e-12)


def test_table_levels_mirror_the_library_s():
    from umeregrobust_amd import sparse_conv
    for t in range(13):
        assert sparse_conv.out_level(t) == gref.out_level(t) and sparse_conv.in_level(t) == gref.in_level(t)
        assert sparse_conv.adjoint(t) == gref.adjoint(t)


# ---- 3. the C ABI's host side -----------------------------------------------------------------------------------------------

def test_sparse_conv_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts and disjointness: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import sparse_conv
    assert sorted(sparse_conv.SPARSE_CONV_SIGNATURES) == [
        "umereg_sparse_conv1_f32", "umereg_sparse_conv_f32", "umereg_sparse_conv_repack_f32", "umereg_sparse_conv_wgrad_f32",
        "umereg_sparse_conv_wgrad_scratch_bytes", "umereg_sparse_conv_wgrad_segments"]
    umereg_h = open(os.path.join(REPO, "include", "umereg.h")).read()
    assert "sparse_conv" not in umereg_h


def test_wgrad_sizes_are_host_arithmetic():
    from umeregrobust_amd import sparse_conv
    lib = sparse_conv.load_native()
    seg, size = lib.umereg_sparse_conv_wgrad_segments, lib.umereg_sparse_conv_wgrad_scratch_bytes
    for n in (1, 1000, 50000, 132308, 800000):
        for cin, cout in ((1, 32), (32, 32), (64, 128), (192, 64), (256, 256)):
            s = seg(n, cin, cout)
            assert 1 <= s <= 64 and size(n, cin, cout) == s * 27 * cin * cout * 4
    # sensible at the training shape: the largest layer's partial blocks stay under 64 MiB
    assert size(800000, 256, 256) <= 64 << 20
    assert seg(1024, 32, 32) == 1 and seg(1025, 32, 32) == 2
    for bad in ((0, 32, 32), (10, 48, 32), (10, 32, 16), (10, 32, 288), (10, 0, 32), (-5, 32, 32)):
        assert size(*bad) == 0 and seg(*bad) == 0


def test_sparse_conv_entry_points_check_arguments_and_need_a_device():
    from umeregrobust_amd import models, sparse_conv
    lib = sparse_conv.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    ws_bytes = lib.umereg_featnet_workspace_bytes(4, 1)
    sc_bytes = lib.umereg_sparse_conv_wgrad_scratch_bytes(4, 32, 32)
    conv = lambda **kw: lib.umereg_sparse_conv_f32(*[kw.get(k, d) for k, d in (          # noqa: E731
        ("ws", p), ("ws_bytes", ws_bytes), ("status", p), ("n", 4), ("table", 0), ("x", p), ("ld_in", 32), ("W", p), ("cin", 32), ("cout", 32),
        ("scale", p), ("shift", p), ("out", p), ("ld_out", 32), ("accumulate", 0), ("stream", None))])
    wgrad = lambda **kw: lib.umereg_sparse_conv_wgrad_f32(*[kw.get(k, d) for k, d in (   # noqa: E731
        ("ws", p), ("ws_bytes", ws_bytes), ("status", p), ("n", 4), ("table", 0), ("x", p), ("ld_in", 32), ("cin", 32), ("dy", p),
        ("ld_dy", 32), ("cout", 32), ("dW", p), ("scratch", p), ("scratch_bytes", sc_bytes), ("stream", None))])
    # argument errors come before the device probe
    for k in ("ws", "status", "x", "W", "scale", "shift", "out"):
        assert conv(**{k: None}) == -1, k
        assert b"null" in lib.umereg_last_error()
    for kw in (dict(n=0), dict(table=13), dict(table=-1), dict(cin=48), dict(cout=16), dict(cout=288), dict(ld_in=16), dict(ld_in=34),
               dict(ld_out=8), dict(x=p + 4)):
        assert conv(**kw) == -1, kw
    for k in ("ws", "status", "x", "dy", "dW", "scratch"):
        assert wgrad(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(table=13), dict(cin=48), dict(cin=0), dict(cout=16), dict(ld_in=16), dict(ld_dy=8)):
        assert wgrad(**kw) == -1, kw
    assert lib.umereg_sparse_conv1_f32(p, ws_bytes, p, 4, None, p, p, p, p, None) == -1
    assert lib.umereg_sparse_conv1_f32(None, ws_bytes, p, 4, p, p, p, p, p, None) == -1
    assert lib.umereg_sparse_conv1_f32(p, ws_bytes, p, 0, p, p, p, p, p, None) == -1
    assert lib.umereg_sparse_conv_repack_f32(None, 32, 32, 1, 0, 32, p, None) == -1
    assert lib.umereg_sparse_conv_repack_f32(p, 32, 32, 1, 0, 32, None, None) == -1
    assert lib.umereg_sparse_conv_repack_f32(p, 32, 32, 1, 0, 32, p, None) == -1            # in place
    assert lib.umereg_sparse_conv_repack_f32(p, 0, 32, 1, 0, 32, p + 65536, None) == -1
    assert lib.umereg_sparse_conv_repack_f32(p, 64, 96, 1, 0, 64, p + 65536, None) == -1    # 64 does not divide the 96 rows of W^T
    assert lib.umereg_sparse_conv_repack_f32(p, 64, 96, 0, 0, 0, p + 65536, None) == -1
    if lib.umereg_device_count(None, 0) == 0:
        assert conv() == -2                                                            # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        assert wgrad() == -2 and wgrad(cin=1, ld_in=1) == -2
        assert lib.umereg_sparse_conv1_f32(p, ws_bytes, p, 4, p, p, p, p, p, None) == -2
        assert lib.umereg_sparse_conv_repack_f32(p, 32, 32, 1, 1, 32, p + 65536, None) == -2


# ---- 4. the point-wise loss against the reference's own class ---------------------------------------------------------------

@pytest.mark.parametrize("kind", ["far", "near"])
def test_infonce_equals_the_reference_s(kind):
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    g = np.load(os.path.join(GOLDEN, "g13_infonce.npz"))
    fn = MyInfoNCELossNoSeg(tau=float(g["tau"]), neg_euclid_dist=float(g["neg_euclid_dist"]))
    src = torch.from_numpy(g[f"{kind}_src_feat"]).requires_grad_()
    tgt = torch.from_numpy(g[f"{kind}_tgt_feat"]).requires_grad_()
    pts, matches = torch.from_numpy(g[f"{kind}_src_pts"]), torch.from_numpy(g[f"{kind}_matches"])
    # the case is what its name says: the mask matters in `near` only
    a = pts[0][matches[0, :, 0]]
    close = int((torch.cdist(a, a) <= fn.neg_euclid_dist).sum()) - len(a)
    assert (close == 0) == (kind == "far") and src.dtype == torch.float32
    loss = fn(src, pts, tgt, matches)
    loss.backward()
    want = float(g[f"{kind}_loss"])
    print(f"[infonce {kind}] loss {float(loss.detach()):.7f} reference {want:.7f}; close anchor pairs {close // 2}")
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    for got, name in ((src.grad, "grad_src"), (tgt.grad, "grad_tgt")):
        w = g[f"{kind}_{name}"]
        assert np.abs(w).max() > 0
        assert np.abs(got.numpy() - w).max() <= 1e-5 * np.abs(w).max(), name


def test_infonce_signature_and_the_losses_out_of_scope():
    import inspect
    from umeregrobust_amd import loss
    sig = inspect.signature(loss.MyInfoNCELossNoSeg.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [("num_samples", 2048), ("tau", 0.1), ("match_r", 0.1),
                                                                            ("neg_euclid_dist", 5)]
    assert list(inspect.signature(loss.MyInfoNCELossNoSeg.forward).parameters)[1:] == ["velo_feat", "velo_pts", "ref_feat", "matches"]
    for cls in (loss.UMEContrastiveLoss, loss.CubeRegistrationLoss):
        with pytest.raises(NotImplementedError, match="out of scope"):
            cls()


# ---- 5. the trainable model without a GPU -------------------------------------------------------------------------------------

def test_trainable_model_refuses_cpu_tensors_in_both_modes():
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    m = ResUNetSmall2(trainable=True)
    assert m.trainable and not ResUNetSmall2().trainable
    assert list(m.state_dict()) == list(SHAPES)
    st = SparseTensor(torch.ones(2, 1), coordinates=torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train()(st)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(st)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(st)
    from umeregrobust_amd import sparse_conv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_conv.sparse_conv(torch.ones(2, 32), torch.ones(27, 32, 32), None, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_conv.CoordinateMaps(st.C, 1)
