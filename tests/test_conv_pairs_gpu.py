"""GPU: the pair-compacted convolution engine (include/umereg_sparse_conv_pairs.h, csrc/sparse_conv_pairs.hip; conv_mode="pairs")
against the union engine.  The contract is equality: every output element runs the union engine's chain minus its no-op links, so
every comparison here is `torch.equal` -- no tolerance -- in f32 and with f16 operands; on integer data both engines must also
EQUAL the fp64 restatement.

Where the compaction can go wrong is at the edges of its plan (tests/conv_pairs_ref.py): a list that is empty, that holds one row,
that ends one short of, on, or one past a block of 32 slots, that fills the tile.  `test_the_clouds_cover_the_plan_s_edges` computes,
from the reference's masks over the row order the library reports, the active count P of every (table, tile, offset) of the edge
clouds and asserts that P = 0, 1, 31, 32, 33, 63, 64, 65 and TM all occur: a coverage condition on the inputs, checked from the
reference side.  The clouds are seeded random subsets of a 16 x 16 x 8 slab at densities 0.02 ... 1.0 and a full 16^3 cube; the
seeds are fixed below, and the test prints where each P was met."""
import os

import numpy as np
import pytest
import torch

import conv_pairs_ref as cpr
import featnet_grad_ref as gref
import featnet_ref as ref
from test_featnet_gpu import edge_cloud, seeded, torch_state, voxel_cloud

pytestmark = pytest.mark.gpu

TM = cpr.TM
PRECISIONS = ["f32", "f16"]
# (table, C_in, C_out) of the seventeen 27-offset layers after conv1, in layer order
LAYER_OPS = [(0, 32, 32), (5, 32, 64), (1, 64, 64), (6, 64, 64), (2, 64, 64), (7, 64, 128), (3, 128, 128), (8, 128, 256), (4, 256, 256),
             (12, 256, 128), (3, 128, 128), (11, 256, 128), (2, 128, 128), (10, 192, 64), (1, 64, 64), (9, 128, 64), (0, 64, 64)]
# their input gradients: the same operator over the adjoint table, C_out -> C_in
ADJOINT_OPS = [(gref.adjoint(t)[0], cout, cin) for t, cin, cout in LAYER_OPS]
EDGE_P = (0, 1, 31, 32, 33, 63, 64, 65, TM)
# (density, seed) of the random subsets of the 16 x 16 x 8 slab, plus the full 16^3 cube ("cube")
SLAB_CLOUDS = [(0.02, 0), (0.05, 1), (0.1, 2), (0.2, 3), (0.35, 4), (0.5, 5), (0.75, 6), (1.0, 7)]

_cache = {}


def slab_cloud(density, seed):
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(-1, 3) - 5
    rng = np.random.default_rng(seed)
    c = g[rng.random(len(g)) < density] if density < 1.0 else g
    return np.concatenate([np.zeros((len(c), 1), np.int64), c[rng.permutation(len(c))]], axis=1)


def cube_cloud():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3) - 8
    return np.concatenate([np.zeros((len(g), 1), np.int64), g[np.random.default_rng(9).permutation(len(g))]], axis=1)


def kt6000():
    return voxel_cloud(0, "KT")[:6000]


CLOUDS = {"kt6000": kt6000, "cube": cube_cloud, "isolated": lambda: edge_cloud("isolated"), "one_cell": lambda: edge_cloud("one_cell"),
          "one_point": lambda: edge_cloud("one_point"), "batch2x3000": lambda: np.concatenate([voxel_cloud(3, "NS")[:3000],
                                                                                               voxel_cloud(4, "KT", batch=1)[:3000]])}
CLOUDS.update({f"slab{d}": (lambda d=d, s=s: slab_cloud(d, s)) for d, s in SLAB_CLOUDS})
CLOUDS.update({f"n{n}": (lambda n=n: voxel_cloud(0, "KT")[:n]) for n in (TM - 1, TM, TM + 1, 2 * TM - 1, 2 * TM, 2 * TM + 1)})
EDGE_CLOUDS = [f"slab{d}" for d, _ in SLAB_CLOUDS] + ["cube"]


def cloud(name):
    if ("cloud", name) not in _cache:
        _cache[("cloud", name)] = CLOUDS[name]()
    return _cache[("cloud", name)]


def gpu_maps(name, dev):
    """-> (CoordinateMaps, the reference's 13 masks over the library's own row order of every level)"""
    from umeregrobust_amd import sparse_conv as sc
    if ("maps", name) not in _cache:
        c = cloud(name)
        maps = sc.CoordinateMaps(torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev), int(c[:, 0].max()) + 1)
        levels = [maps.level_coords(l).cpu().numpy().astype(np.int64) for l in range(5)]
        assert np.array_equal(levels[0], c[maps.perm.cpu().numpy()])
        _cache[("maps", name)] = (maps, ref.neighbour_masks(levels))
    return _cache[("maps", name)]


def helper_tables(name, maps):
    """-> (featnet_grad_ref.Tables, per level the helper's row of every GPU row)"""
    if ("tables", name) not in _cache:
        tables = gref.Tables(cloud(name))
        rows = []
        for l in range(5):
            idx = ref.Index(tables.levels[l]).find(maps.level_coords(l).cpu().numpy().astype(np.int64))
            assert (idx >= 0).all() and len(np.unique(idx)) == tables.sizes[l] == len(idx)
            rows.append(torch.from_numpy(idx))
        _cache[("tables", name)] = (tables, rows)
    return _cache[("tables", name)]


# ---- the single operator through the C ABI ------------------------------------------------------------------------------------------

POISON = 7.25          # what `out` holds before a call: a finite value, so that a row left unwritten shows in every comparison


def conv_entry(maps, table, x, col_in, cin, W, scale, shift, out, col_out, accumulate, f16, pairs):
    """one call of umereg_sparse_conv_{f32, f16, pairs}: x [rows_in, ld_in] read from column col_in, out [rows, ld_out] written
    from column col_out"""
    from umeregrobust_amd import _lib, sparse_conv as sc
    lib = sc.load_native()
    cout = W.shape[-1]
    args = (maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, table, x.data_ptr() + 4 * col_in, x.stride(0),
            W.data_ptr(), cin, cout, scale.data_ptr(), shift.data_ptr(), out.data_ptr() + 4 * col_out, out.stride(0), int(accumulate),
            torch.cuda.current_stream(x.device).cuda_stream)
    if pairs:
        rc = lib.umereg_sparse_conv_pairs(*args, int(f16))
    else:
        rc = (lib.umereg_sparse_conv_f16 if f16 else lib.umereg_sparse_conv_f32)(*args)
    _lib.check(rc, "sparse_conv")


def draw(shape, integer, bound, g):
    if integer:
        return torch.randint(-bound, bound + 1, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g, dtype=torch.float32)


def run_case(maps, t, cin, cout, f16, pairs, integer, dev, variant="plain", seed=0):
    """-> the whole output buffer (guard rows and guard columns included) of one variant of the operator:
    plain: contiguous x and out;  slices: two calls over the two halves of C_in, the second accumulating;  offset: x and out are
    wider than their channel counts (ld_in > C_in, ld_out > C_out) and read / written from a column offset."""
    from umeregrobust_amd import sparse_conv as sc
    g = torch.Generator().manual_seed(1000 * t + cin + 7 * cout + seed)
    rows_in, rows_out = maps.sizes[sc.in_level(t)], maps.sizes[sc.out_level(t)]
    x = draw((rows_in, cin), integer, 8, g)
    W = draw((27, cin, cout), integer, 4, g)
    if integer:
        scale, shift = torch.ones(cout), torch.zeros(cout)
    else:
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    scale, shift = scale.to(dev), shift.to(dev)
    pad_in, pad_out = (32, 16) if variant == "offset" else (0, 0)
    xw = torch.full((rows_in, cin + 2 * pad_in), float("nan"))
    xw[:, pad_in:pad_in + cin] = x
    xw = xw.to(dev)
    out = torch.full((rows_out + 3, cout + 2 * pad_out), POISON, device=dev)      # three guard rows: rows past the level's end
    if variant == "slices":
        h = cin // 2
        Ws = [W[:, :h].contiguous().to(dev), W[:, h:].contiguous().to(dev)]
        conv_entry(maps, t, xw, 0, h, Ws[0], scale, shift, out, 0, False, f16, pairs)
        conv_entry(maps, t, xw, h, cin - h, Ws[1], scale, shift, out, 0, True, f16, pairs)
    else:
        conv_entry(maps, t, xw, pad_in, cin, W.to(dev), scale, shift, out, pad_out, False, f16, pairs)
    return out, x, W, (pad_out, rows_out)


def assert_engines_equal(maps, t, cin, cout, f16, integer, dev, variant, tag):
    a, x, W, (pad, rows) = run_case(maps, t, cin, cout, f16, False, integer, dev, variant)
    b = run_case(maps, t, cin, cout, f16, True, integer, dev, variant)[0]
    assert torch.equal(a, b), f"{tag} table {t} {cin}->{cout} f16={f16} {variant}: {int((a != b).sum())} of {a.numel()} elements differ"
    assert bool((b[rows:] == POISON).all()) and bool((b[:, :pad] == POISON).all()) and bool((b[:, pad + cout:] == POISON).all())
    assert bool(torch.isfinite(b).all())
    return b[:rows, pad:pad + cout], x, W


@pytest.mark.parametrize("precision", PRECISIONS)
def test_operator_equals_the_union_engine_on_every_layer_shape(gpu, precision):
    """N(0, 1) inputs and weights on the 6 000-point cloud: the seventeen layer shapes over their own tables and over their adjoint
    tables; `accumulate` over two channel slices; ld_in > C_in and ld_out > C_out with column offsets; rows past a level's end stay
    untouched (every level above 0 has fewer rows than the workspace was sized for)."""
    maps, _ = gpu_maps("kt6000", gpu)
    f16 = precision == "f16"
    for t, cin, cout in LAYER_OPS + ADJOINT_OPS:
        assert_engines_equal(maps, t, cin, cout, f16, False, gpu, "plain", "kt6000")
    for t, cin, cout in LAYER_OPS[::3] + ADJOINT_OPS[1::3]:
        if cin >= 64:
            assert_engines_equal(maps, t, cin, cout, f16, False, gpu, "slices", "kt6000")
        assert_engines_equal(maps, t, cin, cout, f16, False, gpu, "offset", "kt6000")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_operator_is_exact_on_small_integers(gpu, precision):
    """Inputs in [-8, 8], weights in [-4, 4], integer valued: every operand is an f16 number and every partial sum an integer below
    27 x 256 x 32 < 2^24, so both engines must EQUAL the fp64 restatement, in both precisions."""
    maps, _ = gpu_maps("kt6000", gpu)
    tables, rows = helper_tables("kt6000", maps)
    f16 = precision == "f16"
    for ops, variants in ((LAYER_OPS + ADJOINT_OPS, ("plain",)), (LAYER_OPS[::3] + ADJOINT_OPS[1::3], ("slices", "offset"))):
        for t, cin, cout in ops:
            for variant in variants:
                if variant == "slices" and cin < 64:
                    continue
                got, x, W = assert_engines_equal(maps, t, cin, cout, f16, True, gpu, variant, "kt6000 integers")
                li, lo = gref.in_level(t), gref.out_level(t)
                x64 = torch.empty(x.shape, dtype=torch.float64).index_copy_(0, rows[li], x.double())       # GPU row order -> helper's
                want = gref.conv(x64, W.double(), tables, t)[rows[lo]]
                assert torch.equal(got.cpu().double(), want), f"table {t} {cin}->{cout} {variant}: differs from the fp64 restatement"


# ---- the edges of the compaction plan -----------------------------------------------------------------------------------------------

def test_the_clouds_cover_the_plan_s_edges(gpu):
    seen = {}
    for name in EDGE_CLOUDS:
        maps, masks = gpu_maps(name, gpu)
        for t, m in enumerate(masks):
            for p in np.unique(cpr.active_counts(m)):
                seen.setdefault(int(p), (name, t))
    print("[conv pairs edges] " + " ".join(f"P={p}: {seen.get(p)}" for p in EDGE_P))
    assert all(p in seen for p in EDGE_P), [p for p in EDGE_P if p not in seen]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", EDGE_CLOUDS + ["isolated", "one_cell", "one_point", "n%d" % (TM + 1)])
def test_operator_equals_the_union_engine_at_the_plan_s_edges(gpu, name, precision):
    """every table of the edge clouds, a narrow (32: TN = 32) and a wide (64) layer; plus isolated points (only offset 13), one
    stride-24 cell, one point, and a level 0 whose second tile holds one row"""
    maps, masks = gpu_maps(name, gpu)
    if name == "isolated":
        assert all((m == np.uint32(1 << 13)).all() for m in masks[:5]) and all((cpr.bits(m).sum(1) <= 1).all() for m in masks)
    if name == "one_cell":
        assert maps.sizes[4] == 1
    if name == "n%d" % (TM + 1):
        assert maps.sizes[0] == TM + 1
    for t in range(13):
        for c in (32, 64):
            assert_engines_equal(maps, t, c, c, precision == "f16", False, gpu, "plain", name)
            assert_engines_equal(maps, t, c, c, precision == "f16", True, gpu, "plain", name)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_with_an_empty_mask_get_their_epilogue(gpu, precision):
    """Table 12 (level 3 <- level 4, stride 3): some rows have no neighbour at all.  Their element is `shift`, and with `accumulate`
    (the ABI's residual) shift + what was there -- in both engines, bit for bit.  (The ReLU is not reachable through the single
    operator; the fused forward applies it to table 12's consumer, and `test_network_*` compares that.)"""
    maps, masks = gpu_maps("kt6000", gpu)
    empty = torch.from_numpy(masks[12] == 0)
    assert 0 < int(empty.sum()) < len(empty), "the cloud must have rows with and without neighbours in table 12"
    f16 = precision == "f16"
    from umeregrobust_amd import sparse_conv as sc
    g = torch.Generator().manual_seed(12)
    x = torch.randn(maps.sizes[sc.in_level(12)], 256, generator=g).to(gpu)
    W = torch.randn(27, 256, 128, generator=g).to(gpu)
    scale, shift = (torch.rand(128, generator=g) + 0.5).to(gpu), torch.randn(128, generator=g).to(gpu)
    prev = torch.randn(maps.sizes[3], 128, generator=g).to(gpu)
    outs = {}
    for pairs in (False, True):
        for accumulate in (False, True):
            out = prev.clone()
            conv_entry(maps, 12, x, 0, 256, W, scale, shift, out, 0, accumulate, f16, pairs)
            outs[(pairs, accumulate)] = out
    for accumulate in (False, True):
        assert torch.equal(outs[(True, accumulate)], outs[(False, accumulate)])
    e = empty.to(gpu)
    assert torch.equal(outs[(True, False)][e], shift.expand(int(empty.sum()), -1))
    assert torch.equal(outs[(True, True)][e], (shift + prev)[e])
    assert not torch.equal(outs[(True, False)][~e], shift.expand(int((~empty).sum()), -1))


# ---- the network --------------------------------------------------------------------------------------------------------------------

def eval_model(dev, precision, conv_mode, seed=42):
    from umeregrobust_amd.models import ResUNetSmall2
    key = ("model", precision, conv_mode, seed)
    if key not in _cache:
        m = ResUNetSmall2(in_channels=1, out_channels=32, precision=precision, conv_mode=conv_mode)
        m.load_state_dict(torch_state(seeded(seed)))
        _cache[key] = m.eval().to(dev)
    return _cache[key]


def run(m, coords, dev, debug=False):
    from umeregrobust_amd.sparse import SparseTensor
    C = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(dev)
    with torch.no_grad():
        return m(SparseTensor(torch.ones(len(C), 1, device=dev), coordinates=C), debug=debug)


def assert_same_forward(a, b, tag):
    (ra, ia), (rb, ib) = a, b
    assert torch.equal(ra.F, rb.F), f"{tag}: outputs differ"
    assert ia["levels"] == ib["levels"] and torch.equal(ia["perm"], ib["perm"])
    for k in ("hidden", "s4"):
        assert torch.equal(ia[k], ib[k]), f"{tag}: {k} differs"
    for l in range(4):
        assert torch.equal(ia["cat"][l], ib["cat"][l]), f"{tag}: cat{l} differs"
    for l in range(5):
        assert torch.equal(ia["coords"][l], ib["coords"][l])


NET_CLOUDS = ["one_point", "isolated", "kt6000", "batch2x3000"] + [f"n{n}" for n in (TM - 1, TM, TM + 1, 2 * TM - 1, 2 * TM, 2 * TM + 1)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NET_CLOUDS)
def test_network_equals_the_union_engine(gpu, name, precision):
    """eval mode, the fused call: the output and every debug intermediate (cat0..3, s4, hidden, levels)"""
    c = cloud(name)
    want = run(eval_model(gpu, precision, "union"), c, gpu, debug=True)
    got = run(eval_model(gpu, precision, "pairs"), c, gpu, debug=True)
    assert_same_forward(got, want, f"{name} {precision}")
    assert bool(torch.isfinite(got[0].F).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_network_is_deterministic_batch_equals_clouds_and_rows_permute(gpu, precision):
    m = eval_model(gpu, precision, "pairs")
    both = cloud("batch2x3000")
    a, b = run(m, both, gpu).F, run(m, both, gpu).F
    assert a.view(torch.int32).equal(b.view(torch.int32))
    parts = run(m, both, gpu).decomposed_features
    for i in range(2):
        one = both[both[:, 0] == i].copy()
        one[:, 0] = 0
        assert run(m, one, gpu).F.view(torch.int32).equal(parts[i].contiguous().view(torch.int32)), f"cloud {i}"
    p = np.random.default_rng(1).permutation(len(both))
    assert run(m, both[p], gpu).F.view(torch.int32).equal(a[torch.from_numpy(p).to(gpu)].view(torch.int32))


@pytest.mark.parametrize("train_precision,fused_norm", [("f32", False), ("f32", True), ("f16", False), ("f16", True)])
def test_training_step_equals_the_union_engine(gpu, train_precision, fused_norm):
    """train mode, one forward and one backward of the layer-wise path: loss, running statistics and every parameter gradient"""
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    c = cloud("batch2x3000")
    C = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(gpu)
    G = torch.randn(len(c), 32, generator=torch.Generator().manual_seed(3)).to(gpu)
    res = {}
    for mode in ("union", "pairs"):
        m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, train_precision=train_precision, fused_norm=fused_norm,
                          conv_mode=mode)
        m.load_state_dict(torch_state(seeded(5)))
        m = m.to(gpu).train()
        st = SparseTensor(torch.ones(len(C), 1, device=gpu), coordinates=C)
        loss = (m(st).F * G).sum()
        loss.backward()
        res[mode] = (loss.detach(), {k: v.clone() for k, v in m.named_buffers()}, {k: p.grad.clone() for k, p in m.named_parameters()})
    (la, ba, ga), (lb, bb, gb) = res["union"], res["pairs"]
    assert torch.equal(la, lb) and bool(torch.isfinite(la))
    assert ba.keys() == bb.keys() and ga.keys() == gb.keys() and len(ga) > 40
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
        assert bool(torch.isfinite(ga[k]).all()), k
    assert all(float(ga[k].abs().max()) > 0 for k in ga if k.endswith(".kernel")), "a kernel received no gradient"


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


@pytest.mark.parametrize("f16", [0, 1])
def test_guard_bands_and_run_twice(gpu, f16):
    """Both entries of include/umereg_sparse_conv_pairs.h with every device buffer between 4 KiB canaries at exactly the size the
    headers state, the workspace pre-filled with garbage and the outputs with poison: two runs with other garbage agree byte for
    byte with each other and with the union engine's entries, `status` included."""
    from umeregrobust_amd import models, sparse_conv as sc
    lib = sc.load_native()
    coords = cloud("batch2x3000")[::3].copy()
    n, batch = len(coords), 2
    params = eval_model(gpu, "f32", "union").packed_parameters()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    g = torch.Generator().manual_seed(4)
    W = torch.randn(27, 64, 96, generator=g).numpy()
    sc_sh = torch.randn(2, 96, generator=g).numpy()
    results = []
    for pairs, poison, garbage in ((True, 0xCD, 0xEE), (True, 0x3C, 0x17), (False, 0x3C, 0x17)):
        bufs = []

        def alloc(nbytes, fill):
            full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=gpu)
            full[:PAD] = CANARY
            full[PAD + nbytes:] = CANARY
            full[PAD:PAD + nbytes] = fill
            bufs.append((full, nbytes))
            return full

        def inp(a):
            a = np.ascontiguousarray(a)
            full = alloc(a.nbytes, 0)
            full[PAD:PAD + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(gpu))
            return full.data_ptr() + PAD

        def intact():
            torch.cuda.synchronize()
            for full, nb in bufs:
                assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"

        c_p, f_p, p_p = inp(coords.astype(np.int32)), inp(np.ones((n, 1), np.float32)), inp(params.cpu().numpy())
        out = alloc(n * 32 * 4, poison)
        status = alloc(8 * 4, poison)
        ws_bytes = lib.umereg_featnet_workspace_bytes(n, batch)
        ws = alloc(ws_bytes, garbage)
        fwd_args = (c_p, f_p, n, batch, p_p, out.data_ptr() + PAD, status.data_ptr() + PAD, ws.data_ptr() + PAD, ws_bytes, stream)
        if pairs:
            rc = lib.umereg_featnet_forward_pairs(*fwd_args, f16)
        else:
            rc = (lib.umereg_featnet_forward_f16 if f16 else lib.umereg_featnet_forward_f32)(*fwd_args)
        assert rc == 0, lib.umereg_last_error()
        intact()
        st = status[PAD:PAD + 32].view(torch.int32).cpu()
        assert int(st[0]) == 0 and int(st[1]) == n
        # the single convolution over the maps that forward left in the workspace: table 6 (level 1 -> 2), 64 -> 96 channels
        rows_in, rows_out = int(st[2]), int(st[3])
        x_p = inp(torch.randn(rows_in, 64, generator=torch.Generator().manual_seed(6)).numpy())
        w_p, s_p, h_p = inp(W), inp(sc_sh[0]), inp(sc_sh[1])
        y = alloc(rows_out * 96 * 4, poison)
        conv_args = (ws.data_ptr() + PAD, ws_bytes, status.data_ptr() + PAD, n, 6, x_p, 64, w_p, 64, 96, s_p, h_p, y.data_ptr() + PAD, 96, 0,
                     stream)
        if pairs:
            rc = lib.umereg_sparse_conv_pairs(*conv_args, f16)
        else:
            rc = (lib.umereg_sparse_conv_f16 if f16 else lib.umereg_sparse_conv_f32)(*conv_args)
        assert rc == 0, lib.umereg_last_error()
        intact()
        results.append((out[PAD:PAD + n * 32 * 4].clone(), st, y[PAD:PAD + rows_out * 96 * 4].clone()))
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert torch.equal(a, b)
    assert models.workspace_bytes(n, batch) == ws_bytes


def test_f16_range_flag_and_errors(gpu):
    """an activation beyond +-65504 raises ValueError in f16 on the pairs engine too, with the union engine's status bit; duplicate
    coordinates raise as ever; and the model works afterwards"""
    from umeregrobust_amd import models
    from umeregrobust_amd.sparse import SparseTensor
    c = cloud("one_cell")
    C = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(gpu)
    big = SparseTensor(torch.full((len(C), 1), 1e6, device=gpu), coordinates=C)
    m16, m32 = eval_model(gpu, "f16", "pairs"), eval_model(gpu, "f32", "pairs")
    with torch.no_grad():
        with pytest.raises(ValueError, match="precision='f16'.*f16 range"):
            m16(big)
        assert torch.equal(m32(big).F, eval_model(gpu, "f32", "union")(big).F)
    ws = torch.empty(models.workspace_bytes(len(C), 1), dtype=torch.uint8, device=gpu)
    o = torch.empty(len(C), 32, device=gpu)
    status = {mode: torch.empty(models.N_STATUS, dtype=torch.int32, device=gpu) for mode in models.CONV_MODES}
    for mode in models.CONV_MODES:
        models.forward_raw(C, torch.full((len(C), 1), 1e6, device=gpu), 1, m16.packed_parameters(), ws, o, status[mode], precision="f16",
                           conv_mode=mode)
    assert int(status["pairs"][0]) == models.ERR_F16_RANGE and torch.equal(status["pairs"], status["union"])
    with pytest.raises(ValueError, match="duplicate"):
        run(m32, np.concatenate([c, c[5:6]]), gpu)
    assert_same_forward(run(m16, c, gpu, debug=True), run(eval_model(gpu, "f16", "union"), c, gpu, debug=True), "one_cell f16")


def test_entry_points_return_the_union_engine_s_error_codes(gpu):
    from umeregrobust_amd import sparse_conv as sc
    lib = sc.load_native()
    maps, _ = gpu_maps("one_cell", gpu)
    x = torch.zeros(maps.n, 64, device=gpu)
    W = torch.zeros(27, 64, 64, device=gpu)
    out = torch.zeros(maps.n, 64, device=gpu)
    names = (("ws", maps.ws.data_ptr()), ("ws_bytes", maps.ws.numel()), ("status", maps.status.data_ptr()), ("n", maps.n), ("table", 0),
             ("x", x.data_ptr()), ("ld_in", 64), ("W", W.data_ptr()), ("cin", 64), ("cout", 64), ("scale", maps.ones.data_ptr()),
             ("shift", maps.zeros.data_ptr()), ("out", out.data_ptr()), ("ld_out", 64), ("accumulate", 0), ("stream", None))
    for f16 in (0, 1):
        for kw in (dict(ws=None), dict(x=None), dict(W=None), dict(out=None), dict(status=None), dict(cin=48), dict(cout=16), dict(cout=288),
                   dict(table=13), dict(table=-2), dict(n=0), dict(ld_in=32), dict(ws_bytes=maps.ws.numel() - 256 * 1024)):
            args = [kw.get(k, d) for k, d in names]
            union = (lib.umereg_sparse_conv_f16 if f16 else lib.umereg_sparse_conv_f32)(*args)
            assert union < 0 and lib.umereg_sparse_conv_pairs(*args, f16) == union, (f16, kw)
    coords = torch.zeros(4, 4, dtype=torch.int32, device=gpu)
    p = x.data_ptr()
    for f16 in (0, 1):
        assert lib.umereg_featnet_forward_pairs(None, p, 4, 1, p, p, p, maps.ws.data_ptr(), maps.ws.numel(), None, f16) == -1
        assert lib.umereg_featnet_forward_pairs(coords.data_ptr(), p, 4, 1, p, p, p, maps.ws.data_ptr(), 1024, None, f16) == \
            lib.umereg_featnet_forward_f32(coords.data_ptr(), p, 4, 1, p, p, p, maps.ws.data_ptr(), 1024, None) < 0
    torch.cuda.synchronize()


# ---- the evaluation loop ------------------------------------------------------------------------------------------------------------

def test_cached_pairs_with_checkpoint_gives_the_union_engine_s_features(gpu, tmp_path):
    import argparse
    from umeregrobust_amd import evaluate
    from umeregrobust_amd.datasets import write_cached_pair
    from umeregrobust_amd.synth import synth_pair_cfg
    from umeregrobust_amd.utils.general_utils import benchmark_config_path, update_namespace_from_yaml
    ck = tmp_path / "w.pth"
    torch.save({"epoch": 1, "model_state_dict": torch_state(seeded(7)), "optimizer_state_dict": {}, "total_loss": 0.0}, ck)
    p = synth_pair_cfg(20, "NS", "test", n_src=3000, n_tgt=2500)
    item = []
    for pts in (p.src_pts, p.tgt_pts):
        c = np.round(pts / 0.3).astype(np.int32)
        keep = np.sort(np.unique(c, axis=0, return_index=True)[1])
        item.append((pts[keep], np.zeros(len(keep), np.int64), c[keep]))
    (sp, ss, sc_), (tp, ts_, tc) = item
    T = p.gt_tform.astype(np.float32)
    moved = (sp @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    matches = np.stack([np.arange(min(len(sp), len(tp)))] * 2, 1).astype(np.int64)
    fields = (torch.from_numpy(sp), torch.from_numpy(ss), torch.from_numpy(sc_), torch.from_numpy(tp), torch.from_numpy(ts_),
              torch.from_numpy(tc), torch.from_numpy(moved), torch.from_numpy(T), matches)
    write_cached_pair(str(tmp_path / "cache" / os.path.join("test", "08", "000000_000001.pickle")), fields)
    args = update_namespace_from_yaml(argparse.Namespace(benchmark="kitti_test"), benchmark_config_path("kitti_test"))
    args.max_pc_size = 100000
    args.split = "test"
    for precision in PRECISIONS:
        feats = {}
        for mode in ("union", "pairs"):
            pair = next(evaluate.cached_pairs(str(tmp_path / "cache"), None, "test", range(1), args, gpu, rng=np.random.RandomState(0),
                                              checkpoint=str(ck), feature_precision=precision, conv_mode=mode))
            feats[mode] = (pair["src_feat"], pair["tgt_feat"])
        for a, b in zip(feats["union"], feats["pairs"]):
            assert torch.equal(a, b) and a.shape[-1] == 32 and bool(torch.isfinite(a).all())
