"""CPU: the feature network's fp64 restatement (tests/featnet_ref.py) pinned against torch's dense convolutions, the
state-dict contract of `umeregrobust_amd.models.ResUNetSmall2` against the reference's own constructor (fixture
tests/golden/featnet_state_dict.json, tools/gen_featnet_state.py), and the host side of include/umereg_featnet.h."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import featnet_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "featnet_state_dict.json")


# ---- the restatement against torch conv3d / conv_transpose3d ---------------------------------------------------------------

def _cloud(rng, n, lo, hi, batch=2, occupancy=None):
    """unique int coordinates (batch, x, y, z) in [lo, hi)^3; negative coordinates included."""
    rows = []
    for b in range(batch):
        c = rng.integers(lo, hi, (n, 3))
        c = np.unique(c, axis=0)
        c = c[rng.permutation(len(c))]
        rows.append(np.concatenate([np.full((len(c), 1), b), c], axis=1))
    return np.concatenate(rows).astype(np.int64)


def _dense(feat, coords, ts, origin, size, batch):
    """zero-filled dense grid [batch, C, X, Y, Z] in units of ts with the given origin."""
    g = torch.zeros(batch, feat.shape[1], size, size, size, dtype=torch.float64)
    i = (coords[:, 1:] - origin) // ts
    assert ((coords[:, 1:] - origin) % ts == 0).all() and (i >= 0).all() and (i < size).all()
    g[coords[:, 0], :, i[:, 0], i[:, 1], i[:, 2]] = torch.from_numpy(feat)
    return g


def _sample(g, coords, ts, origin):
    i = (coords[:, 1:] - origin) // ts
    assert ((coords[:, 1:] - origin) % ts == 0).all()
    return g[coords[:, 0], :, i[:, 0], i[:, 1], i[:, 2]].numpy()


def _grid(coords, ts, s):
    """origin (a multiple of 24, below every coordinate and its coarse cell) and size (in units of ts, a multiple of s) of a
    dense grid that holds the coordinates, their neighbours and their coarse cells"""
    origin = int(coords[:, 1:].min()) // 24 * 24 - 24
    size = (int(coords[:, 1:].max()) - origin) // ts + 2 * 24 // ts + 2 * s
    return origin, size + (-size) % s


def _torch_weight(W, transposed):
    """[27, C_in, C_out] -> conv3d [C_out, C_in, 3, 3, 3] / conv_transpose3d [C_in, C_out, 3, 3, 3], axes (x, y, z)."""
    w = torch.from_numpy(W).reshape(3, 3, 3, W.shape[1], W.shape[2])      # [dz, dy, dx, in, out]
    w = w.permute(3, 4, 2, 1, 0)                                          # [in, out, dx, dy, dz]
    return w if transposed else w.transpose(0, 1).contiguous()


# (tensor stride in, stride): every layer type of the network, the stride-3 one included
CONV_CASES = [(1, 1), (2, 1), (24, 1), (1, 2), (2, 2), (4, 2), (8, 3)]


@pytest.mark.parametrize("ts,s", CONV_CASES)
def test_restated_convolution_matches_torch_conv3d(ts, s):
    rng = np.random.default_rng(100 * ts + s)
    cin, cout, batch = 3, 4, 2
    fine = ref.coarsen(_cloud(rng, 300, -11 * ts, 9 * ts, batch), ts)            # partial occupancy at tensor stride ts
    fine = fine[np.unique(ref.keys(fine), return_index=True)[1]]
    out_coords = ref.strided_map(fine, ts * s) if s > 1 else fine
    feat = rng.standard_normal((len(fine), cin))
    W = rng.standard_normal((27, cin, cout))
    got = ref.conv(feat, fine, out_coords, W, ts)
    origin, size = _grid(fine, ts, s)
    dense = torch.nn.functional.conv3d(_dense(feat, fine, ts, origin, size, batch), _torch_weight(W, False), stride=s, padding=1)
    want = _sample(dense, out_coords, ts * s, origin)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("ts,s", [c for c in CONV_CASES if c[1] > 1])
def test_restated_transposed_convolution_matches_torch_conv_transpose3d(ts, s):
    rng = np.random.default_rng(7 * ts + s)
    cin, cout, batch = 4, 3, 2
    fine = ref.coarsen(_cloud(rng, 300, -11 * ts, 9 * ts, batch), ts)
    fine = fine[np.unique(ref.keys(fine), return_index=True)[1]]
    coarse = ref.strided_map(fine, ts * s)
    coarse = coarse[rng.random(len(coarse)) < 0.7]                               # partial coarse occupancy: missing sources
    feat = rng.standard_normal((len(coarse), cin))
    W = rng.standard_normal((27, cin, cout))
    got = ref.conv(feat, coarse, fine, W, ts, transposed=True)
    origin, size = _grid(fine, ts, s)
    size_c = size // s
    dense = torch.nn.functional.conv_transpose3d(_dense(feat, coarse, ts * s, origin, size_c, batch), _torch_weight(W, True),
                                                 stride=s, padding=1, output_padding=s - 1)
    want = _sample(dense, fine, ts, origin)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())


def test_restated_strided_map_floors_negative_coordinates():
    c = np.array([[0, -1, -2, -3], [0, 0, 1, 2], [1, -1, -2, -3], [0, -24, 23, -25]])
    assert ref.coarsen(c, 2).tolist() == [[0, -2, -2, -4], [0, 0, 0, 2], [1, -2, -2, -4], [0, -24, 22, -26]]
    assert ref.strided_map(c, 24).tolist() == [[0, -24, -24, -24], [0, -24, 0, -48], [0, 0, 0, 0], [1, -24, -24, -24]]


def test_restated_network_runs_on_partial_occupancy():
    """A small cloud through the whole restatement: unit rows, finite intermediates, levels nested."""
    rng = np.random.default_rng(3)
    c = _cloud(rng, 400, -40, 40, batch=2)
    sd = ref.seeded_state_dict(0, json.load(open(GOLDEN)))
    out, inter = ref.network(c, np.ones((len(c), 1)), sd)
    assert out.shape == (len(c), 32) and np.allclose(np.linalg.norm(out, axis=1), 1.0)
    sizes = [len(x) for x in inter["coords"]]
    assert sizes[0] == len(c) and all(a >= b for a, b in zip(sizes, sizes[1:]))
    assert [x.shape[1] for x in inter["cat"]] == [96, 128, 192, 256] and inter["s4"].shape == (sizes[4], 256)


def _dense_cube(lo, hi, batch=0):
    g = np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([np.full((len(g), 1), batch), g], axis=1).astype(np.int64)


def _mask_clouds():
    rng = np.random.default_rng(11)
    return {"sparse": _cloud(rng, 500, -60, 60, batch=2), "dense": _cloud(rng, 3000, -9, 9, batch=2),
            "cube": _dense_cube(-12, 12), "isolated": np.array([[0, 0, 0, 0], [0, 100, 0, 0], [1, 0, 0, 0]])}


@pytest.mark.parametrize("cloud", ["sparse", "dense", "cube", "isolated"])
def test_neighbour_masks_follow_the_rule_of_conv(cloud):
    """Bit k of a row's mask in every one of the 13 tables is set exactly when `conv` gathers a row at offset k: a one-hot
    kernel per offset (W[k] = e_k) over features of ones counts each offset's neighbour."""
    lv = ref.levels(_mask_clouds()[cloud])
    masks = ref.neighbour_masks(lv)
    assert len(masks) == 13 and all(m.dtype == np.uint32 for m in masks)
    W = np.zeros((27, 1, 27))
    W[np.arange(27), 0, np.arange(27)] = 1.0
    for t, (ql, tl, sign) in enumerate(ref.TABLES):
        assert len(masks[t]) == len(lv[ql])
        hit = ref.conv(np.ones((len(lv[tl]), 1)), lv[tl], lv[ql], W, ref.TSTRIDES[min(ql, tl)], transposed=sign < 0)
        assert set(np.unique(hit)) <= {0.0, 1.0}
        bits = (masks[t][:, None] >> np.arange(27, dtype=np.uint32)) & 1
        assert np.array_equal(bits, hit.astype(np.uint32)), f"table {t}"
    if cloud == "cube":         # every offset of an interior row of the self tables hits
        inner = (np.abs(lv[0][:, 1:] + 0.5) < 11).all(axis=1)
        assert inner.any() and (masks[0][inner] == (1 << 27) - 1).all()


def test_neighbour_masks_follow_the_header_order():
    """Tables in the order of UMEREG_FN_MASKS on two points one voxel apart: self l, strided l -> l+1 (5 + l, queried on the
    coarse map), transposed l+1 -> l (9 + l, queried on the fine map at -offset)."""
    m = ref.neighbour_masks(ref.levels(np.array([[0, 0, 0, 0], [0, 1, 0, 0]])))
    b = lambda *ks: sum(1 << k for k in ks)      # noqa: E731
    assert m[0].tolist() == [b(13, 14), b(12, 13)]          # k = 13 is the row itself; k = 14 is dx = +1
    assert m[1].tolist() == [b(13)] and m[4].tolist() == [b(13)]
    assert m[5].tolist() == [b(13, 14)]                     # level 1's (0, 0, 0) reads level 0 at (0, 0, 0) and (1, 0, 0)
    assert m[9].tolist() == [b(13), b(14)]                  # level 0's (1, 0, 0) reads level 1 at (1 - 1, 0, 0)
    assert [len(x) for x in m] == [2, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1]


def test_keys_and_lookup_stay_exact_at_batch_and_coordinate_limits():
    """Keys are the device's unsigned 64-bit fn_key: exact and ordered (batch, x, y, z) lexicographically up to batch 127 and
    the coordinate limits, where a signed key would wrap from batch 64 on; a lookup never confuses batch items that differ in
    the top bit of the batch index."""
    lim, bias = ref.COORD_LIM, 1 << 18
    vals = [-lim, -lim + 1, -1, 0, 1, lim - 2, lim - 1]
    xyz = np.array(np.meshgrid(vals, vals, vals, indexing="ij")).reshape(3, -1).T
    c = np.concatenate([np.concatenate([np.full((len(xyz), 1), b), xyz], 1) for b in (0, 1, 62, 63, 64, 65, 126, 127)])
    c = np.concatenate([c, [[127, bias - 1, bias - 1, bias - 1], [0, -bias, -bias, -bias]]]).astype(np.int64)
    k = ref.keys(c)
    assert k.dtype == np.uint64
    want = [(int(b) << 57) | ((int(x) + bias) << 38) | ((int(y) + bias) << 19) | (int(z) + bias) for b, x, y, z in c]
    assert [int(v) for v in k] == want
    assert int(k[c[:, 0] <= 126].max()) < (1 << 64) - 1     # never the empty slot's all-ones key up to batch 126 ...
    assert int(k[-2]) == (1 << 64) - 1                      # ... which is why the header stops there
    order = np.lexsort(c[:, ::-1].T)
    assert (np.diff(k[order].astype(object)) > 0).all()     # strictly increasing in lexicographic order
    idx = ref.Index(c[::-1])
    assert np.array_equal(idx.find(c), np.arange(len(c))[::-1])
    for have, other in ((63, 64), (62, 126), (64, 0), (126, 127), (1, 65)):
        part = ref.Index(c[c[:, 0] == have])
        q = c[c[:, 0] == have].copy()
        q[:, 0] = other
        assert (part.find(q) == -1).all(), (have, other)
    with pytest.raises(AssertionError):
        ref.keys([[128, 0, 0, 0]])
    with pytest.raises(AssertionError):
        ref.keys([[0, bias, 0, 0]])


def _sparse_h():
    return open(os.path.join(REPO, "umeregrobust_amd", "csrc", "sparse.h")).read()


def test_key_and_hash_mirror_match_sparse_h():
    """featnet_ref's mirror of fn_key / fn_hash / the table size (which the hash wraparound test aims with) is the header's:
    a change of key layout, bias, multiplier or capacity rule fails here instead of quietly making that test ordinary."""
    h = _sparse_h()
    body = lambda name: re.search(name + r"\(.*?\n\{(.*?)\n\}", h, re.S).group(1)       # noqa: E731
    assert int(re.search(r"kFnKeyBias = 1 << (\d+);", h).group(1)) == 18 and ref._BIAS == 1 << 18
    assert int(re.search(r"kFnCoordLim = 1 << (\d+);", h).group(1)) == 17 and ref.COORD_LIM == 1 << 17
    key = re.sub(r"\s+", " ", body("fn_key"))
    packed = re.search(r"key = (.*?);", key).group(1)
    terms = [t.strip() for t in packed.split("|")]
    assert terms == ["((unsigned long long)b << %d)" % ref.KEY_SHIFTS[0],
                     "((unsigned long long)(x + kFnKeyBias) << %d)" % ref.KEY_SHIFTS[1],
                     "((unsigned long long)(y + kFnKeyBias) << %d)" % ref.KEY_SHIFTS[2],
                     "(unsigned long long)(z + kFnKeyBias)"], terms
    assert "x < -kFnKeyBias || x >= kFnKeyBias" in key
    hb = re.sub(r"\s+", " ", body("fn_hash"))
    m = re.search(r"return \(unsigned int\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> (\d+)\) & \(cap - 1u\);", hb)
    assert m and int(m.group(1), 16) == ref.HASH_MUL and int(m.group(2)) == 32, hb
    ws = re.sub(r"\s+", " ", body("inline FnWs fn_ws"))
    assert "unsigned int cap = %du; while (cap < 2u * (unsigned int)n) cap <<= 1;" % ref.MIN_CAP in ws, ws
    assert [ref.table_cap(n) for n in (1, 512, 513, 50000, 132308)] == [1024, 1024, 2048, 131072, 524288]
    assert re.search(r"#define UMEREG_FEATNET_MAX_BATCH (\d+)", open(os.path.join(REPO, "include", "umereg_featnet.h")).read()).group(1) \
        == str(ref.MAX_BATCH)
    # the mirror's arithmetic: the top 32 bits of the 64-bit product, masked (exact integers)
    for k in (0, 1, 0x9E3779B97F4A7C15, int(ref.keys([[126, -5, 7, 131071]])[0])):
        want = ((k * ref.HASH_MUL) % (1 << 64)) >> 32 & (2048 - 1)
        assert int(ref.hash_slot(np.uint64(k), 2048)) == want


def test_restated_levels_and_cells():
    c = np.array([[0, -1, -1, -1], [0, -8, -8, -8], [0, 0, 0, 0], [0, 7, 7, 7], [3, 0, 0, 0], [0, -9, 0, 0]])
    lv = ref.levels(c)
    assert [len(x) for x in lv] == [6, 6, 6, 4, 4] and ref.cells(c) == 4
    assert np.array_equal(lv[0], c) and np.array_equal(lv[4][:, 1:] % 24, np.zeros((4, 3)))


# ---- state dict ----------------------------------------------------------------------------------------------------------

def test_state_dict_names_and_shapes_match_the_reference():
    from umeregrobust_amd.models import ResUNetSmall2
    want = json.load(open(GOLDEN))
    got = {k: list(v.shape) for k, v in ResUNetSmall2(in_channels=1, out_channels=32).state_dict().items()}
    assert list(got) == list(want)
    assert got == want


def test_checkpoint_round_trip(tmp_path):
    from umeregrobust_amd.datasets import checkpoint_state_dict
    from umeregrobust_amd.models import ResUNetSmall2
    sd = {k: torch.from_numpy(np.asarray(v)).to(torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
          for k, v in ref.seeded_state_dict(1, json.load(open(GOLDEN))).items()}
    path = tmp_path / "w.pth"
    torch.save({"epoch": 3, "model_state_dict": sd, "optimizer_state_dict": {}, "total_loss": 0.5}, path)
    m = ResUNetSmall2(in_channels=1, out_channels=32)
    m.load_state_dict(checkpoint_state_dict(str(path)))
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_unsupported_configurations_raise():
    from umeregrobust_amd.models import ResUNetSmall2
    with pytest.raises(ValueError):
        ResUNetSmall2(in_channels=3)
    with pytest.raises(ValueError):
        ResUNetSmall2(out_channels=16)


def test_forward_refuses_cpu_tensors_and_train_mode():
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    m = ResUNetSmall2()
    st = SparseTensor(torch.ones(2, 1), coordinates=torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="eval"):
        m.train()(st)
    with pytest.raises(RuntimeError, match="no backward"):
        m.eval()(st)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(st)


def test_sparse_tensor_decomposes_by_batch_index_in_row_order():
    from umeregrobust_amd.sparse import SparseTensor
    C = torch.tensor([[0, 5, 0, 0], [1, 1, 1, 1], [0, -3, 2, 2], [1, 0, 0, 0]], dtype=torch.int32)
    F = torch.arange(8.0).reshape(4, 2)
    st = SparseTensor(F, coordinates=C)
    assert st.batch_size == 2 and st.F is st.features and torch.equal(st.C, C)
    d = st.decomposed_features
    assert torch.equal(d[0], F[[0, 2]]) and torch.equal(d[1], F[[1, 3]])
    assert torch.equal(st.decomposed_coordinates[0], C[[0, 2], 1:])
    with pytest.raises(ValueError):
        SparseTensor(torch.ones(3, 1), coordinates=C)


# ---- the C ABI's host side ------------------------------------------------------------------------------------------------

def test_featnet_table_mirrors_its_header():
    """(keys, exports and parameter counts against the header: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import models
    lib = models.load_native()
    info = models.layer_info()
    assert [(k, ci, co) for k, ci, co, _, _ in info] == [
        (27, 1, 32), (27, 32, 32), (27, 32, 64), (27, 64, 64), (27, 64, 64), (27, 64, 64), (27, 64, 128), (27, 128, 128),
        (27, 128, 256), (27, 256, 256), (27, 256, 128), (27, 128, 128), (27, 256, 128), (27, 128, 128), (27, 192, 64),
        (27, 64, 64), (27, 128, 64), (27, 64, 64), (1, 96, 64), (1, 64, 32)]
    end = max(s + 2 * co for _, _, co, _, s in info)
    assert all(w % 4 == 0 and s % 4 == 0 and w + k * ci * co <= s for k, ci, co, w, s in info)
    assert end <= lib.umereg_featnet_params_count() < end + 4
    # sizes are host arithmetic, by n (and batch) only
    assert lib.umereg_featnet_workspace_bytes(50000, 1) == lib.umereg_featnet_workspace_bytes(50000, 2) > 50000 * 27 * 13 * 4
    assert lib.umereg_featnet_workspace_bytes(0, 1) == 0 and lib.umereg_featnet_workspace_bytes(10, 128) == 0


def test_featnet_entry_points_check_arguments_and_need_a_device():
    from umeregrobust_amd import models
    lib = models.load_native()
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    ws_bytes = lib.umereg_featnet_workspace_bytes(4, 1)
    # argument errors come before the device probe
    assert lib.umereg_featnet_forward_f32(None, p, 4, 1, p, p, p, p, ws_bytes, None) == -1
    assert lib.umereg_featnet_forward_f32(p, p, 0, 1, p, p, p, p, ws_bytes, None) == -1
    assert lib.umereg_featnet_forward_f32(p, p, 4, 0, p, p, p, p, ws_bytes, None) == -1
    assert lib.umereg_featnet_layer_info(20, p) == -1
    off, cols = ctypes.c_size_t(), ctypes.c_int32()
    assert lib.umereg_featnet_buffer(4, 1, models.BUF_S4, ctypes.addressof(off), ctypes.addressof(cols)) == 0 and cols.value == 256
    if lib.umereg_device_count(None, 0) == 0:
        assert lib.umereg_featnet_forward_f32(p, p, 4, 1, p, p, p, p, ws_bytes, None) == -2          # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
