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

def _featnet_header_symbols():
    text = open(os.path.join(REPO, "include", "umereg_featnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(umereg_[a-z0-9_]+)\s*\(", text)))


def test_featnet_table_mirrors_its_header():
    from umeregrobust_amd import models
    assert sorted(models.FEATNET_SIGNATURES) == _featnet_header_symbols()
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
