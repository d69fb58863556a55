"""CPU: the host side of the raw-scan path -- the readers against the bytes of tests/golden/g17_raw_scan.npz, the label map from a
yaml, both dataset classes' pair lists against the reference's constructors, the cache-writing command's argument handling, and the
host side of include/umereg_scan_prep.h (exports, the signature table, the size query, argument checks before the device probe)."""
import os
import re

import numpy as np
import pytest
import torch

import raw_scan_ref as rref
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "umereg_scan_prep.h")


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_raw_scan.npz")


@pytest.fixture(scope="module")
def tree(g17, tmp_path_factory):
    return rref.write_g17_tree(g17, tmp_path_factory.mktemp("g17"))


def test_readers_return_the_files_bytes(g17, tree):
    from umeregrobust_amd import raw_scan
    lut = raw_scan.load_learning_map(tree["label_config"])
    for f in (0, 1):
        scan = raw_scan.read_kitti_scan(os.path.join(tree["kitti"], "00", "velodyne", f"{f:06d}.bin"))
        words = raw_scan.read_kitti_label(os.path.join(tree["kitti"], "00", "labels", f"{f:06d}.label"), len(scan))
        assert scan.dtype == np.float32 and scan.shape[1] == 4 and np.array_equal(scan, g17[f"kitti_scan{f}"])
        assert words.dtype == np.uint32 and np.array_equal(words, g17[f"kitti_label{f}"]) and (words >> 16).min() > 0
        nscan, nlab = raw_scan.read_nuscenes_cloud(tree["nuscenes"], "test", rref.NUSC_SEQ, f)
        assert np.array_equal(nscan, g17[f"nuscenes_scan{f}"]) and np.array_equal(nlab, g17[f"nuscenes_label{f}"])
    # the reference's loader on frame 0: the points are the first three columns, the labels the mapped low halves
    scan, words = g17["kitti_scan0"], g17["kitti_label0"]
    assert np.array_equal(scan[:, :3], g17["kitti_load_pts"])
    assert np.array_equal(lut[words & 0xFFFF].astype(np.int64), g17["kitti_load_seg"])
    pts, seg, _, err = rref.scan_prep(scan, words, lut, sem16=True, keep_unlabeled=True)
    assert err == 0 and np.array_equal(pts, g17["kitti_load_pts"]) and np.array_equal(seg, g17["kitti_load_seg"])


def test_nuscenes_reader_takes_npy_clouds_and_missing_labels(g17, tmp_path):
    from umeregrobust_amd import raw_scan
    scan = g17["nuscenes_scan0"]
    rref.write_nuscenes_frame(tmp_path, "val", "s", 7, scan[:, :3].astype(np.float64), None, velo_data_type="npy")
    got, labels = raw_scan.read_nuscenes_cloud(str(tmp_path), "val", "s", 7, velo_data_type="npy")
    assert labels is None and got.dtype == np.float32 and np.array_equal(got, scan[:, :3])
    with pytest.raises(NotImplementedError):
        raw_scan.read_nuscenes_cloud(str(tmp_path), "val", "s", 7, velo_data_type="pcd")
    rref.write_nuscenes_frame(tmp_path, "val", "s", 8, scan, g17["nuscenes_label0"][:-1])
    with pytest.raises(ValueError, match="same number of points"):
        raw_scan.read_nuscenes_cloud(str(tmp_path), "val", "s", 8)


def test_readers_refuse_wrong_extensions_and_lengths(g17, tmp_path):
    from umeregrobust_amd import raw_scan
    scan, words = g17["kitti_scan0"], g17["kitti_label0"]
    for name, a in (("a.bin", scan), ("a.npy", scan), ("a.label", words), ("b.label", words[:-3]), ("a.txt", words)):
        a.tofile(str(tmp_path / name))
    with pytest.raises(RuntimeError, match="not valid scan file"):
        raw_scan.read_kitti_scan(str(tmp_path / "a.npy"))
    with pytest.raises(RuntimeError, match="not valid label file"):
        raw_scan.read_kitti_label(str(tmp_path / "a.txt"))
    with pytest.raises(TypeError):
        raw_scan.read_kitti_scan(tmp_path / "a.bin")
    with pytest.raises(ValueError, match="same number of points"):
        raw_scan.read_kitti_label(str(tmp_path / "b.label"), len(scan))
    assert len(raw_scan.read_kitti_label(str(tmp_path / "b.label"))) == len(words) - 3
    assert len(raw_scan.read_kitti_label(str(tmp_path / "a.label"), len(scan))) == len(scan)


def test_learning_map_from_a_yaml(g17, tree, tmp_path):
    from umeregrobust_amd import raw_scan
    keys, values = g17["lm_keys"], g17["lm_values"]
    lut = raw_scan.load_learning_map(tree["label_config"])
    assert lut.dtype == np.int32 and len(lut) == keys.max() + 1 and np.array_equal(lut[keys], values)
    rest = np.setdiff1d(np.arange(len(lut)), keys)
    assert len(rest) and (lut[rest] == -1).all()
    assert (values[np.isin(keys, [0, 1, 52, 99])] == 0).all() and len(np.unique(values)) == 20
    (tmp_path / "no_map.yaml").write_text("labels:\n  0: unlabeled\n")
    with pytest.raises(KeyError, match="learning_map"):
        raw_scan.load_learning_map(str(tmp_path / "no_map.yaml"))
    with pytest.raises(ValueError):
        raw_scan.learning_map_lut([1, -2], [0, 1])


@pytest.mark.parametrize("kind", ["kitti", "nuscenes"])
def test_pair_lists_equal_the_references(g17, tree, kind):
    from umeregrobust_amd.datasets import CachedPairDataset, NuscenesDataset, SemanticKITTIDataset
    cls = SemanticKITTIDataset if kind == "kitti" else NuscenesDataset
    n_variants = len(g17["variant_size"])
    assert n_variants == 5
    for i in range(n_variants):
        kw = dict(cache_data_path=str(g17["variant_cache"][i]), skip_invalid_entries=bool(g17["variant_skip"][i]),
                  overied_cache=bool(g17["variant_overied"][i]), dataset_size=int(g17["variant_size"][i]))
        ds = cls("unused", "test", metadata_dir=tree[kind + "_meta"], **kw)
        want = g17[f"{kind}_v{i}_files"]
        assert isinstance(ds, CachedPairDataset) and len(ds) == len(want) and ds.cache_data_path == str(g17[f"{kind}_v{i}_cache"])
        assert np.array_equal(ds.gt_tforms, g17[f"{kind}_v{i}_tforms"]) and ds.gt_tforms.dtype == np.float32
        if kind == "kitti":
            assert all(type(v) is int for e in ds.files for v in e) and np.array_equal(np.array(ds.files).reshape(-1, 3), want)
        else:
            assert all(type(e[0]) is str and type(e[1]) is int and type(e[2]) is int for e in ds.files)
            assert [(s, str(a), str(b)) for s, a, b in ds.files] == [tuple(r) for r in want.tolist()]
    if kind == "kitti":
        at_50 = np.flatnonzero(np.linalg.norm(g17["kitti_tforms"][:, :3, 3], axis=-1) == 50)
        above = np.flatnonzero(np.linalg.norm(g17["kitti_tforms"][:, :3, 3], axis=-1) > 50)
        ds = cls("unused", "test", metadata_dir=tree["kitti_meta"])
        assert len(at_50) and len(above) and len(ds) == len(g17["kitti_meta"]) - len(above)
        assert all(g17["kitti_meta"][r].tolist() in ds.files for r in at_50), "the row with |t| exactly 50 is kept"
        assert not any(g17["kitti_meta"][r].tolist() in ds.files for r in above)
        assert len(cls("unused", "test", cache_data_path="/c", metadata_dir=tree["kitti_meta"])) == len(ds) - 1     # IN_VALID_IDXS['test'] = [9]
    # constructor arguments in the reference's order, then the keyword-only additions
    import inspect
    params = list(inspect.signature(cls.__init__).parameters.values())[1:]
    assert [p.name for p in params[:10]] == ["data_path", "split", "voxel_size", "use_pc_completion", "cache_data_path", "dataset_size",
                                             "use_augmentations", "convert_points_to_grid", "skip_invalid_entries", "overied_cache"]
    assert [p.default for p in params[2:10]] == [0.3, False, "", -1, False, True, True, False]
    assert all(p.kind is p.KEYWORD_ONLY for p in params[10:])
    assert {"metadata_dir", "label_config", "device", "completion_fn"} <= {p.name for p in params[10:]}
    with pytest.raises(ValueError, match="metadata_dir"):
        cls("unused", "test")


def test_cached_items_come_from_the_shared_cache_code(g17, tree, tmp_path):
    """with a cache path an item is what CachedPairDataset serves, file layout of both datasets included"""
    from umeregrobust_amd.datasets import CachedPairDataset, NuscenesDataset, SemanticKITTIDataset, write_cached_pair
    item = tuple(torch.from_numpy(g17["kitti_grid_" + k]) for k in rref.NAMES)
    for cls, kind, seq_dir in ((SemanticKITTIDataset, "kitti", "00"), (NuscenesDataset, "nuscenes", rref.NUSC_SEQ)):
        write_cached_pair(str(tmp_path / kind / "test" / seq_dir / "000000_000001.pickle"), item)
        ds = cls("unused", "test", cache_data_path=str(tmp_path / kind), metadata_dir=tree[kind + "_meta"])
        assert cls.__getitem__ is not CachedPairDataset.__getitem__ and ds.path(0).endswith(os.path.join(seq_dir, "000000_000001.pickle"))
        assert all(torch.equal(a, b) for a, b in zip(ds[0], item))


def test_completion_needs_a_hook(tree):
    from umeregrobust_amd.datasets import NuscenesDataset, SemanticKITTIDataset
    for cls, kind in ((SemanticKITTIDataset, "kitti"), (NuscenesDataset, "nuscenes")):
        with pytest.raises(NotImplementedError, match="NKSR.*completion_fn"):
            cls("unused", "test", use_pc_completion=True, metadata_dir=tree[kind + "_meta"])
        with pytest.raises(NotImplementedError, match="NKSR.*completion_fn"):
            cls("unused", "test", use_pc_completion=True, cache_data_path="/c", overied_cache=True, metadata_dir=tree[kind + "_meta"])
        assert len(cls("unused", "test", use_pc_completion=True, metadata_dir=tree[kind + "_meta"], completion_fn=lambda p: p)) > 0
        assert len(cls("unused", "test", use_pc_completion=True, cache_data_path="/c", metadata_dir=tree[kind + "_meta"])) > 0   # served from the cache


def test_raw_items_need_a_device_and_no_worker(tree, monkeypatch):
    from umeregrobust_amd.datasets import SemanticKITTIDataset
    ds = SemanticKITTIDataset(tree["kitti"], "test", metadata_dir=tree["kitti_meta"], label_config=tree["label_config"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ds[0]
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="worker"):
        ds[0]


def completion_for_the_command_line(pts):
    return pts


def test_command_line_is_the_references(g17, tree, tmp_path, capsys):
    from umeregrobust_amd.datasets import sem_preprocessing as sp
    # the reference's own command line (README, "Training", step 2) parses, with its defaults
    args = sp.make_parser().parse_args(["--data_path", "/d", "--output_path", "/o", "--split", "val", "--nksr", "False", "--dataset_mode",
                                        "nuscenes", "--convert_points_to_grid", "False", "--voxel_size", "0.25", "--range_idxs", "[2, 5]"])
    assert (args.data_path, args.output_path, args.split, args.nksr, args.dataset_mode, args.convert_points_to_grid, args.voxel_size,
            args.range_idxs) == ("/d", "/o", "val", False, "nuscenes", False, 0.25, [2, 5])
    d = sp.make_parser().parse_args([])
    assert (d.output_path, d.split, d.nksr, d.dataset_mode, d.convert_points_to_grid, d.voxel_size, d.range_idxs, d.completion) == (
        "", "train", True, "kitti", True, 0.3, [], None)
    with pytest.raises(SystemExit):
        sp.make_parser().parse_args(["--split", "lokitti"])
    named = sp.make_parser().parse_args(["--completion", "test_raw_scan_cpu:completion_for_the_command_line"]).completion
    assert named.__name__ == "completion_for_the_command_line"
    # --nksr defaults to True: without a completion the command stops with the message
    base = ["--data_path", tree["kitti"], "--output_path", str(tmp_path), "--split", "test", "--metadata_dir", tree["kitti_meta"],
            "--label_config", tree["label_config"]]
    with pytest.raises(NotImplementedError, match="NKSR.*--completion module:function.*--nksr False"):
        sp.main(base)
    assert not os.path.exists(tmp_path / "test")
    # files that exist are skipped, before anything touches a scan or the GPU
    n_pairs = len(g17["kitti_v0_files"])
    for seq, f0, f1 in g17["kitti_v0_files"].tolist():
        os.makedirs(tmp_path / "test" / f"{seq:02d}", exist_ok=True)
        (tmp_path / "test" / f"{seq:02d}" / f"{f0:06d}_{f1:06d}.pickle").write_bytes(b"")
    assert sp.main(base + ["--nksr", "False"]) == (0, n_pairs)
    assert capsys.readouterr().out.count("EXIST (Skip)") == n_pairs
    assert sp.main(base + ["--nksr", "False", "--range_idxs", "[1, 4]"]) == (0, 3)
    nusc = ["--data_path", tree["nuscenes"], "--output_path", str(tmp_path / "n"), "--split", "test", "--dataset_mode", "nuscenes",
            "--metadata_dir", tree["nuscenes_meta"], "--nksr", "False"]
    for seq, f0, f1 in g17["nuscenes_v0_files"].tolist():
        os.makedirs(tmp_path / "n" / "test" / seq, exist_ok=True)
        (tmp_path / "n" / "test" / seq / f"{int(f0):06d}_{int(f1):06d}.pickle").write_bytes(b"")
    assert sp.main(nusc) == (0, len(g17["nuscenes_v0_files"]))


# ---- the host side of include/umereg_scan_prep.h ----

def test_scan_prep_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import raw_scan
    text = open(HEADER).read()
    assert sorted(raw_scan.SCAN_PREP_SIGNATURES) == ["umereg_scan_prep_f32", "umereg_scan_prep_workspace_bytes"]
    assert "umereg_scan_prep" not in open(os.path.join(REPO, "include", "umereg.h")).read()
    consts = dict(re.findall(r"#define\s+(UMEREG_SCAN_\w+)\s+(\d+)", text))
    assert (int(consts["UMEREG_SCAN_SEM16"]), int(consts["UMEREG_SCAN_KEEP_UNLABELED"])) == (raw_scan.SCAN_SEM16, raw_scan.SCAN_KEEP_UNLABELED)
    assert (int(consts["UMEREG_SCAN_ERR_KEY_RANGE"]), int(consts["UMEREG_SCAN_ERR_KEY_UNMAPPED"])) == (raw_scan.ERR_KEY_RANGE, raw_scan.ERR_KEY_UNMAPPED)
    assert int(consts["UMEREG_SCAN_PREP_BLOCK"]) == raw_scan.SCAN_PREP_BLOCK


def test_scan_prep_workspace_query_refuses_bad_sizes():
    from umeregrobust_amd import raw_scan
    q = raw_scan.load_native().umereg_scan_prep_workspace_bytes
    B = raw_scan.SCAN_PREP_BLOCK
    up = lambda v: (v + 255) // 256 * 256                                               # noqa: E731
    last = 0
    for n in (1, 63, 64, 65, B - 1, B, B + 1, 5000, 124668, B * 1024, B * 1024 + 1, 2 ** 31 - 1):
        got = q(n)
        assert got == 2 * up(4 * -(-n // B)) and got >= last and got % 256 == 0, n       # the blocks' counts and error bits
        last = got
    for bad in (0, -1, -2 ** 40, 2 ** 31, 2 ** 40):
        assert q(bad) == 0, bad
    assert raw_scan.workspace_bytes(2 ** 31) == 0 and raw_scan.workspace_bytes(5) == 512


def test_scan_prep_entry_checks_arguments_and_needs_a_device():
    from umeregrobust_amd import raw_scan
    lib = raw_scan.load_native()
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    names = ("scan", "n", "stride", "labels", "flags", "lut", "n_lut", "ego_hx", "ego_hy", "out_pts", "out_seg", "out_index", "out_count",
             "workspace", "workspace_bytes", "stream")
    sizes = dict(n=9, stride=4, flags=3, n_lut=5, ego_hx=2.5, ego_hy=1.0, workspace_bytes=1 << 12, stream=None)
    call = lambda **kw: lib.umereg_scan_prep_f32(*[kw.get(k, sizes.get(k, p)) for k in names])           # noqa: E731
    for kw in (dict(n=0), dict(n=-3), dict(n=2 ** 31), dict(stride=2), dict(stride=5), dict(flags=4), dict(flags=-1), dict(n_lut=-1),
               dict(n_lut=2 ** 31), dict(n_lut=0), dict(lut=None), dict(ego_hx=float("nan")), dict(ego_hy=float("nan")), dict(scan=None),
               dict(out_pts=None), dict(out_seg=None), dict(out_count=None), dict(scan=p + 2), dict(out_seg=p + 4), dict(labels=p + 1)):
        assert call(**kw) == -1, kw                                                      # UMEREG_EINVAL
        assert lib.umereg_last_error()
    if lib.umereg_device_count(None, 0) == 0:
        assert call() == -2                                                              # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        # optional pointers, a switched-off box and an unaligned 16-byte row are fine as arguments
        assert call(labels=None) == -2 and call(out_index=None) == -2 and call(lut=None, n_lut=0) == -2
        assert call(ego_hx=0.0) == -2 and call(ego_hy=-1.0) == -2 and call(stride=3) == -2 and call(scan=p + 4) == -2
        assert call(workspace=None, workspace_bytes=0) == -2                             # (the workspace is checked after the probe)


def test_prepare_cloud_raises_without_a_device(monkeypatch):
    from umeregrobust_amd import raw_scan
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device and no CPU fallback"):
        raw_scan.prepare_cloud(np.zeros((5, 4), np.float32))
    with pytest.raises(RuntimeError, match="GPU"):
        raw_scan.prepare_pair((torch.zeros(5, 3), torch.ones(5)), (torch.zeros(5, 3), torch.ones(5)), torch.eye(4), 0.3)
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="worker"):
        raw_scan.prepare_cloud(np.zeros((5, 4), np.float32))
