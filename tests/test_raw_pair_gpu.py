"""GPU: from raw scans to pair-cache items -- `prepare_pair` and both dataset classes without a cache against the reference's
`preprocess_getitem` (tests/golden/g17_raw_scan.npz: the same files, every row compared; the generator made them decided), the label
copy, the completion hook, the cache-writing command's round trip, and one training step on a cache written this way."""
import os

import numpy as np
import pytest
import torch

import raw_scan_ref as rref
from conftest import load_golden

pytestmark = pytest.mark.gpu

NAMES = rref.NAMES
# neighbourhoods sized for clouds of ~3 000 points, as the training driver's own tests use them
SMALL_TRAINING = dict(batch_size=2, ume_max_nn=64, ume_min_nn=8, ume_r_nn=2.0, ume_n_samples=32, num_pw_samples=128, eval_num_kpts=32, lr=1e-3,
                      use_aug=False)


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_raw_scan.npz")


@pytest.fixture(scope="module")
def tree(g17, tmp_path_factory):
    return rref.write_g17_tree(g17, tmp_path_factory.mktemp("g17"))


def dataset(kind, tree, gpu, **kw):
    from umeregrobust_amd.datasets import NuscenesDataset, SemanticKITTIDataset
    if kind == "kitti":
        return SemanticKITTIDataset(tree["kitti"], "test", metadata_dir=tree["kitti_meta"], label_config=tree["label_config"], device=gpu, **kw)
    return NuscenesDataset(tree["nuscenes"], "rotnuscenes", metadata_dir=tree["nuscenes_meta"], device=gpu, **kw)     # reads `test`


def compare(got, g17, tag, exact_points):
    """seg, coords, matches and the ground truth equal, on every row; points and src_pts_tform within 16 ulp of the largest
    |coordinate| (the bound of test_train_data_gpu.py for G16: alpha and beta of the grid map each carry the rounding of one max /
    min and are multiplied by a voxel index <= extent / voxel; the transform is three products and three sums at that magnitude)"""
    got = dict(zip(NAMES, got))
    want = {k: g17[tag + k] for k in NAMES}
    assert all(isinstance(v, torch.Tensor) for v in got.values())
    for k in ("src_coords", "tgt_coords", "src_seg", "tgt_seg", "matches", "gt_tform"):
        assert got[k].dtype == torch.from_numpy(want[k]).dtype and np.array_equal(got[k].cpu().numpy(), want[k]), tag + k
    assert len(want["matches"]) > 100 and (want["src_seg"] > 0).all()
    big = max(float(np.abs(want[k]).max()) for k in ("src_pts", "tgt_pts", "src_pts_tform"))
    ulp = float(np.spacing(np.float32(big)))
    for k in ("src_pts", "tgt_pts", "src_pts_tform"):
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape, tag + k
        err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - want[k]).max())
        print(f"{tag}{k}: max |ours - reference| {err:.3e} m = {err / ulp:.2f} ulp of {big:.2f} (bound 16 ulp = {16 * ulp:.3e})")
        if exact_points and k != "src_pts_tform":
            assert err == 0.0, tag + k
        assert err <= 16 * ulp, tag + k


@pytest.mark.parametrize("kind", ["kitti", "nuscenes"])
@pytest.mark.parametrize("grid", [True, False])
def test_raw_items_equal_the_reference(gpu, g17, tree, kind, grid):
    ds = dataset(kind, tree, gpu, convert_points_to_grid=grid)
    assert ds.cache_data_path == "" and ds.files[0][1:] == ([0, 1] if kind == "kitti" else (0, 1))
    item = ds[0]
    assert all(t.device.type == "cpu" for t in item)
    compare(item, g17, f"{kind}_{'grid' if grid else 'first'}_", exact_points=not grid)
    on_dev = dataset(kind, tree, gpu, convert_points_to_grid=grid, items_on_device=True)[0]
    assert all(t.device == gpu for t in on_dev) and all(torch.equal(a.cpu(), b) for a, b in zip(on_dev, item))


def test_prepare_pair_from_clouds(gpu, g17):
    """the two steps by hand: prepare_cloud per scan, prepare_pair on the clouds"""
    from umeregrobust_amd import raw_scan
    lut = raw_scan.learning_map_lut(g17["lm_keys"], g17["lm_values"])
    clouds = [raw_scan.prepare_cloud(g17[f"kitti_scan{f}"], g17[f"kitti_label{f}"], lut=lut, sem16=True, device=gpu) for f in (0, 1)]
    want = rref.scan_prep(g17["kitti_scan0"], g17["kitti_label0"], lut, sem16=True)
    assert np.array_equal(clouds[0][0].cpu().numpy(), want[0]) and np.array_equal(clouds[0][1].cpu().numpy(), want[1])
    item = raw_scan.prepare_pair(clouds[0], clouds[1], g17["kitti_tforms"][0], float(g17["voxel"]))
    compare(item, g17, "kitti_grid_", exact_points=False)
    # the nuScenes scans: ego box, labels as stored, no map
    clouds = [raw_scan.prepare_cloud(g17[f"nuscenes_scan{f}"], g17[f"nuscenes_label{f}"], ego_box=raw_scan.NUSCENES_EGO_BOX, device=gpu)
              for f in (0, 1)]
    scan = g17["nuscenes_scan0"]
    on_box = ((np.abs(scan[:, 0]) == 2.5) & (np.abs(scan[:, 1]) <= 1)) | ((np.abs(scan[:, 1]) == 1) & (np.abs(scan[:, 0]) <= 2.5))
    want = rref.scan_prep(scan, g17["nuscenes_label0"], ego_box=raw_scan.NUSCENES_EGO_BOX)
    assert on_box.sum() >= 6 and not np.isin(np.flatnonzero(on_box), want[2]).any()
    assert np.array_equal(clouds[0][0].cpu().numpy(), want[0]) and np.array_equal(clouds[0][1].cpu().numpy(), want[1])
    item = raw_scan.prepare_pair(clouds[0], clouds[1], g17["nuscenes_tforms"][0], float(g17["voxel"]), convert_points_to_grid=False)
    compare(item, g17, "nuscenes_first_", exact_points=True)


def test_label_copy_equals_the_reference(gpu, g17):
    from umeregrobust_amd import raw_scan
    pts, seg = torch.from_numpy(g17["kitti_load_pts"]).to(gpu), torch.from_numpy(g17["kitti_load_seg"]).to(gpu)
    new_pts = torch.from_numpy(g17["copy_new_pts"]).to(gpu)
    got = raw_scan.copy_labels_nearest(new_pts, pts, seg, thr=float(g17["copy_thr"]))
    want = g17["copy_new_seg"]
    assert got.dtype == torch.int64 and got.device == gpu and got.shape == want.shape
    print(f"label copy: {len(want)} new points, {int((want != 0).sum())} labelled, {int((got.cpu().numpy() != want).sum())} differ")
    assert (want != 0).sum() > 500 and (want == 0).sum() > 100 and np.array_equal(got.cpu().numpy(), want)
    assert raw_scan.copy_labels_nearest(new_pts[:0], pts, seg).shape == (0,)
    assert (raw_scan.copy_labels_nearest(new_pts[:7], pts[:0], seg[:0]) == 0).all()


@pytest.mark.parametrize("kind", ["kitti", "nuscenes"])
def test_completion_hook_runs_in_the_references_order(gpu, g17, tree, kind):
    """ego filter with the unlabelled points kept -> completion -> label copy -> unlabelled mask.  The toy completion keeps every
    second point, moved by 1 cm, and records what it was given; the expectation is built from the numpy restatement and a
    brute-force fp64 nearest neighbour (no point of these scans has two neighbours within rounding of each other at 1 cm)."""
    from umeregrobust_amd import raw_scan
    seen = []

    def toy(pts):
        seen.append(pts.clone())
        return pts[::2] + torch.tensor([0.01, 0.0, 0.0], device=pts.device)

    ds = dataset(kind, tree, gpu, use_pc_completion=True, completion_fn=toy)
    item = ds[0]
    assert len(seen) == 2
    lut = raw_scan.learning_map_lut(g17["lm_keys"], g17["lm_values"])
    clouds = []
    for f in (0, 1):
        opts = dict(lut=lut, sem16=True) if kind == "kitti" else dict(ego_box=raw_scan.NUSCENES_EGO_BOX)
        pts, seg, _, _ = rref.scan_prep(g17[f"{kind}_scan{f}"], g17[f"{kind}_label{f}"], keep_unlabeled=True, **opts)
        assert (seg == 0).sum() > 100, "the completion must see the unlabelled points"
        assert np.array_equal(seen[f].cpu().numpy(), pts), "the completion gets the cloud after the ego filter, unlabelled points included"
        new = pts[::2] + np.array([0.01, 0.0, 0.0], np.float32)
        d2 = ((new[:, None, :].astype(np.float64) - pts[None].astype(np.float64)) ** 2).sum(-1)
        new_seg = seg[d2.argmin(axis=1)]                                             # every distance is <= 1 cm: far below the threshold
        assert (new_seg == 0).any()
        clouds.append((torch.from_numpy(new[new_seg != 0]).to(gpu), torch.from_numpy(new_seg[new_seg != 0]).to(gpu)))
    want = raw_scan.prepare_pair(clouds[0], clouds[1], g17[f"{kind}_tforms"][0], float(g17["voxel"]))
    assert all(torch.equal(a, b) for a, b in zip(item, want)) and len(item[8]) > 0
    assert (item[1] != 0).all() and (item[4] != 0).all()


@pytest.fixture(scope="module")
def training_tree(g17, tmp_path_factory):
    """two pairs per split (frames 0 -> 1 and 1 -> 0) of small labelled scans, as a SemanticKITTI tree"""
    root = tmp_path_factory.mktemp("raw")
    (s0, w0), (s1, w1), T = rref.synth_labelled_scans(170, n=3000)
    rref.write_kitti_frame(root / "sequences", 3, 10, s0, w0)
    rref.write_kitti_frame(root / "sequences", 3, 12, s1, w1)
    tforms = np.stack([T, np.linalg.inv(T.astype(np.float64)).astype(np.float32)])
    for split in ("train", "val"):
        rref.write_metadata(root / "meta", split, np.array([[3, 10, 12], [3, 12, 10]], np.int64), tforms)
    return dict(data=str(root / "sequences"), meta=str(root / "meta"),
                label_config=rref.write_learning_map(root / "labels.yaml", g17["lm_keys"], g17["lm_values"]))


@pytest.fixture(scope="module")
def written_cache(gpu, training_tree, tmp_path_factory):
    from umeregrobust_amd.datasets import sem_preprocessing as sp
    out = tmp_path_factory.mktemp("cache")
    runs = {}
    for split in ("train", "val"):
        argv = ["--data_path", training_tree["data"], "--output_path", str(out), "--split", split, "--nksr", "False", "--dataset_mode", "kitti",
                "--metadata_dir", training_tree["meta"], "--label_config", training_tree["label_config"]]
        runs[split] = (sp.main(argv), sp.main(argv))
    return str(out), runs


def test_command_line_round_trip(gpu, training_tree, written_cache):
    from umeregrobust_amd.datasets import CachedPairDataset, SemanticKITTIDataset, batch_collate_fn_dset
    cache, runs = written_cache
    assert runs == {"train": ((2, 0), (0, 2)), "val": ((2, 0), (0, 2))}, "the first run writes both files, the second skips them"
    assert sorted(os.listdir(os.path.join(cache, "train", "03"))) == ["000010_000012.pickle", "000012_000010.pickle"]
    raw = SemanticKITTIDataset(training_tree["data"], "train", metadata_dir=training_tree["meta"], label_config=training_tree["label_config"], device=gpu)
    named = SemanticKITTIDataset(training_tree["data"], "train", cache_data_path=cache, skip_invalid_entries=False, metadata_dir=training_tree["meta"])
    listed = CachedPairDataset(cache, split="train")
    assert listed.files == [(3, 10, 12), (3, 12, 10)] and len(named) == len(raw) == 2
    items = [raw[i] for i in range(2)]
    for i, item in enumerate(items):
        assert [t.dtype for t in item] == [torch.float32, torch.int64, torch.int32] * 2 + [torch.float32, torch.float32, torch.int64]
        assert len(item[8]) > 300 and set(np.unique(item[1].numpy())) <= set(range(1, 10))
        for back in (listed[i], named[i]):
            assert len(back) == 9 and all(torch.equal(a, b) for a, b in zip(back, item))
    out = batch_collate_fn_dset([listed[0], listed[1]], num_matches=128, rng=np.random.RandomState(0))
    assert len(out) == 11 and out[10].shape == (2, 128, 2) and out[2].shape[1] == 4 and out[0].shape[0] == 2


def test_one_training_step_on_a_written_cache(gpu, written_cache, tmp_path):
    from umeregrobust_amd import train_coloring as tc

    class Scalars:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, float(value), int(step)))

        def of(self, tag):
            return [v for t, v, _ in self.rows if t == tag]

    cache, _ = written_cache
    args = tc.make_config("kitti", **{**SMALL_TRAINING, "device": str(gpu), "num_epochs": 1, "cache_data_path": cache, "num_workers": 0, "random_seed": 3})
    log = Scalars()
    run_dir = tc.run(args, summary_writer=log, out_path=str(tmp_path / "run"))
    losses = log.of("train/total_loss")
    print(f"one step on the written cache: train/total_loss {losses}, rows {[t for t, _, _ in log.rows]}")
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert os.path.exists(os.path.join(run_dir, "last_epoch_checkpoint.pth"))
