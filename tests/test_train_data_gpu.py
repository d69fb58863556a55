"""GPU: the trainer's data side on the device -- the augmented cache item against the reference's `cached_getitem_augmented`
(tests/golden/g16_train_data.npz: same cached item, same seed), the loader-worker guard, and `synth_train_item`."""
import numpy as np
import pytest
import torch

import train_data_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

NAMES = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_train_data.npz")


@pytest.fixture(scope="module")
def cache_dir(g16, tmp_path_factory):
    from umeregrobust_amd.datasets.kitti_dataset import write_cached_pair
    root = tmp_path_factory.mktemp("cache")
    item = tuple(torch.from_numpy(g16["item_" + k]) for k in NAMES)
    write_cached_pair(str(root / "train" / "00" / "000000_000001.pickle"), item)
    return str(root)


def test_augmented_item_equals_the_reference(gpu, g16, cache_dir):
    """coords, seg and the ground truth equal; grid points and src_pts_tform within 16 ulp of the largest |coordinate| (alpha and
    beta each carry the rounding of one max / min and are multiplied by a voxel index <= extent / voxel); matches equal on every
    source point whose margins exceed 1e-4 m, at most 1 % excluded"""
    from umeregrobust_amd.datasets.kitti_dataset import CachedPairDataset
    voxel = float(g16["item_voxel"])
    ds = CachedPairDataset(cache_dir, split="train", use_augmentations=True, voxel_size=voxel, device=gpu,
                           rng=np.random.RandomState(int(g16["item_seed"])))
    got = dict(zip(NAMES, ds[0]))
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" for v in got.values())
    for k in ("src_coords", "tgt_coords", "src_seg", "tgt_seg"):
        assert got[k].dtype == torch.from_numpy(g16["aug_" + k]).dtype and np.array_equal(got[k].numpy(), g16["aug_" + k]), k
    assert float(np.abs(got["gt_tform"].numpy() - g16["aug_gt_tform"]).max()) <= 1e-6
    big = max(float(np.abs(g16["aug_" + k]).max()) for k in ("src_pts", "tgt_pts", "src_pts_tform"))
    tol = 16 * float(np.spacing(np.float32(big)))
    for k in ("src_pts", "tgt_pts", "src_pts_tform"):
        err = float(np.abs(got[k].numpy().astype(np.float64) - g16["aug_" + k]).max())
        print(f"{k}: max |ours - reference| {err:.3e} m = {err / float(np.spacing(np.float32(big))):.2f} ulp of {big:.2f} (bound 16 ulp = {tol:.3e})")
        assert got[k].dtype == torch.float32 and err <= tol, k
    ok = ref.decided(g16["aug_src_pts"], g16["aug_tgt_pts"], g16["aug_gt_tform"], voxel / 2, 1e-4)
    print(f"matches: {int((~ok).sum())} of {len(ok)} source points inside the margin; ours {len(got['matches'])}, reference {len(g16['aug_matches'])}")
    assert (~ok).mean() <= 0.01
    assert got["matches"].dtype == torch.int64
    assert np.array_equal(ref.rows_on(got["matches"].numpy(), ok), ref.rows_on(g16["aug_matches"], ok))
    # without augmentation the item is the cache file's
    plain = CachedPairDataset(cache_dir, split="train")[0]
    assert all(np.array_equal(np.asarray(a), g16["item_" + k]) for k, a in zip(NAMES, plain))


def test_gpu_items_are_refused_inside_a_loader_worker(gpu, cache_dir, monkeypatch):
    from umeregrobust_amd.datasets.kitti_dataset import CachedPairDataset
    from umeregrobust_amd.synth import synth_train_item
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="worker"):
        CachedPairDataset(cache_dir, split="train", use_augmentations=True, device=gpu)[0]
    with pytest.raises(RuntimeError, match="worker"):
        synth_train_item(0, N=500)
    assert len(CachedPairDataset(cache_dir, split="train")[0]) == 9          # the plain item never touches the GPU


def test_synth_train_item_is_a_cache_item(gpu):
    from umeregrobust_amd.datasets.kitti_dataset import batch_collate_fn_dset
    from umeregrobust_amd.synth import FLAT_LABEL, synth_train_item
    items = [synth_train_item(40 + i, N=3000, device=gpu) for i in range(2)]
    for it in items:
        src, sseg, scoords, tgt, tseg, tcoords, moved, T, matches = it
        assert [x.dtype for x in it] == [torch.float32, torch.int64, torch.int32] * 2 + [torch.float32, torch.float32, torch.int64]
        assert src.shape == (len(sseg), 3) == tuple(scoords.shape) and tgt.shape == (len(tseg), 3) == tuple(tcoords.shape)
        assert 2500 <= len(src) <= 3000 and 2500 <= len(tgt) <= 3000 and moved.shape == src.shape and T.shape == (4, 4)
        assert len(np.unique(scoords.numpy(), axis=0)) == len(scoords) and len(np.unique(tcoords.numpy(), axis=0)) == len(tcoords)
        assert 0.2 < float((sseg == FLAT_LABEL).float().mean()) < 0.9 and set(np.unique(sseg.numpy())) - {FLAT_LABEL} <= set(range(1, 9))
        T_inv = torch.linalg.inv(T).numpy()
        want = ref.mutual(src.numpy(), tgt.numpy(), T.numpy(), T_inv, 0.15)
        print(f"synth item: {len(src)} / {len(tgt)} points, {len(matches)} mutual matches")
        assert len(want) > 300 and np.array_equal(matches.numpy(), want)
        assert float((moved - (src @ T[:3, :3].T + T[:3, 3])).abs().max()) < 1e-4
    out = batch_collate_fn_dset(items, num_matches=128, rng=np.random.RandomState(0))
    assert len(out) == 11 and out[10].shape == (2, 128, 2) and out[2].shape[1] == 4 and out[0].shape[0] == 2
    again = synth_train_item(40, N=3000, device=gpu)
    assert all(torch.equal(a, b) for a, b in zip(items[0], again))
