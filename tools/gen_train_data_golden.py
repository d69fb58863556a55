"""Regenerate tests/golden/g16_train_data.npz: results of the reference's own data-side functions, run on the CPU from the
reference tree with its un-installable imports replaced by the placeholders of oracle/gen_golden.py.  Only data goes into the file.

    python tools/gen_train_data_golden.py [out.npz]

  * `one_side_ball_query_matches`, `mutual_ball_query_matches` (utils/general_utils.py:38-59) on a 0.3 m lattice pair with a 17
    degree yaw, radius 0.15;
  * `convert_coords_to_grid_pts` (:27-35) on that pair's source cloud;
  * `cached_getitem_augmented` (datasets/kitti/kitti_dataset.py:460-509), called unbound on a stand-in `self` that serves one
    cached item, with `np.random` seeded; the two rotation matrices it draws are recomputed here from the same seed by the
    reference's expression and stored beside the item.

`ME.utils.sparse_quantize` is not installable: it is restated here as the first point of every occupied voxel, indices
ascending (parity unpinned, as everywhere in this project).  So that the fixture does not depend on the last bit of a matmul,
the cached item's clouds lose every point with a rotated coordinate within 1e-4 voxel of a voxel boundary (checked in fp64);
the number of dropped points is printed."""
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "g16_train_data.npz")
MAX_BYTES = 1 << 20       # no committed file above 1 MiB
VOXEL = 0.3
ITEM_SEED = 16


def sparse_quantize(coordinates, return_index=True, quantization_size=1.0, **_):
    q = torch.floor(torch.as_tensor(coordinates) / quantization_size).to(torch.int64).numpy()
    _, first = np.unique(q, axis=0, return_index=True)
    inds = np.sort(first)
    return torch.from_numpy(q[inds].astype(np.int32)), torch.from_numpy(inds)


def lattice_pair(seed, n, yaw_deg, shift):
    """source: lattice points at voxel centres; target: another subset of the same scene, rigidly moved and re-snapped to ITS lattice"""
    from umeregrobust_amd.synth import synth_scene
    rng = np.random.RandomState(seed)
    scene = synth_scene(rng, int(1.25 * n), VOXEL) + 0.5 * VOXEL
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = shift
    src = scene[rng.permutation(len(scene))[:n]]
    tgt = scene[rng.permutation(len(scene))[:n]] @ T[:3, :3].T + T[:3, 3]
    tgt = np.unique(np.floor(tgt / VOXEL), axis=0) * VOXEL + 0.5 * VOXEL
    tgt = tgt[rng.permutation(len(tgt))]
    return src.astype(np.float32), tgt.astype(np.float32), T.astype(np.float32)


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    from oracle import gen_golden
    gen_golden.import_reference()
    sys.modules["MinkowskiEngine"].utils.sparse_quantize = sparse_quantize
    import utils.general_utils as gu                      # the reference's
    from datasets.kitti import kitti_dataset as kd        # the reference's
    from scipy.spatial.transform import Rotation as R
    data = {}

    # ---- matches on a lattice pair ----
    src, tgt, T = lattice_pair(160, 4700, 17.0, [3.0, -2.0, 0.1])
    r = VOXEL / 2
    one = gu.one_side_ball_query_matches(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(T), r)
    mut = gu.mutual_ball_query_matches(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(T), r)
    print(f"pair: {len(src)} / {len(tgt)} points, one side {len(one)} rows, mutual {len(mut)} rows")
    assert 0 < len(mut) <= len(one) < len(src)
    coords = torch.floor(torch.from_numpy(src) / VOXEL).int()
    grid = gu.convert_coords_to_grid_pts(torch.from_numpy(src), coords, VOXEL)
    data.update(m_src=src, m_tgt=tgt, m_T=T, m_radius=np.float64(r), m_one_side=np.asarray(one, np.int64).reshape(-1, 2),
                m_mutual=np.asarray(mut, np.int64).reshape(-1, 2), g_coords=coords.numpy(), g_ds=np.float64(VOXEL), g_grid=grid.numpy())

    # ---- the augmented item ----
    s, t, Tg = lattice_pair(161, 2600, 8.0, [2.0, 1.0, 0.05])
    rs = np.random.RandomState(7)
    np.random.seed(ITEM_SEED)
    angles = [np.random.uniform(low=-180, high=180), np.random.uniform(low=-180, high=180)]
    rots = [torch.from_numpy(R.from_euler('z', a, degrees=True).as_matrix()).float().numpy() for a in angles]
    kept = []
    for pts, rot in ((s, rots[0]), (t, rots[1])):
        q = (pts.astype(np.float64) @ rot.astype(np.float64)) / VOXEL
        ok = (np.abs(q - np.round(q)) > 1e-4).all(axis=1)
        kept.append(pts[ok])
        print(f"augmented item: dropped {int((~ok).sum())} of {len(pts)} points within 1e-4 voxel of a boundary after rotation")
    s, t = kept
    item = (torch.from_numpy(s), torch.from_numpy(rs.randint(1, 12, len(s))).long(), torch.floor(torch.from_numpy(s) / VOXEL).int(),
            torch.from_numpy(t), torch.from_numpy(rs.randint(1, 12, len(t))).long(), torch.floor(torch.from_numpy(t) / VOXEL).int(),
            torch.from_numpy(s) @ torch.from_numpy(Tg[:3, :3]).T + torch.from_numpy(Tg[:3, 3]), torch.from_numpy(Tg),
            torch.from_numpy(np.asarray(gu.mutual_ball_query_matches(torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(Tg), r),
                                        np.int64).reshape(-1, 2)))
    stand_in = SimpleNamespace(voxel_size=VOXEL, cached_getitem=lambda idx: item)
    np.random.seed(ITEM_SEED)
    aug = kd.SemanticKITTIDataset.cached_getitem_augmented(stand_in, 0)
    names = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")
    for k, v in zip(names, item):
        data["item_" + k] = v.numpy()
    for k, v in zip(names, aug):
        data["aug_" + k] = v.numpy()
    data.update(item_seed=np.int64(ITEM_SEED), item_voxel=np.float64(VOXEL), aug_angles=np.asarray(angles), aug_rot_src=rots[0],
                aug_rot_tgt=rots[1])
    print(f"augmented item: {len(aug[0])} / {len(aug[3])} grid points, {len(aug[8])} matches")
    assert len(aug[8]) > 100

    with zipfile.ZipFile(out, "w", zipfile.ZIP_LZMA) as z:
        for k, v in data.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asarray(v), allow_pickle=False)
            z.writestr(k + ".npy", b.getvalue())
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes")
    assert size <= MAX_BYTES, "the fixture outgrew the size limit of a committed file"


if __name__ == "__main__":
    main(sys.argv)
