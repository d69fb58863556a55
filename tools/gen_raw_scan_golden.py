"""Regenerate tests/golden/g17_raw_scan.npz: results of the reference's own raw-scan path -- `load_semantic_kitti_point_cloud`,
`preprocess_getitem` of both dataset classes, both constructors' pair lists, the label-copy lines of
`lidar_point_cloud_completion` -- run on the CPU from the reference tree with its un-installable imports replaced by the
placeholders of oracle/gen_golden.py, on synthetic scans written to a temporary directory.  Only arrays go into the file.

    python tools/gen_raw_scan_golden.py [out.npz]

  * two SemanticKITTI frames (`.bin` x, y, z, remission; `.label` words with non-zero instance halves, about 10 % label 0, keys of
    the learning map that map to 0 among the others) and two nuScenes frames (`.bin`, labels `.npy`, points inside, outside and
    exactly on the ego box), cut from `synth.synth_scene`, the second frame of each moved by a known transform;
  * the reference's `learning_map` as two int arrays (the tests write their own yaml from them);
  * a 12-row metadata / transform set with |t| below, at and above 50 m, written where the reference's constructors look for it
    (they read it, like the label config, relative to the working directory: the reference is imported from its tree, then the
    work happens in the temporary directory);
  * `preprocess_getitem` called unbound on a stand-in `self`, with `convert_points_to_grid` True and False; the nuScenes item under
    split `rotnuscenes`, which reads the `test` directory;
  * `lidar_point_cloud_completion` called unbound with stand-ins for NKSR and the mesh sampler that hand back a prepared point set,
    so that its label-copy lines (KDTree, threshold 3 m) run as they are.

`ME.utils.sparse_quantize` is not installable: it is restated as the first point of every occupied voxel, indices ascending
(parity unpinned, as everywhere in this project).

So that the tests can compare every row, the generator makes the fixture DECIDED and asserts it: no kept point within 1e-4 voxel
of a voxel boundary; every match candidate, in both directions, decided in the sense of tests/train_data_ref.decided at 1e-4 m
(raw points of voxels that are not are removed and the item is made again, until none is left); no label-copy distance within
1e-4 m of 3 m or of a tie; more than 100 mutual matches per item."""
import io
import os
import sys
import tempfile
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "g17_raw_scan.npz")
MAX_BYTES = 1 << 20       # no committed file above 1 MiB
VOXEL = 0.3
N_FRAME = 3000            # scene points per frame, before the extra points
MARGIN = 1e-4
NAMES = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")
EGO = (2.5, 1.0)
NUSC_SEQ = "n000-2018-01-01-00-00-00+0000"


def sparse_quantize(coordinates, return_index=True, quantization_size=1.0, **_):
    q = torch.floor(torch.as_tensor(coordinates) / quantization_size).to(torch.int64).numpy()
    _, first = np.unique(q, axis=0, return_index=True)
    inds = np.sort(first)
    return torch.from_numpy(q[inds].astype(np.int32)), torch.from_numpy(inds)


def rigid(yaw_deg, shift):
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = shift
    return T.astype(np.float32)


def off_boundary(pts):
    q = pts.astype(np.float64) / VOXEL
    return (np.abs(q - np.round(q)) > MARGIN).all(axis=1)


def frame_pair(seed, T, extra):
    """two scans of one scene: points jittered inside their voxels, a third of the voxels hit twice (so that thinning has work),
    the second scan in the frame T maps to; `extra` [k,3] points are appended to both as they are; rows shuffled"""
    from umeregrobust_amd.synth import synth_scene
    rng = np.random.RandomState(seed)
    scene = synth_scene(rng, int(1.25 * N_FRAME), VOXEL) + 0.5 * VOXEL
    out = []
    for f in range(2):
        p = scene[rng.permutation(len(scene))[:N_FRAME]]
        p = np.concatenate([p, p[rng.permutation(N_FRAME)[:N_FRAME // 3]]])
        p = p + rng.uniform(-0.4 * VOXEL, 0.4 * VOXEL, p.shape)
        if f == 1:
            p = p @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
        p = np.concatenate([p, extra])[rng.permutation(len(p) + len(extra))].astype(np.float32)
        out.append(p[off_boundary(p)])
    return out, rng


def ego_points():
    """inside, exactly on and just outside the box |x| <= 2.5, |y| <= 1"""
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))      # noqa: E731
    xy = [(0.2, 0.1), (-1.9, 0.7), (2.5, 0.5), (-2.5, -0.4), (1.3, 1.0), (0.7, -1.0), (2.5, 1.0), (-2.5, -1.0),
          (up(2.5), 0.5), (-up(2.5), 1.0), (1.3, up(1.0)), (2.5, -up(1.0)), (3.1, 0.2), (0.4, 1.6)]
    return np.array([(x, y, -1.56 + 0.007 * i) for i, (x, y) in enumerate(xy)])


def write_frames(root, kind, scans, labels):
    for f, (scan, lab) in enumerate(zip(scans, labels)):
        base = os.path.join(root, "00") if kind == "kitti" else os.path.join(root, "test", "sequences", NUSC_SEQ)
        os.makedirs(os.path.join(base, "velodyne"), exist_ok=True)
        os.makedirs(os.path.join(base, "labels"), exist_ok=True)
        scan.tofile(os.path.join(base, "velodyne", f"{f:06d}.bin"))
        if kind == "kitti":
            lab.tofile(os.path.join(base, "labels", f"{f:06d}.label"))
        else:
            np.save(os.path.join(base, "labels", f"{f:06d}.npy"), lab)


def undecided_voxels(ref, item, T):
    """per side, the voxel coordinates whose grid point's match hangs on the last bits, in either direction"""
    sp, tp = item[0].numpy(), item[3].numpy()
    T_inv = torch.linalg.inv(torch.from_numpy(T)).numpy()
    bad_s = ~ref.decided(sp, tp, T, VOXEL / 2, MARGIN)
    bad_t = ~ref.decided(tp, sp, T_inv, VOXEL / 2, MARGIN)
    return item[2].numpy()[bad_s], item[5].numpy()[bad_t]


def without_voxels(scan, voxels):
    if len(voxels) == 0:
        return np.ones(len(scan), bool)
    q = np.floor(scan[:, :3].astype(np.float32) / np.float32(VOXEL)).astype(np.int64)
    key = lambda a: (a[:, 0] + 4096) * (1 << 26) + (a[:, 1] + 4096) * (1 << 13) + (a[:, 2] + 4096)      # noqa: E731
    return ~np.isin(key(q), key(voxels.astype(np.int64)))


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import train_data_ref as ref
    from oracle import gen_golden
    gen_golden.import_reference()
    sys.modules["MinkowskiEngine"].utils.sparse_quantize = sparse_quantize
    from datasets.kitti import kitti_dataset as kd            # the reference's (reads its label config from its own tree)
    from datasets.nuscenes import nuscenes_dataset as nd      # the reference's
    data = {}
    lm = kd.CFG["learning_map"]
    lm_keys, lm_values = np.array(list(lm.keys()), np.int64), np.array(list(lm.values()), np.int64)
    data.update(lm_keys=lm_keys, lm_values=lm_values, voxel=np.float64(VOXEL))

    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        # ---- metadata: 12 rows, |t| below, at and above 50 m; row 0 is the pair on disk ----
        T_k, T_n = rigid(17.0, [3.0, -2.0, 0.1]), rigid(-9.0, [-2.5, 1.5, 0.05])
        rs = np.random.RandomState(170)
        shifts = [None, (10, 5, 0), (30, 40, 0), (float(np.nextafter(np.float32(50), np.float32(60))), 0, 0), (60, 0, 0), (0, -49.5, 3),
                  (35, 35, 0), (1, 1, 1), (48, 14, 0), (20, -20, 2), (0, 50, 0), (-29, 40, 1)]
        assert np.linalg.norm(np.float32([30, 40, 0])) == 50 and np.linalg.norm(np.float32(shifts[3])) > 50
        for kind, T0 in (("kitti", T_k), ("nuscenes", T_n)):
            tf = np.stack([T0] + [rigid(rs.uniform(-180, 180), s) for s in shifts[1:]])
            frames = np.array([[0, 0, 1]] + [[rs.randint(0, 11), a, a + rs.randint(1, 20)] for a in rs.randint(0, 4000, 11)], np.int64)
            if kind == "nuscenes":
                seqs = [NUSC_SEQ] + [f"n{rs.randint(0, 999):03d}-2018-0{rs.randint(1, 9)}-11-11-54-16+0800" for _ in range(11)]
                meta = np.array([[s, str(a), str(b)] for s, (_, a, b) in zip(seqs, frames)])
            else:
                meta = frames
            os.makedirs(f"datasets/{kind}/metadata")
            for split in ("test", "rotnuscenes") if kind == "nuscenes" else ("test",):
                np.save(f"datasets/{kind}/metadata/{split}_metadata.npy", meta)
                np.save(f"datasets/{kind}/metadata/{split}_gt_tforms.npy", tf)
            data[f"{kind}_meta"], data[f"{kind}_tforms"] = meta, tf

        # ---- both constructors' pair lists ----
        variants = [dict(), dict(cache_data_path="/c"), dict(cache_data_path="/c", skip_invalid_entries=False),
                    dict(cache_data_path="/c", overied_cache=True, dataset_size=5), dict(dataset_size=3)]
        data["variant_cache"] = np.array([v.get("cache_data_path", "") for v in variants])
        data["variant_skip"] = np.array([v.get("skip_invalid_entries", True) for v in variants])
        data["variant_overied"] = np.array([v.get("overied_cache", False) for v in variants])
        data["variant_size"] = np.array([v.get("dataset_size", -1) for v in variants], np.int64)
        for kind, cls in (("kitti", kd.SemanticKITTIDataset), ("nuscenes", nd.NuscenesDataset)):
            for i, v in enumerate(variants):
                ds = cls("unused", "test", **v)
                data[f"{kind}_v{i}_files"] = np.array(ds.files) if kind == "nuscenes" else np.array(ds.files, np.int64).reshape(-1, 3)
                data[f"{kind}_v{i}_tforms"] = ds.gt_tforms
                data[f"{kind}_v{i}_cache"] = np.array(ds.cache_data_path)
                print(f"{kind} variant {i} {v}: {len(ds.files)} pairs")
        assert len(data["kitti_v0_files"]) == 10 and len(data["kitti_v1_files"]) == 9 and len(data["nuscenes_v0_files"]) == 12
        assert (data["kitti_v0_files"] == data["kitti_meta"][2]).all(axis=1).any(), "the row with |t| exactly 50 must be kept"

        # ---- the frames ----
        rl = np.random.RandomState(171)
        kitti_keys = np.array([0, 1, 52, 99, 10, 11, 30, 40, 44, 48, 50, 51, 60, 70, 71, 72, 80, 81, 252, 259])
        p_keys = np.array([0.10, 0.02, 0.02, 0.02] + [0.84 / 16] * 16)
        (k0, k1), _ = frame_pair(172, T_k, np.zeros((0, 3)))
        (n0, n1), _ = frame_pair(173, T_n, ego_points())
        scans = {"kitti": [np.concatenate([p, rl.randint(0, 256, (len(p), 1)).astype(np.float32) / 255], axis=1).astype(np.float32)
                           for p in (k0, k1)],
                 "nuscenes": [np.concatenate([p, rl.randint(0, 256, (len(p), 1)).astype(np.float32)], axis=1).astype(np.float32)
                              for p in (n0, n1)]}
        labels = {"kitti": [(rl.choice(kitti_keys, len(s), p=p_keys).astype(np.uint32) | (rl.randint(1, 1 << 16, len(s)).astype(np.uint32) << 16))
                            for s in scans["kitti"]],
                  "nuscenes": [np.where(rl.uniform(size=len(s)) < 0.1, 0, rl.randint(1, 17, len(s))).astype(np.int64) for s in scans["nuscenes"]]}
        assert all((lab >> 16).min() > 0 for lab in labels["kitti"])

        def reference_item(kind, grid):
            if kind == "kitti":
                self = SimpleNamespace(files=[[0, 0, 1]], data_path=os.path.join(tmp, "kitti"), gt_tforms=T_k[None], use_pc_completion=False,
                                       voxel_size=VOXEL, convert_points_to_grid=grid, split="test")
                return kd.SemanticKITTIDataset.preprocess_getitem(self, 0)
            self = SimpleNamespace(files=[(NUSC_SEQ, 0, 1)], data_path=os.path.join(tmp, "nusc"), gt_tforms=T_n[None], use_pc_completion=False,
                                   voxel_size=VOXEL, convert_points_to_grid=grid, split="rotnuscenes")
            return nd.NuscenesDataset.preprocess_getitem(self, 0)

        for kind, T in (("kitti", T_k), ("nuscenes", T_n)):
            root = os.path.join(tmp, "kitti" if kind == "kitti" else "nusc")
            for rounds in range(20):
                write_frames(root, kind, scans[kind], labels[kind])
                items = {g: reference_item(kind, g) for g in (True, False)}
                bad = [undecided_voxels(ref, items[g], T) for g in (True, False)]
                n_bad = sum(len(b[0]) + len(b[1]) for b in bad)
                print(f"{kind} round {rounds}: {len(scans[kind][0])} / {len(scans[kind][1])} scan rows, {n_bad} undecided grid points")
                if n_bad == 0:
                    break
                for side in (0, 1):
                    keep = without_voxels(scans[kind][side], np.concatenate([b[side] for b in bad]))
                    scans[kind][side], labels[kind][side] = scans[kind][side][keep], labels[kind][side][keep]
            assert n_bad == 0, "the fixture did not become decided"
            for f in (0, 1):
                data[f"{kind}_scan{f}"], data[f"{kind}_label{f}"] = scans[kind][f], labels[kind][f]
            for g in (True, False):
                tag = f"{kind}_{'grid' if g else 'first'}_"
                for k, v in zip(NAMES, items[g]):
                    data[tag + k] = np.asarray(v)
                print(f"{tag}: {len(items[g][0])} / {len(items[g][3])} points, {len(items[g][8])} mutual matches")
                assert len(items[g][8]) > 100 and items[g][8].dtype == torch.int64 and items[g][2].dtype == torch.int32
            frac0 = np.mean([((lab & 0xFFFF) == 0).mean() for lab in labels[kind]])
            assert 0.07 < frac0 < 0.13, frac0
        # what is kept lies off the voxel boundaries (the scans were cut that way; the removals cannot change it)
        assert all(off_boundary(s[:, :3]).all() for k in scans for s in scans[k])
        on_box = lambda s: ((np.abs(s[:, 0]) == 2.5) & (np.abs(s[:, 1]) <= 1)) | ((np.abs(s[:, 1]) == 1) & (np.abs(s[:, 0]) <= 2.5))      # noqa: E731
        inside = lambda s: (np.abs(s[:, 0]) < 2.5) & (np.abs(s[:, 1]) < 1)                                                               # noqa: E731
        for s in scans["nuscenes"]:
            assert on_box(s).sum() >= 6 and inside(s).sum() >= 2 and (~inside(s) & ~on_box(s)).sum() > 1000

        # ---- load_semantic_kitti_point_cloud ----
        pts, seg = kd.load_semantic_kitti_point_cloud(os.path.join(tmp, "kitti"), 0, 0)
        data.update(kitti_load_pts=np.asarray(pts), kitti_load_seg=np.asarray(seg, np.int64))
        assert set(np.unique(labels["kitti"][0] & 0xFFFF)) >= {0, 1, 52, 99, 10, 252} and (seg == 0).mean() > 0.12

        # ---- the label-copy lines on a second point set ----
        rc = np.random.RandomState(174)
        src_pts, src_seg = torch.from_numpy(np.ascontiguousarray(pts)).float(), torch.from_numpy(np.asarray(seg)).long()
        new_pts = np.concatenate([np.asarray(pts)[rc.permutation(len(pts))[:1500]] + rc.uniform(-2.5, 2.5, (1500, 3)),
                                  rc.uniform(-60, 60, (700, 3)) * [1, 1, 0.2]]).astype(np.float32)
        d2 = ((new_pts[:, None, :].astype(np.float64) - np.asarray(pts)[None].astype(np.float64)) ** 2).sum(-1)
        two = np.sqrt(np.partition(d2, 1, axis=1)[:, :2])
        ok = (np.abs(two[:, 0] - 3.0) > MARGIN) & (two[:, 1] - two[:, 0] > MARGIN)
        new_pts = new_pts[ok]
        print(f"label copy: {len(new_pts)} new points ({int((~ok).sum())} within {MARGIN} m of 3 m or of a tie removed), "
              f"{int((two[ok, 0] <= 3).sum())} within 3 m")
        assert (two[ok, 0] <= 3).sum() > 500 and (two[ok, 0] > 3).sum() > 100

        class _Sampled:
            points = new_pts.astype(np.float64)

        class _Mesh:
            v = f = None

            def sample_points_uniformly(self, **_):
                return _Sampled()

        class _Reconstructor:
            def __init__(self, device):
                pass

            def reconstruct(self, *a, **k):
                return SimpleNamespace(extract_dual_mesh=lambda **_: _Mesh())

        kd.nksr.Reconstructor, kd.nksr.get_estimate_normal_preprocess_fn = _Reconstructor, lambda *a: None
        kd.vis.mesh = lambda v, f: _Mesh()
        self = SimpleNamespace(NKSR_DEVICE="cpu", NKSR_DETAIL_LEVEL=None, NKSR_KNN=128, NKSR_FOV_DEG=90.0, NKSR_NUM_SAMPLED_POINTS=len(new_pts),
                               LABEL_COPY_DIST_THR=kd.SemanticKITTIDataset.LABEL_COPY_DIST_THR)
        got_pts, got_seg = kd.SemanticKITTIDataset.lidar_point_cloud_completion(self, src_pts, src_seg)
        assert np.array_equal(got_pts.numpy(), new_pts) and got_seg.dtype == torch.int64
        data.update(copy_new_pts=new_pts, copy_new_seg=got_seg.numpy(), copy_thr=np.float64(self.LABEL_COPY_DIST_THR))
        os.chdir(REPO)

    with zipfile.ZipFile(out, "w", zipfile.ZIP_LZMA) as z:
        for k, v in data.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asarray(v), allow_pickle=False)
            z.writestr(k + ".npy", b.getvalue())
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes, {len(data)} arrays")
    assert size <= MAX_BYTES, "the fixture outgrew the size limit of a committed file"


if __name__ == "__main__":
    main(sys.argv)
