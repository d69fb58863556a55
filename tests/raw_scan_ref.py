"""Shared by the CPU and GPU tests of the raw-scan path: a numpy restatement of the semantics of include/umereg_scan_prep.h (the
reference's boolean masks, applied one after the other), and writers that lay the arrays of tests/golden/g17_raw_scan.npz out as
the dataset trees the readers expect."""
import os

import numpy as np

NAMES = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")
NUSC_SEQ = "n000-2018-01-01-00-00-00+0000"       # the sequence of G17's nuScenes frames (row 0 of its metadata)


def scan_prep(scan, labels=None, lut=None, sem16=False, keep_unlabeled=False, ego_box=None):
    """-> (pts f32 [m,3], seg i64 [m], index i64 [m], error bits): sem = word (& 0xFFFF), seg = lut[sem] (bit 1: a key beyond the
    table, bit 2: a negative entry; such rows count as label 0), then `pts[~ego]`, then `pts[~(seg == 0)]`, as the reference does."""
    scan = np.asarray(scan, dtype=np.float32)
    n = len(scan)
    sem = np.ones(n, np.uint32) if labels is None else np.asarray(labels).astype(np.uint32)
    if sem16:
        sem = sem & np.uint32(0xFFFF)
    err = 0
    if lut is None:
        seg = sem.astype(np.int64)
    else:
        lut = np.asarray(lut, dtype=np.int64)
        beyond = sem >= len(lut)
        seg = np.where(beyond, 0, lut[np.minimum(sem, len(lut) - 1)])
        err |= 1 if beyond.any() else 0
        err |= 2 if (seg < 0).any() else 0
        seg = np.maximum(seg, 0).astype(np.int64)
    pts, index = scan[:, :3], np.arange(n, dtype=np.int64)
    if ego_box is not None and ego_box[0] > 0 and ego_box[1] > 0:
        with np.errstate(invalid="ignore"):
            ego = (np.abs(pts[:, 0]) <= np.float32(ego_box[0])) & (np.abs(pts[:, 1]) <= np.float32(ego_box[1]))
        pts, seg, index = pts[~ego], seg[~ego], index[~ego]
    if not keep_unlabeled:
        unlabeled = seg == 0
        pts, seg, index = pts[~unlabeled], seg[~unlabeled], index[~unlabeled]
    return np.ascontiguousarray(pts), seg, index, err


def write_learning_map(path, keys, values):
    with open(path, "w") as f:
        f.write("name: test\nlearning_map:\n" + "".join(f"  {int(k)}: {int(v)}\n" for k, v in zip(keys, values)))
    return str(path)


def write_kitti_frame(root, seq, frame, scan, labels):
    base = os.path.join(str(root), f"{seq:02d}")
    os.makedirs(os.path.join(base, "velodyne"), exist_ok=True)
    os.makedirs(os.path.join(base, "labels"), exist_ok=True)
    np.ascontiguousarray(scan, dtype=np.float32).tofile(os.path.join(base, "velodyne", f"{frame:06d}.bin"))
    np.ascontiguousarray(labels, dtype=np.uint32).tofile(os.path.join(base, "labels", f"{frame:06d}.label"))


def write_nuscenes_frame(root, split, seq, frame, scan, labels, velo_data_type="bin"):
    base = os.path.join(str(root), split, "sequences", seq)
    os.makedirs(os.path.join(base, "velodyne"), exist_ok=True)
    os.makedirs(os.path.join(base, "labels"), exist_ok=True)
    if velo_data_type == "bin":
        np.ascontiguousarray(scan, dtype=np.float32).tofile(os.path.join(base, "velodyne", f"{frame:06d}.bin"))
    else:
        np.save(os.path.join(base, "velodyne", f"{frame:06d}.npy"), scan)
    if labels is not None:
        np.save(os.path.join(base, "labels", f"{frame:06d}.npy"), labels)


def write_metadata(root, split, files, tforms):
    os.makedirs(str(root), exist_ok=True)
    np.save(os.path.join(str(root), f"{split}_metadata.npy"), np.asarray(files))
    np.save(os.path.join(str(root), f"{split}_gt_tforms.npy"), np.asarray(tforms, dtype=np.float32))
    return str(root)


def write_g17_tree(g, root):
    """G17 as files -> dict(kitti=<sequences dir>, nuscenes=<base dir>, kitti_meta=, nuscenes_meta=<metadata dirs>, label_config=)"""
    root = str(root)
    out = dict(kitti=os.path.join(root, "kitti"), nuscenes=os.path.join(root, "nusc"), kitti_meta=os.path.join(root, "meta_kitti"),
               nuscenes_meta=os.path.join(root, "meta_nusc"))
    for f in (0, 1):
        write_kitti_frame(out["kitti"], 0, f, g[f"kitti_scan{f}"], g[f"kitti_label{f}"])
        write_nuscenes_frame(out["nuscenes"], "test", NUSC_SEQ, f, g[f"nuscenes_scan{f}"], g[f"nuscenes_label{f}"])
    write_metadata(out["kitti_meta"], "test", g["kitti_meta"], g["kitti_tforms"])
    for split in ("test", "rotnuscenes"):
        write_metadata(out["nuscenes_meta"], split, g["nuscenes_meta"], g["nuscenes_tforms"])
    out["label_config"] = write_learning_map(os.path.join(root, "label_config.yaml"), g["lm_keys"], g["lm_values"])
    return out


def synth_labelled_scans(seed, n=3000, voxel=0.3):
    """Two small SemanticKITTI-style scans of one `synth_scene` with labels that follow the geometry (road on the ground, eight
    classes by wall patch: what the UME loss needs), the second in the frame T maps to -> ((scan0, words0), (scan1, words1), T).
    Label keys 40 and 10, 11, 15, 18, 20, 30, 31, 32 map to nine distinct classes under SemanticKITTI's learning map."""
    from umeregrobust_amd.synth import synth_scene
    rng = np.random.RandomState(seed)
    n_all = int(np.ceil(n / 0.8))
    scene = synth_scene(rng, n_all, voxel)
    ground = scene[:, 2] < -1.4
    patch = (np.round(scene[:, 0] / 8.0) * 3 + np.round(scene[:, 1] / 8.0) * 5).astype(np.int64)
    keys = np.where(ground, 40, np.array([10, 11, 15, 18, 20, 30, 31, 32])[patch % 8]).astype(np.uint32)
    scene = scene + 0.5 * voxel
    a = np.deg2rad(rng.normal(0.0, 5.0))
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [rng.uniform(1, 3), rng.uniform(-2, 2), 0.05]
    out = []
    for f, idx in enumerate((rng.permutation(n_all)[:n], rng.permutation(n_all)[:n])):
        p = scene[idx] if f == 0 else scene[idx] @ T[:3, :3].T + T[:3, 3]
        scan = np.concatenate([p, rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
        out.append((scan, keys[idx] | (rng.randint(1, 1 << 16, n).astype(np.uint32) << 16)))
    return out[0], out[1], T.astype(np.float32)
