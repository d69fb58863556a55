"""From raw lidar scans to a pair-cache item: the reference's `preprocess_getitem` (datasets/kitti/kitti_dataset.py:388-439,
datasets/nuscenes/nuscenes_dataset.py:387-447) without MinkowskiEngine, nksr or pycg.

    scan = read_kitti_scan(".../velodyne/000000.bin");  labels = read_kitti_label(".../labels/000000.label", len(scan))
    lut = load_learning_map("kitti_config.yaml")                                  # the user's own copy of the label map
    pts, seg = prepare_cloud(scan, labels, lut=lut, sem16=True)                   # on the device, through csrc/scan_prep.hip
    item = prepare_pair((src_pts, src_seg), (tgt_pts, tgt_seg), gt_tform, 0.3)    # the 9-tuple of a cache file

The readers are the host's (numpy, the reference's own calls and checks).  Everything behind them runs on the GPU:
`prepare_cloud` is ONE call of `umereg_scan_prep_f32` (include/umereg_scan_prep.h: the semantic half of the label word, the
learning map, the ego box, the unlabelled mask, compaction in scan order) and one device -> host read for the count;
`prepare_pair` is voxel thinning (`quantize_on_device`), grid points, the exact mutual radius search (`gt_matches.mutual`) and
the transformed source (`rotate_rows`), the same calls the augmentation of a cached item makes.  There is no CPU fallback.

The surface reconstruction of `lidar_point_cloud_completion` (NKSR, :511-533) is not part of this library; its label-transfer
half is (`copy_labels_nearest`), and `complete_cloud` joins a caller-supplied `completion_fn(pts) -> new_pts` to it
(`equalizer.sampling_equalizer` is a ready-made one: the library's own density equalizer, not NKSR's output).

The entry points of include/umereg_scan_prep.h are typed by `_lib.TABLES`; `scan_prep_raw` takes caller-owned outputs and
workspace and never waits for the device."""
import os
from contextlib import nullcontext

import numpy as np
import torch

from . import _lib
from .datasets.kitti_dataset import _refuse_gpu_in_worker, quantize_on_device, rotate_rows

SCAN_PREP_SIGNATURES = _lib.TABLES["umereg_scan_prep.h"]
load_native = _lib.load

SCAN_SEM16, SCAN_KEEP_UNLABELED = 1, 2                       # UMEREG_SCAN_* flags
ERR_KEY_RANGE, ERR_KEY_UNMAPPED = 1, 2                       # UMEREG_SCAN_ERR_* bits
SCAN_PREP_BLOCK = 1024                                       # UMEREG_SCAN_PREP_BLOCK: rows per workgroup
SCAN_PREP_SCAN_THREADS = 1024                                # threads of the block that scans the block counts

EXTENSIONS_SCAN, EXTENSIONS_LABEL = (".bin",), (".label",)   # LaserScan.EXTENSIONS_SCAN, SemLaserScan.EXTENSIONS_LABEL
NUSCENES_EGO_BOX = (2.5, 1.0)                                # nuscenes_dataset.py:404
LABEL_COPY_DIST_THR = 3.0                                    # SemanticKITTIDataset.LABEL_COPY_DIST_THR


def workspace_bytes(n):
    return int(_lib.load().umereg_scan_prep_workspace_bytes(int(n)))


# ---- host readers -------------------------------------------------------------------------------------------------------------

def read_kitti_scan(path):
    """`LaserScan.open_scan` (kitti_dataset.py:73-95): f32 [n,4] rows x, y, z, remission.  The reference keeps `scan[:, 0:3]`;
    the whole rows are returned here, because `prepare_cloud` reads them as they are (one 16-byte load per point)."""
    if not isinstance(path, str):
        raise TypeError(f"Filename should be string type, but was {type(path)}")
    if not any(path.endswith(ext) for ext in EXTENSIONS_SCAN):
        raise RuntimeError("Filename extension is not valid scan file.")
    return np.fromfile(path, dtype=np.float32).reshape((-1, 4))


def read_kitti_label(path, n_points=None):
    """`SemLaserScan.open_label` (kitti_dataset.py:234-251): the u32 label words (semantic label in the lower half, instance id
    in the upper).  n_points: the size of the scan the labels belong to; another length raises, as `set_label` does (:261-267)."""
    if not isinstance(path, str):
        raise TypeError(f"Filename should be string type, but was {type(path)}")
    if not any(path.endswith(ext) for ext in EXTENSIONS_LABEL):
        raise RuntimeError("Filename extension is not valid label file.")
    label = np.fromfile(path, dtype=np.uint32).reshape((-1))
    if n_points is not None and label.shape[0] != int(n_points):
        raise ValueError(f"Scan and Label don't contain same number of points ({int(n_points)} points, {label.shape[0]} labels)")
    return label


def read_nuscenes_cloud(base_path, split, seq_id, frame_id, velo_data_type="bin"):
    """`load_nuscenes_point_cloud` (nuscenes_dataset.py:294-312) -> (scan f32 [n,4] for "bin" / the stored array for "npy",
    labels int [n] or None where `labels/<frame>.npy` does not exist: every point then counts as label 1, :310)."""
    velo_path = os.path.join(base_path, split, "sequences", seq_id, "velodyne", f"{frame_id:06d}." + velo_data_type)
    label_path = os.path.join(base_path, split, "sequences", seq_id, "labels", f"{frame_id:06d}.npy")
    if velo_data_type == "bin":
        scan = read_kitti_scan(velo_path)
    elif velo_data_type == "npy":
        scan = np.load(velo_path).astype(np.float32, copy=False)          # (preprocess_getitem's `.float()`)
    else:
        raise NotImplementedError(velo_path)
    labels = np.load(label_path).astype(int) if os.path.exists(label_path) else None
    if labels is not None and labels.shape[0] != scan.shape[0]:
        raise ValueError(f"Scan and Label don't contain same number of points ({scan.shape[0]} points, {labels.shape[0]} labels)")
    return scan, labels


def learning_map_lut(keys, values):
    """A label map as the table `seg = lut[sem]` of the kernel: int32 [max key + 1], -1 where the map has no such key."""
    keys, values = np.asarray(keys, dtype=np.int64).reshape(-1), np.asarray(values, dtype=np.int64).reshape(-1)
    if len(keys) == 0 or len(keys) != len(values) or keys.min() < 0 or values.min() < 0 or max(keys.max(), values.max()) >= 2 ** 31 - 1:
        raise ValueError("learning map: keys and values must be non-negative 32-bit integers, one value per key")
    lut = np.full(int(keys.max()) + 1, -1, dtype=np.int32)
    lut[keys] = values
    return lut


def load_learning_map(yaml_path):
    """The `learning_map` of a SemanticKITTI label config (the reference's `CFG['learning_map']`, kitti_dataset.py:17, :312) as a
    LUT for `prepare_cloud`.  The config is the dataset's: point this at your copy of `kitti_config.yaml` / `semantic-kitti.yaml`."""
    import yaml
    with open(yaml_path, "r") as f:
        cfg = yaml.safe_load(f)
    if not isinstance(cfg, dict) or not isinstance(cfg.get("learning_map"), dict):
        raise KeyError(f"{yaml_path}: no `learning_map` mapping")
    m = cfg["learning_map"]
    return learning_map_lut(list(m.keys()), list(m.values()))


# ---- one scan on the device ---------------------------------------------------------------------------------------------------

def scan_prep_raw(scan, labels, lut, flags, ego_box, out_pts, out_seg, out_index, out_count, workspace):
    """Enqueue one `umereg_scan_prep_f32` on the current stream.  scan f32 [n,3|4] contiguous; labels int32 [n] holding the u32
    words, or None; lut int32 [k] or None; ego_box (hx, hy) or None; out_pts f32 [n,3], out_seg i64 [n], out_index i64 [n] or None,
    out_count i32 [2] (kept, error bits), workspace uint8 of >= workspace_bytes(n): all on one device."""
    hx, hy = (0.0, 0.0) if ego_box is None else ego_box
    p = _lib.ptr
    _lib.call(scan.device, _lib.load().umereg_scan_prep_f32, scan.data_ptr(), scan.shape[0], scan.shape[1], p(labels), int(flags), p(lut),
              0 if lut is None else lut.shape[0], float(hx), float(hy), out_pts.data_ptr(), out_seg.data_ptr(), p(out_index),
              out_count.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(scan.device))


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("raw scans are prepared on the GPU (csrc/scan_prep.hip); there is no HIP device and no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _label_words(labels, n, dev):
    """the u32 label words as an int32 device tensor (same bits)"""
    if isinstance(labels, torch.Tensor):
        if labels.is_floating_point() or labels.shape != (n,):
            raise ValueError(f"prepare_cloud: labels must be {n} integers, got {labels.dtype} {tuple(labels.shape)}")
        return labels.to(dev).to(torch.int32).contiguous()
    a = np.asarray(labels)
    if a.dtype.kind not in "iu" or a.shape != (n,):
        raise ValueError(f"prepare_cloud: labels must be {n} integers, got {a.dtype} {a.shape}")
    if a.dtype != np.uint32:
        if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
            raise ValueError("prepare_cloud: a label does not fit an unsigned 32-bit word")
        a = a.astype(np.uint32)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def prepare_cloud(scan, labels=None, *, lut=None, sem16=False, keep_unlabeled=False, ego_box=None, device=None, return_index=False):
    """One raw scan -> (pts f32 [m,3], seg i64 [m]) on the device (with return_index: + the scan row of every kept point,
    i64 [m], ascending): what the reference's loaders and the masks of `preprocess_getitem` leave of it, in scan order.

    scan    f32 [n,3] or [n,4] (numpy array, host or device tensor); only x, y, z are read
    labels  [n] integers (KITTI: the u32 words of a `.label` file, with sem16=True), or None: label 1 everywhere
    lut     int32 table from `load_learning_map` / `learning_map_lut`, or None for the identity; a label that is no key of the
            map raises KeyError, as the reference's dictionary lookup does
    ego_box (hx, hy): drop points with |x| <= hx and |y| <= hy (nuScenes: NUSCENES_EGO_BOX)
    keep_unlabeled  keep the points whose mapped label is 0 (the state before a point-cloud completion)
    One device -> host read (the count and the error bits)."""
    who = "prepare_cloud"
    _refuse_gpu_in_worker(who)
    dev = _device(device)
    scan = torch.as_tensor(scan)
    if scan.dim() != 2 or scan.shape[1] not in (3, 4) or scan.dtype != torch.float32:
        raise ValueError(f"{who}: the scan must be float32 [n,3] or [n,4], got {scan.dtype} {tuple(scan.shape)}")
    n = scan.shape[0]
    scan = scan.to(dev).contiguous()
    words = None if labels is None else _label_words(labels, n, dev)
    table = None if lut is None else torch.as_tensor(lut).to(device=dev, dtype=torch.int32).contiguous()
    if table is not None and (table.dim() != 1 or table.shape[0] == 0):
        raise ValueError(f"{who}: the label map must be a non-empty 1-d table")
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    seg = torch.empty(n, dtype=torch.int64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev) if return_index else None
    if n == 0:
        return (pts, seg, index) if return_index else (pts, seg)
    cnt = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(n), dtype=torch.uint8, device=dev)
    flags = (SCAN_SEM16 if sem16 else 0) | (SCAN_KEEP_UNLABELED if keep_unlabeled else 0)
    scan_prep_raw(scan, words, table, flags, ego_box, pts, seg, index, cnt, ws)
    m, bad = cnt.tolist()                                    # the one device -> host read
    if bad:
        what = [s for bit, s in ((ERR_KEY_RANGE, f"beyond the map's largest key {table.shape[0] - 1}"),
                                 (ERR_KEY_UNMAPPED, "that is no key of the map")) if bad & bit]
        raise KeyError(f"{who}: the scan has a semantic label " + " and one ".join(what))
    return (pts[:m], seg[:m], index[:m]) if return_index else (pts[:m], seg[:m])


def copy_labels_nearest(new_pts, pts, seg, thr=LABEL_COPY_DIST_THR):
    """The label-transfer half of `lidar_point_cloud_completion` (kitti_dataset.py:535-540): a new point takes the label of its
    nearest original point where their distance is <= thr, else 0.  new_pts f32 [k,3], pts f32 [n,3], seg [n] on the device ->
    int64 [k].  Built from `ops.nn1_pair` and a gather.
    The distance is the kernel's fp32 one: the nearest point is the one `ops.nn1_pair` finds on fp32 distances, and the test
    against the threshold is (dx*dx + dy*dy) + dz*dz <= thr*thr in fp32 on the gathered point, where scipy's KDTree works in
    fp64.  Only new points within rounding of `thr`, or with two original points within rounding of the same distance, can differ."""
    from . import ops
    new_pts, pts = new_pts.float().contiguous(), pts.float().contiguous()
    if new_pts.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=new_pts.device)
    if pts.shape[0] == 0:
        return torch.zeros(new_pts.shape[0], dtype=torch.int64, device=new_pts.device)
    idx, _ = ops.nn1_pair(new_pts, new_pts[:1], pts, pts[:1])         # (the call serves a pair; the second side is one point)
    d = new_pts - pts[idx]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    near = d2 <= torch.tensor(float(thr), dtype=torch.float32, device=d2.device) ** 2
    return torch.where(near, seg.to(torch.int64)[idx], torch.zeros((), dtype=torch.int64, device=d2.device))


def completion_missing():
    return NotImplementedError(
        "use_pc_completion=True asks for the reference's NKSR surface reconstruction (lidar_point_cloud_completion), which is not part of "
        "this library: pass completion_fn(pts) -> new_pts (command line: --completion module:function), or switch it off "
        "(use_pc_completion=False, command line: --nksr False).  The library's own equalizer is a ready-made one: "
        "umeregrobust_amd.equalizer.sampling_equalizer (command line: --completion umeregrobust_amd.equalizer:sampling_equalizer)")


def complete_cloud(pts, seg, completion_fn, thr=LABEL_COPY_DIST_THR):
    """`lidar_point_cloud_completion` with the reconstruction supplied by the caller: new_pts = completion_fn(pts) (f32 [k,3];
    a host result is copied up), labels copied from the nearest original point -> (new_pts, new_seg) on the device of `pts`."""
    if completion_fn is None:
        raise completion_missing()
    new_pts = torch.as_tensor(completion_fn(pts)).to(device=pts.device, dtype=torch.float32)
    if new_pts.dim() != 2 or new_pts.shape[1] != 3:
        raise ValueError(f"completion_fn must return points [k,3], got {tuple(new_pts.shape)}")
    new_pts = new_pts.contiguous()
    return new_pts, copy_labels_nearest(new_pts, pts, seg, thr)


def drop_unlabeled(pts, seg):
    """"Remove unlabeled points" (kitti_dataset.py:407-413) of a cloud that is already on the device"""
    keep = seg != 0
    return pts[keep], seg[keep]


# ---- one pair -----------------------------------------------------------------------------------------------------------------

def prepare_pair(src, tgt, gt_tform, voxel_size, convert_points_to_grid=True, to_host=True, phase=None):
    """`preprocess_getitem` from "Voxlize point clouds" to its end (kitti_dataset.py:415-439) on the device.  src, tgt: (pts f32
    [n,3], seg i64 [n]) device tensors with the unlabelled points already removed (`prepare_cloud`); gt_tform [4,4].
    -> (src_pts, src_seg, src_coords i32, tgt_pts, tgt_seg, tgt_coords, src_pts_tform, gt_tform, matches i64 [m,2]): on the host,
    or with to_host=False on the device where it was made, as `augmented_item` returns it.
    Thinning is `quantize_on_device`; the points are the grid points of `convert_coords_to_grid_pts` or, with
    convert_points_to_grid=False, the first point of every voxel; matches are the exact mutual search at voxel_size / 2;
    src_pts_tform is `rotate_rows(src_pts, R^T) + t`, the stated order of `augmented_item`.
    phase: optional `phase(name)` -> context manager around "thinning", "grid_points", "matches", "to_host"."""
    from .utils.general_utils import convert_coords_to_grid_pts, mutual_ball_query_matches
    _refuse_gpu_in_worker("prepare_pair")
    phase = phase or (lambda name: nullcontext())
    sides = []
    for pts, seg in (src, tgt):
        if pts.device.type != "cuda":
            raise RuntimeError("prepare_pair: the clouds must be on the GPU (prepare_cloud puts them there); there is no CPU fallback")
        with phase("thinning"):
            pts = pts.float().contiguous()
            coords, inds = quantize_on_device(pts, voxel_size)
            seg = seg.long()[inds]
        with phase("grid_points"):
            grid = convert_coords_to_grid_pts(pts, coords, voxel_size) if convert_points_to_grid else pts[inds]
        sides.append((grid, seg, coords))
    gt_tform = torch.as_tensor(gt_tform).float().cpu()
    with phase("matches"):
        T_dev = gt_tform.to(sides[0][0].device)
        matches = mutual_ball_query_matches(sides[0][0], sides[1][0], gt_tform, voxel_size / 2).long()
        moved = rotate_rows(sides[0][0], T_dev[:3, :3].T.contiguous()) + T_dev[:3, 3]
    if not to_host:
        return (*sides[0], *sides[1], moved, T_dev, matches)
    with phase("to_host"):
        out = tuple(t.cpu() for t in (*sides[0], *sides[1], moved)) + (gt_tform, matches.cpu())
    return out
