"""SURVEY 8(f4), the data formats in front of the hot path -- what can be built without the datasets, the MinkUNet
weights and a sparse-convolution backend:

  * the reference's pre-processed pair cache, one pickle per pair
    `<cache_data_path>/<split>/<seq:02d>/<frame0:06d>_<frame1:06d>.pickle` with the nine keys written at
    reference datasets/kitti/kitti_dataset.py:647-655 and read back by `cached_getitem` (:441-458);
  * `batch_collate_fn_dset` (:546-616), the loader output contract `evaluate.py:175-178` unpacks: the per-pair random
    dilution to `max_pc_size` points with the HOST numpy RNG (the draws come in the reference's order, so a seeded run
    consumes the same stream), the matches that survive the dilution, MinkowskiEngine's `sparse_collate` layout
    (batch index in column 0 of the coordinates);
  * the weight-file schema of reference train_coloring.py:214-222 (`evaluate.py:164` reads `['model_state_dict']`).

A cache pickle may carry two extra keys, `src_feat` / `tgt_feat` [n,32] (the feature network's output at the cached points);
the collate function then dilutes them with the same indices and appends them to its return tuple, and `python -m
umeregrobust_amd.evaluate --cache <dir>` runs the reference's loop from such a cache.  Without them, `--checkpoint W.pth`
computes the features with `umeregrobust_amd.models.ResUNetSmall2` (reference models.py:691-698) from the collate's
coordinates.

MinkowskiEngine 0.5.4 `sparse_collate` is restated from its documented behaviour (parity unpinned, like the other
third-party boundaries); everything else is pinned by golden G10 (the reference's own collate on seeded items)."""
import glob
import os
import pickle

import numpy as np
import torch

CACHE_KEYS = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")
FEATURE_KEYS = ("src_feat", "tgt_feat")


def load_pickle(filename):
    """reference utils/general_utils.py:16-19.  The cache format IS a pickle (kitti_dataset.py:647-657), and unpickling
    executes what the file says: read cache files only from a source you trust (your own preprocessing run)."""
    with open(filename, "rb") as f:
        return pickle.load(f)


def read_cached_pair(path, with_features=False):
    """One cache file -> the 9-tuple of `cached_getitem` (reference kitti_dataset.py:441-458):
    (src_pts f32[n,3], src_seg i64[n], src_coords i32[n,3], tgt_pts, tgt_seg, tgt_coords, src_pts_tform f32[n,3],
    gt_tform f32[4,4], matches i64[m,2]); with_features: + (src_feat f32[n,d], tgt_feat f32[m,d]) if the file has them."""
    d = load_pickle(path)
    missing = [k for k in CACHE_KEYS if k not in d]
    if missing:
        raise KeyError(f"{path}: not a pair cache file, keys {missing} are missing (expected {list(CACHE_KEYS)})")
    item = tuple(d[k] for k in CACHE_KEYS)
    if with_features:
        if not all(k in d for k in FEATURE_KEYS):
            raise KeyError(f"{path}: no `src_feat` / `tgt_feat`: compute the features with the feature network "
                           "(evaluate --checkpoint / cached_pairs(checkpoint=...)) or dump them into the cache files")
        item = item + tuple(d[k] for k in FEATURE_KEYS)
    return item


def write_cached_pair(path, item, src_feat=None, tgt_feat=None):
    """The writer of reference kitti_dataset.py:647-657 (same keys, same pickle protocol), plus the optional features."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    d = dict(zip(CACHE_KEYS, item[:9]))
    if src_feat is not None:
        d["src_feat"], d["tgt_feat"] = src_feat, tgt_feat
    with open(path, "wb") as handle:
        pickle.dump(d, handle, protocol=pickle.HIGHEST_PROTOCOL)


def z_rotation_matrix(deg):
    """`scipy.spatial.transform.Rotation.from_euler('z', deg, degrees=True).as_matrix()` (kitti_dataset.py:473-474) in own
    code: fp64 [[c, -s, 0], [s, c, 0], [0, 0, 1]] with c, s the cosine and sine of the angle in radians."""
    a = np.deg2rad(np.float64(deg))
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)


def rotate_rows(pts, rot):
    """`pts @ rot` (kitti_dataset.py:476-477) for pts f32 [n,3] and rot f32 [3,3] on the device of `pts`, in a stated order:
    column k = (x rot[0,k] + y rot[1,k]) + z rot[2,k], every product and sum rounded to fp32 on its own (a BLAS matmul may
    fuse or reorder them; the result differs from it in the last bit at most)."""
    x, y, z = pts[:, 0:1], pts[:, 1:2], pts[:, 2:3]
    return (x * rot[0][None, :] + y * rot[1][None, :]) + z * rot[2][None, :]


def quantize_on_device(pts, voxel_size):
    """`ME.utils.sparse_quantize(coordinates=pts, return_index=True, quantization_size=voxel_size)` (kitti_dataset.py:416-419,
    :480-487) on the device: (coords int32 [m,3] = floor(p / voxel) of the first point of every occupied voxel, inds int64 [m]
    ascending).  `ops.voxel_first_index` restates MinkowskiEngine's choice of representative (parity unpinned, as everywhere).
    The division is a true fp32 division, like the kernel's (torch turns a division by a Python number into a multiplication
    by its reciprocal on the device, which can land on the other side of a voxel boundary)."""
    from .. import ops
    inds = ops.voxel_first_index(pts.contiguous(), float(voxel_size))
    coords = torch.floor(pts[inds] / torch.tensor(float(voxel_size), dtype=torch.float32, device=pts.device)).to(torch.int32)
    return coords, inds


def _refuse_gpu_in_worker(what):
    if torch.utils.data.get_worker_info() is not None:
        raise RuntimeError(f"{what} runs on the GPU and was asked for inside a DataLoader worker process: a forked worker must "
                           "not open the GPU.  Use num_workers=0 (the item's work is a few kernel launches)")


def augmented_gt_tform(gt_tform, rot_src, rot_tgt):
    """The ground truth between the two rotated clouds, by the reference's expressions (kitti_dataset.py:492-499), on the host
    in fp32 as there: R' = (rot_src^T R^T rot_tgt)^T, t' = t rot_tgt."""
    T = torch.as_tensor(gt_tform).float()
    out = torch.zeros_like(T)
    out[:3, :3] = ((rot_src.T @ T[:3, :3].T) @ rot_tgt).T
    out[:3, 3] = T[:3, 3] @ rot_tgt
    out[3, 3] = 1
    return out


def augmented_item(item, voxel_size, rng, device, phase=None, to_host=True):
    """`cached_getitem_augmented` (kitti_dataset.py:460-509; the same in nuscenes_dataset.py:467-516) on the device: two
    rotations about z drawn as `rng.uniform(-180, 180)` (source first, then target), both clouds rotated (rotate_rows),
    re-quantised (quantize_on_device) and turned into grid points, the ground truth re-expressed in the rotated frames
    (augmented_gt_tform), and new one-side matches at voxel_size / 2.  -> the 9-tuple, on the host; with to_host=False on the device,
    where it was made (the "to_host" phase is skipped): what `collate.batch_collate_fn_dset_device` takes without a round trip.
    phase: optional `phase(name)` -> context manager entered around each part ("to_device", "thinning", "grid_points", "matches",
    "to_host"): how tools/train_step_time.py times the parts of exactly this code."""
    from contextlib import nullcontext

    from ..utils.general_utils import convert_coords_to_grid_pts, one_side_ball_query_matches
    phase = phase or (lambda name: nullcontext())
    dev = torch.device(device)
    rots = [torch.from_numpy(z_rotation_matrix(rng.uniform(low=-180, high=180))).float() for _ in ("src", "tgt")]
    sides = []
    for first, rot in ((0, rots[0]), (3, rots[1])):
        with phase("to_device"):
            pts, seg, rot_dev = torch.as_tensor(item[first]).float().to(dev), torch.as_tensor(item[first + 1]).to(dev), rot.to(dev)
        with phase("thinning"):
            pts = rotate_rows(pts, rot_dev)
            coords, inds = quantize_on_device(pts, voxel_size)
            seg = seg[inds]
        with phase("grid_points"):
            grid = convert_coords_to_grid_pts(pts, coords, voxel_size)
        sides.append((grid, seg, coords))
    gt_tform = augmented_gt_tform(torch.as_tensor(item[7]).cpu(), rots[0], rots[1])
    with phase("matches"):
        T_dev = gt_tform.to(dev)
        src_grid, tgt_grid = sides[0][0], sides[1][0]
        moved = rotate_rows(src_grid, T_dev[:3, :3].T.contiguous()) + T_dev[:3, 3]
        matches = one_side_ball_query_matches(src_grid, tgt_grid, T_dev, voxel_size / 2).long()
    if not to_host:
        return (*sides[0], *sides[1], moved, T_dev, matches)
    with phase("to_host"):
        out = tuple(t.cpu() for t in (*sides[0], *sides[1], moved)) + (gt_tform, matches.cpu())
    return out


class CachedPairDataset(torch.utils.data.Dataset):
    """The cache-backed half of the reference's SemanticKITTIDataset / NuscenesDataset (`cache_data_path != ""`,
    kitti_dataset.py:380-385): item i = the pickle of pair i.  The reference takes its pair list from the raw dataset's
    pose files; here it is the sorted content of `<cache_data_path>/<split>/*/` (or an explicit list of
    (seq_id, frame0_id, frame1_id)).

    use_augmentations: every item goes through `augmented_item` (the reference's `cached_getitem_augmented`) on `device`
    (default: the current HIP device) with angles from `rng` (default: the global numpy stream, like the reference).  The
    reference hides that work -- two KDTree builds' worth per item -- behind loader workers; here it is a few kernel launches
    in the loading process, and asking for it inside a worker raises: use num_workers=0, with which the host RNG is also
    consumed in the reference's order (item draws, then the collate's)."""

    def __init__(self, cache_data_path, split="test", files=None, with_features=False, dataset="kitti", use_augmentations=False,
                 voxel_size=0.3, device=None, rng=np.random, items_on_device=False):
        """dataset: "kitti" -- sequence ids are integers, directories `%02d` (kitti_dataset.py:444); "nuscenes" -- sequence
        ids are the directory names themselves (nuscenes_dataset.py:452).  items_on_device: an augmented item stays on the device
        (`augmented_item(..., to_host=False)`), for the device-side collate; a plain item is the cache file's either way."""
        self.cache_data_path, self.split, self.with_features, self.dataset = cache_data_path, split, with_features, dataset
        self.items_on_device = bool(items_on_device)
        self.use_augmentations, self.voxel_size, self.device, self.rng = bool(use_augmentations), voxel_size, device, rng
        if self.use_augmentations and with_features:
            raise ValueError("CachedPairDataset: cached features belong to the cached points; an augmented item has other points")
        if files is None:
            files = []
            for p in sorted(glob.glob(os.path.join(cache_data_path, split, "*", "*.pickle"))):
                seq, name = os.path.basename(os.path.dirname(p)), os.path.splitext(os.path.basename(p))[0]
                f0, f1 = name.split("_")
                files.append((int(seq) if dataset == "kitti" else seq, int(f0), int(f1)))
        self.files = list(files)

    def path(self, idx):
        seq_id, frame0_id, frame1_id = self.files[idx]
        seq_dir = seq_id if isinstance(seq_id, str) else f"{seq_id:02d}"
        return os.path.join(self.cache_data_path, self.split, seq_dir, f"{frame0_id:06d}_{frame1_id:06d}.pickle")

    def __len__(self):
        return len(self.files)

    def __getitem__(self, idx):
        item = read_cached_pair(self.path(idx), self.with_features)
        if not self.use_augmentations:
            return item
        _refuse_gpu_in_worker("CachedPairDataset(use_augmentations=True)")
        if not torch.cuda.is_available():
            raise RuntimeError("CachedPairDataset(use_augmentations=True) needs a HIP device; there is no CPU fallback")
        device = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        return augmented_item(item, self.voxel_size, self.rng, device, to_host=not self.items_on_device)


def sparse_collate(coords, feats):
    """MinkowskiEngine.utils.sparse_collate as called at reference kitti_dataset.py:593,599 (no labels): coordinates
    [n_i, D] of every batch element stacked with the batch index in a new column 0 (int32), features concatenated."""
    bcoords, bfeats = [], []
    for b, (c, f) in enumerate(zip(coords, feats)):
        c = torch.as_tensor(c)
        c = (torch.floor(c) if c.is_floating_point() else c).to(torch.int32)
        bcoords.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32), c], dim=1))
        bfeats.append(torch.as_tensor(f))
    return torch.cat(bcoords, dim=0), torch.cat(bfeats, dim=0)


class _Dilution:
    """One cloud of one batch element thinned to `size` points: the draw (`rng.choice(n, size, replace=False)`, the call the
    reference makes at kitti_dataset.py:571 / :579) and the inverse map original index -> position in the thinned cloud
    (-1: dropped), which is what the match bookkeeping below needs."""

    def __init__(self, n, size, rng):
        self.keep = rng.choice(n, size, replace=False)
        self.position = np.full(n, -1, dtype=np.int64)
        self.position[self.keep] = np.arange(size, dtype=np.int64)

    def __call__(self, *fields):
        return tuple(f[self.keep] for f in fields)


def surviving_matches(matches, src, tgt):
    """The correspondences (source index, target index) whose two end points both survive the dilutions `src` / `tgt`,
    re-indexed into the thinned clouds -- the result of the reference's two `np.intersect1d(..., return_indices=True)` calls
    (kitti_dataset.py:585-589), expressed through the inverse maps:
      * a source point keeps only its first correspondence (in file order); candidates are visited in ascending source index;
      * a target point keeps only the first of those candidates; rows come out in ascending target index."""
    matches = np.asarray(matches)
    _, first_of_src = np.unique(matches[:, 0], return_index=True)              # ascending source index, first occurrence
    rows = first_of_src[src.position[matches[first_of_src, 0]] >= 0]
    _, first_of_tgt = np.unique(matches[rows, 1], return_index=True)           # ascending target index, first candidate
    rows = rows[first_of_tgt]
    rows = rows[tgt.position[matches[rows, 1]] >= 0]
    return np.stack([src.position[matches[rows, 0]], tgt.position[matches[rows, 1]]], axis=1)


def batch_collate_fn_dset(data, num_matches, max_pc_size=100000, rng=np.random):
    """The loader output contract of reference datasets/kitti/kitti_dataset.py:546-616 (what evaluate.py:175-178 unpacks).
    data: list of items (src_pts, src_sem, src_coords, tgt_pts, tgt_sem, tgt_coords, src_pts_tform, gt_tform, matches
    [, src_feat, tgt_feat]).  Every cloud of the batch is thinned to the batch-minimum size (at most max_pc_size).  The
    host RNG is consumed in the reference's order, on the reference's (global numpy) stream by default: per element the
    source draw, then the target draw; after the loop one draw per element for the matches.
    -> (src_pts [bs,n,3], src_seg [bs,n], src_coords [bs*n,4], src_feat [bs*n,1] (ones: the network's input),
        tgt_pts, tgt_seg, tgt_coords, tgt_feat, src_pts_tform [bs,n,3], gt_tform [bs,4,4], matches [bs,k,2])
       + (src_net_feat [bs,n,d], tgt_net_feat [bs,m,d]) when the items carry features."""
    with_feat = len(data[0]) > 9
    n_src = min(min(len(d[0]) for d in data), max_pc_size)                     # :565-566
    n_tgt = min(min(len(d[3]) for d in data), max_pc_size)
    sides = {"src": [], "tgt": []}                                             # per element: (pts, seg, coords, ones[, net feature])
    moved, kept_matches = [], []
    for d in data:
        src = _Dilution(len(d[0]), n_src, rng)                                 # :571
        tgt = _Dilution(len(d[3]), n_tgt, rng)                                 # :579
        for name, dil, first, feat_at in (("src", src, 0, 9), ("tgt", tgt, 3, 10)):
            pts, seg, coords = dil(d[first], d[first + 1], d[first + 2])
            fields = (pts, seg, coords, torch.ones_like(pts[:, :1]).float())
            sides[name].append(fields + (dil(d[feat_at]) if with_feat else ()))
        moved.append(src(d[6])[0])
        kept_matches.append(surviving_matches(d[8], src, tgt))                 # :585-589

    def batched(name):
        pts, seg, coords, ones = (list(col) for col in list(zip(*sides[name]))[:4])
        coords, ones = sparse_collate(coords, ones)                            # :593, :599
        return torch.stack(pts, dim=0), torch.stack(seg, dim=0), coords, ones

    k = min(min(len(m) for m in kept_matches), num_matches)                    # :606-607
    matches = torch.stack([torch.from_numpy(m[rng.choice(len(m), k, replace=False)]) for m in kept_matches], dim=0)
    out = batched("src") + batched("tgt") + (torch.stack(moved, dim=0), torch.stack([d[7] for d in data], dim=0), matches)
    if with_feat:
        out = out + tuple(torch.stack([e[4] for e in sides[name]], dim=0) for name in ("src", "tgt"))
    return out


def checkpoint_state_dict(path_or_obj, allow_pickle=False):
    """The weight-file schema of reference train_coloring.py:214-222 as `evaluate.py:164` consumes it: a dict with
    'epoch', 'model_state_dict', 'optimizer_state_dict', 'total_loss'.  -> the model state dict (name -> tensor); raises
    with the offending keys otherwise.  (Bare state dicts, `save_model` :209-211, are accepted as they are.)
    Files are read with torch's restricted unpickler (`weights_only=True`); a checkpoint that needs the full one (arbitrary
    pickled objects = arbitrary code at load time) is refused unless `allow_pickle=True`: only for files you trust."""
    if isinstance(path_or_obj, (str, os.PathLike)):
        try:
            # tensors, containers and scalars only: nothing in the file is executed
            ck = torch.load(path_or_obj, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError:
            if not allow_pickle:
                raise
            ck = torch.load(path_or_obj, map_location="cpu", weights_only=False)     # full unpickler: trusted files only
    else:
        ck = path_or_obj
    if not isinstance(ck, dict):
        raise TypeError(f"checkpoint: expected a dict, got {type(ck).__name__}")
    if "model_state_dict" in ck:
        missing = [k for k in ("epoch", "optimizer_state_dict", "total_loss") if k not in ck]
        if missing:
            raise KeyError(f"checkpoint: keys {missing} of the save_checkpoint schema are missing")
        sd = ck["model_state_dict"]
    else:
        sd = ck
    bad = [k for k, v in sd.items() if not isinstance(v, torch.Tensor)]
    if bad or not sd:
        raise TypeError(f"checkpoint: model_state_dict must map parameter names to tensors (offending: {bad[:5]})")
    return sd
