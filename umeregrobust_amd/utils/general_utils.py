"""Config plumbing with the reference's key names (reference utils/general_utils.py:62-69), and the trainer's data-side
helpers of the same file (:27-59): grid points from voxel coordinates, and the ground-truth matches of a pair, which the
reference takes from a scipy KDTree and this library from the HIP search of `gt_matches` (csrc/gt_match.hip)."""
import os

import numpy as np
import torch
import yaml

CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "benchmarks")

# reference evaluate.py:118-124
BENCHMARK_CONFIGS = {
    "kitti_test": "test_kitti_config.yaml",
    "lokitti": "lokitti_config.yaml",
    "rotkitti": "rotkitti_config.yaml",
    "nuscenes_test": "test_nuscenes_config.yaml",
    "lonuscenes": "lonuscenes_config.yaml",
    "rotnuscenes": "rotnuscenes_config.yaml",
}


def update_namespace_from_yaml(args, yaml_path):
    """Flat YAML -> attributes on an argparse.Namespace-like object (same behaviour as the reference)."""
    with open(yaml_path, "r") as f:
        data = yaml.safe_load(f)
    for key, value in data.items():
        setattr(args, key, value)
    return args


def benchmark_config_path(benchmark):
    return os.path.join(CONFIG_DIR, BENCHMARK_CONFIGS[benchmark])


def convert_coords_to_grid_pts(pts, coords, ds):
    """reference utils/general_utils.py:27-35 in plain torch, on whatever device the inputs are, with the same operations in the
    same order, so the values are the reference's: per axis, the affine map that sends the smallest voxel index to
    `pts.min + ds / 2` and the largest to `pts.max - ds / 2`, applied to the integer voxel coordinates.
    pts f32 [n,3] (the whole cloud), coords int [m,3] -> f32 [m,3].
    An axis on which all points share one voxel divides 0 by 0 (NaN), as in the reference."""
    half = 0.5 * ds
    hi, lo = pts.max(dim=0).values - half, pts.min(dim=0).values + half            # centres of the outermost voxels, per axis
    k_hi, k_lo = coords.max(dim=0).values, coords.min(dim=0).values
    span = k_hi - k_lo
    scale = (hi - lo) / span
    offset = (k_hi * lo - hi * k_lo) / span
    return (coords * scale + offset).float()


def _match_inputs(src_pts, tgt_pts):
    """-> (src, tgt on the GPU, on_host): host inputs (numpy arrays, CPU tensors) are copied to the current HIP device --
    the search itself has no host form -- and the result then goes back to the host as a numpy array, the reference's type."""
    on_host = not (isinstance(src_pts, torch.Tensor) and src_pts.device.type == "cuda")
    if on_host and not torch.cuda.is_available():
        raise RuntimeError("ball-query matches run on the GPU (csrc/gt_match.hip); there is no HIP device and no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if on_host else src_pts.device
    to = lambda p: torch.as_tensor(p).to(device=dev, dtype=torch.float32)
    return to(src_pts), to(tgt_pts), on_host


def one_side_ball_query_matches(src_pts, tgt_pts, trans, search_voxel_size):
    """reference utils/general_utils.py:38-44 on the GPU: rows (i, j) int64 [m,2], i ascending, j the nearest target of
    `trans` applied to source point i, kept where the distance is below `search_voxel_size`.

    Where the reference is a torch matmul followed by scipy's KDTree, the arithmetic here is fixed (include/umereg_gt_matches.h):
    the query in fp32 as ((x R[:,0] + y R[:,1]) + z R[:,2]) + t, the squared distance in fp64, the lower index on an exact tie,
    kept iff d^2 < r^2.  The two differ only on points within rounding (~1e-5 m) of the radius or of a tie.
    Device tensors in -> a device tensor out (one device -> host read, for the row count); host inputs -> a numpy array."""
    from .. import gt_matches
    src, tgt, on_host = _match_inputs(src_pts, tgt_pts)
    rows = gt_matches.one_side(src, tgt, trans, float(search_voxel_size))
    return rows.cpu().numpy() if on_host else rows


def mutual_ball_query_matches(src_pts, tgt_pts, tform, voxel_size):
    """reference utils/general_utils.py:47-59 on the GPU: the one-side matches (i, j) of source -> target under `tform` for which
    the one-side matches of target -> source under `torch.linalg.inv(tform)` (formed here as there) hold (j, i); order as
    source -> target.  The reference's O(n^2) Python loop is one kernel.
    DIFFERENCE: without any match the result is [0,2]; the reference's `np.array([])` has shape (0,) there (while its one-side
    function returns (0,2))."""
    from .. import gt_matches
    src, tgt, on_host = _match_inputs(src_pts, tgt_pts)
    tform = torch.as_tensor(tform).float()
    rows = gt_matches.mutual(src, tgt, tform, torch.linalg.inv(tform), float(voxel_size))
    return rows.cpu().numpy() if on_host else rows
