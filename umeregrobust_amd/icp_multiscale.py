"""Voxel-centroid downsampling and coarse-to-fine ICP: open3d's `voxel_down_sample` and `multi_scale_icp` (names as recalled).

    small = ops.voxel_down_sample(pts, 0.4)                                       # one centroid per occupied voxel, f32 [m,3]
    small, first_index, counts = ops.voxel_down_sample(pts, 0.4, return_info=True)
    levels = ops.voxel_pyramid(src, tgt, (0.8, 0.4, 0))                           # [(src_k, tgt_k)], one host read for all counts
    reg = ops.icp_multi_scale(src, tgt, T_init, (0.8, 0.4, 0), (1.6, 0.8, 0.2), (30, 30, 30), estimation="point_to_plane")
    python -m umeregrobust_amd.evaluate --icp-voxel-sizes 0.8,0.4,0 [--icp-level-distances 1.6,0.8,0.2] [--icp-level-iterations 30,30,30]

A single-scale ICP converges only from within its correspondence distance, and every one of its iterations runs on the full clouds.
Coarse levels widen the basin and run on an order of magnitude fewer points; the full clouds get the last few updates.

`voxel_down_sample`: the voxel of a point is floorf(p / voxel) per axis, the key and table of `voxel_first_index`, and rows come in
the order `voxel_first_index` returns (by every voxel's lowest point index).  The centroid is an integer sum, so the outputs are the
same bits from run to run (csrc/voxel_centroid_api.h, csrc/voxel_centroid_math.h).  Two deviations from open3d: the
grid is anchored at the origin (open3d: the cloud's minimum bound), so two clouds share it; rows are in first-point order (open3d:
hash order).  At most 2^20 points: up to there the 64-bit sums are exact in fp64.

`icp_multi_scale` builds the pyramid once, then per level re-estimates normals where the estimation needs them (the library's normals
carry a canonical sign, so a per-voxel mean could cancel: they are not averaged) and makes the EXISTING synchronous call with that
level's distance and iteration limit; the fp64 transformation of level k is the host T_init of level k + 1.  One host wait per level.

`levels_of(args)` reads `args.icp_voxel_sizes`, `args.icp_level_distances`, `args.icp_level_iterations` (None when unset: every path
is then what it was).  Defaults when only the voxel sizes are given: distance = max(2 * voxel, icp_max_correspondence_distance), on
a level of voxel size 0 icp_max_correspondence_distance, and icp_max_iteration on every level.  These are choices, not tuned on real
scans.

The entries are declared in csrc/voxel_centroid_api.h, a private header: VOXEL_CENTROID_SIGNATURES is their table, typed by
`load_native` through `_lib.load_typed`."""
import ctypes
import math
import numbers
from types import SimpleNamespace

import torch

from . import _lib, icp_gicp, icp_plane

c_void_p, c_int, c_float, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

VOXEL_CENTROID_SIGNATURES = {
    "umereg_voxel_centroid_workspace_bytes": (c_size_t, [c_int]),
    "umereg_voxel_centroid_f32": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

MAX_POINTS = 1 << 20            # UMEREG_VOXEL_CENTROID_MAX_POINTS: |q| <= 2^32 per point, so |S| <= 2^52 and (double)S is exact
MAX_LEVELS = 8
BAD_COORDINATE = "voxel_first_index: a coordinate is NaN, infinite or beyond 2^20 voxels from the origin"


def load_native():
    """the library with the voxel-centroid entries typed"""
    return _lib.load_typed(VOXEL_CENTROID_SIGNATURES)


# ---- argument rules (no tensor and no library touched) ------------------------------------------------------------------------------

def _number(x):
    return not isinstance(x, bool) and isinstance(x, numbers.Real) and math.isfinite(float(x))


def check_voxel_size(who, voxel_size):
    """a positive, finite number whose f32 value is positive and finite too"""
    if not _number(voxel_size) or not 0.0 < c_float(float(voxel_size)).value < math.inf:
        raise ValueError(f"{who}: voxel_size must be a positive finite number, got {voxel_size!r}")
    return float(voxel_size)


def _sequence(who, name, values):
    if isinstance(values, (str, bytes)) or not hasattr(values, "__len__") or not hasattr(values, "__iter__"):
        raise ValueError(f"{who}: {name} must be a sequence of 1 to {MAX_LEVELS} numbers, got {values!r}")
    values = list(values)
    if not 1 <= len(values) <= MAX_LEVELS:
        raise ValueError(f"{who}: {name} must have 1 to {MAX_LEVELS} entries, got {len(values)}")
    return values


def check_voxel_sizes(who, voxel_sizes):
    """positive and strictly decreasing; the last may be 0 or negative (stored as 0.0): the clouds as given.  -> list of floats"""
    sizes = _sequence(who, "voxel_sizes", voxel_sizes)
    out = []
    for k, v in enumerate(sizes):
        if not _number(v):
            raise ValueError(f"{who}: voxel_sizes[{k}] must be a finite number, got {v!r}")
        if k == len(sizes) - 1 and float(v) <= 0.0:
            out.append(0.0)
            continue
        out.append(check_voxel_size(f"{who}: voxel_sizes[{k}]", v))
        if k and not out[k] < out[k - 1]:
            raise ValueError(f"{who}: voxel_sizes must be strictly decreasing, got {sizes!r}")
    return out


def check_levels(who, voxel_sizes, max_correspondence_distances, max_iterations):
    """the three lists of a coarse-to-fine run -> [(voxel_size, max_correspondence_distance, max_iteration)]"""
    sizes = check_voxel_sizes(who, voxel_sizes)
    dists = _sequence(who, "max_correspondence_distances", max_correspondence_distances)
    iters = _sequence(who, "max_iterations", max_iterations)
    if not len(sizes) == len(dists) == len(iters):
        raise ValueError(f"{who}: voxel_sizes, max_correspondence_distances and max_iterations must have one entry per level, got "
                         f"{len(sizes)}, {len(dists)} and {len(iters)}")
    for k, d in enumerate(dists):
        if not _number(d) or not float(d) > 0.0:
            raise ValueError(f"{who}: max_correspondence_distances[{k}] must be a positive finite number, got {d!r}")
    for k, i in enumerate(iters):
        if isinstance(i, bool) or not isinstance(i, numbers.Real) or int(i) != i or int(i) < 0:
            raise ValueError(f"{who}: max_iterations[{k}] must be a non-negative integer, got {i!r}")
    return [(v, float(d), int(i)) for v, d, i in zip(sizes, dists, iters)]


def levels_of(args):
    """the levels a refinement site reads from its `args`, or None when args.icp_voxel_sizes is unset (single scale, as ever).
    Defaults -- choices, not tuned on real scans: distance = max(2 * voxel, args.icp_max_correspondence_distance), on a level of
    voxel size 0 args.icp_max_correspondence_distance (0.2); args.icp_max_iteration (200) on every level."""
    sizes = getattr(args, "icp_voxel_sizes", None)
    if sizes is None:
        for name in ("icp_level_distances", "icp_level_iterations"):
            if getattr(args, name, None) is not None:
                raise ValueError(f"icp: args.{name} is set without args.icp_voxel_sizes")
        return None
    sizes = check_voxel_sizes("icp", sizes)
    base = float(getattr(args, "icp_max_correspondence_distance", 0.2))
    dists = getattr(args, "icp_level_distances", None)
    iters = getattr(args, "icp_level_iterations", None)
    if dists is None:
        dists = [max(2.0 * v, base) if v > 0.0 else base for v in sizes]
    if iters is None:
        iters = [int(getattr(args, "icp_max_iteration", 200))] * len(sizes)
    return check_levels("icp", sizes, dists, iters)


def parse_list(text, kind=float):
    """"0.8,0.4,0" -> [0.8, 0.4, 0.0]: the command line's form of a per-level list"""
    return [kind(t) for t in str(text).split(",") if t.strip()]


# ---- downsampling -------------------------------------------------------------------------------------------------------------------

def _cloud(who, pts, name="pts"):
    if not isinstance(pts, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(pts).__name__}")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be [n,3], got {tuple(pts.shape)}")
    if not 1 <= pts.shape[0] <= MAX_POINTS:
        raise ValueError(f"{who}: {name} must have 1 to 2^20 points (the 64-bit sums are exact in fp64 up to there), got {pts.shape[0]}")
    if pts.device.type != "cuda":
        raise RuntimeError(f"{who}: {name} on the CPU; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
    return pts.to(torch.float32).contiguous()


def _launch(p, voxel, cnt):
    """enqueue the native call for a checked cloud -> (centroids [n,3], first_index [n], counts [n]), written up to the count in cnt[0]"""
    from . import ops
    lib = load_native()
    n, dev = p.shape[0], p.device
    centroids = torch.empty(n, 3, dtype=torch.float32, device=dev)
    first = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    ws = ops._workspace(dev, lib.umereg_voxel_centroid_workspace_bytes(n), "voxel_centroid")
    _lib.call(dev, lib.umereg_voxel_centroid_f32, p.data_ptr(), n, voxel, centroids.data_ptr(), first.data_ptr(), counts.data_ptr(),
              cnt.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    return centroids, first, counts


def voxel_down_sample(pts, voxel_size, return_info=False):
    """One centroid per occupied voxel of edge `voxel_size` (open3d's voxel_down_sample): pts [n,3] f32 on the device, n <= 2^20 ->
    f32 [m,3]; with return_info: (centroids, first_index int64 [m], counts int32 [m]).  Rows are in the order of
    `voxel_first_index` (first_index is its output); the grid is anchored at the origin.  Equal inputs give equal bits.  One device ->
    host read (the number of voxels).  A NaN, infinite or out-of-range coordinate: voxel_first_index's ValueError."""
    who = "voxel_down_sample"
    voxel = check_voxel_size(who, voxel_size)
    p = _cloud(who, pts)
    cnt = torch.empty(2, dtype=torch.int32, device=p.device)
    centroids, first, counts = _launch(p, voxel, cnt)
    m, bad = cnt.tolist()                         # the one device -> host read
    if bad:
        raise ValueError(BAD_COORDINATE)
    return (centroids[:m], first[:m], counts[:m]) if return_info else centroids[:m]


def voxel_pyramid(src_pts, tgt_pts, voxel_sizes):
    """The levels of both clouds, [(src_k f32 [m_k,3], tgt_k f32 [m'_k,3])] for k over `voxel_sizes` (positive, strictly decreasing,
    the last may be 0: the clouds as given), each equal to `voxel_down_sample` of that cloud; enqueued on the current stream behind
    ONE host read of all counts."""
    who = "voxel_pyramid"
    sizes = check_voxel_sizes(who, voxel_sizes)
    s, t = _cloud(who, src_pts, "src_pts"), _cloud(who, tgt_pts, "tgt_pts")
    if s.device != t.device:
        raise ValueError(f"{who}: src_pts and tgt_pts must be on one device")
    coarse = [v for v in sizes if v > 0.0]
    out = []
    if coarse:
        cnt = torch.empty(len(coarse), 2, 2, dtype=torch.int32, device=s.device)
        rows = [(_launch(s, v, cnt[k, 0])[0], _launch(t, v, cnt[k, 1])[0]) for k, v in enumerate(coarse)]
        host = cnt.tolist()                       # the one device -> host read
        if any(c[1] for level in host for c in level):
            raise ValueError(BAD_COORDINATE)
        out = [(a[:host[k][0][0]], b[:host[k][1][0]]) for k, (a, b) in enumerate(rows)]
    if len(coarse) < len(sizes):
        out.append((s, t))
    return out


# ---- coarse to fine -----------------------------------------------------------------------------------------------------------------

def icp_multi_scale(src_pts, tgt_pts, T_init, voxel_sizes, max_correspondence_distances, max_iterations, estimation="point_to_point",
                    normal_knn=icp_plane.DEFAULT_KNN, normal_radius=None, epsilon=icp_gicp.DEFAULT_EPSILON, relative_fitness=1e-6,
                    relative_rmse=1e-6):
    """Coarse-to-fine ICP (open3d's multi_scale_icp): per level k both clouds downsampled to voxel_sizes[k] centroids (0: as given),
    normals re-estimated on them where `estimation` needs them, then ops.icp_point_to_point / icp_point_to_plane / icp_plane_to_plane
    with max_correspondence_distances[k] and max_iterations[k], started from the fp64 transformation of level k - 1 (level 0: T_init,
    as those calls take it, a device f32 tensor included).  The three lists have equal length, 1 to 8; voxel sizes are positive and
    strictly decreasing, the last may be 0.  -> SimpleNamespace(transformation, fitness, inlier_rmse (the last level's), iterations
    (summed), levels: per level voxel_size, max_correspondence_distance, n_src, n_tgt, fitness, inlier_rmse, iterations,
    transformation).  One host wait per level on top of the pyramid's one.  A single level of voxel size 0 is the plain call."""
    who = "icp_multi_scale"
    levels = check_levels(who, voxel_sizes, max_correspondence_distances, max_iterations)
    estimation = icp_plane.check_estimation(who, estimation)
    if estimation != "point_to_point":
        normal_knn = icp_plane.check_knn(who, normal_knn)
        if normal_radius is not None and not float(normal_radius) > 0.0:
            raise ValueError(f"{who}: normal_radius must be positive or None, got {normal_radius!r}")
    if estimation == icp_gicp.ESTIMATION:
        epsilon = icp_gicp.check_epsilon(who, epsilon)
    from . import ops
    if len(levels) == 1 and levels[0][0] == 0.0:
        clouds = [(src_pts, tgt_pts)]             # the plain call: nothing is downsampled, the clouds go in as given
    else:
        clouds = voxel_pyramid(src_pts, tgt_pts, [v for v, _, _ in levels])
    T, done = T_init, []
    for (voxel, dist, iters), (s, t) in zip(levels, clouds):
        if estimation == "point_to_plane":
            reg = ops.icp_point_to_plane(s, t, ops.estimate_normals(t, normal_knn, normal_radius), T, dist, iters, relative_fitness,
                                         relative_rmse)
        elif estimation == icp_gicp.ESTIMATION:
            reg = ops.icp_plane_to_plane(s, t, ops.estimate_normals(s, normal_knn, normal_radius),
                                         ops.estimate_normals(t, normal_knn, normal_radius), T, dist, iters, relative_fitness,
                                         relative_rmse, epsilon)
        else:
            reg = ops.icp_point_to_point(s, t, T, dist, iters, relative_fitness, relative_rmse)
        T = reg.transformation                    # fp64, on the host: the next level's start, unrounded
        done.append(SimpleNamespace(voxel_size=voxel, max_correspondence_distance=dist, n_src=int(s.shape[0]), n_tgt=int(t.shape[0]),
                                    fitness=reg.fitness, inlier_rmse=reg.inlier_rmse, iterations=reg.iterations,
                                    transformation=reg.transformation))
    return SimpleNamespace(transformation=done[-1].transformation, fitness=done[-1].fitness, inlier_rmse=done[-1].inlier_rmse,
                           iterations=sum(lv.iterations for lv in done), levels=done)
