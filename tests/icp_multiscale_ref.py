"""The case, the levels and the per-level restatements of tests/test_icp_multiscale_cpu.py and tests/test_icp_multiscale_gpu.py: the
corner of tests/icp_plane_ref.py from a start half a metre off, three levels of voxel centroids (tests/voxel_centroid_ref.py), and
coarse-to-fine runs of the three fp64 restatements (oracle.icp_point_to_point, icp_plane_ref.icp_point_to_plane,
icp_gicp_ref.icp_plane_to_plane).  Nothing here needs a device; everything expensive is computed once per process."""
import functools

import numpy as np

import icp_gicp_ref as gicp
import icp_plane_ref as plane
from oracle import oracle as orc
from tests import voxel_centroid_ref as vc

N, SEED = 3000, 3
START = (0.05, -0.04, 0.06, 0.5, -0.4, 0.45)          # rad, rad, rad, m, m, m: 0.78 m from the truth
VOXEL_SIZES = (0.8, 0.4, 0.0)
DISTANCES = (1.6, 0.8, 0.2)
ITERATIONS = (60, 60, 60)
SINGLE_DISTANCE, SINGLE_ITERATIONS = 0.2, 200
ESTIMATIONS = ("point_to_point", "point_to_plane", "plane_to_plane")
KNN = 30


@functools.lru_cache(maxsize=None)
def case(seed=SEED):
    """(src f32 [N,3], tgt f32 [N,3], gt [4,4], T0 [4,4] = the truth off by START)"""
    src, tgt, gt, _ = plane.corner_case(N, seed)
    return src, tgt, gt, plane.euler_update(np.array(START)) @ gt


@functools.lru_cache(maxsize=None)
def pyramid(seed=SEED):
    """[(src_k, tgt_k)] of the mirror, level by level (voxel size 0: the clouds as given)"""
    src, tgt, _, _ = case(seed)
    return [(vc.down_sample(src, v)[0], vc.down_sample(tgt, v)[0]) if v > 0 else (src, tgt) for v in VOXEL_SIZES]


@functools.lru_cache(maxsize=None)
def level_normals(level, seed=SEED):
    """(src normals, tgt normals) f32 of a level's clouds, from the fp64 restatement"""
    s, t = pyramid(seed)[level]
    return plane.normals_ref(s, KNN)[0].astype(np.float32), plane.normals_ref(t, KNN)[0].astype(np.float32)


def run_level(estimation, level, T_init, seed=SEED, conds=None, trace=None, max_dist=None, max_iteration=None):
    """one level of the restatement from T_init -> (T, fitness, rmse, iterations)"""
    s, t = pyramid(seed)[level]
    d = DISTANCES[level] if max_dist is None else max_dist
    it = ITERATIONS[level] if max_iteration is None else max_iteration
    if estimation == "point_to_point":
        return orc.icp_point_to_point(s, t, T_init, d, it, trace=trace)
    ns, nt = level_normals(level, seed)
    if estimation == "point_to_plane":
        return plane.icp_point_to_plane(s, t, nt, T_init, d, it, conds=conds, trace=trace)
    return gicp.icp_plane_to_plane(s, t, ns, nt, T_init, d, it, conds=conds, trace=trace)


@functools.lru_cache(maxsize=None)
def coarse_to_fine(estimation, seed=SEED):
    """the restatement's own chain -> [(T, fitness, rmse, iterations, trace, conds)] per level"""
    T, out = case(seed)[3], []
    for k in range(len(VOXEL_SIZES)):
        trace, conds = [], []
        res = run_level(estimation, k, T, seed, conds=conds, trace=trace)
        out.append(res + (trace, conds))
        T = res[0]
    return out


@functools.lru_cache(maxsize=None)
def single_scale(seed=SEED):
    """point to point at 0.2 m on the full clouds from the same start"""
    src, tgt, _, T0 = case(seed)
    return orc.icp_point_to_point(src, tgt, T0, SINGLE_DISTANCE, SINGLE_ITERATIONS)
