"""numpy mirror of csrc/voxel_centroid_math.h and of ops.voxel_down_sample, for tests/test_voxel_centroid_cpu.py (which holds it against
the header itself, compiled for the host) and the GPU tests (which hold the kernels against it, bit for bit).  Nothing here needs a
device.  Cells, keys and their limits are tests/glue_cases.py's; the sums are int64, so they do not depend on the order of the points."""
import fractions

import numpy as np

from tests import glue_cases as gc

SCALE = 4294967296.0                                  # 2^32
MAX_POINTS = 1 << 20                                  # kVoxCentroidMaxPoints


def cells(p, voxel):
    """floorf(p / voxel) in fp32, any shape"""
    return gc.quotients(p, voxel)


def quanta(p, voxel):
    """-> (cell f32, q int64): q = llrint(((double)p / (double)voxel - (double)cell) * 2^32); rint rounds to nearest even, as llrint"""
    p = np.asarray(p, np.float32)
    c = cells(p, voxel)
    u = p.astype(np.float64) / np.float64(np.float32(voxel)) - c.astype(np.float64)
    return c, np.rint(u * SCALE).astype(np.int64)


def centroid(cell, total, count, voxel):
    """(float)(((double)c + (double)S / ((double)cnt * 2^32)) * (double)voxel), one rounding per operation"""
    cell, total, count = np.asarray(cell, np.float32), np.asarray(total, np.int64), np.asarray(count, np.int64)
    return ((cell.astype(np.float64) + total.astype(np.float64) / (count.astype(np.float64) * SCALE))
            * np.float64(np.float32(voxel))).astype(np.float32)


def voxel_sums(pts, voxel):
    """-> (first int64 [m] ascending, cell f32 [m,3], S int64 [m,3], count int64 [m]): row r is the voxel whose lowest point index is
    the r-th smallest"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    ok, key = gc.keys(pts, voxel)
    assert ok.all(), "a point without a key: the library raises, there is nothing to mirror"
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    row = rank[inverse.reshape(-1)]
    c, q = quanta(pts, voxel)
    S = np.zeros((len(first), 3), np.int64)
    np.add.at(S, row, q)
    count = np.bincount(row, minlength=len(first)).astype(np.int64)
    return first[order].astype(np.int64), c[first[order]], S, count


def down_sample(pts, voxel):
    """ops.voxel_down_sample(pts, voxel, return_info=True) -> (centroids f32 [m,3], first_index int64 [m], counts int32 [m])"""
    first, c, S, count = voxel_sums(pts, voxel)
    return centroid(c, S, count[:, None], voxel), first, count.astype(np.int32)


def exact_means(pts, voxel):
    """the exact mean of every voxel's f32 points, as Fractions [m][3], in down_sample's row order"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    first, _, _, count = voxel_sums(pts, voxel)
    _, key = gc.keys(pts, voxel)
    row_of_key = {int(key[i]): r for r, i in enumerate(first)}
    sums = [[fractions.Fraction(0)] * 3 for _ in first]
    for p, k in zip(pts, key):
        r = row_of_key[int(k)]
        sums[r] = [a + fractions.Fraction(float(x)) for a, x in zip(sums[r], p)]
    return [[a / int(n) for a in s] for s, n in zip(sums, count)]


# ---- clouds of the CPU and GPU tests ------------------------------------------------------------------------------------------------

def dense_cloud(n, per_voxel=4, voxel=0.3, seed=0):
    """n points with about `per_voxel` points in every occupied voxel, in random order"""
    rng = np.random.RandomState(seed + n)
    side = max(1, int(round((n / per_voxel) ** (1.0 / 3.0))))
    return (rng.uniform(-0.5 * side, 0.5 * side, (n, 3)) * voxel).astype(np.float32)


def one_voxel_cloud(n, voxel=0.3, cell=(3, -2, 5), seed=1):
    """n points strictly inside one voxel: the worst contention"""
    rng = np.random.RandomState(seed)
    pts = ((np.array(cell) + rng.uniform(0.05, 0.95, (n, 3))) * voxel).astype(np.float32)
    assert (cells(pts, voxel) == np.float32(cell)).all()
    return pts


def far_cloud(n=2000, voxel=0.3, seed=2):
    """a cloud at coordinates ~1e5: cells ~3.3e5, where an f32 ulp is 1/128 and the quotient's rounding reaches a few per cent of a cell"""
    rng = np.random.RandomState(seed)
    return (np.array([1e5, -1e5, 9e4]) + rng.uniform(-2.0, 2.0, (n, 3))).astype(np.float32)


def boundary_cloud(voxel):
    """p = fl32(k v) for k in -3 .. 3 on every axis in turn (the other two mid-cell), every point twice"""
    rows = []
    for axis in range(3):
        for k in range(-3, 4):
            p = [0.5 * voxel] * 3
            p[axis] = k * float(np.float32(voxel))
            rows.append(p)
    return np.array(rows + rows, np.float32)


def near_boundary_cloud(voxel, axis, k=64):
    """glue_cases.sweep_cloud's points for |k| <= 64: fl32(k v), its successor and its predecessor, quotients within an ulp of a boundary"""
    pts = gc.sweep_cloud(voxel, axis)
    return pts[np.abs(pts[:, axis]) <= (k + 0.5) * voxel]
