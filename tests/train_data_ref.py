"""numpy restatement of the ground-truth match semantics of include/umereg_gt_matches.h (brute force, fp64), shared by the
CPU and GPU tests of the trainer's data side; and the margins under which the reference's KDTree results may differ from it.

    query     q_i = ((x R[:,0] + y R[:,1]) + z R[:,2]) + t in fp32 (numpy float32 arithmetic rounds every operation)
    distance  d2 = dx*dx + dy*dy + dz*dz, left to right, fp64 on the widened fp32 values
    match     the lowest j of minimal d2, kept iff d2 < r*r (r a double)
"""
import numpy as np


def transform_f32(pts, T):
    """The kernel's query: fp32, ((x R[:,0] + y R[:,1]) + z R[:,2]) + t; T None: the points as given."""
    p = np.ascontiguousarray(pts, dtype=np.float32)
    if T is None:
        return p
    T = np.asarray(T, dtype=np.float32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    R, t = T[:3, :3], T[:3, 3]
    return ((x * R[None, :, 0] + y * R[None, :, 1]) + z * R[None, :, 2]) + t[None, :]


def nearest(q, tgt, chunk=512):
    """-> (j* int64 [n], d2 f64 [n], gap f64 [n]): lowest index of minimal d2, that d2, and the distance (not squared) from the
    nearest to the second nearest target (inf with one target)."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    t = np.asarray(tgt, dtype=np.float32).astype(np.float64)
    n = q.shape[0]
    js, d2s, gaps = np.empty(n, np.int64), np.empty(n), np.empty(n)
    for a in range(0, n, chunk):
        d = q[a:a + chunk, None, :] - t[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = d2.argmin(axis=1)                                  # (numpy: the first occurrence of the minimum)
        rows = np.arange(d2.shape[0])
        best = d2[rows, j]
        js[a:a + chunk], d2s[a:a + chunk] = j, best
        if t.shape[0] > 1:
            d2[rows, j] = np.inf
            gaps[a:a + chunk] = np.sqrt(d2.min(axis=1)) - np.sqrt(best)
        else:
            gaps[a:a + chunk] = np.inf
    return js, d2s, gaps


def one_side(src, tgt, T, radius):
    """int64 [m,2] rows (i, j*), i ascending."""
    j, d2, _ = nearest(transform_f32(src, T), tgt)
    keep = d2 < float(radius) * float(radius)
    return np.stack([np.flatnonzero(keep), j[keep]], axis=1).astype(np.int64).reshape(-1, 2)


def mutual(src, tgt, T, T_inv, radius):
    """The one-side rows (i, j) of src -> tgt under T that tgt -> src under T_inv holds as (j, i); [0,2] when empty."""
    st, ts = one_side(src, tgt, T, radius), one_side(tgt, src, T_inv, radius)
    back = np.full(np.asarray(tgt).shape[0], -1, np.int64)
    back[ts[:, 0]] = ts[:, 1]
    return st[back[st[:, 1]] == st[:, 0]].reshape(-1, 2)


def decided(src, tgt, T, radius, margin=1e-4):
    """bool [n]: the source points whose match does not hang on the last bits of the transform -- |d_min - r| and the gap to
    the second nearest target both exceed `margin` metres (fp64).  The reference transforms with a torch matmul, whose fp32
    rounding at <= 50 m is ~1e-5 m; 1e-4 is ten times that."""
    _, d2, gap = nearest(transform_f32(src, T), tgt)
    return (np.abs(np.sqrt(d2) - float(radius)) > margin) & (gap > margin)


def rows_on(rows, mask):
    """The rows whose source index is in the mask."""
    rows = np.asarray(rows).reshape(-1, 2)
    return rows[mask[rows[:, 0]]]


def z_rotation(deg):
    """scipy's Rotation.from_euler('z', deg, degrees=True).as_matrix() in own code (fp64): [[c,-s,0],[s,c,0],[0,0,1]]."""
    a = np.deg2rad(np.float64(deg))
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
