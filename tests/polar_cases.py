"""Constructed inputs with a prescribed, graded cross-moment spectrum, shared by tests/test_polar_cpu.py (no GPU: the routine itself, and
that these inputs qualify for the bars) and tests/test_polar_gpu.py (the two kernels that call it).  Test infrastructure only."""
import itertools

import numpy as np

R2 = [1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7]          # s2 / s1
R3 = [1.0, 0.5, 1e-1, 1e-3, 0.0]                              # s3 / s2
CELLS = list(itertools.product(R2, R3, (1, -1)))              # 80 cells


def rot(rng):
    """a random proper rotation"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def compose(U, sig, V, det=1):
    return (U * (np.asarray(sig, np.float64) * [1.0, 1.0, float(det)])) @ V.T


def ladder_cell(r2, r3, det, seed=0, n=50):
    """n matrices U diag(1, r2, det * r2 * r3) V^T"""
    rng = np.random.RandomState([seed, R2.index(r2), R3.index(r3), (det + 1) // 2])
    return np.stack([compose(rot(rng), [1.0, r2, r2 * r3], rot(rng), det) for _ in range(n)])


# ------------------------------------------------------------------------------------------------ RTUME
# One lane pattern per singular pair: rows 8k .. 8k+7 of the 32 carry +-w_j times row k of a 3x3 factor, rows 24 .. 31 are zero, and
# mg = mh = const.  Every entry of g, h is then ONE product of an fp32 number and a power of two (no sum that could round away a
# row of size 1e-7 next to a row of size 1), each column sums to zero against mg exactly, and
#     left^T right = sum_k |w|^2 (s_k u~_k) v~_k^T        with u~_k, v~_k the fp32 roundings of u_k, v_k:
# the prescribed spectrum to 1e-7 RELATIVE in each singular value, which an fp32 rounding of a dense X diag(s) U^T cannot give.
_W = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0])  # sums to zero; |w|^2 = 42.5


def rtume_ladder(n, family="plain", seed=0, order=None):
    """-> G, H f32 [n,32,4], cell int [n] (index into CELLS).  Hypothesis i belongs to cell order[i % len(order)].
    family "plain": wlc = wrc = 0, t = 0.  family "shift": multiples of mg added to g and h (wlc, wrc != 0, |t| up to 145); the
    structured part is scaled by 2^12 so that the cancellation in g - wlc mg leaves the ladder intact down to s2/s1 = 1e-7."""
    rng = np.random.RandomState([seed, 77, 0 if family == "plain" else 1])
    order = list(range(len(CELLS))) if order is None else list(order)
    G = np.zeros((n, 32, 4), np.float64)
    H = np.zeros((n, 32, 4), np.float64)
    cell = np.empty(n, np.int64)
    c = 1.0 if family == "plain" else 4096.0
    for i in range(n):
        cell[i] = order[i % len(order)]
        r2, r3, det = CELLS[cell[i]]
        U, V = rot(rng), rot(rng)
        sig = np.array([1.0, r2, r2 * r3 * det])
        m = rng.uniform(0.5, 1.5)
        G[i, :, 0] = m
        H[i, :, 0] = m
        for k in range(3):
            # A = left^T right = sum_k |w|^2 c^2 sig_k U[:, k] V[:, k]^T
            G[i, 8 * k:8 * k + 8, 1:] = c * np.outer(_W, (sig[k] * U[:, k]).astype(np.float32))
            H[i, 8 * k:8 * k + 8, 1:] = c * np.outer(_W, V[:, k].astype(np.float32))
        if family != "plain":
            mag = [0.3, 5.0, 40.0, 145.0][i % 4]
            tg, th = rng.normal(size=3), rng.normal(size=3)
            G[i, :, 1:] += m * (mag * rng.uniform(0.2, 0.5)) * tg / np.linalg.norm(tg)
            H[i, :, 1:] += m * (mag * rng.uniform(0.2, 0.5)) * th / np.linalg.norm(th)
    return G.astype(np.float32), H.astype(np.float32), cell


# ------------------------------------------------------------------------------------------------ ICP
def icp_thin_case(kind, w=1.0, seed=0, n_tgt=400, n_src=300):
    """A target that is thin in two directions (a 20 m segment with transverse scatter +-w), planar (exact z = const) or exactly
    collinear, in fp32 with 5 cm or more between neighbours; the source is a subset moved by far less than that, so the
    nearest neighbours are the identity pairing.  -> src f32 [n_src,3], tgt f32 [n_tgt,3], T_init [4,4], max_dist."""
    rng = np.random.RandomState([seed, 55, {"segment": 0, "planar": 1, "collinear": 2}[kind], int(round(w * 1e4))])
    q = 2.0 ** -12                                                      # transverse lattice
    along = (np.arange(n_tgt) - n_tgt / 2) * 0.05
    if kind == "segment":
        p = np.stack([along, np.round(rng.uniform(-w, w, n_tgt) / q) * q, np.round(rng.uniform(-w, w, n_tgt) / q) * q], axis=1)
        D = rot(rng)                                                    # a generic direction, a centroid off the origin
        tgt = (p @ D.T + [3.0, -2.0, 1.0]).astype(np.float32)
    elif kind == "planar":
        side = int(np.sqrt(n_tgt))
        gx, gy = np.meshgrid(np.arange(side) * 0.25, np.arange(side) * 0.25, indexing="ij")
        tgt = np.stack([gx.ravel() - 2.0, gy.ravel() + 1.0, np.full(side * side, 1.5)], axis=1).astype(np.float32)
    else:
        k = (np.arange(n_tgt) - n_tgt // 2) * 0.0625
        tgt = np.stack([k + 3.0, k - 2.0, np.full(n_tgt, 0.5)], axis=1).astype(np.float32)      # along (1, 1, 0): exact in fp32
    n_tgt = tgt.shape[0]
    pick = np.sort(rng.choice(n_tgt, min(n_src, n_tgt), replace=False))
    if kind == "collinear":
        src = (tgt[pick] + np.float32(2.0 ** -8) * np.array([1, 1, 0], np.float32)).astype(np.float32)   # a slide along the line: still exact
        return src, tgt, np.eye(4), 0.02
    if kind == "planar":
        a = 4e-4
        Rm = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])         # in-plane motion: source planar too
        src = tgt[pick].astype(np.float64) @ Rm.T + [2e-3, -3e-3, 0.0]
        src[:, 2] = 1.5
        return src.astype(np.float32), tgt, np.eye(4), 0.05
    v = rng.normal(size=3)
    v *= 3e-4 / np.linalg.norm(v)                                       # 0.3 mrad about a generic axis: 3 mm at the segment's ends
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    Rm = np.eye(3) + K + K @ K / 2
    Rm = np.linalg.qr(Rm)[0] * np.sign(np.diag(np.linalg.qr(Rm)[1]))
    src = (tgt[pick].astype(np.float64) - tgt.mean(0)) @ Rm.T + tgt.mean(0) + rng.uniform(-3e-3, 3e-3, 3)
    return src.astype(np.float32), tgt, np.eye(4), 0.02
