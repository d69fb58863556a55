"""fp64 restatement of the point-to-plane refinement (include/umereg_icp_plane.h), for tests/test_icp_plane_cpu.py and
tests/test_icp_plane_gpu.py: normals from numpy's `eigh`, the open3d ICP loop with a thresholded `eigh` solve of the 6x6 normal
equations.  Correspondences and neighbour lists come from the oracle (oracle.icp_evaluate, oracle.knn_points), which already mirror
the device's fp32 distance and its tie rule (lower index)."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_TOL = 1e-12            # kPlaneRankTol of csrc/icp_plane_math.h
GAP_MIN = 0.1               # normals are judged where (l1 - l0) / l2 >= GAP_MIN
GAP_EXCLUDED_MAX = 0.02     # and at most this share of a cloud may fall below it
ANGLE_F64 = 1e-9            # fp64 throughout: ~10 eps / gap = 1e-14; 1e-9 leaves room for the summation order
# the library returns f32 normals: each component of a unit vector is rounded by at most half an ulp of 1, 2^-25, so the vector
# moves by at most sqrt(3) 2^-25 rad on top of the fp64 bound
ANGLE_F32 = ANGLE_F64 + np.sqrt(3.0) * 2.0 ** -25


# ------------------------------------------------------------------------------------------------ clouds
def corner_cloud(n, rng, sigma=0.01, size=8.0):
    """n points on three orthogonal size x size patches (z = 0, y = 0, x = 0) meeting in the origin, isotropic noise sigma."""
    uv = rng.uniform(0.0, size, (n, 2))
    face = rng.randint(0, 3, n)
    pts = np.zeros((n, 3))
    for f, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        m = face == f
        pts[m, a], pts[m, b] = uv[m, 0], uv[m, 1]
    return pts + rng.normal(0.0, sigma, (n, 3))


def cluster_cloud(n, rng, radius=0.05, jitter=1e-3, pitch=0.5):
    """n >= 3 points in clusters of three (the last one takes the n % 3 left over): jittered regular polygons of circumradius `radius`
    in random planes, centred on distinct nodes of a `pitch` lattice.  The 3 nearest of every point, itself included, are itself and
    its two polygon neighbours: a well-shaped triangle whose plane the normal must be perpendicular to.  (Three nearest points of a
    RANDOM cloud are close to collinear half of the time -- 50 % of a corner cloud falls below the gap at K = 3, measured -- and the
    gate would judge little.)"""
    sizes = [3] * (n // 3)
    sizes[-1] += n % 3
    side = int(np.ceil(len(sizes) ** (1.0 / 3.0))) + 1
    nodes = rng.choice(side ** 3, len(sizes), replace=False)
    out = []
    for node, m in zip(nodes, sizes):
        c = pitch * np.array([node % side, (node // side) % side, node // side ** 2], np.float64)
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = 2.0 * np.pi * (np.arange(m) + rng.uniform()) / m
        out.append(c + radius * (np.cos(a)[:, None] * Q[:, 0] + np.sin(a)[:, None] * Q[:, 1]) + rng.normal(0.0, jitter, (m, 3)))
    return np.concatenate(out)[rng.permutation(n)]


def normals_cloud(n, knn, seed=0):
    """the cloud the normals of (n, knn) are judged on: the corner; where the neighbourhood is three points, the cluster cloud"""
    rng = np.random.RandomState(seed)
    if n >= 3 and min(n, knn) == 3:
        return cluster_cloud(n, rng).astype(np.float32)
    return corner_cloud(n, rng).astype(np.float32)


def euler_update(x):
    """open3d's TransformVector6dToMatrix4d: [Rz(x2) Ry(x1) Rx(x0) | x3..5]"""
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    T = np.eye(4)
    T[:3, :3] = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                 [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                 [-sy, cy * sx, cy * cx]]
    T[:3, 3] = x[3:6]
    return T


START_OFFSET = (0.02, -0.03, 0.05, 0.15, -0.10, 0.12)     # rad, rad, rad, m, m, m
CORNER_MAX_DIST = 0.5


def corner_case(n, seed, sigma=0.01):
    """(src f32 [n,3], tgt f32 [n,3], gt [4,4] (src -> tgt), T0): source and target are INDEPENDENT samples of the corner, the
    source moved by a rigid transform; the start is the ground truth off by START_OFFSET."""
    rng = np.random.RandomState(seed)
    tgt = corner_cloud(n, rng, sigma).astype(np.float32)
    gt = euler_update(np.array([0.3, -0.2, 0.5, 1.0, -2.0, 0.5]))
    s = corner_cloud(n, rng, sigma)
    src = ((s - gt[:3, 3]) @ gt[:3, :3]).astype(np.float32)            # R^T (s - t)
    return src, tgt, gt, euler_update(np.array(START_OFFSET)) @ gt


def rot_err_deg(T, gt):
    R = T[:3, :3] @ gt[:3, :3].T
    return float(np.rad2deg(np.arctan2(np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0,
                                       (np.trace(R) - 1.0) / 2.0)))


def trans_err(T, gt):
    return float(np.linalg.norm(T[:3, 3] - gt[:3, 3]))


# ------------------------------------------------------------------------------------------------ normals
def canonical(v):
    """the sign rule of covariance_normal: the component of largest magnitude positive, ties -> the lowest axis"""
    k = int(np.argmax(np.abs(v)))          # (argmax returns the first maximum)
    return -v if v[k] < 0 else v


def neighbourhoods(pts, knn, radius=None):
    """[(indices of the neighbours kept)] per point: the min(knn, n) nearest, without those with fp32 d2 > fp32(radius)^2"""
    p = np.asarray(pts, np.float32)
    K = min(int(knn), p.shape[0])
    nn = orc.knn_points(p[None], p[None], K=K)
    idx, d2 = nn.idx[0], nn.dists[0]
    keep = np.ones_like(idx, bool) if radius is None else ~(d2 > np.float32(radius) * np.float32(radius))
    return [idx[i][keep[i]] for i in range(p.shape[0])]


def covariance(pts64, nb):
    q = pts64[nb]
    d = q - q.mean(axis=0)
    return d.T @ d


def normals_ref(pts, knn=30, radius=None):
    """-> (normals f64 [n,3], gap [n], fixed bool [n]): gap = (l1 - l0) / l2 (0 where the rule (0,0,1) applied or l2 = 0);
    fixed = fewer than 3 neighbours or a zero covariance."""
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    n = p64.shape[0]
    out, gap, fixed = np.zeros((n, 3)), np.zeros(n), np.zeros(n, bool)
    for i, nb in enumerate(neighbourhoods(pts, knn, radius)):
        C = covariance(p64, nb) if len(nb) >= 3 else np.zeros((3, 3))
        if not C.any():
            out[i], fixed[i] = (0.0, 0.0, 1.0), True
            continue
        w, V = np.linalg.eigh(C)
        out[i] = canonical(V[:, 0])
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    return out, gap, fixed


def angle(a, b):
    """angle between rows of a and b (atan2 of cross and dot: resolves 1e-16 rad where arccos stops at 1e-8)"""
    a, b = np.atleast_2d(np.asarray(a, np.float64)), np.atleast_2d(np.asarray(b, np.float64))
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))


def judge_normals(got, ref, gap, fixed, bar):
    """the gate both suites use: rule points exactly (0,0,1); everywhere the gap allows, angle <= bar WITH the sign (canonical on both
    sides); at most GAP_EXCLUDED_MAX of the cloud outside the gate.  -> (worst angle judged, share excluded)"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    assert np.array_equal(got[fixed], np.tile([0.0, 0.0, 1.0], (int(fixed.sum()), 1)))
    judged = ~fixed & (gap >= GAP_MIN)
    excluded = float((~fixed & ~judged).mean()) if len(gap) else 0.0
    worst = float(angle(got[judged], ref[judged]).max()) if judged.any() else 0.0
    assert np.abs(np.linalg.norm(got[~fixed], axis=1) - 1.0).max(initial=0.0) < 1e-6
    return worst, excluded


# ------------------------------------------------------------------------------------------------ ICP
def plane_system(p, q, nq):
    """A = sum J J^T [6,6], b = sum J r [6] with r = (p - q) . n, J = [p x n, n]"""
    r = ((p - q) * nq).sum(axis=1)
    J = np.concatenate([np.cross(p, nq), nq], axis=1)
    return J.T @ J, J.T @ r


def plane_solve(A, b):
    """x = -pinv(A) b with eigenvalues <= RANK_TOL * l_max treated as zero"""
    w, V = np.linalg.eigh(A)
    if not w.max() > 0:
        return np.zeros(6)
    k = w > RANK_TOL * w.max()
    return -(V[:, k] @ ((V[:, k].T @ b) / w[k]))


def icp_point_to_plane(src, tgt, normals, T_init, max_dist=0.2, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                       conds=None, trace=None):
    """open3d's RegistrationICP with TransformationEstimationPointToPlane -> (T float64 [4,4], fitness, inlier_rmse, iterations).
    conds: optional list; receives cond(J^T J) of every system solved.  trace: optional list; receives one record per evaluation,
    (T evaluated, fitness, rmse, |d fitness|, |d rmse|, stopped), the differences against the evaluation before (None for the first)."""
    T = np.asarray(T_init, np.float64).copy()
    tgt64 = np.asarray(tgt, np.float32).astype(np.float64)
    nrm64 = np.asarray(normals, np.float32).astype(np.float64)
    idx, fit, rmse, q = orc.icp_evaluate(src, tgt, T, max_dist)
    if trace is not None:
        trace.append((T.copy(), fit, rmse, None, None, False))
    it = 0
    for _ in range(max_iteration):
        ok = idx >= 0
        upd = np.eye(4)
        if ok.any():
            A, b = plane_system(q[ok], tgt64[idx[ok]], nrm64[idx[ok]])
            if conds is not None:
                conds.append(float(np.linalg.cond(A)))
            upd = euler_update(plane_solve(A, b))
            T = upd @ T
        it += 1
        pf, pr = fit, rmse
        idx, fit, rmse, q = orc.icp_evaluate(src, tgt, T, max_dist)
        stop = abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse
        if trace is not None:
            trace.append((T.copy(), fit, rmse, abs(pf - fit), abs(pr - rmse), stop))
        if stop:
            break
    return T, fit, rmse, it


# ------------------------------------------------------------------------------------------------ csrc/icp_plane_math.h on the host
_exe = []


def host_program():
    """path of tests/icp_plane_host.cpp compiled with the compiler that builds the library, or None where there is none"""
    if _exe:
        return _exe[0]
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    exe = None
    if hipcc:
        tmp = tempfile.mkdtemp(prefix="icp_plane_host_")
        atexit.register(shutil.rmtree, tmp, True)
        exe = os.path.join(tmp, "icp_plane_host")
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", _build.CSRC,
                               "-I", _build.INCLUDE, os.path.join(REPO, "tests", "icp_plane_host.cpp"), "-o", exe])
    _exe.append(exe)
    return exe


def host_run(kind, rows, width):
    """one record of `kind` per row of `rows` through the host program -> float64 [len(rows), width]; every number crosses as a
    hexadecimal float, bit for bit"""
    text = "".join(kind + " " + " ".join(float(v).hex() for v in r) + "\n" for r in rows)
    out = subprocess.run([host_program()], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    vals = np.array([[float.fromhex(v) for v in ln.split()] for ln in out if ln], np.float64)
    assert vals.shape == (len(rows), width), vals.shape
    return vals


def upper6(C):
    return [C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]


def upper21(A):
    return [A[p, q] for p in range(6) for q in range(p, 6)]
