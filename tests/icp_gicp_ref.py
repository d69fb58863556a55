"""fp64 restatement of the plane-to-plane (generalized) ICP refinement (include/umereg_icp_gicp.h), for
tests/test_icp_gicp_cpu.py and tests/test_icp_gicp_gpu.py: the open3d loop of icp_plane_ref.icp_point_to_plane with the system

    a = R n_s, b = n_q, M = 2 I - (1 - eps) (a a^T + b b^T), W = inv(M), d = p - q, J0 = [-[p]x I3]
    (sum J0^T W J0) x = -(sum J0^T W d)

built by numpy in fp64 (np.linalg.inv for W), icp_plane_ref's thresholded solve and update, correspondences from the oracle
(oracle.icp_evaluate mirrors the device's fp32 distance and its tie rule), f32-rounded normals widened to fp64, and epsilon rounded to
f32 first, as the C entries receive it."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import icp_plane_ref as plane
from oracle import oracle as orc

REPO = plane.REPO
MIN_EPSILON, MAX_EPSILON, DEFAULT_EPSILON = 1e-4, 1.0, 1e-3


def skew(p):
    """[p]x per row: skew(p) @ v = p x v"""
    z = np.zeros(len(p))
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], 1), np.stack([p[:, 2], z, -p[:, 0]], 1), np.stack([-p[:, 1], p[:, 0], z], 1)], 1)


def covariance_sum(a, b, eps):
    """M [n,3,3] = C_q + R C_s R^T with C = I - (1 - eps) n n^T"""
    return 2.0 * np.eye(3) - (1.0 - eps) * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])


def weight(a, b, eps):
    return np.linalg.inv(covariance_sum(np.atleast_2d(a), np.atleast_2d(b), eps))


def gicp_system(p, q, a, b, eps):
    """A = sum J0^T W J0 [6,6], g = sum J0^T W d [6]"""
    W = weight(a, b, eps)
    J0 = np.concatenate([-skew(p), np.broadcast_to(np.eye(3), (len(p), 3, 3))], axis=2)
    return np.einsum("nki,nkl,nlj->ij", J0, W, J0), np.einsum("nki,nkl,nl->i", J0, W, p - q)


def retained_cond(A):
    """condition number of A over the eigenvalues plane_solve keeps"""
    w = np.linalg.eigvalsh(A)
    if not w.max() > 0:
        return 1.0
    k = w[w > plane.RANK_TOL * w.max()]
    return float(k.max() / k.min())


def icp_plane_to_plane(src, tgt, src_normals, tgt_normals, T_init, max_dist=0.2, max_iteration=30, relative_fitness=1e-6,
                       relative_rmse=1e-6, epsilon=DEFAULT_EPSILON, conds=None, margins=None, trace=None):
    """open3d's RegistrationICP loop with the plane-to-plane system -> (T float64 [4,4], fitness, inlier_rmse, iterations).
    conds: optional list; receives the retained condition number of every system solved.  margins: optional list; receives, per stop
    test, how far the decision is from flipping.  trace: optional list; receives one record per evaluation, (T evaluated, fitness,
    rmse, |d fitness|, |d rmse|, stopped), the differences against the evaluation before (None for the first)."""
    eps = float(np.float32(epsilon))
    T = np.asarray(T_init, np.float64).copy()
    tgt64 = np.asarray(tgt, np.float32).astype(np.float64)
    ns64 = np.asarray(src_normals, np.float32).astype(np.float64)
    nt64 = np.asarray(tgt_normals, np.float32).astype(np.float64)
    idx, fit, rmse, p = orc.icp_evaluate(src, tgt, T, max_dist)
    if trace is not None:
        trace.append((T.copy(), fit, rmse, None, None, False))
    it = 0
    for _ in range(max_iteration):
        ok = idx >= 0
        if ok.any():
            A, g = gicp_system(p[ok], tgt64[idx[ok]], ns64[ok] @ T[:3, :3].T, nt64[idx[ok]], eps)
            if conds is not None:
                conds.append(retained_cond(A))
            T = plane.euler_update(plane.plane_solve(A, g)) @ T
        it += 1
        pf, pr = fit, rmse
        idx, fit, rmse, p = orc.icp_evaluate(src, tgt, T, max_dist)
        df, dr = abs(pf - fit), abs(pr - rmse)
        stop = df < relative_fitness and dr < relative_rmse
        if margins is not None:      # what either difference would have to move by for the decision to flip
            margins.append(min(relative_fitness - df, relative_rmse - dr) if stop else max(df - relative_fitness, dr - relative_rmse))
        if trace is not None:
            trace.append((T.copy(), fit, rmse, df, dr, stop))
        if stop:
            break
    return T, fit, rmse, it


@functools.lru_cache(maxsize=None)
def corner(n=2000, seed=0):
    """icp_plane_ref.corner_case with the normals of both clouds (f32; the source's in the source's own frame)"""
    src, tgt, gt, T0 = plane.corner_case(n, seed)
    ns = plane.normals_ref(src, 30)[0].astype(np.float32)
    nt = plane.normals_ref(tgt, 30)[0].astype(np.float32)
    return src, tgt, ns, nt, gt, T0


# ------------------------------------------------------------------------------------------------ csrc/icp_gicp_math.h on the host
_exe = []


def host_program():
    """path of tests/icp_gicp_host.cpp compiled with the compiler that builds the library, or None where there is none"""
    if _exe:
        return _exe[0]
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    exe = None
    if hipcc:
        tmp = tempfile.mkdtemp(prefix="icp_gicp_host_")
        atexit.register(shutil.rmtree, tmp, True)
        exe = os.path.join(tmp, "icp_gicp_host")
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", _build.CSRC,
                               "-I", _build.INCLUDE, os.path.join(REPO, "tests", "icp_gicp_host.cpp"), "-o", exe])
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


def full3(w6):
    """[xx, xy, xz, yy, yz, zz] -> symmetric 3x3"""
    return np.array([[w6[0], w6[1], w6[2]], [w6[1], w6[3], w6[4]], [w6[2], w6[4], w6[5]]])
