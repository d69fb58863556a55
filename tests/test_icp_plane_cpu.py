"""CPU: the ground the point-to-plane refinement stands on -- csrc/icp_plane_math.h compiled for the host
(tests/icp_plane_host.cpp) against numpy, the fp64 restatement (tests/icp_plane_ref.py) on the corner case, the header's place in the one ABI
(tests/test_abi.py checks include/umereg_icp_plane.h against its table), and the refusals of the Python entry points without a GPU.

Bounds (derived, not measured): the arithmetic is fp64 throughout, so an eigenvector errs by ~10 eps / gap ~ 1e-14 where the gap
(l1 - l0) / l2 >= 0.1 -- 1e-9 rad leaves room for the summation order; a solve of a system with cond <= 1e4 errs by
~cond * eps ~ 1e-12 relative -- 1e-10."""
import os
import re

import numpy as np
import pytest
import torch

import abi_headers
import icp_plane_ref as ref

HEADER = "umereg_icp_plane.h"


@pytest.fixture(scope="module")
def host():
    if ref.host_program() is None:
        pytest.skip("no hipcc found: csrc/icp_plane_math.h cannot be compiled here")
    return ref.host_run


def _covariances(pts, knn):
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    return [ref.covariance(p64, nb) for nb in ref.neighbourhoods(pts, knn)]


@pytest.mark.parametrize("n,knn,seed", [(600, 16, 0), (2000, 30, 1)])
def test_host_normals_match_numpy(host, n, knn, seed):
    """covariance_normal against numpy's eigenvector: angle <= 1e-9 rad wherever the gap allows, canonical sign, and at most 2 % of
    the cloud outside the gate (measured: 0.33 % at 600 points with K = 16, 0 at 2 000 with K = 30)."""
    pts = ref.corner_cloud(n, np.random.RandomState(seed)).astype(np.float32)
    want, gap, fixed = ref.normals_ref(pts, knn)
    got = host("N", [ref.upper6(C) for C in _covariances(pts, knn)], 3)
    worst, excluded = ref.judge_normals(got, want, gap, fixed, ref.ANGLE_F64)
    print(f"[host normals n={n} K={knn}] worst angle {worst:.2e} rad, excluded {100 * excluded:.2f} %")
    assert not fixed.any()
    assert worst <= ref.ANGLE_F64
    assert excluded <= ref.GAP_EXCLUDED_MAX
    # canonical sign on every point, judged or not: the largest component is positive
    k = np.abs(got).argmax(axis=1)
    assert (got[np.arange(n), k] > 0).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-15


def test_host_normal_rules(host):
    """zero covariance -> (0,0,1); an exact axis plane -> exactly the axis; sign ties -> the lowest axis; collinear -> finite, unit"""
    z = host("N", [[0.0] * 6], 3)
    assert np.array_equal(z, [[0.0, 0.0, 1.0]])
    rng = np.random.RandomState(3)
    for axis in range(3):
        d = rng.normal(size=(20, 3)); d[:, axis] = 0.0
        n = host("N", [ref.upper6(d.T @ d)], 3)[0]
        e = np.zeros(3); e[axis] = 1.0
        assert np.array_equal(n, e), (axis, n)
    # the normal of the plane x + y = 0 is (1, 1, 0) / sqrt 2 up to sign and rounding: whichever of the two equal-looking components is
    # larger, it is positive
    d = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    n = host("N", [ref.upper6(d.T @ d)], 3)[0]
    assert n[np.abs(n).argmax()] > 0 and abs(abs(n[0]) - np.sqrt(0.5)) < 1e-15 and abs(n[0] - n[1]) < 1e-15
    d = np.outer(np.linspace(-1, 1, 9), [1.0, 2.0, -0.5])
    n = host("N", [ref.upper6(d.T @ d)], 3)[0]
    assert np.isfinite(n).all() and abs(np.linalg.norm(n) - 1.0) < 1e-15 and abs(n @ [1.0, 2.0, -0.5]) < 1e-12


def test_host_solve_matches_numpy(host):
    """plane_solve against numpy on systems whose condition number this test itself asserts is <= 1e4:
    |x - x_numpy| <= 1e-10 |x|."""
    rng = np.random.RandomState(5)
    rows, want = [], []
    for case in range(24):
        n = 50 + 20 * case
        p = ref.corner_cloud(n, rng, 0.01)
        nq = np.eye(3)[np.abs(p).argmin(axis=1)] + rng.normal(0, 0.02, (n, 3))
        q = p + rng.normal(0, 0.03, (n, 3))
        A, b = ref.plane_system(p, q, nq)
        assert np.linalg.cond(A) <= 1e4
        rows.append(ref.upper21(A) + list(b))
        want.append(np.linalg.solve(A, -b))
    got = host("S", rows, 6)
    for x, w in zip(got, want):
        assert np.linalg.norm(x - w) <= 1e-10 * np.linalg.norm(w)
    # the restatement's own solve is the same solution on these systems
    for r, w in zip(rows, want):
        A = np.zeros((6, 6)); A[np.triu_indices(6)] = r[:21]; A = A + A.T - np.diag(np.diag(A))
        assert np.linalg.norm(ref.plane_solve(A, np.array(r[21:])) - w) <= 1e-10 * np.linalg.norm(w)


def test_host_rank3_plane(host):
    """an exact z = 0 plane constrains rotation about x and y and translation along z only: the update's x2, x3, x4 are exactly
    zero, the rest is the minimum-norm solution, everything finite"""
    rng = np.random.RandomState(7)
    n = 200
    p = np.concatenate([rng.uniform(-4, 4, (n, 2)), np.zeros((n, 1))], axis=1)
    th = np.array([0.01, -0.02, 0.0, 0.0, 0.0, 0.03])
    moved = p @ ref.euler_update(th)[:3, :3].T + th[3:]
    nq = np.tile([0.0, 0.0, 1.0], (n, 1))
    q = moved.copy(); q[:, 2] = 0.0
    A, b = ref.plane_system(moved, q, nq)
    x = host("S", [ref.upper21(A) + list(b)], 6)[0]
    assert np.isfinite(x).all()
    assert x[2] == 0.0 and x[3] == 0.0 and x[4] == 0.0
    w = ref.plane_solve(A, b)
    assert np.linalg.norm(x - w) <= 1e-10 * np.linalg.norm(w) and np.linalg.norm(x) > 1e-2
    # the update moves the points back onto the plane (to second order in the angles)
    back = moved @ ref.euler_update(x)[:3, :3].T + x[3:]
    assert np.abs(back[:, 2]).max() < 2e-3 and np.abs(moved[:, 2]).max() > 5e-2
    # no correspondences at all: A = 0 -> x = 0
    assert np.array_equal(host("S", [[0.0] * 27], 6)[0], np.zeros(6))


def test_host_euler_update(host):
    """Rz(x2) Ry(x1) Rx(x0) and t = x3..5, against the product of the three elementary rotations"""
    rng = np.random.RandomState(9)
    xs = rng.uniform(-1, 1, (16, 6))
    got = host("U", xs, 12)
    for x, g in zip(xs, got):
        cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        assert np.abs(g[:9].reshape(3, 3) - Rz @ Ry @ Rx).max() < 1e-15
        assert np.array_equal(g[9:], x[3:])
        assert np.abs(ref.euler_update(x)[:3, :3] - Rz @ Ry @ Rx).max() < 1e-15


def test_restatement_on_the_corner_case():
    """The restatement alone, on the corner case (2 000 points per cloud, independent samples, sigma 0.01 m, start off by
    (0.02, -0.03, 0.05) rad and (0.15, -0.10, 0.12) m, correspondence distance 0.5 m): point to plane needs fewer iterations than
    point to point, ends no farther from the ground truth in rotation and in translation, and cond(J^T J) <= 1e4 at every iteration."""
    from oracle import oracle as orc
    src, tgt, gt, T0 = ref.corner_case(2000, 0)
    normals, gap, fixed = ref.normals_ref(tgt, 30)
    conds = []
    Tpl, fit_pl, _, it_pl = ref.icp_point_to_plane(src, tgt, normals.astype(np.float32), T0, ref.CORNER_MAX_DIST, 100, conds=conds)
    Tpp, fit_pp, _, it_pp = orc.icp_point_to_point(src, tgt, T0, ref.CORNER_MAX_DIST, 100)
    print(f"[corner] plane: {it_pl} iterations, {ref.rot_err_deg(Tpl, gt):.3f} deg, {1e3 * ref.trans_err(Tpl, gt):.1f} mm, cond "
          f"{min(conds):.1e} .. {max(conds):.1e}; point: {it_pp} iterations, {ref.rot_err_deg(Tpp, gt):.3f} deg, "
          f"{1e3 * ref.trans_err(Tpp, gt):.1f} mm; start {ref.rot_err_deg(T0, gt):.3f} deg, {1e3 * ref.trans_err(T0, gt):.1f} mm")
    assert it_pl < it_pp
    assert ref.rot_err_deg(Tpl, gt) <= ref.rot_err_deg(Tpp, gt)
    assert ref.trans_err(Tpl, gt) <= ref.trans_err(Tpp, gt)
    assert max(conds) <= 1e4
    assert fit_pl > 0.95 and not fixed.any()
    assert float((gap < ref.GAP_MIN).mean()) <= ref.GAP_EXCLUDED_MAX


# ---- the header's place and the Python surface without a GPU -----------------------------------------------------------------

def test_the_header_is_one_of_include_s_and_its_table_is_the_package_s():
    from umeregrobust_amd import _build, _lib, icp_plane
    # typed by the package tables; of the public headers this one, and no other, declares the point-to-plane entries
    assert icp_plane.ICP_PLANE_SIGNATURES is _lib.TABLES[HEADER] and icp_plane.load_native is _lib.load
    assert len(os.listdir(abi_headers.INCLUDE)) == len(abi_headers.HEADERS) == len(_lib.TABLES)      # the number: tests/test_abi.py
    assert [h for h in sorted(os.listdir(abi_headers.INCLUDE)) if "icp_point_to_plane" in abi_headers.text(h)] == [HEADER]
    assert os.path.join(abi_headers.INCLUDE, HEADER) in _build.headers()          # part of the build hash
    text = abi_headers.text(HEADER)
    assert (icp_plane.MIN_KNN, icp_plane.MAX_KNN) == tuple(int(re.search(rf"#define UMEREG_NORMALS_{k}_KNN (\d+)", text).group(1))
                                                           for k in ("MIN", "MAX"))
    lib = icp_plane.load_native()
    assert lib.umereg_abi_version() == _lib.ABI_VERSION == 2


def test_entries_check_arguments_before_the_device():
    from umeregrobust_amd import icp_plane
    lib = icp_plane.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    assert lib.umereg_normals_workspace_bytes(0, 30) == 0 and lib.umereg_normals_workspace_bytes(10, 2) == 0
    assert lib.umereg_normals_workspace_bytes(10, 65) == 0 and lib.umereg_normals_workspace_bytes(10, 30) > 0
    assert lib.umereg_icp_plane_workspace_bytes(0, 5) == 0 and lib.umereg_icp_plane_workspace_bytes(5, 0) == 0
    # 29 sums per block of 64 source points where point to point has 17 (32 blocks: both partial tables are multiples of 256 bytes)
    assert lib.umereg_icp_plane_workspace_bytes(2048, 100) - lib.umereg_icp_workspace_bytes(2048, 100) == 32 * 12 * 8
    assert lib.umereg_estimate_normals_f32(None, 10, 30, 0.0, p, p, 1 << 16, None) == -1
    assert lib.umereg_estimate_normals_f32(p, 0, 30, 0.0, p, p, 1 << 16, None) == -1
    for knn in (2, 65, -1):
        assert lib.umereg_estimate_normals_f32(p, 10, knn, 0.0, p, p, 1 << 16, None) == -1
        assert b"knn" in lib.umereg_last_error()
    T = np.eye(4)
    run = lambda **kw: lib.umereg_icp_point_to_plane_f32(*[kw.get(k, d) for k, d in (                                # noqa: E731
        ("src", p), ("tgt", p), ("nrm", p), ("n_src", 10), ("n_tgt", 10), ("T0", T.ctypes.data), ("d", 0.2), ("it", 5), ("rf", 1e-6),
        ("rr", 1e-6), ("T", T.ctypes.data), ("fit", None), ("rmse", None), ("iters", None), ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(nrm=None), dict(T0=None), dict(src=None), dict(n_src=0), dict(d=-1.0), dict(it=-1), dict(T=None)):
        assert run(**kw) == -1, kw
    assert b"icp_point_to_plane" in lib.umereg_last_error()
    assert lib.umereg_icp_plane_enqueue_f32(p, p, None, 10, 10, p, 0.2, 5, 1e-6, 1e-6, 1, 4, p, p, 1 << 16, None) == -1
    assert lib.umereg_icp_plane_enqueue_f32(p, p, p, 10, 10, p, 0.2, 5, 1e-6, 1e-6, 1, 4, None, p, 1 << 16, None) == -1
    if lib.umereg_device_count(None, 0) == 0:
        assert run() == -2 and lib.umereg_estimate_normals_f32(p, 10, 30, 0.0, p, p, 1 << 16, None) == -2      # UMEREG_ENODEV


def test_python_surface_without_a_gpu():
    from types import SimpleNamespace
    from umeregrobust_amd import evaluate, icp_plane, ops
    import inspect
    pts = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estimate_normals(pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.icp_point_to_plane(pts, pts, pts, np.eye(4))
    for knn in (2, 65, 3.5, True):
        with pytest.raises(ValueError, match="knn"):
            ops.estimate_normals(pts, knn=knn)
    with pytest.raises(ValueError, match="radius"):
        ops.estimate_normals(pts, radius=0.0)
    assert icp_plane.estimation_of(SimpleNamespace()) == ("point_to_point", 30, None)
    assert icp_plane.estimation_of(SimpleNamespace(icp_estimation="point_to_plane", icp_normal_knn=16, icp_normal_radius=0.5)) == \
        ("point_to_plane", 16, 0.5)
    assert icp_plane.estimation_of(SimpleNamespace(icp_estimation="point_to_plane"), "point_to_point")[0] == "point_to_point"
    with pytest.raises(ValueError, match="icp_estimation"):
        icp_plane.estimation_of(SimpleNamespace(icp_estimation="plane"))
    with pytest.raises(ValueError, match="icp_estimation"):
        evaluate.refine_registration([], [], SimpleNamespace(), [], estimation="generalized")
    with pytest.raises(ValueError, match="icp_estimation"):
        evaluate.evaluate_pairs([], SimpleNamespace(icp_estimation="colored"))
    with pytest.raises(ValueError, match="knn"):
        evaluate.evaluate_pairs([], SimpleNamespace(icp_estimation="point_to_plane", icp_normal_knn=100))
    # the defaults stay the reference's estimator
    assert inspect.signature(evaluate.refine_registration).parameters["estimation"].default is None
    assert inspect.signature(ops.IcpJob.__init__).parameters["tgt_normals"].default is None
    assert inspect.signature(ops.estimate_normals).parameters["knn"].default == 30
