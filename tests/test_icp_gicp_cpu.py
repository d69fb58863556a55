"""CPU: the ground the plane-to-plane (generalized) ICP stands on -- csrc/icp_gicp_math.h compiled for the host
(tests/icp_gicp_host.cpp) against numpy, the fp64 restatement (tests/icp_gicp_ref.py) on the corner case, and the refusals of the
Python entry points without a GPU.

Bounds (derived, not measured): M = 2 I - (1 - eps) (a a^T + b b^T) has eigenvalues in [2 eps, 2], so cond(M) <= 1 / eps and an
inverse computed in fp64 errs by a small multiple of cond(M) 2^-53 relative to max |W|: the bar is ten such units, 10 * 2^-53 / eps.
The 27 sums are a few hundred fp64 terms each, every term a short product of W (already within 1e-13 of numpy's): 1e-12 relative."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icp_gicp_ref as ref
import icp_plane_ref as plane

EPSILONS = (1e-3, 1e-2, 1e-1, 1.0)


@pytest.fixture(scope="module")
def host():
    if ref.host_program() is None:
        pytest.skip("no hipcc found: csrc/icp_gicp_math.h cannot be compiled here")
    return ref.host_run


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _weight_cases(rng):
    """(a, b) pairs: random unit vectors, b = +-a, b within 1e-3 of a, b = 0, both zero"""
    a = _unit(rng.normal(size=(64, 3)))
    near = _unit(a[:16] + 1e-3 * _unit(rng.normal(size=(16, 3))))
    pairs = [(a, _unit(rng.normal(size=(64, 3)))), (a[:16], a[:16].copy()), (a[:16], -a[:16]), (a[:16], near),
             (a[:16], np.zeros((16, 3))), (np.zeros((1, 3)), np.zeros((1, 3)))]
    # the axes themselves, where M is exactly diagonal
    pairs.append((np.eye(3), np.eye(3)[[1, 2, 0]]))
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


@pytest.mark.parametrize("eps", EPSILONS)
def test_host_weight_matches_numpy(host, eps):
    """gicp_weight against np.linalg.inv(M): max |W - inv(M)| <= 10 * 2^-53 / eps * max |W|, on every family of normals"""
    a, b = _weight_cases(np.random.RandomState(11))
    got = host("W", [list(x) + list(y) + [eps] for x, y in zip(a, b)], 6)
    want = ref.weight(a, b, eps)
    bar = 10.0 * 2.0 ** -53 / eps
    worst = max(np.abs(ref.full3(g) - w).max() / np.abs(w).max() for g, w in zip(got, want))
    print(f"[host weight eps={eps:g}] worst relative error {worst:.2e} (bar {bar:.2e}) over {len(a)} cases")
    assert worst <= bar
    # both normals zero: an isotropic pair, W = I / 2 exactly; eps = 1: the same whatever the normals are
    zero = host("W", [[0.0] * 6 + [eps]], 6)[0]
    assert np.array_equal(zero, [0.5, 0.0, 0.0, 0.5, 0.0, 0.5])
    if eps == 1.0:
        assert all(np.array_equal(g, zero) for g in got)
    # even in a and in b: equal bits with either negated
    for sa, sb in ((-1.0, 1.0), (1.0, -1.0)):
        flipped = host("W", [list(sa * x) + list(sb * y) + [eps] for x, y in zip(a, b)], 6)
        assert flipped.tobytes() == got.tobytes()


def test_host_sums_with_a_rank_one_weight_are_point_to_plane_s(host):
    """the sign check of the contract: with W = n n^T the terms are point to plane's J J^T and J r, J = [p x n, n]; gicp_accumulate
    takes any W, so fed n n^T it must reproduce icp_plane_ref.plane_system -- and so must the restatement's J0"""
    rng = np.random.RandomState(13)
    p, q, n = rng.normal(size=(50, 3)) * 3.0, rng.normal(size=(50, 3)) * 3.0, _unit(rng.normal(size=(50, 3)))
    A, g = plane.plane_system(p, q, n)
    W = n[:, :, None] * n[:, None, :]
    J0 = np.concatenate([-ref.skew(p), np.broadcast_to(np.eye(3), (50, 3, 3))], axis=2)
    A2, g2 = np.einsum("nki,nkl,nlj->ij", J0, W, J0), np.einsum("nki,nkl,nl->i", J0, W, p - q)
    assert np.abs(A2 - A).max() <= 1e-12 * np.abs(A).max() and np.abs(g2 - g).max() <= 1e-12 * np.abs(g).max()
    row = [50.0] + [v for k in range(50) for v in (*p[k], *(p[k] - q[k]), *plane.upper6(W[k]))]
    s = host("T", [row], 27)[0]
    assert np.abs(np.array(plane.upper21(A)) - s[:21]).max() <= 1e-12 * np.abs(A).max()
    assert np.abs(g - s[21:]).max() <= 1e-12 * np.abs(g).max()


@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("n", [1, 300])
def test_host_sums_match_the_restatement(host, n, eps):
    """the 27 sums gicp_accumulate builds over n correspondences against the restatement's system: 1e-12 relative to the largest
    entry of the matrix and of the right-hand side"""
    rng = np.random.RandomState(17 + n)
    p = plane.corner_cloud(n, rng, 0.01)
    a = _unit(np.eye(3)[np.abs(p).argmin(axis=1)] + rng.normal(0, 0.05, (n, 3)))
    b = _unit(np.eye(3)[np.abs(p).argmin(axis=1)] + rng.normal(0, 0.05, (n, 3)))
    d = np.array([0.05, -0.03, 0.04]) + rng.normal(0, 0.02, (n, 3))
    A, g = ref.gicp_system(p, p - d, a, b, eps)
    row = [float(n)] + [v for k in range(n) for v in (*p[k], *d[k], *a[k], *b[k], eps)]
    s = host("A", [row], 27)[0]
    dA = np.abs(np.array(plane.upper21(A)) - s[:21]).max() / np.abs(A).max()
    dg = np.abs(g - s[21:]).max() / np.abs(g).max()
    print(f"[host sums n={n} eps={eps:g}] matrix {dA:.2e}, right-hand side {dg:.2e} (bar 1e-12)")
    assert dA <= 1e-12 and dg <= 1e-12


# ---- the restatement alone -------------------------------------------------------------------------------------------------------

def _same_bits(x, y):
    return np.array_equal(x[0], y[0]) and x[1:] == y[1:]


def test_restatement_epsilon_one_ignores_the_normals():
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, 0)
    rng = np.random.RandomState(19)
    base = ref.icp_plane_to_plane(src, tgt, ns, nt, T0, plane.CORNER_MAX_DIST, 30, epsilon=1.0)
    other = ref.icp_plane_to_plane(src, tgt, _unit(rng.normal(size=ns.shape)).astype(np.float32), nt[::-1].copy(), T0,
                                   plane.CORNER_MAX_DIST, 30, epsilon=1.0)
    zero = ref.icp_plane_to_plane(src, tgt, np.zeros_like(ns), np.zeros_like(nt), T0, plane.CORNER_MAX_DIST, 30, epsilon=1e-3)
    assert _same_bits(base, other) and _same_bits(base, zero)
    assert base[3] > 4        # Gauss-Newton point to point: slower than the plane-to-plane loop below


def test_restatement_is_even_in_either_set_of_normals():
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, 1)
    base = ref.icp_plane_to_plane(src, tgt, ns, nt, T0, plane.CORNER_MAX_DIST, 30)
    assert _same_bits(base, ref.icp_plane_to_plane(src, tgt, -ns, nt, T0, plane.CORNER_MAX_DIST, 30))
    assert _same_bits(base, ref.icp_plane_to_plane(src, tgt, ns, -nt, T0, plane.CORNER_MAX_DIST, 30))


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_on_the_corner_case(seed):
    """On the corner case (2 000 points per cloud, correspondence distance 0.5 m): plane to plane converges within 30 iterations to
    below 0.1 deg and 0.02 m (the plane test's bar), in fewer iterations than epsilon = 1, and ends closer in translation than point
    to plane from the same start.  Measured: seed 0 -- 3 iterations, 0.030 deg / 4.55 mm against 8.70 mm; seed 1 -- 4 iterations,
    0.017 deg / 2.86 mm against 5.96 mm."""
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, seed)
    conds, margins = [], []
    T, fit, rmse, it = ref.icp_plane_to_plane(src, tgt, ns, nt, T0, plane.CORNER_MAX_DIST, 30, conds=conds, margins=margins)
    Tpl, _, _, it_pl = plane.icp_point_to_plane(src, tgt, nt, T0, plane.CORNER_MAX_DIST, 30)
    _, _, _, it_one = ref.icp_plane_to_plane(src, tgt, ns, nt, T0, plane.CORNER_MAX_DIST, 30, epsilon=1.0)
    print(f"[corner seed {seed}] plane to plane: {it} iterations, {plane.rot_err_deg(T, gt):.3f} deg, {1e3 * plane.trans_err(T, gt):.2f} mm, "
          f"cond <= {max(conds):.0f}, stop margin >= {min(margins):.1e}; point to plane: {it_pl} iterations, "
          f"{plane.rot_err_deg(Tpl, gt):.3f} deg, {1e3 * plane.trans_err(Tpl, gt):.2f} mm; epsilon = 1: {it_one} iterations")
    assert it < 30 and fit > 0.95
    assert plane.rot_err_deg(T, gt) < 0.1 and plane.trans_err(T, gt) < 0.02
    assert it < it_one
    assert plane.trans_err(T, gt) < plane.trans_err(Tpl, gt)
    assert max(conds) <= 1e4


def test_restatement_without_correspondences_is_the_identity():
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, 0)
    far = np.eye(4); far[:3, 3] = [500.0, 0.0, 0.0]
    T, fit, rmse, it = ref.icp_plane_to_plane(src, tgt, ns, nt, far, 0.5, 30)
    assert np.array_equal(T, far) and fit == 0.0 and rmse == 0.0 and it == 1


# ---- the entries and the Python surface without a GPU ------------------------------------------------------------------------------

def test_the_table_is_the_module_s_and_mirrors_the_header():
    """the header is one of include/ and its table one of _lib.TABLES (names, parameter counts and return types against the header:
    test_abi.py::test_table_mirrors_its_header_and_every_symbol_is_exported); here what is the module's own"""
    import abi_headers
    from umeregrobust_amd import _build, _lib, icp_gicp
    import os
    import re
    path = os.path.join(abi_headers.INCLUDE, "umereg_icp_gicp.h")
    assert path in _build.headers() and os.path.join(_build.CSRC, "icp_gicp_math.h") in _build.headers()      # part of the build hash
    assert icp_gicp.ICP_GICP_SIGNATURES is _lib.TABLES["umereg_icp_gicp.h"] and abi_headers.HEADERS["umereg_icp_gicp.h"][1] == 4
    assert icp_gicp.load_native is _lib.load
    lib = icp_gicp.load_native()
    assert lib is _lib.load() and lib.umereg_icp_plane_to_plane_f32.argtypes == icp_gicp.ICP_GICP_SIGNATURES["umereg_icp_plane_to_plane_f32"][1]
    raw = open(path).read()
    assert (icp_gicp.MIN_EPSILON, icp_gicp.MAX_EPSILON) == tuple(float(re.search(rf"#define UMEREG_GICP_{k}_EPSILON ([0-9.e-]+)f", raw).group(1))
                                                                 for k in ("MIN", "MAX"))


def test_entries_check_arguments_before_the_device():
    from umeregrobust_amd import icp_gicp
    lib = icp_gicp.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    size = lib.umereg_icp_plane_to_plane_workspace_bytes
    assert size(0, 5) == 0 and size(5, 0) == 0 and size(-1, -1) == 0
    assert size(2048, 100) == lib.umereg_icp_plane_workspace_bytes(2048, 100) > 0            # the 29 sums of point to plane
    T = np.eye(4)
    run = lambda **kw: lib.umereg_icp_plane_to_plane_f32(*[kw.get(k, d) for k, d in (                                # noqa: E731
        ("src", p), ("tgt", p), ("ns", p), ("nt", p), ("n_src", 10), ("n_tgt", 10), ("T0", T.ctypes.data), ("d", 0.2), ("it", 5),
        ("rf", 1e-6), ("rr", 1e-6), ("eps", 1e-3), ("T", T.ctypes.data), ("fit", None), ("rmse", None), ("iters", None), ("ws", p),
        ("nws", 1 << 16), ("st", None))])
    for kw in (dict(ns=None), dict(nt=None), dict(T0=None), dict(src=None), dict(n_src=0), dict(d=-1.0), dict(it=-1), dict(T=None)):
        assert run(**kw) == -1, kw
        assert b"icp_plane_to_plane" in lib.umereg_last_error()
    for eps in (0.0, 9e-5, 1.0001, 2.0, -1e-3, float("nan"), float("inf")):
        assert run(eps=eps) == -1, eps
        assert b"epsilon" in lib.umereg_last_error()
    enq = lambda **kw: lib.umereg_icp_plane_to_plane_enqueue_f32(*[kw.get(k, d) for k, d in (                        # noqa: E731
        ("src", p), ("tgt", p), ("ns", p), ("nt", p), ("n_src", 10), ("n_tgt", 10), ("T0", p), ("d", 0.2), ("it", 5), ("rf", 1e-6),
        ("rr", 1e-6), ("eps", 1e-3), ("first", 1), ("iterations", 4), ("state", p), ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(ns=None), dict(nt=None), dict(state=None), dict(T0=None), dict(eps=0.0), dict(eps=1.5)):
        assert enq(**kw) == -1, kw
    assert lib.umereg_icp_plane_to_plane_dev_f32(p, p, p, p, 10, 10, None, 0.2, 5, 1e-6, 1e-6, 1e-3, T.ctypes.data, None, None, None, p,
                                                 1 << 16, None) == -1
    if lib.umereg_device_count(None, 0) == 0:
        for eps in (1e-4, 1e-3, 1.0):
            assert run(eps=eps) == -2 and enq(eps=eps) == -2                                                         # UMEREG_ENODEV


def test_python_surface_without_a_gpu():
    from umeregrobust_amd import evaluate, icp_gicp, icp_plane, ops
    pts = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.icp_plane_to_plane(pts, pts, pts, pts, np.eye(4))
    for eps in (0.0, 9.9e-5, 1.0001, -1e-3, float("nan"), float("inf"), "1e-3", None, True, [1e-3]):
        with pytest.raises(ValueError, match="epsilon"):
            ops.icp_plane_to_plane(pts, pts, pts, pts, np.eye(4), epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            ops.IcpJob(pts, pts, pts, src_normals=pts, tgt_normals=pts, epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            icp_gicp.check_epsilon("icp", eps)
        if eps is not None:
            with pytest.raises(ValueError, match="epsilon"):
                icp_gicp.epsilon_of(SimpleNamespace(icp_gicp_epsilon=eps))
    for eps in (1e-4, 1e-3, np.float32(0.5), 1):
        assert icp_gicp.check_epsilon("icp", eps) == float(eps)
    assert icp_gicp.epsilon_of(SimpleNamespace()) == 1e-3 == icp_gicp.DEFAULT_EPSILON
    assert icp_gicp.epsilon_of(SimpleNamespace(icp_gicp_epsilon=0.01)) == 0.01
    with pytest.raises(ValueError, match="src_normals"):
        ops.IcpJob(pts, pts, pts, src_normals=pts)
    # the normals of either cloud: shape, dtype and device are refused under the argument's own name
    cloud = torch.zeros(10, 3)
    for name in ("src_normals", "tgt_normals"):
        for bad in (torch.zeros(9, 3), torch.zeros(10, 2), torch.zeros(10, 3, dtype=torch.float64), torch.zeros(10, 3, device="meta"),
                    np.zeros((10, 3), np.float32), None):
            with pytest.raises(ValueError, match=name):
                ops._normals_arg("icp_plane_to_plane", bad, cloud, name)
    assert ops._normals_arg("icp_plane_to_plane", cloud, cloud, "src_normals") is not None
    # the names of the estimations
    assert icp_plane.ESTIMATIONS == ("point_to_point", "point_to_plane", "plane_to_plane") and icp_gicp.ESTIMATION == "plane_to_plane"
    assert icp_plane.estimation_of(SimpleNamespace(icp_estimation="plane_to_plane")) == ("plane_to_plane", 30, None)
    assert icp_plane.estimation_of(SimpleNamespace(), "plane_to_plane")[0] == "plane_to_plane"
    with pytest.raises(ValueError, match="epsilon"):
        evaluate.evaluate_pairs([], SimpleNamespace(icp_estimation="plane_to_plane", icp_gicp_epsilon=1e-5))
    with pytest.raises(ValueError, match="epsilon"):
        evaluate.refine_registration([], [], SimpleNamespace(icp_gicp_epsilon=2.0), [], estimation="plane_to_plane")
    with pytest.raises(ValueError, match="icp_estimation"):
        icp_plane.estimation_of(SimpleNamespace(icp_estimation="generalized"))
    # opt-in: the defaults stay what they were
    sig = inspect.signature(ops.IcpJob.__init__).parameters
    assert sig["src_normals"].default is None and sig["tgt_normals"].default is None and sig["epsilon"].default == 1e-3
    assert inspect.signature(ops.icp_plane_to_plane).parameters["epsilon"].default == 1e-3
    assert list(inspect.signature(ops.icp_plane_to_plane).parameters)[:5] == ["src_pts", "tgt_pts", "src_normals", "tgt_normals", "T_init"]
