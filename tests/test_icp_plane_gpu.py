"""GPU: the opt-in point-to-plane refinement (include/umereg_icp_plane.h) against its fp64 restatement (tests/icp_plane_ref.py).

Normals: the library returns f32, so against the fp64 eigenvector the bar is the CPU suite's 1e-9 rad plus the rounding of a unit
vector to f32, sqrt(3) 2^-25 rad (icp_plane_ref.ANGLE_F32), wherever the gap (l1 - l0) / l2 >= 0.1; at most 2 % of a cloud may fall
outside that gate.  ICP: the point-to-point test's own gate -- equal iteration count, |d fitness| < 1e-12, |d rmse| < 1e-9,
max |dT| < 1e-9 -- which cond(J^T J) <= 1e4 justifies (fp64 sums in another order: ~1e-13 relative on the system, 1e-9 on x)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icp_plane_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _normals_case(n, knn):
    pts = ref.normals_cloud(n, knn)
    return (pts,) + ref.normals_ref(pts, knn)


@functools.lru_cache(maxsize=None)
def _corner(n=2000, seed=0):
    src, tgt, gt, T0 = ref.corner_case(n, seed)
    normals = ref.normals_ref(tgt, 30)[0].astype(np.float32)
    return src, tgt, normals, gt, T0


def _same(out, want, tag):
    T, fit, rmse, it = want
    print(f"[{tag}] iterations {out.iterations} / {it}, d fitness {abs(out.fitness - fit):.1e}, d rmse {abs(out.inlier_rmse - rmse):.1e}, "
          f"max |dT| {np.abs(out.transformation - T).max():.1e}")
    assert out.iterations == it, tag
    assert abs(out.fitness - fit) < 1e-12 and abs(out.inlier_rmse - rmse) < 1e-9, tag
    assert np.abs(out.transformation - T).max() < 1e-9, tag


def _bits_equal(a, b):
    return np.array_equal(a.transformation, b.transformation) and a.iterations == b.iterations and a.fitness == b.fitness \
        and a.inlier_rmse == b.inlier_rmse


# ------------------------------------------------------------------------------------------------ normals
@pytest.mark.parametrize("knn", [3, 30, 64])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 2000])
def test_normals_vs_restatement(gpu, n, knn):
    from umeregrobust_amd import ops
    pts, want, gap, fixed = _normals_case(n, knn)
    got = N_(ops.estimate_normals(T_(pts, gpu), knn))
    assert got.dtype == np.float32 and got.shape == (n, 3)
    worst, excluded = ref.judge_normals(got, want, gap, fixed, ref.ANGLE_F32)
    print(f"[normals n={n} K={knn}] worst angle {worst:.2e} rad, excluded {100 * excluded:.2f} %, rule points {int(fixed.sum())}")
    assert worst <= ref.ANGLE_F32
    assert excluded <= ref.GAP_EXCLUDED_MAX
    assert fixed.all() == (n < 3)
    # canonical sign: the f32 component of largest magnitude is positive wherever it is the largest by more than the rounding
    j = ~fixed
    top = np.sort(np.abs(want[j]), axis=1)
    clear = top[:, 2] - top[:, 1] > 1e-6
    assert (np.take_along_axis(got[j], np.abs(want[j]).argmax(axis=1)[:, None], 1)[clear, 0] > 0).all()


def test_normals_hybrid_radius(gpu):
    """open3d's hybrid search: neighbours beyond the radius are dropped; five isolated points keep only themselves -> (0,0,1)"""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(4)
    far = 50.0 + 5.0 * np.arange(15).reshape(5, 3) * np.array([1.0, 0.3, 0.1])
    pts = np.concatenate([ref.corner_cloud(2000, rng), far]).astype(np.float32)
    want, gap, fixed = ref.normals_ref(pts, 30, radius=1.0)
    assert fixed.sum() == 5 and fixed[-5:].all()
    got = N_(ops.estimate_normals(T_(pts, gpu), 30, radius=1.0))
    worst, excluded = ref.judge_normals(got, want, gap, fixed, ref.ANGLE_F32)
    print(f"[normals hybrid] worst angle {worst:.2e} rad, excluded {100 * excluded:.2f} %")
    assert worst <= ref.ANGLE_F32 and excluded <= ref.GAP_EXCLUDED_MAX
    # the radius matters: without it the isolated points take the corner's points as neighbours
    free = N_(ops.estimate_normals(T_(pts, gpu), 30))
    assert not np.array_equal(free[-5:], got[-5:])
    # a radius below every distance: every point is alone
    alone = N_(ops.estimate_normals(T_(pts, gpu), 30, radius=1e-6))
    assert np.array_equal(alone, np.tile(np.float32([0, 0, 1]), (len(pts), 1)))


def test_normals_degenerate_clouds(gpu):
    from umeregrobust_amd import ops
    rng = np.random.RandomState(6)
    # all points equal: zero covariance -> (0,0,1)
    same = np.tile(np.float32([3.25, -7.5, 100.0]), (100, 1))
    assert np.array_equal(N_(ops.estimate_normals(T_(same, gpu), 16)), np.tile(np.float32([0, 0, 1]), (100, 1)))
    # collinear: no plane; finite and unit (not judged by angle)
    line = (np.float32([1.0, -2.0, 0.5]) + np.linspace(0, 4, 50, dtype=np.float32)[:, None] * np.float32([0.6, 0.0, 0.8]))
    got = N_(ops.estimate_normals(T_(line, gpu), 10)).astype(np.float64)
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-6
    # exact axis planes: the covariance row of the axis is exactly zero, the normal exactly the axis
    for axis, c in ((2, 2.0), (0, -1.5), (1, 64.0)):
        p = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
        p[:, axis] = c
        e = np.zeros(3, np.float32); e[axis] = 1.0
        assert np.array_equal(N_(ops.estimate_normals(T_(p, gpu), 16)), np.tile(e, (300, 1))), axis


def test_normals_far_from_the_origin(gpu):
    """the corner 1e3 m from the origin: the covariance about the neighbourhood's own mean does not cancel, the normals are those
    of the unshifted cloud to the gate.  (The shifted coordinates are the f32 values; the unshifted cloud is their exact difference
    to 1000, so both clouds have the same fp32 distances and neighbours.)"""
    from umeregrobust_amd import ops
    shifted = (ref.corner_cloud(2000, np.random.RandomState(8)) + 1000.0).astype(np.float32)
    base64 = shifted.astype(np.float64) - 1000.0
    base = base64.astype(np.float32)
    assert np.array_equal(base.astype(np.float64), base64)
    want, gap, fixed = ref.normals_ref(base, 30)
    for name, cloud in (("base", base), ("shifted", shifted)):
        got = N_(ops.estimate_normals(T_(cloud, gpu), 30))
        worst, excluded = ref.judge_normals(got, want, gap, fixed, ref.ANGLE_F32)
        print(f"[normals {name}] worst angle {worst:.2e} rad, excluded {100 * excluded:.2f} %")
        assert worst <= ref.ANGLE_F32 and excluded <= ref.GAP_EXCLUDED_MAX


def test_normals_guard_rows_and_garbage_workspace(gpu):
    """the entry writes its [n,3] rows and nothing around them, and reads no workspace word it did not write: same bytes over two
    workspaces full of different garbage"""
    from umeregrobust_amd import _lib, icp_plane
    lib = icp_plane.load_native()
    pts = T_(ref.normals_cloud(257, 30), gpu)
    n, pad = 257, 64
    need = int(lib.umereg_normals_workspace_bytes(n, 30))
    outs = []
    for fill in (0xA5, 0x3C):
        buf = torch.full((n + 2 * pad, 3), -77.0, dtype=torch.float32, device=gpu)
        g = torch.Generator(device="cpu").manual_seed(fill)
        ws = (torch.randint(0, 256, (need,), generator=g, dtype=torch.uint8) ^ fill).to(gpu)
        _lib.call(gpu, lib.umereg_estimate_normals_f32, pts.data_ptr(), n, 30, 0.0, buf[pad:].data_ptr(), ws.data_ptr(), need,
                  _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        assert bool((buf[:pad] == -77.0).all()) and bool((buf[pad + n:] == -77.0).all())
        outs.append(N_(buf[pad:pad + n]))
    assert outs[0].tobytes() == outs[1].tobytes()
    want, gap, fixed = ref.normals_ref(N_(pts), 30)
    assert ref.judge_normals(outs[0], want, gap, fixed, ref.ANGLE_F32)[0] <= ref.ANGLE_F32
    # a workspace one byte short is refused
    with pytest.raises(_lib.NativeCallError):
        _lib.call(gpu, lib.umereg_estimate_normals_f32, pts.data_ptr(), n, 30, 0.0, buf[pad:].data_ptr(), ws.data_ptr(), need - 1,
                  _lib.stream_ptr(gpu))


# ------------------------------------------------------------------------------------------------ ICP
def test_icp_point_to_plane_vs_restatement(gpu):
    from umeregrobust_amd import ops
    src, tgt, normals, gt, T0 = _corner()
    s_, t_, n_ = T_(src, gpu), T_(tgt, gpu), T_(normals, gpu)
    for max_it in (0, 1, 5, 30):
        conds = []
        want = ref.icp_point_to_plane(src, tgt, normals, T0, ref.CORNER_MAX_DIST, max_it, conds=conds)
        assert max(conds, default=0.0) <= 1e4
        out = ops.icp_point_to_plane(s_, t_, n_, T0, ref.CORNER_MAX_DIST, max_it)
        _same(out, want, f"corner max_it={max_it}")
    # it converged, and onto the ground truth; point to point from the same start needs more iterations
    assert out.iterations < 30 and out.fitness > 0.95
    assert ref.rot_err_deg(out.transformation, gt) < 0.1 and ref.trans_err(out.transformation, gt) < 0.02
    pp = ops.icp_point_to_point(s_, t_, T0, ref.CORNER_MAX_DIST, 100)
    assert out.iterations < pp.iterations
    # two runs: equal bits; every target normal negated: the same bits again (J J^T and J r do not see the sign)
    again = ops.icp_point_to_plane(s_, t_, n_, T0, ref.CORNER_MAX_DIST, 30)
    assert _bits_equal(again, out)
    neg = ops.icp_point_to_plane(s_, t_, -n_, T0, ref.CORNER_MAX_DIST, 30)
    assert _bits_equal(neg, out)
    # a start transform on the device (f32) is the same as its host copy
    T0d = T_(T0.astype(np.float32), gpu)
    assert _bits_equal(ops.icp_point_to_plane(s_, t_, n_, T0d, ref.CORNER_MAX_DIST, 30),
                       ops.icp_point_to_plane(s_, t_, n_, T0.astype(np.float32), ref.CORNER_MAX_DIST, 30))


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 257])
def test_icp_plane_source_count_edges(gpu, n_src):
    """the lane-group, round and block edges of the evaluation kernel (eight lanes per point, 32 points per round, 64 per block)"""
    from umeregrobust_amd import ops
    src, tgt, normals, gt, T0 = _corner()
    s = src[:n_src]
    for max_it in (1, 30):
        want = ref.icp_point_to_plane(s, tgt, normals, T0, ref.CORNER_MAX_DIST, max_it)
        _same(ops.icp_point_to_plane(T_(s, gpu), T_(tgt, gpu), T_(normals, gpu), T0, ref.CORNER_MAX_DIST, max_it), want,
              f"n_src={n_src} max_it={max_it}")


def test_icp_plane_edge_cases(gpu):
    from umeregrobust_amd import ops
    src, tgt, normals, gt, T0 = _corner()
    s_, t_, n_ = T_(src, gpu), T_(tgt, gpu), T_(normals, gpu)
    # a start 500 m away: no correspondence, identity updates, stop after one
    far = np.eye(4); far[:3, 3] = [500.0, 0.0, 0.0]
    out = ops.icp_point_to_plane(s_, t_, n_, far, 0.5, 30)
    want = ref.icp_point_to_plane(src, tgt, normals, far, 0.5, 30)
    assert out.fitness == 0.0 and out.inlier_rmse == 0.0 and out.iterations == want[3] == 1
    assert np.array_equal(out.transformation, far)
    # a correspondence radius that spans several grid cells
    want = ref.icp_point_to_plane(src, tgt, normals, T0, 2.0, 3)
    _same(ops.icp_point_to_plane(s_, t_, n_, T0, 2.0, 3), want, "wide radius")


def test_icp_plane_rank_deficient_plane(gpu):
    """a ground plane alone: the exact z = 0 lattice with normals (0,0,1).  The system has rank 3; the update is finite and leaves
    yaw and the in-plane translation exactly untouched (from the identity: T[1,0], T[0,3], T[1,3] stay 0)."""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(12)
    g = np.arange(-20, 21) * 0.25
    tgt = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    normals = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    flat = np.concatenate([rng.uniform(-4, 4, (500, 2)), np.zeros((500, 1))], axis=1)
    move = ref.euler_update(np.array([0.01, -0.015, 0.0, 0.0, 0.0, 0.04]))
    src = (flat @ move[:3, :3].T + move[:3, 3]).astype(np.float32)
    s_, t_, n_ = T_(src, gpu), T_(tgt, gpu), T_(normals, gpu)
    one = ops.icp_point_to_plane(s_, t_, n_, np.eye(4), 0.5, 1)
    T = one.transformation
    assert np.isfinite(T).all() and one.fitness == 1.0
    assert T[1, 0] == 0.0 and T[0, 3] == 0.0 and T[1, 3] == 0.0
    assert abs(T[2, 3] + 0.04) < 5e-3 and np.abs(T[:3, :3] - np.eye(3)).max() > 5e-3
    for max_it in (1, 30):
        want = ref.icp_point_to_plane(src, tgt, normals, np.eye(4), 0.5, max_it)
        out = ops.icp_point_to_plane(s_, t_, n_, np.eye(4), 0.5, max_it)
        _same(out, want, f"ground plane max_it={max_it}")
    moved = src.astype(np.float64) @ out.transformation[:3, :3].T + out.transformation[:3, 3]
    assert np.abs(moved[:, 2]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ jobs
def test_icp_job_with_normals_equals_the_synchronous_call(gpu):
    """ops.IcpJob(..., tgt_normals=...) returns what ops.icp_point_to_plane returns, bit for bit -- also when four updates are not
    enough (a continuation batch), with several jobs in flight on one stream (a workspace each) and with the start transform still
    being written when the job is created."""
    from umeregrobust_amd import ops
    jobs, refs = [], []
    for seed, k, max_dist, max_it in ((0, 1.0, 0.5, 30), (1, 1.0, 0.5, 2), (0, 3.0, 0.3, 200)):
        src, tgt, normals, gt, _ = _corner(2000, seed)
        T0 = ref.euler_update(k * np.array(ref.START_OFFSET)) @ gt
        s_, t_, n_ = T_(src, gpu), T_(tgt, gpu), T_(normals, gpu)
        T0d = torch.zeros((4, 4), dtype=torch.float32, device=gpu)
        T0d.copy_(torch.from_numpy(T0.astype(np.float32)), non_blocking=True)
        jobs.append(ops.IcpJob(s_, t_, T0d, max_dist, max_it, tgt_normals=n_))
        refs.append((s_, t_, n_, T0d, max_dist, max_it))
    assert sorted(j.slot for j in jobs) == [0, 1, 2]
    for job, (s_, t_, n_, T0d, max_dist, max_it) in zip(jobs, refs):
        out = job.result()
        want = ops.icp_point_to_plane(s_, t_, n_, T0d, max_dist, max_it)
        assert _bits_equal(out, want)
        assert job.result() is out
    assert out.iterations > 4 and job.launched > 4                     # the last case needed its continuation batch
    # a job without normals next to one with: the point-to-point chain is what it was
    s_, t_, n_, T0d, max_dist, _ = refs[0]
    a, b = ops.IcpJob(s_, t_, T0d, max_dist, 30), ops.IcpJob(s_, t_, T0d, max_dist, 30, tgt_normals=n_)
    assert _bits_equal(a.result(), ops.icp_point_to_point(s_, t_, T0d, max_dist, 30))
    assert _bits_equal(b.result(), ops.icp_point_to_plane(s_, t_, n_, T0d, max_dist, 30))


# ------------------------------------------------------------------------------------------------ integration
def test_refine_registration_estimations(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import refine_registration
    src, tgt, normals, gt, T0 = _corner()
    s_, t_ = T_(src, gpu), T_(tgt, gpu)
    pairs = [(s_, t_, torch.from_numpy(gt).float())]
    R_hat, t_hat = [T0[:3, :3]], [T0[:3, 3]]
    par = dict(icp_max_correspondence_distance=ref.CORNER_MAX_DIST, icp_max_iteration=50)
    unset = refine_registration(R_hat, t_hat, SimpleNamespace(**par), pairs)
    named = refine_registration(R_hat, t_hat, SimpleNamespace(icp_estimation="point_to_point", **par), pairs)
    for a, b in zip(unset, named):
        assert N_(a).tobytes() == N_(b).tobytes()
    plane = refine_registration(R_hat, t_hat, SimpleNamespace(icp_estimation="point_to_plane", icp_normal_knn=16, **par), pairs)
    by_kw = refine_registration(R_hat, t_hat, SimpleNamespace(icp_normal_knn=16, **par), pairs, estimation="point_to_plane")
    Tfull = np.eye(4); Tfull[:3, :3], Tfull[:3, 3] = R_hat[0], t_hat[0]
    direct = ops.icp_point_to_plane(s_, t_, ops.estimate_normals(t_, 16), Tfull, ref.CORNER_MAX_DIST, 50)
    want = torch.from_numpy(direct.transformation).float()
    assert torch.equal(plane[0][0], want) and torch.equal(by_kw[0][0], want)
    assert not torch.equal(plane[0][0], unset[0][0])
    assert float(plane[1][0]) <= float(unset[1][0]) + 1e-3 and float(plane[2][0]) <= float(unset[2][0]) + 1e-3


def test_evaluate_pairs_estimations(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import evaluate_pairs
    from umeregrobust_amd.synth import synth_pair
    from umeregrobust_amd.utils.general_utils import benchmark_config_path, update_namespace_from_yaml
    args = update_namespace_from_yaml(SimpleNamespace(), benchmark_config_path("kitti_test"))
    args.batch_size = 1
    p = synth_pair(2, N=12000, n_kp=64)
    pair = dict(src_pts=T_(p.src_pts, gpu)[None], tgt_pts=T_(p.tgt_pts, gpu)[None], src_feat=T_(p.src_feat, gpu)[None],
                tgt_feat=T_(p.tgt_feat, gpu)[None], gt_tform=T_(p.gt_tform, gpu))
    run = lambda **kw: evaluate_pairs([pair], SimpleNamespace(**vars(args), **kw), rng=np.random.RandomState(0))   # noqa: E731
    unset, named = run(), run(icp_estimation="point_to_point")
    for k in ("R_sel", "t_sel", "T_est", "rre", "rte"):
        assert N_(unset[k]).tobytes() == N_(named[k]).tobytes(), k
    plane = run(icp_estimation="point_to_plane", icp_normal_knn=20)
    assert torch.equal(plane["R_sel"], unset["R_sel"]) and torch.equal(plane["t_sel"], unset["t_sel"])     # same selection, same RNG use
    T_sel = torch.eye(4); T_sel[:3, :3], T_sel[:3, 3] = plane["R_sel"][0], plane["t_sel"][0]
    tgt_raw, src_raw = pair["tgt_pts"][0], pair["src_pts"][0]
    direct = ops.icp_point_to_plane(src_raw, tgt_raw, ops.estimate_normals(tgt_raw, 20), T_sel.to(gpu).contiguous(),
                                    float(getattr(args, "icp_max_correspondence_distance", 0.2)), int(getattr(args, "icp_max_iteration", 200)))
    assert torch.equal(plane["T_est"][0], torch.from_numpy(direct.transformation).float())
    assert plane["rr_sp"] == 1.0
    # one pair at a time on the caller's stream (the synchronous form): the same refinement
    serial = evaluate_pairs([pair], SimpleNamespace(**vars(args), icp_estimation="point_to_plane", icp_normal_knn=20),
                            rng=np.random.RandomState(0), overlap=False)
    assert torch.equal(serial["T_est"], plane["T_est"])


def test_bad_arguments(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import evaluate_pairs, refine_registration
    src, tgt, normals, gt, T0 = _corner()
    s_, t_, n_ = T_(src[:100], gpu), T_(tgt[:200], gpu), T_(normals[:200], gpu)
    T0d = T_(T0.astype(np.float32), gpu)
    for bad in (n_[:199], n_[:, :2], n_.double(), n_.cpu(), N_(n_), None):
        with pytest.raises(ValueError, match="tgt_normals"):
            ops.icp_point_to_plane(s_, t_, bad, T0)
        if bad is not None:
            with pytest.raises(ValueError, match="tgt_normals"):
                ops.IcpJob(s_, t_, T0d, 0.2, 30, tgt_normals=bad)
    with pytest.raises(ValueError, match="4x4"):
        ops.icp_point_to_plane(s_, t_, n_, np.eye(3))
    with pytest.raises(ValueError, match="clouds"):
        ops.icp_point_to_plane(s_[:, :2], t_, n_, T0)
    for knn in (2, 65, 0, -1):
        with pytest.raises(ValueError, match="knn"):
            ops.estimate_normals(t_, knn)
    with pytest.raises(ValueError, match="cloud"):
        ops.estimate_normals(t_[None], 30)
    with pytest.raises(ValueError, match="icp_estimation"):
        refine_registration([T0[:3, :3]], [T0[:3, 3]], SimpleNamespace(icp_estimation="generalized"), [(s_, t_, torch.eye(4))])
    with pytest.raises(ValueError, match="icp_estimation"):
        evaluate_pairs([], SimpleNamespace(icp_estimation="colored"))
    # nothing above left a job's workspace slot taken
    job = ops.IcpJob(s_, t_, T0d, 0.5, 5, tgt_normals=n_)
    assert job.slot == 0
    job.result()
