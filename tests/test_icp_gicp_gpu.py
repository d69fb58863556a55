"""GPU: the opt-in plane-to-plane (generalized) ICP (include/umereg_icp_gicp.h) against its fp64 restatement
(tests/icp_gicp_ref.py).

The gate is the point-to-plane test's own -- equal iteration count, |d fitness| < 1e-12, |d rmse| < 1e-9, max |dT| < 1e-9.  What
justifies it is asserted here, from the restatement, on every case judged: the condition number of every 6x6 system over its retained
eigenvalues is <= 1e4 (fp64 sums in another order and a closed-form W within 1e-13 of numpy's: ~1e-13 relative on the system, 1e-9 on
x).  Measured: <= 712 on the corner with its own normals, 1.6e3 with every normal (0,0,1), 5.8e3 on the ground plane.  The one case outside (the continuation batch, 2.1e4) is compared with
the synchronous call only."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icp_gicp_ref as ref
import icp_plane_ref as plane

pytestmark = pytest.mark.gpu

D = plane.CORNER_MAX_DIST


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    return np.array_equal(a.transformation, b.transformation) and a.iterations == b.iterations and a.fitness == b.fitness \
        and a.inlier_rmse == b.inlier_rmse


@functools.lru_cache(maxsize=None)
def _want(seed, n_src, max_dist, max_it, eps, start=1.0, normals="own"):
    """the restatement on the corner case (seed; the first n_src source points), computed once per case: (result, worst retained
    condition number, smallest stop margin).  normals: "own" or "z" (every normal (0,0,1))"""
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, seed)
    if start != 1.0:
        T0 = plane.euler_update(start * np.array(plane.START_OFFSET)) @ gt
    if normals == "z":
        ns, nt = np.tile(np.float32([0, 0, 1]), (len(ns), 1)), np.tile(np.float32([0, 0, 1]), (len(nt), 1))
    conds, margins = [], []
    out = ref.icp_plane_to_plane(src[:n_src], tgt, ns[:n_src], nt, T0, max_dist, max_it, epsilon=eps, conds=conds, margins=margins)
    return out, max(conds, default=1.0), min(margins, default=np.inf)


def _same(out, want, tag):
    """the gate, and the condition that justifies it"""
    (T, fit, rmse, it), cond, margin = want
    print(f"[{tag}] iterations {out.iterations} / {it}, d fitness {abs(out.fitness - fit):.1e}, d rmse {abs(out.inlier_rmse - rmse):.1e}, "
          f"max |dT| {np.abs(out.transformation - T).max():.1e}; cond <= {cond:.0f}, stop margin >= {margin:.1e}")
    assert cond <= 1e4, tag
    assert out.iterations == it, tag
    assert abs(out.fitness - fit) < 1e-12 and abs(out.inlier_rmse - rmse) < 1e-9, tag
    assert np.abs(out.transformation - T).max() < 1e-9, tag


def _dev_case(seed, gpu):
    src, tgt, ns, nt, gt, T0 = ref.corner(2000, seed)
    return T_(src, gpu), T_(tgt, gpu), T_(ns, gpu), T_(nt, gpu), gt, T0


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("seed", [0, 1])
def test_icp_plane_to_plane_vs_restatement(gpu, seed):
    from umeregrobust_amd import ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(seed, gpu)
    for max_it, eps in ((0, 1e-3), (1, 1e-3), (5, 1e-3), (30, 1e-1), (30, 1.0), (30, 1e-3)):
        out = ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, max_it, epsilon=eps)
        _same(out, _want(seed, 2000, D, max_it, eps), f"corner seed={seed} max_it={max_it} eps={eps:g}")
    # (the last one, eps = 1e-3:) it converged, and onto the ground truth; point to point from the same start needs more iterations
    assert out.iterations < 30 and out.fitness > 0.95
    assert plane.rot_err_deg(out.transformation, gt) < 0.1 and plane.trans_err(out.transformation, gt) < 0.02
    pp = ops.icp_point_to_point(s_, t_, T0, D, 100)
    assert out.iterations < pp.iterations
    # two runs: equal bits; either set of normals negated: the same bits again (only a a^T and b b^T enter)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, 30), out)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, -ns_, nt_, T0, D, 30), out)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, ns_, -nt_, T0, D, 30), out)
    # a start transform on the device (f32) is the same as its host copy
    T0d = T_(T0.astype(np.float32), gpu)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0d, D, 30), ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0.astype(np.float32), D, 30))


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 257])
def test_icp_gicp_source_count_edges(gpu, n_src):
    """the lane-group, round and block edges of the evaluation kernel (eight lanes per point, 32 points per round, 64 per block); one
    correspondence gives a rank-3 system (retained condition 212): the minimum-norm solve is well inside the gate"""
    from umeregrobust_amd import ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(0, gpu)
    for max_it in (1, 30):
        out = ops.icp_plane_to_plane(s_[:n_src].contiguous(), t_, ns_[:n_src].contiguous(), nt_, T0, D, max_it)
        _same(out, _want(0, n_src, D, max_it, 1e-3), f"n_src={n_src} max_it={max_it}")


def test_icp_gicp_edge_cases(gpu):
    from umeregrobust_amd import ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(0, gpu)
    src, tgt, ns, nt, _, _ = ref.corner(2000, 0)
    # a start 500 m away: no correspondence, the update is the identity, stop after one; T comes back bit-equal
    far = np.eye(4); far[:3, 3] = [500.0, 0.0, 0.0]
    out = ops.icp_plane_to_plane(s_, t_, ns_, nt_, far, 0.5, 30)
    assert out.fitness == 0.0 and out.inlier_rmse == 0.0 and out.iterations == 1
    assert ref.icp_plane_to_plane(src, tgt, ns, nt, far, 0.5, 30)[3] == 1
    assert np.array_equal(out.transformation, far)
    # a correspondence radius that spans several grid cells
    _same(ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, 2.0, 3), _want(0, 2000, 2.0, 3, 1e-3), "wide radius")
    # both sets of normals zero: isotropic covariances, M = 2 I -- the restatement at epsilon = 1 with the real normals
    zero = ops.icp_plane_to_plane(s_, t_, torch.zeros_like(ns_), torch.zeros_like(nt_), T0, D, 30)
    _same(zero, _want(0, 2000, D, 30, 1.0), "zero normals")
    # every normal (0,0,1), estimate_normals' fallback
    z_s, z_t = torch.zeros_like(ns_), torch.zeros_like(nt_)
    z_s[:, 2], z_t[:, 2] = 1.0, 1.0
    _same(ops.icp_plane_to_plane(s_, t_, z_s, z_t, T0, D, 30), _want(0, 2000, D, 30, 1e-3, normals="z"), "fallback normals")


def test_icp_gicp_ground_plane(gpu):
    """the exact z = 0 lattice of the point-to-plane suite's rank-deficient case, with the source's normals those of the moved plane:
    here the system has full rank (the in-plane directions carry weight 1/2), so the loop also moves in the plane; only the restatement
    gate is asserted"""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(12)
    g = np.arange(-20, 21) * 0.25
    tgt = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nt = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    flat = np.concatenate([rng.uniform(-4, 4, (500, 2)), np.zeros((500, 1))], axis=1)
    move = plane.euler_update(np.array([0.01, -0.015, 0.0, 0.0, 0.0, 0.04]))
    src = (flat @ move[:3, :3].T + move[:3, 3]).astype(np.float32)
    ns = np.tile((move[:3, :3] @ np.array([0.0, 0.0, 1.0])).astype(np.float32), (len(src), 1))
    s_, t_, ns_, nt_ = T_(src, gpu), T_(tgt, gpu), T_(ns, gpu), T_(nt, gpu)
    for max_it in (1, 30):
        conds, margins = [], []
        want = ref.icp_plane_to_plane(src, tgt, ns, nt, np.eye(4), 0.5, max_it, conds=conds, margins=margins)
        out = ops.icp_plane_to_plane(s_, t_, ns_, nt_, np.eye(4), 0.5, max_it)
        _same(out, (want, max(conds), min(margins)), f"ground plane max_it={max_it}")
    assert np.isfinite(out.transformation).all() and out.fitness == 1.0


def test_icp_gicp_index_discipline(gpu):
    """the target's normal is looked up by the ORIGINAL index the packed table carries, the source's by the source index: the same pair
    with the target's points and normals permuted together, and separately the source's, stays inside the gate of the unpermuted
    restatement (not bit-equal: the sums change order)"""
    from umeregrobust_amd import ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(1, gpu)
    want = _want(1, 2000, D, 30, 1e-3)
    g = torch.Generator().manual_seed(5)
    pt, ps = torch.randperm(2000, generator=g).to(gpu), torch.randperm(2000, generator=g).to(gpu)
    _same(ops.icp_plane_to_plane(s_, t_[pt].contiguous(), ns_, nt_[pt].contiguous(), T0, D, 30), want, "target permuted")
    _same(ops.icp_plane_to_plane(s_[ps].contiguous(), t_, ns_[ps].contiguous(), nt_, T0, D, 30), want, "source permuted")
    # and it is a discipline: normals permuted WITHOUT their points give another result
    off = ops.icp_plane_to_plane(s_, t_, ns_[ps].contiguous(), nt_[pt].contiguous(), T0, D, 30)
    assert np.abs(off.transformation - want[0][0]).max() > 1e-6


# ------------------------------------------------------------------------------------------------ jobs
def test_icp_job_plane_to_plane_equals_the_synchronous_call(gpu):
    """ops.IcpJob(..., src_normals=, tgt_normals=, epsilon=) returns what ops.icp_plane_to_plane returns, bit for bit: with three jobs
    in flight on one stream (a workspace each), with the start transform still being written when the job is created, and when four
    updates are not enough (3 x START_OFFSET, distance 0.3: 17 iterations, a continuation batch; its condition number of 2.1e4 is
    outside the restatement gate, so it is compared with the synchronous call only)."""
    from umeregrobust_amd import ops
    jobs, refs = [], []
    for seed, k, max_dist, max_it, eps in ((0, 1.0, 0.5, 30, 1e-3), (1, 1.0, 0.5, 2, 1e-2), (0, 3.0, 0.3, 200, 1e-3)):
        s_, t_, ns_, nt_, gt, _ = _dev_case(seed, gpu)
        T0 = plane.euler_update(k * np.array(plane.START_OFFSET)) @ gt
        T0d = torch.zeros((4, 4), dtype=torch.float32, device=gpu)
        T0d.copy_(torch.from_numpy(T0.astype(np.float32)), non_blocking=True)
        jobs.append(ops.IcpJob(s_, t_, T0d, max_dist, max_it, src_normals=ns_, tgt_normals=nt_, epsilon=eps))
        refs.append((s_, t_, ns_, nt_, T0d, max_dist, max_it, eps))
    assert sorted(j.slot for j in jobs) == [0, 1, 2]
    for job, (s_, t_, ns_, nt_, T0d, max_dist, max_it, eps) in zip(jobs, refs):
        out = job.result()
        assert _bits_equal(out, ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0d, max_dist, max_it, epsilon=eps))
        assert job.result() is out
    assert out.iterations > 4 and job.launched > 4                     # the last case needed its continuation batch
    # a point-to-point job and a point-to-plane job created next to a plane-to-plane one return what they return alone
    s_, t_, ns_, nt_, T0d, max_dist, _, _ = refs[0]
    a, b, c = (ops.IcpJob(s_, t_, T0d, max_dist, 30), ops.IcpJob(s_, t_, T0d, max_dist, 30, src_normals=ns_, tgt_normals=nt_),
               ops.IcpJob(s_, t_, T0d, max_dist, 30, tgt_normals=nt_))
    assert _bits_equal(a.result(), ops.icp_point_to_point(s_, t_, T0d, max_dist, 30))
    assert _bits_equal(b.result(), ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0d, max_dist, 30))
    assert _bits_equal(c.result(), ops.icp_point_to_plane(s_, t_, nt_, T0d, max_dist, 30))


def test_icp_gicp_stale_workspace(gpu):
    """no word of the workspace is read that the call did not write: equal bits after another ICP of other sizes has used the same
    cached workspace, and after that workspace has been filled with 0xFF bytes"""
    from umeregrobust_amd import _lib, ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(0, gpu)
    first = ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, 30)
    ops.icp_point_to_point(s_[:777].contiguous(), t_[:1501].contiguous(), T0, 0.3, 7)
    ops.icp_point_to_plane(s_[:300].contiguous(), t_[:911].contiguous(), nt_[:911].contiguous(), T0, 1.0, 3)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, 30), first)
    ws = ops._workspaces[(gpu.index, _lib.stream_ptr(gpu), "icp_sync")]
    ws.fill_(0xFF)
    assert _bits_equal(ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, 30), first)


# ------------------------------------------------------------------------------------------------ integration
def test_refine_registration_plane_to_plane(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import refine_registration
    s_, t_, ns_, nt_, gt, T0 = _dev_case(0, gpu)
    pairs = [(s_, t_, torch.from_numpy(gt).float())]
    R_hat, t_hat = [T0[:3, :3]], [T0[:3, 3]]
    par = dict(icp_max_correspondence_distance=D, icp_max_iteration=50)
    Tfull = np.eye(4); Tfull[:3, :3], Tfull[:3, 3] = R_hat[0], t_hat[0]
    # the new name, by args and by keyword, with its epsilon: the direct call on normals estimated with the same knn
    gicp = refine_registration(R_hat, t_hat, SimpleNamespace(icp_estimation="plane_to_plane", icp_normal_knn=16, **par), pairs)
    by_kw = refine_registration(R_hat, t_hat, SimpleNamespace(icp_normal_knn=16, icp_gicp_epsilon=1e-2, **par), pairs,
                                estimation="plane_to_plane")
    n16s, n16t = ops.estimate_normals(s_, 16), ops.estimate_normals(t_, 16)
    for got, eps in ((gicp, 1e-3), (by_kw, 1e-2)):
        direct = ops.icp_plane_to_plane(s_, t_, n16s, n16t, Tfull, D, 50, epsilon=eps)
        assert torch.equal(got[0][0], torch.from_numpy(direct.transformation).float())
    assert not torch.equal(gicp[0][0], by_kw[0][0])
    # the option unset, or "point_to_plane": the bits they return when called the way the point-to-plane suite calls them
    unset = refine_registration(R_hat, t_hat, SimpleNamespace(**par), pairs)
    named = refine_registration(R_hat, t_hat, SimpleNamespace(icp_estimation="point_to_point", **par), pairs)
    for a, b in zip(unset, named):
        assert N_(a).tobytes() == N_(b).tobytes()
    assert torch.equal(unset[0][0], torch.from_numpy(ops.icp_point_to_point(s_, t_, Tfull, D, 50).transformation).float())
    p2pl = refine_registration(R_hat, t_hat, SimpleNamespace(icp_estimation="point_to_plane", icp_normal_knn=16, **par), pairs)
    assert torch.equal(p2pl[0][0], torch.from_numpy(ops.icp_point_to_plane(s_, t_, n16t, Tfull, D, 50).transformation).float())
    assert not torch.equal(gicp[0][0], unset[0][0]) and not torch.equal(gicp[0][0], p2pl[0][0])


def test_evaluate_pairs_plane_to_plane(gpu):
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
    max_corr, max_it = float(getattr(args, "icp_max_correspondence_distance", 0.2)), int(getattr(args, "icp_max_iteration", 200))
    tgt_raw, src_raw = pair["tgt_pts"][0], pair["src_pts"][0]
    unset, named = run(), run(icp_estimation="point_to_point")
    for k in ("R_sel", "t_sel", "T_est", "rre", "rte"):
        assert N_(unset[k]).tobytes() == N_(named[k]).tobytes(), k
    T_sel = torch.eye(4); T_sel[:3, :3], T_sel[:3, 3] = unset["R_sel"][0], unset["t_sel"][0]
    T_sel = T_sel.to(gpu).contiguous()
    assert torch.equal(unset["T_est"][0], torch.from_numpy(ops.icp_point_to_point(src_raw, tgt_raw, T_sel, max_corr, max_it).transformation).float())
    p2pl = run(icp_estimation="point_to_plane", icp_normal_knn=20)
    n20s, n20t = ops.estimate_normals(src_raw, 20), ops.estimate_normals(tgt_raw, 20)
    direct = ops.icp_point_to_plane(src_raw, tgt_raw, n20t, T_sel, max_corr, max_it)
    assert torch.equal(p2pl["T_est"][0], torch.from_numpy(direct.transformation).float())
    gicp = run(icp_estimation="plane_to_plane", icp_normal_knn=20, icp_gicp_epsilon=1e-2)
    assert torch.equal(gicp["R_sel"], unset["R_sel"]) and torch.equal(gicp["t_sel"], unset["t_sel"])       # same selection, same RNG use
    direct = ops.icp_plane_to_plane(src_raw, tgt_raw, n20s, n20t, T_sel, max_corr, max_it, epsilon=1e-2)
    assert torch.equal(gicp["T_est"][0], torch.from_numpy(direct.transformation).float())
    assert gicp["rr_sp"] == 1.0
    # one pair at a time on the caller's stream (the synchronous form): the same refinement
    serial = evaluate_pairs([pair], SimpleNamespace(**vars(args), icp_estimation="plane_to_plane", icp_normal_knn=20, icp_gicp_epsilon=1e-2),
                            rng=np.random.RandomState(0), overlap=False)
    assert torch.equal(serial["T_est"], gicp["T_est"])


def test_bad_arguments(gpu):
    from umeregrobust_amd import ops
    s_, t_, ns_, nt_, gt, T0 = _dev_case(0, gpu)
    s_, ns_, t_, nt_ = s_[:100].contiguous(), ns_[:100].contiguous(), t_[:200].contiguous(), nt_[:200].contiguous()
    T0d = T_(T0.astype(np.float32), gpu)
    for bad in (ns_[:99], ns_[:, :2], ns_.double(), ns_.cpu(), N_(ns_), None):
        with pytest.raises(ValueError, match="src_normals"):
            ops.icp_plane_to_plane(s_, t_, bad, nt_, T0)
        if bad is not None:
            with pytest.raises(ValueError, match="src_normals"):
                ops.IcpJob(s_, t_, T0d, 0.2, 30, src_normals=bad, tgt_normals=nt_)
    for bad in (nt_[:199], nt_[:, :2], nt_.double(), nt_.cpu(), N_(nt_), None):
        with pytest.raises(ValueError, match="tgt_normals"):
            ops.icp_plane_to_plane(s_, t_, ns_, bad, T0)
    with pytest.raises(ValueError, match="src_normals"):
        ops.IcpJob(s_, t_, T0d, 0.2, 30, src_normals=ns_)
    for eps in (0.0, 9.9e-5, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="epsilon"):
            ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            ops.IcpJob(s_, t_, T0d, 0.2, 30, src_normals=ns_, tgt_normals=nt_, epsilon=eps)
    with pytest.raises(ValueError, match="4x4"):
        ops.icp_plane_to_plane(s_, t_, ns_, nt_, np.eye(3))
    # the bounds themselves are accepted
    for eps in (1e-4, 1.0):
        assert ops.icp_plane_to_plane(s_, t_, ns_, nt_, T0, D, 2, epsilon=eps).iterations >= 1
    # nothing above left a job's workspace slot taken
    job = ops.IcpJob(s_, t_, T0d, 0.5, 5, src_normals=ns_, tgt_normals=nt_)
    assert job.slot == 0
    job.result()
