"""ops.icp_multi_scale on the GPU, on the case tests/test_icp_multiscale_cpu.py qualifies (tests/icp_multiscale_ref.py: the corner from
a start 0.8 m off, levels 0.8 m / 1.6 m, 0.4 m / 0.8 m, the clouds as given / 0.2 m).

(a) the call equals, bit for bit, the same levels composed by hand from ops.voxel_down_sample, ops.estimate_normals and the plain calls;
(b) each level against its fp64 restatement, started from the LIBRARY's own previous transform on the mirror's downsampled clouds, with
    the project's one-level gate (tests/test_icp_plane_gpu.py): equal iteration count, |d fitness| < 1e-12, |d rmse| < 1e-9,
    max |dT| < 1e-9, and cond(J^T J) <= 1e4 asserted for the two normal-based estimations;
(c) the basin; (d) one level of voxel size 0 is the plain call; (e) evaluate's two refinement sites; (f) bad arguments."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icp_plane_ref as plane
from tests import icp_multiscale_ref as ms

pytestmark = pytest.mark.gpu


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_equal(a, b):
    return np.array_equal(a.transformation, b.transformation) and a.iterations == b.iterations and a.fitness == b.fitness \
        and a.inlier_rmse == b.inlier_rmse


def _same(out, want, cond, tag):
    """the one-level gate of tests/test_icp_plane_gpu.py, and the condition that justifies it"""
    T, fit, rmse, it = want
    print(f"[{tag}] iterations {out.iterations} / {it}, d fitness {abs(out.fitness - fit):.1e}, d rmse {abs(out.inlier_rmse - rmse):.1e}, "
          f"max |dT| {np.abs(out.transformation - T).max():.1e}; cond <= {cond:.0f}")
    assert cond <= 1e4, tag
    assert out.iterations == it, tag
    assert abs(out.fitness - fit) < 1e-12 and abs(out.inlier_rmse - rmse) < 1e-9, tag
    assert np.abs(out.transformation - T).max() < 1e-9, tag


_runs = {}


def _run(gpu, estimation):
    """ops.icp_multi_scale on the case, once per estimation and process"""
    from umeregrobust_amd import ops
    if estimation not in _runs:
        src, tgt, gt, T0 = ms.case()
        _runs[estimation] = ops.icp_multi_scale(T_(src, gpu), T_(tgt, gpu), T0, ms.VOXEL_SIZES, ms.DISTANCES, ms.ITERATIONS,
                                                estimation=estimation, normal_knn=ms.KNN)
    return _runs[estimation]


def _plain(ops, estimation, s, t, T, dist, iters, normals=None):
    if estimation == "point_to_point":
        return ops.icp_point_to_point(s, t, T, dist, iters)
    ns, nt = normals if normals is not None else (ops.estimate_normals(s, ms.KNN), ops.estimate_normals(t, ms.KNN))
    if estimation == "point_to_plane":
        return ops.icp_point_to_plane(s, t, nt, T, dist, iters)
    return ops.icp_plane_to_plane(s, t, ns, nt, T, dist, iters)


@pytest.mark.parametrize("estimation", ms.ESTIMATIONS)
def test_equals_the_levels_composed_by_hand(gpu, estimation):
    from umeregrobust_amd import ops
    src, tgt, gt, T0 = ms.case()
    s_, t_ = T_(src, gpu), T_(tgt, gpu)
    out = _run(gpu, estimation)
    T, total = T0, 0
    assert len(out.levels) == 3
    for k, (voxel, dist, iters) in enumerate(zip(ms.VOXEL_SIZES, ms.DISTANCES, ms.ITERATIONS)):
        s, t = (ops.voxel_down_sample(s_, voxel), ops.voxel_down_sample(t_, voxel)) if voxel else (s_, t_)
        reg = _plain(ops, estimation, s, t, T, dist, iters)
        lv = out.levels[k]
        assert _bits_equal(lv, reg), (estimation, k)
        assert (lv.voxel_size, lv.max_correspondence_distance, lv.n_src, lv.n_tgt) == (voxel, dist, s.shape[0], t.shape[0])
        T, total = reg.transformation, total + reg.iterations
    assert np.array_equal(out.transformation, T) and out.iterations == total
    assert (out.fitness, out.inlier_rmse) == (reg.fitness, reg.inlier_rmse)
    assert out.transformation.dtype == np.float64


@pytest.mark.parametrize("estimation", ms.ESTIMATIONS)
def test_every_level_against_its_restatement(gpu, estimation):
    from umeregrobust_amd import ops
    out = _run(gpu, estimation)
    T = ms.case()[3]
    for k, (s, t) in enumerate(ms.pyramid()):
        conds = []
        want = ms.run_level(estimation, k, T, conds=conds)
        normals = None if estimation == "point_to_point" else tuple(T_(a, gpu) for a in ms.level_normals(k))
        got = _plain(ops, estimation, T_(s, gpu), T_(t, gpu), T, ms.DISTANCES[k], ms.ITERATIONS[k], normals)
        _same(got, want, max(conds, default=1.0), f"{estimation} level {k}")
        assert (out.levels[k].n_src, out.levels[k].n_tgt) == (len(s), len(t))           # the library's clouds are the mirror's
        T = out.levels[k].transformation                                               # the LIBRARY's own transform starts the next level


def test_the_basin(gpu):
    """from 0.8 m off, the plain call at 0.2 m ends more than 0.4 m away; the three levels end within 0.1 m and 0.5 degrees"""
    from umeregrobust_amd import ops
    src, tgt, gt, T0 = ms.case()
    single = ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), T0, ms.SINGLE_DISTANCE, ms.SINGLE_ITERATIONS)
    print(f"single scale: {single.iterations} updates, {plane.trans_err(single.transformation, gt):.3f} m")
    assert plane.trans_err(single.transformation, gt) > 0.4
    for estimation in ms.ESTIMATIONS:
        out = _run(gpu, estimation)
        te, re = plane.trans_err(out.transformation, gt), plane.rot_err_deg(out.transformation, gt)
        print(f"{estimation}: {[lv.iterations for lv in out.levels]} updates, {te:.4f} m / {re:.4f} deg")
        assert te < 0.1 and re < 0.5


def test_one_level_of_voxel_size_zero_is_the_plain_call(gpu):
    from umeregrobust_amd import ops
    src, tgt, gt, _ = ms.case()
    s_, t_ = T_(src, gpu), T_(tgt, gpu)
    T0 = plane.euler_update(np.array(plane.START_OFFSET)) @ gt
    plain = ops.icp_point_to_point(s_, t_, T0, 0.5, 30)
    for zero in (0, 0.0, -1.0):
        out = ops.icp_multi_scale(s_, t_, T0, [zero], [0.5], [30])
        assert _bits_equal(out, plain) and len(out.levels) == 1 and out.levels[0].voxel_size == 0.0
    # a device f32 start reaches level 0 as the plain call takes it
    T0d = T_(T0.astype(np.float32), gpu)
    assert _bits_equal(ops.icp_multi_scale(s_, t_, T0d, [0], [0.5], [30]), ops.icp_point_to_point(s_, t_, T0d, 0.5, 30))
    a = ops.icp_multi_scale(s_, t_, T0d, (0.4, 0), (0.8, 0.2), (30, 30))
    b = ops.icp_multi_scale(s_, t_, T0.astype(np.float32), (0.4, 0), (0.8, 0.2), (30, 30))
    assert _bits_equal(a, b)


def test_refine_registration_with_levels(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import refine_registration
    src, tgt, gt, T0 = ms.case()
    s_, t_ = T_(src, gpu), T_(tgt, gpu)
    pairs = [(s_, t_, torch.from_numpy(gt).float())]
    R_hat, t_hat = [T0[:3, :3]], [T0[:3, 3]]
    Tfull = np.zeros((4, 4)); Tfull[:3, :3], Tfull[:3, 3], Tfull[3, 3] = R_hat[0], t_hat[0], 1
    par = dict(icp_max_correspondence_distance=0.2, icp_max_iteration=60)
    # unset: what the parent returns, the plain call
    unset = refine_registration(R_hat, t_hat, SimpleNamespace(**par), pairs)
    plain = ops.icp_point_to_point(s_, t_, Tfull, 0.2, 60)
    assert torch.equal(unset[0][0], torch.from_numpy(plain.transformation).float())
    none = refine_registration(R_hat, t_hat, SimpleNamespace(icp_voxel_sizes=None, **par), pairs)
    assert all(torch.equal(a, b) for a, b in zip(unset, none))
    for estimation in ms.ESTIMATIONS:
        # the defaults of levels_of: max(2 voxel, 0.2) and 0.2 on the last level, 60 everywhere -- the levels of the case
        got = refine_registration(R_hat, t_hat, SimpleNamespace(icp_voxel_sizes=list(ms.VOXEL_SIZES), icp_estimation=estimation, **par), pairs)
        want = ops.icp_multi_scale(s_, t_, Tfull, ms.VOXEL_SIZES, ms.DISTANCES, ms.ITERATIONS, estimation=estimation)
        assert torch.equal(got[0][0], torch.from_numpy(want.transformation).float()), estimation
        assert float(got[2][0]) < 0.1 < 0.4 < float(unset[2][0])
    explicit = refine_registration(R_hat, t_hat, SimpleNamespace(icp_voxel_sizes=[0.4, 0], icp_level_distances=[1.0, 0.3],
                                                                 icp_level_iterations=[20, 10], **par), pairs)
    want = ops.icp_multi_scale(s_, t_, Tfull, [0.4, 0], [1.0, 0.3], [20, 10])
    assert torch.equal(explicit[0][0], torch.from_numpy(want.transformation).float())


def test_evaluate_pairs_with_levels(gpu):
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
    unset, none = run(), run(icp_voxel_sizes=None)
    for k in ("R_sel", "t_sel", "T_est", "rre", "rte"):
        assert unset[k].numpy().tobytes() == none[k].numpy().tobytes(), k
    max_corr = float(getattr(args, "icp_max_correspondence_distance", 0.2))
    max_it = int(getattr(args, "icp_max_iteration", 200))
    src_raw, tgt_raw = pair["src_pts"][0], pair["tgt_pts"][0]
    T_sel = torch.eye(4); T_sel[:3, :3], T_sel[:3, 3] = unset["R_sel"][0], unset["t_sel"][0]
    # unset: the parent's path, an IcpJob, which returns what the plain call returns from the selected transform on the device
    plain = ops.icp_point_to_point(src_raw, tgt_raw, T_sel.to(gpu).contiguous(), max_corr, max_it)
    assert torch.equal(unset["T_est"][0], torch.from_numpy(plain.transformation).float())
    sizes = [1.2, 0.6, 0]
    for estimation in ("point_to_point", "plane_to_plane"):
        multi = run(icp_voxel_sizes=sizes, icp_estimation=estimation)
        assert torch.equal(multi["R_sel"], unset["R_sel"]) and torch.equal(multi["t_sel"], unset["t_sel"])     # same selection, same RNG use
        want = ops.icp_multi_scale(src_raw, tgt_raw, T_sel.to(gpu).contiguous(), sizes, [max(2.4, max_corr), max(1.2, max_corr), max_corr],
                                   [max_it] * 3, estimation=estimation)
        assert len(want.levels) == 3 and want.levels[0].n_src < want.levels[2].n_src == src_raw.shape[0]
        assert torch.equal(multi["T_est"][0], torch.from_numpy(want.transformation).float()), estimation
        serial = evaluate_pairs([pair], SimpleNamespace(**vars(args), icp_voxel_sizes=sizes, icp_estimation=estimation),
                                rng=np.random.RandomState(0), overlap=False)
        assert torch.equal(serial["T_est"], multi["T_est"])
        print(f"{estimation}: levels {[(lv.n_src, lv.n_tgt, lv.iterations) for lv in want.levels]}, rte {float(multi['rte'][0]):.4f} m "
              f"(single scale {float(unset['rte'][0]):.4f} m)")


def test_bad_arguments(gpu):
    from umeregrobust_amd import ops
    from umeregrobust_amd.evaluate import refine_registration
    src, tgt, gt, T0 = ms.case()
    s_, t_ = T_(src[:300], gpu), T_(tgt[:400], gpu)
    run = lambda *a, **kw: ops.icp_multi_scale(s_, t_, T0, *a, **kw)       # noqa: E731
    for a in (((), (), ()), ((0.8, 0.4), (1.6,), (30, 30)), ((0.4, 0.8), (1.6, 0.8), (30, 30)), ((0.0, 0.4), (1.6, 0.8), (30, 30)),
              ((0.8, 0.4), (1.6, -0.8), (30, 30)), ((0.8, 0.4), (1.6, 0.8), (30, 2.5)), ([0.9 - 0.1 * k for k in range(9)], [1.0] * 9, [3] * 9)):
        with pytest.raises(ValueError):
            run(*a)
    with pytest.raises(ValueError, match="icp_estimation"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="colored")
    with pytest.raises(ValueError, match="knn"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="point_to_plane", normal_knn=65)
    with pytest.raises(ValueError, match="epsilon"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="plane_to_plane", epsilon=2.0)
    with pytest.raises(ValueError, match="4x4"):
        ops.icp_multi_scale(s_, t_, np.eye(3), (0.8, 0), (1.6, 0.2), (3, 3))        # (the plain call's own rule, at level 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.icp_multi_scale(s_.cpu(), t_, T0, (0.8, 0), (1.6, 0.2), (3, 3))
    with pytest.raises(ValueError, match="strictly decreasing"):
        refine_registration([T0[:3, :3]], [T0[:3, 3]], SimpleNamespace(icp_voxel_sizes=[0.4, 0.8]), [(s_, t_, torch.eye(4))])
    # the library still works afterwards
    assert run((0.8, 0), (1.6, 0.2), (3, 3)).iterations > 0
