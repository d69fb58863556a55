"""Coarse-to-fine ICP without a GPU: the argument rules of umeregrobust_amd/icp_multiscale.py, `levels_of(args)`, the hand-over between
levels (with recording stand-ins for the three ops, in the manner of test_sync_wrappers_pass_fitness_before_rmse), and the
qualification of the inputs tests/test_icp_multiscale_gpu.py judges the library on: the basin numbers and the stop-rule margin of the
fp64 restatements (tests/icp_multiscale_ref.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icp_plane_ref as plane
from tests import icp_multiscale_ref as ms


# ---- argument rules ------------------------------------------------------------------------------------------------------------------

def test_argument_rules():
    from umeregrobust_amd import icp_multiscale as m
    ok = m.check_levels("t", (0.8, 0.4, 0), (1.6, 0.8, 0.2), (30, 20, 10))
    assert ok == [(0.8, 1.6, 30), (0.4, 0.8, 20), (0.0, 0.2, 10)]
    assert m.check_levels("t", [0.5], [1.0], [7]) == [(0.5, 1.0, 7)]
    assert m.check_levels("t", [0], [0.2], [7]) == [(0.0, 0.2, 7)]
    assert m.check_levels("t", [0.4, -1.0], [0.8, 0.2], [7, 0]) == [(0.4, 0.8, 7), (0.0, 0.2, 0)]        # negative: stored as 0
    assert len(m.check_levels("t", np.linspace(0.8, 0.1, 8), [0.5] * 8, [3] * 8)) == 8
    assert m.check_voxel_sizes("t", np.array([0.8, 0.4])) == [0.8, 0.4]
    bad = [
        ((), (), ()),                                                   # no level
        (np.linspace(0.9, 0.1, 9), [0.5] * 9, [3] * 9),                 # nine
        ((0.8, 0.4), (1.6,), (30, 30)),                                 # lengths
        ((0.8, 0.4), (1.6, 0.8), (30,)),
        ((0.8,), (1.6, 0.8), (30, 30)),
        ((0.4, 0.8), (1.6, 0.8), (30, 30)),                             # increasing
        ((0.4, 0.4), (1.6, 0.8), (30, 30)),                             # not strictly decreasing
        ((0.0, 0.4), (1.6, 0.8), (30, 30)),                             # the zero anywhere but last
        ((-0.8, 0.4), (1.6, 0.8), (30, 30)),
        ((0.8, 0.0, 0.0), (1.6, 0.8, 0.2), (30, 30, 30)),
        ((0.8, float("nan")), (1.6, 0.8), (30, 30)),
        ((float("inf"), 0.4), (1.6, 0.8), (30, 30)),
        ((0.8, "0.4"), (1.6, 0.8), (30, 30)),
        ((True, 0.4), (1.6, 0.8), (30, 30)),
        ((1e-50, 0.0), (1.6, 0.8), (30, 30)),                           # zero as an f32
        ((0.8, 0.4), (1.6, 0.0), (30, 30)),                             # distances
        ((0.8, 0.4), (1.6, -0.8), (30, 30)),
        ((0.8, 0.4), (1.6, float("nan")), (30, 30)),
        ((0.8, 0.4), (1.6, None), (30, 30)),
        ((0.8, 0.4), (1.6, 0.8), (30, -1)),                             # iteration limits
        ((0.8, 0.4), (1.6, 0.8), (30, 2.5)),
        ((0.8, 0.4), (1.6, 0.8), (30, True)),
        ("0.8", (1.6,), (30,)),                                         # not sequences
        (0.8, 1.6, 30),
    ]
    for sizes, dists, iters in bad:
        with pytest.raises(ValueError):
            m.check_levels("t", sizes, dists, iters)
    for v in (0, -1.0, float("nan"), float("inf"), None, "1", True, 1e-50):
        with pytest.raises(ValueError, match="voxel_size"):
            m.check_voxel_size("t", v)


def test_entry_points_check_arguments_before_any_tensor_or_library(monkeypatch):
    """every rule fires with host tensors and without a library: neither is looked at before the arguments are"""
    from umeregrobust_amd import _lib, icp_multiscale as m, ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    s, t = torch.zeros(5, 3), torch.zeros(7, 3)
    for v in (0, -0.3, float("nan"), None):
        with pytest.raises(ValueError, match="voxel_size"):
            ops.voxel_down_sample(s, v)
    with pytest.raises(ValueError, match="strictly decreasing"):
        ops.voxel_pyramid(s, t, (0.4, 0.8))
    with pytest.raises(ValueError, match="1 to 8"):
        ops.voxel_pyramid(s, t, ())
    run = lambda *a, **kw: ops.icp_multi_scale(s, t, np.eye(4), *a, **kw)       # noqa: E731
    with pytest.raises(ValueError, match="one entry per level"):
        run((0.8, 0.4), (1.6,), (30, 30))
    with pytest.raises(ValueError, match="strictly decreasing"):
        run((0.4, 0.8), (1.6, 0.8), (30, 30))
    with pytest.raises(ValueError, match="icp_estimation"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="point_to_line")
    with pytest.raises(ValueError, match="knn"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="point_to_plane", normal_knn=2)
    with pytest.raises(ValueError, match="normal_radius"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="plane_to_plane", normal_radius=0.0)
    with pytest.raises(ValueError, match="epsilon"):
        run((0.8, 0), (1.6, 0.2), (30, 30), estimation="plane_to_plane", epsilon=0.0)
    # clouds: the type and the shape before the device
    with pytest.raises(TypeError):
        ops.voxel_down_sample(np.zeros((5, 3), np.float32), 0.3)
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        ops.voxel_down_sample(torch.zeros(5, 4), 0.3)
    with pytest.raises(ValueError, match="2\\^20"):
        ops.voxel_down_sample(torch.zeros(0, 3), 0.3)
    with pytest.raises(ValueError, match="2\\^20"):
        ops.voxel_down_sample(torch.zeros(m.MAX_POINTS + 1, 3), 0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.voxel_down_sample(s, 0.3)
    assert ops.icp_multi_scale is m.icp_multi_scale and ops.voxel_down_sample is m.voxel_down_sample and ops.voxel_pyramid is m.voxel_pyramid


def test_levels_of_args():
    from umeregrobust_amd import icp_multiscale as m
    assert m.levels_of(SimpleNamespace()) is None
    assert m.levels_of(SimpleNamespace(icp_voxel_sizes=None, icp_level_distances=None, icp_level_iterations=None)) is None
    # defaults: max(2 voxel, the single-scale distance), that distance on the level of voxel size 0, the single-scale limit everywhere
    assert m.levels_of(SimpleNamespace(icp_voxel_sizes=[0.8, 0.4, 0])) == [(0.8, 1.6, 200), (0.4, 0.8, 200), (0.0, 0.2, 200)]
    got = m.levels_of(SimpleNamespace(icp_voxel_sizes=(0.8, 0.2, 0.1), icp_max_correspondence_distance=0.5, icp_max_iteration=40))
    assert got == [(0.8, 1.6, 40), (0.2, 0.5, 40), (0.1, 0.5, 40)]
    # explicit
    got = m.levels_of(SimpleNamespace(icp_voxel_sizes=[0.8, 0], icp_level_distances=[1.0, 0.3], icp_level_iterations=[5, 9]))
    assert got == [(0.8, 1.0, 5), (0.0, 0.3, 9)]
    got = m.levels_of(SimpleNamespace(icp_voxel_sizes=[0.8, 0], icp_level_iterations=[5, 9]))
    assert got == [(0.8, 1.6, 5), (0.0, 0.2, 9)]
    for kw in (dict(icp_voxel_sizes=[0.4, 0.8]), dict(icp_voxel_sizes=[0.8, 0.4], icp_level_distances=[1.0]),
               dict(icp_voxel_sizes=[0.8], icp_level_iterations=[1, 2]), dict(icp_level_distances=[1.0]), dict(icp_level_iterations=[3])):
        with pytest.raises(ValueError):
            m.levels_of(SimpleNamespace(**kw))
    assert m.parse_list("0.8,0.4,0") == [0.8, 0.4, 0.0] and m.parse_list("30, 20,10", int) == [30, 20, 10]


# ---- the hand-over between levels ------------------------------------------------------------------------------------------------------

def _stand_ins(monkeypatch):
    from umeregrobust_amd import icp_multiscale as m, ops
    calls = []
    step = np.eye(4)
    step[:3, 3] = (0.1 + 2.0 ** -40, -(0.3 + 2.0 ** -41), 2.0 ** -45)              # does not survive a trip through float32

    def result(T):
        T = np.asarray(T.cpu() if isinstance(T, torch.Tensor) else T, np.float64)
        k = len(calls) - 1                               # (the call was recorded first)
        return SimpleNamespace(transformation=step @ T, fitness=0.5 + 0.1 * k, inlier_rmse=0.05 - 0.01 * k, iterations=3 + k)

    def p2p(s, t, T, d, it, rf=1e-6, rr=1e-6):
        calls.append(("point_to_point", s, t, T, d, it, rf, rr))
        return result(T)

    def p2l(s, t, nt, T, d, it, rf=1e-6, rr=1e-6):
        calls.append(("point_to_plane", s, t, T, d, it, rf, rr, nt))
        return result(T)

    def gicp(s, t, ns, nt, T, d, it, rf=1e-6, rr=1e-6, epsilon=1e-3):
        calls.append(("plane_to_plane", s, t, T, d, it, rf, rr, ns, nt, epsilon))
        return result(T)
    monkeypatch.setattr(ops, "icp_point_to_point", p2p)
    monkeypatch.setattr(ops, "icp_point_to_plane", p2l)
    monkeypatch.setattr(ops, "icp_plane_to_plane", gicp)
    monkeypatch.setattr(ops, "estimate_normals", lambda p, knn=30, radius=None: ("normals of", p, knn, radius))
    levels = [(torch.zeros(4, 3), torch.zeros(5, 3)), (torch.zeros(14, 3), torch.zeros(15, 3)), (torch.zeros(24, 3), torch.zeros(25, 3))]
    monkeypatch.setattr(m, "voxel_pyramid", lambda s, t, sizes: levels[:len(sizes)])
    return calls, step, levels


@pytest.mark.parametrize("estimation", ms.ESTIMATIONS)
def test_every_level_starts_from_the_unrounded_transform_of_the_one_before(monkeypatch, estimation):
    from umeregrobust_amd import ops
    calls, step, levels = _stand_ins(monkeypatch)
    T0 = np.eye(4)
    T0[:3, 3] = (1.0 + 2.0 ** -50, 2.0, 3.0)
    s, t = torch.zeros(24, 3), torch.zeros(25, 3)
    out = ops.icp_multi_scale(s, t, T0, (0.8, 0.4, 0), (1.6, 0.8, 0.2), (11, 12, 13), estimation=estimation, normal_knn=17, normal_radius=0.9,
                              epsilon=0.01, relative_fitness=1e-5, relative_rmse=1e-7)
    assert [c[0] for c in calls] == [estimation] * 3
    want = T0
    for k, c in enumerate(calls):
        assert c[1] is levels[k][0] and c[2] is levels[k][1]
        assert isinstance(c[3], np.ndarray) and c[3].dtype == np.float64 and np.array_equal(c[3], want), k       # fp64, bit for bit
        assert (c[4], c[5]) == ((1.6, 0.8, 0.2)[k], (11, 12, 13)[k])                                         # its own distance and limit
        assert (c[6], c[7]) == (1e-5, 1e-7)
        if estimation == "point_to_plane":
            assert c[8] == ("normals of", levels[k][1], 17, 0.9)                                              # re-estimated on the level's target
        if estimation == "plane_to_plane":
            assert c[8] == ("normals of", levels[k][0], 17, 0.9) and c[9] == ("normals of", levels[k][1], 17, 0.9) and c[10] == 0.01
        want = step @ want
    assert not np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert np.array_equal(out.transformation, want) and out.iterations == 3 + 4 + 5
    assert (out.fitness, out.inlier_rmse) == (out.levels[2].fitness, out.levels[2].inlier_rmse) == (0.5 + 0.2, 0.05 - 0.02)
    for k, lv in enumerate(out.levels):
        assert (lv.voxel_size, lv.max_correspondence_distance, lv.n_src, lv.n_tgt) == ((0.8, 0.4, 0.0)[k], (1.6, 0.8, 0.2)[k], 4 + 10 * k, 5 + 10 * k)
        assert lv.iterations == 3 + k and lv.transformation is not None
    assert np.array_equal(out.levels[0].transformation, step @ T0)


def test_level_zero_takes_a_device_style_start_and_a_single_zero_level_is_the_plain_call(monkeypatch):
    from umeregrobust_amd import icp_multiscale as m, ops
    calls, step, levels = _stand_ins(monkeypatch)
    monkeypatch.setattr(m, "voxel_pyramid", lambda *a: pytest.fail("a single level of voxel size 0 builds no pyramid"))
    s, t = torch.zeros(24, 3), torch.zeros(25, 3)
    T0 = torch.eye(4)                                   # (stands for the device f32 tensor: it must reach the first call as it is)
    out = ops.icp_multi_scale(s, t, T0, [0], [0.2], [30])
    (c,) = calls
    assert c[1] is s and c[2] is t and c[3] is T0 and (c[4], c[5]) == (0.2, 30)
    assert out.iterations == 3 and len(out.levels) == 1 and (out.levels[0].n_src, out.levels[0].n_tgt) == (24, 25)


def test_refine_registration_hands_the_levels_over(monkeypatch):
    from umeregrobust_amd import evaluate, ops
    seen = []

    def fake(s, t, T, sizes, dists, iters, **kw):
        seen.append((T.copy(), tuple(sizes), tuple(dists), tuple(iters), kw))
        return SimpleNamespace(transformation=np.eye(4))
    monkeypatch.setattr(ops, "icp_multi_scale", fake)
    monkeypatch.setattr(evaluate, "relative_rotation_error", lambda a, b: torch.zeros(1))
    s, t = torch.zeros(5, 3), torch.zeros(7, 3)
    args = SimpleNamespace(icp_voxel_sizes=[0.8, 0], icp_estimation="plane_to_plane", icp_normal_knn=12, icp_gicp_epsilon=0.01,
                           icp_max_iteration=9)
    evaluate.refine_registration([np.eye(3)], [np.array([1.0, 2.0, 3.0])], args, [(s, t, torch.eye(4))])
    (T, sizes, dists, iters, kw), = seen
    assert T[:3, 3].tolist() == [1.0, 2.0, 3.0] and sizes == (0.8, 0.0) and dists == (1.6, 0.2) and iters == (9, 9)
    assert kw == dict(estimation="plane_to_plane", normal_knn=12, normal_radius=None, epsilon=0.01)


# ---- the qualification of the GPU inputs -----------------------------------------------------------------------------------------------

def test_the_basin_of_the_case():
    """single scale at 0.2 m stays where it started looking; three levels arrive (observed 0.551 m against 0.021 m / 0.126 deg)"""
    src, tgt, gt, T0 = ms.case()
    assert [tuple(map(len, lv)) for lv in ms.pyramid()] == [(401, 570), (1247, 1691), (3000, 3000)]
    T, fit, rmse, it = ms.single_scale()
    print(f"single scale: {it} updates, fitness {fit:.3f}, {plane.trans_err(T, gt):.3f} m from the truth (start: {plane.trans_err(T0, gt):.3f} m)")
    assert plane.trans_err(T, gt) > 0.4 and it < ms.SINGLE_ITERATIONS
    for estimation in ms.ESTIMATIONS:
        levels = ms.coarse_to_fine(estimation)
        T = levels[-1][0]
        print(f"{estimation}: {[lv[3] for lv in levels]} updates, {plane.trans_err(T, gt):.4f} m / {plane.rot_err_deg(T, gt):.4f} deg")
        assert plane.trans_err(T, gt) < 0.1 and plane.rot_err_deg(T, gt) < 0.5
    assert [lv[3] for lv in ms.coarse_to_fine("point_to_point")] == [22, 18, 18]


def test_the_stop_rule_margin_of_the_case():
    """At every evaluation of every level of every estimation, both differences are farther than 1e-8 from their threshold: ten times the
    1e-9 the GPU gate allows the rmse to differ by (the fitness is a ratio of small integers: it is equal or 1/n apart).  A library that
    passes the gate therefore takes the same stop decisions.  Smallest observed: 4.1e-7 point to point, 2.1e-7 point to plane, 4.7e-8
    plane to plane.  Also the precondition of the gate for the two normal-based estimations: cond(J^T J) <= 1e4."""
    for estimation in ms.ESTIMATIONS:
        margins, conds = [], []
        for T, fit, rmse, it, trace, cond in ms.coarse_to_fine(estimation):
            assert trace[0][3] is None and len(trace) == it + 1
            margins += [abs(rec[k] - 1e-6) for rec in trace[1:] for k in (3, 4)]
            conds += cond
        print(f"{estimation}: smallest stop-rule margin {min(margins):.2e}, largest cond {max(conds, default=0.0):.0f}")
        assert min(margins) > 1e-8
        assert max(conds, default=0.0) <= 1e4
