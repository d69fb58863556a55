"""ops.voxel_down_sample / ops.voxel_pyramid (csrc/voxel_centroid.hip) against the numpy mirror (tests/voxel_centroid_ref.py, which
tests/test_voxel_centroid_cpu.py holds against the header itself): centroids, first indices and counts, bit for bit.  The sums are
integers, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import glue_cases as gc
from tests import voxel_centroid_ref as vc

pytestmark = pytest.mark.gpu


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(gpu, pts, voxel, tag):
    from umeregrobust_amd import ops
    cen, first, count = vc.down_sample(pts, voxel)
    got = ops.voxel_down_sample(T_(pts, gpu), voxel, return_info=True)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32, tag
    assert torch.equal(got[1].cpu(), torch.from_numpy(first)), tag
    assert torch.equal(got[2].cpu(), torch.from_numpy(count)), tag
    assert torch.equal(got[0].cpu(), torch.from_numpy(cen)), (tag, np.abs(got[0].cpu().numpy() - cen).max())
    assert got[0].cpu().numpy().tobytes() == cen.tobytes(), tag                           # (torch.equal takes -0.0 for 0.0)
    assert torch.equal(ops.voxel_down_sample(T_(pts, gpu), voxel), got[0]), tag
    assert torch.equal(ops.voxel_first_index(T_(pts, gpu), voxel), got[1]), tag         # the rows are voxel_first_index's
    return got


def test_one_point_and_two_points_in_one_voxel(gpu):
    got = same(gpu, np.float32([[1.25, -2.5, 0.75]]), 0.3, "n = 1")
    assert got[0].shape == (1, 3) and got[2].tolist() == [1]
    got = same(gpu, np.float32([[1.21, -2.5, 0.75], [1.29, -2.45, 0.77]]), 0.3, "two in one")
    assert got[0].shape == (1, 3) and got[2].tolist() == [2]
    got = same(gpu, np.float32([[1.21, -2.5, 0.75], [1.81, -2.45, 0.77]]), 0.3, "two in two")
    assert got[2].tolist() == [1, 1]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 3000])
def test_the_compaction_block_with_four_points_per_voxel(gpu, n):
    pts = vc.dense_cloud(n)
    got = same(gpu, pts, 0.3, f"dense n={n}")
    assert 2.0 < n / got[0].shape[0] < 8.0


def test_worst_contention_and_none(gpu):
    got = same(gpu, vc.one_voxel_cloud(3000), 0.3, "3000 points in one voxel")
    assert got[2].tolist() == [3000]
    pts = gc.distinct_cloud(3000)
    got = same(gpu, pts, gc.CELL_VOXEL, "3000 points in 3000 voxels")
    assert got[0].shape[0] == 3000 and torch.equal(got[0].cpu(), torch.from_numpy(pts))   # exact cell centres come back as they are


def test_far_from_the_origin_and_the_ends_of_the_key_range(gpu):
    got = same(gpu, vc.far_cloud(), 0.3, "coordinates ~1e5")
    assert got[2].max() > 1
    pts = gc.range_cloud()
    got = same(gpu, pts, 1.0, "cells at +-(2^20 - 1)")
    assert got[2].tolist() == [2] * (len(pts) // 2)


def test_boundaries_and_their_neighbours(gpu):
    for voxel in (0.3, 0.25, 0.8, 0.4):
        same(gpu, vc.boundary_cloud(voxel), voxel, f"p = k v, v={voxel}")
    for i, voxel in enumerate(gc.SWEEP_VOXELS):
        same(gpu, gc.sweep_cloud(voxel, gc.sweep_axis(i)), voxel, f"sweep v={voxel}")


@pytest.mark.parametrize("cap", [2048, 4096])
def test_probe_chain_of_300_cells(gpu, cap):
    same(gpu, gc.chain_cloud(cap), gc.CELL_VOXEL, f"chain cap={cap}")
    if cap == 2048:
        same(gpu, gc.wrap_cloud(), gc.CELL_VOXEL, "wrap")


def test_equal_bits_on_a_workspace_of_garbage_and_guard_rows(gpu):
    """The call twice with the workspace filled with 0xA5 in between: nothing is read that the call did not write.  The native entry
    on guarded buffers: rows at and beyond m keep their guard values, and so does everything around the three outputs."""
    from umeregrobust_amd import _lib, icp_multiscale as m, ops
    pts = T_(vc.dense_cloud(3000, seed=7), gpu)
    a = ops.voxel_down_sample(pts, 0.3, return_info=True)
    keys = [k for k in ops._workspaces if k[2] == "voxel_centroid" and k[0] == gpu.index]
    assert keys
    for k in keys:
        ops._workspaces[k].fill_(0xA5)
    b = ops.voxel_down_sample(pts, 0.3, return_info=True)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    lib = m.load_native()
    n, pad = pts.shape[0], 64
    need = int(lib.umereg_voxel_centroid_workspace_bytes(n))
    assert need > 0 and lib.umereg_voxel_centroid_workspace_bytes(0) == 0 and lib.umereg_voxel_centroid_workspace_bytes(m.MAX_POINTS + 1) == 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=gpu)
    cen = torch.full((n + 2 * pad, 3), -7.5, dtype=torch.float32, device=gpu)
    first = torch.full((n + 2 * pad,), -77, dtype=torch.int64, device=gpu)
    counts = torch.full((n + 2 * pad,), -777, dtype=torch.int32, device=gpu)
    cnt = torch.full((2 + 2 * pad,), -7, dtype=torch.int32, device=gpu)
    _lib.call(gpu, lib.umereg_voxel_centroid_f32, pts.data_ptr(), n, 0.3, cen[pad:].data_ptr(), first[pad:].data_ptr(), counts[pad:].data_ptr(),
              cnt[pad:].data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(gpu))
    mm, bad = cnt[pad:pad + 2].tolist()
    assert bad == 0 and mm == a[0].shape[0] and 0 < mm < n
    assert torch.equal(cen[pad:pad + mm], a[0]) and torch.equal(first[pad:pad + mm], a[1]) and torch.equal(counts[pad:pad + mm], a[2])
    assert (cen[:pad] == -7.5).all() and (cen[pad + mm:] == -7.5).all()
    assert (first[:pad] == -77).all() and (first[pad + mm:] == -77).all()
    assert (counts[:pad] == -777).all() and (counts[pad + mm:] == -777).all()
    assert (cnt[:pad] == -7).all() and (cnt[pad + 2:] == -7).all()
    # a workspace one byte short is refused, and nothing is launched
    with pytest.raises(_lib.NativeCallError, match="workspace"):
        _lib.call(gpu, lib.umereg_voxel_centroid_f32, pts.data_ptr(), n, 0.3, cen[pad:].data_ptr(), first[pad:].data_ptr(),
                  counts[pad:].data_ptr(), cnt[pad:].data_ptr(), ws.data_ptr(), need - 1, _lib.stream_ptr(gpu))
    for bad_n in (0, m.MAX_POINTS + 1):
        with pytest.raises(_lib.NativeCallError, match="2\\^20"):
            _lib.call(gpu, lib.umereg_voxel_centroid_f32, pts.data_ptr(), bad_n, 0.3, cen[pad:].data_ptr(), first[pad:].data_ptr(),
                      counts[pad:].data_ptr(), cnt[pad:].data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(gpu))


def test_pyramid_equals_the_single_calls(gpu):
    from umeregrobust_amd import ops
    src, tgt = T_(vc.dense_cloud(3000, seed=8), gpu), T_(vc.dense_cloud(2500, seed=9), gpu)
    sizes = (1.2, 0.6, 0.3, 0.0)
    levels = ops.voxel_pyramid(src, tgt, sizes)
    assert len(levels) == 4
    for (s, t), v in zip(levels, sizes):
        assert torch.equal(s, ops.voxel_down_sample(src, v) if v else src), v
        assert torch.equal(t, ops.voxel_down_sample(tgt, v) if v else tgt), v
    assert levels[0][0].shape[0] < levels[1][0].shape[0] < levels[2][0].shape[0] < 3000
    only = ops.voxel_pyramid(src, tgt, [0.6])
    assert len(only) == 1 and torch.equal(only[0][0], levels[1][0]) and torch.equal(only[0][1], levels[1][1])
    # f64 input: converted like every op of the library converts it
    assert torch.equal(ops.voxel_down_sample(src.double(), 0.6), levels[1][0])


def test_bad_coordinates_and_bad_arguments(gpu):
    from umeregrobust_amd import ops
    pts = vc.dense_cloud(500)
    for value in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[123, 1] = value
        with pytest.raises(ValueError, match="NaN, infinite or beyond"):
            ops.voxel_down_sample(T_(p, gpu), 0.3)
    for axis in range(3):
        p = np.concatenate([np.float32([[5.5, -7.5, 9.5]]), gc.beyond_range_point(axis, -1)])
        with pytest.raises(ValueError, match="NaN, infinite or beyond"):
            ops.voxel_down_sample(T_(p, gpu), 1.0)
    with pytest.raises(ValueError, match="NaN, infinite or beyond"):
        ops.voxel_pyramid(T_(pts, gpu), T_(p, gpu), (2.0, 1.0))
    good = T_(pts, gpu)
    for v in (0, -0.3, float("nan"), None, "0.3"):
        with pytest.raises(ValueError, match="voxel_size"):
            ops.voxel_down_sample(good, v)
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        ops.voxel_down_sample(good[None], 0.3)
    with pytest.raises(ValueError, match="2\\^20"):
        ops.voxel_down_sample(good[:0], 0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.voxel_down_sample(good.cpu(), 0.3)
    with pytest.raises(ValueError, match="strictly decreasing"):
        ops.voxel_pyramid(good, good, (0.3, 0.3))
    # the library still works afterwards
    same(gpu, pts, 0.3, "after the errors")
