"""GPU: the open-addressing table of csrc/voxel.hip at its own edges (its compaction has tests/test_compact_edges_gpu.py).

Every cloud comes from tests/glue_cases.py, which tests/test_voxel_key_cpu.py holds against the header: probes that wrap past the
last slot, one probe chain of 300 cells with every cell twice, the capacity switch at 2 n = 2^k, the +-(2^20 - 1) key range with its
21-bit fields, and the fp32 quotient within an ulp of 8 193 voxel boundaries per voxel size.  The reference everywhere is numpy's
`unique` over the rows of floor(pts / float32(voxel)); results are compared with `==`."""
import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu


def thin(pts, voxel, gpu):
    from umeregrobust_amd import ops
    got = ops.voxel_first_index(torch.from_numpy(pts).to(gpu), voxel).cpu().numpy()
    assert got.dtype == np.int64
    return got


def test_probes_wrap_past_the_last_slot(gpu):
    pts = gc.wrap_cloud()
    assert np.array_equal(thin(pts, gc.CELL_VOXEL, gpu), np.arange(600))
    twice = np.concatenate([pts[:400], pts[::-1]])                                    # 1000 points, still 2048 slots
    assert gc.capacity(len(twice)) == 2048
    assert np.array_equal(thin(twice, gc.CELL_VOXEL, gpu), gc.first_of_every_voxel(twice, gc.CELL_VOXEL))


@pytest.mark.parametrize("cap", (2048, 4096))
def test_one_chain_of_300_cells_drops_every_second_copy(gpu, cap):
    pts = gc.chain_cloud(cap)
    want = gc.first_of_every_voxel(pts, gc.CELL_VOXEL)
    assert len(want) == 600
    got = thin(pts, gc.CELL_VOXEL, gpu)
    assert np.array_equal(got, want)
    assert np.array_equal(thin(pts, gc.CELL_VOXEL, gpu), got)                          # whatever order the insertions took


@pytest.mark.parametrize("n", gc.CAPACITY_N[1:])
def test_all_distinct_at_the_capacity_switch(gpu, n):
    pts = gc.distinct_cloud(n)
    assert np.array_equal(thin(pts, gc.CELL_VOXEL, gpu), np.arange(n))


def test_key_range_and_fields(gpu):
    pts = gc.range_cloud()
    want = gc.first_of_every_voxel(pts, 1.0)
    assert 2 * len(want) == len(pts)
    assert np.array_equal(thin(pts, 1.0, gpu), want)


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("sign", (1, -1))
def test_one_cell_beyond_the_key_range_raises(gpu, axis, sign):
    from umeregrobust_amd import ops
    inside = gc.range_cloud()
    bad = np.concatenate([inside[:7], gc.beyond_range_point(axis, sign), inside[7:]])
    with pytest.raises(ValueError, match="beyond 2\\^20 voxels"):
        ops.voxel_first_index(torch.from_numpy(bad).to(gpu), 1.0)


@pytest.mark.parametrize("i", range(len(gc.SWEEP_VOXELS)))
def test_quotient_within_an_ulp_of_every_voxel_boundary(gpu, i):
    voxel = gc.SWEEP_VOXELS[i]
    pts = gc.sweep_cloud(voxel, gc.sweep_axis(i))
    want = gc.first_of_every_voxel(pts, voxel)
    print(f"voxel {voxel}: {len(pts)} points, {len(want)} voxels")
    assert 2 * gc.SWEEP_K < len(want) <= 2 * gc.SWEEP_K + 3
    assert np.array_equal(thin(pts, voxel, gpu), want)


def test_voxel_thinning_is_voxel_first_index_read_later(gpu):
    from umeregrobust_amd import ops
    a = torch.from_numpy(gc.sweep_cloud(0.3, 0)).to(gpu)
    b = torch.from_numpy(gc.chain_cloud(2048)).to(gpu)
    want = ops.voxel_first_index(a, 0.3, b, gc.CELL_VOXEL)
    later = ops.VoxelThinning(a, 0.3, b, gc.CELL_VOXEL)
    between = ops.voxel_first_index(b, gc.CELL_VOXEL)                                    # the workspace is reused before result()
    got = later.result()
    assert len(got) == 2 and all(g.dtype == torch.int64 and torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(between, want[1])
    assert np.array_equal(got[0].cpu().numpy(), gc.first_of_every_voxel(a.cpu().numpy(), 0.3))
    assert np.array_equal(got[1].cpu().numpy(), gc.first_of_every_voxel(b.cpu().numpy(), gc.CELL_VOXEL))
    # a NaN in the second cloud: the same error from both forms
    b_nan = b.clone()
    b_nan[417, 1] = float("nan")
    with pytest.raises(ValueError) as now:
        ops.voxel_first_index(a, 0.3, b_nan, gc.CELL_VOXEL)
    with pytest.raises(ValueError) as deferred:
        ops.VoxelThinning(a, 0.3, b_nan, gc.CELL_VOXEL).result()
    assert str(now.value) == str(deferred.value) and "NaN" in str(now.value)
