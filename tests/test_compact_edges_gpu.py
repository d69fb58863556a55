"""GPU: the stream compaction of voxel thinning, ground-truth matches and the device collate at its own edges.  All three
compact by 1024-row blocks (waves of 64 rows) and scan the block counts with one block of 1024 threads: up to 1024 blocks
(1024 * 1024 rows) a scanning thread owns one count, with one more block it owns two.  Every comparison is `==` against the
CPU restatement the unit's own tests use: numpy's `unique` on the fp32 quotient (voxel), the brute-force fp64 search of
tests/train_data_ref.py (matches), the host collate `batch_collate_fn_dset` (collate).

(The coordinate maps of the feature network compact the same way; tests/test_featnet_edges_gpu.py gates them at their block
edges.  A network run of more than 2^20 rows is no test of a few seconds.)"""
import functools

import numpy as np
import pytest
import torch

import train_data_ref as ref
from test_collate_gpu import assert_same, make_item, on_device, same_state

pytestmark = pytest.mark.gpu

BLOCK = 1024
AROUND_A_WAVE_AND_A_BLOCK = (1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17)
AROUND_THE_SCAN_CHUNK = (1024 * 1024, 1024 * 1024 + 1, 2 * 1024 * 1024 + 1024 + 5)
SIZES = AROUND_A_WAVE_AND_A_BLOCK + AROUND_THE_SCAN_CHUNK


# ---- 1. voxel thinning -----------------------------------------------------------------------------------------------------

VOXEL = 0.3


def points_of_cells(cell, rng):
    """One point per entry of `cell` (a voxel number), somewhere well inside that voxel; negative coordinates included."""
    cell = np.asarray(cell, dtype=np.int64)
    q = np.stack([cell % 128 - 64, (cell // 128) % 128 - 64, cell // 16384 - 3], axis=1)
    return ((q + rng.uniform(0.1, 0.9, q.shape)) * VOXEL).astype(np.float32)


def first_of_every_voxel(pts):
    """tests/test_gpu_parity.py::test_voxel_first_index_vs_numpy's reference, the three cell indices packed into one int64."""
    q = np.floor(pts / np.float32(VOXEL)).astype(np.int64) + (1 << 20)
    assert (q >= 0).all() and (q < (1 << 21)).all()
    _, first = np.unique((q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2], return_index=True)
    return np.sort(first)


def voxel_first_index(pts, gpu):
    from umeregrobust_amd import ops
    got = ops.voxel_first_index(torch.from_numpy(pts).to(gpu), VOXEL).cpu().numpy()
    assert got.dtype == np.int64
    return got


@pytest.mark.parametrize("n", SIZES)
def test_voxel_first_index_at_wave_block_and_scan_edges(gpu, n):
    rng = np.random.RandomState(n % 9973)
    pts = points_of_cells(rng.randint(0, max(1, n // 2), n), rng)         # twice as many points as voxels: some kept, some not
    want = first_of_every_voxel(pts)
    print(f"n = {n}: {len(want)} voxels")
    if n >= 64:
        assert 0 < len(want) < n
    assert np.array_equal(voxel_first_index(pts, gpu), want)


# the voxel number of point i; index 0 is always the first of its voxel, so it is a representative in every pattern
PATTERNS = {
    "every_point_its_own_voxel": (lambda i: i, lambda n: n),
    "all_points_in_one_voxel": (lambda i: 0 * i, lambda n: 1),
    "only_in_the_last_wave_of_a_block": (lambda i: np.where(i % BLOCK >= BLOCK - 64, i, 0), lambda n: 1 + 64 * (n // BLOCK)),
    "only_in_the_first_lane_of_a_wave": (lambda i: np.where(i % 64 == 0, i, 0), lambda n: (n + 63) // 64),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_voxel_first_index_where_the_representatives_sit(gpu, pattern):
    n = 3 * BLOCK + 17
    cell_of, kept = PATTERNS[pattern]
    pts = points_of_cells(cell_of(np.arange(n)), np.random.RandomState(len(pattern)))
    want = first_of_every_voxel(pts)
    assert len(want) == kept(n)
    assert np.array_equal(voxel_first_index(pts, gpu), want)


# ---- 2. ground-truth matches -------------------------------------------------------------------------------------------------

RADIUS = 0.3


def nearest_source_in_slices(tgt, src, step=1 << 16):
    """ref.nearest(tgt, src) with the sources taken a slice at a time: lowest index of minimal d2 (a later slice wins only
    with a strictly smaller distance)."""
    best_j, best_d2 = np.zeros(len(tgt), np.int64), np.full(len(tgt), np.inf)
    for a in range(0, len(src), step):
        j, d2, _ = ref.nearest(tgt, src[a:a + step])
        better = d2 < best_d2
        best_j[better], best_d2[better] = j[better] + a, d2[better]
    return best_j, best_d2


@functools.lru_cache(maxsize=2)
def match_case(n_src):
    """A handful of targets; every second source (at random) within the radius of one of them, the others spread over a box
    in which a hit is rare.  -> (src, tgt, one-side rows, mutual rows) by the restatement."""
    rng = np.random.RandomState(n_src % 9973)
    n_tgt = min(8, n_src)
    tgt = rng.uniform(-20, 20, (n_tgt, 3)).astype(np.float32)
    near = rng.rand(n_src) < 0.5
    near[0] = True
    src = rng.uniform(-40, 40, (n_src, 3))
    src[near] = tgt[rng.randint(0, n_tgt, int(near.sum()))] + rng.uniform(-0.15, 0.15, (int(near.sum()), 3))
    src = src.astype(np.float32)
    one = ref.one_side(src, tgt, None, RADIUS)
    j, d2 = nearest_source_in_slices(tgt, src)                       # ref.mutual's reverse side, in slices of the source
    back = np.where(d2 < RADIUS * RADIUS, j, -1)
    return src, tgt, one, one[back[one[:, 1]] == one[:, 0]].reshape(-1, 2)


@pytest.mark.parametrize("n_src", SIZES)
def test_gt_matches_at_wave_block_and_scan_edges(gpu, n_src):
    from umeregrobust_amd import gt_matches
    src, tgt, want_one, want_mut = match_case(n_src)
    print(f"n_src = {n_src}, n_tgt = {len(tgt)}: {len(want_one)} one-side rows, {len(want_mut)} mutual rows")
    if n_src >= 64:
        assert 0 < len(want_mut) <= len(tgt) < len(want_one) < n_src, "kept and dropped rows must both occur"
    s, t = torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)
    got = gt_matches.one_side(s, t, None, RADIUS).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want_one)
    got = gt_matches.mutual(s, t, None, None, RADIUS).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want_mut)


# ---- 3. device collate -------------------------------------------------------------------------------------------------------

N_SRC, N_ROWS = 700, 4000


@pytest.mark.parametrize("nt", SIZES)
def test_device_collate_at_wave_block_and_scan_edges(gpu, nt):
    """The compaction runs over the TARGET cloud.  A third of the match rows name targets anywhere, a third targets of the last
    blocks, a third targets around row 1024 * 1024; the cap does not bind, so every point and every survivor is kept."""
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    from umeregrobust_amd.datasets import batch_collate_fn_dset
    rng = np.random.RandomState(nt % 9973)
    item = make_item(rng, N_SRC, nt, N_ROWS)
    mid = min(nt, BLOCK * BLOCK)
    t = np.concatenate([rng.randint(0, nt, N_ROWS - 2 * (N_ROWS // 3)), rng.randint(max(0, nt - 1100), nt, N_ROWS // 3),
                        rng.randint(max(0, mid - 1100), min(nt, mid + 1100), N_ROWS // 3)])
    rows = np.stack([rng.randint(0, N_SRC, N_ROWS), rng.permutation(t)], axis=1).astype(np.int64)
    item = item[:8] + (torch.from_numpy(rows),)
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    want = batch_collate_fn_dset([item], num_matches=10 ** 6, max_pc_size=1 << 22, rng=a)
    got = batch_collate_fn_dset_device(on_device([item], gpu), num_matches=10 ** 6, max_pc_size=1 << 22, rng=b)
    print(f"nt = {nt}: clouds {tuple(want[0].shape)} / {tuple(want[4].shape)}, matches {tuple(want[10].shape)}")
    assert tuple(want[4].shape) == (1, nt, 3) and want[10].shape[1] > 0, "every target kept, some matches survive"
    assert_same(got, want)
    assert same_state(a.get_state(), b.get_state())
