"""GPU: the ground-truth match kernels of include/umereg_gt_matches.h (csrc/gt_match.hip) against the brute-force fp64
restatement of their stated semantics (tests/train_data_ref.py) -- equality, no tolerance: shapes on both sides of every block
and wavefront size, with and without a transform, both grid geometries (half-radius cells / capped cells), the edge cases of the
radius test and of the tie rule, the mutual form, and the raw C entries twice between guard bands."""
import functools

import numpy as np
import pytest
import torch

import train_data_ref as ref
from test_abi_guard import Guard, rigid

pytestmark = pytest.mark.gpu

# (n_src, n_tgt) -> half extent of the target cloud [m]: (2, 2, 0.5) takes the half-radius cells at r = 0.3, the others the capped grid
SHAPES = {(1, 1): (1.0, 1.0, 1.0), (63, 65): (2.0, 2.0, 0.5), (257, 1000): (10.0, 10.0, 2.0), (5000, 4096): (40.0, 40.0, 3.0)}
RADIUS = 0.3


@functools.lru_cache(maxsize=None)
def case(n_src, n_tgt, with_T):
    """A pair with every kind of query: near twins of targets (noise around the radius), exact twins (d = 0, and duplicated
    targets, so exact ties), points of the same box without a twin, and points well outside the targets' box.  On a 0.05 m
    lattice when there is no transform, so that equal distances really occur."""
    rng = np.random.RandomState(1000 * n_src + n_tgt + int(with_T))
    ext = np.asarray(SHAPES[(n_src, n_tgt)])
    tgt = rng.uniform(-1, 1, (n_tgt, 3)) * ext
    tgt = np.round(tgt / 0.05) * 0.05
    if n_tgt >= 8:
        tgt[n_tgt // 2:n_tgt // 2 + n_tgt // 8] = tgt[:n_tgt // 8]          # duplicated targets: the lower index must win
    kind = rng.randint(0, 4, n_src)
    twin = rng.randint(0, n_tgt, n_src)
    src = tgt[twin].copy()
    near = kind == 0
    src[near] += np.round(rng.normal(0, 0.2, (int(near.sum()), 3)) / 0.05) * 0.05
    free = kind == 2
    src[free] = np.round(rng.uniform(-1, 1, (int(free.sum()), 3)) * ext / 0.05) * 0.05
    far = kind == 3
    src[far] = rng.uniform(-1, 1, (int(far.sum()), 3)) * ext * 3.0 + np.array([0.0, 0.0, 1.0])
    T = T_inv = None
    if with_T:
        T64 = rigid(rng, 17.0, 5.0)
        T = T64.astype(np.float32)
        T_inv = np.linalg.inv(T64).astype(np.float32)
        src = src @ T64[:3, :3] - T64[:3, 3] @ T64[:3, :3]                  # T(src) = the points above, up to fp32 rounding
    src, tgt = src.astype(np.float32), tgt.astype(np.float32)
    return src, tgt, T, T_inv, ref.one_side(src, tgt, T, RADIUS), ref.mutual(src, tgt, T, T_inv, RADIUS)


def dev_t(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.mark.parametrize("with_T", [False, True], ids=["asgiven", "T"])
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_side_and_mutual_equal_the_restatement(gpu, shape, with_T):
    from umeregrobust_amd import gt_matches
    src, tgt, T, T_inv, want_one, want_mut = case(*shape, with_T)
    got = gt_matches.one_side(dev_t(src, gpu), dev_t(tgt, gpu), dev_t(T, gpu), RADIUS)
    assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2 and got.device.type == "cuda"
    print(f"one side {shape} T={with_T}: {got.shape[0]} rows, restatement {want_one.shape[0]}")
    assert np.array_equal(got.cpu().numpy(), want_one)
    got = gt_matches.mutual(dev_t(src, gpu), dev_t(tgt, gpu), dev_t(T, gpu), dev_t(T_inv, gpu), RADIUS)
    print(f"mutual {shape} T={with_T}: {got.shape[0]} rows, restatement {want_mut.shape[0]}")
    assert tuple(got.shape[1:]) == (2,) and np.array_equal(got.cpu().numpy(), want_mut)
    if shape[0] >= 257:
        assert 0 < want_mut.shape[0] < want_one.shape[0] < shape[0], "the case must exercise kept and dropped rows"


def test_python_surface_keeps_the_reference_names(gpu):
    """utils.general_utils: device tensors in -> device tensors out; host arrays in -> numpy out; the inverse is formed inside"""
    from umeregrobust_amd.utils import general_utils as gu
    src, tgt, T, T_inv, want_one, _ = case(257, 1000, True)
    got = gu.one_side_ball_query_matches(dev_t(src, gpu), dev_t(tgt, gpu), dev_t(T, gpu), RADIUS)
    assert got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want_one)
    got = gu.one_side_ball_query_matches(src, tgt, torch.from_numpy(T), RADIUS)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want_one)
    inv = torch.linalg.inv(torch.from_numpy(T)).numpy()
    got = gu.mutual_ball_query_matches(dev_t(src, gpu), dev_t(tgt, gpu), torch.from_numpy(T), RADIUS)
    assert np.array_equal(got.cpu().numpy(), ref.mutual(src, tgt, T, inv, RADIUS))


def test_edges_of_the_radius_the_tie_rule_and_the_grid(gpu):
    from umeregrobust_amd import gt_matches
    one = lambda s, t, r, T=None: gt_matches.one_side(dev_t(np.asarray(s, np.float32), gpu), dev_t(np.asarray(t, np.float32), gpu),
                                                      dev_t(T, gpu), r).cpu().numpy()
    rng = np.random.RandomState(5)
    grid = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)     # 1 m lattice
    # zero matches (an empty result is [0, 2]) / every point matched, in order
    got = one(grid + 0.5, grid, 0.3)
    assert got.shape == (0, 2) and got.dtype == np.int64
    perm = rng.permutation(len(grid))
    got = one(grid[perm] + 0.01, grid, 0.3)
    assert np.array_equal(got, np.stack([np.arange(len(grid)), perm], 1))
    # duplicated targets: the lower index wins, wherever the duplicates sit
    t = np.concatenate([grid[::-1], grid, grid[perm]])
    got = one(grid, t, 0.3)
    assert np.array_equal(got, np.stack([np.arange(len(grid)), len(grid) - 1 - np.arange(len(grid))], 1))
    # r = 0.25: a query at distance exactly 0.25 is not matched, one at the next double below 0.25... is -- the radius is a DOUBLE
    # and the comparison strict.  (0.25 and 0.5 are exact in fp32; d2 = 0.0625 exactly.)
    t = np.array([[0.0, 0.0, 0.0], [8.0, 8.0, 1.0]])
    q = np.array([[0.25, 0.0, 0.0], [8.0, 8.25, 1.0], [0.0, 0.0, -0.25]])
    assert one(q, t, 0.25).shape == (0, 2)
    assert np.array_equal(one(q, t, np.nextafter(0.25, 1.0)), [[0, 0], [1, 1], [2, 0]])
    below = np.float32(np.nextafter(np.float32(0.25), np.float32(0)))
    assert np.array_equal(one([[below, 0.0, 0.0]], t, 0.25), [[0, 0]])
    # the distance one DOUBLE below 0.25: 0.25 - 2^-55 is the widened difference of the fp32 values 0.25 and 2^-55, and its square
    # 0.0625 - 2^-56 is a double below r^2; in fp32 the two distances are the same number
    assert np.nextafter(0.25, 0.0) == 0.25 - 2.0 ** -55
    assert np.array_equal(one([[0.25, 0.0, 0.0]], [[2.0 ** -55, 0.0, 0.0]], 0.25), [[0, 0]])
    assert one([[0.25, 0.0, 0.0]], [[0.0, 0.0, 0.0]], 0.25).shape == (0, 2)
    # negative coordinates, a query 1e4 m away (and one 1e30 m away), queries outside the box on every side
    t = grid - np.array([30.0, 30.0, 5.0])
    q = np.concatenate([t[:5] + 0.01, [[1e4, 0, 0], [-1e30, 1e30, 0], [-31.0, -31.0, -6.0], [0.0, 0.0, 0.0]]])
    assert np.array_equal(one(q, t, 0.3), np.stack([np.arange(5), np.arange(5)], 1))
    # targets all in one cell (and all in one POINT: a grid of zero extent), n not a multiple of 64 or 256
    t = rng.uniform(0, 1e-3, (333, 3)).astype(np.float32)
    q = np.concatenate([t[::-1][:131], t[:70] + 1.0])
    assert np.array_equal(one(q, t, 0.3), ref.one_side(q, t, None, 0.3)) and len(ref.one_side(q, t, None, 0.3)) == 131
    t = np.zeros((65, 3), np.float32) + 2.5
    assert np.array_equal(one([[2.5, 2.5, 2.6], [2.5, 2.5, 3.5]], t, 0.3), [[0, 0]])
    # a radius far larger than the cloud, and one far smaller than a cell
    src, tgt, T, _, _, _ = case(257, 1000, True)
    for r in (1e-4, 50.0, 1e6):
        assert np.array_equal(one(src, tgt, r, T), ref.one_side(src, tgt, T, r)), r


def test_nan_and_infinite_coordinates_are_refused(gpu):
    from umeregrobust_amd import gt_matches
    from umeregrobust_amd.utils import general_utils as gu
    src, tgt, T, T_inv, _, _ = case(257, 1000, True)
    for which, bad in (("src", np.nan), ("src", np.inf), ("tgt", np.nan), ("tgt", -np.inf), ("tgt", 3e6)):
        s, t = src.copy(), tgt.copy()
        (s if which == "src" else t)[100, 1] = bad
        with pytest.raises(RuntimeError, match="NaN"):
            gt_matches.one_side(dev_t(s, gpu), dev_t(t, gpu), dev_t(T, gpu), RADIUS)
        with pytest.raises(RuntimeError, match="NaN"):
            gu.mutual_ball_query_matches(dev_t(s, gpu), dev_t(t, gpu), torch.from_numpy(T), RADIUS)
    Tn = T.copy()
    Tn[0, 3] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        gt_matches.one_side(dev_t(src, gpu), dev_t(tgt, gpu), dev_t(Tn, gpu), RADIUS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gt_matches.one_side(torch.from_numpy(src), torch.from_numpy(tgt), None, RADIUS)


def test_raw_entries_are_deterministic_between_guard_bands(gpu):
    """Both compute entries through ctypes, twice, every buffer at exactly its stated size between 4 KiB canaries, the workspace
    full of (different) garbage: canaries intact, outputs byte-equal between the runs and equal to the restatement -- the rows
    behind the count included (never written: they carry the run's poison, so only the counted rows are compared)."""
    from umeregrobust_amd import gt_matches
    lib = gt_matches.load_native()
    src, tgt, T, T_inv, want_one, want_mut = case(5000, 4096, True)
    n, m = src.shape[0], tgt.shape[0]
    outs = []
    for run in range(2):
        gd = Guard(gpu, run)
        p_src, _ = gd.inp(src, "src")
        p_tgt, _ = gd.inp(tgt, "tgt")
        p_T, _ = gd.inp(T, "T")
        p_Ti, _ = gd.inp(T_inv, "T_inv")
        p_r1, t_r1 = gd.out((n, 2), torch.int64, "rows one side")
        p_c1, t_c1 = gd.out((2,), torch.int32, "count one side")
        p_ws, n_ws = gd.ws(lib.umereg_gt_matches_workspace_bytes(n, m, 0), "one-side workspace")
        gd.call("umereg_gt_matches_one_side_f32", p_src, n, p_tgt, m, p_T, RADIUS, p_r1, p_c1, p_ws, n_ws, gd.stream)
        p_r2, t_r2 = gd.out((n, 2), torch.int64, "rows mutual")
        p_c2, t_c2 = gd.out((2,), torch.int32, "count mutual")
        p_ws2, n_ws2 = gd.ws(lib.umereg_gt_matches_workspace_bytes(n, m, 1), "mutual workspace")
        gd.call("umereg_gt_matches_mutual_f32", p_src, n, p_tgt, m, p_T, p_Ti, RADIUS, p_r2, p_c2, p_ws2, n_ws2, gd.stream)
        gd.check()
        c1, c2 = t_c1.tolist(), t_c2.tolist()
        assert c1 == [len(want_one), 0] and c2 == [len(want_mut), 0]
        outs.append((t_r1[:c1[0]].cpu().numpy(), t_r2[:c2[0]].cpu().numpy()))
        # nothing behind the counted rows was touched
        assert bool((t_r1[c1[0]:].view(torch.uint8) == gd.poison).all()) and bool((t_r2[c2[0]:].view(torch.uint8) == gd.poison).all())
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    assert np.array_equal(outs[0][0], want_one) and np.array_equal(outs[0][1], want_mut)
    # argument errors come before any launch; size queries refuse what the entries refuse
    assert lib.umereg_gt_matches_workspace_bytes(0, 5, 0) == 0 and lib.umereg_gt_matches_workspace_bytes(5, -1, 1) == 0
    assert lib.umereg_gt_matches_one_side_f32(None, 5, None, 5, None, 0.3, None, None, None, 0, None) == -1
    gd = Guard(gpu, 0)
    p, _ = gd.inp(src, "src")
    po, _ = gd.out((n, 2), torch.int64)
    pc, _ = gd.out((2,), torch.int32)
    assert lib.umereg_gt_matches_one_side_f32(p, n, p, n, None, -1.0, po, pc, p, 16, None) == -1
    assert lib.umereg_gt_matches_one_side_f32(p, n, p, n, None, 0.3, po, pc, p, 16, None) == -3      # UMEREG_EWORKSPACE
