"""GPU: `umereg_scan_prep_f32` (csrc/scan_prep.hip) against the numpy restatement of the reference's masks (raw_scan_ref.scan_prep),
compared with ==: sizes around the kernel's tile and the chunk boundary of its scan, kept / dropped patterns, every option, the
inclusive ego box, error bits, and repeat runs between guard bands."""
import numpy as np
import pytest
import torch

import raw_scan_ref as rref

pytestmark = pytest.mark.gpu

# the kernel's constants (include/umereg_scan_prep.h, csrc/scan_prep.hip): rows per workgroup; threads of the block that scans the
# block counts -- with more blocks than that, a thread scans a chunk of several
BLOCK = 1024
SCAN_THREADS = 1024
EGO = (2.5, 1.0)


def test_the_sizes_below_are_the_kernels():
    from umeregrobust_amd import raw_scan
    assert (raw_scan.SCAN_PREP_BLOCK, raw_scan.SCAN_PREP_SCAN_THREADS) == (BLOCK, SCAN_THREADS)


def make_scan(seed, n, stride=4, p_zero=0.3, p_ego=0.2):
    """rows in [-6, 6] x [-3, 3] (a fifth inside the ego box), label words with instance halves, semantic keys 0..19"""
    rng = np.random.RandomState(seed)
    scan = rng.uniform(-1, 1, (n, stride)).astype(np.float32) * np.array([6, 3, 2, 1][:stride], np.float32)
    inside = rng.uniform(size=n) < p_ego
    scan[inside, :2] = rng.uniform(-1, 1, (int(inside.sum()), 2)).astype(np.float32) * np.array(EGO, np.float32)
    sem = np.where(rng.uniform(size=n) < p_zero, 0, rng.randint(1, 20, n)).astype(np.uint32)
    words = sem | (rng.randint(1, 1 << 16, n).astype(np.uint32) << 16)
    lut = rng.randint(0, 6, 20).astype(np.int32)               # several keys map to 0
    lut[0] = 0
    return scan, words, lut


def run(gpu, scan, labels=None, lut=None, sem16=False, keep_unlabeled=False, ego_box=None):
    from umeregrobust_amd import raw_scan
    pts, seg, index = raw_scan.prepare_cloud(scan, labels, lut=lut, sem16=sem16, keep_unlabeled=keep_unlabeled, ego_box=ego_box, device=gpu,
                                             return_index=True)
    assert pts.device == gpu and (pts.dtype, seg.dtype, index.dtype) == (torch.float32, torch.int64, torch.int64)
    return pts.cpu().numpy(), seg.cpu().numpy(), index.cpu().numpy()


def check(gpu, scan, labels=None, lut=None, **opts):
    got = run(gpu, scan, labels, lut, **opts)
    pts, seg, index, err = rref.scan_prep(scan, labels, lut, **opts)
    assert err == 0
    assert got[0].shape == pts.shape and np.array_equal(got[0].view(np.uint32), pts.view(np.uint32))      # the bytes, NaNs included
    assert np.array_equal(got[1], seg) and np.array_equal(got[2], index)
    assert (np.diff(got[2]) > 0).all()
    return len(seg)


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17])
def test_sizes_around_the_tile(gpu, n):
    for stride in (4, 3):
        scan, words, lut = make_scan(n + stride, n, stride)
        kept = check(gpu, scan, words, lut, sem16=True, ego_box=EGO)
        assert n < 64 or 0 < kept < n


@pytest.mark.parametrize("n", [BLOCK * SCAN_THREADS, BLOCK * SCAN_THREADS + 1, 2 * BLOCK * SCAN_THREADS + BLOCK + 5])
def test_sizes_around_the_chunk_boundary_of_the_scan(gpu, n):
    """up to SCAN_THREADS blocks every scanning thread has one block count; one more block and each has a chunk of two"""
    scan, words, lut = make_scan(7, n)
    assert 0 < check(gpu, scan, words, lut, sem16=True, ego_box=EGO) < n


def test_kept_and_dropped_patterns(gpu):
    n = 5 * BLOCK + 3
    scan, words, lut = make_scan(11, n, p_zero=0.0, p_ego=0.0)
    words = np.where((words & 0xFFFF) == 0, 1, words).astype(np.uint32)
    assert check(gpu, scan, words & 0xFFFF) == n                                     # none dropped
    assert check(gpu, scan, np.zeros(n, np.uint32)) == 0                             # all dropped: count 0
    assert check(gpu, scan, np.zeros(n, np.uint32), keep_unlabeled=True) == n
    hole = (words & 0xFFFF).copy()
    hole[BLOCK:3 * BLOCK] = 0                                                        # two whole blocks dropped between kept ones
    assert check(gpu, scan, hole) == n - 2 * BLOCK
    hole[:BLOCK] = 0
    hole[4 * BLOCK:] = 0                                                             # only one block in the middle survives
    assert check(gpu, scan, hole) == BLOCK
    boxed = scan.copy()
    boxed[:, :2] = 0.5                                                               # every point inside the box
    assert check(gpu, boxed, hole, ego_box=EGO, keep_unlabeled=True) == 0


def test_options(gpu):
    from umeregrobust_amd import raw_scan
    n = 2 * BLOCK + 77
    for stride in (3, 4):
        scan, words, lut = make_scan(20 + stride, n, stride)
        counts = [check(gpu, scan),                                                  # labels NULL: label 1 everywhere, nothing dropped
                  check(gpu, scan, ego_box=EGO),
                  check(gpu, scan, words, lut, sem16=True),
                  check(gpu, scan, words, lut, sem16=True, keep_unlabeled=True),
                  check(gpu, scan, words, lut, sem16=True, keep_unlabeled=True, ego_box=EGO),
                  check(gpu, scan, words & 0xFFFF),                                  # identity map
                  check(gpu, scan, words)]                                           # without SEM16 the whole word is the label: never 0 here
        assert counts[0] == n == counts[3] == counts[6] and counts[1] < n and counts[2] < counts[5] < n and counts[4] == counts[1]
        # the instance half must not leak into the label: with it, the keys would lie beyond the map
        assert (words >> 16).min() > 0
        with pytest.raises(KeyError, match="beyond the map's largest key 19"):
            run(gpu, scan, words, lut)
        # an ego box with one extent <= 0 is switched off
        assert check(gpu, scan, ego_box=(0.0, 1.0)) == n and check(gpu, scan, ego_box=(2.5, -1.0)) == n
        # labels as the int64 array np.load(...).astype(int) gives, and a device tensor input
        assert check(gpu, scan, (words & 0xFFFF).astype(np.int64)) == counts[5]
        dev_scan = torch.from_numpy(scan).to(gpu)
        pts, seg = raw_scan.prepare_cloud(dev_scan, torch.from_numpy((words & 0xFFFF).astype(np.int64)).to(gpu))
        assert len(pts) == counts[5] and seg.min() > 0


def test_a_scan_that_is_not_16_byte_aligned(gpu):
    """a [n,4] view that starts 4 bytes into an allocation takes the scalar-load path"""
    from umeregrobust_amd import raw_scan
    n = BLOCK + 9
    scan, words, lut = make_scan(31, n)
    flat = torch.zeros(4 * n + 1, dtype=torch.float32, device=gpu)
    flat[1:] = torch.from_numpy(scan).to(gpu).reshape(-1)
    view = flat[1:].view(n, 4)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    pts, seg = raw_scan.prepare_cloud(view, words, lut=lut, sem16=True, ego_box=EGO)
    want = rref.scan_prep(scan, words, lut, sem16=True, ego_box=EGO)
    assert np.array_equal(pts.cpu().numpy(), want[0]) and np.array_equal(seg.cpu().numpy(), want[1])


def test_ego_box_is_inclusive_and_a_nan_is_kept(gpu):
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))                     # noqa: E731
    nan = np.float32(np.nan)
    rows = [(2.5, 0.5, "drop"), (-2.5, 0.5, "drop"), (1.0, 1.0, "drop"), (1.0, -1.0, "drop"), (2.5, 1.0, "drop"), (-2.5, -1.0, "drop"),
            (0.0, 0.0, "drop"), (-0.0, 0.3, "drop"), (up(2.5), 0.5, "keep"), (-up(2.5), 0.5, "keep"), (1.0, up(1.0), "keep"),
            (1.0, -up(1.0), "keep"), (2.5, up(1.0), "keep"), (nan, 0.5, "keep"), (1.0, nan, "keep"), (nan, nan, "keep"),
            (np.float32(np.inf), 0.0, "keep"), (0.0, -np.float32(np.inf), "keep"), (40.0, 0.0, "keep"), (0.0, 7.0, "keep")]
    scan = np.array([(x, y, -1.7, 0.0) for x, y, _ in rows], np.float32)
    want = np.array([i for i, r in enumerate(rows) if r[2] == "keep"])
    for stride in (4, 3):
        pts, seg, index = run(gpu, scan[:, :stride].copy(), ego_box=EGO)
        assert np.array_equal(index, want), index
        assert np.array_equal(pts.view(np.uint32), scan[want, :3].view(np.uint32)) and (seg == 1).all()
        check(gpu, scan[:, :stride].copy(), ego_box=EGO)
    # a NaN z, and NaNs without a box, pass through untouched
    scan[3, 2] = nan
    check(gpu, scan)


def test_label_keys_outside_the_map_raise(gpu):
    scan, words, lut = make_scan(41, 3 * BLOCK + 5)
    holes = lut.copy()
    holes[7] = -1
    sem = (words & 0xFFFF).astype(np.uint32)
    sem = np.where(sem == 7, 3, sem).astype(np.uint32)                               # the scan itself never names key 7
    beyond, unmapped, both = sem.copy(), sem.copy(), sem.copy()
    beyond[2 * BLOCK + 3] = 20                                                      # one row, in the last full block
    unmapped[5] = 7
    both[[5, 2 * BLOCK + 3]] = 7, 20
    with pytest.raises(KeyError, match="beyond the map's largest key 19"):
        run(gpu, scan, beyond, lut)
    with pytest.raises(KeyError, match="no key of the map"):
        run(gpu, scan, unmapped, holes)
    with pytest.raises(KeyError, match="beyond.*and one that is no key"):
        run(gpu, scan, both, holes)
    # the reference maps every label before it masks any point: a bad key raises on a row the ego box would drop, too
    inside = scan.copy()
    inside[2 * BLOCK + 3, :2] = 0.1
    with pytest.raises(KeyError, match="beyond"):
        run(gpu, inside, beyond, lut, ego_box=EGO)
    # keys of the map whose holes the scan never names are fine
    check(gpu, scan, sem, holes)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        run(gpu, scan, -sem.astype(np.int64) - 1)


def test_two_runs_between_guard_bands_give_the_same_bytes(gpu):
    """outputs and workspace lie between guard bands and hold different garbage before each run: the same bytes both times, rows
    beyond the count untouched, no guard byte touched, and out_index ascending"""
    from umeregrobust_amd import raw_scan
    n, G = 4 * BLOCK + 321, 4096
    scan, words, lut = make_scan(51, n)
    want_pts, want_seg, want_idx, err = rref.scan_prep(scan, words, lut, sem16=True, ego_box=EGO)
    m = len(want_seg)
    assert err == 0 and 0 < m < n
    d_scan, d_lut = torch.from_numpy(scan).to(gpu), torch.from_numpy(lut).to(gpu)
    d_words = torch.from_numpy(words.view(np.int32)).to(gpu)
    ws_bytes = raw_scan.workspace_bytes(n)
    sizes = dict(pts=12 * n, seg=8 * n, index=8 * n, count=8, ws=ws_bytes)
    results = []
    for fill in (0x5A, 0xC3):
        bufs = {k: torch.full((G + b + G,), fill, dtype=torch.uint8, device=gpu) for k, b in sizes.items()}
        inner = {k: bufs[k][G:G + b] for k, b in sizes.items()}
        raw_scan.scan_prep_raw(d_scan, d_words, d_lut, raw_scan.SCAN_SEM16, EGO, inner["pts"].view(torch.float32).view(n, 3),
                               inner["seg"].view(torch.int64), inner["index"].view(torch.int64), inner["count"].view(torch.int32), inner["ws"])
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in bufs.items()}
        for k, b in sizes.items():
            assert (host[k][:G] == fill).all() and (host[k][G + b:] == fill).all(), f"guard band of {k} touched"
        count = host["count"][G:G + 8].view(np.int32)
        assert count.tolist() == [m, 0]
        for k, row in (("pts", 12), ("seg", 8), ("index", 8)):
            assert (host[k][G + row * m:G + sizes[k]] == fill).all(), f"rows of {k} beyond the count were written"
        results.append({k: host[k][G:G + row * m].copy() for k, row in (("pts", 12), ("seg", 8), ("index", 8))})
    for k in ("pts", "seg", "index"):
        assert np.array_equal(results[0][k], results[1][k]), k
    assert np.array_equal(results[0]["pts"].view(np.float32).reshape(m, 3), want_pts)
    assert np.array_equal(results[0]["seg"].view(np.int64), want_seg)
    idx = results[0]["index"].view(np.int64)
    assert np.array_equal(idx, want_idx) and (np.diff(idx) > 0).all()


def test_an_empty_scan_and_bad_inputs(gpu):
    from umeregrobust_amd import raw_scan
    pts, seg = raw_scan.prepare_cloud(np.zeros((0, 4), np.float32), device=gpu)
    assert pts.shape == (0, 3) and seg.shape == (0,) and pts.device == gpu
    with pytest.raises(ValueError, match="float32"):
        raw_scan.prepare_cloud(np.zeros((5, 4), np.float64), device=gpu)
    with pytest.raises(ValueError, match=r"\[n,3\] or \[n,4\]"):
        raw_scan.prepare_cloud(np.zeros((5, 5), np.float32), device=gpu)
    with pytest.raises(ValueError, match="labels must be 5 integers"):
        raw_scan.prepare_cloud(np.zeros((5, 4), np.float32), np.zeros(4, np.uint32), device=gpu)
