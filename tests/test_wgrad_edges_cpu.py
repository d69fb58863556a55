"""No GPU: the plan mirror of tests/wgrad_cases.py against the library's host arithmetic, and every edge that a cloud of
tests/wgrad_cases.py is there for -- pair counts per offset, rows per ballot chunk and per segment, queue positions -- asserted on
the cloud itself, so that a change to a cloud that loses its edge fails here."""
import numpy as np
import pytest

import wgrad_cases as wc
from test_sparse_grad_gpu import OPS

CHANNELS = sorted({(cin, cout) for _, cin, cout in OPS} | {(96, 32), (32, 96)})
SIZES = (1, 1023, 1024, 1025, 2049, 9216, 9217, 65536, 65537, 132308, 800000)


def test_plan_mirror_equals_the_library():
    from umeregrobust_amd import sparse_conv
    lib = sparse_conv.load_native()
    assert {(96, 32), (32, 96), (1, 32), (256, 256), (192, 64)} <= set(CHANNELS)
    for n in SIZES:
        for cin, cout in CHANNELS:
            rps, segments = wc.plan(n, cin, cout)
            assert lib.umereg_sparse_conv_wgrad_segments(n, cin, cout) == segments, (n, cin, cout)
            assert lib.umereg_sparse_conv_wgrad_scratch_bytes(n, cin, cout) == segments * 27 * cin * cout * 4, (n, cin, cout)
            assert 1 <= segments <= wc.MAX_SEGMENTS and rps % 64 == 0 and rps >= wc.MIN_RPS
            assert (segments - 1) * rps < n <= segments * rps
    assert wc.plan(1024, 32, 32) == (1024, 1) and wc.plan(1025, 32, 32) == (1024, 2)
    assert wc.plan(2049, 32, 32) == (1024, 3)
    assert wc.plan(9216, 256, 256) == (1024, 9) and wc.plan(9217, 256, 256) == (1088, 9)      # rps leaves its floor here
    assert wc.plan(800000, 256, 256) == (88896, 9) and wc.plan(800000, 32, 32)[1] == 64


def active_rows(name, t, k):
    """the output rows (level-0 order of the library) of offset k's pairs of table 0 or 9, ascending"""
    assert t in (0, 9)
    rank = np.empty(len(wc.cloud(name)), np.int64)
    rank[wc.level0_order(wc.cloud(name))] = np.arange(len(rank))
    return np.sort(rank[wc.tables_of(name).pairs[t][k][0].numpy()])


def queue_trace(rows, n_rows, rps, G):
    """wg_body's bookkeeping over the active rows of one offset -> per segment (most pairs queued at once, pairs carried into a
    chunk at most, last queue position written, padded slots)"""
    out = []
    for r0 in range(0, n_rows, rps):
        r1 = min(r0 + rps, n_rows)
        head = tail = most = carried = 0
        for base in range(r0, r1, wc.CHUNK):
            carried = max(carried, tail - head)
            tail += int(((rows >= base) & (rows < min(base + wc.CHUNK, r1))).sum())
            most = max(most, tail - head)
            head += (tail - head) // G * G
        pad = G - (tail - head) if tail > head else 0
        out.append((most, carried, tail + pad - 1, pad))
    return out


@pytest.mark.parametrize("m", wc.LINES)
def test_line_has_its_groups_chunks_and_carries(m):
    name = f"line{m}"
    sizes = wc.tables_of(name).sizes
    p0, p5, p9 = (wc.pair_counts(name, t) for t in (0, 5, 9))
    assert (wc.level0_order(wc.cloud(name)) == np.arange(m)).all()                 # level-0 order = the order given
    assert p0[13] == m and p0[12] == p0[14] == m - 1 and sum(p0) == 3 * m - 2
    # tables 5 and 9: floor(m / 2) pairs at offsets 15 and 16, ceil(m / 2) at 17 -- every level-1 row when m is odd
    for p in (p5, p9):
        assert p[15] == p[16] == m // 2 and p[17] == (m + 1) // 2 and sum(p) == m // 2 * 2 + (m + 1) // 2
    assert sizes[0] == m and sizes[1] == m // 2 + 1
    if m % 2:
        assert p5[17] == sizes[1]
    if m == 129:
        assert (p5[15], p5[16], p5[17]) == (64, 64, 65)
        for prec, G in wc.GROUP.items():
            # offset 12: row 0 has no -x neighbour, so the first chunk queues 63 and carries G - 1 into a chunk that adds 64
            (most, carried, last, pad), = queue_trace(active_rows(name, 0, 12), m, 1024, G)
            assert (most, carried) == (G - 1 + 64, G - 1) and most < wc.QUEUE
            # offset 13: 129 pairs, the last one and its padding lie past position 127 of the ring
            (_, _, last, pad), = queue_trace(active_rows(name, 0, 13), m, 1024, G)
            assert last >= wc.QUEUE and pad == G - 1


def test_lines_cover_both_sides_of_one_and_two_groups():
    """pair counts of the lines' offsets over tables 0, 5 and 9: G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1 for G = 8 and 16, the
    64-row chunk on both sides, and the 8 row lanes of wg_c1_kernel"""
    counts = {n for m in wc.LINES for t in (0, 5, 9) for n in wc.pair_counts(f"line{m}", t)}
    for G in wc.GROUP.values():
        assert {G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1} <= counts, G
    assert {63, 64, 65, 128, 129} <= counts
    assert [m for m in wc.LINES if m <= 17] == [1, 7, 8, 9, 15, 16, 17] and len(wc.LINES[:9]) == 9


@pytest.mark.parametrize("m", wc.TWOS)
def test_pairs_of_two_put_holes_into_the_ballot(m):
    name = f"twos{m}"
    assert (wc.level0_order(wc.cloud(name)) == np.arange(2 * m)).all()
    p0 = wc.pair_counts(name, 0)
    assert p0[13] == 2 * m and p0[12] == p0[14] == m and sum(p0) == 4 * m
    assert (active_rows(name, 0, 14) == 2 * np.arange(m)).all() and (active_rows(name, 0, 12) == 2 * np.arange(m) + 1).all()
    for t in (5, 9):
        assert sum(wc.pair_counts(name, t)) == 3 * m


@pytest.mark.parametrize("name", ["isolated_then_line", "line_then_isolated"])
def test_isolated_and_line_leave_one_segment_without_pairs(name):
    c = wc.cloud(name)
    assert len(c) == 1064 and wc.plan(1064, 32, 64) == wc.plan(1064, 64, 32) == wc.plan(1064, 1, 32) == (1024, 2)
    assert int(c[:, 1:].max()) == 52150 < 1 << 17
    assert (wc.level0_order(c) == np.arange(1064)).all()
    p0 = wc.pair_counts(name, 0)
    assert p0[13] == 1064 and p0[12] == p0[14] == 39 and sum(p0) == 1064 + 78
    first = name == "isolated_then_line"
    for k in range(27):
        rows = active_rows(name, 0, k)
        if k != 13:                                    # 26 offsets: all of their pairs lie in one segment, the other's block is zero
            assert (rows >= 1024).all() if first else (rows < 1024).all()
    assert (active_rows(name, 0, 13) == np.arange(1064)).all()


def test_rows1024_and_rows1025_are_one_and_two_segments():
    for n, segments in ((1024, 1), (1025, 2)):
        name = f"rows{n}"
        for ch in wc.SEGMENT_CHANNELS + [(1, 32)]:
            assert wc.plan(n, *ch) == (1024, segments)
        p0 = wc.pair_counts(name, 0)
        assert min(p0) == 735 and p0[13] == n                    # 15 x 7 x 7 pairs at the corner offsets of the 16 x 8 x 8 block
        order = wc.level0_order(wc.cloud(name))
        assert not (order == np.arange(n)).all() and sorted(order) == list(range(n))
    # the one row of segment 1 is the far point (its cell is the last to occur): that segment has a pair at the centre offset only
    c = wc.cloud("rows1025")
    assert c[wc.level0_order(c)[1024], 1] == 1000
    assert [k for k in range(27) if (active_rows("rows1025", 0, k) == 1024).any()] == [13]


def test_deep_has_plan_segments_without_rows():
    t = wc.tables_of("deep")
    assert t.sizes[:3] == [2049, 257, 33]
    for ch in wc.DEEP_CHANNELS + [(32, 32)]:
        assert wc.plan(2049, *ch) == (1024, 3)
    # table 5 writes level 1: 257 rows, all in segment 0 of 3; table 9 writes level 0: three segments that hold rows
    assert wc.ceil_div(t.sizes[1], 1024) == 1 and wc.ceil_div(t.sizes[0], 1024) == 3
    assert sum(wc.pair_counts("deep", 5)) == sum(wc.pair_counts("deep", 9)) == 5820
    for k in range(27):
        rows = active_rows("deep", 9, k)
        if len(rows):
            assert (rows < 1024).any() and ((rows >= 1024) & (rows < 2048)).any()
    assert max(len(active_rows("deep", 9, k)) and int(active_rows("deep", 9, k)[-1]) for k in range(27)) == 2048


def test_long_segments_leave_the_1024_floor():
    assert len(wc.cloud("long_segments")) == 9217
    assert wc.plan(9217, 256, 256) == (1088, 9) and wc.plan(9216, 256, 256) == (1024, 9)
    p0 = wc.pair_counts("long_segments", 0)
    assert min(p0) == 7935 and max(p0) == p0[13] == 9217
    # every segment holds pairs of every offset, and the last one is short: 9217 - 8 x 1088 = 513 rows
    for k in range(27):
        per_segment = np.bincount(active_rows("long_segments", 0, k) // 1088, minlength=9)
        assert (per_segment > 0).all()
    assert 9217 - 8 * 1088 == 513


def test_every_exact_case_sums_integers_below_2_24():
    """operands in [-3, 3]: |x| |dy| <= 9 per pair, so every partial sum of dW is an integer of at most 9 x pairs; f16 takes dY
    2^12, whose largest magnitude 3 x 2^12 is an f16 number, and the sums scale with it exactly"""
    most = max(max(wc.pair_counts(name, t)) for name, t in wc.EXACT_CASES)
    assert most == 9217 and most * 9 < 2 ** 24
    assert 3 * 2 ** 12 < 65504 and most * 9 * 2 ** 12 < 2 ** 24 * 2 ** 12
    assert len(wc.EXACT_CASES) == 17 * 3 + 4 + 1 + 2


def test_repack_statement_is_the_header_formula():
    """wgrad_cases.repacked against the header's index formula, element by element, on a small kernel"""
    cin, cout = 4, 6
    W = np.arange(27 * cin * cout, dtype=np.float32).reshape(27, cin, cout)
    for transpose in (False, True):
        R, C = (cout, cin) if transpose else (cin, cout)
        for mirror in (False, True):
            for slice in (1, 2, R):
                out = wc.repacked(W, transpose, mirror, slice).reshape(R // slice, 27, slice, C)
                for s in range(R // slice):
                    for k in range(27):
                        kp = 26 - k if mirror else k
                        for r in range(s * slice, (s + 1) * slice):
                            for c in range(C):
                                assert out[s, kp, r - s * slice, c] == (W[k, c, r] if transpose else W[k, r, c])
