"""The voxel key, the table capacity and the home slot of csrc/voxel_key.h against their Python mirror, without a GPU.

tests/test_voxel_hash_edges_gpu.py chooses its clouds with tests/glue_cases.py's `keys` / `capacity` / `home_slot`: cells whose probes
wrap past the last slot, 300 cells in one probe chain, clouds at the capacity switch.  If the mirror drifted from the header, those
clouds would stop being what they claim while the GPU comparisons (against numpy's `unique`) stayed green.  A host program
(tests/voxel_key_host.cpp, compiled here with the hipcc that builds the library) prints the header's own answers; the two must agree
line by line.  The second half pins what the GPU cases rely on: where their cells live and how many sweep points tell the IEEE
division from its usual replacements."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import glue_cases as gc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's key arithmetic cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("voxel_key") / "voxel_key_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-I", _build.INCLUDE,
                           "-I", _build.CSRC, os.path.join(REPO, "tests", "voxel_key_host.cpp"), "-o", exe])

    def run(pts, voxel, n):
        """-> int64 [len(pts), 4]: ok, key, cap, home slot as the header computes them (n: one table size or one per point)"""
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        n = np.broadcast_to(np.asarray(n), (len(pts),))
        v = float(np.float32(voxel)).hex()
        text = "".join(f"{float(p[0]).hex()} {float(p[1]).hex()} {float(p[2]).hex()} {v} {int(k)}\n" for p, k in zip(pts, n))
        out = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout
        rows = np.array([[int(t) for t in ln.split()] for ln in out.split("\n") if ln], np.uint64)
        assert rows.shape == (len(pts), 4)
        return rows
    return run


def mirror(pts, voxel, n):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    n = np.broadcast_to(np.asarray(n), (len(pts),))
    ok, key = gc.keys(pts, voxel)
    cap = np.array([gc.capacity(int(k)) for k in n], np.uint64)
    slot = np.array([gc.home_slot(k, int(c)) if o else 0 for k, c, o in zip(key, cap, ok)], np.uint64)
    return np.stack([ok.astype(np.uint64), key, cap, slot], axis=1)


def same(header, pts, voxel, n):
    got, want = header(pts, voxel, n), mirror(pts, voxel, n)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (np.asarray(pts)[bad[:5]], got[bad[:5]], want[bad[:5]])
    return got


def test_capacity_switches_where_twice_the_points_reach_a_power_of_two(header):
    got = same(header, np.zeros((len(gc.CAPACITY_N), 3)), 1.0, gc.CAPACITY_N)
    assert got[:, 2].tolist() == [1024, 1024, 1024, 2048, 131072, 262144]
    assert [gc.capacity(n) for n in (600, 900, 1024, 1025, 1200, 24579)] == [2048, 2048, 2048, 4096, 4096, 65536]


def test_every_axis_extreme(header):
    q = gc.Q_MAX
    rows = []
    for axis in range(3):
        for v in (q, q - 1, q + 1, -q, -q + 1, -q - 1, 0, -1):
            c = [5, -7, 9]
            c[axis] = v
            rows.append(c)
    rows += [[q, q, q], [-q, -q, -q], [q + 1, q + 1, q + 1], [-q - 1, 0, q]]
    pts = (np.array(rows, np.float64) + 0.5).astype(np.float32)
    for n in gc.CAPACITY_N:
        got = same(header, pts, 1.0, n)
        assert got[:, 0].tolist() == [int(np.abs(r).max() <= q) for r in rows]
    ok = got[:, 0] == 1
    assert len(set(got[ok, 1].tolist())) == int(ok.sum())                  # distinct cells, distinct keys
    assert int(got[:, 1].max()) < 1 << 63
    # the fields: x above bit 42, y above bit 21, z below
    x1, x2, z2 = (header((np.array([c], np.float64) + 0.5), 1.0, 1)[0, 1] for c in ([5, -7, 9], [6, -7, 9], [5, -7, 10]))
    assert int(x2) - int(x1) == 1 << 42 and int(z2) - int(x1) == 1
    # a coarser voxel far out, and what has no cell at all
    far = np.array([[3e5, -3e5, 0.0], [314572.4, 0, 0], [314573.0, 0, 0], [-314572.4, 0, 0], [-314573.0, 0, 0],
                    [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3.4e38, 0, 0]], np.float32)
    got = same(header, far, 0.3, 513)
    assert got[5:, 0].tolist() == [0, 0, 0, 0] and got[0, 0] == 1


def test_random_points_at_every_voxel_size(header):
    rng = np.random.RandomState(5)
    for i, voxel in enumerate(gc.SWEEP_VOXELS):
        pts = (rng.uniform(-120, 120, (2500, 3)) * (1 if i % 2 else 40)).astype(np.float32)
        same(header, pts, voxel, gc.CAPACITY_N[1 + i])
    same(header, rng.uniform(-4e5, 4e5, (2000, 3)).astype(np.float32), 0.3, 65537)      # some beyond the range, some within


def test_sweep_points_sit_on_the_voxel_boundaries(header):
    """The GPU sweep has teeth: at these points a reciprocal multiply or an fp64 division takes another floor than the fp32 division
    does (counted here, so the sweep cannot quietly lose them), and the header takes the fp32 division's."""
    flips_rcp, flips_f64 = [], []
    for i, voxel in enumerate(gc.SWEEP_VOXELS):
        pts = gc.sweep_cloud(voxel, gc.sweep_axis(i))
        assert pts.shape == (3 * (2 * gc.SWEEP_K + 1), 3) and gc.capacity(len(pts)) == 65536
        x, v = pts[:, gc.sweep_axis(i)], np.float32(voxel)
        q = np.floor(x / v)
        flips_rcp.append(int((np.floor(x * (np.float32(1.0) / v)) != q).sum()))
        flips_f64.append(int((np.floor(x.astype(np.float64) / voxel) != q).sum()))
        same(header, pts, voxel, len(pts))
    print("floors moved by a reciprocal multiply:", flips_rcp, " by an fp64 division:", flips_f64)
    assert flips_rcp == [1908, 1217, 1908, 1217]
    assert min(flips_f64) > 3000


def test_gpu_clouds_are_what_they_claim(header):
    # wrap: 600 distinct cells, every home slot among the last 6 of 2048
    pts = gc.wrap_cloud()
    got = same(header, pts, gc.CELL_VOXEL, len(pts))
    assert (got[:, 2] == 2048).all() and (got[:, 3] >= 2042).all() and len(set(got[:, 1].tolist())) == 600
    assert len(set(got[:, 3].tolist())) == 6
    # chains: 300 cells on the last home slot, each of them twice
    for cap, n in ((2048, 900), (4096, 1200)):
        pts = gc.chain_cloud(cap)
        got = same(header, pts, gc.CELL_VOXEL, len(pts))
        assert len(pts) == n and (got[:, 2] == cap).all()
        last = got[got[:, 3] == cap - 1, 1]
        assert len(last) == 600 and len(set(last.tolist())) == 300
        assert len(gc.first_of_every_voxel(pts, gc.CELL_VOXEL)) == 600
    # there are enough such cells to choose from
    cells, home = gc.cells_by_home_slot(2048)
    print(f"{len(cells)} cells: {(home >= 2042).sum()} on the last 6 slots of 2048, {(home == 2047).sum()} on the last")
    assert (home >= 2042).sum() > 5000 and (home == 2047).sum() > 800
    # capacity switch: all distinct
    for n in gc.CAPACITY_N:
        pts = gc.distinct_cloud(n)
        assert np.array_equal(gc.first_of_every_voxel(pts, gc.CELL_VOXEL), np.arange(n))
    same(header, gc.distinct_cloud(513), gc.CELL_VOXEL, 513)
    # key range: every point has a key, every cell twice
    pts = gc.range_cloud()
    got = same(header, pts, 1.0, len(pts))
    assert (got[:, 0] == 1).all() and 2 * len(set(got[:, 1].tolist())) == len(pts) == 2 * len(gc.first_of_every_voxel(pts, 1.0))
    for axis in range(3):
        for sign in (1, -1):
            assert same(header, gc.beyond_range_point(axis, sign), 1.0, 1)[0, 0] == 0
