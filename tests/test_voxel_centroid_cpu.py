"""The arithmetic of csrc/voxel_centroid_math.h against its numpy mirror (tests/voxel_centroid_ref.py), without a GPU.

The GPU tests compare the kernels with the mirror bit for bit; if the mirror drifted from the header they would fail for the wrong
reason, or -- worse -- a kernel and a mirror wrong in the same way would agree.  A host program (tests/voxel_centroid_host.cpp, compiled
here with the hipcc that builds the library) prints the header's own answers; the two must agree bit for bit.  The second half pins
what the contract promises of the mirror itself: independence of the order, closeness to the fp64 mean, centroids inside their boxes."""
import fractions
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import glue_cases as gc
from tests import voxel_centroid_ref as vc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXELS = (0.3, 0.05, 0.6, 0.1, 0.25, 0.8, 0.4)


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's arithmetic cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("voxel_centroid") / "voxel_centroid_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-I", _build.INCLUDE,
                           "-I", _build.CSRC, os.path.join(REPO, "tests", "voxel_centroid_host.cpp"), "-o", exe])

    def run(text, width):
        out = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout
        rows = np.array([[int(t) for t in ln.split()] for ln in out.split("\n") if ln], np.int64).reshape(-1, width)
        return rows

    def quanta(p, voxel):
        """-> int64 [len(p), 2]: cell and quantum as the header computes them"""
        p = np.asarray(p, np.float32).reshape(-1)
        v = float(np.float32(voxel)).hex()
        rows = run("".join(f"q {float(x).hex()} {v}\n" for x in p), 2)
        assert len(rows) == len(p)
        return rows

    def centroid(cell, total, count, voxel):
        """-> f32 [len(cell)]: the centroids as the header computes them"""
        v = float(np.float32(voxel)).hex()
        rows = run("".join(f"c {int(c)} {int(s)} {int(n)} {v}\n" for c, s, n in zip(cell, total, count)), 1)
        assert len(rows) == len(cell)
        return rows[:, 0].astype(np.uint32).view(np.float32)
    return SimpleHeader(quanta, centroid)


class SimpleHeader:
    def __init__(self, quanta, centroid):
        self.quanta, self.centroid = quanta, centroid


def same_quanta(header, p, voxel):
    p = np.asarray(p, np.float32).reshape(-1)
    got = header.quanta(p, voxel)
    c, q = vc.quanta(p, voxel)
    want = np.stack([c.astype(np.int64), q], axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (p[bad[:5]], got[bad[:5]], want[bad[:5]])
    return got


def same_cloud(header, pts, voxel):
    """every point's cell and quantum, then every voxel's centroid from the mirror's sums, against the header"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    same_quanta(header, pts, voxel)
    first, c, S, count = vc.voxel_sums(pts, voxel)
    want = vc.centroid(c, S, count[:, None], voxel)
    got = header.centroid(c.reshape(-1), S.reshape(-1), np.repeat(count, 3), voxel).reshape(-1, 3)
    assert got.tobytes() == want.tobytes(), (got[:3], want[:3])
    return want, first, count


# ---- the header against the mirror ---------------------------------------------------------------------------------------------------

def test_one_point(header):
    for voxel in VOXELS:
        for p in ([0.0, 0.0, 0.0], [1.2345, -6.789, 0.001], [-0.0, 7.5, -7.5]):
            want, first, count = same_cloud(header, [p], voxel)
            assert first.tolist() == [0] and count.tolist() == [1]
            # cnt = 1: the centroid is the point again up to the quantum, v 2^-33, and the final rounding
            assert np.abs(want[0].astype(np.float64) - np.float32(p).astype(np.float64)).max() <= np.spacing(np.float32(8.0)) / 2 + voxel * 2.0 ** -32


def test_points_exactly_on_a_boundary(header):
    for voxel in VOXELS:
        pts = vc.boundary_cloud(voxel)
        got = same_quanta(header, pts, voxel)
        assert np.abs(got[:, 1]).max() <= 1 << 32
        same_cloud(header, pts, voxel)
    # where v is a power of two the quotient is exact: the cell is k and the quantum 0
    pts = vc.boundary_cloud(0.25)
    got = header.quanta(pts[:, 0], 0.25)
    on = np.abs(pts[:, 0] - 0.125) > 1e-6
    assert (got[on, 1] == 0).all() and sorted(set(got[on, 0].tolist())) == [-3, -2, -1, 0, 1, 2, 3]


def test_quotients_within_an_ulp_of_a_boundary(header):
    """glue_cases' sweep: fl32(k v), its successor and its predecessor.  Some quotients round UP to the integer the real quotient stays
    below: u < 0 there, which is why the quantum is signed (counted, so the sweep cannot lose them)."""
    negative = []
    for i, voxel in enumerate(gc.SWEEP_VOXELS):
        axis = gc.sweep_axis(i)
        pts = gc.sweep_cloud(voxel, axis)
        got = same_quanta(header, pts[:, axis], voxel)
        negative.append(int((got[:, 1] < 0).sum()))
        # u >= -half an f32 ulp of a quotient below 2^13, which is 2^-11; times 2^32
        assert got[:, 1].min() >= -(1 << 21) and got[:, 1].max() <= 1 << 32
        same_cloud(header, vc.near_boundary_cloud(voxel, axis), voxel)
    print("quanta below zero per sweep:", negative)
    assert min(negative) > 100


def test_negative_cells_and_the_ends_of_the_key_range(header):
    rng = np.random.RandomState(3)
    for voxel in VOXELS:
        pts = rng.uniform(-50.0, -1.0, (500, 3)).astype(np.float32)
        want, _, _ = same_cloud(header, pts, voxel)
        assert (vc.cells(want, voxel) < 0).all()
    # cells at +-(2^20 - 1) and their neighbours, every cell twice (voxel 1: coordinates ~1e6, an f32 ulp of 1/16)
    pts = gc.range_cloud()
    want, first, count = same_cloud(header, pts, 1.0)
    assert (count == 2).all() and np.abs(vc.cells(pts, 1.0)).max() == gc.Q_MAX
    jit = pts + np.float32(0.25) * np.random.RandomState(4).randint(-1, 2, pts.shape).astype(np.float32)
    same_cloud(header, jit, 1.0)


def test_count_one_and_count_at_the_cap(header):
    """cnt = 1 and cnt = 2^20 points in one voxel: the largest sum the contract admits, |S| <= 2^52, still exact as a double"""
    rng = np.random.RandomState(5)
    for voxel, cell in ((0.3, (3, -2, 5)), (0.8, (-7, 0, 11))):
        pts = ((np.array(cell) + rng.uniform(0.0, 1.0, (vc.MAX_POINTS, 3))) * voxel).astype(np.float32)
        pts = pts[(vc.cells(pts, voxel) == np.float32(cell)).all(axis=1)]
        pts = np.concatenate([pts, pts[:vc.MAX_POINTS - len(pts)]])
        assert len(pts) == vc.MAX_POINTS
        first, c, S, count = vc.voxel_sums(pts, voxel)
        assert count.tolist() == [vc.MAX_POINTS] and first.tolist() == [0] and np.abs(S).max() < 1 << 52
        assert (S.astype(np.float64).astype(np.int64) == S).all()
        want = vc.centroid(c, S, count[:, None], voxel)
        got = header.centroid(c.reshape(-1), S.reshape(-1), np.repeat(count, 3), voxel).reshape(-1, 3)
        assert got.tobytes() == want.tobytes()
        mean = pts.astype(np.float64).mean(axis=0)
        assert np.abs(want[0] - mean).max() < 1e-6
        same_quanta(header, pts[:2000], voxel)
    # the extreme sums themselves: S = +-2^52 and one off, cnt = 2^20
    cellv = np.array([0, 5, -5, gc.Q_MAX, -gc.Q_MAX] * 4)
    S = np.repeat(np.array([1 << 52, -(1 << 52), (1 << 52) - 1, -(1 << 52) + 1]), 5)
    for voxel in VOXELS:
        want = vc.centroid(cellv.astype(np.float32), S, np.full(len(S), vc.MAX_POINTS), voxel)
        assert header.centroid(cellv, S, np.full(len(S), vc.MAX_POINTS), voxel).tobytes() == want.tobytes()


# ---- what the contract promises of the mirror ----------------------------------------------------------------------------------------

def test_the_sums_do_not_depend_on_the_order():
    for seed, voxel in enumerate(VOXELS):
        pts = vc.dense_cloud(3000, voxel=voxel, seed=seed)
        cen, first, count = vc.down_sample(pts, voxel)
        perm = np.random.RandomState(seed).permutation(len(pts))
        cen2, first2, count2 = vc.down_sample(pts[perm], voxel)
        # the same voxels, found in another order: match the rows of the two runs by their voxel's key
        _, key = gc.keys(pts, voxel)
        k1, k2 = key[first], key[perm][first2]
        o1, o2 = np.argsort(k1), np.argsort(k2)
        assert np.array_equal(k1[o1], k2[o2])
        assert cen[o1].tobytes() == cen2[o2].tobytes() and np.array_equal(count[o1], count2[o2])


def bound(x_abs, voxel):
    """|centroid - exact mean| <= 0.5 ulp_f32(|x|) + v 2^-32, for cells |c| <= 2^18.  Derivation, per axis, in units of the cell (times v):
      u_i  the double quotient carries one rounding, <= 2^-53 |p / v| <= 2^-35; the subtraction of c is exact (Sterbenz, or c = 0) or
           rounds a number below 1 (2^-54);
      q_i  rounding u 2^32 to an integer moves u by at most 2^-33;
      S    is an exact integer, (double)S exact below 2^53, cnt 2^32 exact; the mean of the u's errs by at most 2^-33 + 2^-35 + 2^-54,
           the division adds 2^-54;
      c + that and the product by v: two roundings of a number below 2^18 + 1, 2^-35 each.
    Together < 2^-33 + 4 * 2^-35 = 2^-32 cells, times v; the conversion to f32 rounds once more: half an f32 ulp of the value."""
    return 0.5 * float(np.spacing(np.float32(x_abs))) + voxel * 2.0 ** -32


def test_centroids_are_the_fp64_mean_to_half_an_ulp_and_lie_in_their_box():
    worst = 0.0
    clouds = [(vc.dense_cloud(3000, voxel=v, seed=i), v) for i, v in enumerate(VOXELS)]
    clouds += [(vc.one_voxel_cloud(3000), 0.3), (vc.far_cloud(500) * np.float32(0.5), 0.3), (vc.boundary_cloud(0.3), 0.3),
               (vc.near_boundary_cloud(0.3, 0), 0.3)]
    from tests import icp_multiscale_ref as ms
    src, tgt, _, _ = ms.case()
    clouds += [(src, 0.8), (tgt, 0.4)]
    for pts, voxel in clouds:
        assert np.abs(vc.cells(pts, voxel)).max() <= 1 << 18
        cen, first, count = vc.down_sample(pts, voxel)
        means = vc.exact_means(pts, voxel)
        c = vc.cells(pts[first], voxel).astype(np.float64)
        v = float(np.float32(voxel))
        for r in range(len(first)):
            for a in range(3):
                got, mean = fractions.Fraction(float(cen[r, a])), means[r][a]
                b = bound(max(abs(float(cen[r, a])), abs(float(mean))), voxel)
                err = float(abs(got - mean))
                worst = max(worst, err / b)
                assert err <= b, (voxel, r, a, float(cen[r, a]), float(mean), err, b)
                # the closed box [c v, (c + 1) v] (products exact in fp64: 19 bits by 24), up to the same bound
                assert c[r, a] * v - b <= float(cen[r, a]) <= (c[r, a] + 1.0) * v + b
    print(f"worst |centroid - exact mean| / bound = {worst:.3f}")
