"""GPU: the one-query-per-lane nearest-neighbour search above 65 536 target points, and f1 above its lattice limit.

`knn_wave` (csrc/corr_dev.h) is compiled with 16-bit and with 32-bit indices in its per-lane LDS list; `knn_lds_plan` picks by
n2 <= 65 536, and with 32-bit indices it asks for exactly 64 KiB of LDS at K = 58 and for a single wavefront per workgroup from
K = 59 on.  `knn_points_kernel`, `spatial_var_kernel` (corr_knn.hip) and `corr_score_kernel` (corr_leftover.hip) run that search;
`corr_scores` has no lattice, no consensus pass and no cell pass above 65 471 target points.  No benchmark shape reaches any of this
(their f1 jobs are of the order of 13 000 x 30 000), so this module is the gate of the region.

A truncated or mis-strided index there is no fault but a wrong neighbour, so the clouds are built for a wrong index to show:
  * targets are KITTI-like slabs (uniform in +-60 m x +-60 m x +-3 m), half of the points snapped to a 0.3 m lattice (exact distance
    ties) and the order shuffled (tied candidates carry indices on both sides of 65 536);
  * point 65 536 + k, for up to 96 values of k, is an exact copy of a point that is NOT point k and lies metres from it, and queries
    sit on the copy, on its original and on point k: an index cut to 16 bits names another point.  (n2 = 65 537 has room for one such
    k; the cases at 65 700 / 66 000 points carry 96.);
  * queries also sit on original indices 0..63 and n2-64..n2-1, on the first and last 64 rows of the cell-sorted table (read back from
    the structure the library built), hundreds of metres outside the cloud, and one is NaN;
  * features are unit-variance noise: one wrong neighbour moves a spatial variance or a score far beyond the rounding bars.
Every reference is the CPU oracle's brute force (`knn_points`, `corr_judge`); the bars are the suite's own: searches bit-equal,
spatial variances within (knn + 20) u of the fp64 value on the oracle's neighbours (the derivation of test_f1_support_at_full_size: 34 u
for the 32 squares, 17 + 2 u for the root, knn - 2 u for the knn - 1 positive terms, 1 u for the division), scores within
_f1_error_units(K, Ns) u A of the oracle's fp64 score."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.test_abi_guard import Guard
from tests.test_gpu_parity import N_, T_, _f1_error_units

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDE = 65536                     # the last target size whose lists hold 16-bit indices (knn_lds_plan)
N_ALIAS = 96


def _npad(n):
    """GridWs.Npad (csrc/grid.h): tables are padded to a multiple of 256 points."""
    return (n + 255) // 256 * 256


@functools.lru_cache(maxsize=4)
def _slab(n, seed=0):
    """-> (points f32 [n,3], alias int64 [m,3]: rows (copy = 65 536 + k, original, k)).  Shared between the tests: never written to."""
    rng = np.random.RandomState(1000 + seed)
    p = rng.uniform(-1.0, 1.0, (n, 3)) * [60.0, 60.0, 3.0]
    snap = rng.rand(n) < 0.5
    p[snap] = np.round(p[snap] / 0.3) * 0.3
    p = p[rng.permutation(n)].astype(np.float32)
    m = max(0, min(N_ALIAS, n - WIDE))
    alias = np.zeros((m, 3), np.int64)
    for k in range(m):
        o = int(rng.randint(N_ALIAS, WIDE))
        while np.linalg.norm(p[o].astype(np.float64) - p[k]) < 5.0:
            o = int(rng.randint(N_ALIAS, WIDE))
        p[WIDE + k] = p[o]
        alias[k] = (WIDE + k, o, k)
    return p, alias


@functools.lru_cache(maxsize=8)
def _features(n, seed=0):
    return np.random.RandomState(2000 + seed).standard_normal((n, 32)).astype(np.float32)


def _table_order(dev, n):
    """Original index of every row of the sorted table that the last B = 1 `ops.knn_points` / `ops.feature_spatial_var` call built for
    an n-point cloud on this device and stream: GridWs (csrc/grid.h) starts with the packed table of Npad float4, then the sorted one,
    whose fourth word is the original index."""
    from umeregrobust_amd import ops
    ws = ops._workspace(dev, 0, "knn")
    tab = ws[_npad(n) * 16:(_npad(n) + n) * 16].view(torch.int32).view(n, 4)
    order = N_(tab[:, 3]).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "the sorted table is not where GridWs puts it"
    return order


def _marked_points(n, alias, order):
    """The target points every case looks at: aliased rows (copy, original and the point a 16-bit index would name), everything from
    65 472 to 65 791, original indices 0..63 and n-64..n-1, the first and last 64 rows of the sorted table."""
    return np.unique(np.concatenate([alias.reshape(-1), np.arange(min(n, WIDE - 64), min(n, WIDE + 256)), np.arange(min(64, n)), np.arange(max(0, n - 64), n),
                                     order[:64], order[-64:]]))


def _queries(rng, p2, alias, order, n1):
    """n1 queries (f32 [n1,3]) and the row of the NaN one: on the marked points, 8 far outside the bounding box, one NaN, the rest on
    random target points -- half of them exactly, half displaced by ~0.7 m."""
    n2 = len(p2)
    marked = _marked_points(n2, alias, order)
    assert len(marked) + 9 <= n1
    n_rest = n1 - len(marked) - 9
    rest = p2[rng.randint(0, n2, n_rest)].copy()
    rest[n_rest // 2:] += (rng.standard_normal((n_rest - n_rest // 2, 3)) * 0.7).astype(np.float32)
    far = (rng.choice([-1.0, 1.0], (8, 3)) * rng.uniform(150.0, 600.0, (8, 3))).astype(np.float32)
    q = np.concatenate([p2[marked], far, np.zeros((1, 3), np.float32), rest]).astype(np.float32)
    perm = rng.permutation(n1)
    q = q[perm]
    nan_row = int(np.flatnonzero(perm == len(marked) + 8)[0])
    q[nan_row] = (3.0, np.nan, 0.5)
    return q, nan_row


def _build_table(gpu, p2, K):
    """One query builds the target's structure for K neighbours -> the order of its sorted table."""
    from umeregrobust_amd import ops
    ops.knn_points(T_(p2[:1], gpu)[None], T_(p2, gpu)[None], K=K)
    return _table_order(gpu, len(p2))


def _assert_knn_equals_oracle(gpu, q, p2, K, nan_rows):
    """q [B,n1,3], p2 [B,n2,3], nan_rows [B]: idx and dists of ops.knn_points == the oracle's on every finite query; -1 / 0 on the NaN one.
    -> the oracle's idx."""
    from umeregrobust_amd import ops
    q_fin = q.copy()
    for b, r in enumerate(nan_rows):
        q_fin[b, r] = 0.0
    ref = orc.knn_points(q_fin, p2, K=K)
    out = ops.knn_points(T_(q, gpu), T_(p2, gpu), K=K)
    idx, dists = N_(out.idx), N_(out.dists)
    for b, r in enumerate(nan_rows):
        ok = np.ones(q.shape[1], bool)
        ok[r] = False
        bad = np.flatnonzero((idx[b, ok] != ref.idx[b, ok]).any(1))
        assert bad.size == 0, (b, K, bad.size, np.flatnonzero(ok)[bad][:4], idx[b, ok][bad][:2], ref.idx[b, ok][bad][:2])
        assert np.array_equal(dists[b, ok], ref.dists[b, ok]), (b, K)
        assert np.all(idx[b, r] == -1) and np.all(dists[b, r] == 0.0), (b, K, idx[b, r], dists[b, r])
    return ref.idx


# ---------------------------------------------------------------------------------------------------------------- 1. knn_points
@pytest.mark.parametrize("K", [2, 20, 57, 58, 59, 64])
@pytest.mark.parametrize("n2", [65536, 65537, 65700])
def test_knn_points_at_the_index_width_and_lds_plan_edges(gpu, n2, K):
    """knn_points with 1 500 queries (no multiple of 64; cell-ordered path) at the last 16-bit size, the first 32-bit size and one with
    96 aliased pairs, for K on both sides of the 32-bit plan's steps: 57 / 58 (two wavefronts, 58: exactly 64 KiB of LDS) and 59 / 64
    (one wavefront).  n2 = 65 536, K = 64 is the 16-bit list holding index 65 535.  idx and dists equal the oracle's bit for bit."""
    p2, alias = _slab(n2)
    order = _build_table(gpu, p2, K)
    q, nan_row = _queries(np.random.RandomState(n2 + K), p2, alias, order, 1500)
    ref_idx = _assert_knn_equals_oracle(gpu, q[None], p2[None], K, [nan_row])
    assert (ref_idx == n2 - 1).any() and (ref_idx == WIDE - 1).any()          # the highest index went through the lists
    if n2 > WIDE:
        assert (ref_idx >= WIDE).sum() >= len(alias) and np.isin(alias[:, 1], ref_idx).all()
    assert np.array_equal(order, _table_order(gpu, n2))                       # the queries sat on the ends of the table that was searched


def test_knn_points_unordered_path_with_32bit_indices(gpu):
    """More queries than the order buffer holds (n1 = Npad + 1): the caller's order, 32-bit lists.  Every target point is a query."""
    n2, K = 65537, 20
    p2, alias = _slab(n2)
    n1 = _npad(n2) + 1
    rng = np.random.RandomState(5)
    extra, nan_row = _queries(rng, p2, alias, np.arange(n2), n1 - n2)
    q = np.concatenate([p2, extra])
    _assert_knn_equals_oracle(gpu, q[None], p2[None], K, [n2 + nan_row])


def test_knn_points_batch_of_two_wide_clouds(gpu):
    """B = 2 through the general kernel: two different clouds of 65 537 points, each with its own queries."""
    n2, K = 65537, 20
    clouds, qs, nan_rows = [], [], []
    for seed in (0, 1):
        p2, alias = _slab(n2, seed)
        q, nan_row = _queries(np.random.RandomState(70 + seed), p2, alias, _build_table(gpu, p2, K), 1500)
        clouds.append(p2); qs.append(q); nan_rows.append(nan_row)
    _assert_knn_equals_oracle(gpu, np.stack(qs), np.stack(clouds), K, nan_rows)


# ---------------------------------------------------------------------------------------------------- 2. feature_spatial_var
def _fsv64(p, f, rows, knn):
    """fp64 mean of fp64 norms over idx[:, 1:] of the oracle's neighbours of `rows` (the reference drops rank 0 whoever that is)."""
    nb = orc.knn_points(p[rows][None], p[None], K=knn).idx[0]
    assert np.array_equal(nb[:, 0] != rows, (p[nb[:, 0]] == p[rows]).all(1) & (nb[:, 0] < rows))      # rank 0: the row, or a lower-indexed copy
    f64 = f.astype(np.float64)
    out = np.empty(len(rows))
    for a in range(0, len(rows), 4096):
        r = rows[a:a + 4096]
        out[a:a + 4096] = np.linalg.norm(f64[r][:, None, :] - f64[nb[a:a + 4096, 1:]], axis=-1).mean(-1)
    return out, nb


def _assert_fsv(gpu, p, f, knn, alias=np.zeros((0, 3), np.int64)):
    """feature_spatial_var within (knn + 20) u of the fp64 value: every row up to 33 000 points, above that >= 8 192 rows with the marked
    ones among them.  -> the device result (tensor [N])."""
    from umeregrobust_amd import ops
    N = len(p)
    v_d = ops.feature_spatial_var(T_(p, gpu)[None], T_(f, gpu)[None], knn=knn)[0]
    if N <= 33000:
        rows = np.arange(N)
    else:
        marked = _marked_points(N, alias, _table_order(gpu, N))
        rest = np.setdiff1d(np.arange(N), marked)
        rows = np.union1d(marked, np.random.RandomState(N + knn).choice(rest, 8192 - len(marked), replace=False))
        assert len(rows) == 8192
    v64, _ = _fsv64(p, f, rows, knn)
    v = N_(v_d).astype(np.float64)[rows]
    # unit-variance features: a term is of the order of 8.  (A value of 0 is possible and must come out as 0: knn = 2 on the higher-indexed of
    # two identical points -- rank 0, which is dropped, is the copy, and the one term left is the point itself.)
    assert np.median(v64) > 4.0
    err = np.abs(v - v64) / (U * np.maximum(v64, 1e-300))
    print(f"\n[fsv N {N} knn {knn}] {len(rows)} rows judged ({int((v64 == 0).sum())} of value 0), worst error {err.max():.2f} u of a bar of {knn + 20} u")
    assert np.all(np.abs(v - v64) <= (knn + 20) * U * v64), (N, knn, rows[np.argmax(err)], float(err.max()))
    return v_d


@pytest.mark.parametrize("N,knn", [(32768, 10), (32768, 50), (32769, 10), (32769, 50), (65472, 10), (65473, 10),
                                   (65536, 2), (65536, 10), (65536, 50), (65536, 64), (65537, 2), (65537, 10), (65537, 50), (65537, 64),
                                   (65700, 10), (65700, 59)])
def test_feature_spatial_var_across_its_switches(gpu, N, knn):
    """The cooperative kernel's last size and the per-lane kernel's first (32 768 / 32 769), 32 / 64 queries per wavefront (65 472 /
    65 473), 16- / 32-bit lists (65 536 / 65 537) with knn from the entry's lower limit over the reference's default (10) and
    FeatureCorrelator's 50 to the upper limit; 65 700 points carry 96 aliased pairs (knn = 59: the single-wavefront plan)."""
    p, alias = _slab(N)
    _assert_fsv(gpu, p, _features(N), knn, alias)


@pytest.mark.parametrize("case", ["N=knn=2", "N=knn=64", "N=65,knn=64", "duplicates"])
def test_feature_spatial_var_small_clouds(gpu, case):
    """The cooperative kernel at its small ends: a cloud that is one neighbourhood (N = knn = 2 and 64), one point more (65, 64), and
    3 000 points of which 300 are exact copies of lower-indexed points -- for those the dropped rank 0 is the original, not the point."""
    rng = np.random.RandomState(len(case))
    N, knn = {"N=knn=2": (2, 2), "N=knn=64": (64, 64), "N=65,knn=64": (65, 64), "duplicates": (3000, 10)}[case]
    p = (rng.uniform(-1.0, 1.0, (N, 3)) * [20.0, 20.0, 2.0]).astype(np.float32)
    if case == "duplicates":
        p[-300:] = p[rng.choice(N - 300, 300, replace=False)]
    f = rng.standard_normal((N, 32)).astype(np.float32)
    _assert_fsv(gpu, p, f, knn)
    if case == "duplicates":
        nb = orc.knn_points(p[None], p[None], K=knn).idx[0]
        assert (nb[-300:, 0] < N - 300).all() and (nb[:-300, 0] == np.arange(N - 300)).all()


def test_feature_spatial_var_batch_of_two_equals_single_calls(gpu):
    """B = 2 at N = 65 537, knn = 10: the bytes of the two single calls (each of which meets the bar)."""
    from umeregrobust_amd import ops
    N, knn = 65537, 10
    (p0, a0), (p1, a1) = _slab(N, 0), _slab(N, 1)
    f0, f1 = _features(N, 0), _features(N, 1)
    one = [_assert_fsv(gpu, p, f, knn, a) for p, f, a in ((p0, f0, a0), (p1, f1, a1))]
    two = ops.feature_spatial_var(T_(np.stack([p0, p1]), gpu), T_(np.stack([f0, f1]), gpu), knn=knn)
    assert torch.equal(two[0].view(torch.int32), one[0].view(torch.int32)) and torch.equal(two[1].view(torch.int32), one[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 3. corr_scores
def _rigid(axis, ang_deg, shift):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    th = np.deg2rad(ang_deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = shift
    return T


def _hypotheses(rng, T_true, n_near, n_far, nan_at):
    """[true | n_near within 5 degrees / 0.3 m of it | n_far far off], one more with a NaN entry inserted at `nan_at` (None: none)."""
    Ts = [T_true]
    for _ in range(n_near):
        v = rng.standard_normal(3)
        Ts.append(_rigid(rng.standard_normal(3), rng.uniform(0.2, 5.0), v / np.linalg.norm(v) * rng.uniform(0.02, 0.3)) @ T_true)
    for _ in range(n_far):
        v = rng.standard_normal(3)
        Ts.append(_rigid(rng.standard_normal(3), rng.uniform(20.0, 180.0), v / np.linalg.norm(v) * rng.uniform(10.0, 150.0)) @ T_true)
    Ts = np.stack(Ts).astype(np.float32)
    if nan_at is not None:
        bad = Ts[1].copy()
        bad[1, 3] = np.nan
        Ts = np.insert(Ts, nan_at, bad, axis=0)
    return Ts


@functools.lru_cache(maxsize=2)
def _corr_job(Nt, Ns=1500):
    """-> (src [Ns,3], tgt [Nt,3], vp [Ns,32], vq [Nt,32], T_true [4,4] f64).  The source points are target points under the inverse of
    T_true (the marked ones among them; half exactly, half with 2 cm of noise) and carry their twins' features plus noise, so the true
    transform wins by a wide margin."""
    rng = np.random.RandomState(3000 + Nt)
    tgt, alias = _slab(Nt)
    marked = _marked_points(Nt, alias, np.arange(Nt))
    pick = np.concatenate([marked, rng.choice(np.setdiff1d(np.arange(Nt), marked), Ns - len(marked), replace=False)])
    pick = pick[rng.permutation(Ns)]
    T_true = _rigid([0.2, -0.1, 1.0], 3.0, [2.0, -1.0, 0.3])
    img = tgt[pick].astype(np.float64)
    img[Ns // 2:] += rng.standard_normal((Ns - Ns // 2, 3)) * 0.02
    src = ((img - T_true[:3, 3]) @ T_true[:3, :3]).astype(np.float32)
    vq = _features(Nt)
    vp = (vq[pick] + 0.25 * rng.standard_normal((Ns, 32))).astype(np.float32)
    return src, tgt, vp, vq, T_true


def _assert_scores(S, T, src, tgt, vp, vq, K, sigma, what):
    """|S - S64| Ns <= _f1_error_units(K, Ns) u A on every finite hypothesis (a NaN one, at most one, is all that is excluded), and the same arg-max."""
    Ns = len(src)
    fin = np.isfinite(T.reshape(len(T), -1)).all(1)
    assert fin.sum() >= len(T) - 1
    j = orc.corr_judge(T[fin], src, tgt, K, vp, vq, sigma)
    bar = _f1_error_units(K, Ns) * U * j.absum
    err = np.abs(S[fin].astype(np.float64) - j.score) * Ns
    print(f"\n[corr {what}] K {K}: worst |err| / bar {float((err / bar).max()):.4f} over {int(fin.sum())} hypotheses; scores {S}")
    assert np.all(err <= bar), (what, K, np.flatnonzero(fin)[np.argmax(err / bar)], float((err / bar).max()))
    assert int(np.argmax(np.where(fin, S, -np.inf))) == int(np.flatnonzero(fin)[np.argmax(j.score)]) == 0, (what, S, j.score)


def _dev_job(gpu, Nt):
    src, tgt, vp, vq, T_true = _corr_job(Nt)
    return tuple(T_(x, gpu) for x in (src, tgt, vp, vq))


@pytest.mark.parametrize("Nt", [65471, 65472, 65536, 65537])
def test_corr_scores_across_the_lattice_limit_and_the_index_width(gpu, Nt):
    """Ns = 1 500, K = 20, sigma = 1.5, twelve hypotheses (the true one, seven near it, three far off, one with a NaN entry) at the last size
    with a lattice (65 471), the first without (65 472: 16-bit grid walk for every query), and on both sides of the index width."""
    from umeregrobust_amd import ops
    K, sigma = 20, 1.5
    src, tgt, vp, vq, T_true = _corr_job(Nt)
    T = _hypotheses(np.random.RandomState(Nt), T_true, 7, 3, nan_at=5)
    assert T.shape == (12, 4, 4)
    d = _dev_job(gpu, Nt)
    T_d = T_(T, gpu)
    S = N_(ops.corr_scores(*d, T_d, K=K, sigma=sigma))
    _assert_scores(S, T, src, tgt, vp, vq, K, sigma, f"Nt {Nt} default")
    again = N_(ops.corr_scores(*d, T_d, K=K, sigma=sigma))
    assert np.array_equal(S.view(np.uint32), again.view(np.uint32))
    # the NaN hypothesis does not disturb the others: the eleven were judged above with it in the call, and here without.  (Not the same bits: the
    # source's processing order comes from the mean rotation of the call's hypotheses, so the chunks' sums are taken in another order.)
    fin = np.isfinite(T.reshape(12, -1)).all(1)
    alone = N_(ops.corr_scores(*d, T_(T[fin], gpu), K=K, sigma=sigma))
    _assert_scores(alone, T[fin], src, tgt, vp, vq, K, sigma, f"Nt {Nt} without the NaN hypothesis")
    LC = ops.CORR_FORCE_LATTICE | ops.CORR_FORCE_CONSENSUS
    if Nt >= 65472:
        # corr_ws routes every flag set to the one grid-walk kernel here: the same bytes
        for fl in (LC, ops.CORR_BOUND_OUTSIDE, ops.CORR_NO_LATTICE):
            assert ops._lib.load().umereg_corr_workspace_bytes_ex(1500, Nt, 12, fl) == ops._lib.load().umereg_corr_workspace_bytes_ex(1500, Nt, 12, 0)
            s = N_(ops.corr_scores(*d, T_d, K=K, sigma=sigma, flags=fl))
            assert np.array_equal(s.view(np.uint32), S.view(np.uint32)), (Nt, hex(fl), s, S)
    else:
        # the forced routes run: the lattice is built (marked cells) / the consensus pass serves queries, and both meet the same bar
        s, _, hdr = ops.corr_scores_profile(*d, T_d, K=K, sigma=sigma, flags=ops.CORR_FORCE_LATTICE | ops.CORR_NO_CONSENSUS)
        assert hdr is not None and int(hdr[3]) > 0 and int(hdr[7]) == 0, hdr[:16]
        _assert_scores(N_(s), T, src, tgt, vp, vq, K, sigma, f"Nt {Nt} lattice, no consensus")
        s, _, hdr = ops.corr_scores_profile(*d, T_d, K=K, sigma=sigma, flags=LC)
        assert hdr is not None and int(hdr[7]) > 0, hdr[:16]
        _assert_scores(N_(s), T, src, tgt, vp, vq, K, sigma, f"Nt {Nt} consensus")


@pytest.mark.parametrize("K", [58, 59, 64])
def test_corr_scores_wide_target_at_the_lds_plan_edges(gpu, K):
    """Nt = 65 537 with four hypotheses: K = 58 is two wavefronts on exactly 64 KiB of LDS, from K = 59 on the workgroup is one wavefront."""
    from umeregrobust_amd import ops
    Nt, sigma = 65537, 1.5
    src, tgt, vp, vq, T_true = _corr_job(Nt)
    T = _hypotheses(np.random.RandomState(K), T_true, 1, 1, nan_at=2)
    assert T.shape == (4, 4, 4)
    d = _dev_job(gpu, Nt)
    S = N_(ops.corr_scores(*d, T_(T, gpu), K=K, sigma=sigma))
    _assert_scores(S, T, src, tgt, vp, vq, K, sigma, f"Nt {Nt} M 4")
    assert np.array_equal(S.view(np.uint32), N_(ops.corr_scores(*d, T_(T, gpu), K=K, sigma=sigma)).view(np.uint32))


def test_corr_scores_wide_target_raw_abi_between_canaries(gpu):
    """(1 500, 65 537, 12) through the C ABI with the workspace at exactly umereg_corr_workspace_bytes_ex, every buffer between 4 KiB
    canaries, twice with different garbage in the workspace and poison in the output: no guard byte touched, the same bytes, and
    they are the torch-facing wrapper's."""
    from umeregrobust_amd import ops
    Ns, Nt, M, K, sigma = 1500, 65537, 12, 20, 1.5
    src, tgt, vp, vq, T_true = _corr_job(Nt)
    T = _hypotheses(np.random.RandomState(Nt), T_true, 7, 3, nan_at=5)
    runs = []
    for run in (0, 1):
        G = Guard(gpu, run)
        with torch.cuda.device(gpu):
            a = [G.inp(x)[0] for x in (src, tgt, vp, vq, T)]
            sc, tsc = G.out((M,), torch.float32, "scores")
            ws, nws = G.ws(G.lib.umereg_corr_workspace_bytes_ex(Ns, Nt, M, 0), "corr_ws")
            G.call("umereg_corr_scores_ex_f32", *a, Ns, Nt, M, K, sigma, 0, sc, ws, nws, G.stream)
        G.check()
        runs.append(N_(tsc).copy())
        del G
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), runs
    S = N_(ops.corr_scores(*_dev_job(gpu, Nt), T_(T, gpu), K=K, sigma=sigma))
    assert np.array_equal(runs[0].view(np.uint32), S.view(np.uint32))
    _assert_scores(runs[0], T, src, tgt, vp, vq, K, sigma, "raw ABI")


# ------------------------------------------------------------------------------------------------------- 4. the caller's surface
def test_feature_correlator_on_a_wide_target(gpu):
    """FeatureCorrelator.feature_corr_hypothesis_test with 1 500 source points and a 66 000-point target: feature_spatial_var (knn = 50)
    per cloud, the weighted features, the scores.  The reference side is the oracle's throughout: fp64 spatial variances on its
    neighbours, fp64 column means, `corr_judge` on the weighted features rounded once.  The returned transform is the oracle's
    arg-max and `last_scores` meets the bar of part 3."""
    from umeregrobust_amd.utils.loc_utils import FeatureCorrelator
    Nt, Ns, K, sigma = 66000, 1500, 20, 1.5
    src, tgt, f_s, f_t, T_true = _corr_job(Nt)
    T = _hypotheses(np.random.RandomState(4), T_true, 7, 3, nan_at=None)
    t = lambda a: T_(a, gpu)[None]                                            # noqa: E731
    fc = FeatureCorrelator(sigma=sigma, n_hypotheses=10, corr_num_nn=K)
    best = fc.feature_corr_hypothesis_test(t(src), t(tgt), t(f_s), t(f_t), T_(T, gpu))
    assert fc.last_scores_exact
    S = N_(fc.last_scores)
    w_s, _ = _fsv64(src, f_s, np.arange(Ns), 50)
    w_t, _ = _fsv64(tgt, f_t, np.arange(Nt), 50)
    m64 = np.concatenate([f_s, f_t]).astype(np.float64).mean(0)
    vp = ((f_s.astype(np.float64) - m64) * w_s[:, None]).astype(np.float32)
    vq = ((f_t.astype(np.float64) - m64) * w_t[:, None]).astype(np.float32)
    j = orc.corr_judge(T, src, tgt, K, vp, vq, sigma)
    win = int(np.argmax(j.score))
    assert win == 0 and int(fc.last_best_index) == win and np.array_equal(N_(best), T[win]), (win, int(fc.last_best_index), j.score, S)
    bar = _f1_error_units(K, Ns) * U * j.absum
    err = np.abs(S.astype(np.float64) - j.score) * Ns
    print(f"\n[wide correlator] worst |err| / bar {float((err / bar).max()):.4f}; scores {S}")
    assert np.all(err <= bar), (int(np.argmax(err / bar)), float((err / bar).max()))
