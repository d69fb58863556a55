"""The two kernels that call polar_rotation (csrc/polar.h), on cross-moments / covariances with a thin spectrum.

rtume_kernel (a6) and icp_step_kernel (f2) are held to the project's own bars -- |dR| <= 1e-6, |dt| <= 1e-5 max(1, |t|) against
oracle.batch_estimate_transform_ume_f64, and 1e-9 against oracle.icp_point_to_point -- wherever the PROBLEM's first-order bound
(the cross-moment's own rounding over the gap s2 + det s3; no term for a solve through A^T A) is two orders of magnitude below the
bar.  tests/test_polar_cpu.py judges the routine itself and asserts that the constructed inputs used here qualify.
Also here: the lane-group, round, block and clamped-cell edges of icp_eval_kernel and its strict distance cut.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import polar_cases as pc
from tests.test_gpu_parity import _KAPPA_R_MAX, _KAPPA_T_MAX, _U64, N_, T_, _icp_case

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ a6: RTUME
def _rtume_judge(T_hip, T64, cf, tag):
    """the bars on every hypothesis that qualifies; finiteness, the last row and det R = 1 on all.  -> (qualifying mask, dR, dt_rel)"""
    T_hip = T_hip.astype(np.float64)
    tn = np.maximum(1.0, np.linalg.norm(T64[:, :3, 3], axis=1))
    ok = np.isfinite(T64).all(axis=(1, 2)) & (cf.kappa_R_problem <= _KAPPA_R_MAX) & (cf.kappa_t_problem <= _KAPPA_T_MAX * tn)
    assert np.isfinite(T_hip).all() and np.all(T_hip[:, 3] == [0, 0, 0, 1]), tag
    assert np.abs(np.linalg.det(T_hip[:, :3, :3]) - 1.0).max() <= 1e-5, tag
    dR = np.abs(T_hip[:, :3, :3] - T64[:, :3, :3]).max(axis=(1, 2))
    dt = np.abs(T_hip[:, :3, 3] - T64[:, :3, 3]).max(axis=1) / tn
    return ok, dR, dt


@pytest.mark.parametrize("family", ["plain", "shift"])
def test_rtume_sigma_ladder(gpu, family):
    """4097 hypotheses over the 80 cells of the ladder (s2/s1 = 1 .. 1e-7 x s3/s2 x det sign, 51 a cell), plain, through
    g_index / h_index and through h_of_g: every hypothesis whose problem bound meets _KAPPA_*_MAX -- all cells with a gap -- meets
    |dR| <= 1e-6 and |dt| <= 1e-5 max(1, |t|)."""
    from umeregrobust_amd import ops
    n = 4097
    G, H, cell = pc.rtume_ladder(n, family)
    T64, cf = orc.batch_estimate_transform_ume_f64(G, H)
    has_gap = np.array([not (r3 == 1.0 and det == -1) for (_, r3, det) in pc.CELLS])[cell]
    Gd, Hd = T_(G, gpu), T_(H, gpu)
    rng = np.random.RandomState(5)
    perm = rng.permutation(n)
    hperm = rng.permutation(n)                          # h_of_g: G row i is matched to row hperm[i] of a shuffled H
    Hs = np.empty_like(H)
    Hs[hperm] = H
    routes = {
        "plain": (N_(ops.rtume_solve(Gd, Hd)[0]), np.arange(n)),
        "indexed": (N_(ops.rtume_solve(Gd, Hd, T_(perm, gpu), T_(perm, gpu))[0]), perm),
        "h_of_g": (N_(ops.rtume_solve(Gd, T_(Hs, gpu), T_(perm, gpu), h_of_g=T_(hperm, gpu))[0]), perm),
    }
    Tx, _ = orc.batch_estimate_transform_ume_f64(G, Hs, perm, hperm[perm])
    assert np.array_equal(Tx, T64[perm])                # (the oracle's own gathers)
    for name, (T_hip, rows) in routes.items():
        cfr = type(cf)(*[np.asarray(f)[rows] for f in cf])
        ok, dR, dt = _rtume_judge(T_hip, T64[rows], cfr, (family, name))
        assert ok[has_gap[rows]].all(), (family, name, int((~ok & has_gap[rows]).sum()))     # the whole ladder qualifies
        for r2 in pc.R2:
            m = ok & np.array([pc.CELLS[c][0] == r2 for c in cell[rows]])
            print(f"[rtume ladder {family} {name}] s2/s1={r2:.0e}: {int(m.sum())} judged, max |dR| {dR[m].max():.2e}, "
                  f"max |dt|/max(1,|t|) {dt[m].max():.2e}")
        assert dR[ok].max() <= 1e-6, (family, name, dR[ok].max(), cell[rows][ok][dR[ok].argmax()])
        assert dt[ok].max() <= 1e-5, (family, name, dt[ok].max(), cell[rows][ok][dt[ok].argmax()])
    assert np.array_equal(routes["indexed"][0], routes["plain"][0][perm])
    assert np.array_equal(routes["h_of_g"][0], routes["plain"][0][perm])


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_rtume_thin_spectra_at_the_workgroup_edge(gpu, n):
    """eight hypotheses share a workgroup: n around that edge, drawn from the thinnest rungs (s2/s1 = 1e-5 .. 1e-7), the three routes"""
    from umeregrobust_amd import ops
    thin = [i for i, (r2, r3, det) in enumerate(pc.CELLS) if r2 <= 1e-5 and not (r3 == 1.0 and det == -1)]
    for family in ("plain", "shift"):
        G, H, cell = pc.rtume_ladder(n, family, seed=n, order=thin[n::3])
        T64, cf = orc.batch_estimate_transform_ume_f64(G, H)
        rev = np.arange(n)[::-1].copy()
        Hs = np.empty_like(H)
        Hs[rev] = H
        outs = [(N_(ops.rtume_solve(T_(G, gpu), T_(H, gpu))[0]), np.arange(n)),
                (N_(ops.rtume_solve(T_(G, gpu), T_(H, gpu), T_(rev, gpu), T_(rev, gpu))[0]), rev),
                (N_(ops.rtume_solve(T_(G, gpu), T_(Hs, gpu), h_of_g=T_(rev, gpu))[0]), np.arange(n))]
        for T_hip, rows in outs:
            assert T_hip.shape == (n, 4, 4)
            ok, dR, dt = _rtume_judge(T_hip, T64[rows], type(cf)(*[np.asarray(f)[rows] for f in cf]), (family, n))
            assert ok.all()
            assert dR.max() <= 1e-6 and dt.max() <= 1e-5, (family, n, dR.max(), dt.max())


# ------------------------------------------------------------------------------------------------ f2: ICP
_ICP_BAR = 1e-9


def _first_covariance(src, tgt, T0, max_dist):
    """(problem bound u |A|_F / (s2 + det s3) of the first Umeyama update, |centroid|)"""
    idx, _, _, q = orc.icp_evaluate(src, tgt, T0, max_dist)
    ok = idx >= 0
    p_, q_ = q[ok], np.asarray(tgt, np.float32).astype(np.float64)[idx[ok]]
    cov = (q_ - q_.mean(0)).T @ (p_ - p_.mean(0)) / ok.sum()
    U, S, Vt = np.linalg.svd(cov)
    gap = S[1] + np.sign(np.linalg.det(U @ Vt)) * S[2]
    return (_U64 * np.linalg.norm(cov) / gap if gap > 0 else np.inf), float(np.linalg.norm(q_.mean(0))), S


def _icp_same(out, ref, tag, T_tol=1e-9):
    assert out.iterations == ref[3], (tag, out.iterations, ref[3])
    assert abs(out.fitness - ref[1]) < 1e-12 and abs(out.inlier_rmse - ref[2]) < 1e-9, (tag, out.fitness, ref[1], out.inlier_rmse, ref[2])
    if T_tol is not None:
        assert np.abs(out.transformation - ref[0]).max() < T_tol, (tag, np.abs(out.transformation - ref[0]).max())


@pytest.mark.parametrize("kind,w", [("segment", 1.0), ("segment", 0.1), ("segment", 0.02), ("segment", 0.005), ("planar", 0.0),
                                    ("collinear", 0.0)])
def test_icp_thin_clouds_vs_oracle(gpu, kind, w):
    """A 20 m segment with transverse scatter w, a plane and a line, identity pairing.  Iterations, fitness (1e-12) and RMSE (1e-9) as
    in test_icp_point_to_point_vs_oracle on every case.  The transform: to 1e-9 (translation: 1e-9 max(1, |centroid|)) where the
    covariance's problem bound is two orders below that (w = 1 m, 0.1 m, the plane -- rank 2 leaves R determined); beyond it (2 cm, 5 mm)
    to 100 x bound, the same rule read the other way round; on the line (rank 1: R is free about the line) by det R = 1 and by where
    the source points end up."""
    from umeregrobust_amd import ops
    src, tgt, T0, max_dist = pc.icp_thin_case(kind, w)
    bound, cent, S = _first_covariance(src, tgt, T0, max_dist)
    judged = bound <= _ICP_BAR / 100
    assert judged == ((kind, w) in (("segment", 1.0), ("segment", 0.1), ("planar", 0.0))), (kind, w, bound)   # (fixed by the construction)
    barR = _ICP_BAR if judged else 100 * bound
    for max_it in (0, 1, 2, 30):
        ref = orc.icp_point_to_point(src, tgt, T0, max_dist, max_it)
        out = ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), T0, max_dist, max_it)
        _icp_same(out, ref, (kind, w, max_it), T_tol=None)
        assert ref[1] == 1.0                                                           # the identity pairing, all of it
        To = out.transformation
        assert np.all(To[3] == [0, 0, 0, 1]) and abs(np.linalg.det(To[:3, :3]) - 1.0) <= 1e-12
        assert np.abs(To[:3, :3].T @ To[:3, :3] - np.eye(3)).max() <= 1e-12
        dR, dt = np.abs(To[:3, :3] - ref[0][:3, :3]).max(), np.abs(To[:3, 3] - ref[0][:3, 3]).max()
        s64 = src.astype(np.float64)
        moved = np.abs((s64 @ To[:3, :3].T + To[:3, 3]) - (s64 @ ref[0][:3, :3].T + ref[0][:3, 3])).max()
        print(f"[icp thin {kind} w={w} max_it={max_it}] sigma {S}, bound {bound:.2e}, iterations {out.iterations}, |dR| {dR:.2e}, "
              f"|dt| {dt:.2e}, points moved apart {moved:.2e}, |rmse - oracle's| {abs(out.inlier_rmse - ref[2]):.2e}")
        if np.isfinite(barR) and barR < 0.1:
            assert dR <= barR and dt <= barR * max(1.0, cent), (kind, w, max_it, dR, dt, barR)
        else:
            # rank 1: both transforms put every source point in the same place along the line to the bar; across it they may differ by a
            # rotation about the line, which moves no point of the line
            assert kind == "collinear" and moved <= _ICP_BAR * max(1.0, cent), (kind, moved)


@pytest.mark.parametrize("n_src", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 129])
def test_icp_source_count_edges(gpu, n_src):
    """eight lanes a point, 32 points a round, 64 a block: n_src on each edge"""
    from umeregrobust_amd import ops
    src, tgt, gt, T0 = _icp_case(40 + n_src, n_tgt=900, n_src=129)
    src = src[:n_src]
    for max_it in (0, 1, 30):
        _icp_same(ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), T0, 0.2, max_it),
                  orc.icp_point_to_point(src, tgt, T0, 0.2, max_it), (n_src, max_it))


def _knn_grid(tgt):
    """The K = 1 search grid of a target cloud as grid.h lays it out (load_grid_compute, kNN mode), restated in fp32 on the host:
    -> (min [3], inv [3], n [3])."""
    f = np.float32
    mn, mx = tgt.min(axis=0).astype(f), tgt.max(axis=0).astype(f)
    e = np.maximum(mx - mn, f(1e-3))
    area = f(f(f(e[0] * e[1]) * e[2]) / e.min())
    c = f(0.5) * np.sqrt(f(f(f(2.0) * area) / f(f(3.14159265) * f(tgt.shape[0]))), dtype=f)
    for _ in range(64):
        cap = [1 if e[a] < f(4.0) * c else min(int(e[a] / c) + 2, 64) for a in range(3)]
        if cap[0] * cap[1] * cap[2] <= 4096:
            break
        c = f(c * f(1.1))
    inv, n = np.empty(3, f), np.empty(3, np.int64)
    for a in range(3):
        cs = f(max(f(c * f(1.0001)), f(f(max(mx[a] - mn[a], f(0))) / f(cap[a]) * f(1.0001))) + f(1e-30))
        inv[a] = f(1.0) / cs
        n[a] = min(max(int(np.floor(f(max(mx[a] - mn[a], f(0))) * inv[a])) + 1, 1), cap[a])
    return mn, inv, n


def _row_walks(q, tgt, max_dist):
    """For every query q[i] (fp32) the lengths of the candidate runs icp_eval_kernel's lane group walks: one per (z, y) row of its
    cell range, the points in cells x0 .. x1 of that row.  Also the smallest distance, in cells, of any point or range end from a
    cell boundary (the host restatement is only trusted away from the boundaries)."""
    f = np.float32
    mn, inv, n = _knn_grid(tgt)
    t_of = lambda p: ((p.astype(f) - mn) * inv).astype(f)                       # noqa: E731
    cell_of = lambda t: np.clip(np.floor(t).astype(np.int64), 0, n - 1)        # noqa: E731
    tc = cell_of(t_of(tgt))
    r = f(f(max_dist) * f(1.001)) + f(1e-6)
    lo_t, hi_t = t_of(q - r), t_of(q + r)
    lo, hi = cell_of(lo_t), cell_of(hi_t)
    # (t == 0 is exact on both sides: the point that defines the box's minimum)
    margin = min(np.abs(x - np.round(x))[x != 0].min() for x in (t_of(tgt), lo_t, hi_t))
    walks = []
    for i in range(q.shape[0]):
        w = []
        for z in range(lo[i, 2], hi[i, 2] + 1):
            for y in range(lo[i, 1], hi[i, 1] + 1):
                w.append(int(((tc[:, 2] == z) & (tc[:, 1] == y) & (tc[:, 0] >= lo[i, 0]) & (tc[:, 0] <= hi[i, 0])).sum()))
        walks.append(w)
    return walks, float(margin), n


def test_icp_target_rows_of_1_7_8_9_points(gpu):
    """Candidate runs of 1, 7, 8 and 9 points (the eight lanes of a group walk a run together, `k += 8`: one lane idle, all busy once,
    a second trip for one lane): four short runs along x, far apart in y and z, every source point next to one of them.  The runs'
    lengths are CHECKED on the host against the grid the kernel builds (_row_walks), not assumed."""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(61)
    runs, src = [], []
    for j, m in enumerate((1, 7, 8, 9)):
        base = np.array([2.0 * j + 0.25, 6.0 * j, 1.5 * j])
        pts = base + np.stack([np.arange(m) * 0.03125, np.zeros(m), np.zeros(m)], axis=1)
        runs.append(pts)
        src.append(pts + rng.uniform(-0.01, 0.01, (m, 3)))
        src.append(pts[-1:] + [0.03, 0.01, -0.01])                    # beyond the run's last point
    tgt = np.concatenate(runs).astype(np.float32)
    src = np.concatenate(src).astype(np.float32)
    T0 = np.eye(4); T0[:3, 3] = [0.004, -0.003, 0.002]
    q = orc.icp_evaluate(src, tgt, T0, 0.2)[3].astype(np.float32)
    walks, margin, n = _row_walks(q, tgt, 0.2)
    assert margin > 1e-4, margin                                       # (fp32 rounding of a cell coordinate <= 22: 2e-6)
    owner = np.repeat(np.arange(4), [2, 8, 9, 10])                     # which run each source point sits at
    for j, m in enumerate((1, 7, 8, 9)):
        for i in np.flatnonzero(owner == j):
            assert max(walks[i]) == m and sum(walks[i]) == m, (j, m, i, walks[i], n)    # the whole run, in ONE walk, and nothing else
    for max_it in (0, 1, 30):
        ref = orc.icp_point_to_point(src, tgt, T0, 0.2, max_it)
        _icp_same(ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), T0, 0.2, max_it), ref, max_it)
    assert ref[1] == 1.0
    idx = orc.icp_evaluate(src, tgt, T0, 0.2)[0]
    assert set(idx.tolist()) == set(range(25))                        # every point of every run is some source point's neighbour


def test_icp_source_points_outside_the_target_box(gpu):
    """Source points carried outside the target's bounding box by less than max_dist (they still match, through the clamped edge cells)
    and by much more (no match), on every face."""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(62)
    g = np.arange(9) * 0.5
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)        # the box [0, 4]^3
    face = tgt[(tgt.min(axis=1) == 0.0) | (tgt.max(axis=1) == 4.0)]
    out_dir = np.where(face == 0.0, -1.0, 0.0) + np.where(face == 4.0, 1.0, 0.0)
    near = face + out_dir * rng.uniform(0.05, 0.15, (face.shape[0], 1))
    far = face[::7] + out_dir[::7] * rng.uniform(3.0, 500.0, (face[::7].shape[0], 1))
    inside = tgt[rng.choice(tgt.shape[0], 100, replace=False)] + rng.uniform(-0.05, 0.05, (100, 3))
    src = np.concatenate([near, far, inside]).astype(np.float32)
    T0 = np.eye(4); T0[:3, 3] = [0.01, -0.01, 0.005]
    for max_it in (0, 1, 30):
        ref = orc.icp_point_to_point(src, tgt, T0, 0.2, max_it)
        _icp_same(ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), T0, 0.2, max_it), ref, max_it)
    idx = orc.icp_evaluate(src, tgt, T0, 0.2)[0]
    n_near, n_far = near.shape[0], far.shape[0]
    assert (idx[:n_near] >= 0).mean() > 0.9 and (idx[n_near:n_near + n_far] < 0).all()


def test_icp_strict_distance_cut(gpu):
    """d^2 == max_dist^2 exactly in fp32 (coordinates on a 2^-6 lattice, max_dist = 0.25): excluded by the strict <, like open3d's
    search radius; one fp32 step inside it: included."""
    from umeregrobust_amd import ops
    tgt = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [0, 8, 2], [4, 0, 1], [2, 6, 1]], np.float32)
    inside = np.nextafter(np.float32(0.25), np.float32(0))
    off = np.array([[0.25, 0, 0], [0, -0.25, 0], [0, 0, 0.25], [inside, 0, 0], [0, inside, 0], [0.125, 0.125, 0.125]], np.float32)
    src = (tgt + off).astype(np.float32)
    d2 = ((src - tgt) ** 2).astype(np.float32)
    d2 = (d2[:, 0] + d2[:, 1]) + d2[:, 2]
    assert np.array_equal(d2[:3], np.full(3, np.float32(0.0625))) and (d2[3:] < np.float32(0.0625)).all()
    ref0 = orc.icp_point_to_point(src, tgt, np.eye(4), 0.25, 0)
    out0 = ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), np.eye(4), 0.25, 0)
    assert ref0[1] == 0.5 and out0.fitness == 0.5                     # three of six: the three at the exact radius are out
    _icp_same(out0, ref0, "cut")
    for max_it in (1, 30):
        _icp_same(ops.icp_point_to_point(T_(src, gpu), T_(tgt, gpu), np.eye(4), 0.25, max_it),
                  orc.icp_point_to_point(src, tgt, np.eye(4), 0.25, max_it), ("cut", max_it))
