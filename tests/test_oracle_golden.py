"""CPU: pins the oracle (oracle/oracle.py + ume_oracle.c) to golden vectors produced by the
reference's own Python (oracle/gen_golden.py).  No GPU, no /root/reference at run time."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.conftest import load_golden


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_ball_query_c_vs_numpy_vs_golden(tag):
    g = load_golden("g12_ballquery_moments.npz")
    K, r = int(g[f"K_{tag}"]), float(g[f"r_{tag}"])
    bq = orc.ball_query(g["kpts"][None], g["pts"][None], K=K, radius=r, return_nn=True)
    # bit-exact indices: C loop == vectorised numpy restatement == committed fixture
    assert np.array_equal(bq.idx[0], g[f"idx_{tag}"].astype(np.int64))
    assert np.array_equal(orc.ball_query_numpy(g["kpts"], g["pts"], K, r), bq.idx[0])
    assert np.array_equal(bq.dists[0], g[f"dists_{tag}"])
    if f"nn_{tag}" in g:
        assert np.array_equal(bq.knn[0], g[f"nn_{tag}"])
    # semantics: ascending indices, -1 padding at the tail, empty ball row is all -1
    idx = bq.idx[0]
    for row in idx:
        v = row[row >= 0]
        assert np.all(np.diff(v) > 0)
        assert np.all(row[len(v):] == -1)
    assert np.all(idx[62] == -1)          # keypoint at (500,500,500)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_moments_vs_reference(tag):
    """my_ume_generation (reference evaluate.py:50-60) golden vs the three oracle forms."""
    g = load_golden("g12_ballquery_moments.npz")
    K, r = int(g[f"K_{tag}"]), float(g[f"r_{tag}"])
    F_ref = g[f"F_{tag}"]
    F_np = orc.my_ume_generation(g["pts"][None], g["kpts"][None], g["feat"][None], K, r)[0]
    F_32 = orc.ume_moments(g["pts"], g["kpts"], g["feat"], K, r, accum="f32")
    F_64, cnt = orc.ume_moments(g["pts"], g["kpts"], g["feat"], K, r, accum="f64", return_count=True)
    assert np.array_equal(cnt, (g[f"idx_{tag}"] >= 0).sum(-1))
    # scale per keypoint: entries are O(|p|) after normalisation; compare relative to the row max
    scale = np.abs(F_ref).max(axis=(1, 2), keepdims=True) + 1e-30
    for F in (F_np, F_32, F_64):
        err = np.abs(F - F_ref) / scale
        assert err.max() < 2e-4, err.max()
        assert np.median(err) < 2e-6
    # empty ball -> exact zeros in every form (0 / 1e-6)
    for F in (F_ref, F_np, F_32, F_64):
        assert np.all(F[62] == 0)


def well_conditioned(ume, max_cond=1e6):
    s = np.linalg.svd(ume.astype(np.float64), compute_uv=False)
    return s[:, -1] * max_cond > s[:, 0]


def test_ume_cdist_vs_reference():
    g = load_golden("g3_ume_cdist.npz")
    D = orc.ume_cdist(g["ume1"][None], g["ume2"][None])[0]
    D64 = orc.ume_cdist_f64(g["ume1"], g["ume2"])
    # Rank-deficient UMEs (flat-ground balls: every neighbour on one lattice z => rank 3; the
    # injected zero / rank-1 rows) have noise-defined trailing basis vectors in ANY fp32 QR,
    # the reference's included -> compare only well-conditioned pairs.
    ok = np.outer(well_conditioned(g["ume1"]), well_conditioned(g["ume2"]))
    assert ok.mean() > 0.8 and not ok[63].any() and not ok[:, 95].any()
    # fp32 projector/cdist form has ~1e-3 absolute noise near D ~ 0
    assert np.abs(D - g["D"])[ok].max() < 3e-3
    assert np.abs(D64 - g["D"])[ok].max() < 3e-3
    am = orc.row_argmin(np.where(ok, D, 9.0))
    am_ref = orc.row_argmin(np.where(ok, g["D"], 9.0))
    rows = ok.any(axis=1)
    assert (am[rows] == am_ref[rows]).mean() >= 0.98
    tw = np.array([i for i in range(32) if ok[i, i]])      # physical twins are the matches
    assert len(tw) >= 28 and np.array_equal(am[tw], tw)
    assert np.array_equal(orc.row_argmin(np.where(ok, D64, 9.0))[tw], tw)
    # zero UME against well-conditioned ones: LAPACK tau = 0 -> Q = I[:, :4]; the fp64
    # Householder follows the same convention
    assert np.abs(D64[63] - g["D"][63])[ok[0]].max() < 3e-3


def test_rtume_vs_reference():
    g = load_golden("g4_rtume.npz")
    T, D = orc.batch_estimate_transform_ume_old(g["G"], g["H"])
    # rows 0..31 = physical twins (well-posed); 32..61 = deliberately mismatched pairs whose 3x3
    # cross-moment can be ill-conditioned (the SVD then amplifies LAPACK-vs-LAPACK noise);
    # 62..69 = reflection inputs.
    dR = np.abs(T[:, :3, :3] - g["T"][:, :3, :3]).max(axis=(1, 2))
    assert dR[:32].max() < 2e-6 and dR[62:].max() < 2e-6 and np.median(dR) < 2e-6 and dR.max() < 1e-3
    # translation noise floor of the fp32 reference itself
    dt = np.abs(T[:, :3, 3] - g["T"][:, :3, 3]).max(axis=1)
    assert dt[:32].max() < 1e-4 and dt[62:].max() < 1e-4 and np.median(dt) < 1e-4
    assert np.all(T[:, 3] == np.array([0, 0, 0, 1], np.float32))
    wc = well_conditioned(g["G"]) & well_conditioned(g["H"])
    assert wc.mean() > 0.8 and np.abs(D - g["D"])[wc].max() < 3e-3
    # first 32 are physical twins: recovers the ground-truth transform
    assert np.abs(T[:32] - g["gt_tform"]).max() < 2e-4
    # reflection inputs still give proper rotations (det fix, loc_utils.py:327-329)
    assert np.allclose(np.linalg.det(T[62:, :3, :3].astype(np.float64)), 1.0, atol=1e-5)


def test_ume_kp_layer_vs_reference():
    """a8: the oracle's restatement of `ume_kp_layer.forward` against the reference's own outputs (golden G11: diag_only on 64
    keypoints, the full n_kp x n_kp form on 8, the n_rand triplet form with the seeded host draw)."""
    g6, g = load_golden("g6_pair_k1.npz"), load_golden("g11_ume_kp_layer.npz")
    b = lambda a: a[None]    # noqa: E731
    kp_s, kp_t = g6["src_pts"][g6["src_inds"][:64]], g6["tgt_pts"][g6["tgt_inds"][:64]]
    args = (b(g6["src_pts"]), b(g6["src_feat"]), b(kp_s), b(g6["tgt_pts"]), b(g6["tgt_feat"]), b(kp_t))
    T, D, G, H = orc.ume_kp_layer_forward(*args, 750, 5.0, diag_only=True)
    assert T.shape == g["T_diag"].shape and D.shape == g["D_diag"].shape and G.shape == g["G_diag"].shape
    scale = np.abs(g["G_diag"]).max(axis=(1, 2), keepdims=True)
    assert (np.abs(G - g["G_diag"]) / scale).max() < 2e-4 and (np.abs(H - g["H_diag"]) / scale).max() < 2e-4
    assert np.abs(T[..., :3, :3] - g["T_diag"][..., :3, :3]).max() < 1e-4
    assert np.median(np.abs(T[..., :3, 3] - g["T_diag"][..., :3, 3])) < 1e-4
    wc = well_conditioned(g["G_diag"]) & well_conditioned(g["H_diag"])
    assert np.abs(D - g["D_diag"])[0][wc].max() < 3e-3
    sub = tuple(a[:, :8] if i in (2, 5) else a for i, a in enumerate(args))
    T2, D2, _, _ = orc.ume_kp_layer_forward(*sub, 750, 5.0, diag_only=False)
    assert T2.shape == g["T_full"].shape == (1, 8, 8, 4, 4) and D2.shape == (1, 8, 8)
    assert np.median(np.abs(T2 - g["T_full"])) < 1e-4
    np.random.seed(int(g["rand_seed"]))
    trip = np.random.choice(np.arange(64), (int(g["n_rand"]), 3))                 # utils/loc_utils.py:411
    T3, D3, _, _ = orc.ume_kp_layer_forward(*args, 750, 5.0, diag_only=True, triplets=trip)
    assert T3.shape == g["T_rand"].shape and np.median(np.abs(T3 - g["T_rand"])) < 1e-4


def test_rre_vs_reference():
    g = load_golden("g5_rre.npz")
    rre = orc.relative_rotation_error(g["R"], g["R_hat"])
    # acos amplifies 1-ulp trace differences near 0 and 180 deg
    assert np.abs(rre - g["rre"]).max() < 0.05
    assert np.abs(rre[2:8] - g["deg"][2:8]).max() < 2e-2


def test_pair_k1_whole_path():
    """Config 1 (BASELINE.json configs[0]): 4k-point pair, known SE(3), injected indices."""
    g = load_golden("g6_pair_k1.npz")
    out = orc.register_pair(g["src_pts"], g["tgt_pts"], g["src_feat"], g["tgt_feat"],
                            g["src_inds"], g["tgt_inds"], cond=g["cond"], accum="f32")
    assert (out["match"] == g["match"]).mean() >= 0.995
    same = out["match"] == g["match"]
    wc = well_conditioned(g["ume_src"]) & well_conditioned(g["ume_tgt"])[g["match"]]
    assert wc.mean() > 0.7
    assert np.abs(out["match_d"] - g["match_d"])[same & wc].max() < 3e-3
    prob = orc.match_prob(g["match_d"], 0.05)
    assert np.allclose(prob, g["prob"], rtol=1e-4, atol=1e-12)
    ok = same[g["cond"]]
    T, Tg = out["T"][ok], g["T"][ok]
    assert np.abs(T[:, :3, :3] - Tg[:, :3, :3]).max() < 1e-4
    dt = np.abs(T[:, :3, 3] - Tg[:, :3, 3])
    assert np.median(dt) < 1e-4 and dt.max() < 2e-3
    rre = orc.relative_rotation_error(T[:, :3, :3], np.broadcast_to(g["gt_tform"][:3, :3], T[:, :3, :3].shape))
    assert np.median(rre) < 0.1


def test_knn_points_matches_bruteforce():
    rng = np.random.RandomState(0)
    a = rng.standard_normal((1, 50, 3)).astype(np.float32)
    b = rng.standard_normal((1, 200, 3)).astype(np.float32)
    r = orc.knn_points(a, b, K=7)
    d2 = ((a[0][:, None, :].astype(np.float64) - b[0][None].astype(np.float64)) ** 2).sum(-1)
    ref = np.argsort(d2, axis=1, kind="stable")[:, :7]
    assert np.array_equal(r.idx[0], ref)
    assert np.all(np.diff(r.dists[0], axis=1) >= 0)


def test_feature_correlator_vs_reference():
    """utils/loc_utils.py:579-681 -- golden G7 produced by the reference's own FeatureCorrelator."""
    g = load_golden("g7_feature_corr.npz")
    fsv = orc.feature_spatial_var(g["src_pts"][None], g["src_feat"][None], knn=50)[0]
    assert np.abs(fsv - g["fsv_src"]).max() < 2e-6
    best, scores = orc.feature_corr_hypothesis_test(g["src_pts"][None], g["tgt_pts"][None], g["src_feat"][None],
                                                    g["tgt_feat"][None], g["T_hyp"], sigma=1.5, corr_num_nn=20,
                                                    n_hypotheses=10, batch=3)
    assert np.allclose(scores, g["score"], rtol=2e-5, atol=1e-6)
    assert np.array_equal(best, g["best_T"])
    assert int(np.argmax(scores)) == int(g["gt_index"])          # the ground-truth transform wins
    # the C loops bench.py's cpu_baseline leg uses for thousands of hypotheses: same scores, same selection
    best_c, scores_c = orc.feature_corr_hypothesis_test(g["src_pts"][None], g["tgt_pts"][None], g["src_feat"][None],
                                                        g["tgt_feat"][None], g["T_hyp"], sigma=1.5, corr_num_nn=20,
                                                        n_hypotheses=10, fast=True)
    assert np.allclose(scores_c, g["score"], rtol=2e-5, atol=1e-6) and np.array_equal(best_c, g["best_T"])


def test_icp_oracle_recovers_ground_truth():
    """f2 (parity unpinned, open3d not installable): the restated ICP loop must at least converge onto the
    transform that generated the data, stop by its own criterion and leave a perfect alignment untouched."""
    rng = np.random.RandomState(0)
    tgt = rng.uniform([-10, -10, -1], [10, 10, 1], (1500, 3)).astype(np.float32)
    ang = 0.1; R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]); t = np.array([1.0, -2.0, 0.1])
    src = ((tgt[:900].astype(np.float64) - t) @ R).astype(np.float32)
    gt = np.eye(4); gt[:3, :3] = R; gt[:3, 3] = t
    T0 = gt.copy(); T0[:3, 3] += [0.05, -0.04, 0.01]
    T, fit, rmse, it = orc.icp_point_to_point(src, tgt, T0, 0.2, 30)
    assert fit == 1.0 and rmse < 1e-5 and it < 30
    assert np.abs(T - gt).max() < 1e-5
    T2, fit2, _, it2 = orc.icp_point_to_point(src, tgt, gt, 0.2, 30)
    assert it2 == 1 and fit2 == 1.0 and np.abs(T2 - gt).max() < 1e-6
    Rr, tr = orc.umeyama_no_scaling(src[:50].astype(np.float64), tgt[:50].astype(np.float64))
    assert np.abs(Rr - R).max() < 1e-6 and np.abs(tr - t).max() < 1e-5 and abs(np.linalg.det(Rr) - 1) < 1e-12


def _g8_call(fn, g, tag, extra=None):
    kw = dict(nn_r=float(g[f"cfg_nn_r_{tag}"]), max_nn=int(g[f"cfg_max_nn_{tag}"]), min_nn=int(g[f"cfg_min_nn_{tag}"]),
              num_samples=int(g[f"cfg_num_samples_{tag}"]), normalized_ume=bool(g[f"cfg_normalized_ume_{tag}"]))
    return fn(g["src_pts"][None], g["src_seg"][None], g["src_feat"][None], g["tgt_pts"][None], g["tgt_feat"][None],
              g["gt_tform"][None], flat_labels=[9], nn_intersection_r=0.6, **kw)


def check_g8_outputs(out, g, tag, f_tol):
    F_velo, F_ref, velo_kp, ref_kp, ratio, with_kpts = out
    assert np.array_equal(velo_kp, g[f"velo_kp_{tag}"])                      # same keypoints, same (descending) order
    assert np.abs(ref_kp - g[f"ref_kp_{tag}"]).max() < 1e-5
    assert np.array_equal(ratio, g[f"ratio_{tag}"]) and np.array_equal(with_kpts, g[f"with_kpts_{tag}"])
    for F, key in ((F_velo, "F_velo"), (F_ref, "F_ref")):
        ref = g[f"{key}_{tag}"]
        scale = np.abs(ref).max(axis=(2, 3), keepdims=True) + 1e-30
        err = (np.abs(F - ref) / scale).max(axis=(2, 3))
        # the normaliser sum_c sum_n f (+1e-6) cancels heavily for zero-mean descriptors: a different fp32 summation
        # order moves such rows by up to ~1e-3 relative (the reference's own noise)
        assert np.median(err) < f_tol and err.max() < (2e-3 if bool(g[f"cfg_normalized_ume_{tag}"]) else 20 * f_tol)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_generate_ume_from_keypoints2_golden(tag):
    """f3: the restatement against the reference's own generate_ume_from_keypoints2 (G8)."""
    g = load_golden("g8_gt_ume_inlier.npz")
    check_g8_outputs(_g8_call(orc.generate_ume_from_keypoints2, g, tag), g, tag, 2e-5)


def test_calc_inliear_ratio_golden():
    g = load_golden("g8_gt_ume_inlier.npz")
    src = dict(pts=g["src_pts"][None], seg=g["src_seg"][None], feat=g["src_feat"][None])
    tgt = dict(pts=g["tgt_pts"][None], seg=None, feat=g["tgt_feat"][None])
    for tag, kw in dict(a=dict(ume_r_nn=5.0, ume_max_nn=64, ume_min_nn=10, eval_num_kpts=48),
                        b=dict(ume_r_nn=4.0, ume_max_nn=32, ume_min_nn=12, eval_num_kpts=30)).items():
        ir = orc.calc_inliear_ratio(src, tgt, g["gt_tform"][None], keypoints_ignore_segments=[9], **kw)
        # Hungarian on a noisy fp32 distance matrix: a couple of assignments may differ from the reference's
        assert abs(float(ir[0]) - float(g[f"inlier_ratio_{tag}"][0])) <= 2.5 / kw["eval_num_kpts"]


def test_hungarian_block_vs_reference():
    """evaluate.py:215-254 with hungarian_matching_flag (golden G9 = the reference's own statements executed): the oracle's
    pieces (ume_cdist, match_prob, the numpy draw, batch_estimate_transform_ume_old) chained the same way."""
    from scipy.optimize import linear_sum_assignment
    g = load_golden("g9_hungarian.npz")
    D = orc.ume_cdist(g["ume_src"][None], g["ume_tgt"][None])[0]
    src_m, tgt_m = linear_sum_assignment(D)
    # the assignment minimises a SUM over an fp32 matrix; numpy's and torch's cdist differ by fp32 rounding, which can
    # swap a few non-twin rows with near-equal costs: twins identical, total cost equal to 1e-3, >= 95 % of rows identical
    m = np.stack([src_m, tgt_m], 1)
    same = (m == g["m_all"]).all(axis=1)
    assert same[:48].all() and same.mean() >= 0.95 and np.array_equal(g["m_all"], g["m_filt"])
    assert abs(D[src_m, tgt_m].sum() - D[g["m_all"][:, 0], g["m_all"][:, 1]].sum()) < 1e-3 * D[src_m, tgt_m].sum()
    src_m, tgt_m = g["m_all"][:, 0], g["m_all"][:, 1]
    prob = orc.match_prob(D[src_m, tgt_m], float(g["tau"]))
    wcp = well_conditioned(g["ume_src"])[src_m] & well_conditioned(g["ume_tgt"])[tgt_m]
    assert np.allclose(prob[wcp], g["prob"][wcp], rtol=0.1, atol=1e-9)      # exp(d / 0.05) amplifies d noise 20x
    np.random.seed(int(g["seed"]))
    cond = np.random.choice(D.shape[0], int(g["ume_n_samples"]), replace=False, p=g["prob"])
    assert np.array_equal(cond, g["cond"])
    T, _ = orc.batch_estimate_transform_ume_old(g["ume_src"][src_m][cond], g["ume_tgt"][tgt_m][cond], with_dist=False)
    wc = well_conditioned(g["ume_src"])[src_m][cond] & well_conditioned(g["ume_tgt"])[tgt_m][cond]
    assert np.abs(T - g["T_filt"])[wc][:, :3, :3].max() < 1e-4


def test_full_pipeline_oracle_on_a_hard_pair():
    """bench.py's recall check uses oracle.evaluate_pair_full (evaluate.py:195-309 restated): it must register an easy
    pair exactly and be deterministic given the RNG seed; sparse_quantize keeps the first point of every voxel."""
    from umeregrobust_amd.synth import synth_pair, synth_pair_hard
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.7, 0.1, 0.1], [-0.1, 0.0, 0.0], [0.65, 0.0, 0.0]], np.float32)
    assert np.array_equal(orc.sparse_quantize(pts, 0.6), [0, 2, 3])
    p = synth_pair(2, N=1500, n_kp=256, voxel=0.6)
    kw = dict(ume_n_samples=64, pc_corr_max_size=1500)
    r = orc.evaluate_pair_full(p.src_pts, p.tgt_pts, p.src_feat, p.tgt_feat, p.gt_tform, np.random.RandomState(0), **kw)
    assert r["rre"] < 0.05 and r["rte"] < 0.01 and r["n_hyp"] == 64
    h = synth_pair_hard(2, N=1500, n_kp=256, voxel=0.6)
    assert h.src_pts.shape == (1500, 3) and 0.2 < (h.tgt_twin_of_src >= 0).mean() < 0.8
    tw = h.tgt_twin_of_src
    ok = tw >= 0
    e = (h.src_pts[ok].astype(np.float64) @ h.gt_tform[:3, :3].T.astype(np.float64) + h.gt_tform[:3, 3]) - h.tgt_pts[tw[ok]]
    assert 0.005 < np.abs(e).std() < 0.06                                 # two independent N(0, 2 cm) noises
    a = orc.evaluate_pair_full(h.src_pts, h.tgt_pts, h.src_feat, h.tgt_feat, h.gt_tform, np.random.RandomState(4), **kw)
    b = orc.evaluate_pair_full(h.src_pts, h.tgt_pts, h.src_feat, h.tgt_feat, h.gt_tform, np.random.RandomState(4), **kw)
    assert np.array_equal(a["T_est"], b["T_est"]) and np.isfinite(a["T_est"]).all()


def test_contracted_ball_query_variant_against_numpy():
    """oracle.ball_query(fma=True) -- the checker of the library's opt-in UMEREG_BALL_FMA mode (pytorch3d's CUDA kernel as nvcc
    contracts it: d2 = fma(dz, dz, fma(dy, dy, dx dx))) -- against an independent numpy evaluation of both predicates (fp64 products
    rounded once per fused step) on a cloud built to sit on the boundary, where the two forms select different neighbours."""
    rng = np.random.RandomState(12)
    r2 = np.float32(5.0) * np.float32(5.0)
    nq, per = 60, 300
    q = rng.uniform(-30, 30, (nq, 3)).astype(np.float32)
    dirs = rng.standard_normal((nq, per, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    shell = (q[:, None, :].astype(np.float64) + dirs * (5.0 + rng.uniform(-3e-6, 3e-6, (nq, per, 1)))).astype(np.float32).reshape(-1, 3)
    pts = np.concatenate([shell, rng.uniform(-40, 40, (5000, 3)).astype(np.float32)])
    pts = pts[rng.permutation(pts.shape[0])]
    d = q[:, None, :] - pts[None, :, :]
    un = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d64 = d.astype(np.float64)
    inner = (d64[..., 0] * d64[..., 0]).astype(np.float32).astype(np.float64)
    mid = (d64[..., 1] * d64[..., 1] + inner).astype(np.float32).astype(np.float64)
    co = (d64[..., 2] * d64[..., 2] + mid).astype(np.float32)
    assert int(((un < r2) != (co < r2)).sum()) >= 20
    K = 64
    for fma, pred in ((False, un < r2), (True, co < r2)):
        got = orc.ball_query(q[None], pts[None], K=K, radius=5.0, fma=fma)
        for i in range(nq):
            want = np.flatnonzero(pred[i])[:K]
            assert np.array_equal(got.idx[0, i][:want.size], want) and (got.idx[0, i][want.size:] == -1).all()
        hit = got.idx[0] >= 0
        assert np.array_equal(got.dists[0][hit], np.take_along_axis(co if fma else un, np.where(hit, got.idx[0], 0), 1)[hit])


def test_ume_match_f64_equals_the_matrix_reduced():
    """oracle.ume_match_f64 (per-row arg-min / two smallest D^2 / D at a given column, no n1 x n2 matrix) against
    ume_cdist_f64(...).argmin / sort on small inputs, exact ties included (duplicated targets, a zero UME, one target)."""
    rng = np.random.RandomState(4)
    u1 = rng.standard_normal((57, 32, 4)).astype(np.float32)
    u2 = rng.standard_normal((90, 32, 4)).astype(np.float32)
    u2[:20] = u1[:20] @ (np.eye(4) + 0.1 * rng.standard_normal((4, 4))).astype(np.float32)
    u2[40:43] = u2[3]                      # exact ties: row 3's best target exists four times -> the lowest index, d2sec == d2min
    u2[60] = u2[61] = u2[62] = u1[30]      # and three copies of row 30 itself (D = 0)
    u1[50] = 0.0                           # zero UME: Q = I[:, :4]
    for a, b in ((u1, u2), (u1[:7], u2[:1]), (u1[:1], u2)):
        D = orc.ume_cdist_f64(a, b)
        cols = rng.randint(0, b.shape[0], a.shape[0])
        r = orc.ume_match_f64(a, b, cols=cols)
        assert np.array_equal(r.argmin, D.argmin(axis=1))
        s = np.sort(D ** 2, axis=1)
        assert np.array_equal(np.sqrt(r.d2min), D.min(axis=1))                 # the same statements, bit for bit
        assert np.allclose(r.d2min, s[:, 0], rtol=0, atol=1e-15)
        if b.shape[0] > 1:
            assert np.allclose(r.d2sec, s[:, 1], rtol=0, atol=1e-15)
        else:
            assert np.isinf(r.d2sec).all()
        assert np.array_equal(r.d_at, D[np.arange(a.shape[0]), cols])
        assert orc.ume_match_f64(a, b).d_at is None
    r = orc.ume_match_f64(u1, u2)
    assert r.argmin[3] == 3 and r.d2sec[3] == r.d2min[3]                         # (row 3 -> target 3, tied with 40..42)
    assert r.argmin[30] == 60 and r.d2min[30] == 0.0 and r.d2sec[30] == 0.0


def test_rtume_f64_against_its_fp32_sibling_and_its_conditioning_figures():
    """oracle.batch_estimate_transform_ume_f64 (utils/loc_utils.py:292-350 in fp64, with the row gathers) on golden G4:
    on the well-posed rows (0..31 physical twins, 62..69 reflections) it agrees with the fp32 restatement
    (batch_estimate_transform_ume_old) to the bar that pins that one to the reference; the conditioning figures flag the
    deliberately mismatched rows 32..61, and bound the fp32 sibling's deviation on every row (kappa * 2^-24)."""
    g = load_golden("g4_rtume.npz")
    T64, c = orc.batch_estimate_transform_ume_f64(g["G"], g["H"])
    T32, _ = orc.batch_estimate_transform_ume_old(g["G"], g["H"], with_dist=False)
    dR = np.abs(T32[:, :3, :3] - T64[:, :3, :3]).max(axis=(1, 2))
    dt = np.abs(T32[:, :3, 3] - T64[:, :3, 3]).max(axis=1)
    well = np.r_[0:32, 62:70]
    assert dR[well].max() < 2e-6 and dt[well].max() < 1e-4
    assert np.abs(T64[:32] - g["gt_tform"]).max() < 2e-4
    assert np.allclose(np.linalg.det(T64[:, :3, :3]), 1.0, atol=1e-12) and np.all(T64[:, 3] == [0, 0, 0, 1])
    # figures: a true match has mg ~ mh (cosine 1); the mismatched rows do not, and their cross-moments are worse conditioned
    assert c.cos_mg_mh[well].min() > 0.999 and c.cos_mg_mh[32:62].max() < 0.5
    assert np.median(c.kappa_R[32:62]) > np.median(c.kappa_R[well]) and c.kappa_R.argmax() in range(32, 62)
    assert c.s.shape == (70, 3) and np.all(np.diff(c.s, axis=1) <= 0) and np.allclose(c.s3_s1, c.s[:, 2] / c.s[:, 0])
    u32 = 2.0 ** -24
    assert np.all(dR <= u32 * c.kappa_R) and np.all(dt <= u32 * c.kappa_t)
    # gathers: hypothesis k = (G[gi[k]], H[hi[k]])
    gi, hi = np.array([5, 0, 69, 33]), np.array([5, 0, 69, 34])
    Tg, cg = orc.batch_estimate_transform_ume_f64(g["G"], g["H"], gi, hi)
    Tx, _ = orc.batch_estimate_transform_ume_f64(g["G"][gi], g["H"][hi])
    assert np.array_equal(Tg, Tx) and np.array_equal(Tg[:3], T64[[5, 0, 69]]) and cg.kappa_R.shape == (4,)
    # a zero cross-moment (rank 0) is degenerate in every figure and still gives a finite transform
    Z = np.zeros((1, 32, 4), np.float32)
    Tz, cz = orc.batch_estimate_transform_ume_f64(Z, Z)
    assert np.isfinite(Tz).all() and np.isinf(cz.kappa_R).all() and cz.cos_mg_mh[0] == 0.0


# ---- f1 judged per neighbour (orc_corr_images_f32 / orc_corr_judge_f32) -------------------------------------------------------
def _round_f32(x):
    """A Fraction rounded to the nearest fp32 (ties to even), as a Fraction: the exact-rational model of one IEEE fp32 operation."""
    from fractions import Fraction
    if x == 0:
        return Fraction(0)
    v = float(x)                                      # nearest double (correctly rounded by Fraction.__float__)
    f = np.float32(v)                                 # may round twice: decide by hand around it
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = None
    for c in cands:
        if not np.isfinite(c):
            continue
        e = abs(Fraction(float(c)) - x)
        if best is None or e < best[0] or (e == best[0] and (int(np.float32(c).view(np.uint32)) & 1) == 0):
            best = (e, c)
    return Fraction(float(best[1]))


def _fmaf_exact(a, b, c):
    from fractions import Fraction
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _image_exact(T, p, form):
    from fractions import Fraction
    F = lambda v: Fraction(float(v))
    out = []
    for a in range(3):
        if form == orc.CORR_FORM_FMA:
            v = _round_f32(F(T[a, 0]) * F(p[0]))
            v = _round_f32(F(T[a, 1]) * F(p[1]) + v)
            v = _round_f32(F(T[a, 2]) * F(p[2]) + v)
        else:
            v = _round_f32(F(T[a, 0]) * F(p[0]))
            v = _round_f32(v + _round_f32(F(T[a, 1]) * F(p[1])))
            v = _round_f32(v + _round_f32(F(T[a, 2]) * F(p[2])))
        out.append(np.float32(float(_round_f32(v + F(T[a, 3])))))
    return np.array(out, np.float32)


def test_corr_images_fma_form_is_correctly_rounded():
    """The FMA form (the HIP routes' q = fmaf(T2, z, fmaf(T1, y, T0 x)) + T3) equals an exact-rational emulation of fmaf on 4 096
    triples, ~half of them built so that an fp64 emulation (a*b + c in double, then to fp32) rounds twice and misses: a = b = 1 + m 2^-12
    (m odd) puts a*b exactly on an fp32 midpoint and a tiny c of either sign decides the side."""
    rng = np.random.RandomState(3)
    M, Ns = 64, 64
    T = np.zeros((M, 4, 4), np.float32)
    sp = np.ones((Ns, 3), np.float32)
    m = (2 * rng.randint(1, 1 << 10, Ns) + 1).astype(np.float64)
    half = Ns // 2
    sp[:half, 1] = (1.0 + m[:half] * 2.0 ** -12).astype(np.float32)                          # b: midpoint family
    sp[half:, 1] = (rng.standard_normal(Ns - half) * 10.0 ** rng.uniform(-3, 3, Ns - half)).astype(np.float32)
    for h in range(M):
        if h < M // 2:
            T[h, 0, 1] = sp[h % half, 1] * np.float32(2.0 ** rng.randint(-3, 4))                # a: the same family, a power of two apart
            T[h, 0, 0] = np.float32((-1) ** h * 2.0 ** -rng.randint(40, 60))                  # c: far below the midpoint bit
        else:
            T[h, 0, :2] = (rng.standard_normal(2) * 10.0 ** rng.uniform(-3, 3, 2)).astype(np.float32)
    q = orc.corr_images(T, sp, orc.CORR_FORM_FMA)
    n_double = 0
    for h in range(M):
        for n in range(Ns):
            a, b, c = T[h, 0, 1], sp[n, 1], T[h, 0, 0]
            want = np.float32(float(_fmaf_exact(a, b, c)))
            assert q[h, n, 0] == want, (h, n, a, b, c, q[h, n, 0], want)
            n_double += int(np.float32(float(a) * float(b) + float(c)) != want)
    assert n_double >= 100, n_double                   # the fp64 emulation would have failed here
    # the whole chain, all three rows, random transforms and points, both forms
    T = rng.standard_normal((24, 4, 4)).astype(np.float32) * np.float32(3)
    sp = (rng.standard_normal((40, 3)) * 50).astype(np.float32)
    for form in (orc.CORR_FORM_REF, orc.CORR_FORM_FMA):
        q = orc.corr_images(T, sp, form)
        for h in range(T.shape[0]):
            for n in range(sp.shape[0]):
                assert np.array_equal(q[h, n], _image_exact(T[h], sp[n], form)), (form, h, n)


def _numpy_neighbours(q, tp, K):
    """K smallest (fp32 d2 = ((dx*dx) + (dy*dy)) + (dz*dz), index), ascending -- numpy, one rounding per operation."""
    d = q[:, None, :] - tp[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.lexsort((np.broadcast_to(np.arange(tp.shape[0]), d2.shape), d2), axis=-1)[:, :K]
    return order, np.take_along_axis(d2, order, axis=1)


def _int_features(rng, Ns, Nt, K, d=32):
    L = (2 ** 24 - 1) // (K * Ns)
    vp = np.zeros((Ns, d), np.float32)
    vp[np.arange(Ns), np.arange(Ns) % d] = rng.choice([-1.0, 1.0], Ns)
    vq = rng.randint(-L, L + 1, (Nt, d)).astype(np.float32)
    return vp, vq, L


def test_corr_judge_neighbour_sets_labels_and_scores():
    """orc_corr_judge_f32 in both forms: neighbour sets equal a numpy brute force on the same form's images; the reference form's sets
    are orc_pc_corr_cost_f32's (with unit weights and integer features both scores are exact: equal to the label / Ns); the labels equal
    a numpy recomputation from the returned sets; the fp64 score and absum equal a numpy fp64 restatement on real features."""
    rng = np.random.RandomState(8)
    Ns, Nt, K, M = 300, 700, 20, 12
    tp = (rng.uniform(-10, 10, (Nt, 3)) * [1, 1, 0.2]).astype(np.float32)
    sp = (tp[rng.randint(0, Nt, Ns)] + rng.standard_normal((Ns, 3)) * 0.3).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (M, 1, 1))
    for h in range(1, M):
        th = rng.uniform(-0.3, 0.3)
        T[h, :2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        T[h, :3, 3] = rng.standard_normal(3) * rng.choice([0.1, 3.0])
    vp, vq, L = _int_features(rng, Ns, Nt, K)
    assert L == (2 ** 24 - 1) // (K * Ns)
    sets = {}
    for form in (orc.CORR_FORM_REF, orc.CORR_FORM_FMA):
        j = orc.corr_judge(T, sp, tp, K, vp, vq, 2.0 ** 22, form=form, neighbours=True)
        q = orc.corr_images(T, sp, form)
        for h in range(M):
            idx, d2 = _numpy_neighbours(q[h], tp, K)
            assert np.array_equal(j.idx[h], idx) and np.array_equal(j.d2[h], d2), (form, h)
            lab = (vp[:, None, :] * vq[idx]).sum(-1, dtype=np.float64).sum()
            assert j.label[h] == lab == np.rint(lab), (form, h)
        sets[form] = j
    # the two forms differ on some images (by an ulp), and can differ on the sets
    assert not np.array_equal(orc.corr_images(T, sp, 0), orc.corr_images(T, sp, 1))
    ref = orc.pc_corr_cost_c(T, sp, tp, K, vp, vq, 2.0 ** 22)
    assert np.array_equal(ref, (sets[orc.CORR_FORM_REF].label / Ns).astype(np.float32))
    assert np.all(np.abs(sets[orc.CORR_FORM_REF].score * Ns - sets[orc.CORR_FORM_REF].label) <= 1e-9 * sets[orc.CORR_FORM_REF].absum)
    # real features and sigma: the fp64 score / absum on the same sets
    vp = rng.standard_normal((Ns, 32)).astype(np.float32); vq = rng.standard_normal((Nt, 32)).astype(np.float32)
    sigma = 0.7
    j = orc.corr_judge(T, sp, tp, K, vp, vq, sigma, neighbours=True)
    assert np.array_equal(j.idx, sets[orc.CORR_FORM_FMA].idx)
    for h in range(M):
        w = 1.0 / (1.0 + j.d2[h].astype(np.float64) / sigma ** 2)
        t = vp.astype(np.float64)[:, None, :] * vq.astype(np.float64)[j.idx[h]]
        assert abs(j.score[h] - (w * t.sum(-1)).sum() / Ns) <= 1e-12 * np.abs(w * t.sum(-1)).sum() / Ns
        assert abs(j.absum[h] - (w * np.abs(t).sum(-1)).sum()) <= 1e-12 * j.absum[h]
    ref = orc.pc_corr_cost(T[:, :3, :3], T[:, :3, 3], sp, tp, K, vp, vq, sigma)
    assert np.all(np.abs(ref - j.score) <= 1e-5 * j.absum / Ns)


def test_corr_judge_lattice_ties_go_to_the_lower_index():
    """A target on an integer lattice (shuffled, with duplicated points) and queries on lattice points, cell centres and edge midpoints:
    distance ties by the dozen at the K-th place.  The sets equal the numpy (d2, index) order: every tie goes to the lower index."""
    rng = np.random.RandomState(4)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    tp = np.concatenate([g, g[rng.randint(0, len(g), 40)]])[rng.permutation(len(g) + 40)]
    sp = np.concatenate([g[rng.randint(0, len(g), 60)], g[rng.randint(0, len(g), 60)] + 0.5,
                         g[rng.randint(0, len(g), 60)] + [0.5, 0, 0]]).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    T[1, :3, 3] = [1.0, -2.0, 0.0]
    vp, vq, _ = _int_features(rng, sp.shape[0], tp.shape[0], 20)
    n_ties = 0
    for K in (1, 6, 20):
        j = orc.corr_judge(T, sp, tp, K, vp, vq, 2.0 ** 22, neighbours=True)
        for h in range(2):
            q = orc.corr_images(T[h:h + 1], sp)[0]
            idx, d2 = _numpy_neighbours(q, tp, K)
            assert np.array_equal(j.idx[h], idx) and np.array_equal(j.d2[h], d2), (K, h)
            d = q[:, None, :] - tp[None]
            full = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            n_ties += int((full == d2[:, -1:]).sum(1).__gt__((d2 == d2[:, -1:]).sum(1)).sum())
    assert n_ties > 100, n_ties                        # K-boundary ties were there to break


# ---- the "f16r" refine restated on split-f16 planes (oracle.decode_split_f16 / orc_match_split_f64) ------------------------
def split_planes(Q):
    """hi = f16(q), lo = f16(q - hi) of an fp64 basis, as the library's orthobasis kernel splits it."""
    Q = np.asarray(Q, np.float64)
    hi = Q.astype(np.float16)
    return hi, (Q - hi.astype(np.float64)).astype(np.float16)


def _crowd_bases(rng, n1, n2, crowd=40, tiny=False):
    """fp64 bases: n2 targets, the first n1 // 2 sources each with a crowd of `crowd` near-duplicate targets (eps 1e-7 .. 1e-3)."""
    def orth(u):
        return np.linalg.qr(u)[0]
    u1 = rng.standard_normal((n1, 32, 4))
    u2 = rng.standard_normal((n2, 32, 4))
    if tiny:                                          # many near-zero channels: lo (and some hi) in the f16 subnormal range
        u1[:, 4:] *= 10.0 ** rng.uniform(-6, -3, (n1, 28, 1))
        u2[:, 4:] *= 10.0 ** rng.uniform(-6, -3, (n2, 28, 1))
    for r in range(min(n1 // 2, n2 // crowd)):
        s = r * crowd
        eps = 10.0 ** rng.uniform(-7, -3, crowd)
        u2[s:s + crowd] = u1[r] * (1.0 + eps[:, None, None] * rng.standard_normal((crowd, 32, 4)))
    return orth(u1), orth(u2)


def _split_brute_force(A, B):
    """D2 = 4 - |Qa^T Qb|_F^2 of the split bases in numpy's own order (float64(hi) + float64(lo)), and the hi-only coarse score."""
    qa = A[0].astype(np.float64) + A[1].astype(np.float64)
    qb = B[0].astype(np.float64) + B[1].astype(np.float64)
    C = np.einsum("ika,jkb->ijab", qa, qb)
    D2 = np.maximum(4.0 - (C * C).sum(axis=(2, 3)), 0.0)
    Ch = np.einsum("ika,jkb->ijab", A[0].astype(np.float64), B[0].astype(np.float64))
    return D2, (Ch * Ch).sum(axis=(2, 3))


def _fma_exact(a, b, c):
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))    # one rounding (Fraction.__float__ is exact-rounded)


def test_split_f16_layout_decoder_round_trips():
    """decode_split_f16 inverts encode_split_f16 bit for bit (subnormals, signed zeros), the index map is injective and in range,
    padding stays zero, and a few offsets equal qlayout.h's formulas evaluated by hand."""
    rng = np.random.RandomState(0)
    for layout in (orc.QLAYOUT_ROWS_F16X2, orc.QLAYOUT_COLS_F16X2):
        for n in (1, 7, 33, 129, 300):
            hi = rng.standard_normal((n, 32, 4)).astype(np.float16)
            lo = (rng.standard_normal((n, 32, 4)) * 2.0 ** rng.randint(-26, -10, (n, 32, 4))).astype(np.float16)
            lo[0, 0, 0], hi[-1, 31, 3] = np.float16(-0.0), np.float16(2.0 ** -24)
            buf = orc.encode_split_f16(hi, lo, layout)
            assert buf.size == orc.split_f16_halfs(n, layout)
            h2, l2 = orc.decode_split_f16(buf, n, layout)
            assert np.array_equal(h2.view(np.uint16), hi.view(np.uint16)) and np.array_equal(l2.view(np.uint16), lo.view(np.uint16))
            off = orc.split_f16_offsets(n, layout).reshape(-1)
            assert np.unique(off).size == off.size and off.min() >= 0 and off.max() < buf.size
            pad = np.ones(buf.size, bool); pad[off] = False
            assert not buf.view(np.uint16)[pad].any()
            # the decoder reads any dtype viewing the same bytes (the library's buffers come back as float32)
            assert np.array_equal(orc.decode_split_f16(buf.view(np.float32), n, layout)[1].view(np.uint16), lo.view(np.uint16))
    # hoff_rows(i = 9, a = 2, k = 21, plane = 1): s = 1, h = 0, e = 5 -> ((((1*2+1)*2+1)*64 + 0 + 1*4 + 2)*8 + 5
    assert orc.split_f16_offsets(10, orc.QLAYOUT_ROWS_F16X2)[9, 21, 2, 1] == 3637
    # hoff_cols(j = 37, b = 3, k = 10, plane = 0): s = 0, h = 1, e = 2 -> (((((1*4+3)*2+0)*2+0)*64 + 32 + 5)*8 + 2
    assert orc.split_f16_offsets(40, orc.QLAYOUT_COLS_F16X2)[37, 10, 3, 0] == 14634
    assert orc.split_f16_halfs(1, orc.QLAYOUT_ROWS_F16X2) == 128 * 256 and orc.split_f16_halfs(33, orc.QLAYOUT_COLS_F16X2) == 64 * 256


def test_match_split_f64_restates_the_refine_term_for_term():
    """The oracle's key is the refine kernel's, bit for bit: its fma chain in the kernel's order, evaluated in exact rationals with
    one rounding per fma, then (float)max(4 - s, 0) -- on crowd pairs whose D^2 lives in the last bits of 4 - s."""
    rng = np.random.RandomState(1)
    A, B = (split_planes(Q) for Q in _crowd_bases(rng, 6, 40, crowd=12))
    r = orc.match_split_f64(A, B)
    qa = A[0].astype(np.float64) + A[1].astype(np.float64)
    vb = (B[0].astype(np.float32) + B[1].astype(np.float32)).astype(np.float64)
    for i in range(3):
        keys = []
        for j in range(B[0].shape[0]):
            dot = np.zeros((4, 4))
            for k in range(32):
                for a in range(4):
                    for b in range(4):
                        dot[a, b] = _fma_exact(qa[i, k, a], vb[j, k, b], dot[a, b])
            s = 0.0
            for a in range(4):
                for b in range(4):
                    s = _fma_exact(dot[a, b], dot[a, b], s)
            keys.append((np.float32(max(4.0 - s, 0.0)), j))
        best = min(keys, key=lambda t: (t[0], t[1]))
        assert r.argmin[i] == best[1] and r.key[i].view(np.uint32) == best[0].view(np.uint32), (i, r.argmin[i], r.key[i], best)
        second = min((t for t in keys if t[1] != best[1]), key=lambda t: (t[0], t[1]))
        assert r.arg2[i] == second[1] and r.key2[i] == second[0]
    assert (r.key[:3] < 1e-7).all()                   # the crowd rows' winners are near-duplicates (key 0: s rounded to >= 4)


@pytest.mark.parametrize("tiny", [False, True])
def test_match_split_f64_equals_brute_force_on_the_summed_planes(tiny):
    """orc_match_split_f64 against numpy's brute force on float64(hi) + float64(lo), which sums in another order: every row whose
    best two fp64 D^2 cannot swap their fp32 keys within 2 SPLIT_EVAL_ERR has the same arg-min; any other row picks a target within
    4 SPLIT_EVAL_ERR of numpy's minimum.  Keys, runner-ups and coarse hi-only scores agree to the same bound.  tiny: bases with many
    near-zero entries, whose lo planes are mostly f16 subnormals -- they must survive (flushing them changes the answer)."""
    rng = np.random.RandomState(7 if tiny else 3)
    A, B = (split_planes(Q) for Q in _crowd_bases(rng, 120, 900, crowd=30, tiny=tiny))
    r = orc.match_split_f64(A, B)
    D2, Ch = _split_brute_force(A, B)
    n1 = D2.shape[0]
    rows = np.arange(n1)
    e2 = 2 * orc.SPLIT_EVAL_ERR
    srt = np.sort(D2, axis=1)
    decided = np.float32(srt[:, 1] - e2) > np.float32(srt[:, 0] + e2)
    assert np.array_equal(r.argmin[decided], D2.argmin(axis=1)[decided])
    assert (D2[rows, r.argmin] - srt[:, 0]).max() <= 2 * e2
    assert np.abs(r.d64 - D2[rows, r.argmin]).max() <= e2 and np.abs(r.d64sec - srt[:, 1]).max() <= 2 * e2
    assert np.abs(r.key.astype(np.float64) - r.d64).max() <= np.spacing(r.key).max()
    assert np.all(r.key <= r.key2) and np.all((r.key < r.key2) | (r.argmin < r.arg2))
    assert np.abs(r.coarse_max - Ch.max(axis=1)).max() <= 1e-12 and np.abs(r.coarse_win - Ch[rows, r.argmin]).max() <= 1e-12
    crowd = rows < min(n1 // 2, B[0].shape[0] // 30)
    assert (r.key[crowd] < 1e-5).all()
    # rows a reference summing in another order cannot decide: D^2 below the evaluation error (eps ~1e-7); these are the rows only
    # a term-for-term restatement can judge
    assert (~decided[crowd]).sum() >= 3 and decided.mean() > 0.7, (decided[crowd].mean(), decided.mean())
    # the point of the split check: inside a crowd the coarse order is not the exact order
    inv = (r.coarse_max - r.coarse_win > 1e-4) & crowd
    assert inv.sum() >= 20, inv.sum()
    sub = (A[1] != 0) & (np.abs(A[1].astype(np.float32)) < 2.0 ** -14)
    assert sub.mean() > 0.1, sub.mean()
    if tiny:                                          # near-zero entries: hi itself is subnormal in places
        assert ((A[0] != 0) & (np.abs(A[0].astype(np.float32)) < 2.0 ** -14)).sum() > 1000
    flushed = (A[0], np.where(sub, np.float16(0), A[1]))
    rf = orc.match_split_f64(flushed, B, coarse=False)
    assert (rf.key != r.key).sum() >= n1 // 4 and (rf.argmin != r.argmin).any(), ((rf.key != r.key).sum(), (rf.argmin != r.argmin).sum())
    print(f"[split oracle tiny={tiny}] decided {int(decided.sum())}/{n1}, inversions {int(inv.sum())}, subnormal lo {sub.mean():.2f}")
