"""GPU: `selection="device"` of generate_ume_from_keypoints2 (umeregrobust_amd/gt_keypoints.py, csrc/gt_keypoints.hip) against the
default path -- all six outputs `torch.equal` -- on the G8 golden inputs, the three-element batch of the parity suite and the edge
clouds of tests/gt_keypoints_cases.py, where the candidate list, the selected indices and the record are also judged by the numpy
restatement (pinned to the oracle in tests/test_gt_keypoints_cpu.py); `ball_any` against `ops.ball_query(K=1)`; every new entry
twice between guard bands over differently filled workspaces; and the keyword through the loss, the inlier ratio and one epoch of
the training driver.  No test looks at how many candidates were tested: that number depends on timing by design."""
import os

import numpy as np
import pytest
import torch

import gt_keypoints_cases as gc
from tests.conftest import load_golden
from test_abi_guard import Guard

pytestmark = pytest.mark.gpu

CASES = gc.all_cases()


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def both(args, kw):
    from umeregrobust_amd.utils.loc_utils import generate_ume_from_keypoints2
    return [generate_ume_from_keypoints2(*args, selection=s, **kw) for s in ("torch", "device")]


def assert_equal_outputs(a, b):
    names = ("F_velo", "F_ref", "velo_keypoint_pts", "ref_keypoint_pts", "ratio", "with_kpts")
    assert len(a) == len(b) == 6
    for name, x, y in zip(names, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, name
        assert x.is_contiguous() == y.is_contiguous(), name
        assert torch.equal(x, y), f"{name} differs between the two selections"


# ---- 1. the generator: real inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_the_six_outputs_are_equal_on_the_golden_inputs(gpu, tag, normalized):
    g = load_golden("g8_gt_ume_inlier.npz")
    kw = dict(nn_r=float(g[f"cfg_nn_r_{tag}"]), max_nn=int(g[f"cfg_max_nn_{tag}"]), min_nn=int(g[f"cfg_min_nn_{tag}"]),
              num_samples=int(g[f"cfg_num_samples_{tag}"]), normalized_ume=normalized, flat_labels=[9], nn_intersection_r=0.6)
    args = [T_(g[k][None], gpu) for k in ("src_pts", "src_seg", "src_feat", "tgt_pts", "tgt_feat", "gt_tform")]
    a, b = both(args, kw)
    assert_equal_outputs(a, b)
    assert np.array_equal(b[2].cpu().numpy(), g[f"velo_kp_{tag}"])          # and they are the reference's keypoints


def batch_of_three(gpu):
    """the batch of test_generate_ume_from_keypoints2_batch_vs_oracle: different candidate counts, the third element dropped"""
    from umeregrobust_amd.synth import synth_pair
    rng = np.random.RandomState(4)
    ps = [synth_pair(31 + i, N=2500, n_kp=16) for i in range(3)]
    src = np.stack([p.src_pts for p in ps]); tgt = np.stack([p.tgt_pts for p in ps])
    sf = np.stack([p.src_feat for p in ps]); tf = np.stack([p.tgt_feat for p in ps]); gt = np.stack([p.gt_tform for p in ps])
    seg = rng.choice([1, 9], size=(3, 2500, 1), p=[0.7, 0.3]).astype(np.int64)
    src[2] = src[2] * np.float32(6.0); tgt[2] = (src[2] @ gt[2, :3, :3].T + gt[2, :3, 3]).astype(np.float32)
    return [T_(x, gpu) for x in (src, seg, sf, tgt, tf, gt)]


@pytest.mark.parametrize("normalized", [False, True])
def test_the_six_outputs_are_equal_on_the_batch_with_a_dropped_element(gpu, normalized):
    args = batch_of_three(gpu)
    kw = dict(nn_r=5.0, max_nn=48, min_nn=12, num_samples=40, flat_labels=[9], normalized_ume=normalized, nn_intersection_r=0.6)
    a, b = both(args, kw)
    assert_equal_outputs(a, b)
    assert b[5].tolist() == [True, True, False] and b[0].shape[0] == 2


# ---- 2. the edge clouds ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_edge_clouds_against_the_default_path_and_the_restatement(gpu, case):
    from umeregrobust_amd import gt_keypoints as gk, ops
    from umeregrobust_amd.utils.loc_utils import generate_ume_from_keypoints2
    want = gc.select_ref(case)
    src, seg, sf, tgt, tf, gt = gc.inputs(case)
    args = [T_(x, gpu) for x in (src, seg, sf, tgt, tf, gt)]
    kw = case.kw
    # the entries themselves
    moved = args[0] @ args[5][:, :3, :3].transpose(-1, -2) + args[5][:, :3, 3][:, None]
    overlap = ops.ball_query(moved.contiguous(), args[3], K=1, radius=kw["nn_intersection_r"], return_nn=False).idx[..., 0]
    non_flat = (args[1] != torch.tensor(kw["flat_labels"], device=gpu)).all(dim=-1).flatten(1)
    cand, lengths = gk.candidates(overlap, non_flat)
    assert np.array_equal(cand.cpu().numpy(), want.cand) and np.array_equal(lengths.cpu().numpy(), want.lengths)
    kp_index, record = gk.select(args[0], cand, lengths, kw["nn_r"], kw["max_nn"], kw["min_nn"], kw["num_samples"])
    assert np.array_equal(record.cpu().numpy(), want.record)
    assert np.array_equal(kp_index.cpu().numpy(), want.kp_index)
    # the generator
    if case.error:
        text = {"no_candidate": gk.NO_CANDIDATE, "no_keypoint": gk.NO_KEYPOINT}[case.error]
        for s in ("torch", "device"):
            with pytest.raises(RuntimeError) as e:
                generate_ume_from_keypoints2(*args, selection=s, **kw)
            assert str(e.value) == text, s
        return
    for normalized in (False, True):
        a, b = both(args, dict(kw, normalized_ume=normalized))
        assert_equal_outputs(a, b)
    keep = np.where(want.with_kpts)[0]
    assert b[5].cpu().numpy().tolist() == want.with_kpts.tolist()
    assert np.array_equal(b[2].cpu().numpy(), np.stack([src[e][want.kp_index[e, :want.num_out]] for e in keep]))


def test_max_nn_above_the_limit_is_the_same_error(gpu):
    from umeregrobust_amd.utils.loc_utils import generate_ume_from_keypoints2
    case = next(c for c in CASES if c.name == "one_candidate")
    args = [T_(x, gpu) for x in gc.inputs(case)]
    texts = []
    for s in ("torch", "device"):
        with pytest.raises(RuntimeError) as e:
            generate_ume_from_keypoints2(*args, selection=s, **dict(case.kw, max_nn=7681))
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "7680" in texts[0]


# ---- 3. ball_any ----------------------------------------------------------------------------------------------------------------------

def by_ball_query(q, p, radius):
    from umeregrobust_amd import ops
    return (ops.ball_query(q, p, K=1, radius=radius, return_nn=False).idx > -1).sum(dim=(1, 2)).to(torch.int32)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 255, 256, 257, 750, 4095, 4096, 4097])
@pytest.mark.parametrize("Bk", [1, 300])
def test_ball_any_counts_what_a_k1_ball_query_finds(gpu, Bk, K):
    from umeregrobust_amd import gt_keypoints as gk, ops
    if K > 1000:
        Bk = min(Bk, 3)                       # (the tile edge: a few pairs are enough)
    q, p = gc.ball_any_inputs(Bk, K, 5)       # padded origin rows in p, t-valued rows in q
    q, p = T_(q, gpu), T_(p, gpu)
    hits = gk.ball_any(q, p, gc.INTERSECTION_R)
    assert hits.dtype == torch.int32 and hits.shape == (Bk,)
    want = by_ball_query(q, p, gc.INTERSECTION_R)
    assert torch.equal(hits, want)
    if K >= 63:
        assert 0 < int(hits.sum()) < Bk * K   # (neither everything nor nothing: the inputs exercise both answers)
    want_fma = (ops.ball_query(q, p, K=1, radius=gc.INTERSECTION_R, return_nn=False, fma=True).idx > -1).sum(dim=(1, 2)).to(torch.int32)
    assert torch.equal(gk.ball_any(q, p, gc.INTERSECTION_R, fma=True), want_fma)


def test_ball_any_refuses_more_rows_than_the_ball_search(gpu):
    from umeregrobust_amd import gt_keypoints as gk
    z = torch.zeros(1, gk.BALL_ANY_MAX_K + 1, 3, device=gpu)
    with pytest.raises(ValueError, match="7680"):
        gk.ball_any(z, z, 0.6)
    q, p = gc.ball_any_inputs(1, gk.BALL_ANY_MAX_K, 6)
    q, p = T_(q, gpu), T_(p, gpu)
    assert torch.equal(gk.ball_any(q, p, gc.INTERSECTION_R), by_ball_query(q, p, gc.INTERSECTION_R))     # the limit itself is served


@pytest.mark.parametrize("K", [64, 750])
def test_ball_any_is_strict_at_exactly_the_radius(gpu, K):
    from umeregrobust_amd import gt_keypoints as gk
    for inside in (False, True):
        q, p, radius = gc.lattice_345(K, inside)
        q, p = T_(q, gpu), T_(p, gpu)
        hits = gk.ball_any(q, p, radius)
        assert hits.tolist() == [K if inside else 0] == by_ball_query(q, p, radius).tolist()


# ---- 4. determinism and bounds --------------------------------------------------------------------------------------------------------

def guarded_entries(G):
    """every new entry at a ragged shape, each buffer at exactly its stated size between canaries; -> the specified output bytes"""
    from umeregrobust_amd import gt_keypoints as gk
    lib = gk.load_native()
    case = next(c for c in CASES if c.name == "stop_at_513")
    src, seg, _, _, _, _ = gc.inputs(case)
    B, N = src.shape[:2]
    rng = np.random.RandomState(3)
    overlap = np.where(rng.uniform(size=(B, N)) < 0.9, rng.randint(0, N, (B, N)), -1).astype(np.int64)
    a_ov, _ = G.inp(overlap)
    a_nf, _ = G.inp((seg[..., 0] != gc.FLAT).astype(np.uint8))
    a_pts, _ = G.inp(src)
    need = lib.umereg_gt_keypoints_workspace_bytes(B, N)
    a_ws, n_ws = G.ws(need)
    a_cand, cand = G.out((B, N), torch.int32, "cand")
    a_len, lengths = G.out((B,), torch.int32, "lengths")
    G.call("umereg_gt_candidates", a_ov, a_nf, B, N, a_cand, a_len, a_ws, n_ws, G.stream)
    a_pk, n_pk = G.ws(G.lib.umereg_ume_moments_workspace_bytes(B, N), "packed")
    G.call("umereg_pack_points_f32", a_pts, B, N, gc.R, a_pk, n_pk, G.stream)
    ns = case.kw["num_samples"]
    a_kp, kp = G.out((B, ns), torch.int64, "kp_index")
    a_rec, rec = G.out((B, 2), torch.int32, "record")
    a_ws2, n_ws2 = G.ws(need, "ws_select")
    G.call("umereg_gt_select_f32", a_pk, a_cand, a_len, B, N, gc.R, case.kw["max_nn"], case.kw["min_nn"], ns, 0, a_kp, a_rec, None,
           a_ws2, n_ws2, G.stream)
    Bk, K = 37, 131
    q, p = gc.ball_any_inputs(Bk, K, 9)
    a_q, _ = G.inp(q)
    a_p, _ = G.inp(p)
    a_hits, hits = G.out((Bk,), torch.int32, "hits")
    G.call("umereg_gt_ball_any_f32", a_q, a_p, Bk, K, gc.INTERSECTION_R, 0, a_hits, G.stream)
    return dict(cand=cand, lengths=lengths, kp_index=kp, record=rec, hits=hits)


def test_every_entry_twice_between_guard_bands_over_differently_filled_workspaces(gpu):
    from umeregrobust_amd import gt_keypoints as gk
    gk.load_native()
    runs = []
    for run in (0, 1):
        G = Guard(gpu, run)
        with torch.cuda.device(gpu):
            outs = guarded_entries(G)
        G.check()
        runs.append({k: v.detach().cpu().clone() for k, v in outs.items()})
        assert G.called >= {"umereg_gt_candidates", "umereg_gt_select_f32", "umereg_gt_ball_any_f32"}
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), \
            f"output `{k}` differs between two runs (an unwritten byte, or a dependence on what the workspace held)"
    assert int(runs[0]["record"][:, 0].min()) == 513 and int(runs[0]["hits"].sum()) > 0


def test_the_generator_reads_the_device_once(gpu):
    from umeregrobust_amd import gt_keypoints as gk
    args = batch_of_three(gpu)
    kw = dict(nn_r=5.0, max_nn=48, min_nn=12, num_samples=40, flat_labels=[9], normalized_ume=False, nn_intersection_r=0.6)
    both(args, kw)                                                       # warm: allocations and lazy initialisation are done
    torch.cuda.synchronize()
    before = gk.host_reads
    torch.cuda.set_sync_debug_mode("warn")                               # torch reports every call of its own that waits for the stream
    try:
        with pytest.warns(UserWarning) as w:
            gk.generate(*args, kw["nn_r"], kw["max_nn"], kw["min_nn"], kw["num_samples"], kw["flat_labels"], False, kw["nn_intersection_r"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [x for x in w if "synchroniz" in str(x.message)]
    print(f"synchronising calls reported: {len(syncs)}; host reads counted by the module: {gk.host_reads - before}")
    assert len(syncs) == 1 and gk.host_reads - before == 1, [str(x.message)[:120] for x in syncs]


# ---- 5. through the callers ------------------------------------------------------------------------------------------------------------

def test_the_loss_and_both_feature_gradients_are_equal_across_selection(gpu):
    from umeregrobust_amd.ume_loss import UMEContrastiveLoss
    src, seg, sf, tgt, tf, gt = batch_of_three(gpu)
    got = []
    for s in ("torch", "device"):
        fn = UMEContrastiveLoss(num_samples=40, max_nn=48, min_nn=12, nn_r=5.0, flat_labels=[9]).with_selection(s)
        a, b = sf.clone().requires_grad_(True), tf.clone().requires_grad_(True)
        out = fn(src, seg, a, tgt, b, gt)
        out[0].backward()
        got.append((out, a.grad, b.grad))
    (out_t, ga_t, gb_t), (out_d, ga_d, gb_d) = got
    assert len(out_t) == len(out_d) == 7 and torch.isfinite(out_t[0])
    for x, y in zip(out_t, out_d):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)
    assert torch.equal(ga_t, ga_d) and torch.equal(gb_t, gb_d) and float(ga_t.abs().sum()) > 0 and float(gb_t.abs().sum()) > 0


def test_the_inlier_ratio_is_equal_across_selection(gpu):
    from umeregrobust_amd.utils.eval_utils import calc_inliear_ratio
    g = load_golden("g8_gt_ume_inlier.npz")
    src = dict(pts=T_(g["src_pts"], gpu)[None], seg=T_(g["src_seg"], gpu)[None], feat=T_(g["src_feat"], gpu)[None])
    tgt = dict(pts=T_(g["tgt_pts"], gpu)[None], seg=None, feat=T_(g["tgt_feat"], gpu)[None])
    gt = T_(g["gt_tform"], gpu)[None]
    kw = dict(ume_r_nn=5.0, ume_max_nn=64, ume_min_nn=10, eval_num_kpts=48, keypoints_ignore_segments=[9], inlear_thr=0.6, nn_inter_thr=0.6)
    a = calc_inliear_ratio(src, tgt, None, gt, selection="torch", **kw)
    b = calc_inliear_ratio(src, tgt, None, gt, selection="device", **kw)
    assert a.shape == b.shape == (1,) and torch.equal(a, b)


SMALL = dict(batch_size=2, ume_max_nn=64, ume_min_nn=8, ume_r_nn=2.0, ume_n_samples=32, num_pw_samples=128, eval_num_kpts=32, lr=1e-3,
             use_aug=False)


class Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def state_bytes(sd):
    if isinstance(sd, torch.Tensor):
        return sd.detach().cpu().numpy().tobytes()
    if isinstance(sd, dict):
        return {k: state_bytes(v) for k, v in sd.items()}
    if isinstance(sd, (list, tuple)):
        return [state_bytes(v) for v in sd]
    return sd


def test_one_epoch_is_the_same_with_and_without_device_keypoints(gpu, tmp_path_factory):
    from umeregrobust_amd import train_coloring as tc
    out = tmp_path_factory.mktemp("runs")
    results = []
    for flag in (False, True):
        args = tc.make_config("kitti", **{**SMALL, "device": str(gpu), "num_epochs": 1, "random_seed": 5})
        log = Scalars()
        run_dir = tc.run(args, synthetic=4, summary_writer=log, out_path=str(out / f"flag_{int(flag)}"), device_keypoints=flag)
        ck = torch.load(os.path.join(run_dir, "last_epoch_checkpoint.pth"), weights_only=True)
        results.append((state_bytes(ck["model_state_dict"]), state_bytes(ck["optimizer_state_dict"]), log.rows))
    (model_a, opt_a, rows_a), (model_b, opt_b, rows_b) = results
    assert [s for t, _, s in rows_a if t == "train/total_loss"] == [0, 1], "both batches of the epoch must have taken a step"
    assert any(t.startswith("train/") and "ume" in t for t, _, _ in rows_a)
    assert rows_a == rows_b, "the (tag, value, step) rows differ, or come in another order"
    assert model_a == model_b and opt_a == opt_b and len(opt_a["state"]) > 0
