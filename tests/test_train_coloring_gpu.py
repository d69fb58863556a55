"""GPU: the training driver (umeregrobust_amd/train_coloring.py) on four synthetic items of ~3 000 points, batch 2, with
neighbourhoods sized for such clouds (ume_max_nn 64, ume_min_nn 8, ume_r_nn 2.0, 32 UME samples, 128 point-wise samples)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(batch_size=2, ume_max_nn=64, ume_min_nn=8, ume_r_nn=2.0, ume_n_samples=32, num_pw_samples=128, eval_num_kpts=32, lr=1e-3,
             use_aug=False)


class Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def of(self, tag):
        return [v for t, v, _ in self.rows if t == tag]


@pytest.fixture(scope="module")
def items(gpu):
    from umeregrobust_amd.synth import synth_train_item
    return [synth_train_item(100 + i, N=3000, device=gpu) for i in range(4)]


@pytest.fixture(scope="module")
def batches(items):
    from umeregrobust_amd.datasets.kitti_dataset import batch_collate_fn_dset
    rng = np.random.RandomState(0)
    return [batch_collate_fn_dset(items[a:a + 2], num_matches=SMALL["num_pw_samples"], rng=rng) for a in (0, 2)]


def setup(gpu, seed=0, **over):
    """-> (args, model, point-wise loss, optimizer, context), as `run` builds them, from one seed"""
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    args = tc.make_config("kitti", **{**SMALL, "device": str(gpu), **over})
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = ResUNetSmall2(in_channels=1, out_channels=args.out_channels, trainable=True).to(gpu).train()
    pw = MyInfoNCELossNoSeg(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=tc.NEG_EUCLID_DIST)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=tc.WEIGHT_DECAY)
    return args, model, pw, opt, tc.TrainContext(args)


def state_bytes(sd):
    return {k: (v.detach().cpu().numpy().tobytes() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}


def test_first_iteration_is_the_three_loss_modules(gpu, batches):
    """the three terms the driver logs for its first iteration, and their weighted total, are bit for bit what the three loss modules
    give when called directly on the same batch, weights and initial state (a float32 loss is exact as a Python float)"""
    from umeregrobust_amd import train_coloring as tc
    args, model, pw, opt, ctx = setup(gpu)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    log = Scalars()
    tc.train_one_epoch(0, batches[:1], model, pw, opt, log, ctx)
    got = {k: log.of(f"train/{k}_loss") for k in ("pointwise", "ume", "reg", "total")}
    assert all(len(v) == 1 for v in got.values())
    _, model2, pw2, _, ctx2 = setup(gpu)
    model2.load_state_dict(init)
    b = tc.Batch(batches[0], gpu)
    sf, tf = tc.network_features(model2, b.src), tc.network_features(model2, b.tgt)
    w_pw = pw2(sf, b.src_pts, tf, b.matches)
    w_ume, _, _, su, tu, ratio, valid = ctx2.ume_loss_fn(b.src_pts, b.src_seg, sf, b.tgt_pts, tf, b.gt_tform)
    w_reg, _, _ = ctx2.registration_loss_fn(b.src_pts, su, b.tgt_pts, tu, b.gt_tform, ratio, valid)
    w_total = args.pw_loss_weight * w_pw + args.ume_loss_weight * w_ume + args.reg_loss_weight * w_reg
    print(f"first iteration: pw {got['pointwise'][0]:.6f} ume {got['ume'][0]:.6f} reg {got['reg'][0]:.6f} total {got['total'][0]:.6f}; "
          f"{su.shape[1]} keypoints")
    assert su.shape[1] >= 8 and w_pw.dtype == torch.float32
    assert got["pointwise"][0] == float(w_pw.detach()) and got["ume"][0] == float(w_ume.detach()) and got["reg"][0] == float(w_reg.detach())
    assert got["total"][0] == float(w_total.detach())
    assert (args.pw_loss_weight, args.ume_loss_weight, args.reg_loss_weight) == (0.5, 0.5, 0.25)


def test_one_epoch_moves_every_parameter(gpu, batches):
    from umeregrobust_amd import train_coloring as tc
    _, model, pw, opt, ctx = setup(gpu)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    log = Scalars()
    tc.train_one_epoch(0, batches, model, pw, opt, log, ctx)
    assert len(log.of("train/total_loss")) == 2 and len(log.of("train/reg_loss")) == 2 and ctx.skipped == {"no_matches": 0, "no_keypoints": 0}
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()), k
            assert not torch.equal(p.detach(), before[k]), f"{k} did not move"
    assert sum(p.grad is not None for p in model.parameters()) >= 0.9 * len(before)


def test_25_steps_on_one_batch_lower_the_loss(gpu, batches):
    """25 steps on one repeated batch, augmentation off: the total loss ends strictly below where it began.
    (Measured on an MI355X: see DESIGN 4.13.)"""
    from umeregrobust_amd import train_coloring as tc
    _, model, pw, opt, ctx = setup(gpu)
    log = Scalars()
    tc.train_one_epoch(0, [batches[0]] * 25, model, pw, opt, log, ctx)
    total = log.of("train/total_loss")
    print(f"25 steps: total loss {total[0]:.6f} -> {total[-1]:.6f} (min {min(total):.6f}); pw {log.of('train/pointwise_loss')[0]:.4f} -> "
          f"{log.of('train/pointwise_loss')[-1]:.4f}; ume {log.of('train/ume_loss')[0]:.4f} -> {log.of('train/ume_loss')[-1]:.4f}; "
          f"reg {log.of('train/reg_loss')[0]:.4f} -> {log.of('train/reg_loss')[-1]:.4f}")
    assert len(total) == 25 and all(np.isfinite(total))
    assert total[-1] < total[0]


def test_two_runs_give_the_same_checkpoint_bytes_and_resume_continues(gpu, batches, tmp_path_factory):
    from umeregrobust_amd import train_coloring as tc
    out = tmp_path_factory.mktemp("runs")
    files = []
    for run in range(2):
        _, model, pw, opt, ctx = setup(gpu, seed=3)
        tc.train_one_epoch(0, batches, model, pw, opt, Scalars(), ctx)
        d = out / f"r{run}"
        d.mkdir()
        tc.save_checkpoint(4, 0.5, model, opt, str(d), "last_epoch.pth")
        files.append(d / "last_epoch_checkpoint.pth")
    assert files[0].read_bytes() == files[1].read_bytes()
    # resume into a fresh model / optimizer: state byte-equal to the live ones, START_EPOCH the stored epoch
    _, model2, pw2, opt2, ctx2 = setup(gpu, seed=99)
    assert tc.resume(str(files[1]), model2, opt2, gpu) == 4
    assert state_bytes(model2.state_dict()) == state_bytes(model.state_dict())
    live, back = opt.state_dict(), opt2.state_dict()
    assert live["param_groups"] == back["param_groups"] and sorted(live["state"]) == sorted(back["state"])
    for k in live["state"]:
        assert state_bytes(live["state"][k]) == state_bytes(back["state"][k]), k
    # one further step on the same batch from both
    model2.train()
    tc.train_one_epoch(5, batches[:1], model, pw, opt, Scalars(), ctx)
    tc.train_one_epoch(5, batches[:1], model2, pw2, opt2, Scalars(), ctx2)
    assert state_bytes(model2.state_dict()) == state_bytes(model.state_dict())


def test_eval_returns_six_finite_numbers(gpu, batches):
    from umeregrobust_amd import train_coloring as tc
    _, model, pw, opt, ctx = setup(gpu)
    log = Scalars()
    out = tc.eval_one_epoch(0, batches, model.eval(), pw, log, ctx)
    print("eval:", out)
    assert len(out) == 6 and all(isinstance(v, float) and np.isfinite(v) for v in out)
    assert out[0] == out[1] == out[2], "the reference returns the total loss under three names"
    assert {t for t, _, _ in log.rows} == {"valid/total_loss", "valid/pointwise_loss", "valid/inlear_ratio", "valid/ume_loss", "valid/reg_loss",
                                           "valid/rre", "valid/rte", "valid/chr"}
    # without the registration loss reg_acc is 0.0 (the reference raises there)
    _, model, pw, opt, ctx = setup(gpu, use_reg_loss=False, calc_inlear_ratio_eval=False)
    out = tc.eval_one_epoch(0, batches[:1], model.eval(), pw, Scalars(), ctx)
    assert out[3] == 0.0 and out[4] == 0.0 and out[5] == 0.0 and np.isfinite(out[0])


def test_batches_without_matches_or_keypoints_are_skipped(gpu, batches):
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.datasets.kitti_dataset import batch_collate_fn_dset
    _, model, pw, opt, ctx = setup(gpu)
    params = lambda: state_bytes(dict(model.named_parameters()))          # noqa: E731
    before = params()
    # no matches: the collate's matches are [bs, 0, 2]
    empty = batches[0][:10] + (torch.zeros(2, 0, 2, dtype=torch.int64),)
    # no keypoints: every point of both clouds on one line -- every UME matrix has rank 2, so no keypoint column survives
    n = 400
    line = torch.stack([torch.arange(n) * 0.3 + 0.15, torch.full((n,), 0.15), torch.full((n,), 0.15)], 1).float()
    coords = torch.floor(line / 0.3).int()
    ident = torch.arange(n)[:, None].expand(-1, 2).contiguous()
    item = (line, torch.ones(n, dtype=torch.int64), coords, line.clone(), torch.ones(n, dtype=torch.int64), coords.clone(), line.clone(),
            torch.eye(4), ident)
    flat = batch_collate_fn_dset([item, item], num_matches=128, rng=np.random.RandomState(1))
    log = Scalars()
    tc.train_one_epoch(0, [empty, flat], model, pw, opt, log, ctx)
    assert ctx.skipped == {"no_matches": 1, "no_keypoints": 1} and log.rows == []
    # no optimizer step was taken.  (The no-keypoint batch did go through the network before it was dropped, as in the reference:
    # the batch-norm running statistics have seen it; the no-match batch is dropped before the forward pass.)
    assert params() == before and len(opt.state_dict()["state"]) == 0
    assert int(model.state_dict()["norm2_tr.bn.num_batches_tracked"]) == 2
    out = tc.eval_one_epoch(0, [empty, flat], model.eval(), pw, Scalars(), ctx)
    assert out == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_ume_loss_returns_empty_sets_when_no_keypoint_survives(gpu):
    """`ume_loss.UMEContrastiveLoss` on clouds whose every neighbourhood is degenerate (all points on one line: the moment matrices
    have rank 2): no keypoint column survives, and the module returns what the reference's does -- empty UME tensors and ratio, a
    NaN loss (the mean of nothing) -- instead of failing in the distance kernel.  The trainer's skip tests `src_ume.shape[1] == 0`."""
    from umeregrobust_amd.ume_loss import UMEContrastiveLoss
    n = 400
    line = torch.stack([torch.arange(n) * 0.3 + 0.15, torch.full((n,), 0.15), torch.full((n,), 0.15)], 1).float().to(gpu)
    pts = torch.stack([line, line])
    g = torch.Generator().manual_seed(0)
    feat = torch.nn.functional.normalize(torch.randn(2, n, 32, generator=g), dim=-1).to(gpu).requires_grad_()
    feat2 = feat.detach().clone().requires_grad_()
    fn = UMEContrastiveLoss(num_samples=32, max_nn=64, min_nn=8, nn_r=2.0)
    loss, kp_s, kp_t, ume_s, ume_t, ratio, with_kpts = fn(pts, torch.ones(2, n, 1, dtype=torch.int64, device=gpu), feat, pts, feat2,
                                                          torch.eye(4, device=gpu).expand(2, -1, -1).contiguous())
    assert tuple(ume_s.shape) == (2, 0, 32, 4) == tuple(ume_t.shape) and tuple(ratio.shape) == (2, 0)
    assert bool(with_kpts.all()) and kp_s.shape[0] == 2 and kp_s.shape == kp_t.shape and kp_s.shape[1] > 0
    assert loss.dim() == 0 and bool(torch.isnan(loss))


def test_main_on_synthetic_items_writes_a_checkpoint_the_evaluation_loads(gpu, tmp_path_factory):
    from umeregrobust_amd import train_coloring as tc
    out = tmp_path_factory.mktemp("main")
    run_dir = tc.main(["--synthetic", "4", "--epochs", "1", "--output-path", str(out)])
    names = sorted(os.listdir(run_dir))
    print(names)
    assert "last_epoch_checkpoint.pth" in names and "run_config.json" in names and "scalars.jsonl" in names
    assert "best_total_loss_checkpoint.pth" in names
    ckpt = os.path.join(run_dir, "last_epoch_checkpoint.pth")
    ck = torch.load(ckpt, weights_only=True)
    assert ck["epoch"] == 0 and np.isfinite(ck["total_loss"])
    # `evaluate --cache DIR --checkpoint FILE`: the evaluation's own pair source builds the network from the file and runs it
    from types import SimpleNamespace
    from umeregrobust_amd import evaluate
    from umeregrobust_amd.datasets.kitti_dataset import write_cached_pair
    from umeregrobust_amd.synth import synth_train_item
    cache = tmp_path_factory.mktemp("evalcache")
    item = synth_train_item(7, N=3000, device=gpu)
    write_cached_pair(str(cache / "test" / "00" / "000000_000001.pickle"), item)
    args = SimpleNamespace(dataset="kitti", num_samples=128, max_pc_size=100000)
    pairs = list(evaluate.cached_pairs(str(cache), None, "test", [0], args, gpu, rng=np.random.RandomState(0), checkpoint=ckpt))
    assert len(pairs) == 1
    p = pairs[0]
    assert p["src_feat"].shape == (1, len(item[0]), 32) and p["tgt_feat"].shape == (1, len(item[3]), 32)
    assert bool(torch.isfinite(p["src_feat"]).all()) and bool(torch.isfinite(p["tgt_feat"]).all())
    assert float((p["src_feat"].norm(dim=-1) - 1).abs().max()) < 1e-3          # the network's unit-norm output, not zeros
