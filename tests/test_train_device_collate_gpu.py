"""GPU: the training driver with `device_collate=True` (batches collated on the device, a step's scalars read one batch late)
computes and logs what it does without the flag: four synthetic items of ~3 000 points, batch 2, one epoch, with the small
neighbourhood settings of tests/test_train_coloring_gpu.py (restated here)."""
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


def state_bytes(sd):
    """a (nested) state dict with every tensor replaced by its bytes"""
    if isinstance(sd, torch.Tensor):
        return sd.detach().cpu().numpy().tobytes()
    if isinstance(sd, dict):
        return {k: state_bytes(v) for k, v in sd.items()}
    if isinstance(sd, (list, tuple)):
        return [state_bytes(v) for v in sd]
    return sd


@pytest.mark.parametrize("use_aug", [False, True], ids=["plain_items", "augmented_items"])
def test_one_epoch_is_the_same_with_and_without_the_flag(gpu, use_aug, tmp_path_factory):
    from umeregrobust_amd import train_coloring as tc
    out = tmp_path_factory.mktemp("runs")
    results = []
    for flag in (False, True):
        args = tc.make_config("kitti", **{**SMALL, "device": str(gpu), "num_epochs": 1, "use_aug": use_aug, "random_seed": 5})
        log = Scalars()
        run_dir = tc.run(args, synthetic=4, summary_writer=log, out_path=str(out / f"flag_{int(flag)}"), device_collate=flag)
        ck = torch.load(os.path.join(run_dir, "last_epoch_checkpoint.pth"), weights_only=True)
        results.append((state_bytes(ck["model_state_dict"]), state_bytes(ck["optimizer_state_dict"]), log.rows, np.random.get_state()))
    (model_a, opt_a, rows_a, rng_a), (model_b, opt_b, rows_b, rng_b) = results
    train_rows = [r for r in rows_a if r[0].startswith("train/")]
    print(f"use_aug={use_aug}: {len(train_rows)} training rows, {len(rows_a) - len(train_rows)} validation rows; total losses "
          f"{[round(v, 5) for t, v, _ in train_rows if t == 'train/total_loss']}")
    assert [s for t, _, s in train_rows if t == "train/total_loss"] == [0, 1], "both batches of the epoch must have taken a step"
    assert rows_a == rows_b, "the (tag, value, step) rows differ, or come in another order"
    assert model_a == model_b and opt_a == opt_b
    assert len(opt_a["state"]) > 0
    assert rng_a[0] == rng_b[0] and np.array_equal(rng_a[1], rng_b[1]) and rng_a[2:] == rng_b[2:], "the host RNG was consumed differently"


def test_a_batch_without_matches_is_skipped_under_the_late_read(gpu):
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.synth import synth_train_item
    items = [tuple(t.to(gpu) for t in synth_train_item(100 + i, N=3000, device=gpu)) for i in range(4)]
    rng = np.random.RandomState(0)
    batches = [batch_collate_fn_dset_device(items[a:a + 2], num_matches=SMALL["num_pw_samples"], rng=rng) for a in (0, 2)]
    empty = batches[0][:10] + (torch.zeros(2, 0, 2, dtype=torch.int64, device=gpu),)

    def setup():
        args = tc.make_config("kitti", **{**SMALL, "device": str(gpu)})
        torch.manual_seed(0)
        np.random.seed(0)
        model = ResUNetSmall2(in_channels=1, out_channels=args.out_channels, trainable=True).to(gpu).train()
        pw = MyInfoNCELossNoSeg(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=tc.NEG_EUCLID_DIST)
        return model, pw, torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=tc.WEIGHT_DECAY), tc.TrainContext(args)

    # the empty batch alone: skipped, nothing moves, nothing is reported
    model, pw, opt, ctx = setup()
    before = state_bytes(dict(model.named_parameters()))
    log = Scalars()
    tc.train_one_epoch(0, [empty], model, pw, opt, log, ctx, late_read=True)
    assert ctx.skipped == {"no_matches": 1, "no_keypoints": 0} and log.rows == []
    assert state_bytes(dict(model.named_parameters())) == before and len(opt.state_dict()["state"]) == 0
    # between two real batches: the same skip count, rows and parameters as the plain loop; steps 0 and 2 are reported once each
    got = []
    for late in (False, True):
        model, pw, opt, ctx = setup()
        log = Scalars()
        tc.train_one_epoch(3, [batches[0], empty, batches[1]], model, pw, opt, log, ctx, late_read=late)
        got.append((ctx.skipped, log.rows, state_bytes(model.state_dict()), state_bytes(opt.state_dict())))
    assert got[0][0] == got[1][0] == {"no_matches": 1, "no_keypoints": 0}
    assert [s for t, _, s in got[1][1] if t == "train/total_loss"] == [9, 11]
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] and got[0][3] == got[1][3]
