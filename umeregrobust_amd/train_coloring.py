"""The reference's training driver (train_coloring.py:20-439) on this library: `ResUNetSmall2(trainable=True)` trained on
`PW * MyInfoNCELossNoSeg + UME * UMEContrastiveLoss + REG * CubeRegistrationLoss`, with the data side of every item -- the
z-rotation augmentation, re-quantisation and ground-truth matches -- on the GPU (datasets.kitti_dataset.augmented_item).

    python -m umeregrobust_amd.train_coloring --config kitti --cache <pair cache dir>
    python -m umeregrobust_amd.train_coloring --config-path my.yaml --cache <dir>
    python -m umeregrobust_amd.train_coloring --synthetic 16 --epochs 2          # no dataset: synth.synth_train_item

`train_one_epoch` / `eval_one_epoch` / `save_model` / `save_checkpoint` / `create_params_dict` keep the reference's names and
leading arguments.  What the reference reads from module globals (device, loss weights, the two other loss modules,
thresholds, inlier-ratio settings) travels in one `TrainContext` passed as the trailing argument.  Config keys are the
reference's (configs/train/*.yaml); the defaults live in `DEFAULTS` below.

The reference's behaviour is mirrored, quirks included; each is named where it happens:
  * a batch whose collate kept no match, or in which no UME keypoint was found, is skipped (no optimizer step);
  * `total = PW * pw + UME * ume + REG * reg`, `PW * pw + UME * ume` without the registration loss, `pw` ALONE (unweighted)
    without the UME loss;
  * `Adam(lr, weight_decay=0)`;
  * resuming from a `_checkpoint` file starts at `START_EPOCH = ckpt['epoch']`, so the saved epoch is run again;
  * six "best" checkpoints plus `last_epoch`, all carrying the validation TOTAL loss;
  * `eval_one_epoch` returns the total loss under three names (total, point-wise, UME);
  * `tgt_inputs['seg']` of the inlier-ratio call is a list holding the batch mask; it is never read;
  * without the registration loss the reference's `eval_one_epoch` raises on its return statement (`valid_reg_acc` is never
    bound); here `reg_acc` is 0.0 then.
Loader workers: the augmented item opens the GPU, which a forked worker must not do -- `num_workers` of the config is
overridden to 0 whenever items are made or collated on the GPU (and the dataset and the device collate raise if asked inside a
worker anyway).

`--device-collate` (`run(..., device_collate=True)`; not a config key: those are the reference's) keeps a training batch on the GPU
end to end: items stay where the augmentation made them, `collate.batch_collate_fn_dset_device` gathers them there, and
`train_one_epoch` reads a step's scalars one batch late, after it has fetched and collated the next batch, so that the host's share
of the data side (item read, augmentation launches, the numpy draws, collate launches) runs under the device's backward pass.  What
is computed, the order in which the host RNG is consumed and everything that is logged are the same as without the flag.

`--device-assignment` (`run(..., device_assignment=True)`) gives the validation epoch's inlier ratio the device solver
(`calc_inliear_ratio(..., assignment="device")`): the distance matrices of a validation batch stay on the GPU and are solved side
by side instead of one after another by scipy on the host.  Off by default.

`--fused-pointwise` (`run(..., fused_pointwise=True)`) computes the point-wise term with `pw_loss.MyInfoNCELossNoSeg`: one fused HIP
forward and backward (include/umereg_infonce.h) instead of the torch statements of `loss.MyInfoNCELossNoSeg`.  Off by default."""
import argparse
import json
import os
import time
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch
import torch.optim as optim

from .cube_loss import CubeRegistrationLoss
from .collate import batch_collate_fn_dset_device
from .datasets.kitti_dataset import CachedPairDataset, batch_collate_fn_dset
from .loss import MyInfoNCELossNoSeg
from .models import ResUNetSmall2
from .pw_loss import MyInfoNCELossNoSeg as FusedInfoNCELossNoSeg
from .sparse import SparseTensor
from .ume_loss import UMEContrastiveLoss
from .utils.eval_utils import calc_inliear_ratio
from .utils.general_utils import update_namespace_from_yaml

# the reference's config keys (configs/train/train_kitti_config.yaml) with its KITTI values; paths are the user's
_COMMON = dict(batch_size=8, cache_data_path="", calc_inlear_ratio_eval=True, data_path="", device="cuda:0", eval_batch_size=-1,
               eval_inlear_thr=0.6, eval_num_kpts=1000, lr=1e-4, max_pc_size=100000, num_epochs=100, num_pw_samples=512,
               num_workers=8, out_channels=32, output_path="outputs", pw_loss_weight=0.5, random_seed=0, reg_loss_cube_r=30.0,
               reg_loss_intersection_thr=0.75, reg_loss_weight=0.25, resume_train_path="", run_name="Coloring",
               skip_invalid_entries=True, tau=0.1, tau_ume=0.1, tau_ume_neg=0.1, train_size=-1, ume_loss_weight=0.5, ume_max_nn=750,
               ume_min_nn=300, ume_n_samples=256, ume_r_nn=5, use_aug=True, use_reg_loss=True, use_ume_loss=True, val_size=-1)
DEFAULTS = {"kitti": dict(_COMMON, dataset="kitti"), "nuscenes": dict(_COMMON, dataset="nuscenes", max_pc_size=40000)}

NEG_EUCLID_DIST = 5             # train_coloring.py:310
REG_ROT_THR_DEG = 5.0           # :313
REG_TRANS_THR_M = 0.6           # :314
WEIGHT_DECAY = 0.0              # :322


def make_config(name="kitti", yaml_path=None, **overrides):
    """Namespace with every key of the reference's training config: our defaults for `name`, then the YAML file (any key the
    reference's files have is accepted; an unknown key is an error, not a silent attribute), then keyword overrides."""
    args = SimpleNamespace(**DEFAULTS[name])
    args.config, args.config_path = name, yaml_path
    if yaml_path is not None:
        before = set(vars(args))
        update_namespace_from_yaml(args, yaml_path)
        unknown = sorted(set(vars(args)) - before)
        if unknown:
            raise KeyError(f"{yaml_path}: unknown config keys {unknown} (known: {sorted(DEFAULTS[name])})")
    for k, v in overrides.items():
        if k not in DEFAULTS[name]:
            raise KeyError(f"unknown config key {k!r}")
        setattr(args, k, v)
    return args


class TrainContext:
    """What the reference's train / eval functions read from module globals (train_coloring.py:263-322), made explicit."""

    def __init__(self, args, ume_loss_fn=None, registration_loss_fn=None, selection="torch"):
        self.selection = selection      # engine of the keypoint generator, training and validation (gt_keypoints)
        self.device = torch.device(args.device)
        self.use_ume_loss, self.use_reg_loss = bool(args.use_ume_loss), bool(args.use_reg_loss)
        self.pw_loss_weight, self.ume_loss_weight, self.reg_loss_weight = args.pw_loss_weight, args.ume_loss_weight, args.reg_loss_weight
        self.reg_rot_thr_deg, self.reg_trans_thr_m = REG_ROT_THR_DEG, REG_TRANS_THR_M
        self.calc_inlear_ratio_eval = bool(args.calc_inlear_ratio_eval)
        self.eval_num_kpts, self.eval_inlear_thr = args.eval_num_kpts, args.eval_inlear_thr
        self.ume_r_nn, self.ume_max_nn, self.ume_min_nn = args.ume_r_nn, args.ume_max_nn, args.ume_min_nn
        # :380-389 (the reference passes no flat_labels: keypoints are drawn from every class)
        self.ume_loss_fn = ume_loss_fn or UMEContrastiveLoss(num_samples=args.ume_n_samples, max_nn=args.ume_max_nn, min_nn=args.ume_min_nn,
                                                             nn_r=args.ume_r_nn, tau=args.tau_ume, tau_neg=args.tau_ume_neg).with_selection(selection)
        self.registration_loss_fn = registration_loss_fn or CubeRegistrationLoss(
            rtume_max_nn=args.ume_max_nn, rtume_r_nn=args.ume_r_nn, nn_inter_ratio_thr=args.reg_loss_intersection_thr,
            cube_scale=args.reg_loss_cube_r)
        self.skipped = {"no_matches": 0, "no_keypoints": 0}


class JsonlWriter:
    """`add_scalar(tag, value, step)` of a SummaryWriter, written as JSON lines (TensorBoard is not a dependency)."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, "scalars.jsonl")
        self._f = open(self.path, "a")

    def add_scalar(self, tag, value, step):
        self._f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self._f.flush()

    def close(self):
        self._f.close()


class Batch:
    """One collated batch on the device: the two sparse tensors the network reads and the tensors the losses read."""

    def __init__(self, data, device):
        (src_pts, src_seg, src_coords, src_ones, tgt_pts, tgt_seg, tgt_coords, tgt_ones, moved, gt_tform, matches) = data[:11]
        self.src = SparseTensor(src_ones, coordinates=src_coords, device=device)
        self.tgt = SparseTensor(tgt_ones, coordinates=tgt_coords, device=device)
        self.src_pts, self.tgt_pts = src_pts.to(device), tgt_pts.to(device)
        self.src_seg, self.tgt_seg = src_seg.to(device)[..., None], tgt_seg.to(device)[..., None]
        self.gt_tform, self.matches = gt_tform.to(device), matches.to(device)
        self.src_pts_tform = moved                       # stays on the host: only the inlier-ratio call takes it, and never reads it


def network_features(model, stensor):
    """[bs, n, C]: the network's rows, split by batch element (every cloud of a collated batch has n rows)."""
    return torch.stack(model(stensor).decomposed_features, dim=0)


def has_matches(data):
    return data[10].shape[1] > 0


def objective(batch, src_feat, tgt_feat, loss_func, ctx):
    """The trainer's objective on one batch -> (terms, extras), or (None, None) when no UME keypoint survived.
    terms: {'pointwise', 'ume', 'reg', 'total'} (absent terms are missing); extras: (valid_batch_entries, rre, rte).
    total = PW pw + UME ume + REG reg; PW pw + UME ume without the registration loss; pw alone, UNWEIGHTED, without the UME loss."""
    terms = {"pointwise": loss_func(src_feat, batch.src_pts, tgt_feat, batch.matches)}
    if not ctx.use_ume_loss:
        terms["total"] = terms["pointwise"]
        return terms, (torch.ones(batch.gt_tform.shape[0], dtype=torch.bool, device=batch.gt_tform.device), None, None)
    terms["ume"], _, _, src_ume, tgt_ume, ratio, valid = ctx.ume_loss_fn(batch.src_pts, batch.src_seg, src_feat, batch.tgt_pts, tgt_feat,
                                                                        batch.gt_tform)
    if src_ume.shape[1] == 0:
        return None, None
    total = ctx.pw_loss_weight * terms["pointwise"] + ctx.ume_loss_weight * terms["ume"]
    rre = rte = None
    if ctx.use_reg_loss:
        # (the full clouds go in where the keypoints would: the reference passes them, and the loss never reads them)
        terms["reg"], rre, rte = ctx.registration_loss_fn(batch.src_pts, src_ume, batch.tgt_pts, tgt_ume, batch.gt_tform, ratio, valid)
        total = total + ctx.reg_loss_weight * terms["reg"]
    terms["total"] = total
    return terms, (valid, rre, rte)


class RunningSums:
    def __init__(self):
        self.v = {}

    def add(self, **values):
        for k, x in values.items():
            self.v[k] = self.v.get(k, 0.0) + float(x)

    def get(self, k):
        return self.v.get(k, 0.0)


def check_loss_is_finite(values, model):
    """Where a step's loss scalars are on the host: with train_precision='f16' the layer-wise path makes no range check of its own
    (it would synchronise), so an activation beyond the f16 range shows here, as a non-finite loss -- name the cause."""
    if getattr(model, "train_precision", "f32") == "f16" and not np.isfinite(values["total"]):
        raise FloatingPointError(f"the training loss is {values['total']} with train_precision='f16': an activation or a gradient left "
                                 "the f16 range (|x| > 65504 reaches the next layer as infinity); train this run with "
                                 "train_precision='f32'")


def train_one_epoch(epoch, data_loader, model, loss_func, optimizer, summary_writer, ctx, late_read=False):
    """The reference's train_one_epoch (train_coloring.py:20-93) with its globals in `ctx`.  Quirks kept: a batch without matches is
    dropped before the forward pass and one without UME keypoints after it (so batch-norm statistics have seen it), both before
    `zero_grad`: model parameters and optimizer stay untouched, and the batch still counts in the step numbering; without the UME
    loss the total is the unweighted point-wise loss; every tenth iteration prints the mean of the last ten.
    late_read: the loop of `train_one_epoch_late_read` instead (same steps, same log; the scalars are read one batch late)."""
    if late_read:
        return train_one_epoch_late_read(epoch, data_loader, model, loss_func, optimizer, summary_writer, ctx)
    sums = RunningSums()
    n_batches = len(data_loader)
    for i, data in enumerate(data_loader):
        if not has_matches(data):
            print("no matches in this batch: skipped")
            ctx.skipped["no_matches"] += 1
            continue
        batch = Batch(data, ctx.device)
        terms, _ = objective(batch, network_features(model, batch.src), network_features(model, batch.tgt), loss_func, ctx)
        if terms is None:
            print("no UME keypoints in this batch: skipped")
            ctx.skipped["no_keypoints"] += 1
            continue
        optimizer.zero_grad()
        terms["total"].backward()
        optimizer.step()
        values = {k: float(v.detach()) for k, v in terms.items()}
        check_loss_is_finite(values, model)
        sums.add(**values)
        for k in ("total", "pointwise", "ume", "reg"):
            if k in values:
                summary_writer.add_scalar(f"train/{k}_loss", values[k], epoch * n_batches + i)
        if (i + 1) % 10 == 0:
            print(" | ".join(f"{k} {sums.get(k) / 10:.4f}" for k in ("total", "pointwise", "ume", "reg")))
            sums = RunningSums()
    print(f"train epoch {epoch + 1} done")


def train_one_epoch_late_read(epoch, data_loader, model, loss_func, optimizer, summary_writer, ctx):
    """`train_one_epoch` with the host reads of a step deferred: once `optimizer.step()` of batch i is enqueued, the NEXT batch is
    fetched and collated first (the host work of the data side then runs while the device is still in the backward pass of batch
    i), and only then are the scalars of batch i read, logged and printed.  Batches are fetched in the same order and between the
    same two steps as in the plain loop, so the host RNG is consumed identically; `add_scalar` sees the same (tag, value, step) rows
    in the same order; the two skip rules are the plain loop's.  The last batch is read before the function returns."""
    sums = RunningSums()
    n_batches = len(data_loader)
    batches = iter(data_loader)
    data = next(batches, None)
    i = 0
    while data is not None:
        launched = None
        if not has_matches(data):
            print("no matches in this batch: skipped")
            ctx.skipped["no_matches"] += 1
        else:
            batch = Batch(data, ctx.device)
            terms, _ = objective(batch, network_features(model, batch.src), network_features(model, batch.tgt), loss_func, ctx)
            if terms is None:
                print("no UME keypoints in this batch: skipped")
                ctx.skipped["no_keypoints"] += 1
            else:
                optimizer.zero_grad()
                terms["total"].backward()
                optimizer.step()
                launched = {k: v.detach() for k, v in terms.items()}
        data = next(batches, None)                        # item read, augmentation, draws, collate: under the step just enqueued
        if launched is not None:
            values = {k: float(v) for k, v in launched.items()}
            check_loss_is_finite(values, model)
            sums.add(**values)
            for k in ("total", "pointwise", "ume", "reg"):
                if k in values:
                    summary_writer.add_scalar(f"train/{k}_loss", values[k], epoch * n_batches + i)
            if (i + 1) % 10 == 0:
                print(" | ".join(f"{k} {sums.get(k) / 10:.4f}" for k in ("total", "pointwise", "ume", "reg")))
                sums = RunningSums()
        i += 1
    print(f"train epoch {epoch + 1} done")


def eval_one_epoch(epoch, data_loader, model, loss_func, summary_writer, ctx, assignment="host"):
    """The reference's eval_one_epoch (train_coloring.py:96-207) -> (valid_loss, valid_pw_loss, valid_ume_loss, valid_reg_loss,
    valid_inlear_ratio, valid_reg_acc).  Quirks kept: the first three are all the TOTAL loss (the UME one 0.0 without the UME loss);
    sums are divided by the number of batches, skipped ones included; the inlier-ratio call gets `[valid_batch_entries]`, a list, as
    the target's 'seg', which it never reads; with `calc_inlear_ratio_eval` off the ratio is 0.  One departure: `valid_reg_acc` is
    0.0 without the registration loss, where the reference's return statement raises UnboundLocalError.  assignment: "host" or
    "device", where the Hungarian matching of the inlier ratio runs (calc_inliear_ratio)."""
    sums = RunningSums()
    n_batches = len(data_loader)
    with_reg = ctx.use_ume_loss and ctx.use_reg_loss
    for i, data in enumerate(data_loader):
        if not has_matches(data):
            print("no matches in this batch: skipped")
            continue
        batch = Batch(data, ctx.device)
        with torch.no_grad():
            src_feat, tgt_feat = network_features(model, batch.src), network_features(model, batch.tgt)
            terms, extras = objective(batch, src_feat, tgt_feat, loss_func, ctx)
            if terms is None:
                print("no UME keypoints in this batch: skipped")
                continue
            valid, rre, rte = extras
            sums.add(**terms)
            if with_reg:
                hit = (rre <= ctx.reg_rot_thr_deg) & (rte <= ctx.reg_trans_thr_m)
                sums.add(rre=rre.median(dim=-1)[0].mean(), rte=rte.median(dim=-1)[0].mean(), reg_acc=hit.float().mean())
            if ctx.calc_inlear_ratio_eval:
                src_inputs = dict(pts=batch.src_pts[valid], seg=batch.src_seg[valid], feat=src_feat[valid])
                tgt_inputs = dict(pts=batch.tgt_pts[valid], seg=[valid], feat=tgt_feat[valid])
                ratio = calc_inliear_ratio(src_inputs, tgt_inputs, batch.src_pts_tform, batch.gt_tform[valid], ctx.ume_r_nn, ctx.ume_max_nn,
                                           ctx.ume_min_nn, eval_num_kpts=ctx.eval_num_kpts, inlear_thr=ctx.eval_inlear_thr,
                                           assignment=assignment, selection=ctx.selection)
                sums.add(inlier_ratio=ratio.mean())
        if (i + 1) % 10 == 0:
            print(" | ".join(f"{k} {sums.get(k) / (i + 1):.4f}" for k in ("total", "pointwise", "ume", "reg")) +
                  f" | inlier ratio {100 * sums.get('inlier_ratio') / (i + 1):.2f}")
    mean = lambda k: sums.get(k) / n_batches          # noqa: E731
    total = mean("total")
    scalars = [("total_loss", total), ("pointwise_loss", total), ("inlear_ratio", mean("inlier_ratio"))]       # (sic: the total, twice)
    if ctx.use_ume_loss:
        scalars.append(("ume_loss", total))                                                                   # (sic)
    if with_reg:
        scalars += [("reg_loss", mean("reg")), ("rre", mean("rre")), ("rte", mean("rte")), ("chr", mean("reg_acc"))]
    for tag, value in scalars:
        summary_writer.add_scalar("valid/" + tag, value, epoch)
    print(f"validation epoch {epoch + 1} done")
    return (total, total, total if ctx.use_ume_loss else 0.0, mean("reg") if with_reg else 0.0, mean("inlier_ratio"),
            mean("reg_acc") if with_reg else 0.0)


def save_model(model, save_path, save_name):
    """train_coloring.py:210-212: the bare state dict."""
    torch.save(model.state_dict(), os.path.join(save_path, save_name))


def checkpoint_file_name(save_name):
    """`best_total_loss.pth` -> `best_total_loss_checkpoint.pth` (train_coloring.py:221; every `.pth` in the name is replaced)."""
    return save_name.replace('.pth', '_checkpoint.pth')


def checkpoint_dict(epoch, total_loss, model, optimizer):
    return {'epoch': epoch, 'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(), 'total_loss': total_loss}


def save_checkpoint(epoch, total_loss, model, optimizer, save_path, save_name):
    """train_coloring.py:215-222: {epoch, model_state_dict, optimizer_state_dict, total_loss} at `<name>_checkpoint.pth`
    (`os.path.join` first, then the replacement, as there: a `.pth` in the DIRECTORY name is replaced too)."""
    full_save_path = os.path.join(save_path, save_name)
    torch.save(checkpoint_dict(epoch, total_loss, model, optimizer), checkpoint_file_name(full_save_path))


def resume(path, model, optimizer, device):
    """train_coloring.py:369-376 and :394-397 -> START_EPOCH.  A `_checkpoint` file restores model and optimizer and gives
    `ckpt['epoch']` -- the epoch that was SAVED, which is therefore run again (the reference does not add 1); any other file
    is a bare state dict, and training starts at epoch 0 with a fresh optimizer.  The test is the reference's: `"_checkpoint" in path`,
    on the whole path, directories included."""
    print(f'Resume Model: {path}')
    if "_checkpoint" in path:
        ckpt = torch.load(path, map_location=device, weights_only=True)
        model.load_state_dict(ckpt['model_state_dict'])
        optimizer.load_state_dict(ckpt['optimizer_state_dict'])
        print(f"Continue from Epoch: {ckpt['epoch']}")
        return ckpt['epoch']
    model.load_state_dict(torch.load(path, map_location=device, weights_only=True))
    return 0


def create_params_dict(args, run_name, out_path, model):
    """train_coloring.py:225-249: the run's parameters, also written to `<out_path>/run_config.json`."""
    config_dict = {'run_name': run_name, 'seed': args.random_seed, 'device': str(args.device), 'num_workers': args.num_workers,
                   'data_path': args.cache_data_path, 'checkpoint_path': out_path, 'num_epochs': args.num_epochs,
                   'num_samples': args.num_pw_samples, 'batch_size': args.batch_size, 'num_out_ch': args.out_channels, 'tau': args.tau,
                   'USE_UME_LOSS': args.use_ume_loss, 'ume_n_samples': args.ume_n_samples, 'UME_MAX_NN': args.ume_max_nn,
                   'UME_MIN_NN': args.ume_min_nn, 'UME_R_NN': args.ume_r_nn, 'PW_LOSS_WEIGHT': args.pw_loss_weight,
                   'UME_LOSS_WEIGHT': args.ume_loss_weight, 'LR': args.lr, 'WEIGHT_DECAY': WEIGHT_DECAY,
                   'model_type': model.__class__.__name__}
    with open(os.path.join(out_path, 'run_config.json'), 'w') as f:
        json.dump(config_dict, f, indent=6)
    return config_dict


class SyntheticPairs(torch.utils.data.Dataset):
    """`n_items` items of `synth.synth_train_item` (made once, on the GPU, in the constructor), optionally augmented like a cache item."""

    def __init__(self, n_items, n_points=3000, seed=0, use_augmentations=False, voxel_size=0.3, device=None, rng=np.random,
                 items_on_device=False):
        """items_on_device: the stored items live on the device (all but gt_tform, which the augmentation reads on the host), and an
        augmented item stays there: for the device-side collate."""
        from .synth import synth_train_item
        self.items = [synth_train_item(seed + i, N=n_points, voxel=voxel_size, device=device) for i in range(n_items)]
        self.use_augmentations, self.voxel_size, self.device, self.rng = use_augmentations, voxel_size, device, rng
        self.items_on_device = bool(items_on_device)
        if self.items_on_device:
            dev = self._device()
            self.items = [tuple(t if k == 7 else t.to(dev) for k, t in enumerate(item)) for item in self.items]

    def _device(self):
        return torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        if not self.use_augmentations:
            return self.items[idx]
        from .datasets.kitti_dataset import _refuse_gpu_in_worker, augmented_item
        _refuse_gpu_in_worker("SyntheticPairs(use_augmentations=True)")
        return augmented_item(self.items[idx], self.voxel_size, self.rng, self._device(), to_host=not self.items_on_device)


def make_loaders(args, synthetic=0, synthetic_points=3000, device_collate=False):
    """train_coloring.py:324-363.  The train loader shuffles (torch's RNG), the validation loader does not; both collate with
    `batch_collate_fn_dset(num_matches=num_pw_samples, max_pc_size=max_pc_size)`.  device_collate: items stay on the device and both
    loaders collate there (`collate.batch_collate_fn_dset_device`: the same batches), without pinning (torch refuses to pin device
    tensors)."""
    collate_fn = partial(batch_collate_fn_dset, num_matches=args.num_pw_samples, max_pc_size=args.max_pc_size)
    if device_collate:
        collate_fn = partial(batch_collate_fn_dset_device, num_matches=args.num_pw_samples, max_pc_size=args.max_pc_size, device=args.device)
    if synthetic:
        n_val = max(1, synthetic // 4)
        dset_train = SyntheticPairs(synthetic, synthetic_points, seed=args.random_seed, use_augmentations=args.use_aug, device=args.device,
                                    items_on_device=device_collate)
        dset_valid = SyntheticPairs(n_val, synthetic_points, seed=args.random_seed + 100003, device=args.device, items_on_device=device_collate)
    else:
        if not args.cache_data_path:
            raise ValueError("no pair cache: give --cache DIR (or `cache_data_path` in the config), or --synthetic N")

        def cached(split, size, aug):
            d = CachedPairDataset(args.cache_data_path, split=split, dataset=args.dataset, use_augmentations=aug, device=args.device,
                                  items_on_device=device_collate)
            if size != -1:
                d.files = d.files[:size]
            return d
        dset_train, dset_valid = cached('train', args.train_size, args.use_aug), cached('val', args.val_size, False)
    # a worker process must not open the GPU: items made there (augmentation) or collated there force the loading into this process
    workers = 0 if (args.use_aug or synthetic or device_collate) else args.num_workers
    mk = lambda d, shuffle: torch.utils.data.DataLoader(d, shuffle=shuffle, num_workers=workers, batch_size=args.batch_size,
                                                        collate_fn=collate_fn, pin_memory=not device_collate)
    return mk(dset_train, True), mk(dset_valid, False)


def run(args, synthetic=0, synthetic_points=3000, summary_writer=None, out_path=None, device_collate=False, device_assignment=False,
        train_precision="f32", fused_norm=False, conv_mode="union", fused_pointwise=False, device_keypoints=False):
    """train_coloring.py:263-437 -> the run directory.  Quirks kept: every "best" file stores the validation TOTAL loss; the
    UME and point-wise "best" follow the total (eval_one_epoch returns it three times); without the registration loss the validation
    registration loss is 0.0, so `best_reg_loss` (from inf) is written once, after the first epoch, and `best_mCHR` (from 0.0) never.
    device_collate: batches are collated on the device and the training loop reads its scalars one batch late (module docstring).
    device_assignment: the validation epoch's Hungarian matching runs on the device (module docstring).
    train_precision: "f32", or "f16" for f16 operands in the network's layer-wise path (models.py; f32 parameters, so checkpoints
    are the same either way); a non-finite loss then raises FloatingPointError.
    fused_norm: batch norm, residual and ReLU of the layer-wise path on the kernels of include/umereg_bn_act.h (models.py; the same
    parameters and checkpoint keys).
    conv_mode: "union", or "pairs" for the pair-compacted engine of the 27-offset convolutions (models.py; the same values bit for bit).
    fused_pointwise: the point-wise loss is `pw_loss.MyInfoNCELossNoSeg`, the fused HIP forward and backward of include/umereg_infonce.h, in
    place of the torch statements of `loss.MyInfoNCELossNoSeg` (same constructor and call; values agree to fp32 rounding).
    device_keypoints: the ground-truth-driven keypoints of the UME loss and of the validation inlier ratio are selected on the device
    (`generate_ume_from_keypoints2(..., selection="device")`, include/umereg_gt_keypoints.h; the same keypoints and values bit for bit)."""
    torch.manual_seed(args.random_seed)
    np.random.seed(args.random_seed)
    device = torch.device(args.device)
    if out_path is None:
        run_name = f"{args.run_name}_{args.dataset}_{time.strftime('%d%m%y_%H%M%S')}"
        out_path = os.path.join(args.output_path, run_name)
    else:
        run_name = os.path.basename(os.path.normpath(out_path))
    os.makedirs(out_path, exist_ok=True)
    dloader_train, dloader_valid = make_loaders(args, synthetic, synthetic_points, device_collate)
    model = ResUNetSmall2(in_channels=1, out_channels=args.out_channels, trainable=True, train_precision=train_precision,
                          fused_norm=fused_norm, conv_mode=conv_mode).to(device)
    pw_class = FusedInfoNCELossNoSeg if fused_pointwise else MyInfoNCELossNoSeg
    point_wise_loss_fn = pw_class(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=NEG_EUCLID_DIST)
    ctx = TrainContext(args, selection="device" if device_keypoints else "torch")
    optimizer = optim.Adam(model.parameters(), lr=args.lr, weight_decay=WEIGHT_DECAY)
    start_epoch = resume(args.resume_train_path, model, optimizer, device) if args.resume_train_path != '' else 0
    create_params_dict(args, run_name, out_path, model)
    own_writer = summary_writer is None
    summary_writer = summary_writer or JsonlWriter(out_path)
    best = {"best_total_loss": np.inf, "best_pointwise_loss": np.inf, "best_ume_loss": np.inf, "best_reg_loss": np.inf,
            "best_inlear_ratio": 0.0, "best_mCHR": 0.0}
    for epoch in range(start_epoch, args.num_epochs):
        model.train()
        train_one_epoch(epoch, dloader_train, model, point_wise_loss_fn, optimizer, summary_writer, ctx, late_read=device_collate)
        model.eval()
        total, pw, ume, reg, inlear, mchr = eval_one_epoch(epoch, dloader_valid, model, point_wise_loss_fn, summary_writer, ctx,
                                                            assignment="device" if device_assignment else "host")
        for name, value, better in (("best_total_loss", total, total < best["best_total_loss"]),
                                    ("best_pointwise_loss", pw, pw < best["best_pointwise_loss"]),
                                    ("best_ume_loss", ume, ume < best["best_ume_loss"]),
                                    ("best_reg_loss", reg, reg < best["best_reg_loss"]),
                                    ("best_inlear_ratio", inlear, inlear > best["best_inlear_ratio"]),
                                    ("best_mCHR", mchr, mchr > best["best_mCHR"])):
            if better:
                best[name] = value
                save_checkpoint(epoch, total, model, optimizer, out_path, name + ".pth")
        save_checkpoint(epoch, total, model, optimizer, out_path, "last_epoch.pth")
    if own_writer:
        summary_writer.close()
    return out_path


def main(argv=None):
    parser = argparse.ArgumentParser(description="Train ResUNetSmall2 with the reference's objective (train_coloring.py)")
    parser.add_argument('--config', type=str, choices=['kitti', 'nuscenes'], default="kitti")
    parser.add_argument('--config-path', default=None, help="a YAML file with the reference's training-config keys (over the defaults)")
    parser.add_argument('--cache', default=None, help="pair cache directory (the config's cache_data_path)")
    parser.add_argument('--synthetic', type=int, default=0, metavar="N_ITEMS", help="train on N synthetic items instead of a cache")
    parser.add_argument('--synthetic-points', type=int, default=3000)
    parser.add_argument('--epochs', type=int, default=None, help="num_epochs of the config")
    parser.add_argument('--batch-size', type=int, default=None)
    parser.add_argument('--output-path', default=None)
    parser.add_argument('--resume', default=None, help="resume_train_path of the config")
    parser.add_argument('--device-collate', action='store_true',
                        help="collate on the GPU and read each step's scalars one batch late (same batches, same log)")
    parser.add_argument('--device-assignment', action='store_true',
                        help="solve the validation epoch's Hungarian matching on the GPU instead of with scipy on the host")
    parser.add_argument('--train-precision', choices=['f32', 'f16'], default='f32',
                        help="operand precision of the network's forward and backward matrix products (f32 sums and parameters)")
    parser.add_argument('--fused-norm', action='store_true',
                        help="run the network's batch norm, residual and ReLU (and the f16 gradient scale) on the fused HIP kernels")
    parser.add_argument('--conv-mode', choices=['union', 'pairs'], default='union',
                        help="engine of the network's 27-offset convolutions, forward and input gradient (pairs: pair-compacted; same values)")
    parser.add_argument('--fused-pointwise', action='store_true',
                        help="run the point-wise InfoNCE loss, forward and backward, on the fused HIP kernels (pw_loss.MyInfoNCELossNoSeg)")
    parser.add_argument('--device-keypoints', action='store_true',
                        help="select the UME loss's and the inlier ratio's keypoints on the GPU (lazy density test, one host read; same values)")
    cli = parser.parse_args(argv)
    over = {k: v for k, v in (("cache_data_path", cli.cache), ("num_epochs", cli.epochs), ("batch_size", cli.batch_size),
                              ("output_path", cli.output_path), ("resume_train_path", cli.resume)) if v is not None}
    args = make_config(cli.config, cli.config_path, **over)
    if cli.synthetic and cli.config_path is None:
        # a synthetic item has ~synthetic_points points: the KITTI neighbourhood sizes (750 in 5 m) do not exist on it
        args.ume_max_nn, args.ume_min_nn, args.ume_r_nn, args.ume_n_samples, args.num_pw_samples = 64, 8, 2.0, 32, 128
        args.eval_num_kpts, args.batch_size = 32, min(args.batch_size, 2)
    print(f"Train {args.dataset} config: {cli.config_path or 'built-in defaults'}")
    out = run(args, synthetic=cli.synthetic, synthetic_points=cli.synthetic_points, device_collate=cli.device_collate,
              device_assignment=cli.device_assignment, train_precision=cli.train_precision, fused_norm=cli.fused_norm,
              conv_mode=cli.conv_mode, fused_pointwise=cli.fused_pointwise, device_keypoints=cli.device_keypoints)
    print(f"run directory: {out}")
    return out


if __name__ == '__main__':
    main()
