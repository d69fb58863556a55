"""Where a training step spends its time, at the trainer's shape: synthetic 50 000-point items, batch 2 and batch 8, K = 750,
r = 5, 256 UME samples, 512 point-wise samples.

    python tools/train_step_time.py [--points 50000] [--steps 7] [--warmup 3] [--out profiles/train/train_step_time.jsonl]
    python tools/train_step_time.py --device-collate          # only the "device_collate" lines below
    python tools/train_step_time.py --phases-only [--train-precision f16]      # only the "phases" lines

`--train-precision f16`: the network of the "phases" lines is ResUNetSmall2(trainable=True, train_precision="f16") (f16 operands
in its forward and backward, include/umereg_sparse_conv_f16.h); every "phases" line carries a "train_precision" key.

Three kinds of lines (JSON, appended to --out):
  * "phases": per-phase medians of one training step.  Device phases are timed with events on the stream after warm-up
    (the elapsed time between two events recorded around the phase, read after the step's final synchronisation); host phases
    (item read = unpickling a cache file, collate) with the host clock.  The augmentation is split into its parts: rotation +
    thinning + coordinates, grid points, matches.
  * "matches": the new match kernel (`gt_matches.one_side`) against the composition available before it (`ops.nn1_pair`
    followed by a torch distance, threshold and mask), on the same inputs: an ordinary pair and a half-overlapping one
    (`synth_pair_hard`), both thinned to their grid points, at radius voxel / 2.  The two are called alternately, --match-reps
    times each after a warm-up, and the medians reported; both include the one device -> host read of the row count.
    `nn1_pair` serves two clouds per call: its second one is given 64 points, so that it builds one 50 000-point structure,
    like the new call.  The same line carries the host cost of the reference's way: scipy's KDTree build + query + mask on
    the same points (host clock, median of 3).
  * "device_collate" (--device-collate): the trainer's loop on the same cached items in three forms, in one process --
    "host" (items back to the host, `batch_collate_fn_dset`, batch up again, scalars read at once: the loop as it is without the
    flag), "device" (items stay on the device, `collate.batch_collate_fn_dset_device`, scalars read at once) and "device_late" (the
    same with the scalars read after the next batch has been fetched and collated: `--device-collate` of the driver).  The forms
    take turns, --rounds times each, warmup + steps consecutive steps per turn; per turn the medians (host clock) of the step's
    wall time from one `optimizer.step()` to the next, of the whole fetch (item read + augmentation + collate) and of the
    collate call alone.  The difference between the "host" turns is the run-to-run spread against which the others are read.
    "draws_ms" is the time of the collate's numpy draws alone (the same `choice` calls on the batch's sizes; the match draw on
    the item's match count, an upper bound of its survivor count)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class Phases:
    def __init__(self):
        self.events, self.host = {}, {}

    def gpu(self, name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.events.setdefault(name, []).append((a, b))
        return a, b

    def add_host(self, name, seconds):
        self.host.setdefault(name, []).append(seconds * 1e3)

    def medians(self, skip):
        torch.cuda.synchronize()
        out = {k: statistics.median([a.elapsed_time(b) for a, b in v][skip:]) for k, v in self.events.items()}
        out.update({k: statistics.median(v[skip:]) for k, v in self.host.items()})
        return {k: round(v, 4) for k, v in out.items()}


class timed:
    def __init__(self, ph, name):
        self.a, self.b = ph.gpu(name)

    def __enter__(self):
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()


def step_phases(points, batch, steps, warmup, dev, train_precision="f32", fused_norm=False, fused_pointwise=False, device_keypoints=False):
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.datasets.kitti_dataset import augmented_item, batch_collate_fn_dset, read_cached_pair, write_cached_pair
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.synth import synth_train_item
    args = tc.make_config("kitti", batch_size=batch, device=str(dev))          # K = 750, r = 5, 256 UME samples, 512 point-wise samples
    tmp = tempfile.mkdtemp()
    paths = []
    for i in range(batch):
        paths.append(os.path.join(tmp, f"{i}.pickle"))
        write_cached_pair(paths[-1], synth_train_item(500 + i, N=points, device=dev))
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    model = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, train_precision=train_precision, fused_norm=fused_norm).to(dev).train()
    if fused_pointwise:
        from umeregrobust_amd.pw_loss import MyInfoNCELossNoSeg             # noqa: F811  (the fused class, same constructor)
    pw = MyInfoNCELossNoSeg(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=tc.NEG_EUCLID_DIST)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=0.0)
    ctx = tc.TrainContext(args, selection="device" if device_keypoints else "torch")
    ph = Phases()
    n_pts = None
    for _ in range(warmup + steps):
        items = []
        for p in paths:
            t0 = time.perf_counter()
            item = read_cached_pair(p)
            ph.add_host("item_read_host", time.perf_counter() - t0)
            t0 = time.perf_counter()
            items.append(augmented_item(item, 0.3, rng, dev, phase=lambda name: timed(ph, "aug_" + name)))
            ph.add_host("aug_item_wall_host", time.perf_counter() - t0)
        t0 = time.perf_counter()
        data = batch_collate_fn_dset(items, num_matches=args.num_pw_samples, max_pc_size=args.max_pc_size, rng=rng)
        ph.add_host("collate_host", time.perf_counter() - t0)
        n_pts = (data[0].shape[1], data[4].shape[1], data[10].shape[1])
        with timed(ph, "h2d"):
            b = tc.Batch(data, dev)
        with timed(ph, "net_forward"):
            sf, tf = tc.network_features(model, b.src), tc.network_features(model, b.tgt)
        with timed(ph, "loss_pointwise"):
            l_pw = pw(sf, b.src_pts, tf, b.matches)
        with timed(ph, "loss_ume"):
            l_ume, _, _, su, tu, ratio, valid = ctx.ume_loss_fn(b.src_pts, b.src_seg, sf, b.tgt_pts, tf, b.gt_tform)
        with timed(ph, "loss_reg"):
            l_reg, _, _ = ctx.registration_loss_fn(b.src_pts, su, b.tgt_pts, tu, b.gt_tform, ratio, valid)
        total = 0.5 * l_pw + 0.5 * l_ume + 0.25 * l_reg
        opt.zero_grad()
        with timed(ph, "backward"):
            total.backward()
        with timed(ph, "optimizer"):
            opt.step()
        torch.cuda.synchronize()
    med = ph.medians(warmup)
    # per-item phases were recorded `batch` (or 2 x batch) times per step: report them per STEP as well
    per_item = {"aug_to_device": 2, "aug_thinning": 2, "aug_grid_points": 2, "aug_matches": 1, "aug_to_host": 1, "item_read_host": 1,
                "aug_item_wall_host": 1}
    per_step = {k: round(v * per_item.get(k, 0) * batch, 4) if k in per_item else v for k, v in med.items()}
    return {"kind": "phases", "train_precision": train_precision, "fused_norm": bool(fused_norm), "fused_pointwise": bool(fused_pointwise), "device_keypoints": bool(device_keypoints), "points": points, "batch": batch, "steps": steps, "warmup": warmup, "collated_src_tgt_matches": n_pts,
            "keypoints": int(su.shape[1]), "median_ms_per_call": med, "median_ms_per_step": per_step}


def match_compare(points, reps, warmup, dev, hard):
    from umeregrobust_amd import gt_matches, ops
    from umeregrobust_amd.datasets.kitti_dataset import quantize_on_device, rotate_rows
    from umeregrobust_amd.synth import synth_pair, synth_pair_hard
    from umeregrobust_amd.utils.general_utils import convert_coords_to_grid_pts
    p = (synth_pair_hard if hard else synth_pair)(77, N=points, n_kp=16)
    clouds = []
    for pts in (p.src_pts, p.tgt_pts):
        pts = torch.from_numpy(pts + np.float32(0.15)).to(dev)
        coords, _ = quantize_on_device(pts, 0.3)
        clouds.append(convert_coords_to_grid_pts(pts, coords, 0.3).contiguous())
    src, tgt = clouds
    T = torch.from_numpy(p.gt_tform).to(dev)
    r = 0.15
    few = tgt[:64].contiguous()

    def new():
        return gt_matches.one_side(src, tgt, T, r)

    def composed():
        moved = rotate_rows(src, T[:3, :3].T.contiguous()) + T[:3, 3]
        idx, _ = ops.nn1_pair(moved, few, tgt, few)         # (the pair call's second cloud: 64 points, so ONE large structure is built)
        keep = (moved - tgt[idx]).norm(dim=-1) < r
        i = torch.nonzero(keep)[:, 0]                       # (a device -> host read of the count, like the kernel's)
        return torch.stack([i, idx[i]], dim=1)

    variants = (("gt_matches", new), ("nn1_pair_composed", composed))
    times, rows = {k: [] for k, _ in variants}, {}
    for k in range(warmup + reps):                          # alternately, so that clocks and caches are the same for both
        for name, fn in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                times[name].append(a.elapsed_time(b))
            rows[name] = int(out.shape[0])
    res = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "rows": rows[name]} for name, v in times.items()}
    # the reference's way, on the host: torch matmul transform, scipy KDTree build + 1-NN query + mask (utils/general_utils.py:38-44)
    from scipy.spatial import KDTree
    s_h, t_h, T_h = src.cpu(), tgt.cpu().numpy(), T.cpu()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        moved = (s_h @ T_h[:3, :3].T + T_h[:3, 3]).numpy()
        dist, idx = KDTree(t_h).query(moved, 1)
        keep = dist < r
        host_rows = np.stack([np.flatnonzero(keep), idx[keep]], axis=1)
        host.append((time.perf_counter() - t0) * 1e3)
    return {"kind": "matches", "pair": "half-overlapping" if hard else "ordinary", "n_src": int(src.shape[0]), "n_tgt": int(tgt.shape[0]),
            "radius": r, "reps": reps, **res, "ratio_composed_over_new": round(res["nn1_pair_composed"]["median_ms"] / res["gt_matches"]["median_ms"], 3),
            "host_kdtree": {"median_ms": round(statistics.median(host), 3), "rows": int(host_rows.shape[0])}}


def device_collate_compare(points, batch, steps, warmup, rounds, dev):
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    from umeregrobust_amd.datasets.kitti_dataset import augmented_item, batch_collate_fn_dset, read_cached_pair, write_cached_pair
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.synth import synth_train_item
    args = tc.make_config("kitti", batch_size=batch, device=str(dev))
    tmp = tempfile.mkdtemp()
    paths = []
    for i in range(batch):
        paths.append(os.path.join(tmp, f"{i}.pickle"))
        write_cached_pair(paths[-1], synth_train_item(500 + i, N=points, device=dev))
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    model = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True).to(dev).train()
    pw = MyInfoNCELossNoSeg(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=tc.NEG_EUCLID_DIST)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=0.0)
    ctx = tc.TrainContext(args)
    sizes = {}

    def fetch(on_device, t_fetch, t_collate):
        t0 = time.perf_counter()
        items = [augmented_item(read_cached_pair(p), 0.3, rng, dev, to_host=not on_device) for p in paths]
        t1 = time.perf_counter()
        collate = batch_collate_fn_dset_device if on_device else batch_collate_fn_dset
        data = collate(items, num_matches=args.num_pw_samples, max_pc_size=args.max_pc_size, rng=rng)
        t2 = time.perf_counter()
        t_fetch.append((t2 - t0) * 1e3)
        t_collate.append((t2 - t1) * 1e3)
        sizes.update(clouds=[(len(it[0]), len(it[3]), len(it[8])) for it in items], n_src=data[0].shape[1], n_tgt=data[4].shape[1],
                     k=data[10].shape[1])
        return data

    def turn(on_device, late):
        t_fetch, t_collate, stamps = [], [], []
        data = fetch(on_device, t_fetch, t_collate)
        for _ in range(warmup + steps + 1):
            b = tc.Batch(data, dev)
            terms, _ = tc.objective(b, tc.network_features(model, b.src), tc.network_features(model, b.tgt), pw, ctx)
            opt.zero_grad()
            terms["total"].backward()
            opt.step()
            stamps.append(time.perf_counter())
            if late:
                data = fetch(on_device, t_fetch, t_collate)
                values = {k: float(v.detach()) for k, v in terms.items()}
            else:
                values = {k: float(v.detach()) for k, v in terms.items()}
                data = fetch(on_device, t_fetch, t_collate)
            assert np.isfinite(values["total"])
        torch.cuda.synchronize()
        wall = [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])]
        med = lambda v: round(statistics.median(v[warmup:]), 4)                                             # noqa: E731
        return {"step_wall_ms": med(wall), "step_wall_min_ms": round(min(wall[warmup:]), 4), "fetch_ms": med(t_fetch[1:]),
                "collate_ms": med(t_collate[1:])}

    forms = (("host", False, False), ("device", True, False), ("device_late", True, True))
    res = {name: [] for name, _, _ in forms}
    for _ in range(rounds):
        for name, on_device, late in forms:
            res[name].append(turn(on_device, late))
    # the collate's draws alone, on the sizes of the last batch (a generator of their own: the loop's stream is not touched)
    own, draws = np.random.RandomState(1), []
    for _ in range(warmup + steps):
        t0 = time.perf_counter()
        for ns, nt, _ in sizes["clouds"]:
            own.choice(ns, sizes["n_src"], replace=False)
            own.choice(nt, sizes["n_tgt"], replace=False)
        for _, _, m in sizes["clouds"]:
            own.choice(max(m, sizes["k"]), sizes["k"], replace=False)          # (the item's match count stands in for its survivor count)
        draws.append((time.perf_counter() - t0) * 1e3)
    return {"kind": "device_collate", "points": points, "batch": batch, "steps": steps, "warmup": warmup, "rounds": rounds,
            "collated_src_tgt_matches": (sizes["n_src"], sizes["n_tgt"], sizes["k"]), "draws_ms": round(statistics.median(draws[warmup:]), 4),
            **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--match-reps", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="*", default=[2, 8])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train", "train_step_time.jsonl"))
    ap.add_argument("--device-collate", action="store_true", help="only the host / device / device_late comparison of the collate")
    ap.add_argument("--rounds", type=int, default=2, help="turns per form of the --device-collate comparison")
    ap.add_argument("--train-precision", default="f32", choices=["f32", "f16"], help="operand precision of the network in the phases lines")
    ap.add_argument("--fused-norm", action="store_true", help="the network of the phases lines with fused_norm=True (include/umereg_bn_act.h)")
    ap.add_argument("--fused-pointwise", action="store_true", help="the point-wise loss of the phases lines on pw_loss.MyInfoNCELossNoSeg")
    ap.add_argument("--device-keypoints", action="store_true", help="the UME loss of the phases lines with selection=\"device\" (include/umereg_gt_keypoints.h)")
    ap.add_argument("--phases-only", action="store_true", help="skip the match-kernel comparison")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        if a.device_collate:
            for batch in a.batches:
                line = device_collate_compare(a.points, batch, a.steps, a.warmup, a.rounds, dev)
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")
                f.flush()
            return
        for hard in () if a.phases_only else (False, True):
            line = match_compare(a.points, a.match_reps, 10, dev, hard)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
            f.flush()
        for batch in a.batches:
            line = step_phases(a.points, batch, a.steps, a.warmup, dev, a.train_precision, a.fused_norm, a.fused_pointwise, a.device_keypoints)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
