"""Time generate_ume_from_keypoints2 with selection="torch" (the default path) against selection="device" on the same inputs in one
process, the two engines alternating; one JSON line per shape.

    python tools/gt_keypoints_time.py [--out profiles/gt_keypoints/gt_keypoints_time.jsonl] [--iters 15] [--warmup 3] [--points 45000]

Shapes: the trainer's (bs 2 and 8, max_nn 750, min_nn 300, num_samples 256, nn_r 5) and the validation's (num_samples 1000, bs 2) on
synthetic pairs of `--points` points (synth.synth_pair; the ground, z < -1.4 m, is the flat class).  Per shape:

  * `generator_ms`: the whole call, median and minimum over `--iters` calls per engine after `--warmup` calls, each call between two
    device events and ended by a synchronise (the call reads the device, so the events bracket all of it);
  * `pieces_ms`: the three new entries alone on the inputs the generator gives them (candidates, select with the packing of the search
    structure, ball_any) and, for scale, the default path's counterparts (the two sorts are not separable from it and are not listed):
    the moment matrices of every candidate, and the K = 1 ball query over bs * num_samples tiny clouds;
  * `tested_share`: candidates whose ball was tested / candidates below the batch-minimum length (it varies from run to run);
  * `host_syncs`: calls that made the host wait for the stream, as torch's sync debug mode reports them, per engine;
  * `equal`: the six outputs of the two engines are torch.equal at this shape."""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from umeregrobust_amd import gt_keypoints as gk, ops                                    # noqa: E402
from umeregrobust_amd.synth import FLAT_LABEL, synth_pair                               # noqa: E402
from umeregrobust_amd.utils.loc_utils import generate_ume_from_keypoints2               # noqa: E402

SHAPES = (("train", 2, 256), ("train", 8, 256), ("validation", 2, 1000))
KW = dict(nn_r=5.0, max_nn=750, min_nn=300, flat_labels=[FLAT_LABEL], normalized_ume=True, nn_intersection_r=0.6)


def inputs(dev, bs, points):
    ps = [synth_pair(900 + i, N=points, n_kp=16) for i in range(bs)]
    src = np.stack([p.src_pts for p in ps]).astype(np.float32)
    seg = np.where(src[..., 2:3] < -1.4, FLAT_LABEL, 1).astype(np.int64)
    arrs = (src, seg, np.stack([p.src_feat for p in ps]), np.stack([p.tgt_pts for p in ps]), np.stack([p.tgt_feat for p in ps]),
            np.stack([p.gt_tform for p in ps]).astype(np.float32))
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4)}


def alternate(fns, iters, warmup):
    """{name: [ms]}: the functions in turn, `warmup` untimed rounds first"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    return {k: stats(v) for k, v in ms.items()}


def host_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message) for x in w)


def measure(dev, kind, bs, num_samples, points, iters, warmup):
    args = inputs(dev, bs, points)
    kw = dict(KW, num_samples=num_samples)
    line = dict(kind=kind, bs=bs, points=points, iters=iters, warmup=warmup, **{k: v for k, v in kw.items() if k != "flat_labels"})
    gen = {s: (lambda s=s: generate_ume_from_keypoints2(*args, selection=s, **kw)) for s in ("torch", "device")}
    try:
        out_t, out_d = gen["torch"](), gen["device"]()
    except RuntimeError as e:
        line["error"] = str(e).splitlines()[0][:200]
        return line
    line["equal"] = all(torch.equal(x, y) for x, y in zip(out_t, out_d))
    line["keypoints"] = int(out_d[2].shape[1])
    line["generator_ms"] = alternate(gen, iters, warmup)
    line["speedup_median"] = round(line["generator_ms"]["torch"]["median"] / line["generator_ms"]["device"]["median"], 3)
    line["host_syncs"] = {s: host_syncs(fn) for s, fn in gen.items()}
    # the pieces, on what the generator hands them
    src, seg, sf, tgt, tf, gt = args
    moved = (src @ gt[:, :3, :3].transpose(-1, -2) + gt[:, :3, 3][:, None]).contiguous()
    overlap = ops.ball_query(moved, tgt, K=1, radius=kw["nn_intersection_r"], return_nn=False).idx[..., 0]
    non_flat = (seg[..., 0] != FLAT_LABEL)
    cand, lengths = gk.candidates(overlap, non_flat)
    kp, rec, tested = gk.select(src, cand, lengths, kw["nn_r"], kw["max_nn"], kw["min_nn"], num_samples, return_tested=True)
    L = int(lengths.min())
    line["candidates"] = lengths.tolist()
    line["dense_found"] = rec[:, 0].tolist()
    ns = int(rec[:, 0].min())
    kpi = kp[:, :ns].contiguous()
    kpts = torch.gather(src, 1, kpi[..., None].expand(-1, -1, 3))
    ref_kpts = (kpts @ gt[:, :3, :3].transpose(-1, -2) + gt[:, :3, 3][:, None]).contiguous()
    velo_nn = ops.ball_query(kpts.contiguous(), src, K=kw["max_nn"], radius=kw["nn_r"], return_nn=True).knn
    ref_nn = ops.ball_query(ref_kpts, tgt, K=kw["max_nn"], radius=kw["nn_r"], return_nn=True).knn
    q = (velo_nn @ gt[:, :3, :3][:, None].transpose(-1, -2) + gt[:, :3, 3][:, None, None]).flatten(0, 1).contiguous()
    p = ref_nn.flatten(0, 1).contiguous()
    cand64 = cand[:, :L].long().clamp_min(0)
    pieces = {
        "device_candidates": lambda: gk.candidates(overlap, non_flat),
        "device_select": lambda: gk.select(src, cand, lengths, kw["nn_r"], kw["max_nn"], kw["min_nn"], num_samples),
        "device_ball_any": lambda: gk.ball_any(q, p, kw["nn_intersection_r"]),
        "torch_moments_of_every_candidate": lambda: ops.ume_moments(src, None, sf, kw["max_nn"], kw["nn_r"], return_count=True, kp_index=cand64),
        "torch_ball_query_per_keypoint": lambda: ops.ball_query(q, p, K=1, radius=kw["nn_intersection_r"], return_nn=False),
    }
    line["pieces_ms"] = alternate(pieces, iters, warmup)
    shares = []
    for _ in range(5):
        t = gk.select(src, cand, lengths, kw["nn_r"], kw["max_nn"], kw["min_nn"], num_samples, return_tested=True)[2]
        shares.append(float(t.sum()) / max(1, bs * L))
    line["tested_share"] = {"min": round(min(shares), 4), "max": round(max(shares), 4)}
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gt_keypoints",
                                                  "gt_keypoints_time.jsonl"))
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=45000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_keypoints_time: no HIP device visible; a time is a measurement on the GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for kind, bs, num_samples in SHAPES:
            text = json.dumps(measure(dev, kind, bs, num_samples, a.points, a.iters, a.warmup))
            print(text, flush=True)
            f.write(text + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
