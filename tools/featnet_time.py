"""Time one forward pass of the HIP ResUNetSmall2 at a bench shape and print one JSON line:

  * ms per cloud for the coordinate maps (umereg_featnet_build_maps) and for the convolutions (forward - maps), device events
    over `--iters` back-to-back calls after `--warmup`;
  * useful GFLOP: 2 C_in C_out per existing kernel-map entry (1x1 layers: per row), counted from the neighbour masks the
    library built;
  * the fraction of the 157 TF fp32 matrix peak those useful flops reach in the convolution time;
  * the fraction of the issued MFMA work that was useful: a tile of TM rows issues every offset some row of it uses, for all
    its rows (conv1 and `final` run on the VALU and are left out of both counts).

    python tools/featnet_time.py [--config KT|NS] [--iters 50] [--warmup 10] [--precision f32|f16]

`--precision f16`: the f16-operand forward (include/umereg_featnet_f16.h); the line carries a "precision" key, and the peak
fraction stays relative to the fp32 matrix peak so that the two precisions' lines compare.

`--conv-mode pairs`: the pair-compacted engine (include/umereg_sparse_conv_pairs.h) in the fused forward and in `--train`; the line
carries a "conv_mode" key, and the issued MFMA work and its useful share are those of the chosen engine.

`--train`: the trainable network (ResUNetSmall2(trainable=True), train mode) at the same cloud, or with `--batch B` at B such
clouds in one call (16 KITTI-test clouds are 800 000 rows, the upper end of the reference's training shape: batch 8 x
max_pc_size 100 000).  One JSON line with ms per call of the fused eval forward (re-measured here, same session), the layer-
wise forward, forward + backward and their difference, the useful flops of the weight gradients (the forward's useful pairs:
the same products) and, with `--stats-csv`, the split of a profiled run into kernel groups:

    rocprofv3 --kernel-trace --stats -d DIR -o train -- python tools/featnet_time.py --train --profile-steps 5 [--batch B]
    python tools/featnet_time.py --train [--batch B] --stats-csv DIR/train_kernel_stats.csv >> profiles/featnet/featnet_time.jsonl

(`--profile-steps N`: N forward + backward passes and nothing else, no timing: the run to put under the profiler.)
`--train --train-precision f16`: the same with ResUNetSmall2(trainable=True, train_precision="f16") (f16 operands in the
layer-wise forward and in both gradients, include/umereg_sparse_conv_f16.h); the line carries a "train_precision" key, and
the peak fraction stays relative to the fp32 matrix peak.
`--train --fused-norm`: ResUNetSmall2(trainable=True, fused_norm=True) (batch norm, residual, ReLU and the f16 gradient scale on
include/umereg_bn_act.h); the line carries a "fused_norm" key, and the profile's `norm_act` group holds the new kernels.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from umeregrobust_amd import models                       # noqa: E402
from umeregrobust_amd.synth import synth_pair_cfg         # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
# layer -> (neighbour table: self l = l, strided l -> l+1 = 5 + l, transposed l+1 -> l = 9 + l; None = 1x1), output level
LAYER_MAPS = [(0, 0), (0, 0), (5, 1), (1, 1), (6, 2), (2, 2), (7, 3), (3, 3), (8, 4), (4, 4),
              (12, 3), (3, 3), (11, 2), (2, 2), (10, 1), (1, 1), (9, 0), (0, 0), (None, 0), (None, 0)]
VALU_LAYERS = (0, 19)


def voxel_cloud(seed, config):
    p = synth_pair_cfg(seed, config, "test")
    c = np.round(p.src_pts / 0.3).astype(np.int64)
    c = c[np.sort(np.unique(c, axis=0, return_index=True)[1])]
    c = c[np.random.default_rng(seed).permutation(len(c))]
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], axis=1).astype(np.int32)


def flop_counts(masks, levels, info, conv_mode="union"):
    """-> (useful flops per layer, issued MFMA flops per layer); issued: what the engine `conv_mode` feeds the matrix unit -- "union":
    a tile issues every offset some row of it uses, for all its rows; "pairs" (csrc/conv_pairs_plan.h): per tile of 128 rows and
    offset, the active rows rounded up to blocks of 32 (1x1 layers run the union engine's kernel in both modes)"""
    pop = np.array([bin(i).count("1") for i in range(1 << 9)], dtype=np.int64)

    def popcount(m):
        m = m.astype(np.int64)
        return pop[m & 511] + pop[(m >> 9) & 511] + pop[(m >> 18) & 511]

    useful, issued = [], []
    for i, ((mp, lo), (K, cin, cout, _, _)) in enumerate(zip(LAYER_MAPS, info)):
        rows = levels[lo]
        per = 2 * cin * cout
        if mp is None:
            useful.append(per * rows)
            entries_tile = np.ones((rows + 63) // 64, dtype=np.int64)
            tm = 64
        else:
            m = masks[mp, :rows]
            useful.append(per * int(popcount(m).sum()))
            if conv_mode == "pairs":
                tm = 128
                pad = np.zeros((-rows) % tm, dtype=m.dtype)
                act = ((np.concatenate([m, pad])[:, None] >> np.arange(27, dtype=m.dtype)) & 1).reshape(-1, tm, 27).sum(axis=1)
                issued.append(0 if i in VALU_LAYERS else per * 32 * int(((act + 31) // 32).sum()))
                continue
            tm = 64 if cout % 64 == 0 else 128
            pad = np.zeros((-rows) % tm, dtype=m.dtype)
            tiles = np.bitwise_or.reduce(np.concatenate([m, pad]).reshape(-1, tm), axis=1)
            entries_tile = popcount(tiles)
        issued.append(0 if i in VALU_LAYERS else per * tm * int(entries_tile.sum()))
    return useful, issued


# kernel groups of a profiled training run (rocprofv3 kernel_stats.csv, by kernel name)
GROUPS = (("conv_forward_and_input_gradient", ("fn_conv_kernel", "fn_conv1_kernel", "fn_conv_f16_kernel", "cp_conv_kernel", "cp_conv_f16_kernel")),
          ("weight_gradient", ("wg_mfma_kernel", "wg_c1_kernel", "wg_reduce_kernel", "wg_f16_kernel")),
          ("repack", ("wg_repack_kernel",)),
          ("norm_act", ("bn_stats_kernel", "bn_fwd_apply_kernel", "bn_bwd_reduce_kernel", "bn_bwd_apply_kernel", "gs_partial_kernel",
                        "gs_finish_kernel")))


def kernel_groups(path, steps):
    """rocprofv3 kernel_stats.csv of `steps` forward + backward passes -> ms per pass by kernel group (anything that is not
    one of the library's kernels is a torch op)"""
    import csv
    ms = {g: 0.0 for g, _ in GROUPS}
    ms["maps"] = ms["torch_ops"] = 0.0          # (maps: every other kernel of the library)
    top = []
    for row in csv.DictReader(open(path)):
        t = float(row["TotalDurationNs"]) / 1e6 / steps
        for g, keys in GROUPS:
            if "umereg::" in row["Name"] and any(k in row["Name"] for k in keys):
                ms[g] += t
                break
        else:
            ms["torch_ops" if "umereg::" not in row["Name"] else "maps"] += t
        top.append((t, row["Name"][:60]))
    return {k: round(v, 4) for k, v in ms.items()}, [f"{t:.3f} ms {nm}" for t, nm in sorted(top, reverse=True)[:4]]


def train_mode(a, dev):
    from umeregrobust_amd.sparse import SparseTensor
    clouds = []
    for b in range(a.batch):
        c = voxel_cloud(a.seed + b, a.config)
        c[:, 0] = b
        clouds.append(c)
    coords = torch.from_numpy(np.concatenate(clouds)).to(dev)
    n = coords.shape[0]
    torch.manual_seed(a.seed)
    m = models.ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, train_precision=a.train_precision, fused_norm=a.fused_norm,
                             conv_mode=a.conv_mode).to(dev)
    st = SparseTensor(torch.ones(n, 1, device=dev), coordinates=coords)
    st._batch_size = a.batch
    G = torch.randn(n, 32, device=dev)

    def fused():
        with torch.no_grad():
            m(st)

    def forward():
        return m(st).F

    def step():
        m.zero_grad(set_to_none=True)
        (forward() * G).sum().backward()

    if a.profile_steps:
        m.train()
        for _ in range(a.profile_steps):
            step()
        torch.cuda.synchronize()
        return

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    m.eval()
    ms_fused = timed(fused)
    m.train()
    ms_fwd = timed(forward)
    ms_step = timed(step)
    # useful flops of the weight gradients = those of the forward's 27-offset layers: one product per (pair, C_in, C_out)
    ws = torch.empty(models.workspace_bytes(n, a.batch), dtype=torch.uint8, device=dev)
    status = torch.empty(models.N_STATUS, dtype=torch.int32, device=dev)
    models.build_maps_raw(coords, a.batch, ws, status)
    levels = models.check_status(status)
    masks = models.buffer_view(ws, n, a.batch, models.BUF_MASKS, n, torch.int32)
    masks = masks.reshape(-1)[:13 * n].cpu().numpy().view(np.uint32).reshape(13, n)
    useful, _ = flop_counts(masks, levels, models.layer_info())
    wgrad_flop = float(sum(u for (mp, _), u in zip(LAYER_MAPS, useful) if mp is not None))
    line = dict(tool="featnet_time", mode="train", conv_mode=a.conv_mode, train_precision=a.train_precision, fused_norm=bool(a.fused_norm), config=a.config, batch=a.batch, n=n, levels=levels, iters=a.iters,
                ms_per_call=dict(fused_eval_forward=round(ms_fused, 4), layerwise_forward=round(ms_fwd, 4),
                                 forward_backward=round(ms_step, 4), backward=round(ms_step - ms_fwd, 4)),
                wgrad_useful_gflop=round(wgrad_flop / 1e9, 3))
    if a.stats_csv:
        groups, top = kernel_groups(a.stats_csv, a.stats_steps)
        line["profiled_ms_per_pass"] = groups
        line["profiled_top_kernels"] = top
        wg = groups["weight_gradient"]
        line["wgrad_useful_tflops"] = round(wgrad_flop / (wg * 1e-3) / 1e12, 2)
        line["wgrad_frac_fp32_matrix_peak"] = round(wgrad_flop / (wg * 1e-3) / PEAK_FP32_MATRIX, 4)
    print(json.dumps(line))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--train", action="store_true", help="time the trainable network's forward and backward")
    ap.add_argument("--batch", type=int, default=1, help="--train: clouds per call")
    ap.add_argument("--profile-steps", type=int, default=0, help="--train: run N forward + backward passes only (for the profiler)")
    ap.add_argument("--stats-csv", default=None, help="--train: rocprofv3 kernel_stats.csv of a --profile-steps run to fold in")
    ap.add_argument("--stats-steps", type=int, default=5, help="--train: the --profile-steps of that run")
    ap.add_argument("--train-precision", default="f32", choices=list(models.PRECISIONS),
                    help="--train: operand precision of the layer-wise forward and backward")
    ap.add_argument("--fused-norm", action="store_true", help="--train: batch norm, residual and ReLU on the fused HIP kernels")
    ap.add_argument("--conv-mode", default="union", choices=list(models.CONV_MODES),
                    help="engine of the 27-offset convolutions (pairs: include/umereg_sparse_conv_pairs.h), fused forward and --train alike")
    ap.add_argument("--config", default="KT", choices=["KT", "NS"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="f32", choices=list(models.PRECISIONS), help="operand precision of the fused forward")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "featnet_time measures on the GPU"
    dev = torch.device("cuda:0")
    if a.train:
        return train_mode(a, dev)
    torch.manual_seed(a.seed)
    m = models.ResUNetSmall2(in_channels=1, out_channels=32, conv_mode=a.conv_mode)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5), mod.bias.normal_(0, 0.1), mod.running_mean.normal_(0, 0.1), mod.running_var.uniform_(0.5, 2)
    m = m.eval().to(dev)
    coords = torch.from_numpy(voxel_cloud(a.seed, a.config)).to(dev)
    n = coords.shape[0]
    feat = torch.ones(n, 1, device=dev)
    params = m.packed_parameters()
    ws = torch.empty(models.workspace_bytes(n, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(n, 32, device=dev)
    status = torch.empty(models.N_STATUS, dtype=torch.int32, device=dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    ms_maps = timed(lambda: models.build_maps_raw(coords, 1, ws, status))
    ms_total = timed(lambda: models.forward_raw(coords, feat, 1, params, ws, out, status, a.precision, a.conv_mode))
    levels = models.check_status(status)
    masks = models.buffer_view(ws, n, 1, models.BUF_MASKS, n, torch.int32)      # [13][n] words, viewed as [n, 13]
    masks = masks.reshape(-1)[:13 * n].cpu().numpy().view(np.uint32).reshape(13, n)
    info = models.layer_info()
    useful, issued = flop_counts(masks, levels, info, a.conv_mode)
    ms_conv = ms_total - ms_maps
    useful_total = float(sum(useful))
    mfma_useful = float(sum(u for i, u in enumerate(useful) if i not in VALU_LAYERS))
    names = [name.split(".")[0] if name.startswith("block") and ".conv1" in name else name for name, _ in models.LAYERS]
    line = dict(tool="featnet_time", precision=a.precision, conv_mode=a.conv_mode, config=a.config, n=n, levels=levels, iters=a.iters,
                ms_per_cloud=dict(maps=round(ms_maps, 4), conv=round(ms_conv, 4), total=round(ms_total, 4)),
                useful_gflop=round(useful_total / 1e9, 3),
                useful_tflops_in_conv=round(useful_total / (ms_conv * 1e-3) / 1e12, 2),
                frac_fp32_matrix_peak=round(useful_total / (ms_conv * 1e-3) / PEAK_FP32_MATRIX, 4),
                mfma_issued_gflop=round(sum(issued) / 1e9, 3), mfma_useful_frac=round(mfma_useful / sum(issued), 4),
                useful_gflop_per_layer={nm: round(u / 1e9, 3) for nm, u in zip(names, useful)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
