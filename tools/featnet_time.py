"""Time one forward pass of the HIP ResUNetSmall2 at a bench shape and print one JSON line:

  * ms per cloud for the coordinate maps (umereg_featnet_build_maps) and for the convolutions (forward - maps), device events
    over `--iters` back-to-back calls after `--warmup`;
  * useful GFLOP: 2 C_in C_out per existing kernel-map entry (1x1 layers: per row), counted from the neighbour masks the
    library built;
  * the fraction of the 157 TF fp32 matrix peak those useful flops reach in the convolution time;
  * the fraction of the issued MFMA work that was useful: a tile of TM rows issues every offset some row of it uses, for all
    its rows (conv1 and `final` run on the VALU and are left out of both counts).

    python tools/featnet_time.py [--config KT|NS] [--iters 50] [--warmup 10]
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


def flop_counts(masks, levels, info):
    """-> (useful flops per layer, issued MFMA flops per layer)"""
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
            tm = 64 if cout % 64 == 0 else 128
            pad = np.zeros((-rows) % tm, dtype=m.dtype)
            tiles = np.bitwise_or.reduce(np.concatenate([m, pad]).reshape(-1, tm), axis=1)
            entries_tile = popcount(tiles)
        issued.append(0 if i in VALU_LAYERS else per * tm * int(entries_tile.sum()))
    return useful, issued


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="KT", choices=["KT", "NS"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "featnet_time measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    m = models.ResUNetSmall2(in_channels=1, out_channels=32)
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
    ms_total = timed(lambda: models.forward_raw(coords, feat, 1, params, ws, out, status))
    levels = models.check_status(status)
    masks = models.buffer_view(ws, n, 1, models.BUF_MASKS, n, torch.int32)      # [13][n] words, viewed as [n, 13]
    masks = masks.reshape(-1)[:13 * n].cpu().numpy().view(np.uint32).reshape(13, n)
    info = models.layer_info()
    useful, issued = flop_counts(masks, levels, info)
    ms_conv = ms_total - ms_maps
    useful_total = float(sum(useful))
    mfma_useful = float(sum(u for i, u in enumerate(useful) if i not in VALU_LAYERS))
    names = [name.split(".")[0] if name.startswith("block") and ".conv1" in name else name for name, _ in models.LAYERS]
    line = dict(tool="featnet_time", config=a.config, n=n, levels=levels, iters=a.iters,
                ms_per_cloud=dict(maps=round(ms_maps, 4), conv=round(ms_conv, 4), total=round(ms_total, 4)),
                useful_gflop=round(useful_total / 1e9, 3),
                useful_tflops_in_conv=round(useful_total / (ms_conv * 1e-3) / 1e12, 2),
                frac_fp32_matrix_peak=round(useful_total / (ms_conv * 1e-3) / PEAK_FP32_MATRIX, 4),
                mfma_issued_gflop=round(sum(issued) / 1e9, 3), mfma_useful_frac=round(mfma_useful / sum(issued), 4),
                useful_gflop_per_layer={nm: round(u / 1e9, 3) for nm, u in zip(names, useful)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
