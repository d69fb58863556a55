"""Time the Hungarian matching of the two call sites on the host, as the library runs it by default, and on the device
(ops.linear_sum_assignment), on subspace distances of `synth` keypoints with 30 % outlier keypoints:

  * 8 x 1000 x 1000: the validation batch of the training driver (calc_inliear_ratio, eval_num_kpts = 1000, batch 8);
  * 1 x 2500^2, 1 x 5000^2, 1 x 10000^2: evaluate's hungarian_matching_flag (ume_n_samples square, or 10 000 with
    filter_by_ume_dist_cond).

Per shape one JSON line, printed and appended to --out (default profiles/assign/assign_time.jsonl):
  host_ms      device D -> .cpu() -> scipy per matrix, one after the other -> upload; a host clock around work that ends in a
               stream synchronise
  device_ms    the op, D where it lies -> (rows, cols) on the device, status read included; device events, then a synchronise;
               the least and the median of --iters runs (one run from 5000 up)
  steps, matched_share, us_per_step
               Dijkstra steps and the share of rows the start matched, as the kernel counts them into its workspace (summed over
               the batch); us_per_step = device time of the raw call / steps of the matrix with the most steps: an upper bound,
               the start's kernels are inside
  same_assignment, total_diff
               the device's assignment against scipy's

    python tools/assign_time.py [--shapes 8x1000,1x2500,1x5000,1x10000] [--iters 3] [--host-max-n 10000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from umeregrobust_amd import assign, ops              # noqa: E402
from umeregrobust_amd.synth import synth_pair         # noqa: E402

OUTLIERS = 0.3


def distances(seed, n, dev):
    """[n, n] subspace distances between n source keypoints and n target keypoints, 70 % of which are the sources' twins"""
    p = synth_pair(seed, N=max(50000, 5 * n) if n > 1000 else 20000, n_kp=n)
    n_in = n - int(round(OUTLIERS * n))
    tgt_inds = np.concatenate([p.tgt_twin_of_src[p.src_inds[:n_in]], p.tgt_inds[:n - n_in]])
    tgt_inds = tgt_inds[np.random.RandomState(seed).permutation(n)]
    t = lambda a: torch.from_numpy(a).to(dev)[None]                            # noqa: E731
    F_src = ops.ume_moments(t(p.src_pts), None, t(p.src_feat), 750, 5.0, kp_index=t(p.src_inds))
    F_tgt = ops.ume_moments(t(p.tgt_pts), None, t(p.tgt_feat), 750, 5.0, kp_index=t(tgt_inds))
    return ops.ume_cdist(F_src, F_tgt)[0]


def host_path(D):
    """what calc_inliear_ratio and evaluate._phase_a do by default"""
    cost = D.cpu().numpy()
    pairs = np.stack([np.stack(scipy_lsa(c), axis=-1) for c in cost])
    return torch.from_numpy(pairs).to(device=D.device, dtype=torch.long)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="8x1000,1x2500,1x5000,1x10000", help="comma-separated BATCHxN")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--host-max-n", type=int, default=10000, help="the host path is not timed above this size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "assign",
                                                  "assign_time.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "assign_time measures on the GPU"
    dev = torch.device("cuda:0")
    ops.linear_sum_assignment(torch.rand(2, 64, 64, device=dev))               # code objects loaded before anything is timed
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        b, n = (int(x) for x in shape.split("x"))
        D = torch.stack([distances(a.seed + k, n, dev) for k in range(b)]).contiguous()
        torch.cuda.synchronize()
        line = dict(tool="assign_time", batch=b, n=n, costs=f"subspace distances, {int(100 * OUTLIERS)} % outlier keypoints")
        ref = None
        if n <= a.host_max_n:
            t0 = time.perf_counter()
            ref = host_path(D)
            torch.cuda.synchronize()
            line["host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        else:
            line["host_ms"] = None                                              # not measured
        iters = a.iters if n < 5000 else 1
        ms, ms_raw = [], []
        for _ in range(iters):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            rows, cols = ops.linear_sum_assignment(D)
            e[1].record()
            pairs, total, status, stats = assign.solve(D, with_stats=True)
            e[2].record()
            torch.cuda.synchronize()
            ms.append(e[0].elapsed_time(e[1]))
            ms_raw.append(e[1].elapsed_time(e[2]))
        stats = stats.cpu().numpy()
        line["device_ms"] = dict(least=round(min(ms), 3), median=round(float(np.median(ms)), 3), runs=iters)
        line["device_raw_call_ms"] = round(min(ms_raw), 3)
        line["steps"] = int(stats[:, 1].sum())
        line["steps_per_matrix"] = [int(s) for s in stats[:, 1]]
        line["matched_share"] = round(float(stats[:, 0].sum()) / (b * n), 4)
        line["us_per_step"] = round(min(ms_raw) * 1e3 / max(int(stats[:, 1].max()), 1), 3)
        if ref is not None:
            line["speedup"] = round(line["host_ms"] / min(ms), 2)
            line["same_assignment"] = bool(torch.equal(ref[..., 1], cols))
            Dh, refh, colh = D.cpu().numpy().astype(np.float64), ref.cpu().numpy(), cols.cpu().numpy()
            line["total_diff"] = max(abs(float(np.cumsum(Dh[k, refh[k, :, 0], refh[k, :, 1]])[-1]) - float(np.cumsum(Dh[k, np.arange(n), colh[k]])[-1]))
                                     for k in range(b))
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del D


if __name__ == "__main__":
    main()
