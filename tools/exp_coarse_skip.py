"""Chain-level evidence for the coarse matcher's early exit: python tools/exp_coarse_skip.py [--config KT] [--hard] [--reps 200] [--stats]

Time of one a1..a5 chain (ops.PairMatchGraph replayed back to back on one stream, HIP events around the whole run) on a synthetic pair
of a benchmark shape, with the library in the tree or another build of it (ALTLIB=<file under tools/>, as tools/bench_altlib.py).
--stats: the library must be a -DUMEREG_COARSE_STATS=1 build (its matcher scratch ends in four 64-bit counters): one replay over a
zeroed workspace, then tiles visited / stopped at the first / at the second test and candidates per row.
A/B builds: UMEREG_COARSE_EXIT = 0 (no test), 1, 2, 3 (both), +4 = the second column's MFMAs issued before the first test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
if os.environ.get("ALTLIB"):
    import umeregrobust_amd._build as _b
    _b.LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.environ["ALTLIB"])
    import umeregrobust_amd._lib as _L
    _L.LIB_PATH = _b.LIB_PATH

import numpy as np   # noqa: E402
import torch         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="KT", choices=["K1", "KT", "NS", "SY"])
    ap.add_argument("--kind", default="test", choices=["test", "rot"])
    ap.add_argument("--hard", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--splits", type=int, default=0, help="umereg_match_opts.splits (0 = the plan's own)")
    a = ap.parse_args()
    from umeregrobust_amd import _lib, ops
    from umeregrobust_amd.synth import synth_pair_cfg
    dev = torch.device("cuda:0")
    p = synth_pair_cfg(a.seed, a.config, kind=a.kind, hard=a.hard)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    pts = torch.stack([t(p.src_pts), t(p.tgt_pts)])
    feat = torch.stack([t(p.src_feat), t(p.tgt_feat)])
    kp = torch.stack([t(p.src_inds), t(p.tgt_inds)])
    N, n = pts.shape[1], kp.shape[1]
    g = ops.PairMatchGraph(pts, feat, kp, 750, 5.0, 0.05, opts=ops.MatchOpts(splits=a.splits) if a.splits else None)
    out = dict(config=a.config, kind=a.kind, hard=a.hard, N=N, n_kp=n, splits=a.splits, lib=os.environ.get("ALTLIB", "product"))
    if a.stats:
        lib = _lib.load()
        up = lambda v, k: (v + k - 1) // k * k   # noqa: E731
        off = up(lib.umereg_ume_moments_workspace_bytes(2, N), 256) + up(n, 128) * 512 + up(n, 32) * 512 \
            + lib.umereg_ume_match_q_scratch_bytes_ex(n, n, _lib.opts_ptr(g.opts)) - 256
        g.ws.zero_()
        g.launch()
        torch.cuda.synchronize()
        c = g.ws[off:off + 32].cpu().numpy().view(np.uint64)
        tiles = int(c[0])
        out.update(wave_tiles=tiles, stopped_after_col0=round(int(c[1]) / max(tiles, 1), 4),
                   stopped_after_col01=round((int(c[1]) + int(c[2])) / max(tiles, 1), 4),
                   run_filter=round(1.0 - (int(c[1]) + int(c[2])) / max(tiles, 1), 4),
                   # a tile stopped after column 0 has done a quarter of its MFMAs and squares, after columns 0-1 a half
                   mfma_and_squares_left=round(1.0 - (0.75 * int(c[1]) + 0.5 * int(c[2])) / max(tiles, 1), 4),
                   candidates_per_row=round(int(c[3]) / n, 2))
    else:
        for _ in range(10):
            g.launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                g.launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(round(e0.elapsed_time(e1) / a.reps * 1e3, 1))
        out.update(chain_us=times)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
