"""Time the sampling equalizer, per stage and as the whole call, in one process; one JSON line per measurement.

    python tools/equalizer_time.py [--out profiles/equalizer/equalize_time.jsonl] [--iters 20] [--warmup 5]

Two shapes, both to M = 125 000 samples with the defaults (knn 16, max_radius 1 m): n = 120 000 and n = 30 000 points of
`synth.synth_scene` (ground disc + wall patches of a street scene, snapped to a 0.3 m lattice).  Per shape:
  surfels   equalizer.surfels: umereg_knn_points_f32 on the cloud itself + eq_surfel_kernel
  sample    equalizer.sample: eq_scan_kernel + eq_sample_kernel, and the one word read back
  project   equalizer.project: launch_prep (the grid) + eq_project_kernel
  cloud     equalizer.equalize_cloud: the three in one native call, and the one word read back
and for the projection what it works on: the mean and the largest number of neighbours inside a sample's support (nb_count), from which
`project_ns_per_neighbour` = time / (samples x mean neighbours x 2 passes): every neighbour is one 16-byte table entry gathered twice.
The candidates a sample's cell walk visits beyond its neighbours are not counted here.

Every time is the median over `--iters` calls, each bracketed by its own pair of device events on the launch stream, after
`--warmup` calls of the same shape.  There is no parent path and no NKSR figure to compare against: these are this library's numbers."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from umeregrobust_amd import equalizer, synth       # noqa: E402


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "equalizer", "equalize_time.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-points", type=int, default=equalizer.NUM_POINTS)
    ap.add_argument("--sizes", type=int, nargs="+", default=[120000, 30000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("equalizer_time: no HIP device visible; a time is a measurement on the GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    M, knn, rmax = args.num_points, equalizer.DEFAULT_KNN, equalizer.DEFAULT_RADIUS
    with open(args.out, "a") as f:
        for n in args.sizes:
            pts = torch.from_numpy(synth.synth_scene(np.random.RandomState(1), n).astype(np.float32)).to(dev)
            normals, r2, q = equalizer.surfels(pts, knn, rmax)
            samples, src, rho2 = equalizer.sample(pts, normals, r2, q, M, knn)
            _, cnt = equalizer.project(samples, rho2, pts, return_count=True)
            line = dict(what="equalize", cloud="synth_scene", n=n, num_points=M, knn=knn, max_radius=rmax, iters=args.iters, warmup=args.warmup,
                        device=torch.cuda.get_device_name(dev), zero_area_points=int((q == 0).sum()),
                        capped_supports=int((r2 >= rmax * rmax).sum()), distinct_sources=int(torch.unique(src).numel()),
                        neighbours_mean=float(cnt.float().mean()), neighbours_max=int(cnt.max()))
            for name, fn in (("surfels", lambda: equalizer.surfels(pts, knn, rmax)),
                             ("sample", lambda: equalizer.sample(pts, normals, r2, q, M, knn)),
                             ("project", lambda: equalizer.project(samples, rho2, pts)),
                             ("cloud", lambda: equalizer.equalize_cloud(pts, M, knn, rmax)),
                             ("cloud_no_project", lambda: equalizer.equalize_cloud(pts, M, knn, rmax, project=False))):
                med, lo, hi = median_ms(fn, args.iters, args.warmup)
                line[name + "_ms"], line[name + "_ms_min_max"] = med, [lo, hi]
            line["project_ns_per_neighbour"] = 1e6 * line["project_ms"] / (M * max(line["neighbours_mean"], 1e-9) * 2)
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")


if __name__ == "__main__":
    main()
