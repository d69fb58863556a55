"""Where the making of one pair-cache item from raw scans spends its time, at SemanticKITTI's size: a synthetic pair of two scans of
~120 000 points each (`synth_scene`, every voxel hit twice, label words with instance halves, 10 % unlabelled), written as `.bin` /
`.label` files and taken through the path of `SemanticKITTIDataset` without a cache and `write_cached_pair`.

    python tools/raw_item_time.py [--points 120000] [--reps 7] [--warmup 3] [--out profiles/raw/raw_item_time.jsonl]

One JSON line (appended to --out): per phase the median over --reps items, after --warmup, of
  * "wall_ms": host clock around the phase, with a device synchronisation at both ends (so a phase's kernels are charged to it and
    not to the next read of a count);
  * "device_ms" (device phases only): elapsed time between two events recorded on the stream around the same calls.
Phases: file_read (numpy, both scans and labels), upload (host -> device copies of scans and label words), prep (`prepare_cloud`
on device tensors: `umereg_scan_prep_f32` and the read of its count), thinning, grid_points, matches (the three parts of
`prepare_pair`; matches includes src_pts_tform), to_host, pickle_write (`write_cached_pair`).  "item_wall_ms" is one whole item
without the synchronisations in between.  Sizes after every stage are in the line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from contextlib import nullcontext

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VOXEL = 0.3


def synth_scan_files(root, points, seed=0):
    """two scans of one scene, the second moved by T; -> ([(bin path, label path)] * 2, T, lut)"""
    from umeregrobust_amd.synth import synth_scene
    rng = np.random.RandomState(seed)
    scene = synth_scene(rng, int(0.625 * points), VOXEL) + 0.5 * VOXEL
    a = np.deg2rad(6.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [4.0, -1.5, 0.1]
    lut = (np.arange(260) % 20).astype(np.int32)             # a stand-in for a learning map: 260 keys, every 20th unlabelled
    paths = []
    for f in range(2):
        p = scene[rng.permutation(len(scene))[:points // 2]]
        p = np.concatenate([p, p]) + rng.uniform(-0.4 * VOXEL, 0.4 * VOXEL, (2 * len(p), 3))
        if f == 1:
            p = p @ T[:3, :3].T + T[:3, 3]
        p = p[rng.permutation(len(p))]
        scan = np.concatenate([p, rng.uniform(0, 1, (len(p), 1))], axis=1).astype(np.float32)
        sem = np.where(rng.uniform(size=len(p)) < 0.1, 0, rng.randint(1, 260, len(p)))
        words = sem.astype(np.uint32) | (rng.randint(1, 1 << 16, len(p)).astype(np.uint32) << 16)
        paths.append((os.path.join(root, f"{f:06d}.bin"), os.path.join(root, f"{f:06d}.label")))
        scan.tofile(paths[-1][0])
        words.tofile(paths[-1][1])
    return paths, T.astype(np.float32), lut


class Clock:
    def __init__(self):
        self.wall, self.device = {}, {}

    def phase(self, name, on_device=True):
        clock = self

        class _Phase:
            def __enter__(self):
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
                if on_device:
                    self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    self.a.record()

            def __exit__(self, *exc):
                if on_device:
                    self.b.record()
                torch.cuda.synchronize()
                clock.wall.setdefault(name, []).append((time.perf_counter() - self.t0) * 1e3)
                if on_device:
                    clock.device.setdefault(name, []).append(self.a.elapsed_time(self.b))
        return _Phase()

    def medians(self, items, skip):
        """per phase the median over items of the phase's SUM within one item (a phase entered once per cloud counts twice)"""
        def per_item(v):
            k = len(v) // items
            return [sum(v[i * k:(i + 1) * k]) for i in range(items)][skip:]
        return ({k: round(statistics.median(per_item(v)), 4) for k, v in self.wall.items()},
                {k: round(statistics.median(per_item(v)), 4) for k, v in self.device.items()})


def one_item(paths, T, lut_dev, dev, clock, out_path):
    from umeregrobust_amd import raw_scan
    from umeregrobust_amd.datasets.kitti_dataset import write_cached_pair
    phase = clock.phase if clock else (lambda name, on_device=True: nullcontext())
    with phase("file_read", on_device=False):
        host = [(raw_scan.read_kitti_scan(b), None) for b, _ in paths]
        host = [(s, raw_scan.read_kitti_label(l, len(s))) for (s, _), (_, l) in zip(host, paths)]
    with phase("upload"):
        up = [(torch.from_numpy(s).to(dev), torch.from_numpy(w.view(np.int32)).to(dev)) for s, w in host]
    with phase("prep"):
        clouds = [raw_scan.prepare_cloud(s, w, lut=lut_dev, sem16=True, device=dev) for s, w in up]
    item = raw_scan.prepare_pair(clouds[0], clouds[1], T, VOXEL, phase=phase)
    with phase("pickle_write", on_device=False):
        write_cached_pair(out_path, item)
    return [len(s) for s, _ in host], [len(c[0]) for c in clouds], item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raw", "raw_item_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp()
    paths, T, lut = synth_scan_files(tmp, a.points)
    lut_dev = torch.from_numpy(lut).to(dev)
    out_path = os.path.join(tmp, "cache", "000000_000001.pickle")
    clock = Clock()
    items = a.warmup + a.reps
    for _ in range(items):
        n_scan, n_kept, item = one_item(paths, T, lut_dev, dev, clock, out_path)
    whole = []
    for _ in range(a.reps):                                   # the same item without the synchronisations between the phases
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_item(paths, T, lut_dev, dev, None, out_path)
        whole.append((time.perf_counter() - t0) * 1e3)
    wall, device = clock.medians(items, a.warmup)
    line = {"kind": "raw_item", "points_per_scan": n_scan, "after_prep": n_kept, "after_thinning": [len(item[0]), len(item[3])],
            "matches": len(item[8]), "pickle_bytes": os.path.getsize(out_path), "reps": a.reps, "warmup": a.warmup, "wall_ms": wall,
            "device_ms": device, "item_wall_ms": round(statistics.median(whole), 4), "item_wall_min_ms": round(min(whole), 4)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
