"""Time the three ICP estimations and the normal estimation on the same inputs in one process; one JSON line per measurement.

    python tools/icp_time.py [--out profiles/icp_plane/icp_time.jsonl] [--iters 10] [--warmup 3]

  * `normals`: ops.estimate_normals(pts, knn=30) at 50 000 and 120 000 points of a synthetic street scene (ground disc + wall
    patches, unsnapped, sigma 0.02 m), the search (umereg_knn_points_f32) and the covariance / eigenvector kernel together.
  * `icp`: ops.icp_point_to_point, ops.icp_point_to_plane and ops.icp_plane_to_plane (epsilon 1e-3; synchronous calls, normals NOT
    included: `normals_ms` is the target's, which point to plane needs, `src_normals_ms` the source's, which plane to plane needs on
    top) from the same start, with open3d's stop rule and max_iteration = 200 --
      corner     three orthogonal 8 m patches, 2 000 points per cloud, independent samples, sigma 0.01 m, start off by
                 (0.02, -0.03, 0.05) rad and (0.15, -0.10, 0.12) m, correspondence distance 0.5 m (the case of DESIGN 4.18);
      kitti_raw  two independent 120 000-point samples of one street scene, start off by 0.5 deg about every axis and
                 (0.10, -0.08, 0.05) m, correspondence distance 0.2 m (refine_registration's).
    Per estimation: iterations, fitness, inlier_rmse, rotation / translation error against the ground truth, and `ms`.

With `--multi-scale` (default --out profiles/icp_multiscale/icp_time.jsonl) the tool measures coarse-to-fine ICP instead:
  * `voxel`: ops.voxel_down_sample at 120 000 points of the street scene for voxel 0.8 / 0.4 / 0.2 m beside ops.voxel_first_index on the
    same cloud (the thinning kernel the centroid pass is built on: its only fair yardstick); both include their one host read.
  * `icp_multi_scale`: per case (the corner at 3 000 points, kitti_raw) and per start (the tool's usual one; one 0.5 m off:
    (0.05, -0.04, 0.06) rad and (0.5, -0.4, 0.45) m), per estimation, the single-scale call (`single`; for the two normal-based
    estimations `ms` includes the normals, as the multi-scale call re-estimates them per level) against ops.icp_multi_scale with
    levels voxel 0.8 m / 0.4 m / the clouds as given, distances max(2 voxel, the case's) and the case's, 200 iterations per level
    (`multi`: iterations per level, points per level, time, final error).
  * `evaluate_pairs`: evaluate.evaluate_pairs over 8 synthetic KITTI-shaped pairs, wall clock per pair, single scale (overlapped
    IcpJob) against --icp-voxel-sizes 0.8,0.4,0 (the synchronous branch: one host wait per level per pair).

Every time is the median over `--iters` calls, each bracketed by its own pair of device events on the launch stream (the ICP calls end
in their own wait for the device), after `--warmup` calls of the same shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from umeregrobust_amd import ops       # noqa: E402


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
    return float(np.median(ms))


def euler(x):
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    T = np.eye(4)
    T[:3, :3] = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                 [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                 [-sy, cy * sx, cy * cx]]
    T[:3, 3] = x[3:6]
    return T


def corner_cloud(n, rng, sigma=0.01, size=8.0):
    uv = rng.uniform(0.0, size, (n, 2))
    face = rng.randint(0, 3, n)
    pts = np.zeros((n, 3))
    for f, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        m = face == f
        pts[m, a], pts[m, b] = uv[m, 0], uv[m, 1]
    return pts + rng.normal(0.0, sigma, (n, 3))


def street_scene(n, rng, sigma=0.02):
    """70 % ground disc (r = 50 m, z = -1.7), 30 % vertical 6 m x 6 m wall patches on an 8 m street grid; isotropic noise sigma"""
    n_g = int(0.7 * n)
    n_w = n - n_g
    rad, ang = 50.0 * np.sqrt(rng.uniform(0, 1, n_g)), rng.uniform(0, 2 * np.pi, n_g)
    ground = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n_g, -1.7)], axis=1)
    centres = np.arange(-40.0, 40.0 + 1e-6, 8.0)
    cx, cy, along = rng.choice(centres, n_w), rng.choice(centres, n_w), rng.uniform(-3.0, 3.0, n_w)
    orient = ((np.round(cx / 8.0) * 7 + np.round(cy / 8.0) * 13).astype(np.int64) % 2) == 0
    walls = np.stack([np.where(orient, cx + along, cx), np.where(orient, cy, cy + along), rng.uniform(-1.7, 4.3, n_w)], axis=1)
    return (np.concatenate([ground, walls]) + rng.normal(0.0, sigma, (n, 3)))[rng.permutation(n)]


def pair(cloud, n, seed, offset, sigma):
    """independent samples of one scene: (src f32, tgt f32, gt src -> tgt, T0 = offset @ gt)"""
    rng = np.random.RandomState(seed)
    tgt = cloud(n, rng, sigma).astype(np.float32)
    gt = euler(np.array([0.3, -0.2, 0.5, 1.0, -2.0, 0.5]))
    src = ((cloud(n, rng, sigma) - gt[:3, 3]) @ gt[:3, :3]).astype(np.float32)
    return src, tgt, gt, euler(np.array(offset)) @ gt


def errors(T, gt):
    R = T[:3, :3] @ gt[:3, :3].T
    ang = np.arctan2(np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0, (np.trace(R) - 1.0) / 2.0)
    return float(np.rad2deg(ang)), float(np.linalg.norm(T[:3, 3] - gt[:3, 3]))


CASES = {
    "corner": dict(cloud=corner_cloud, n=2000, sigma=0.01, offset=(0.02, -0.03, 0.05, 0.15, -0.10, 0.12), max_dist=0.5),
    "kitti_raw": dict(cloud=street_scene, n=120000, sigma=0.02,
                      offset=(np.deg2rad(0.5), np.deg2rad(-0.5), np.deg2rad(0.5), 0.10, -0.08, 0.05), max_dist=0.2),
}


FAR_START = (0.05, -0.04, 0.06, 0.5, -0.4, 0.45)
VOXEL_SIZES = (0.8, 0.4, 0.0)


def multi_scale(args, dev, emit):
    """the measurements of --multi-scale (see the module docstring)"""
    import time
    from types import SimpleNamespace
    pts = torch.from_numpy(street_scene(120000, np.random.RandomState(1)).astype(np.float32)).to(dev)
    line = dict(what="voxel", cloud="street_scene", n=120000, iters=args.iters, warmup=args.warmup)
    for v in (0.8, 0.4, 0.2):
        line[f"voxel_{v}"] = dict(m=int(ops.voxel_down_sample(pts, v).shape[0]),
                                  down_sample_ms=median_ms(lambda: ops.voxel_down_sample(pts, v), args.iters, args.warmup),
                                  first_index_ms=median_ms(lambda: ops.voxel_first_index(pts, v), args.iters, args.warmup))
    emit(line)
    for name, c in CASES.items():
        n = 3000 if name == "corner" else c["n"]
        dists = [max(2.0 * v, c["max_dist"]) if v else c["max_dist"] for v in VOXEL_SIZES]
        for start, offset in (("usual", c["offset"]), ("far", FAR_START)):
            src, tgt, gt, T0 = pair(c["cloud"], n, 0, offset, c["sigma"])
            s_, t_ = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
            line = dict(what="icp_multi_scale", case=name, start=start, n_src=len(src), n_tgt=len(tgt), voxel_sizes=VOXEL_SIZES,
                        max_correspondence_distances=dists, max_iteration=200, knn=args.knn, iters=args.iters, warmup=args.warmup)
            line["start_rot_deg"], line["start_trans_m"] = errors(T0, gt)
            single = dict(
                point_to_point=lambda: ops.icp_point_to_point(s_, t_, T0, c["max_dist"], 200),
                point_to_plane=lambda: ops.icp_point_to_plane(s_, t_, ops.estimate_normals(t_, args.knn), T0, c["max_dist"], 200),
                plane_to_plane=lambda: ops.icp_plane_to_plane(s_, t_, ops.estimate_normals(s_, args.knn), ops.estimate_normals(t_, args.knn),
                                                              T0, c["max_dist"], 200))
            for est, fn in single.items():
                multi = lambda: ops.icp_multi_scale(s_, t_, T0, VOXEL_SIZES, dists, [200] * 3, estimation=est, normal_knn=args.knn)  # noqa: E731
                out = {}
                for kind, call in (("single", fn), ("multi", multi)):
                    ms = median_ms(call, args.iters, args.warmup)
                    reg = call()
                    rot, trans = errors(reg.transformation, gt)
                    out[kind] = dict(iterations=reg.iterations, fitness=reg.fitness, inlier_rmse=reg.inlier_rmse, rot_err_deg=rot,
                                     trans_err_m=trans, ms=ms)
                    if kind == "multi":
                        out[kind]["iterations_per_level"] = [lv.iterations for lv in reg.levels]
                        out[kind]["points_per_level"] = [(lv.n_src, lv.n_tgt) for lv in reg.levels]
                line[est] = out
            emit(line)
    from umeregrobust_amd.evaluate import evaluate_pairs, synthetic_pairs
    from umeregrobust_amd.utils.general_utils import benchmark_config_path, update_namespace_from_yaml
    cfg = update_namespace_from_yaml(SimpleNamespace(benchmark="kitti_test"), benchmark_config_path("kitti_test"))
    cfg.batch_size = 1
    pairs = list(synthetic_pairs("kitti_test", range(8), dev))
    line = dict(what="evaluate_pairs", pairs=len(pairs), benchmark="kitti_test", voxel_sizes=VOXEL_SIZES)
    for kind, extra in (("single", {}), ("multi", dict(icp_voxel_sizes=list(VOXEL_SIZES)))):
        a = SimpleNamespace(**vars(cfg), **extra)
        res = evaluate_pairs(pairs, a, rng=np.random.RandomState(0))       # warm-up: workspaces, streams
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            res = evaluate_pairs(pairs, a, rng=np.random.RandomState(0))
        torch.cuda.synchronize()
        line[kind] = dict(ms_per_pair=1e3 * (time.perf_counter() - t0) / (3 * len(pairs)), mrte=res["mrte"], mrre=res["mrre"])
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--multi-scale", action="store_true", help="measure voxel_down_sample and icp_multi_scale instead")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--knn", type=int, default=30)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "icp_multiscale" if args.multi_scale else "icp_plane", "icp_time.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("icp_time: no HIP device visible; a time is a measurement on the GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def emit(line):
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")

        if args.multi_scale:
            return multi_scale(args, dev, emit)

        for n in (50000, 120000):
            pts = torch.from_numpy(street_scene(n, np.random.RandomState(1)).astype(np.float32)).to(dev)
            emit(dict(what="normals", cloud="street_scene", n=n, knn=args.knn, iters=args.iters, warmup=args.warmup,
                      ms=median_ms(lambda: ops.estimate_normals(pts, args.knn), args.iters, args.warmup)))
        for name, c in CASES.items():
            src, tgt, gt, T0 = pair(c["cloud"], c["n"], 0, c["offset"], c["sigma"])
            s_, t_ = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
            normals, src_normals = ops.estimate_normals(t_, args.knn), ops.estimate_normals(s_, args.knn)
            line = dict(what="icp", case=name, n_src=len(src), n_tgt=len(tgt), max_correspondence_distance=c["max_dist"],
                        max_iteration=200, knn=args.knn, iters=args.iters, warmup=args.warmup)
            line["start_rot_deg"], line["start_trans_m"] = errors(T0, gt)
            line["normals_ms"] = median_ms(lambda: ops.estimate_normals(t_, args.knn), args.iters, args.warmup)
            line["src_normals_ms"] = median_ms(lambda: ops.estimate_normals(s_, args.knn), args.iters, args.warmup)
            for est, fn in (("point_to_point", lambda: ops.icp_point_to_point(s_, t_, T0, c["max_dist"], 200)),
                            ("point_to_plane", lambda: ops.icp_point_to_plane(s_, t_, normals, T0, c["max_dist"], 200)),
                            ("plane_to_plane", lambda: ops.icp_plane_to_plane(s_, t_, src_normals, normals, T0, c["max_dist"], 200))):
                ms = median_ms(fn, args.iters, args.warmup)
                reg = fn()
                rot, trans = errors(reg.transformation, gt)
                line[est] = dict(iterations=reg.iterations, fitness=reg.fitness, inlier_rmse=reg.inlier_rmse, rot_err_deg=rot,
                                 trans_err_m=trans, ms=ms)
            emit(line)


if __name__ == "__main__":
    main()
