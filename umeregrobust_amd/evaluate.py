"""Counterpart of the hot-path part of the reference's evaluate.py.

`my_ume_generation` keeps the reference signature (evaluate.py:50); the per-pair loop between feature extraction and hypothesis
selection (evaluate.py:195-254: `register_pair`, `RegistrationPipeline`) lives in pipeline.py and is imported back under its names.
"""
import contextlib

import numpy as np
import torch

from . import icp_gicp, icp_multiscale, icp_plane, ops, streams as _streams
from .host_rng import choice_uniform_noreplace
from .pipeline import (PairBatch, PairResult, RegistrationPipeline, _draw_keypoints, _draw_keypoints_host, _index_tensor,  # noqa: F401
                       _phase_a, _phase_b, _PinnedRing, _ring, _to_host, phase_a_route, register_pair)
from .utils.eval_utils import relative_rotation_error  # noqa: F401
from .utils.loc_utils import (FeatureCorrelator, batch_estimate_transform_ume_old, ume_cdist,  # noqa: F401
                               ume_kp_layer)


def pc_fcht(pc1_pts, pc2_pts, pc1_feat, pc2_feat, rtume_hypotises, gt_tform, corr_sigma, args, timing=None, return_tform=False):
    """reference evaluate.py:20-47: pick the hypothesis with the highest feature correlation and report
    its error.  Returns (R_err [bs], t_err [bs], R_hat [bs,3,3], t_hat [bs,3]); errors stay on the device.
    return_tform: additionally the selected 4 x 4 transforms [bs,4,4] (contiguous, on the device: the ICP can start from them
    without a host read, see ops.icp_point_to_point)."""
    hypotisis_matcher = FeatureCorrelator(sigma=corr_sigma, batch=args.corr_batch_size, n_hypotheses=10)
    tform_hat = []
    for b_idx in range(args.batch_size):
        tt = hypotisis_matcher.feature_corr_hypothesis_test(
            source_pc=pc1_pts[b_idx][None], target_pc=pc2_pts[b_idx][None], source_feat=pc1_feat[b_idx][None],
            target_feat=pc2_feat[b_idx][None], T_kp=rtume_hypotises[b_idx], src_norm=None, tgt_norm=None, timing=timing)
        tform_hat.append(tt[None])
    tform_hat = torch.cat(tform_hat, dim=0)
    R_hat = tform_hat[:, :3, :3]
    t_hat = tform_hat[:, :3, 3]
    R_gt = gt_tform[:, :3, :3]
    t_gt = gt_tform[:, :3, 3]
    R_err = relative_rotation_error(R_hat.contiguous(), R_gt.contiguous())
    t_err = (t_hat - t_gt).norm(dim=-1)
    if return_tform:
        return R_err, t_err, R_hat, t_hat, tform_hat
    return R_err, t_err, R_hat, t_hat


def prepare_selection(src_pts_raw, tgt_pts_raw, args):
    """The device-only first step of select_hypothesis (voxel thinning of the raw clouds, evaluate.py:261-264), launched ahead of time:
    it depends on the raw clouds alone, so a loop can enqueue it BEFORE the named path of the same pair and find the voxel counts
    waiting when the hypothesis selection starts (one host synchronisation less per pair).  Consumes no random numbers.
    -> handle for select_hypothesis(prepared=...), or None when the inputs do not qualify (host tensors, other dtypes)."""
    if src_pts_raw.is_cuda and tgt_pts_raw.is_cuda and src_pts_raw.dtype == torch.float32 and tgt_pts_raw.dtype == torch.float32 \
            and src_pts_raw.dim() == 2 and tgt_pts_raw.dim() == 2:
        return ops.VoxelThinning(src_pts_raw.contiguous(), args.corr_ds, tgt_pts_raw.contiguous(), 0.3)
    return None


def sparse_quantize(coordinates, return_index=True, quantization_size=1.0):
    """MinkowskiEngine.utils.sparse_quantize as used at reference evaluate.py:261-264: one representative per
    occupied voxel of edge `quantization_size`.  -> (voxel coords int32 [m,3], index int64 [m]).
    MinkowskiEngine is not installable here (parity unpinned): this restates its documented behaviour --
    floor(coordinates / quantization_size), the FIRST point of every voxel, in order of first appearance.
    Device tensors go through the native kernel (`umereg_voxel_first_index_f32`: hash table + atomicMin, no sort); host
    tensors through the torch form below (the same rule; CPU-side callers such as dataset preprocessing)."""
    if coordinates.is_cuda and coordinates.dtype == torch.float32 and coordinates.dim() == 2 and coordinates.shape[1] == 3:
        inds = ops.voxel_first_index(coordinates, quantization_size)
        if not return_index:
            return torch.floor(coordinates[inds] / quantization_size).to(torch.int32)
        return torch.floor(coordinates[inds] / quantization_size).to(torch.int32), inds
    q = torch.floor(coordinates / quantization_size).to(torch.int64)
    qmin = q.min(dim=0).values
    span = (q.max(dim=0).values - qmin + 1)
    rel = q - qmin
    key = (rel[:, 0] * span[1] + rel[:, 1]) * span[2] + rel[:, 2]
    skey, perm = torch.sort(key, stable=True)
    first = torch.ones_like(skey, dtype=torch.bool)
    first[1:] = skey[1:] != skey[:-1]
    inds = torch.sort(perm[first]).values
    coords = q[inds].to(torch.int32)
    return (coords, inds) if return_index else coords


def select_hypothesis(src_pts_raw, tgt_pts_raw, src_pts, tgt_pts, src_feat, tgt_feat, rtume_tform, gt_tform, args,
                      rng=np.random, timing=None, prepared=None, return_tform=False):
    """reference evaluate.py:258-296 (one loop iteration): voxel-thin the RAW clouds (corr_ds / 0.3 m), give every
    kept point the feature of its nearest network point (K=1), random-subsample to pc_corr_max_size with the host
    RNG and let the FeatureCorrelator pick one RTUME hypothesis.
    src_pts_raw [n,3], tgt_pts_raw [m,3]; src_pts/tgt_pts [1,N,3] with src_feat/tgt_feat [1,N,32];
    rtume_tform [1,M,4,4]; gt_tform [4,4].  -> (R_err, t_err, R_hat_corr [1,3,3], t_hat_corr [1,3])."""
    dev = src_pts.device
    src_pts_raw, tgt_pts_raw = src_pts_raw.to(dev), tgt_pts_raw.to(dev)
    if prepared is not None:
        src_inds, tgt_inds = prepared.result()               # (launched by prepare_selection, ahead of the named path)
    elif src_pts_raw.is_cuda and src_pts_raw.dtype == torch.float32 and tgt_pts_raw.dtype == torch.float32:
        # both clouds behind one host read of the two voxel counts (the voxel coordinates themselves are not used, :261-264)
        src_inds, tgt_inds = ops.voxel_first_index(src_pts_raw.contiguous(), args.corr_ds, tgt_pts_raw.contiguous(), 0.3)
    else:
        _, src_inds = sparse_quantize(src_pts_raw, return_index=True, quantization_size=args.corr_ds)       # :261-262
        _, tgt_inds = sparse_quantize(tgt_pts_raw, return_index=True, quantization_size=0.3)                # :263-264
    gt_tform = gt_tform[None].to(dev)
    # The reference transfers features to EVERY kept raw point (K=1 search, :272-275) and sub-samples afterwards (:278-285).
    # A point's feature does not depend on the other points, so the sub-sample is drawn first (same draws, same order on
    # the host stream) and only its <= pc_corr_max_size points are searched: identical tensors, a quarter of the queries.
    src_inds, tgt_inds = src_inds.to(dev), tgt_inds.to(dev)
    n_src, n_tgt = int(src_inds.shape[0]), int(tgt_inds.shape[0])
    src_sel = _index_tensor(choice_uniform_noreplace(rng, n_src, min(args.pc_corr_max_size, n_src)), dev)          # :279-280
    tgt_sel = _index_tensor(choice_uniform_noreplace(rng, n_tgt, min(args.pc_corr_max_size, n_tgt)), dev)          # :283-284
    src_pts_raw = src_pts_raw[src_inds[src_sel]][None].contiguous()
    tgt_pts_raw = tgt_pts_raw[tgt_inds[tgt_sel]][None].contiguous()
    if src_pts_raw.is_cuda and all(x.dtype == torch.float32 for x in (src_pts_raw, tgt_pts_raw, src_pts, tgt_pts)):
        # both clouds as one batch of two through the grid build and the search (same arithmetic per cloud, half the launches), whatever
        # the four sizes are: the collate dilutes source and target independently (kitti_dataset.py:568-569), the thinning keeps what it keeps
        i_s, i_t = ops.nn1_pair(src_pts_raw, tgt_pts_raw, src_pts.contiguous(), tgt_pts.contiguous())                 # :272, :274
        src_feat_corr = src_feat[0][i_s][None]                                                                   # knn_gather(...)[:, :, 0, :]
        tgt_feat_corr = tgt_feat[0][i_t][None]
    else:
        ind = ops.knn_points(src_pts_raw, src_pts, K=1)                                                          # :272
        src_feat_corr = src_feat[0][ind[1][0, :, 0]][None]                                                       # knn_gather(...)[:, :, 0, :]
        ind = ops.knn_points(tgt_pts_raw, tgt_pts, K=1)                                                          # :274
        tgt_feat_corr = tgt_feat[0][ind[1][0, :, 0]][None]
    return pc_fcht(pc1_pts=src_pts_raw.contiguous(), pc2_pts=tgt_pts_raw.contiguous(), pc1_feat=src_feat_corr.contiguous(),
                   pc2_feat=tgt_feat_corr.contiguous(), rtume_hypotises=rtume_tform, gt_tform=gt_tform,
                   corr_sigma=args.corr_kernel_sigma, args=args, timing=timing, return_tform=return_tform)


def refine_registration(R_hat, t_hat, args, pairs, tform_dev=None, estimation=None):
    """reference evaluate.py:63-109 (`refine_registration`): point-to-point ICP from every selected (R_hat, t_hat),
    max correspondence distance 0.2 m, max_iteration=200, then RRE / RTE against the ground truth.
    estimation (default: args.icp_estimation, else "point_to_point", the reference's): "point_to_plane" refines with
    ops.icp_point_to_plane on the target's normals (ops.estimate_normals with args.icp_normal_knn = 30 neighbours and
    args.icp_normal_radius = None), computed once per target cloud; "plane_to_plane" with ops.icp_plane_to_plane on the normals of
    both clouds (the source's in its own frame: the kernel rotates them) and args.icp_gicp_epsilon = 1e-3.
    args.icp_voxel_sizes (with args.icp_level_distances / args.icp_level_iterations, icp_multiscale.levels_of): coarse to fine with
    that estimation, ops.icp_multi_scale, one host wait per level; unset: the single-scale calls below, as ever.
    The reference re-opens its dataset here; this takes the raw clouds instead:
    pairs = iterable of (src_pts_raw [n,3], tgt_pts_raw [m,3], gt_tform [4,4]).
    tform_dev: optional [P,4,4] float32 DEVICE tensor holding the same (R_hat, t_hat) as 4 x 4 transforms: the ICP then starts from
    it on the device (no host read of the hypothesis before its first kernels are enqueued).
    -> (T_est [P,4,4] f32, rre [P] deg, rte [P] m), like the reference."""
    T_est_arr, rre_arr, rte_arr = [], [], []
    max_corr = float(getattr(args, "icp_max_correspondence_distance", 0.2))
    max_it = int(getattr(args, "icp_max_iteration", 200))
    estimation, normal_knn, normal_radius = icp_plane.estimation_of(args, estimation)
    gicp_epsilon = icp_gicp.epsilon_of(args) if estimation == icp_gicp.ESTIMATION else None
    levels = icp_multiscale.levels_of(args)
    for itr, (src_pts_raw, tgt_pts_raw, gt_tform) in enumerate(pairs):
        if tform_dev is not None:
            tform_hat = tform_dev[itr].contiguous()
        else:
            tform_hat = np.zeros((4, 4))
            tform_hat[:3, :3] = np.asarray(R_hat[itr].detach().cpu() if isinstance(R_hat[itr], torch.Tensor) else R_hat[itr])
            tform_hat[:3, 3] = np.asarray(t_hat[itr].detach().cpu() if isinstance(t_hat[itr], torch.Tensor) else t_hat[itr])
            tform_hat[3, 3] = 1
        if levels is not None:
            reg = ops.icp_multi_scale(src_pts_raw, tgt_pts_raw, tform_hat, *zip(*levels), estimation=estimation, normal_knn=normal_knn,
                                      normal_radius=normal_radius, epsilon=icp_gicp.DEFAULT_EPSILON if gicp_epsilon is None else gicp_epsilon)
        elif estimation == "point_to_plane":
            normals = ops.estimate_normals(tgt_pts_raw, normal_knn, normal_radius)
            reg = ops.icp_point_to_plane(src_pts_raw, tgt_pts_raw, normals, tform_hat, max_corr, max_it)
        elif estimation == icp_gicp.ESTIMATION:
            src_normals = ops.estimate_normals(src_pts_raw, normal_knn, normal_radius)
            normals = ops.estimate_normals(tgt_pts_raw, normal_knn, normal_radius)
            reg = ops.icp_plane_to_plane(src_pts_raw, tgt_pts_raw, src_normals, normals, tform_hat, max_corr, max_it, epsilon=gicp_epsilon)
        else:
            reg = ops.icp_point_to_point(src_pts_raw, tgt_pts_raw, tform_hat, max_corr, max_it)
        new_tform = torch.from_numpy(reg.transformation).float()
        T_est_arr.append(new_tform)
        gt = gt_tform.detach().cpu().float() if isinstance(gt_tform, torch.Tensor) else torch.as_tensor(gt_tform).float()
        dev = src_pts_raw.device
        rre = relative_rotation_error(new_tform[:3, :3][None].to(dev).contiguous(), gt[:3, :3][None].to(dev).contiguous()).cpu()
        rte = (new_tform[:3, 3] - gt[:3, 3]).norm(dim=-1)
        rre_arr.append(rre)
        rte_arr.append(rte)
    return torch.stack(T_est_arr), torch.cat(rre_arr), torch.stack(rte_arr)


def my_ume_generation(pts, kpts, feat, args):
    """reference evaluate.py:50-60.  pts [bs,N,3], kpts [bs,n,3], feat [bs,N,32] -> F [bs,n,32,4];
    args.ume_max_nn / args.ume_r_nn as in the benchmark YAMLs."""
    return ops.ume_moments(pts, kpts, feat, args.ume_max_nn, args.ume_r_nn)


_OVERLAP_STREAMS = {}


def evaluate_pairs(pairs, args, rng=np.random, refine=True, verbose=False, overlap=True, collect=None):
    """The reference's evaluation loop (evaluate.py:175-309) over an iterable of registration pairs, with the
    reference's RNG consumption order per pair (keypoint draws, weighted match draw, correlation sub-sampling):

        pair = dict(src_pts [1,N,3], tgt_pts [1,N,3], src_feat [1,N,32], tgt_feat [1,N,32]  (network points + features),
                    src_pts_raw [n,3], tgt_pts_raw [m,3]  (raw clouds; default: the network points), gt_tform [4,4])

    -> dict(R_sel, t_sel [P,...] (selected hypotheses), T_est [P,4,4], rre [P], rte [P], rr_np, rr_sp, mrre, mrte)
    where the last four are the numbers the reference prints (:304-309).  overlap (default): consecutive pairs overlap on
    two HIP streams (same results, same RNG consumption; see the loop).  Datasets and the feature network are the
    caller's business (out of scope); everything between them and the printed metrics is here.
    collect: a list that receives, per pair, the intermediate results a stage-by-stage comparison against a CPU checker needs
    (tests): dict(rtume_tform [M,4,4] (every hypothesis), cond (the drawn rows, host), match [1,n_kp], match_d [1,n_kp],
    prob [n_kp] | None, ume_src / ume_tgt [1,n_kp,32,4], T_sel [4,4] (the selected hypothesis)).  The tensors are device
    CLONES, made on the pair's stream only when `collect` is given; without it nothing is copied."""
    R_sel, t_sel, raw = [], [], []
    # Two pairs overlap on two HIP streams: while the correlation scores of pair i are computed (two thirds of a pair's GPU
    # time, and nothing on the host needs them before the read-back below), pair i + 1 goes through its keypoint draws,
    # a1-a7, the weighted draw, the raw-cloud prep and the enqueue of its own scores.  The host RNG is consumed exactly in
    # the reference's order (pair i completely, then pair i + 1): every host read inside a pair waits for that pair's
    # stream only.  overlap=False: one pair at a time on the caller's stream.
    streams, pending, k = None, None, 0

    refined = []      # per pair: T_est [4,4] (host) when the ICP runs inside the loop
    max_corr = float(getattr(args, "icp_max_correspondence_distance", 0.2))
    max_it = int(getattr(args, "icp_max_iteration", 200))
    estimation, normal_knn, normal_radius = icp_plane.estimation_of(args)
    gicp_epsilon = icp_gicp.epsilon_of(args) if estimation == icp_gicp.ESTIMATION else icp_gicp.DEFAULT_EPSILON
    # coarse to fine (args.icp_voxel_sizes): no IcpJob -- such pairs take the synchronous branch of read_back (`job is None`), one host
    # wait per level per pair; an overlapped pyramid job is deliberately not built
    multi_scale = icp_multiscale.levels_of(args) is not None

    def read_back(p):
        R_hat, t_hat, st, _keep, T_dev, job, clouds = p     # _keep: the pair's input tensors stay alive until its last kernel is done
        with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
            if job is None and refine:
                # (no job could be enqueued for this pair -- one pair at a time on the caller's stream, or clouds the job does not take:
                # the synchronous form, here, so that a loop over 1 475 pairs never holds more than two pairs of raw clouds)
                refined.append(refine_registration(R_hat, t_hat, args, [clouds], tform_dev=T_dev if T_dev.is_cuda else None)[0][0])
            if job is not None:
                # The reference refines all pairs after the loop (:301).  The ICP consumes no random numbers and touches nothing but
                # its own pair: its whole chain was enqueued right behind the pair's hypothesis selection (ops.IcpJob: it starts from
                # the selected transform ON THE DEVICE and stops by a flag on the device), so by now -- one pair later -- its result
                # is waiting in pinned memory and the refinement has cost the host no round trip.
                refined.append(torch.from_numpy(job.result().transformation).float())
            T_host = T_dev.cpu()                   # (one read for R_hat and t_hat: they are views of it)
            R_sel.append(T_host[:, :3, :3])
            t_sel.append(T_host[:, :3, 3])

    for pair in pairs:
        dev = pair["src_pts"].device
        st = None
        if overlap and dev.type == "cuda":
            if streams is None:
                # (kept per device: the native workspaces are per stream, a fresh pair of streams per call would allocate anew)
                streams = _OVERLAP_STREAMS.get(dev)
                if streams is None:
                    # two streams MEASURED to run side by side, neither on the null stream's hardware queue (streams.py: which queue
                    # the runtime gives a new stream depends on what the process created before -- 440 / 380 / 310 pairs/s here)
                    streams = _OVERLAP_STREAMS[dev] = list(_streams.concurrent_streams(dev, 2))
            st = streams[k % 2]
            st.wait_stream(torch.cuda.current_stream(dev))      # the pair's tensors were made on the caller's stream
        with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
            src_raw = pair.get("src_pts_raw", pair["src_pts"][0])
            tgt_raw = pair.get("tgt_pts_raw", pair["tgt_pts"][0])
            # the voxel thinning of :261-264 (no random numbers) is enqueued behind a1-a5, so that it runs while the host makes the
            # weighted draw of :238 and its counts are waiting when the selection starts
            out = register_pair(pair["src_pts"], pair["tgt_pts"], pair["src_feat"], pair["tgt_feat"], args, rng=rng,
                                after_phase_a=lambda: prepare_selection(src_raw, tgt_raw, args))                        # :195-254
            _, _, R_hat, t_hat, T_dev = select_hypothesis(src_raw, tgt_raw, pair["src_pts"], pair["tgt_pts"], pair["src_feat"],
                                                          pair["tgt_feat"], out.rtume_tform, pair["gt_tform"], args, rng=rng,
                                                          prepared=getattr(out, "side", None), return_tform=True)       # :258-296
            if collect is not None:
                cl = lambda t_: t_.clone() if isinstance(t_, torch.Tensor) else t_                                      # noqa: E731
                collect.append(dict(rtume_tform=out.rtume_tform[0].clone(), cond=out.cond, match=cl(out.match), match_d=cl(out.match_d),
                                    prob=cl(out.prob), ume_src=cl(out.ume_src), ume_tgt=cl(out.ume_tgt), T_sel=T_dev[0].clone()))
            job = None
            if refine and not multi_scale and st is not None and src_raw.is_cuda and src_raw.dtype == torch.float32 \
                    and tgt_raw.dtype == torch.float32:
                # (point to plane: the target's normals, once per target cloud, on the pair's stream behind the selection like the
                # chain itself -- opting in adds no host read; plane to plane: the source's too, in the source's own frame)
                src_normals = ops.estimate_normals(src_raw, normal_knn, normal_radius) if estimation == icp_gicp.ESTIMATION else None
                normals = ops.estimate_normals(tgt_raw, normal_knn, normal_radius) if estimation != "point_to_point" else None
                job = ops.IcpJob(src_raw, tgt_raw, T_dev[0].contiguous(), max_corr, max_it, tgt_normals=normals,
                                 src_normals=src_normals, epsilon=gicp_epsilon)                                           # :63-96
        raw.append(pair["gt_tform"])
        if pending is not None:
            read_back(pending)        # the previous pair's result: its scores ran beside everything above
        pending = (R_hat, t_hat, st, pair, T_dev, job, (src_raw, tgt_raw, pair["gt_tform"]))
        if st is None:
            read_back(pending)
            pending = None
        k += 1
    if pending is not None:
        read_back(pending)
    if streams is not None:
        for st in streams:
            torch.cuda.current_stream(streams[0].device).wait_stream(st)
    R_sel, t_sel = torch.cat(R_sel, dim=0), torch.cat(t_sel, dim=0)
    if refine:
        T_est = torch.stack(refined)                                                                               # :301 (refined inside the loop)
    else:
        T_est = torch.eye(4)[None].repeat(R_sel.shape[0], 1, 1)
        T_est[:, :3, :3], T_est[:, :3, 3] = R_sel, t_sel
    gts = torch.stack([g.detach().cpu().float() if isinstance(g, torch.Tensor) else torch.as_tensor(g).float() for g in raw])
    dev = R_hat.device
    rre = relative_rotation_error(T_est[:, :3, :3].to(dev).contiguous(), gts[:, :3, :3].to(dev).contiguous()).cpu()           # :100-107
    rte = (T_est[:, :3, 3] - gts[:, :3, 3]).norm(dim=-1)
    rr_np = float(((rre <= 1.5) & (rte <= 0.6)).float().mean())                                                   # :304-305
    rr_sp = float(((rre <= 1) & (rte <= 0.1)).float().mean())
    res = dict(R_sel=R_sel, t_sel=t_sel, T_est=T_est, rre=rre, rte=rte, rr_np=rr_np, rr_sp=rr_sp,
               mrre=float(rre.mean()), mrte=float(rte.mean()))
    if verbose:
        print(f"N.P: {100 * rr_np:.03f} | S.P: {100 * rr_sp:.03f}")
        print(f"mRRE: {res['mrre']:.03f} | mRTE: {res['mrte']:.03f}")
    return res


def load_pair_file(path, device):
    """One registration pair from an .npz in the loader output contract of SURVEY 8(f4): `src_pts`/`tgt_pts` [N,3] (network
    points), `src_feat`/`tgt_feat` [N,32] (their features), `gt_tform` [4,4], optionally `src_pts_raw`/`tgt_pts_raw`."""
    with np.load(path) as z:
        dev = lambda k: torch.from_numpy(np.ascontiguousarray(z[k], dtype=np.float32)).to(device)   # noqa: E731
        pair = dict(src_pts=dev("src_pts")[None], tgt_pts=dev("tgt_pts")[None], src_feat=dev("src_feat")[None],
                    tgt_feat=dev("tgt_feat")[None], gt_tform=dev("gt_tform"))
        for k in ("src_pts_raw", "tgt_pts_raw"):
            if k in z.files:
                pair[k] = dev(k)
    return pair


def synthetic_pairs(benchmark, indices, device):
    """Synthetic stand-ins of the benchmark's shape: KITTI-shaped or nuScenes-shaped clouds; the rot*
    benchmarks draw the large-yaw distribution.  Generated lazily, one pair resident at a time."""
    from .synth import synth_pair_cfg
    config = "NS" if "nuscenes" in benchmark else "KT"
    kind = "rot" if benchmark.startswith("rot") else "test"
    for i in indices:
        p = synth_pair_cfg(i, config, kind)
        t = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
        yield dict(src_pts=t(p.src_pts)[None], tgt_pts=t(p.tgt_pts)[None], src_feat=t(p.src_feat)[None],
                   tgt_feat=t(p.tgt_feat)[None], gt_tform=t(p.gt_tform))


def cached_pairs(cache, cache_raw, split, indices, args, device, rng=np.random, checkpoint=None, feature_precision="f32", conv_mode="union"):
    """Pairs from the reference's pre-processed cache (`datasets.CachedPairDataset`) through the reference's
    collate (`batch_collate_fn_dset`, batch_size 1: the dilution to args.max_pc_size with the host RNG), as the evaluation
    loop unpacks them (evaluate.py:175-187).  Without `checkpoint` the cache files must carry the feature network's outputs
    (`src_feat` / `tgt_feat`); with it (a weight file of the reference's save_checkpoint schema, or a state dict) the
    features are computed from the collate's coordinates by `models.ResUNetSmall2` (evaluate.py:163-165, :178-179,
    :190-192), with `feature_precision` "f32" or "f16" (f16 operands, f32 accumulation: include/umereg_featnet_f16.h) and
    `conv_mode` "union" or "pairs" (the pair-compacted convolution engine, the same features bit for bit:
    include/umereg_sparse_conv_pairs.h).  The raw clouds of the correlation stage (`dset_no_nksr[itr]`, :260) come from `cache_raw` (default: the
    same files)."""
    from .datasets import CachedPairDataset, batch_collate_fn_dset
    kind = getattr(args, "dataset", "kitti")
    net = None
    if checkpoint is not None:
        from .datasets import checkpoint_state_dict
        from .models import ResUNetSmall2
        from .sparse import SparseTensor
        net = ResUNetSmall2(in_channels=1, out_channels=getattr(args, "out_ch", 32), precision=feature_precision, conv_mode=conv_mode)
        net.load_state_dict(checkpoint_state_dict(checkpoint))
        net = net.to(device).eval()
    ds = CachedPairDataset(cache, split=split, with_features=net is None, dataset=kind)
    ds_raw = CachedPairDataset(cache_raw or cache, split=split, files=ds.files, dataset=kind)
    for i in indices(len(ds)) if callable(indices) else indices:
        b = batch_collate_fn_dset([ds[i]], num_matches=args.num_samples, max_pc_size=args.max_pc_size, rng=rng)
        raw = ds_raw[i]
        if net is None:
            src_feat, tgt_feat = b[11].float().to(device), b[12].float().to(device)
        else:
            with torch.no_grad():
                src_feat = torch.stack(net(SparseTensor(b[3], coordinates=b[2], device=device)).decomposed_features, dim=0)
                tgt_feat = torch.stack(net(SparseTensor(b[7], coordinates=b[6], device=device)).decomposed_features, dim=0)
        yield dict(src_pts=b[0].float().to(device), tgt_pts=b[4].float().to(device), src_feat=src_feat,
                   tgt_feat=tgt_feat, gt_tform=b[9][0].float().to(device),
                   src_pts_raw=raw[0].float().to(device), tgt_pts_raw=raw[3].float().to(device))


def main(argv=None):
    """`python -m umeregrobust_amd.evaluate --benchmark kitti_test` - the reference's command line (evaluate.py:113-124)
    and result lines (:304-309).  Pairs come from the reference's pair cache (--cache; features from the cache files, or
    computed by the feature network with --checkpoint), from --pairs files (points + features as the loader/network would
    hand them over) or, by default, from the synthetic generator at the benchmark's shape.  Under torch.distributed.run every rank takes pairs[rank::world] and the metric
    counts are summed with one all-reduce; each rank then seeds its host RNG with seed + rank."""
    import argparse
    import glob
    import os
    from .dist import RegistrationMetrics, init_distributed, shard_indices
    from .utils.general_utils import BENCHMARK_CONFIGS, benchmark_config_path, update_namespace_from_yaml
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument("--benchmark", type=str, choices=list(BENCHMARK_CONFIGS), default="kitti_test")
    parser.add_argument("--pairs", nargs="*", default=None, help=".npz pair files or directories of them (see load_pair_file)")
    parser.add_argument("--cache", default=None, help="the reference's pair cache (<dir>/<split>/<seq>/<f0>_<f1>.pickle) with "
                                                      "`src_feat`/`tgt_feat` added: datasets.CachedPairDataset + batch_collate_fn_dset")
    parser.add_argument("--cache-raw", default=None, help="cache of the raw clouds for the correlation stage (dset_no_nksr); default: --cache")
    parser.add_argument("--checkpoint", default=None, help="with --cache: weights of the feature network (the reference's "
                                                           "model_checkpoint_path); features are computed by models.ResUNetSmall2 "
                                                           "instead of read from the cache")
    parser.add_argument("--feature-precision", choices=["f32", "f16"], default="f32",
                        help="with --checkpoint: operand precision of the feature network (f16: f16 operands on the f16 matrix "
                             "instructions, f32 accumulation; include/umereg_featnet_f16.h)")
    parser.add_argument("--conv-mode", choices=["union", "pairs"], default="union",
                        help="with --checkpoint: engine of the feature network's 27-offset convolutions (pairs: per offset only the rows "
                             "that have the neighbour reach the matrix unit; same features; include/umereg_sparse_conv_pairs.h)")
    parser.add_argument("--synthetic", type=int, default=8, help="number of synthetic pairs when no --pairs are given")
    parser.add_argument("--no-refine", action="store_true", help="skip the ICP refinement (evaluate.py:301)")
    parser.add_argument("--icp-estimation", choices=list(icp_plane.ESTIMATIONS), default="point_to_point",
                        help="estimation of the ICP refinement: the reference's point to point (default), point to plane on target "
                             "normals estimated on the device (include/umereg_icp_plane.h), or plane to plane (generalized ICP) on the "
                             "normals of both clouds (include/umereg_icp_gicp.h)")
    parser.add_argument("--icp-normal-knn", type=int, default=icp_plane.DEFAULT_KNN,
                        help="with --icp-estimation point_to_plane / plane_to_plane: neighbours per normal (3 .. 64)")
    parser.add_argument("--icp-normal-radius", type=float, default=None,
                        help="with --icp-estimation point_to_plane / plane_to_plane: hybrid search, neighbours farther than this are dropped")
    parser.add_argument("--icp-gicp-epsilon", type=float, default=icp_gicp.DEFAULT_EPSILON,
                        help="with --icp-estimation plane_to_plane: the regularised covariance's small eigenvalue, in [1e-4, 1]")
    parser.add_argument("--icp-voxel-sizes", type=icp_multiscale.parse_list, default=None,
                        help="coarse-to-fine ICP: voxel sizes per level, strictly decreasing, the last may be 0 = the clouds as given "
                             "(e.g. 0.8,0.4,0); unset: single scale")
    parser.add_argument("--icp-level-distances", type=icp_multiscale.parse_list, default=None,
                        help="with --icp-voxel-sizes: max correspondence distance per level (default: max(2 voxel, the single-scale "
                             "distance); a choice, not tuned on real scans)")
    parser.add_argument("--icp-level-iterations", type=lambda s: icp_multiscale.parse_list(s, int), default=None,
                        help="with --icp-voxel-sizes: iteration limit per level (default: the single-scale limit on every level)")
    cli = parser.parse_args(argv)
    config_path = benchmark_config_path(cli.benchmark)
    args = update_namespace_from_yaml(argparse.Namespace(benchmark=cli.benchmark), config_path)
    args.icp_estimation, args.icp_normal_knn, args.icp_normal_radius = cli.icp_estimation, cli.icp_normal_knn, cli.icp_normal_radius
    args.icp_gicp_epsilon = cli.icp_gicp_epsilon
    args.icp_voxel_sizes, args.icp_level_distances, args.icp_level_iterations = cli.icp_voxel_sizes, cli.icp_level_distances, cli.icp_level_iterations
    icp_multiscale.levels_of(args)                 # (a bad list is an error now, not at the first pair)
    rank, local_rank, world = init_distributed()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    args.device = str(device)
    torch.manual_seed(args.seed)
    rng = np.random.RandomState(args.seed + rank) if world > 1 else np.random
    if world == 1:
        np.random.seed(args.seed)                                                                     # :127
    if rank == 0:
        print(f"Evaluate {args.dataset} Benchmark: {args.benchmark} config file: {config_path}")
    if cli.cache:
        pairs = cached_pairs(cli.cache, cli.cache_raw, args.split, lambda n: shard_indices(n, rank, world), args, device, rng=rng,
                             checkpoint=cli.checkpoint, feature_precision=cli.feature_precision, conv_mode=cli.conv_mode)
    elif cli.pairs:
        files = []
        for p in cli.pairs:
            files += sorted(glob.glob(os.path.join(p, "*.npz"))) if os.path.isdir(p) else [p]
        mine = [files[i] for i in shard_indices(len(files), rank, world)]
        pairs = (load_pair_file(f, device) for f in mine)
    else:
        pairs = synthetic_pairs(cli.benchmark, shard_indices(cli.synthetic, rank, world), device)
    metrics = RegistrationMetrics()
    with torch.no_grad():
        # the whole (lazy) stream of pairs through ONE evaluate_pairs loop per chunk: consecutive pairs overlap on two streams and a
        # pair's ICP is read one pair later (a call per pair, as until round 5, gave all of that away: 330 against 440 pairs/s)
        it = iter(pairs)
        while True:
            chunk = list(__import__("itertools").islice(it, 64))
            if not chunk:
                break
            res = evaluate_pairs(chunk, args, rng=rng, refine=not cli.no_refine)
            metrics.update(res["rre"].numpy(), res["rte"].numpy())
    s = metrics.all_reduce(device).summary()
    if rank == 0:
        print(f"N.P: {s['rr_np_06']:.03f} | S.P: {s['rr_sp']:.03f}")
        print(f"mRRE: {s['mrre']:.03f} | mRTE: {s['mrte']:.03f}")
    return s


if __name__ == "__main__":
    main()
