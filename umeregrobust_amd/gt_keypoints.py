"""Device-side selection of the ground-truth-driven keypoints: the engine behind
`utils.loc_utils.generate_ume_from_keypoints2(..., selection="device")` on the HIP kernels of include/umereg_gt_keypoints.h.

    cand, lengths = candidates(overlap_idx, non_flat)                      # descending index order, -1 padded; no sort
    kp_index, record = select(src_pts, cand, lengths, nn_r, max_nn, min_nn, num_samples)
    hits = ball_any(q, p, radius)                                          # [Bk]: rows of q[b] with a row of p[b] within the radius

`select` answers "min(hits, max_nn) >= min_nn" lazily -- a ball's scan ends at its min_nn-th hit and candidates are only tested up
to the one that completes num_samples dense ones -- where the default path forms the moment matrix of every candidate.  `record`
(int32 [B, 2]: min(#dense, num_samples) and the candidate count per element) is the one thing the generator reads on the host.
Every output is the same in every run; nothing here waits for the device."""
import torch

from . import _lib, ops

GT_KEYPOINTS_SIGNATURES = _lib.TABLES["umereg_gt_keypoints.h"]
load_native = _lib.load

SELECTIONS = ("torch", "device")
MAX_B = 1024                # UMEREG_GT_KEYPOINTS_MAX_B
BALL_ANY_MAX_K = 7680       # UMEREG_GT_BALL_ANY_MAX_K
RECORD_WORDS = 2            # UMEREG_GT_RECORD_WORDS
# the launch constants of csrc/gt_keypoints.hip the tests place their edges at
CAND_BLOCK, PICK_BLOCK, TEST_WAVES, MAX_TEST_WG, WORKERS_PER_SAMPLE, ANY_BLOCK, ANY_TILE = 256, 1024, 4, 512, 4, 256, 4096


def check_selection(who, selection):
    """ValueError for anything but "torch" / "device"; touches no tensor and no library."""
    if selection not in SELECTIONS:
        raise ValueError(f"{who}: selection must be 'torch' or 'device', got {selection!r}")


def workspace_bytes(B, N):
    """Python restatement of umereg_gt_keypoints_workspace_bytes (block counts, two counters per element, one flag per position)."""
    if B < 1 or B > MAX_B or N < 1:
        return 0
    up = lambda v, a: -(-v // a) * a
    return up(up(B * -(-N // CAND_BLOCK) * 4, 16) + up(B * 2 * 4, 16) + B * N, 256)


def _workspace(lib, dev, B, N, workspace):
    need = int(lib.umereg_gt_keypoints_workspace_bytes(B, N))
    if need == 0:
        raise ValueError(f"gt_keypoints: sizes B = {B}, N = {N} not supported (1 <= B <= {MAX_B}, N >= 1)")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    return workspace


def candidates(overlap_idx, non_flat, workspace=None):
    """overlap_idx int64 [B, N] (> -1 = the point overlaps the target), non_flat bool / uint8 [B, N] -> (cand int32 [B, N]: the
    flagged indices in descending order, then -1; lengths int32 [B])."""
    lib = load_native()
    _lib.on_gpu("gt_keypoints.candidates", overlap_idx, non_flat)
    if overlap_idx.dim() != 2 or overlap_idx.dtype != torch.int64 or tuple(non_flat.shape) != tuple(overlap_idx.shape):
        raise ValueError(f"gt_keypoints.candidates: overlap_idx int64 [B, N] and non_flat [B, N] expected, got {overlap_idx.dtype} "
                         f"{tuple(overlap_idx.shape)} / {tuple(non_flat.shape)}")
    if non_flat.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"gt_keypoints.candidates: non_flat must be bool or uint8, got {non_flat.dtype}")
    B, N = overlap_idx.shape
    dev = overlap_idx.device
    overlap_idx = overlap_idx.contiguous()
    non_flat = non_flat.contiguous().view(torch.uint8)
    workspace = _workspace(lib, dev, B, N, workspace)
    cand = torch.empty(B, N, dtype=torch.int32, device=dev)
    lengths = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call(dev, lib.umereg_gt_candidates, overlap_idx.data_ptr(), non_flat.data_ptr(), B, N, cand.data_ptr(), lengths.data_ptr(),
              workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(dev))
    return cand, lengths


def select(pts, cand, lengths, radius, max_nn, min_nn, num_samples, fma=False, workspace=None, return_tested=False):
    """pts f32 [B, N, 3], cand / lengths as `candidates` returns them -> (kp_index int64 [B, num_samples]: per element the first
    num_samples candidates -- walking the list, cut to the batch-minimum length, from its end to its head, as the reference's descending
    sort of the dense positions does -- whose ball of `radius` holds >= min_nn points when counted up
    to max_nn, then -1; record int32 [B, 2]: how many those are, and lengths).  return_tested: also int32 [B], how many candidates
    were tested -- a measurement, the only output that differs between runs."""
    lib = load_native()
    _lib.on_gpu("gt_keypoints.select", pts, cand, lengths)
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32:
        raise ValueError(f"gt_keypoints.select: pts must be f32 [B, N, 3], got {pts.dtype} {tuple(pts.shape)}")
    B, N = pts.shape[:2]
    if tuple(cand.shape) != (B, N) or cand.dtype != torch.int32 or tuple(lengths.shape) != (B,) or lengths.dtype != torch.int32:
        raise ValueError(f"gt_keypoints.select: cand int32 [B, N] and lengths int32 [B] expected for pts {tuple(pts.shape)}, got "
                         f"{cand.dtype} {tuple(cand.shape)} / {lengths.dtype} {tuple(lengths.shape)}")
    num_samples = int(num_samples)
    if num_samples < 1:
        raise ValueError(f"gt_keypoints.select: num_samples must be positive, got {num_samples}")
    dev = pts.device
    pts, cand, lengths = pts.contiguous(), cand.contiguous(), lengths.contiguous()
    workspace = _workspace(lib, dev, B, N, workspace)
    packed = ops._workspace(dev, lib.umereg_ume_moments_workspace_bytes(B, N), "mom")
    kp_index = torch.empty(B, num_samples, dtype=torch.int64, device=dev)
    record = torch.empty(B, RECORD_WORDS, dtype=torch.int32, device=dev)
    tested = torch.empty(B, dtype=torch.int32, device=dev) if return_tested else None
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        _lib.checked(lib.umereg_pack_points_f32, pts.data_ptr(), B, N, float(radius), packed.data_ptr(), packed.numel(), st)
        _lib.checked(lib.umereg_gt_select_f32, packed.data_ptr(), cand.data_ptr(), lengths.data_ptr(), B, N, float(radius), int(max_nn),
                     int(min_nn), num_samples, ops.BALL_FMA if fma else 0, kp_index.data_ptr(), record.data_ptr(), _lib.ptr(tested),
                     workspace.data_ptr(), workspace.numel(), st)
    return (kp_index, record, tested) if return_tested else (kp_index, record)


def ball_any(q, p, radius, fma=False):
    """q, p f32 [Bk, K, 3] -> hits int32 [Bk]: the rows of q[b] with some row of p[b] strictly within `radius`; what
    `(ops.ball_query(q, p, K=1, radius=radius).idx > -1).sum((1, 2))` counts, in one launch and without a search structure per b."""
    _lib.on_gpu("gt_keypoints.ball_any", q, p)
    if q.dim() != 3 or q.shape[2] != 3 or tuple(p.shape) != tuple(q.shape) or q.dtype != torch.float32 or p.dtype != torch.float32:
        raise ValueError(f"gt_keypoints.ball_any: q and p must be f32 [Bk, K, 3] of one shape, got {q.dtype} {tuple(q.shape)} / "
                         f"{p.dtype} {tuple(p.shape)}")
    Bk, K = q.shape[:2]
    if not 1 <= K <= BALL_ANY_MAX_K:
        raise ValueError(f"gt_keypoints.ball_any: K = {K}; 1 <= K <= {BALL_ANY_MAX_K} is supported")
    lib = load_native()
    dev = q.device
    hits = torch.empty(Bk, dtype=torch.int32, device=dev)
    if Bk == 0:
        return hits
    q, p = q.contiguous(), p.contiguous()
    _lib.call(dev, lib.umereg_gt_ball_any_f32, q.data_ptr(), p.data_ptr(), Bk, K, float(radius), ops.BALL_FMA if fma else 0,
              hits.data_ptr(), _lib.stream_ptr(dev))
    return hits


NO_CANDIDATE = ("generate_ume_from_keypoints2: a batch element has no candidate keypoint "
                "(no non-flat source point overlaps the target)")
NO_KEYPOINT = "generate_ume_from_keypoints2: no keypoint with >= min_nn neighbours in any batch element"

host_reads = 0      # device-to-host reads issued by generate() since import (tools/gt_keypoints_time.py reports the difference)


def generate(velo_pts, velo_seg, velo_feat, ref_pts, ref_feat, gt_tform, nn_r, max_nn, min_nn, num_samples, flat_labels,
             normalized_ume, nn_intersection_r):
    """generate_ume_from_keypoints2 with the selection on the device (its docstring has the contract): the same six outputs, bit for
    bit, as the default path.  The expressions whose rounding is torch's are the default path's own, on the same shapes."""
    global host_reads
    ball_query = ops.ball_query
    bs, velo_pc_size, dim_size = velo_feat.shape
    dev = velo_pts.device
    if velo_seg.shape[-1] == 1:
        # `(velo_seg != torch.tensor(flat_labels)).all(-1)` label by label: the same mask without a host-to-device copy, which
        # would make the host wait for the stream as a read does
        non_floor_mask = torch.ones(velo_seg.shape[:-1], dtype=torch.bool, device=dev)
        for label in flat_labels:
            non_floor_mask &= velo_seg[..., 0] != label
        non_floor_mask = non_floor_mask.flatten(1)
    else:
        non_floor_mask = (velo_seg != torch.tensor(flat_labels, device=velo_seg.device)).all(dim=-1).flatten(1)
    R_gt = gt_tform[:, :3, :3]
    t_gt = gt_tform[:, :3, 3]
    velo_pts_tform = velo_pts @ R_gt.transpose(-1, -2) + t_gt[:, None]
    tt = ball_query(velo_pts_tform.contiguous(), ref_pts, K=1, radius=nn_intersection_r, return_nn=False).idx
    cand, lengths = candidates(tt[..., 0], non_floor_mask)
    kp_all, record = select(velo_pts.float(), cand, lengths, nn_r, max_nn, min_nn, num_samples)
    with_kpts_batch_cond = record[:, 0] > 0
    rec = record.cpu()              # THE host read of the call: everything the host decides follows from these 2 * bs ints
    host_reads += 1
    n_dense, n_cand = rec[:, 0].tolist(), rec[:, 1].tolist()
    if min(n_cand) == 0:
        raise RuntimeError(NO_CANDIDATE)
    if not 1 <= int(max_nn) <= BALL_ANY_MAX_K:
        # the default path's moment call refuses this K; the same call (one candidate per element) words the same error
        ops.ume_moments(velo_pts, None, velo_feat, max_nn, nn_r, return_count=True, kp_index=cand[:, :1].long(),
                        normalize=bool(normalized_ume))
    if max(n_dense) == 0:
        raise RuntimeError(NO_KEYPOINT)
    if min(n_dense) == 0:
        # the surviving elements by slices and one concatenation: the rows a boolean mask would gather, without the mask's read of
        # the device and without an index tensor's copy to it
        def keep(t):
            return torch.cat([t[b:b + 1] for b in range(bs) if n_dense[b] > 0], dim=0)
        kp_all = keep(kp_all)
        velo_pts, velo_feat, ref_feat, ref_pts, gt_tform = keep(velo_pts), keep(velo_feat), keep(ref_feat), keep(ref_pts), keep(gt_tform)
        R_gt = gt_tform[:, :3, :3]
        t_gt = gt_tform[:, :3, 3]
        bs = R_gt.shape[0]
    num_samples = min(min(n for n in n_dense if n > 0), num_samples)
    kp_index = kp_all[:, :num_samples].contiguous()
    velo_keypoint_pts = torch.gather(velo_pts, 1, kp_index[..., None].expand(-1, -1, 3))
    F_velo = ops.ume_moments(velo_pts, None, velo_feat, max_nn, nn_r, kp_index=kp_index, normalize=bool(normalized_ume))
    ref_keypoint_pts = torch.cat([velo_keypoint_pts, torch.ones_like(velo_keypoint_pts[..., :1])], dim=-1)
    ref_keypoint_pts = ref_keypoint_pts @ gt_tform.transpose(-1, -2)
    ref_keypoint_pts = (ref_keypoint_pts[..., :3] / ref_keypoint_pts[..., 3].unsqueeze(-1)).contiguous()
    F_ref = ops.ume_moments(ref_pts.contiguous(), ref_keypoint_pts, ref_feat.contiguous(), max_nn, nn_r,
                            normalize=bool(normalized_ume))
    velo_nn = ball_query(velo_keypoint_pts.contiguous(), velo_pts.contiguous(), K=max_nn, radius=nn_r, return_nn=True).knn
    ref_nn = ball_query(ref_keypoint_pts, ref_pts.contiguous(), K=max_nn, radius=nn_r, return_nn=True).knn
    velo_nn_tform = velo_nn @ R_gt[:, None].transpose(-1, -2) + t_gt[:, None, None]
    hits = ball_any(velo_nn_tform.flatten(0, 1).contiguous(), ref_nn.flatten(0, 1).contiguous(), nn_intersection_r)
    # the ratio as the default path forms it, `.float().mean()` of a bool tensor with `hits` ones per row (a sum of ones is exact in
    # any order, so which slots hold them does not matter; the division stays torch's)
    slots = torch.arange(max_nn, device=dev)[None] < hits[:, None]
    matched_nn_intersection_ratio = slots.view(bs, num_samples, -1).float().mean(dim=-1)
    return F_velo, F_ref, velo_keypoint_pts, ref_keypoint_pts, matched_nn_intersection_ratio, with_kpts_batch_cond
