"""Ground-truth correspondences of a training pair on the HIP kernels of include/umereg_gt_matches.h (csrc/gt_match.hip): what
`utils.general_utils.one_side_ball_query_matches` / `mutual_ball_query_matches` are made of.

    rows = one_side(src, tgt, T, radius)            # int64 [m, 2] on the device: (i, nearest target of T(src_i)), i ascending
    rows = mutual(src, tgt, T, T_inv, radius)       # the rows whose target maps back to i under T_inv

The semantics are exact and stated in the header (fp32 transform in a fixed order, fp64 distance, lower index on a tie,
`d2 < radius * radius`).  Both calls read the number of rows with ONE device -> host read (like `ops.voxel_first_index`) and
raise RuntimeError when a coordinate is NaN, infinite or (targets) beyond 2^20 m.  The `*_raw` forms take caller-owned outputs and
workspace and never wait for the device."""
import torch

from . import _lib

GT_MATCH_SIGNATURES = _lib.TABLES["umereg_gt_matches.h"]
load_native = _lib.load

MAX_COORD = 1048576.0       # UMEREG_GT_MATCHES_MAX_COORD


def _cloud(who, name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{who}: {name} is a CPU tensor; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be [n, 3], got {tuple(t.shape)}")
    return t.float().contiguous()


def _tform(who, name, T, dev):
    if T is None:
        return None
    T = torch.as_tensor(T)
    if tuple(T.shape) != (4, 4):
        raise ValueError(f"{who}: {name} must be [4, 4], got {tuple(T.shape)}")
    return T.to(device=dev, dtype=torch.float32).contiguous()


def workspace_bytes(n_src, n_tgt, mutual=False):
    return int(_lib.load().umereg_gt_matches_workspace_bytes(int(n_src), int(n_tgt), int(bool(mutual))))


def one_side_raw(src, tgt, T, radius, out_rows, out_count, workspace):
    """Enqueue the one-side search on the current stream.  src [n,3], tgt [m,3] f32 contiguous, T f32 [4,4] or None, out_rows
    int64 [n,2], out_count int32 [2] (rows, error flag), workspace uint8 of >= workspace_bytes(n, m): all on one device."""
    _lib.call(src.device, _lib.load().umereg_gt_matches_one_side_f32, src.data_ptr(), src.shape[0], tgt.data_ptr(), tgt.shape[0],
              _lib.ptr(T), float(radius), out_rows.data_ptr(), out_count.data_ptr(), workspace.data_ptr(), workspace.numel(),
              _lib.stream_ptr(src.device))


def mutual_raw(src, tgt, T, T_inv, radius, out_rows, out_count, workspace):
    """Enqueue the mutual search on the current stream (arguments as one_side_raw; workspace_bytes(n, m, mutual=True))."""
    _lib.call(src.device, _lib.load().umereg_gt_matches_mutual_f32, src.data_ptr(), src.shape[0], tgt.data_ptr(), tgt.shape[0],
              _lib.ptr(T), _lib.ptr(T_inv), float(radius), out_rows.data_ptr(), out_count.data_ptr(), workspace.data_ptr(),
              workspace.numel(), _lib.stream_ptr(src.device))


def _run(who, src, tgt, T, T_inv, radius, is_mutual):
    src, tgt = _cloud(who, "src_pts", src), _cloud(who, "tgt_pts", tgt)
    if tgt.device != src.device:
        raise RuntimeError(f"{who}: the two clouds live on different devices")
    if not float(radius) > 0.0:
        raise ValueError(f"{who}: the radius must be positive, got {radius}")
    dev = src.device
    n, m = src.shape[0], tgt.shape[0]
    if n == 0 or m == 0:
        return torch.empty(0, 2, dtype=torch.int64, device=dev)
    T, T_inv = _tform(who, "the transform", T, dev), _tform(who, "the inverse transform", T_inv, dev)
    rows = torch.empty(n, 2, dtype=torch.int64, device=dev)
    cnt = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(n, m, is_mutual), dtype=torch.uint8, device=dev)
    if is_mutual:
        mutual_raw(src, tgt, T, T_inv, radius, rows, cnt, ws)
    else:
        one_side_raw(src, tgt, T, radius, rows, cnt, ws)
    k, bad = cnt.tolist()                      # the one device -> host read
    if bad:
        raise RuntimeError(f"{who}: a coordinate is NaN or infinite, or a target lies beyond {MAX_COORD:.0f} m from the origin")
    return rows[:k]


def one_side(src, tgt, T, radius):
    """Rows (i, j*) int64 [m, 2], i ascending: j* the nearest target of T(src_i) where its squared distance < radius^2."""
    return _run("gt_matches.one_side", src, tgt, T, None, radius, False)


def mutual(src, tgt, T, T_inv, radius):
    """The one-side rows (i, j) of src -> tgt under T for which tgt -> src under T_inv holds (j, i); [0, 2] when there are none."""
    return _run("gt_matches.mutual", src, tgt, T, T_inv, radius, True)
