"""Linear sum assignment on the device: `scipy.optimize.linear_sum_assignment` for float32 cost matrices that already live on the
GPU, on the HIP kernels of include/umereg_assign.h (csrc/assign.hip) -- an exact shortest-augmenting-path solver with fp64 duals,
one workgroup per matrix of a batch.

    rows, cols = linear_sum_assignment(cost)          # cost [n, m] or [b, n, m] -> int64 [k] or [b, k], k = min(n, m), on the device

Like scipy's, the rows come out ascending, and where the optimum is unique the assignment IS scipy's; where costs tie, another
assignment of the same total may come out (lowest column index first, see the header).  `maximize` is not built.  A matrix with a
NaN or an infinite cost raises ValueError, as scipy does -- that check is the one device -> host read of a call (four bytes per
matrix).  `linear_sum_assignment_raw` takes caller-owned outputs and workspace and never waits for the device."""
import torch

from . import _lib

ASSIGN_SIGNATURES = _lib.TABLES["umereg_assign.h"]
load_native = _lib.load


def workspace_bytes(batch, n_rows, n_cols):
    return int(_lib.load().umereg_assign_workspace_bytes(int(batch), int(n_rows), int(n_cols)))


def linear_sum_assignment_raw(cost, out_pairs, out_total, out_status, workspace):
    """Enqueue one batch on the current stream.  cost: float32 device tensor [b, n, m], n <= m, unit last stride, read through its
    row and batch strides; out_pairs i64 [b, n, 2]; out_total f64 [b] or None; out_status i32 [b]; workspace uint8 of
    >= workspace_bytes(b, n, m)."""
    b, n, m = cost.shape
    row_stride = cost.stride(1) if n > 1 else max(cost.stride(1), m)
    _lib.call(cost.device, _lib.load().umereg_linear_sum_assignment, cost.data_ptr(), b, n, m, row_stride,
              cost.stride(0) if b > 1 else 0, out_pairs.data_ptr(), _lib.ptr(out_total), out_status.data_ptr(), workspace.data_ptr(),
              workspace.numel(), _lib.stream_ptr(cost.device))


def _passes_as_it_lies(c):
    """the kernels read a [b, n, m] tensor in place if its last stride is one, its rows do not overlap and its batch stride is not negative"""
    b, n, m = c.shape
    return (m == 1 or c.stride(2) == 1) and (n == 1 or c.stride(1) >= m) and (b == 1 or c.stride(0) >= 0)


def solve(cost, with_stats=False):
    """The batch as the C entry returns it, without waiting for the device: (pairs i64 [b, n, 2], total f64 [b], status i32 [b]) of
    a float32 device tensor [b, n, m] with n <= m; with_stats: also int64 [b, 2] = (rows matched by the start, Dijkstra steps)."""
    who = "linear_sum_assignment"
    if not isinstance(cost, torch.Tensor) or not cost.is_cuda:
        raise RuntimeError(f"{who}: the cost must be a tensor on the HIP device; umeregrobust_amd has no CPU fallback "
                           "(the host solver is scipy.optimize.linear_sum_assignment)")
    if cost.dtype != torch.float32 or cost.dim() != 3:
        raise ValueError(f"{who}: expected float32 [b, n, m], got {cost.dtype} {tuple(cost.shape)}")
    b, n, m = cost.shape
    if not 0 < n <= m or b == 0:
        raise ValueError(f"{who}: needs 0 < n <= m and a batch that is not empty, got {tuple(cost.shape)}")
    if not _passes_as_it_lies(cost):
        cost = cost.contiguous()
    dev = cost.device
    pairs = torch.empty(b, n, 2, dtype=torch.int64, device=dev)
    total = torch.empty(b, dtype=torch.float64, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = workspace_bytes(b, n, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    linear_sum_assignment_raw(cost, pairs, total, status, ws)
    if with_stats:
        return pairs, total, status, ws.view(b, nbytes // b)[:, :16].contiguous().view(torch.int64)
    return pairs, total, status


def linear_sum_assignment(cost, maximize=False):
    """scipy.optimize.linear_sum_assignment(cost) on the device: cost float32 [n, m] -> (rows, cols) int64 [min(n, m)], or
    [b, n, m] -> [b, min(n, m)] each; rows ascending.  A tall matrix (n > m) is solved as its transpose and reordered here."""
    who = "linear_sum_assignment"
    if maximize:
        raise NotImplementedError(f"{who}: maximize is not built")
    if not isinstance(cost, torch.Tensor) or cost.dim() not in (2, 3):
        raise ValueError(f"{who}: expected a float32 device tensor [n, m] or [b, n, m]")
    c = cost if cost.dim() == 3 else cost[None]
    tall = c.shape[1] > c.shape[2]
    if tall:
        c = c.transpose(1, 2).contiguous()
    pairs, _, status = solve(c)
    bad = torch.nonzero(status).flatten().tolist()                           # THE device -> host read
    if bad:
        raise ValueError(f"{who}: cost matrix {bad[0]} of the batch contains invalid numeric entries (NaN or infinity)")
    rows, cols = pairs[..., 0], pairs[..., 1]
    if tall:                                                                 # pairs are (column, row) of `cost`, ascending by column
        order = torch.argsort(cols, dim=1)
        rows, cols = torch.gather(cols, 1, order), torch.gather(rows, 1, order)
    rows, cols = rows.contiguous(), cols.contiguous()
    return (rows, cols) if cost.dim() == 3 else (rows[0], cols[0])
