"""The loader's collate on the device: `datasets.kitti_dataset.batch_collate_fn_dset` with the index gathers and the match
bookkeeping on the HIP kernels of include/umereg_collate.h (csrc/collate.hip), so that a batch whose items were made on the GPU
(`augmented_item(..., to_host=False)`) never visits the host.

    out = batch_collate_fn_dset_device(items, num_matches, max_pc_size, rng)     # the same 11-tuple (13 with features), on the device

What stays on the host is the random stream: the draws are numpy's `rng.choice(n, size, replace=False)`, made by the same calls in
the same order as the host collate makes them (per element the source draw, then the target draw; after the loop one draw per
element for the matches, also when nothing is drawn), so a seeded run leaves the generator in the same state and every output
equals the host collate's, bit for bit.  Cloud sizes are known from shapes, so all cloud draws are made up front, then one
`umereg_collate_element` call per element is enqueued, then ONE device -> host read fetches the survivor counts that the match
draws need.  Match semantics are exact and stated in the header.  `collate_element_raw` takes caller-owned outputs and
workspace and never waits for the device."""
import numpy as np
import torch

from . import _lib
from .datasets.kitti_dataset import _refuse_gpu_in_worker

COLLATE_SIGNATURES = _lib.TABLES["umereg_collate.h"]
load_native = _lib.load
_ptr = _lib.ptr

# the dtypes the kernel gathers; a field of another dtype (a cache written elsewhere) is gathered with torch indexing instead
KERNEL_DTYPES = {"pts": torch.float32, "seg": torch.int64, "coords": torch.int32}


def workspace_bytes(ns, nt, n_matches):
    return int(_lib.load().umereg_collate_workspace_bytes(int(ns), int(nt), int(n_matches)))


def collate_element_raw(src, ns, tgt, nt, matches, keep_src, keep_tgt, b, out_src, out_tgt, out_matches, out_count, workspace):
    """Enqueue one element on the current stream.  src = (pts f32 [ns,3], seg i64 [ns], coords i32 [ns,3], pts_tform f32 [ns,3]),
    tgt = (pts, seg, coords) of nt points: contiguous device tensors, None for a field the caller gathers itself; matches i64 [m,2];
    keep_src / keep_tgt i64; out_src = (pts [n,3], seg [n], coords i32 [n,4], pts_tform [n,3]) and out_tgt = (pts, seg, coords): this
    element's slices of the batched outputs (None where the input is None); out_matches i64 [min(m, n_src, n_tgt), 2]; out_count
    i32 [2] (rows, error flag); workspace uint8 of >= workspace_bytes(ns, nt, m)."""
    m = matches.shape[0]
    _lib.call(keep_src.device, _lib.load().umereg_collate_element, *[_ptr(t) for t in src], int(ns), *[_ptr(t) for t in tgt], int(nt),
              matches.data_ptr() if m else None, m, keep_src.data_ptr(), keep_src.shape[0], keep_tgt.data_ptr(), keep_tgt.shape[0], int(b),
              *[_ptr(t) for t in out_src], *[_ptr(t) for t in out_tgt], out_matches.data_ptr() if out_matches.shape[0] else None,
              out_count.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(keep_src.device))


def _up(t, dev):
    """one field of one item on the device, as it is (one copy when it lives on the host)"""
    return torch.as_tensor(t).to(dev)


def _kernel_field(ts, kind):
    """the per-element tensors of one field if the kernel can gather them (every element has the contract's dtype), else None"""
    return [t.contiguous() for t in ts] if all(t.dtype == KERNEL_DTYPES[kind] for t in ts) else None


def batch_collate_fn_dset_device(data, num_matches, max_pc_size=100000, rng=np.random, device=None):
    """`batch_collate_fn_dset` (same contract, same 11-tuple, 13 with features, same dtypes and values, same consumption of `rng`)
    with every tensor on `device` (default: the device of the items, else the current HIP device) -- except gt_tform, which stays
    where the items have it when they all have it on the host.  Items may live on the host (each field is copied up once) or on
    the device.  Raises RuntimeError without a HIP device (there is no CPU fallback: use `batch_collate_fn_dset`), inside a DataLoader
    worker process (a forked worker must not open the GPU: use num_workers=0), and when a match or keep index is out of range."""
    who = "batch_collate_fn_dset_device"
    _refuse_gpu_in_worker(who)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a HIP device; umeregrobust_amd has no CPU fallback (the host collate is batch_collate_fn_dset)")
    if device is None:
        on_dev = [t.device for d in data for t in d if isinstance(t, torch.Tensor) and t.device.type == "cuda"]
        device = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    bs, with_feat = len(data), len(data[0]) > 9
    sizes = [(len(d[0]), len(d[3])) for d in data]
    n_src = min(min(s for s, _ in sizes), max_pc_size)                         # kitti_dataset.py:565-566
    n_tgt = min(min(t for _, t in sizes), max_pc_size)
    # every cloud draw, in the host collate's order (:571, :579): sizes are known from shapes, nothing waits for the device
    keeps = [(rng.choice(s, n_src, replace=False), rng.choice(t, n_tgt, replace=False)) for s, t in sizes]
    keep_src = torch.from_numpy(np.stack([k[0] for k in keeps]).astype(np.int64, copy=False)).to(dev)      # [bs, n_src], one copy
    keep_tgt = torch.from_numpy(np.stack([k[1] for k in keeps]).astype(np.int64, copy=False)).to(dev)

    cols = {i: [_up(d[i], dev) for d in data] for i in (0, 1, 2, 3, 4, 5, 6, 8)}    # field -> per-element device tensors
    sides = {"src": (cols[0], cols[1], cols[2], n_src, keep_src), "tgt": (cols[3], cols[4], cols[5], n_tgt, keep_tgt)}
    matches_in = [m.to(torch.int64).contiguous().reshape(-1, 2) for m in cols[8]]
    f32, i64, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)
    k_in, k_out = {}, {}                                                       # what the kernel gathers: inputs, batched outputs
    for name, (pts, seg, coords, n, _) in sides.items():
        k_in[name] = (_kernel_field(pts, "pts"), _kernel_field(seg, "seg"), _kernel_field(coords, "coords"))
        k_out[name] = (torch.empty(bs, n, 3, **f32) if k_in[name][0] else None, torch.empty(bs, n, **i64) if k_in[name][1] else None,
                       torch.empty(bs * n, 4, **i32) if k_in[name][2] else None)
    moved_in = _kernel_field(cols[6], "pts")
    moved_out = torch.empty(bs, n_src, 3, **f32) if moved_in else None
    cap = [min(len(m), n_src, n_tgt) for m in matches_in]                      # rows an element can keep at most
    rows = torch.empty(bs, max(max(cap), 1), 2, **i64)
    counts = torch.zeros(bs, 2, **i32)
    if n_src > 0 and n_tgt > 0:
        ws = torch.empty(max(workspace_bytes(s, t, len(m)) for (s, t), m in zip(sizes, matches_in)), dtype=torch.uint8, device=dev)
        pick = lambda fields, b: tuple(None if f is None else f[b] for f in fields)                       # noqa: E731
        for b in range(bs):
            s_out, t_out = k_out["src"], k_out["tgt"]
            out_src = (pick(s_out[:2], b) + (None if s_out[2] is None else s_out[2][b * n_src:(b + 1) * n_src],
                                             None if moved_out is None else moved_out[b]))
            out_tgt = pick(t_out[:2], b) + (None if t_out[2] is None else t_out[2][b * n_tgt:(b + 1) * n_tgt],)
            collate_element_raw(pick(k_in["src"], b) + (None if moved_in is None else moved_in[b],), sizes[b][0], pick(k_in["tgt"], b),
                                sizes[b][1], matches_in[b], keep_src[b], keep_tgt[b], b, out_src, out_tgt, rows[b, :cap[b]], counts[b], ws)

    def batched(name):
        """(pts, seg, coords, ones) of one side: the kernel's outputs, or the host collate's expressions on the device"""
        pts, seg, coords, n, keep = sides[name]
        o_pts, o_seg, o_coords = k_out[name]
        if o_pts is None:
            o_pts = torch.stack([p[keep[b]] for b, p in enumerate(pts)], dim=0)
        if o_seg is None:
            o_seg = torch.stack([s[keep[b]] for b, s in enumerate(seg)], dim=0)
        if o_coords is None:                                                   # sparse_collate: floor, int32, batch index in column 0
            parts = []
            for b, c in enumerate(coords):
                c = c[keep[b]]
                c = (torch.floor(c) if c.is_floating_point() else c).to(torch.int32)
                parts.append(torch.cat([torch.full((c.shape[0], 1), b, **i32), c], dim=1))
            o_coords = torch.cat(parts, dim=0)
        return o_pts, o_seg, o_coords, torch.ones(bs * n, 1, **f32)

    out_src, out_tgt = batched("src"), batched("tgt")
    if moved_out is None:
        moved_out = torch.stack([p[keep_src[b]] for b, p in enumerate(cols[6])], dim=0)
    got = counts.cpu().numpy()                                                 # THE device -> host read: [bs, 2]
    bad = np.flatnonzero(got[:, 1])
    if len(bad):
        raise RuntimeError(f"{who}: batch element {int(bad[0])} has a match index outside its clouds (or a keep index out of range)")
    kept = [int(c) for c in got[:, 0]]
    k = min(min(kept), num_matches)                                            # :606-607
    sel = np.stack([rng.choice(m, k, replace=False) for m in kept]).astype(np.int64, copy=False)           # one draw per element, k == 0 too
    matches = rows[torch.arange(bs, device=dev)[:, None], torch.from_numpy(sel).to(dev)]                    # [bs, k, 2]
    gts = [torch.as_tensor(d[7]) for d in data]
    if any(g.device.type != "cpu" for g in gts):
        gts = [g.to(dev) for g in gts]
    out = out_src + out_tgt + (moved_out, torch.stack(gts, dim=0), matches)
    if with_feat:
        out = out + tuple(torch.stack([_up(d[at], dev)[keep[b]] for b, d in enumerate(data)], dim=0)
                          for at, keep in ((9, keep_src), (10, keep_tgt)))
    return out
