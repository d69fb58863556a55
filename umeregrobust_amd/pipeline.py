"""The named hot path of one registration pair (reference evaluate.py:195-254) and its software pipeline.

`register_pair` is the body of the per-pair loop between feature extraction and hypothesis selection as a function, with the host RNG
made explicit so a caller can replay or inject the draws; `RegistrationPipeline` is the same computation overlapped over consecutive
pairs (one `_Slot` per pair in flight).  `phase_a_route` is the one place that says which form of a1-a5 a pair takes.  evaluate.py
imports every name back: `evaluate.register_pair` and the others are these objects.
"""
from types import MappingProxyType, SimpleNamespace

import numpy as np
import torch

from . import ops, streams as _streams
from .host_rng import choice_noreplace, choice_uniform_noreplace


class _PinnedRing:
    """Host -> device uploads of the loop's index arrays (keypoint draws, the weighted draw, the correlation sub-samples: 20-80 KB
    each, five per pair) and the download of the match probabilities, through a small ring of PINNED buffers: a copy out of pageable
    numpy memory blocks the host for 50-100 us (staging + synchronisation), a pinned one is an asynchronous enqueue.  A buffer is
    reused only after the event recorded behind its last copy has completed (a no-op wait in practice: a pair passes several host
    synchronisations before the ring comes round).  One ring per host thread (threading.local: the end-to-end legs run pairs on
    several threads) and per device (an event belongs to the device it was first recorded on)."""
    SLOTS = 8

    def __init__(self):
        self.buf = [None] * self.SLOTS
        self.ev = [None] * self.SLOTS
        self.k = 0

    def slot(self, nbytes):
        k = self.k = (self.k + 1) % self.SLOTS
        if self.ev[k] is not None:
            self.ev[k].synchronize()
        if self.buf[k] is None or self.buf[k].numel() < nbytes:
            self.buf[k] = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, pin_memory=True)
        return k, self.buf[k]

    def mark(self, k, dev):
        if self.ev[k] is None:
            self.ev[k] = torch.cuda.Event()
        self.ev[k].record(torch.cuda.current_stream(dev))


_ring_tls = __import__("threading").local()


def _ring(dev):
    rings = getattr(_ring_tls, "rings", None)
    if rings is None:
        rings = _ring_tls.rings = {}
    idx = torch.device(dev).index
    idx = torch.cuda.current_device() if idx is None else idx
    r = rings.get(idx)
    if r is None:
        r = rings[idx] = _PinnedRing()
    return r


def _index_tensor(idx, dev):
    """int64 index tensor on `dev`; numpy / list input goes up asynchronously through the pinned ring."""
    if isinstance(idx, torch.Tensor):
        return idx.to(device=dev, dtype=torch.int64)
    a = np.ascontiguousarray(np.asarray(idx), dtype=np.int64)
    dev = torch.device(dev)
    if dev.type != "cuda" or a.size < 256:
        return torch.as_tensor(a, dtype=torch.int64, device=dev)
    ring = _ring(dev)
    k, buf = ring.slot(a.nbytes)
    host = buf[:a.nbytes].view(torch.int64).view(a.shape)
    host.numpy()[...] = a
    out = torch.empty(a.shape, dtype=torch.int64, device=dev)
    out.copy_(host, non_blocking=True)
    ring.mark(k, dev)
    return out


def _to_host(t):
    """numpy copy of a device tensor through the pinned ring: asynchronous copy + a wait on its own event (a plain .cpu() takes
    the pageable path: tens of microseconds more per call)."""
    if not t.is_cuda:
        return t.detach().numpy()
    ring = _ring(t.device)
    k, buf = ring.slot(t.numel() * t.element_size())
    host = buf[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    host.copy_(t, non_blocking=True)
    ring.mark(k, t.device)
    ring.ev[k].synchronize()
    return host.numpy().copy()


NATIVE, STACKED, PER_CLOUD = "native", "stacked", "per_cloud"


def phase_a_route(args, timing, materialize_D, pair):
    """Which form of a1-a5 a pair takes.  NATIVE: the one native call (ops.pair_match_ragged; RegistrationPipeline replays the same
    chain as the slot's captured graph when it was built with use_graphs, draws on its own thread and runs on the current device) --
    for a pair the native entries can read in place (`pair`: its PairBatch), untimed (per-kernel events need the layered entry
    points), without the distance matrix, at the f16r matcher and without Hungarian matching.  Everything else goes through the
    layered launches: STACKED (both clouds as one batch of two) where the caller holds them stacked, PER_CLOUD otherwise.
    pair=True asks for a pair that is not built yet (register_pair builds one only for the native call)."""
    if pair is not None and timing is None and not materialize_D and ops.DEFAULT_MATCH_PRECISION == "f16r" \
            and not getattr(args, "hungarian_matching_flag", False):
        return NATIVE
    return STACKED if getattr(pair, "pts", None) is not None else PER_CLOUD


def _handle(ume_src, ume_tgt, match, match_d, prob, D, num_kpts, src_inds, tgt_inds, src_pts, tgt_pts, dev, **more):
    """The phase-A handle: what every form of a1-a5 hands to the draw and to phase B (`more`: match_src of the Hungarian matches,
    the pipeline's ready / slot / rng / draw / graph / keep)."""
    return SimpleNamespace(ume_src=ume_src, ume_tgt=ume_tgt, match=match, match_d=match_d, prob=prob, D=D, num_kpts=num_kpts,
                           src_inds=src_inds, tgt_inds=tgt_inds, src_pts=src_pts, tgt_pts=tgt_pts, dev=dev, **more)


def _phase_a(src_pts, tgt_pts, src_feat, tgt_feat, args, src_inds, tgt_inds, materialize_D=False, timing=None,
             pair=None, match_opts=None):
    """evaluate.py:195-236 up to the match probabilities: everything before the host RNG draw."""
    dev = src_pts.device
    where = (src_inds, tgt_inds, src_pts, tgt_pts, dev)
    # UME matrices (:206-212); the keypoint gathers src_pts[0, src_inds] (:201-202) are fused into the kernel
    t_mom = None if timing is None else timing.setdefault("moments", [])
    t_dist = None if timing is None else timing.setdefault("dist", ops.TimingList())
    route = phase_a_route(args, timing, materialize_D, pair)
    if route == NATIVE:
        # the whole of a1..a5 in one native call (same kernels as the layered path below), the two clouds read where they lie:
        # N_src != N_tgt is the normal case (kitti_dataset.py:568-569), nothing is stacked
        F, m_tgt, ume_d, prob = ops.pair_match_ragged(pair.src_pts, pair.tgt_pts, pair.src_feat, pair.tgt_feat, pair.inds[0], pair.inds[1],
                                                      args.ume_max_nn, args.ume_r_nn,
                                                      args.tau if args.filter_by_ume_dist_cond else None, opts=match_opts)
        return _handle(F[0:1], F[1:2], m_tgt, ume_d, prob, None, F.shape[1], *where)
    if route == STACKED:
        # (timed / layered calls) equally large clouds stacked by the caller: ONE batch of 2 through every kernel (same arithmetic
        # per cloud; half the launches, twice the parallelism for the small grid-building kernels)
        ume_both = ops.ume_moments(pair.pts, None, pair.feat, args.ume_max_nn, args.ume_r_nn, timing=t_mom,
                                   kp_index=pair.inds)
        ume_src, ume_tgt = ume_both[0:1], ume_both[1:2]
    else:
        ume_src = ops.ume_moments(src_pts, None, src_feat, args.ume_max_nn, args.ume_r_nn, timing=t_mom, kp_index=src_inds)
        ume_tgt = ops.ume_moments(tgt_pts, None, tgt_feat, args.ume_max_nn, args.ume_r_nn, timing=t_mom, kp_index=tgt_inds)
    num_kpts = min(ume_src.shape[1], ume_tgt.shape[1])
    ume_src = ume_src[:, :num_kpts]
    ume_tgt = ume_tgt[:, :num_kpts]
    # Matches (:215-225).  Hungarian matching (:216-222; off in every shipped config): by default the whole matrix goes to the
    # host, exactly like the reference: D -> scipy.optimize.linear_sum_assignment -> (src rows, tgt columns); with
    # args.assignment == "device" the solver of ops.linear_sum_assignment takes D where it lies
    D = None
    if getattr(args, "hungarian_matching_flag", False):
        assignment = getattr(args, "assignment", "host")
        if assignment not in ("host", "device"):
            raise ValueError(f"args.assignment must be 'host' or 'device', got {assignment!r}")
        D = ops.ume_cdist(ume_src, ume_tgt, timing=t_dist)
        if assignment == "device":
            m_src, m_tgt = ops.linear_sum_assignment(D[0:1])                                  # :219; [1, n] each
        else:
            from scipy.optimize import linear_sum_assignment
            src_m, tgt_m = linear_sum_assignment(D[0].cpu().numpy())                          # :219
            m_src = torch.from_numpy(src_m).long().to(dev)[None]                              # m[..., 0]
            m_tgt = torch.from_numpy(tgt_m).long().to(dev)[None]                              # m[..., 1]
        ume_d = D[0, m_src[0], m_tgt[0]][None]                                                # :234
        prob = ops.match_prob(ume_d[0], args.tau) if args.filter_by_ume_dist_cond else None
        return _handle(ume_src, ume_tgt, m_tgt, ume_d, prob, D if materialize_D else None, m_src.shape[1], *where, match_src=m_src)
    if materialize_D:
        D = ops.ume_cdist(ume_src, ume_tgt, timing=t_dist)
        m_tgt = D.min(dim=-1)[1]
        ume_d = torch.gather(D, 2, m_tgt.unsqueeze(-1)).squeeze(-1)
    else:
        m_tgt, ume_d = ops.ume_match(ume_src, ume_tgt, timing=t_dist, opts=match_opts)
    prob = ops.match_prob(ume_d[0], args.tau) if args.filter_by_ume_dist_cond else None   # (:235-236)
    return _handle(ume_src, ume_tgt, m_tgt, ume_d, prob, D, num_kpts, *where)


class PairBatch:
    """A registration pair as the native a1-a5 entries take it: the two clouds WHERE THEY LIE -- src_pts [N_src,3], tgt_pts [N_tgt,3],
    src_feat [N_src,32], tgt_feat [N_tgt,32], contiguous float32 on the device -- and the keypoint indices of both as the rows of
    one int64 [2,n_kp] tensor (row 0 = source).  N_src != N_tgt is the NORMAL case: the reference's collate dilutes source and target
    independently (datasets/kitti/kitti_dataset.py:568-569: min(len(cloud), max_pc_size) each, and the cached clouds are separately
    voxelised reconstructions), and its loop draws num_init_sel = min(10000, N_src, N_tgt) keypoints from EACH cloud
    (evaluate.py:195-204) -- so the sizes differ and vary pair to pair while the keypoint count is common to both.  Nothing is
    stacked or copied: the kernels read each cloud through a device-side record (ops.pair_match_ragged, ops.PairMatchCapGraph).

    PairBatch(pts, feat, inds) keeps the stacked form of earlier rounds -- pts [2,N,3], feat [2,N,32] -- for callers that hold
    equally large clouds in one tensor (`.pts` / `.feat` are then set, the per-cloud attributes are views of them)."""

    def __init__(self, pts, feat, inds):
        assert pts.dim() == 3 and pts.shape[0] == 2 and feat.shape[:2] == pts.shape[:2] and inds.shape[0] == 2
        self.pts, self.feat, self.inds = pts.contiguous(), feat.contiguous(), inds.contiguous().to(torch.int64)
        self.src_pts, self.tgt_pts, self.src_feat, self.tgt_feat = self.pts[0], self.pts[1], self.feat[0], self.feat[1]

    @property
    def sizes(self):
        """(N_src, N_tgt, n_kp)"""
        return self.src_pts.shape[0], self.tgt_pts.shape[0], self.inds.shape[1]

    def tensors(self):
        return (self.src_pts, self.tgt_pts, self.src_feat, self.tgt_feat, self.inds)

    def native(self):
        """(six device addresses, N_src, N_tgt) as umereg_pair_match_graph_launch_ragged takes them; cached -- a PairBatch is
        immutable once built (rebinding its tensors afterwards is not supported)."""
        na = getattr(self, "_native", None)
        if na is None:
            na = self._native = (self.src_pts.data_ptr(), self.tgt_pts.data_ptr(), self.src_feat.data_ptr(), self.tgt_feat.data_ptr(),
                                 self.inds.data_ptr(), self.inds.data_ptr() + 8 * self.inds.shape[1],
                                 self.src_pts.shape[0], self.tgt_pts.shape[0])
        return na

    @classmethod
    def from_clouds(cls, src_pts, tgt_pts, src_feat, tgt_feat, src_inds, tgt_inds):
        """The pair over the caller's own tensors ([1,N,*] or [N,*] clouds of any two sizes; NO copy of the clouds).  Returns None
        only for what the native entries cannot read in place (another dtype, a non-contiguous view, a host tensor) or for keypoint
        sets of different length -- the layered per-cloud path handles those."""
        cl = []
        for t_, w_ in ((src_pts, 3), (tgt_pts, 3), (src_feat, 32), (tgt_feat, 32)):
            if t_.dim() == 3 and t_.shape[0] == 1:
                t_ = t_[0]
            if not (t_.is_cuda and t_.dim() == 2 and t_.shape[1] == w_ and t_.dtype == torch.float32 and t_.is_contiguous()):
                return None
            cl.append(t_)
        if cl[2].shape[0] != cl[0].shape[0] or cl[3].shape[0] != cl[1].shape[0] or src_inds.numel() != tgt_inds.numel() \
                or src_inds.numel() == 0:
            return None
        base = getattr(src_inds, "_base", None)
        if base is not None and base is getattr(tgt_inds, "_base", None) and base.dim() == 2 and base.shape[0] == 2 \
                and base.is_contiguous() and src_inds.data_ptr() == base.data_ptr() and tgt_inds.data_ptr() == base[1].data_ptr():
            inds = base                   # the two index sets are the rows of one [2, n_kp] upload already (_draw_keypoints)
        else:
            inds = torch.stack([src_inds.view(-1), tgt_inds.view(-1)], 0)
        self = cls.__new__(cls)
        self.pts = self.feat = None
        self.src_pts, self.tgt_pts, self.src_feat, self.tgt_feat = cl
        self.inds = inds.contiguous().to(device=cl[0].device, dtype=torch.int64)
        return self


class PairResult(SimpleNamespace):
    """Namespace of one pair's results; the matched keypoint coordinates the reference materialises
    (evaluate.py:228-229, 240-241) are gathered only if somebody reads them."""

    @property
    def src_keypoint_pts(self):
        return self.src_pts[:, self.src_inds[:self.num_kpts]]

    @property
    def tgt_keypoint_pts(self):
        return self.tgt_pts[:, self.tgt_inds[:self.num_kpts]]

    @property
    def h_index(self):
        return self.match[0][self.g_index]

    @property
    def src_matches_keypoint_pts(self):
        return self.src_keypoint_pts[:, self.g_index]

    @property
    def tgt_matches_keypoint_pts(self):
        return self.tgt_keypoint_pts[:, self.h_index]


def _phase_b(a, args, cond):
    """evaluate.py:238-254: apply the drawn sub-sample and solve one SE(3) per kept match."""
    dev = a.dev
    if args.filter_by_ume_dist_cond:
        g_index = _index_tensor(cond, dev)          # m[:,0] is arange (:225), so src rows = cond itself
    else:
        g_index = None
    # Hypotheses (:248-254); the match gathers (:228-231, 243-244) are fused into the solve through the
    # match table (target row of source row g = match[g])
    if getattr(a, "match_src", None) is not None:
        # Hungarian matches: match k pairs source row match_src[k] with target row match[k] (for a square or wide D the
        # source rows are arange and this is the same table; explicit indices keep the tall case right)
        sel = g_index if g_index is not None else torch.arange(a.num_kpts, device=dev)
        T, _ = ops.rtume_solve(a.ume_src[0], a.ume_tgt[0], a.match_src[0][sel], a.match[0][sel])
    else:
        T, _ = ops.rtume_solve(a.ume_src[0], a.ume_tgt[0], g_index, None, h_of_g=a.match[0])
    out = PairResult(**vars(a))
    out.rtume_tform = T.view(1, -1, 4, 4)
    out.cond = cond
    out.g_index = g_index if g_index is not None else torch.arange(a.num_kpts, device=dev)
    return out


def _draw_keypoints_host(n_src, n_tgt, args, rng, src_inds=None, tgt_inds=None):
    """Keypoint draws (:195-204) on the host numpy RNG (unless injected) -> index arrays, nothing touches the device."""
    if args.filter_by_ume_dist_cond:
        num_init_sel = min(10000, min(n_src, n_tgt))
    else:
        num_init_sel = min(min(n_src, n_tgt), args.ume_n_samples)
    if src_inds is None:
        src_inds = choice_uniform_noreplace(rng, n_src, num_init_sel)
    if tgt_inds is None:
        tgt_inds = choice_uniform_noreplace(rng, n_tgt, num_init_sel)
    return src_inds, tgt_inds


def _draw_keypoints(src_pts, tgt_pts, args, rng, src_inds, tgt_inds):
    """Keypoint draws (:195-204): host numpy RNG unless injected; -> device index tensors."""
    src_inds, tgt_inds = _draw_keypoints_host(src_pts.shape[1], tgt_pts.shape[1], args, rng, src_inds, tgt_inds)
    if not isinstance(src_inds, torch.Tensor) and not isinstance(tgt_inds, torch.Tensor) and len(src_inds) == len(tgt_inds):
        both = _index_tensor(np.stack([np.asarray(src_inds), np.asarray(tgt_inds)]), src_pts.device)      # one upload: [2, n_kp]
        return both[0], both[1]
    return _index_tensor(src_inds, src_pts.device), _index_tensor(tgt_inds, src_pts.device)


def register_pair(src_pts, tgt_pts, src_feat, tgt_feat, args, rng=np.random, src_inds=None, tgt_inds=None,
                  cond=None, materialize_D=False, timing=None, after_phase_a=None):
    """The named hot path for one pair (reference evaluate.py:195-254).

    src_pts/tgt_pts [1,N,3], src_feat/tgt_feat [1,N,32] on the GPU.  Host-RNG draws mirror the
    reference's np.random.choice calls (:199-200, :238) and can be injected (src_inds, tgt_inds,
    cond) for replay.  Returns a namespace with rtume_tform [1,M,4,4] and the intermediates the
    downstream stages (hypothesis selection) need.
    after_phase_a: optional callable, invoked once a1-a5 are enqueued and before the host waits for the match probabilities: device
    work that does not depend on this function's results (the voxel thinning of the raw clouds, evaluate.prepare_selection) then
    runs while the host draws.  It must not consume `rng`.
    """
    assert src_pts.shape[0] == 1, "the reference evaluates with batch_size: 1"
    src_inds, tgt_inds = _draw_keypoints(src_pts, tgt_pts, args, rng, src_inds, tgt_inds)
    pair = None
    if phase_a_route(args, timing, materialize_D, True) == NATIVE:
        # both clouds -- of whatever two sizes the collate produced (kitti_dataset.py:568-569) -- through every kernel as ONE batch
        # of two and a1..a5 as one native call, read where they lie (no stacking copy; None for what cannot be: host tensors, ...)
        pair = PairBatch.from_clouds(src_pts, tgt_pts, src_feat, tgt_feat, src_inds, tgt_inds)
    a = _phase_a(src_pts, tgt_pts, src_feat, tgt_feat, args, src_inds, tgt_inds, materialize_D, timing, pair=pair)
    if after_phase_a is not None:
        a.side = after_phase_a()
    if args.filter_by_ume_dist_cond and cond is None:
        # tau-weighted sub-sampling of matches (:233-245): the draw consumes the HOST numpy RNG
        num_matches = min(a.num_kpts, args.ume_n_samples)
        cond = choice_noreplace(rng, a.num_kpts, num_matches, _to_host(a.prob))
    return _phase_b(a, args, cond)


class _Slot:
    """What one pipeline slot owns: its stream (+ raw pointer) and reusable ready event, the pinned buffer the match probabilities
    come down into, the pinned buffer (+ cached numpy view) the drawn rows go up through with the slot's device index buffer and
    the event behind the last torch copy out of it, the T buffer of the graph path, the in-flight flag (a submitted pair whose
    finish() has not run yet) and the slot's graphs, most recently used last (one per keypoint count; <= 2).  Every buffer is
    made on first use and again when the size changes, whichever path -- plain launches or the graph -- the slot serves."""
    __slots__ = ("stream", "stream_ptr", "ready", "host_prob", "host_cond", "host_cond_np", "cond_dev", "cond_uploaded", "T",
                 "in_flight", "graphs")

    def __init__(self, stream):
        self.stream, self.stream_ptr, self.ready = stream, stream.cuda_stream, torch.cuda.Event()
        self.host_prob = self.host_cond = self.host_cond_np = self.cond_dev = self.cond_uploaded = self.T = None
        self.in_flight, self.graphs = False, []

    def prob_buffer(self, n):
        if self.host_prob is None or self.host_prob.numel() != n:
            self.host_prob = torch.empty(n, dtype=torch.float32, pin_memory=True)
        return self.host_prob

    def T_buffer(self, n, dev):
        if self.T is None or self.T.shape[0] != n:
            self.T = torch.empty((n, 4, 4), dtype=torch.float32, device=dev)
        return self.T

    def upload(self, c, dev, ready=None, own=False):
        """The drawn rows `c` (int64 numpy) through the slot's pinned buffer (a pageable-source copy blocks the host for tens of
        microseconds) -> their device tensor.  The previous copy out of the buffer must be done before it is overwritten: the event
        behind the last torch copy is waited for, and a caller that has not waited for this pair's `ready` since (injected rows; a
        host draw has) passes it -- it lies behind the slot's previous pair, whose copy may have run inside graph.solve.
        own: the tensor is the slot's device buffer and the copy is left to the caller's graph.solve (copy + solve in one native
        call, no per-pair allocation); otherwise a fresh tensor, copied here on the slot's stream (the current one)."""
        if self.cond_uploaded is not None:
            self.cond_uploaded.synchronize()
            self.cond_uploaded = None
        if ready is not None:
            ready.synchronize()
        if self.host_cond is None or self.host_cond.numel() != c.size:
            self.host_cond = torch.empty(c.size, dtype=torch.int64, pin_memory=True)
            self.host_cond_np, self.cond_dev = self.host_cond.numpy(), None
        self.host_cond_np[:] = c
        if own:
            if self.cond_dev is None:
                self.cond_dev = torch.empty(c.size, dtype=torch.int64, device=dev)
            return self.cond_dev
        out = self.host_cond.to(dev, non_blocking=True)
        self.cond_uploaded = torch.cuda.Event()
        self.cond_uploaded.record(self.stream)
        return out


class RegistrationPipeline:
    """Same computation as register_pair, software-pipelined over consecutive pairs.

    The reference draws the match sub-sample on the host (np.random.choice with p from the device,
    evaluate.py:238): a device -> host -> device round trip in the middle of every pair.  Here phase A of
    pair i+1 (moments, matching, probabilities: one native call) is enqueued on another HIP stream before
    the host draws for pair i, so the draw overlaps GPU work, and the streams are not ordered against
    each other, so the single-workgroup kernels of one pair run beside the machine-filling kernels of the
    other.  Results are identical to register_pair given the same RNG stream; `submit` and `finish` must
    be called in order.
    """

    def __init__(self, args, device, depth=2, rng=np.random, threaded_draw=False, use_graphs=False, stream_plan=None,
                 match_opts=None, capacity=None):
        """threaded_draw: run the host draw (event wait + choice) on one worker thread, in submission
        order, so it also overlaps the main thread's kernel enqueues (the native draw releases the GIL).
        Use depth >= 3 with it.  The worker is then the only consumer of `rng` between submit and finish,
        so inject the keypoint indices (or draw them from a different generator)."""
        self.args, self.rng, self.depth = args, rng, depth
        self.match_opts = match_opts       # ops.MatchOpts of THIS pipeline's matcher calls (per call, not process state)
        # use_graphs ("slot"; True / "pair" are accepted as the same thing): phase A (13 launches) as ONE hipGraph per pipeline slot,
        # captured once at a CAPACITY -- clouds of up to `capacity` points (default: args.max_pc_size, the collate's bound,
        # kitti_dataset.py:568-569; grown on demand) and the keypoint count of the first pair -- whose kernels read each submitted
        # pair's clouds WHERE THEY LIE through a 64-byte device record (ops.PairMatchCapGraph).  What a loop over distinct pairs of
        # varying size (reference evaluate.py:175: 1 475 of them, N_src != N_tgt) needs: a new pair, of whatever shape that fits, is
        # a record write + a replay -- no re-capture, no staging copy, no dependence on where the caller keeps its tensors.  Only a
        # cloud beyond the capacity or another keypoint count (min(10000, N_src, N_tgt): clouds below 10 000 points) captures anew.
        # The graph writes into buffers it owns: a pair's phase-A outputs, rtume_tform and g_index (slot buffers) are valid until the
        # slot's next submit / finish: consume or clone them before submitting `depth` more pairs.
        if use_graphs not in (False, True, "pair", "slot"):
            raise ValueError(f"use_graphs must be False, True / 'pair' or 'slot' (got {use_graphs!r})")
        self.use_graphs = "slot" if use_graphs else False
        self.capacity = int(capacity) if capacity else int(getattr(args, "max_pc_size", 0) or 0)
        self.graphs = MappingProxyType({})   # (kept empty: the per-(slot, PairBatch) graphs of rounds 2-5 are gone)
        self.captures = 0                # graphs captured so far (a stream of pairs that fit the capacity: `depth`)
        self.pool = None
        if threaded_draw:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="umereg-draw")
        self.dev = torch.device(device)
        # Which slot streams share a HARDWARE QUEUE decides how the pairs' kernels overlap: the HIP runtime multiplexes all streams of the
        # process onto four queues by a rule a caller cannot read back, and two streams on one queue run strictly one after the other
        # (all slots on one queue 2 820 pairs/s, KT shape; a slot on the NULL stream's queue costs ~10 %).  Rounds 3-5 steered that by
        # creation order ("sd": a spacer stream behind every slot stream) -- which holds only until the process creates one stream more
        # somewhere else (BENCH r05 -> r06: evaluate_pairs 446 -> 375 pairs/s on unchanged code).  Now the slot streams are CHOSEN BY
        # MEASUREMENT (streams.concurrent_streams: a spin kernel on one stream, a one-thread kernel on the other): consecutive slots on
        # different queues, none on the null stream's.  stream_plan = a string of 's' / 'd' keeps the creation-order form (bench.py times
        # both after every run: config.stream_plan_check).
        self.streams, self._spacers = [], []
        self.stream_plan = stream_plan or "measured"
        with torch.cuda.device(self.dev):
            if stream_plan in (None, "measured", "auto"):
                self.streams = list(_streams.concurrent_streams(self.dev, depth))
            else:
                for tok in stream_plan + "s" * depth:           # 's' = the next slot's stream, 'd' = a spacer
                    if tok == "s" and len(self.streams) >= depth:
                        continue
                    s_ = torch.cuda.Stream(self.dev)
                    s_.cuda_stream                          # creates the HIP stream now
                    (self.streams if tok == "s" else self._spacers).append(s_)
        self.slots = [_Slot(s_) for s_ in self.streams]
        self.n_submitted = 0

    @property
    def slot_graphs(self):
        """read-only: slot -> [PairMatchCapGraph, ...] of the slots that have captured"""
        return MappingProxyType({k: s.graphs for k, s in enumerate(self.slots) if s.graphs})

    def submit(self, src_pts, tgt_pts, src_feat, tgt_feat, src_inds=None, tgt_inds=None, timing=None, pair=None, rng=None):
        """pair: optional PairBatch holding the same clouds/keypoints as a batch of 2 (then the per-cloud
        arguments are only used for their shapes and as views for downstream consumers).
        rng: numpy generator for THIS pair's draws (default: the pipeline's)."""
        k = self.n_submitted % self.depth
        s = self.slots[k]
        if s.in_flight:
            raise RuntimeError(f"RegistrationPipeline: slot {k} still holds an unfinished pair -- at most depth={self.depth} "
                               "pairs may be submitted before their finish() (its pinned buffers would be overwritten)")
        a = self._submit_slot(k, s, src_pts, tgt_pts, src_feat, tgt_feat, src_inds, tgt_inds, timing, pair, rng)
        # the slot is taken only once the pair is really enqueued: a submit that raised (graph capture, a bad argument, the
        # host-side Hungarian step) leaves the pipeline usable
        s.in_flight = True
        self.n_submitted += 1
        return a

    def _slot_graph(self, s, pair):
        """The slot's capacity graph for a pair of these sizes; captured when none of the slot's graphs fits (first use, a cloud
        beyond the capacity, another keypoint count)."""
        args = self.args
        tau = args.tau if args.filter_by_ume_dist_cond else None
        n_src, n_tgt, n_kp = pair.sizes
        lst = s.graphs
        for g in lst:
            if g.fits(n_src, n_tgt, n_kp, args.ume_max_nn, args.ume_r_nn, tau, self.match_opts):
                if g is not lst[-1]:
                    lst.remove(g); lst.append(g)
                return g
        need = max(n_src, n_tgt)
        if need > self.capacity:
            self.capacity = (need + need // 8 + 1023) // 1024 * 1024       # (headroom: the next pair is a few per cent larger or smaller)
        if len(lst) >= 2:
            s.stream.synchronize()                # the old exec may still be running on the slot's stream
            lst.pop(0)
        with torch.cuda.stream(s.stream):
            # buffers owned by the graph are allocated under the slot's stream: that is the stream its kernels run on, so
            # the caching allocator cannot hand them to somebody else while a replay is in flight
            g = ops.PairMatchCapGraph(self.dev, self.capacity, n_kp, args.ume_max_nn, args.ume_r_nn, tau, opts=self.match_opts)
        lst.append(g)
        self.captures += 1
        return g

    def _submit_slot(self, k, s, src_pts, tgt_pts, src_feat, tgt_feat, src_inds, tgt_inds, timing, pair, rng):
        st = s.stream
        rng = rng if rng is not None else self.rng
        if pair is not None:
            src_inds, tgt_inds = pair.inds[0], pair.inds[1]
        else:
            src_inds, tgt_inds = _draw_keypoints(src_pts, tgt_pts, self.args, rng, src_inds, tgt_inds)
            if timing is None:
                # the pair over the caller's own tensors (no copy of the clouds, whatever their two sizes): the one-call / graph path
                pair = PairBatch.from_clouds(src_pts, tgt_pts, src_feat, tgt_feat, src_inds, tgt_inds)
        st.wait_stream(torch.cuda.current_stream(self.dev))
        # (no ordering between the phase-A blocks of consecutive pairs: the single-workgroup kernels of one pair --
        # keypoint order, grid scan, softmax, RTUME -- then run beside the machine-filling kernels of the other:
        # 0.416 -> 0.36 ms per pair)
        if self.use_graphs and self.pool is None and phase_a_route(self.args, timing, False, pair) == NATIVE \
                and torch.cuda.current_device() == self.dev.index:
            # graph fast path: record write + replay + probability download in one native call on the slot's stream, no torch stream /
            # device contexts, a per-slot event (the host side of a pair is as long as its GPU side: every 10 us count)
            graph = self._slot_graph(s, pair)
            hp = s.prob_buffer(graph.prob.numel()) if graph.prob is not None else None
            graph.launch_native(pair.native(), hp.data_ptr() if hp is not None else 0, s.stream_ptr)
            s.ready.record(st)
            # the replay reads the caller's tensors on the SLOT's stream: the handle holds them (`keep`) until finish() has waited for
            # `ready` (recorded behind the replay's last kernel), so a caller that rebinds `pair` right after submit() cannot have the
            # caching allocator hand the blocks out on its own stream while the kernels are pending
            return _handle(graph.F[0:1], graph.F[1:2], graph.m, graph.d, graph.prob, None, graph.F.shape[1], src_inds, tgt_inds,
                           src_pts, tgt_pts, self.dev, ready=s.ready, slot=k, rng=rng, draw=None, graph=graph,
                           keep=(pair, src_feat, tgt_feat))
        with torch.cuda.stream(st):
            a = _phase_a(src_pts, tgt_pts, src_feat, tgt_feat, self.args, src_inds, tgt_inds, False, timing, pair,
                         match_opts=self.match_opts)
            if a.prob is not None:
                s.prob_buffer(a.prob.numel()).copy_(a.prob, non_blocking=True)
            a.ready = torch.cuda.Event()
            a.ready.record(st)
        a.slot, a.rng, a.draw = k, rng, None
        a.keep =(pair, src_pts, tgt_pts, src_feat, tgt_feat)     # read on the slot's stream, possibly allocated on another: alive until finish()
        if self.pool is not None and self.args.filter_by_ume_dist_cond:
            a.draw = self.pool.submit(self._draw, a)
        return a

    def _draw(self, a):
        a.ready.synchronize()
        num_matches = min(a.num_kpts, self.args.ume_n_samples)
        return choice_noreplace(a.rng, a.num_kpts, num_matches, self.slots[a.slot].host_prob.numpy())

    def finish(self, a, cond=None, order_caller=True):
        """Host draw (or the injected `cond`) + phase B of pair `a` on its slot's stream.  The CALLER'S current stream is made
        to wait for that stream (no host synchronisation), so the returned tensors can be consumed with ordinary torch
        semantics.  A caller that consumes them under `with torch.cuda.stream(pipe.stream_of(a))` only -- bench.py's loop --
        passes order_caller=False and saves the event record / wait and the allocator bookkeeping (~15 us of host time).
        With use_graphs the phase-A outputs (ume_src/ume_tgt, match, match_d, prob) are buffers owned by the slot's graph:
        valid until the slot's next submit."""
        st = self.streams[a.slot]
        if not order_caller:
            return self._finish_on_slot(a, cond, st)
        caller = torch.cuda.current_stream(self.dev)
        out = self._finish_on_slot(a, cond, st)
        if caller != st:
            caller.wait_stream(st)
            for t_ in (out.rtume_tform, getattr(out, "g_index", None)):
                if isinstance(t_, torch.Tensor):
                    t_.record_stream(caller)          # allocated on the slot's stream, read on the caller's
        return out

    def _finish_on_slot(self, a, cond, st):
        s = self.slots[a.slot]
        if not s.in_flight:
            raise RuntimeError("RegistrationPipeline.finish: this pair was already finished")
        s.in_flight = False
        injected, filt = cond is not None, self.args.filter_by_ume_dist_cond
        if filt and cond is None:
            cond = a.draw.result() if a.draw is not None else self._draw(a)
        # the pair's inputs were read on the slot's stream: after a host draw the host has waited for `ready` (behind those reads) and
        # the handle's hold on them can simply go; otherwise (no weighted draw, or an injected `cond`) the allocator is told
        keep, a.keep = getattr(a, "keep", None), None
        if keep and (injected or not filt):
            for t_ in keep:
                for u_ in (t_.tensors() if isinstance(t_, PairBatch) else (t_,)):
                    if isinstance(u_, torch.Tensor) and u_.is_cuda:
                        u_.record_stream(st)
        del keep
        graph = getattr(a, "graph", None)
        # rows on the host (drawn or injected) go up through the slot's pinned buffer; a device tensor is taken as it is
        c = np.asarray(cond, dtype=np.int64) if filt and not isinstance(cond, torch.Tensor) else None
        if graph is not None and not isinstance(cond, torch.Tensor):
            # graph fast path: index upload + SE(3) solve from the graph's own outputs in one native call.  T and the index tensor are
            # the slot's buffers (no per-pair allocation / cross-stream allocator bookkeeping): like the graph's own outputs they are
            # valid until the slot's next finish
            out = PairResult(**vars(a))
            n = c.size if c is not None else a.num_kpts
            T = s.T_buffer(n, self.dev)
            if c is not None:
                out.cond, out.g_index = c, s.upload(c, self.dev, a.ready if injected else None, own=True)
                graph.solve(s.host_cond.data_ptr(), n, out.g_index, T, s.stream_ptr)
            else:
                graph.solve(0, n, None, T, s.stream_ptr)
                out.cond, out.g_index = cond, torch.arange(n, device=self.dev)
            out.rtume_tform = T.view(1, n, 4, 4)
            return out
        with torch.cuda.stream(st):
            if c is not None:
                out = _phase_b(a, self.args, s.upload(c, self.dev, a.ready if injected else None))
                out.cond = c
                return out
            return _phase_b(a, self.args, cond)

    def stream_of(self, a):
        return self.streams[a.slot]
