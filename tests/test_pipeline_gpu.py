"""RegistrationPipeline: the branches of submit / finish that only the benchmark used to run, each against `register_pair` on the
same clouds, keypoint indices and generator -- the drawn rows equal, every tensor bit for bit.  Smallest shapes of the existing
pipeline tests (N = 4096, 1024 keypoints, 256 samples); keypoints injected, one np.random.RandomState per pair."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_KP = 1024
TENSORS = ("match", "match_d", "ume_src", "ume_tgt", "rtume_tform")
_refs = {}


def _args(filt=True):
    return SimpleNamespace(ume_max_nn=750, ume_r_nn=5.0, filter_by_ume_dist_cond=filt, ume_n_samples=256, tau=0.05)


@pytest.fixture(scope="module")
def pairs(gpu):
    """seed -> (the four clouds [1,N,*] on the device, keypoint indices on the device, the same on the host)"""
    from umeregrobust_amd.synth import synth_pair
    out = {}
    for seed in (5, 6, 7):
        p = synth_pair(seed, N=4096, n_kp=N_KP)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
        out[seed] = SimpleNamespace(clouds=(t(p.src_pts)[None], t(p.tgt_pts)[None], t(p.src_feat)[None], t(p.tgt_feat)[None]),
                                    kw=dict(src_inds=t(p.src_inds), tgt_inds=t(p.tgt_inds)),
                                    host=dict(src_inds=p.src_inds, tgt_inds=p.tgt_inds))
    return out


def _host(c):
    return None if c is None else (c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c))


def _snap(o):
    """what a case compares, cloned at once: with graphs the tensors are the slot's buffers, valid until its next submit"""
    return SimpleNamespace(cond=_host(o.cond), g_index=o.g_index.clone(), **{k: getattr(o, k).clone() for k in TENSORS})


def _ref(pairs, seed, rng_seed, filt=True, cond=None):
    """register_pair's result for (pair, generator[, injected rows]); computed once, shared and left unchanged"""
    from umeregrobust_amd import evaluate
    key = (seed, rng_seed, filt, None if cond is None else cond.tobytes())
    if key not in _refs:
        e = pairs[seed]
        _refs[key] = _snap(evaluate.register_pair(*e.clouds, _args(filt), rng=np.random.RandomState(rng_seed), cond=cond, **e.host))
        torch.cuda.synchronize()
    return _refs[key]


def _same(o, r):
    assert (o.cond is None and r.cond is None) or np.array_equal(o.cond, r.cond)
    for k in TENSORS:
        assert torch.equal(getattr(o, k), getattr(r, k)), k


def _pipe(gpu, filt=True, **kw):
    from umeregrobust_amd import evaluate
    return evaluate.RegistrationPipeline(_args(filt), gpu, rng=None, **kw)


def test_slot_changes_between_plain_and_graph_path(gpu, pairs):
    """both slots serve timed pairs (plain launches), then untimed ones (the slot's graph), then timed ones again"""
    pipe = _pipe(gpu, depth=2, use_graphs="slot")
    for rnd, timed in enumerate((True, False, True)):
        hs = [pipe.submit(*pairs[s].clouds, timing={} if timed else None, rng=np.random.RandomState(10 * rnd + s), **pairs[s].kw)
              for s in (5, 6)]
        assert [h.slot for h in hs] == [0, 1]
        for h in hs:
            assert (getattr(h, "graph", None) is not None) == (not timed)
        outs = [_snap(pipe.finish(h)) for h in hs]
        torch.cuda.synchronize()
        for s, o in zip((5, 6), outs):
            _same(o, _ref(pairs, s, 10 * rnd + s))
    assert pipe.captures == 2


@pytest.mark.parametrize("as_tensor", [False, True])
def test_injected_cond_on_graph_slot(gpu, pairs, as_tensor):
    """rows given by the caller: a numpy array goes through the graph's own solve, a device tensor through _phase_b"""
    cond = np.random.RandomState(3).choice(N_KP, 256, replace=False).astype(np.int64)
    pipe = _pipe(gpu, depth=2, use_graphs="slot")
    for s in (5, 6):                                          # (the second pair: the slot's buffers exist already)
        h = pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(1), **pairs[s].kw)
        assert h.graph is not None
        o = _snap(pipe.finish(h, cond=torch.from_numpy(cond).to(gpu) if as_tensor else cond))
        torch.cuda.synchronize()
        _same(o, _ref(pairs, s, 1, cond=cond))
        assert torch.equal(o.g_index, torch.from_numpy(cond).to(gpu))


@pytest.mark.parametrize("use_graphs", [False, "slot"])
def test_no_weighted_draw(gpu, pairs, use_graphs):
    """filter_by_ume_dist_cond=False: no probabilities, no draw, one hypothesis per keypoint"""
    pipe = _pipe(gpu, filt=False, depth=2, use_graphs=use_graphs)
    for s in (5, 6, 7):
        h = pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(2), **pairs[s].kw)
        o = _snap(pipe.finish(h))
        torch.cuda.synchronize()
        assert o.rtume_tform.shape == (1, N_KP, 4, 4) and o.cond is None
        assert torch.equal(o.g_index, torch.arange(N_KP, device=gpu))
        _same(o, _ref(pairs, s, 2, filt=False))


@pytest.mark.parametrize("use_graphs", [False, "slot"])
def test_threaded_draw(gpu, pairs, use_graphs):
    """the weighted draw on the worker thread, three pairs in flight (which path serves them is not asserted)"""
    pipe = _pipe(gpu, depth=3, threaded_draw=True, use_graphs=use_graphs)
    try:
        for rnd in range(2):
            hs = [pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(20 + 3 * rnd + i), **pairs[s].kw)
                  for i, s in enumerate((5, 6, 7))]
            outs = [_snap(pipe.finish(h)) for h in hs]
            torch.cuda.synchronize()
            for i, (s, o) in enumerate(zip((5, 6, 7), outs)):
                _same(o, _ref(pairs, s, 20 + 3 * rnd + i))
    finally:
        pipe.pool.shutdown()


@pytest.mark.parametrize("use_graphs", [False, "slot"])
def test_order_caller_false_consumed_on_the_slot_stream(gpu, pairs, use_graphs):
    """order_caller=False leaves the caller's stream alone: the result is consumed under the slot's stream"""
    pipe = _pipe(gpu, depth=2, use_graphs=use_graphs)
    for s in (5, 6):
        ordered = _snap(pipe.finish(pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(30), **pairs[s].kw)))
        torch.cuda.synchronize()
        h = pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(30), **pairs[s].kw)
        o = pipe.finish(h, order_caller=False)
        with torch.cuda.stream(pipe.stream_of(h)):
            o = _snap(o)
        torch.cuda.synchronize()
        _same(o, ordered)
        _same(o, _ref(pairs, s, 30))


@pytest.mark.parametrize("use_graphs", [False, "slot"])
def test_order_caller_true_from_another_stream(gpu, pairs, use_graphs):
    """finish() orders the caller's CURRENT stream behind the slot's: clones enqueued there at once, with no host wait in between,
    see the finished results"""
    pipe = _pipe(gpu, depth=2, use_graphs=use_graphs)
    side = torch.cuda.Stream(gpu)
    assert all(side != st for st in pipe.streams)
    side.wait_stream(torch.cuda.current_stream(gpu))
    outs = []
    with torch.cuda.stream(side):
        for s in (5, 6, 7):
            outs.append(_snap_device(pipe.finish(pipe.submit(*pairs[s].clouds, rng=np.random.RandomState(40 + s), **pairs[s].kw))))
    torch.cuda.synchronize()
    for s, o in zip((5, 6, 7), outs):
        _same(o, _ref(pairs, s, 40 + s))


def _snap_device(o):
    """_snap without a device read: the drawn rows are on the host already"""
    return SimpleNamespace(cond=np.asarray(o.cond).copy(), **{k: getattr(o, k).clone() for k in TENSORS})
