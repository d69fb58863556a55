"""The ball search's streaming top-K (csrc/ball_search.h) at every edge of its LDS plan, on clouds whose balls hold a PRESCRIBED number
of points (tests/ball_cases.py; tests/test_ball_plan_cpu.py shows, without a GPU, that the clouds are what they claim and that the K
below straddle every switch of lds_plan).

Within one plan a selection can be off by one in `make_room` (cnt > cap - chunks * 64), the final `cnt > K`, `below < K` / `v <= t` of
the register form, `need > zeros` of the radix form, the `oi <= thr` drop after a selection, the power-of-two padding of sort_kept and
the highest index bit in `nbits`; across plans, in the register -> LDS switch (K = 960 | 961) and in the slot arithmetic of workgroups
of 4, 2 (K = 1 473 .. 4 032) and 1 (.. 7 680 = kMaxBallK) wavefronts.  A ball that keeps K - 1 indices, or the wrong K-th one, moves F by
~1/K: far below what an end-to-end test sees, far above the a2 bar.

Every comparison is against the oracle's linear scan (orc.ball_query) / its fp64 moments (orc.ume_moments(..., "f64")): indices, dists
and neighbours with ==, F within 3e-7 of the matrix' largest entry (the project's a2 bar, BASELINE.json north_star).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import ball_cases as bc
from tests.test_gpu_parity import N_, T_

pytestmark = pytest.mark.gpu

A2_BAR = 3e-7


def _reference(case):
    """(cloud, features, oracle ball query, oracle fp64 moments) of a case: computed once, shared, never written to."""
    return _reference_of(case.name, case.K, tuple(sorted(case.kwargs.items())))


@functools.lru_cache(maxsize=2)
def _reference_of(name, K, items):
    case = bc.Case(name, K, dict(items))
    cl = bc.build(case)
    feat = bc.features(cl.pts.shape[0], case.K)
    bq = orc.ball_query(cl.centres[None], cl.pts[None], K=case.K, radius=bc.R, return_nn=True)
    F64 = orc.ume_moments(cl.pts, cl.centres, feat, case.K, bc.R, "f64")
    for a in (bq.idx, bq.dists, bq.knn, F64):
        a.setflags(write=False)
    return cl, feat, bq, F64


def _check_ball_query(gpu, case, lengths2=None):
    from umeregrobust_amd import ops
    cl, _, ref, _ = _reference(case)
    l2 = None
    if lengths2 is not None:
        l2 = T_(np.array([lengths2], np.int64), gpu)
        ref = orc.ball_query(cl.centres[None], cl.pts[None], None, [lengths2], K=case.K, radius=bc.R, return_nn=True)
    out = ops.ball_query(T_(cl.centres, gpu)[None], T_(cl.pts, gpu)[None], None, l2, K=case.K, radius=bc.R, return_nn=True)
    idx = N_(out.idx)
    bad = np.nonzero((idx != ref.idx).any(axis=-1)[0])[0]
    assert bad.size == 0, (case.name, "ball_query rows", bad[:8], "hits", cl.counts[bad[:8]], "kept", (idx[0][bad[:8]] >= 0).sum(-1))
    assert np.array_equal(N_(out.dists), ref.dists)
    assert np.array_equal(N_(out.knn), ref.knn)
    return ref


def _check_moments(gpu, case, valu=False):
    from umeregrobust_amd import ops
    cl, feat, ref, F64 = _reference(case)
    p, c, f = T_(cl.pts, gpu)[None], T_(cl.centres, gpu)[None], T_(feat, gpu)[None]
    F, cnt, idx = ops.ume_moments(p, c, f, case.K, bc.R, return_count=True, return_idx=True)
    got = N_(idx)[0]
    bad = np.nonzero((got != ref.idx[0]).any(axis=-1))[0]
    assert bad.size == 0, (case.name, "moments rows", bad[:8], "hits", cl.counts[bad[:8]], "kept", (got[bad[:8]] >= 0).sum(-1))
    assert np.array_equal(N_(cnt)[0], np.minimum(cl.counts, case.K))
    scale = np.abs(F64).max(axis=(1, 2), keepdims=True) + 1e-30
    err = (np.abs(N_(F[0]).astype(np.float64) - F64) / scale).max()
    print(f"{case.name}: F max err / row max = {err:.3e}")
    assert err < A2_BAR, (case.name, err)
    if valu:
        Fv, cv, iv = ops.ume_moments(p, c, f, case.K, bc.R, return_count=True, return_idx=True, acc="f64valu")
        assert torch.equal(Fv, F) and torch.equal(cv, cnt) and torch.equal(iv, idx), (case.name, (Fv != F).sum().item())


# ------------------------------------------------------------------------------------------------ plan edges
@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("K", bc.GPU_K)
def test_plan_edges(gpu, K, order):
    """Both sides of every switch of lds_plan (registers | LDS radix passes at 960 | 961; 4 | 2 | 1 wavefronts per workgroup at 1 472 |
    1 473 and 4 032 | 4 033), K = 1 and kMaxBallK, balls of counts_for(K, cap) hits in three index orders: ball query and fused moments."""
    case = bc.edge_case(K, order)
    _check_ball_query(gpu, case)
    _check_moments(gpu, case, valu=K in bc.VALU_K)


# ------------------------------------------------------------------------------------------------ more queries than a workgroup's waves
@pytest.mark.parametrize("K", bc.MANY_K)
def test_two_wave_workgroups_many_queries(gpu, K):
    """131 queries with two wavefronts per workgroup: an odd count (the last workgroup is half empty), >= 64 (the moment kernel takes its
    keypoints in cell order, eight XCD slabs of 66 workgroups: 8 does not divide 66), balls around K and cap."""
    assert bc.plan(K)[1] == 2 and bc.N_MANY % 2 == 1 and bc.N_MANY >= 64
    case = bc.many_case(K)
    _check_ball_query(gpu, case)
    _check_moments(gpu, case)


# ------------------------------------------------------------------------------------------------ dense sweep at the reference's K
def test_dense_sweep_K750(gpu):
    """K = 750 (the reference's), one ball for every count in [K - 2, K + 2] and [cap - 300, cap + 44]: every equality of make_room (four-
    and two-chunk trips, whatever the rows' lengths) is met by some ball."""
    case = bc.dense_case()
    assert len(case.kwargs["counts"]) == 350
    _check_ball_query(gpu, case)
    _check_moments(gpu, case)


# ------------------------------------------------------------------------------------------------ small counts
@pytest.mark.parametrize("K", [750, 64])
def test_small_counts(gpu, K):
    """0 .. 72 hits: with K = 750 nothing saturates and every tail length of the accumulation's 8- / 32-neighbour trips occurs once; with
    K = 64 the counts cross saturation."""
    case = bc.small_case(K)
    _check_ball_query(gpu, case)
    _check_moments(gpu, case)


# ------------------------------------------------------------------------------------------------ highest index bit
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("bits", bc.TOP_BITS)
@pytest.mark.parametrize("K", bc.TOP_K)
def test_highest_index_bit(gpu, K, bits, extra):
    """N = 2^bits + 1: index 2^bits alone needs the selection's highest bit.  Its ball has K hits (it must be kept) or K + 1 (it is the
    largest and must be the one dropped); every other hit index is >= 2^(bits-1)."""
    case = bc.top_case(K, bits, extra)
    ref = _check_ball_query(gpu, case)
    assert ((1 << bits) in ref.idx[0, 0]) == (extra == 0)
    _check_moments(gpu, case)


# ------------------------------------------------------------------------------------------------ lengths2
@pytest.mark.parametrize("K", bc.LENGTHS_K)
def test_lengths2_halves_every_ball(gpu, K):
    """lengths2 = N // 2 on the random-order clouds: the cut halves every ball and seeds the search's threshold."""
    case = bc.edge_case(K, "random")
    N = bc.build(case).pts.shape[0]
    ref = _check_ball_query(gpu, case, lengths2=N // 2)
    assert ref.idx.max() < N // 2 and (ref.idx[0] >= 0).sum(-1).max() == K


# ------------------------------------------------------------------------------------------------ the pair chain
@pytest.mark.parametrize("K", bc.PAIR_K)
def test_pair_chain(gpu, K):
    """a1..a5 of a ragged pair at the LDS plans (4, 2, 1 wavefronts), keypoints as indices: F equals the per-cloud calls bit for bit and
    the matches are ume_match's on them (what test_ragged_pair_one_call_equals_the_per_cloud_calls asserts at K = 750); the per-cloud
    neighbourhoods are the oracle's."""
    from umeregrobust_amd import ops
    src, tgt = bc.build(bc.pair_case(K, 0)), bc.build(bc.pair_case(K, 1))
    assert src.pts.shape[0] != tgt.pts.shape[0]
    fs, ft = bc.features(src.pts.shape[0], K), bc.features(tgt.pts.shape[0], K + 1)
    sp, tp, sf, tf = T_(src.pts, gpu), T_(tgt.pts, gpu), T_(fs, gpu), T_(ft, gpu)
    si, ti = T_(src.kp_index, gpu), T_(tgt.kp_index, gpu)
    F, m, d, prob = ops.pair_match_ragged(sp, tp, sf, tf, si, ti, K, bc.R, tau=0.05)
    Fs, cs = ops.ume_moments(sp[None], None, sf[None], K, bc.R, kp_index=si, return_count=True)
    Ft, ct = ops.ume_moments(tp[None], None, tf[None], K, bc.R, kp_index=ti, return_count=True)
    assert torch.equal(F[0], Fs[0]) and torch.equal(F[1], Ft[0]), ((F[0] != Fs[0]).sum().item(), (F[1] != Ft[0]).sum().item())
    m2, d2 = ops.ume_match(Fs, Ft)
    assert torch.equal(m, m2) and torch.equal(d, d2) and torch.equal(prob, ops.match_prob(d2[0], 0.05))
    for cl, feat, p, f, ki, Fg, cg in ((src, fs, sp, sf, si, Fs, cs), (tgt, ft, tp, tf, ti, Ft, ct)):
        assert np.array_equal(N_(cg)[0], np.minimum(cl.counts, K))
        idx = ops.ume_moments(p[None], None, f[None], K, bc.R, kp_index=ki, return_idx=True)[1]
        assert np.array_equal(N_(idx)[0], orc.ball_query(cl.centres[None], cl.pts[None], K=K, radius=bc.R, return_nn=False).idx[0])
        F64 = orc.ume_moments(cl.pts, cl.centres, feat, K, bc.R, "f64")
        scale = np.abs(F64).max(axis=(1, 2), keepdims=True) + 1e-30
        err = (np.abs(N_(Fg[0]).astype(np.float64) - F64) / scale).max()
        print(f"pair K={K}: F max err / row max = {err:.3e}")
        assert err < A2_BAR
