"""The ball search's LDS plan and the inputs of tests/test_ball_search_edges_gpu.py, without a GPU.

(i)   tests/ball_cases.plan restates csrc/ball_search.h's lds_plan; a host program (tests/ball_plan_host.cpp, compiled here with the
      hipcc that builds the library) prints the header's own answer for every K = 1 .. kMaxBallK, and the two must agree line by line.
(ii)  The K list of the GPU tests straddles every switch of the plan.  A change of kSelRegs / kScanUnroll / the LDS budgets moves the
      switches and fails here, instead of silently moving them away from the K that are tested.
(iii) Every cloud the GPU tests search is what it claims: the oracle's linear scan finds exactly the constructed number of hits per
      ball, and keeps min(count, K) of them.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ball_cases as bc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's lds_plan cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("ball_plan") / "ball_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "ball_plan_host.cpp"), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, check=True, text=True).stdout.split("\n")
    head = lines[0].split()
    consts = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    rows = np.array([[int(v) for v in ln.split()] for ln in lines[1:] if ln], np.int64)
    return consts, rows


def test_plan_restates_the_header_for_every_K(header_plan):
    consts, rows = header_plan
    assert consts == dict(kSelRegs=bc.SEL_REGS, kScanUnroll=bc.SCAN_UNROLL, kMaxBallK=bc.MAX_K, kWave=bc.WAVE)
    assert np.array_equal(rows[:, 0], np.arange(1, bc.MAX_K + 1))
    mine = np.array([(K,) + bc.plan(K) for K in range(1, bc.MAX_K + 1)], np.int64)
    bad = np.nonzero((mine != rows).any(axis=1))[0]
    assert bad.size == 0, (rows[bad[:5]], mine[bad[:5]])


def test_gpu_K_list_straddles_every_switch_of_the_plan():
    plans = {K: bc.plan(K) for K in range(1, bc.MAX_K + 1)}
    first_lds = min(K for K, (cap, _) in plans.items() if cap > bc.SEL_REGS * bc.WAVE)
    first_2w = min(K for K, (_, w) in plans.items() if w == 2)
    first_1w = min(K for K, (_, w) in plans.items() if w == 1)
    # the switch points of today's constants (kSelRegs = 20, kScanUnroll = 4)
    assert (first_lds, first_2w, first_1w) == (961, 1473, 4033)
    assert plans[1] == plans[64] == (384, 4) and plans[750] == plans[960] == (1280, 4)
    assert plans[961] == (2112, 4) and plans[1472] == (3008, 4) and plans[1473] == (3136, 2)
    assert plans[4032] == (8128, 2) and plans[4033] == (8256, 1) and plans[bc.MAX_K] == (15424, 1)
    assert 15424 * 4 == 61696 <= 64 * 1024
    for edge in (first_lds, first_2w, first_1w):
        assert edge - 1 in bc.GPU_K and edge in bc.GPU_K, edge
    assert 1 in bc.GPU_K and bc.MAX_K in bc.GPU_K
    assert bc.in_registers(first_lds - 1) and not bc.in_registers(first_lds)
    # the register path with every register in use: cap_min == reg_cap
    kpad = (first_lds - 1 + 63) // 64 * 64
    assert kpad + (bc.SCAN_UNROLL + 1) * bc.WAVE == bc.SEL_REGS * bc.WAVE
    # the K of the directed tests lie on the plans they are meant for
    assert all(not bc.in_registers(K) for K in bc.VALU_K) and [bc.plan(K)[1] for K in bc.VALU_K] == [4, 2, 1]
    assert [bc.plan(K)[1] for K in bc.MANY_K] == [2, 2]
    assert [bc.plan(K)[1] for K in bc.PAIR_K] == [4, 2, 1]
    assert [bc.in_registers(K) for K in bc.TOP_K] == [True, True, False]


def test_counts_sit_on_the_comparisons():
    for K in bc.GPU_K:
        cap, _ = bc.plan(K)
        c = bc.counts_for(K, cap)
        assert len(set(c)) == len(c) and min(c) >= 0
        for v in (0, 1, K - 1, K, K + 1, cap - 4 * 64, cap - 4 * 64 + 1, cap - 2 * 64, cap - 2 * 64 + 1, cap, cap + 1, 2 * cap + K, 6 * cap):
            assert v in c, (K, v)
        j = 64
        while j <= K:
            assert j - 1 in c and j in c and j + 1 in c
            j *= 2


def _oracle_counts(cl, K):
    idx = orc.ball_query(cl.centres[None], cl.pts[None], K=K, radius=bc.R, return_nn=False).idx[0]
    return idx, (idx >= 0).sum(axis=1)


@pytest.mark.parametrize("case", bc.all_cases(), ids=lambda c: c.name)
def test_cloud_is_what_it_claims(case):
    cl = bc.build(case)
    assert cl.pts.dtype == np.float32 and cl.centres.dtype == np.float32 and cl.pts.shape[1] == 3
    _, found = _oracle_counts(cl, int(cl.counts.max()) + 1)             # K above every count: the constructed counts, exactly
    assert np.array_equal(found, cl.counts)
    idx, kept = _oracle_counts(cl, case.K)                              # the real K
    assert np.array_equal(kept, np.minimum(cl.counts, case.K))
    if cl.kp_index is not None:
        assert np.array_equal(cl.pts[cl.kp_index], cl.centres)
    if case.kwargs["order"] == "top":
        N = cl.pts.shape[0]
        top = N - 1
        assert top & (top - 1) == 0                                     # = 2^k
        assert idx[idx >= 0].min() >= top // 2                          # every hit index >= 2^(k-1)
        full, _ = _oracle_counts(cl, int(cl.counts.max()) + 1)
        assert top in full[0] and not (full[1:] == top).any()           # 2^k is a hit of query 0 alone
        assert (top in idx[0]) == (cl.counts[0] == case.K)              # kept with exactly K hits, the one dropped with K + 1
        assert cl.counts[0] in (case.K, case.K + 1)


def test_scan_and_reverse_orders_follow_the_walk():
    """In "scan" order the indices inside a ball ascend along (z layer, y row, x); "reverse" is its mirror image."""
    K = 750
    for order, sign in (("scan", 1), ("reverse", -1)):
        cl = bc.build(bc.edge_case(K, order))
        q = int(np.argmax(cl.counts))
        d2 = ((cl.pts.astype(np.float64) - cl.centres[q]) ** 2).sum(axis=1)
        hit = np.nonzero(d2 < bc.R ** 2)[0]                             # ascending index
        z = cl.pts[hit, 2]
        layer = np.floor((z - cl.pts[:, 2].min()) / np.float32(1.0001 * bc.R))
        assert (np.diff(layer) * sign >= 0).all() and layer.min() != layer.max()


def test_numpy_restatement_agrees_on_the_K750_cloud():
    cl = bc.build(bc.edge_case(750, "random"))
    ref = orc.ball_query(cl.centres[None], cl.pts[None], K=750, radius=bc.R, return_nn=False).idx[0]
    assert np.array_equal(orc.ball_query_numpy(cl.centres, cl.pts, 750, bc.R), ref)
