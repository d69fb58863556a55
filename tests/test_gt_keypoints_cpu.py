"""CPU: the device-side keypoint selection without a GPU -- the header's place in the one ABI (tests/test_abi.py checks
include/umereg_gt_keypoints.h against its table), the entries' refusals without a device, the `selection=` keyword on its call paths, and the numpy
restatement the GPU tests judge the kernels by (tests/gt_keypoints_cases.py): pinned against oracle.generate_ume_from_keypoints2 on
every edge cloud, each of which is shown to sit on the edge it is named for."""
import inspect
import os

import numpy as np
import pytest
import torch

import abi_headers
import gt_keypoints_cases as gc
from oracle import oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_HEADER = os.path.join(abi_headers.INCLUDE, "umereg_gt_keypoints.h")
CASES = gc.all_cases()


@pytest.fixture(scope="module")
def lib():
    from umeregrobust_amd import gt_keypoints
    return gt_keypoints.load_native()


# ---- 1. the header's place, constants --------------------------------------------------------------------------------------------------

def test_the_header_is_one_of_include_s_and_its_table_is_the_package_s(lib):
    from umeregrobust_amd import _build, _lib, gt_keypoints
    assert gt_keypoints.GT_KEYPOINTS_SIGNATURES is _lib.TABLES["umereg_gt_keypoints.h"] and gt_keypoints.load_native is _lib.load
    assert len(os.listdir(abi_headers.INCLUDE)) == len(abi_headers.HEADERS) == len(_lib.TABLES)      # the number: tests/test_abi.py
    assert API_HEADER in _build.headers()                                          # part of the build hash


def test_the_constants_of_header_kernels_module_and_cases_agree():
    from umeregrobust_amd import gt_keypoints as gk
    header = open(API_HEADER).read()
    for name, value in (("UMEREG_GT_KEYPOINTS_MAX_B", gk.MAX_B), ("UMEREG_GT_BALL_ANY_MAX_K", gk.BALL_ANY_MAX_K),
                        ("UMEREG_GT_RECORD_WORDS", gk.RECORD_WORDS)):
        assert f"#define {name} {value}\n" in header
    kernels = open(os.path.join(REPO, "umeregrobust_amd", "csrc", "gt_keypoints.hip")).read()
    for name, value in (("kGtBlock", gk.CAND_BLOCK), ("kGtPickBlock", gk.PICK_BLOCK), ("kGtTestWaves", gk.TEST_WAVES),
                        ("kGtMaxTestWg", gk.MAX_TEST_WG), ("kGtWorkersPerSample", gk.WORKERS_PER_SAMPLE), ("kAnyBlock", gk.ANY_BLOCK), ("kAnyTile", gk.ANY_TILE)):
        assert f"constexpr int {name} = {value};" in kernels
    assert (gk.CAND_BLOCK, gk.PICK_BLOCK, gk.TEST_WAVES, gk.MAX_TEST_WG, gk.WORKERS_PER_SAMPLE) == \
        (gc.CAND_BLOCK, gc.PICK_BLOCK, gc.TEST_WAVES, gc.MAX_TEST_WG, gc.WORKERS_PER_SAMPLE)
    assert gk.ANY_TILE * 12 <= 48 * 1024 and gk.BALL_ANY_MAX_K == 7680                # a tile of p in LDS; the ball search's limit


def test_the_size_query_equals_its_restatement_and_is_zero_for_what_the_entries_refuse(lib):
    from umeregrobust_amd import gt_keypoints as gk
    q = lib.umereg_gt_keypoints_workspace_bytes
    for B, N in ((1, 1), (1, 255), (1, 256), (1, 257), (3, 2500), (8, 45000), (gk.MAX_B, 7)):
        assert q(B, N) == gk.workspace_bytes(B, N) > B * N
    for B, N in ((0, 10), (-1, 10), (gk.MAX_B + 1, 10), (1, 0), (1, -5)):
        assert q(B, N) == 0 == gk.workspace_bytes(B, N)


# ---- 2. without a device ---------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_before_the_device_probe(lib):
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) // 256 * 256
    B, N = 2, 300
    need = lib.umereg_gt_keypoints_workspace_bytes(B, N)

    def cand(o=p, f=p, B=B, N=N, c=p, n=p, ws=p, nws=need):
        return lib.umereg_gt_candidates(o, f, B, N, c, n, ws, nws, None)

    def select(pk=p, c=p, n=p, B=B, N=N, r=5.0, max_nn=64, min_nn=8, ns=4, flags=0, kp=p, rec=p, tested=None, ws=p, nws=need):
        return lib.umereg_gt_select_f32(pk, c, n, B, N, r, max_nn, min_nn, ns, flags, kp, rec, tested, ws, nws, None)

    def ball_any(q=p, pp=p, Bk=3, K=10, r=0.6, flags=0, hits=p):
        return lib.umereg_gt_ball_any_f32(q, pp, Bk, K, r, flags, hits, None)

    for k in ("o", "f", "c", "n"):
        assert cand(**{k: None}) == -1 and b"null pointer" in lib.umereg_last_error(), k
    for k in ("pk", "c", "n", "kp", "rec"):
        assert select(**{k: None}) == -1 and b"null pointer" in lib.umereg_last_error(), k
    for k in ("q", "pp", "hits"):
        assert ball_any(**{k: None}) == -1 and b"null pointer" in lib.umereg_last_error(), k
    for kw in (dict(B=0), dict(N=0), dict(B=1025)):
        assert cand(**kw) == -1 and select(**kw) == -1, kw
    for kw in (dict(r=0.0), dict(r=-1.0), dict(ns=0), dict(flags=2), dict(pk=p + 4)):
        assert select(**kw) == -1, kw
    for kw in (dict(Bk=0), dict(K=0), dict(K=7681), dict(r=0.0), dict(flags=2)):
        assert ball_any(**kw) == -1, kw
    assert b"7680" in (ball_any(K=7681), lib.umereg_last_error())[1]
    assert cand(ws=None) == -3 and cand(nws=need - 1) == -3 and select(nws=need - 1) == -3            # UMEREG_EWORKSPACE
    if lib.umereg_device_count(None, 0) == 0:
        for rc in (cand(), select(), ball_any()):
            assert rc == -2 and b"no CPU fallback" in lib.umereg_last_error()                           # UMEREG_ENODEV


# ---- 3. the keyword ------------------------------------------------------------------------------------------------------------------

def test_a_bad_selection_is_a_value_error_before_anything_touches_the_gpu():
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.ume_loss import UMEContrastiveLoss
    from umeregrobust_amd.utils.eval_utils import calc_inliear_ratio
    from umeregrobust_amd.utils.loc_utils import generate_ume_from_keypoints2
    with pytest.raises(ValueError, match="selection must be 'torch' or 'device'"):
        generate_ume_from_keypoints2(None, None, None, None, None, None, selection="host")
    with pytest.raises(ValueError, match="selection must be 'torch' or 'device'"):
        UMEContrastiveLoss().with_selection("gpu")
    with pytest.raises(ValueError, match="selection must be 'torch' or 'device'"):
        calc_inliear_ratio(None, None, None, None, 5.0, 64, 8, 32, selection=None)
    for fn in (generate_ume_from_keypoints2, calc_inliear_ratio):
        assert inspect.signature(fn).parameters["selection"].default == "torch"
    assert inspect.signature(tc.run).parameters["device_keypoints"].default is False
    assert inspect.signature(tc.TrainContext.__init__).parameters["selection"].default == "torch"
    # the loss's constructor keeps the reference's signature (tests/test_ume_grad_cpu.py pins it): the engine is set on the object
    assert "selection" not in inspect.signature(UMEContrastiveLoss.__init__).parameters
    assert UMEContrastiveLoss().selection == "torch" and UMEContrastiveLoss().with_selection("device").selection == "device"


def test_python_refuses_cpu_tensors_and_other_shapes():
    from umeregrobust_amd import gt_keypoints as gk
    z = torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gk.ball_any(z, z, 0.6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gk.candidates(torch.zeros(2, 10, dtype=torch.int64), torch.zeros(2, 10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gk.select(z, torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 5.0, 64, 8, 4)


# ---- 4. the restatement and its clouds -------------------------------------------------------------------------------------------------

def test_case_names_are_unique_and_the_base_cloud_is_what_it_claims():
    assert len({c.name for c in CASES}) == len(CASES)
    pts, idx, kinds = gc.base()
    assert pts.shape == (gc.N_TOTAL, 3) and len(idx) == len(kinds) == gc.PER_KIND * len(gc.KINDS)
    assert (np.diff(idx) < 0).all()
    hits = gc.hits_of(pts, idx)
    assert [int(h) for h in hits] == [gc.KINDS[k] for k in kinds]              # every centre's ball holds what its kind prescribes
    assert [bool(min(h, gc.MAX_NN) >= gc.MIN_NN) for h in hits] == [gc.DENSE[k] for k in kinds]
    assert gc.KINDS["m"] == gc.MIN_NN - 1 and gc.KINDS["d"] == gc.MIN_NN and gc.KINDS["p"] == gc.MIN_NN + 1 and gc.KINDS["x"] > gc.MAX_NN


def edge(case, s):
    """the property the case is named for"""
    ns, L = case.kw["num_samples"], s.min_length
    n_dense = [int(d.sum()) for d in s.dense]
    name = case.name
    if name == "last_candidate_completes":
        assert n_dense == [ns] and s.last == [L - 1] and s.dense[0][L - 1]
    elif name == "first_candidates":
        assert s.last == [ns - 1] and s.dense[0][:ns].all() and L > 4 * ns
    elif name in ("exactly_num_samples", "num_samples_plus_one", "num_samples_minus_one"):
        assert n_dense == [ns + {"exactly_num_samples": 0, "num_samples_plus_one": 1, "num_samples_minus_one": -1}[name]]
        assert s.num_out == min(n_dense[0], ns)
    elif name == "dense_at_the_lowest_indices":
        assert s.dense[0][:6].all() and n_dense == [ns + 1] and s.last == [ns - 1] and L == 26
        assert max(s.kp_index[0, :ns]) < min(s.cand[0, :L - 6])                    # (they ARE the lowest indices)
    elif name == "dense_at_the_highest_indices":
        assert int(np.where(s.dense[0])[0][0]) == 20 and n_dense == [ns + 1] and s.last == [L - 2]
    elif name == "truncation_cuts_the_dense_away":
        assert list(s.lengths) == [10, 15] and L == 10 and n_dense == [3, 0] and list(s.with_kpts) == [True, False] and s.num_out == 3
    elif name == "one_candidate":
        assert list(s.lengths) == [1] and ns == 1 and s.num_out == 1
    elif name == "hits_around_min_nn_and_above_max_nn":
        assert sorted(set(int(h) for h in s.hits[0])) == sorted(gc.KINDS.values()) and n_dense == [6]
    elif name == "min_nn_zero_is_always_dense":
        assert n_dense == [5] and max(s.hits[0]) < gc.MIN_NN
    elif name == "min_nn_above_max_nn":
        assert min(s.hits[0]) >= gc.MIN_NN and n_dense == [0] and s.error == "no_keypoint"
    elif name == "nothing_dense_anywhere":
        assert n_dense == [0, 0] and s.error == "no_keypoint"
    elif name == "no_candidate_in_one_element":
        assert list(s.lengths) == [2, 0] and s.error == "no_candidate"
    elif name.startswith("candidates_"):
        n = int(name.split("_")[1])
        assert list(s.lengths) == [n] and n_dense[0] < ns and s.last == [n - 1] and n_dense[0] > 0      # everything is tested
    elif name.startswith("stop_at_"):
        assert ns == int(name.split("_")[2]) and list(s.lengths) == [2100, 1500] and L == 1500
        assert all(n > ns for n in n_dense) and all(v < L - 600 for v in s.last)       # a stop long before the end is possible
        assert s.num_out == ns and ns in (gc.WG_CAP_SAMPLES + k for k in (-1, 0, 1)) and gc.WG_CAP_SAMPLES == 512
    elif name.startswith("workers_"):
        assert n_dense[0] > ns and s.last[0] < L - 1 and L > 8 * ns * gc.WORKERS_PER_SAMPLE
    elif name.startswith("cloud_of_"):
        assert case.n == int(name.split("_")[2]) and case.n % gc.CAND_BLOCK in (gc.CAND_BLOCK - 1, 0, 1) and 0 < n_dense[0]
    else:
        raise AssertionError(f"no edge stated for {name}")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_restatement_on_its_edge_and_against_the_oracle(case):
    s = gc.select_ref(case)
    assert s.error == case.error
    edge(case, s)
    for b in range(len(case.elements)):
        k = int(s.record[b, 0])
        assert (s.kp_index[b, k:] == -1).all() and (s.cand[b, s.lengths[b]:] == -1).all() and (np.diff(s.cand[b, :s.lengths[b]]) < 0).all()
    if case.error:
        return
    src, seg, sf, tgt, tf, gt = gc.inputs(case)
    ref = orc.generate_ume_from_keypoints2(src, seg, sf, tgt, tf, gt, normalized_ume=False, **case.kw)
    assert np.array_equal(ref[5], s.with_kpts)
    keep = np.where(s.with_kpts)[0]
    assert ref[2].shape == (len(keep), s.num_out, 3)
    for row, b in enumerate(keep):
        assert np.array_equal(ref[2][row], src[b][s.kp_index[b, :s.num_out]]), b


def test_ball_any_restatement_against_the_oracle_ball_query():
    for Bk, K in ((1, 1), (3, 63), (2, 65), (2, 750)):
        q, p = gc.ball_any_inputs(Bk, K, 1)
        want = (orc.ball_query(q, p, K=1, radius=gc.INTERSECTION_R, return_nn=False).idx > -1).sum(axis=(1, 2))
        got = gc.ball_any_ref(q, p, gc.INTERSECTION_R)
        assert np.array_equal(got, want) and (K < 60 or 0 < got.sum() < Bk * K)
    for inside in (False, True):
        q, p, radius = gc.lattice_345(750, inside)
        want = (orc.ball_query(q, p, K=1, radius=radius, return_nn=False).idx > -1).sum(axis=(1, 2))
        assert list(want) == list(gc.ball_any_ref(q, p, radius)) == [750 if inside else 0]
