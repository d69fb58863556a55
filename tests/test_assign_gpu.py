"""GPU: the linear sum assignment of include/umereg_assign.h against scipy -- identical permutations where the optimum is unique,
identical fp64 totals where costs tie -- at the wave and workgroup edges of the search kernel and at the sizes where its
per-column state leaves LDS for the workspace; strided batches, guard bands and run-twice idempotence, a NaN in a batch, and the
three call sites (calc_inliear_ratio, evaluate's hungarian_matching_flag, the training driver's validation epoch) with
assignment="device" against the host path.

The seeds of the float cases were chosen on the CPU such that scipy on C, scipy on C.T and the restatement of tests/assign_ref.py
all give the same permutation (the optimum is unique there, so identity is a fair demand)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

from tests.assign_ref import linear_sum_assignment_ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

SQUARE = (1, 2, 63, 64, 65, 257, 1023, 1025)
# (n_rows, n_cols): the search keeps in its workspace slice instead of LDS -- 1900 x 1900: u; 40 x 3000: `visited` and row4col;
# 40 x 8000: `shortest`, v and row4col
STATE_EDGES = ((1900, 1900), (40, 3000), (40, 8000))


def float_costs(n, m):
    return np.random.RandomState(1000 + n).random_sample((n, m)).astype(np.float32)


def crowded_costs(n, m):
    """half as many cheap columns as rows, the others dearer by one: the rows compete, so the start leaves many of them to the search"""
    C = float_costs(n, m)
    C[:, n // 2:] += np.float32(1.0)
    return C


def ordered_sum(C, rows, cols):
    """the fp64 sum of the chosen fp32 costs in row order, one addition after the other"""
    return float(np.cumsum(C[rows, cols].astype(np.float64))[-1])


def solve(C, gpu, with_stats=False):
    """numpy [n, m] or [b, n, m] -> the C entry's outputs as numpy"""
    from umeregrobust_amd import assign
    c = torch.from_numpy(np.ascontiguousarray(C)).to(gpu)
    out = assign.solve(c if c.dim() == 3 else c[None], with_stats=with_stats)
    return tuple(o.cpu().numpy() for o in out)


def check_against_scipy(C, pairs, total, status, same_permutation):
    n, m = C.shape
    assert status == 0
    assert np.array_equal(pairs[:, 0], np.arange(n)), "rows must ascend"
    cols = pairs[:, 1]
    assert ((cols >= 0) & (cols < m)).all() and len(set(cols.tolist())) == n, "not a one-to-one assignment"
    assert total == ordered_sum(C, pairs[:, 0], cols), "out_total is not the ordered fp64 sum of the chosen costs"
    r_s, c_s = scipy_lsa(C)
    total_s = ordered_sum(C, r_s, c_s)
    bound = 2.0 * n * n * 2.0 ** -52 * float(np.abs(C).max())
    print(f"{n} x {m}: |total - scipy's| = {abs(total - total_s):.3e} (bound {bound:.3e}), same permutation: {np.array_equal(cols, c_s)}")
    assert abs(total - total_s) <= bound
    if same_permutation:
        assert np.array_equal(cols, c_s), f"{int((cols != c_s).sum())} of {n} rows differ from scipy's assignment"
    return total_s


@pytest.mark.parametrize("n", SQUARE)
def test_square_float_costs_equal_scipy(gpu, n):
    C = float_costs(n, n)
    pairs, total, status = solve(C, gpu)
    check_against_scipy(C, pairs[0], float(total[0]), int(status[0]), same_permutation=True)


@pytest.mark.parametrize("n", (65, 257))
def test_start_and_step_counts_are_the_restatements(gpu, n):
    C = float_costs(n, n)
    pairs, total, status, stats = solve(C, gpu, with_stats=True)
    want = {}
    _, cols, total_ref = linear_sum_assignment_ref(C, want)
    assert np.array_equal(pairs[0, :, 1], cols) and float(total[0]) == total_ref
    assert (int(stats[0, 0]), int(stats[0, 1])) == (want["matched"], want["steps"])


@pytest.mark.parametrize("n,m", ((37, 200), (1, 300)) + STATE_EDGES, ids=lambda v: str(v))
def test_rectangles_and_state_edges_through_the_c_entry(gpu, n, m):
    C = float_costs(n, m) if n == m or m <= 300 else crowded_costs(n, m)
    pairs, total, status = solve(C, gpu)
    check_against_scipy(C, pairs[0], float(total[0]), int(status[0]), same_permutation=True)


def test_tall_matrix_through_the_python_op(gpu):
    from umeregrobust_amd import ops
    C = float_costs(200, 37)
    rows, cols = ops.linear_sum_assignment(torch.from_numpy(C).to(gpu))
    r_s, c_s = scipy_lsa(C)
    assert rows.dtype == cols.dtype == torch.int64 and rows.is_cuda and cols.is_cuda
    assert np.array_equal(rows.cpu().numpy(), r_s) and np.array_equal(cols.cpu().numpy(), c_s)
    # a batch of them, and a wide one, in one call each
    Cb = np.stack([C, float_costs(200, 37)[::-1].copy()])
    rows, cols = ops.linear_sum_assignment(torch.from_numpy(Cb).to(gpu))
    for b in range(2):
        r_s, c_s = scipy_lsa(Cb[b])
        assert np.array_equal(rows[b].cpu().numpy(), r_s) and np.array_equal(cols[b].cpu().numpy(), c_s)
    rows, cols = ops.linear_sum_assignment(torch.from_numpy(np.ascontiguousarray(C.T)).to(gpu))
    r_s, c_s = scipy_lsa(C.T)
    assert np.array_equal(rows.cpu().numpy(), r_s) and np.array_equal(cols.cpu().numpy(), c_s)


def test_strided_batch_equals_single_calls(gpu):
    from umeregrobust_amd import assign
    n, m, row_stride = 65, 70, 96
    A, B = float_costs(n, m), float_costs(n + 1, m)[1:]
    store = torch.full((3, n + 2, row_stride), float("nan"), device=gpu)        # what lies between the rows is never read
    view = store[:, 1:n + 1, 5:5 + m]
    for b, C in enumerate((A, B, A)):
        view[b] = torch.from_numpy(C).to(gpu)
    assert view.stride() == ((n + 2) * row_stride, row_stride, 1) and not view.is_contiguous()
    pairs, total, status = assign.solve(view)
    assert not status.any()
    for b, C in enumerate((A, B, A)):
        p1, t1, s1 = assign.solve(torch.from_numpy(C).to(gpu)[None])
        assert torch.equal(pairs[b], p1[0]) and total[b].cpu().numpy().tobytes() == t1[0].cpu().numpy().tobytes() and int(s1[0]) == 0
        assert np.array_equal(pairs[b, :, 1].cpu().numpy(), scipy_lsa(C)[1])
    assert torch.equal(pairs[0], pairs[2]) and not torch.equal(pairs[0], pairs[1])
    rows, cols = assign.linear_sum_assignment(view)                              # the op passes the view through as it lies
    assert torch.equal(cols, pairs[..., 1])


def tie_cases():
    rng = np.random.RandomState(7)
    base = rng.randint(0, 1000, (40, 40))
    i = np.arange(1, 129, dtype=np.float64)
    return {"small_integers": rng.randint(0, 8, (128, 128)), "all_equal": np.full((100, 100), 3.0),
            "duplicated_rows_and_columns": base[rng.randint(0, 40, 96)][:, rng.randint(0, 40, 96)], "products": np.outer(i, i)}


@pytest.mark.parametrize("kind", sorted(tie_cases()))
def test_tied_costs_keep_scipys_total(gpu, kind):
    C = tie_cases()[kind].astype(np.float32)
    pairs, total, status = solve(C, gpu)
    total_s = check_against_scipy(C, pairs[0], float(total[0]), int(status[0]), same_permutation=False)
    assert float(total[0]) == total_s, "integer costs: the totals must be equal exactly"


def test_guard_bands_and_run_twice(gpu):
    """outputs and workspace at exactly the stated sizes between 4 KiB canaries, other garbage and other poison on each run"""
    from tests.test_abi_guard import Guard
    from umeregrobust_amd import assign
    assign.load_native()
    b, n, m, row_stride = 2, 67, 131, 140
    C = np.stack([float_costs(n, row_stride), float_costs(n + 1, row_stride)[1:]])
    runs = []
    for run in (0, 1):
        g = Guard(gpu, run)
        cost, _ = g.inp(C, "cost")
        pairs_p, pairs = g.out((b, n, 2), torch.int64, "out_pairs")
        total_p, total = g.out((b,), torch.float64, "out_total")
        status_p, status = g.out((b,), torch.int32, "out_status")
        ws_p, ws_n = g.ws(g.lib.umereg_assign_workspace_bytes(b, n, m), "workspace")
        g.call("umereg_linear_sum_assignment", cost, b, n, m, row_stride, n * row_stride, pairs_p, total_p, status_p, ws_p, ws_n, g.stream)
        g.check()
        runs.append([t.cpu().numpy().tobytes() for t in (pairs, total, status)])
        for k in range(b):
            check_against_scipy(C[k][:, :m], pairs[k].cpu().numpy(), float(total[k]), int(status[k]), same_permutation=True)
    assert runs[0] == runs[1], "an output depends on what the buffers held before the call"


def test_a_nan_ends_its_matrix_and_leaves_the_other(gpu):
    from umeregrobust_amd import assign, ops
    C = np.stack([float_costs(65, 65), float_costs(66, 65)[1:]])
    C[0, 40, 13] = np.nan
    pairs, total, status = solve(C, gpu)
    assert status.tolist() == [1, 0]
    p1, t1, s1 = solve(C[1], gpu)
    assert np.array_equal(pairs[1], p1[0]) and total[1] == t1[0] and int(s1[0]) == 0
    assert np.array_equal(pairs[1, :, 1], scipy_lsa(C[1])[1])
    for bad in (np.inf, -np.inf):
        C[0, 40, 13] = bad
        assert solve(C, gpu)[2].tolist() == [1, 0]
    with pytest.raises(ValueError, match="invalid numeric entries"):
        ops.linear_sum_assignment(torch.from_numpy(C).to(gpu))
    assert assign.linear_sum_assignment(torch.from_numpy(C[1]).to(gpu))[1].tolist() == p1[0, :, 1].tolist()


def test_calc_inliear_ratio_on_the_device_equals_the_host(gpu):
    from umeregrobust_amd.utils.eval_utils import calc_inliear_ratio
    g = load_golden("g8_gt_ume_inlier.npz")
    T = lambda a: torch.from_numpy(a).to(gpu)                                   # noqa: E731
    src = dict(pts=T(g["src_pts"])[None], seg=T(g["src_seg"])[None], feat=T(g["src_feat"])[None])
    tgt = dict(pts=T(g["tgt_pts"])[None], seg=None, feat=T(g["tgt_feat"])[None])
    gt = T(g["gt_tform"])[None]
    for kw in (dict(ume_r_nn=5.0, ume_max_nn=64, ume_min_nn=10, eval_num_kpts=48), dict(ume_r_nn=4.0, ume_max_nn=32, ume_min_nn=12, eval_num_kpts=30)):
        host, dev = (calc_inliear_ratio(src, tgt, None, gt, keypoints_ignore_segments=[9], inlear_thr=0.6, nn_inter_thr=0.6, assignment=a, **kw)
                     for a in ("host", "device"))
        assert dev.shape == (1,) and dev.device == host.device and torch.equal(dev, host)


def test_hungarian_flag_on_the_device_equals_the_host(gpu):
    from umeregrobust_amd import evaluate
    g = load_golden("g9_hungarian.npz")
    t = lambda a: torch.from_numpy(a).to(gpu)[None]                             # noqa: E731
    clouds = (t(g["src_pts"]), t(g["tgt_pts"]), t(g["src_feat"]), t(g["tgt_feat"]))
    for filt in (True, False):
        outs = {}
        for assignment in ("host", "device"):
            args = SimpleNamespace(ume_max_nn=750, ume_r_nn=5.0, filter_by_ume_dist_cond=filt, ume_n_samples=int(g["ume_n_samples"]),
                                   tau=float(g["tau"]), hungarian_matching_flag=True, assignment=assignment)
            outs[assignment] = evaluate.register_pair(*clouds, args, rng=np.random.RandomState(int(g["seed"])), src_inds=g["src_inds"],
                                                      tgt_inds=g["tgt_inds"])
            pipe = evaluate.RegistrationPipeline(args, gpu, depth=2, rng=np.random.RandomState(int(g["seed"])))
            outs[assignment + "_pipe"] = pipe.finish(pipe.submit(*clouds, src_inds=torch.from_numpy(g["src_inds"]).to(gpu),
                                                                 tgt_inds=torch.from_numpy(g["tgt_inds"]).to(gpu)))
        for a, b in (("host", "device"), ("host_pipe", "device_pipe")):
            h, d = outs[a], outs[b]
            assert torch.equal(d.match_src, h.match_src) and torch.equal(d.match, h.match), (filt, a)
            assert np.array_equal(np.asarray(d.cond), np.asarray(h.cond)), (filt, a)
            assert torch.equal(d.rtume_tform, h.rtume_tform), (filt, a)


class Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def test_validation_epoch_logs_the_same_inlier_ratio(gpu, tmp_path):
    from umeregrobust_amd import train_coloring as tc
    small = dict(batch_size=2, ume_max_nn=64, ume_min_nn=8, ume_r_nn=2.0, ume_n_samples=32, num_pw_samples=128, eval_num_kpts=32, lr=1e-3,
                 use_aug=False)
    logs = []
    for flag in (False, True):
        args = tc.make_config("kitti", **{**small, "device": str(gpu), "num_epochs": 1, "random_seed": 5})
        log = Scalars()
        tc.run(args, synthetic=4, summary_writer=log, out_path=os.path.join(str(tmp_path), f"flag_{int(flag)}"), device_assignment=flag)
        logs.append(log.rows)
    ratio = [[r for r in rows if r[0] == "valid/inlear_ratio"] for rows in logs]
    print(f"valid/inlear_ratio: {ratio[0]}")
    assert len(ratio[0]) == 1 and ratio[0] == ratio[1]
    assert logs[0] == logs[1], "the flag changes only where the matching runs, nothing that is logged"
