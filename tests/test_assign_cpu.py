"""CPU: the ground the device-side linear sum assignment stands on -- the host side of include/umereg_assign.h (exports, the
signature table, the size query, argument checks before the device probe), the Python surface's defaults, and the numpy
restatement of the scheme (tests/assign_ref.py) against scipy."""
import inspect
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment as scipy_lsa

from tests.assign_ref import linear_sum_assignment_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assign_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import assign, ops
    assert sorted(assign.ASSIGN_SIGNATURES) == ["umereg_assign_workspace_bytes", "umereg_linear_sum_assignment"]
    assert "umereg_assign" not in open(os.path.join(REPO, "include", "umereg.h")).read()
    assert ops.linear_sum_assignment is assign.linear_sum_assignment


def test_size_query_is_zero_exactly_where_the_entry_refuses():
    from umeregrobust_amd import assign
    lib = assign.load_native()
    q = lib.umereg_assign_workspace_bytes
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    names = ("cost", "batch", "n_rows", "n_cols", "row_stride", "batch_stride", "out_pairs", "out_total", "out_status", "workspace",
             "workspace_bytes", "stream")
    base = dict(batch=2, n_rows=5, n_cols=7, row_stride=8, batch_stride=40, workspace_bytes=1 << 12, stream=None)
    call = lambda **kw: lib.umereg_linear_sum_assignment(*[kw.get(k, base.get(k, p)) for k in names])      # noqa: E731
    no_device = lib.umereg_device_count(None, 0) == 0
    good = ((1, 1, 1), (1, 1, 300), (2, 5, 7), (8, 1000, 1000), (1, 10000, 10000), (65535, 3, 3), (1, 2 ** 31 - 1, 2 ** 31 - 1))
    bad = ((1, 6, 5), (1, 1001, 1000), (0, 5, 5), (-1, 5, 5), (1, 0, 5), (1, -2, 5), (1, 0, 0), (1, 5, -5), (65536, 3, 3), (1, 5, 2 ** 31),
           (1, 2 ** 31, 2 ** 31), (1, 5, 2 ** 40))
    for b, n, m in good:
        assert q(b, n, m) > 0 and q(b, n, m) % 256 == 0 and q(b, n, m) == b * q(1, n, m), (b, n, m)
        if no_device:                                                       # accepted as arguments: the next thing is the probe
            assert call(batch=b, n_rows=n, n_cols=m, row_stride=m, batch_stride=n * m) == -2, (b, n, m)
    for b, n, m in bad:
        assert q(b, n, m) == 0, (b, n, m)
        assert call(batch=b, n_rows=n, n_cols=m, row_stride=max(m, 1), batch_stride=0) == -1, (b, n, m)      # UMEREG_EINVAL
    # per column two doubles, three ints and a byte besides the duals' row side: the slice is a few dozen bytes per column
    assert 37 * 1000 <= q(1, 1000, 1000) <= 56 * 1000 + 11 * 256
    assert q(1, 5, 7) <= q(1, 7, 7) <= q(1, 7, 8)
    assert assign.workspace_bytes(1, 6, 5) == 0 and assign.workspace_bytes(3, 5, 6) == 3 * assign.workspace_bytes(1, 5, 6)


def test_entry_checks_arguments_before_it_needs_a_device():
    from umeregrobust_amd import assign
    lib = assign.load_native()
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    names = ("cost", "batch", "n_rows", "n_cols", "row_stride", "batch_stride", "out_pairs", "out_total", "out_status", "workspace",
             "workspace_bytes", "stream")
    base = dict(batch=2, n_rows=5, n_cols=7, row_stride=8, batch_stride=40, workspace_bytes=1 << 12, stream=None)
    call = lambda **kw: lib.umereg_linear_sum_assignment(*[kw.get(k, base.get(k, p)) for k in names])      # noqa: E731
    for kw in (dict(row_stride=6), dict(row_stride=0), dict(row_stride=-8), dict(batch_stride=-1), dict(cost=None), dict(out_pairs=None),
               dict(out_status=None), dict(n_rows=8), dict(batch=0), dict(n_cols=0)):
        assert call(**kw) == -1, kw                                          # UMEREG_EINVAL
        assert lib.umereg_last_error()
    if lib.umereg_device_count(None, 0) == 0:
        assert call() == -2                                                  # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        assert call(out_total=None) == -2                                    # the total is optional
        assert call(row_stride=7, batch_stride=0) == -2                      # a dense row, one matrix read twice
        assert call(workspace=None, workspace_bytes=0) == -2                 # (the workspace is checked after the probe)


def test_python_surface_refuses_the_host_and_keeps_its_defaults():
    import torch

    from umeregrobust_amd import assign, evaluate
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.utils.eval_utils import calc_inliear_ratio
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assign.linear_sum_assignment(torch.zeros(3, 3))
    with pytest.raises(NotImplementedError):
        assign.linear_sum_assignment(torch.zeros(3, 3), maximize=True)
    with pytest.raises(ValueError):
        assign.linear_sum_assignment(torch.zeros(3))
    assert inspect.signature(calc_inliear_ratio).parameters["assignment"].default == "host"
    assert inspect.signature(tc.run).parameters["device_assignment"].default is False
    assert inspect.signature(tc.eval_one_epoch).parameters["assignment"].default == "host"
    assert 'getattr(args, "assignment", "host")' in inspect.getsource(evaluate._phase_a)
    with pytest.raises(ValueError, match="assignment"):
        calc_inliear_ratio({}, {}, None, None, 1.0, 8, 4, 8, assignment="gpu")
    with pytest.raises(KeyError):
        tc.make_config("kitti", device_assignment=True)                      # a flag of the driver, not a config key


def _cases():
    out = []
    for n, m, seed in ((1, 1, 0), (2, 2, 1), (65, 65, 2), (257, 257, 3), (37, 200, 4)):
        out.append((n, m, np.random.RandomState(seed).random_sample((n, m)).astype(np.float32)))
    return out


@pytest.mark.parametrize("n,m,C", _cases(), ids=lambda v: str(v) if isinstance(v, int) else "C")
def test_restatement_equals_scipy(n, m, C):
    stats = {}
    rows, cols, total = linear_sum_assignment_ref(C, stats)
    r_s, c_s = scipy_lsa(C)
    assert np.array_equal(rows, r_s) and np.array_equal(cols, c_s), "the permutation differs from scipy's"
    total_s = 0.0
    for i, j in zip(r_s, c_s):
        total_s += float(C[i, j])
    assert total == total_s, "the fp64 totals differ"
    assert sorted(set(cols.tolist())) == sorted(cols.tolist()) and 0 <= stats["matched"] <= n and stats["steps"] >= n - stats["matched"]


def test_restatement_keeps_scipys_total_on_ties():
    rng = np.random.RandomState(5)
    i = np.arange(1, 41, dtype=np.float64)
    for C in (rng.randint(0, 8, (48, 48)), np.full((30, 30), 3.0), np.outer(i, i), rng.randint(0, 4, (20, 50))):
        C = C.astype(np.float32)
        _, cols, total = linear_sum_assignment_ref(C)
        assert len(set(cols.tolist())) == C.shape[0]
        assert total == float(C[scipy_lsa(C)].astype(np.float64).sum())     # small integers: every sum is exact
