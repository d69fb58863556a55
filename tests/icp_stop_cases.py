"""The cases of tests/test_icp_stop_cases_cpu.py and tests/test_icp_stop_gpu.py: the ICP stop rule, the state after each evaluation /
update pair, the second stride of the totals loop and the host's batching, for the three estimators that share icp_step_kernel.

Plain data and builders; nothing of the product is imported.  The references are the fp64 restatements (oracle.icp_point_to_point,
icp_plane_ref.icp_point_to_plane, icp_gicp_ref.icp_plane_to_plane) with their `trace`.

A row names thresholds and the iteration count the restatement ends at with them.  Every start transform is rounded to f32 first: the
host start (fp64 [4,4]) and the device start (f32 [4,4]) of a row are then the same numbers, and one reference serves both.

Two conditions hold for every row and every second-stride case; the CPU test asserts them.  They are what lets the GPU test use the
suite's gate (equal iteration count, |d fitness| < 1e-12, |d rmse| < 1e-9, max |dT| < 1e-9):
  * every stop decision of the reference is at least MARGIN_MIN = 1e-7 from flipping (100 times the rmse gate).  The margin is the one
    icp_gicp_ref's `margins` computes -- a stop: min(rel_f - df, rel_r - dr); no stop: max(df - rel_f, dr - rel_r) -- except that a
    comparison against a threshold of 0.0, which no value passes, cannot flip and does not count;
  * for the two plane estimators the condition number of every system solved is <= COND_MAX = 1e4 (icp_plane_ref reports cond(A) of
    the whole system, an upper bound of the retained one; icp_gicp_ref the retained one)."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import icp_gicp_ref as gicp
import icp_plane_ref as plane
from oracle import oracle as orc
from tests.test_gpu_parity import _icp_case

ESTIMATORS = ("point_to_point", "point_to_plane", "plane_to_plane")
MARGIN_MIN = 1e-7
COND_MAX = 1e4
NEVER_MAX_ITERATIONS = (3, 4, 5, 11, 12, 13)
# what IcpJob and the synchronous entries have enqueued when a run that never stops early ends: 4 pairs, then 8 at a time, until the
# pair that finds iters >= max_iteration (pair max_iteration + 1) has run
NEVER_LAUNCHED = {3: 4, 4: 12, 5: 12, 11: 12, 12: 20, 13: 20}
STRIDE_N_SRC = (16384, 16385, 16448 + 1)      # 256, 257 and 258 rows of partial sums; the last two rows hold one point each
STRIDE_MAX_ITERATIONS = (1, 5)
STRIDE_MAX_DIST = plane.CORNER_MAX_DIST

# kind: what the row is in the table for
#   fitness_withholds  at some update before the stop |d rmse| < relative_rmse and |d fitness| >= relative_fitness
#   rmse_withholds     the mirror image
#   swap               the run with the two thresholds exchanged ends at `swapped` iterations, not at `iterations`
#   strict             relative_fitness = 0, relative_rmse above every |d rmse|, the fitness repeats exactly: runs to max_iteration
#   immediate          both thresholds above every difference: stops at the second evaluation
#   never              both thresholds 0: exactly max_iteration updates
Row = namedtuple("Row", "estimator kind case max_dist max_iteration relative_fitness relative_rmse iterations swapped")


def _rows():
    out = []

    def add(estimator, kind, case, max_dist, max_iteration, rel_f, rel_r, iterations, swapped=None):
        out.append(Row(estimator, kind, case, max_dist, max_iteration, rel_f, rel_r, iterations, swapped))

    # point to point on the far start of test_icp_job_equals_the_synchronous_call: the fitness climbs for eight updates
    # (|d fitness| 7e-3 .. 0.42), is exactly 1.0 from update 8 on; |d rmse| is 1.4e-4 at update 2, 1.3e-2 at update 9, 1e-17 after
    add("point_to_point", "fitness_withholds", "lattice8", 0.2, 30, 1e-3, 5e-4, 10)
    add("point_to_point", "rmse_withholds", "lattice8", 0.2, 30, 0.5, 2e-4, 2)
    add("point_to_point", "swap", "lattice8", 0.2, 30, 0.5, 1e-5, 10, 9)
    add("point_to_point", "strict", "lattice8", 0.2, 12, 0.0, 1.0, 12)
    add("point_to_point", "immediate", "lattice8", 0.2, 30, 10.0, 10.0, 1)
    # point to plane on the corner from 3 x START_OFFSET at 0.3 m: |d fitness| 0.19, 0.51, 1.2e-2, then exactly 0;
    # |d rmse| 1.5e-3, 3.9e-2, 8.3e-3, 2.6e-5, 1.8e-6, 3.8e-7
    add("point_to_plane", "fitness_withholds", "corner0x3", 0.3, 30, 1e-2, 5e-3, 4)
    add("point_to_plane", "rmse_withholds", "corner0x3", 0.3, 30, 1e-3, 1e-5, 5)
    add("point_to_plane", "swap", "corner0x3", 0.3, 30, 0.3, 1e-6, 6, 4)
    add("point_to_plane", "strict", "corner0x3", 0.3, 8, 0.0, 1.0, 8)
    add("point_to_plane", "immediate", "corner0x3", 0.3, 30, 10.0, 10.0, 1)
    # plane to plane from 2 x START_OFFSET (from 3 x the systems reach a condition number of 2.1e4): seed 0 has |d fitness| 0.35, 0.25,
    # 0, 5e-4, then 0 and |d rmse| 3.0e-2, 1.8e-2, 4.1e-4, 1.0e-4, 7e-8; seed 1 has |d fitness| 0.41, 0.20, 1e-3, then 0 and |d rmse|
    # 2.4e-2, 2.4e-2, 1.3e-4, 2.7e-6, 2.4e-7, 2.3e-9
    add("plane_to_plane", "fitness_withholds", "corner0x2", 0.3, 30, 1e-4, 2e-4, 5)
    add("plane_to_plane", "rmse_withholds", "corner0x2", 0.3, 30, 1e-3, 3e-4, 4)
    add("plane_to_plane", "swap", "corner1x2", 0.3, 30, 0.5, 1.2e-7, 6, 4)
    add("plane_to_plane", "strict", "corner0x2", 0.3, 8, 0.0, 1.0, 8)
    add("plane_to_plane", "immediate", "corner0x2", 0.3, 30, 10.0, 10.0, 1)
    for estimator, case, max_dist in (("point_to_point", "lattice8", 0.2), ("point_to_plane", "corner0x3", 0.3),
                                      ("plane_to_plane", "corner0x2", 0.3)):
        for max_iteration in NEVER_MAX_ITERATIONS:
            add(estimator, "never", case, max_dist, max_iteration, 0.0, 0.0, max_iteration)
    return tuple(out)


ROWS = _rows()
# the row of each estimator the trajectory test drives pair by pair: a threshold stop after at least 6 updates
TRAJECTORY = {e: next(r for r in ROWS if r.estimator == e and r.kind == k)
              for e, k in (("point_to_point", "fitness_withholds"), ("point_to_plane", "swap"), ("plane_to_plane", "swap"))}


def row_id(row):
    return f"{row.estimator}-{row.kind}-{row.max_iteration}"


def _f32_exact(T):
    return np.asarray(T, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> SimpleNamespace(src, tgt f32 [n,3]; ns, nt f32 normals (None for the lattice); T0 float64 [4,4] holding f32 values)"""
    if case == "lattice8":
        src, tgt, _, T0 = _icp_case(8, ang_deg=2.5, shift=0.15)
        return SimpleNamespace(src=src, tgt=tgt, ns=None, nt=None, T0=_f32_exact(T0))
    seed, k = {"corner0x3": (0, 3.0), "corner0x2": (0, 2.0), "corner1x2": (1, 2.0)}[case]
    src, tgt, ns, nt, gt, _ = gicp.corner(2000, seed)
    return SimpleNamespace(src=src, tgt=tgt, ns=ns, nt=nt, T0=_f32_exact(plane.euler_update(k * np.array(plane.START_OFFSET)) @ gt))


def margins(trace, relative_fitness, relative_rmse):
    """per stop test of a trace, how far the decision is from flipping (icp_gicp_ref's `margins`; inf where a half that withholds is
    compared against 0.0)"""
    out = []
    for _, _, _, df, dr, stopped in trace[1:]:
        if stopped:
            out.append(min(relative_fitness - df, relative_rmse - dr))
        else:
            out.append(max(np.inf if relative_fitness == 0.0 else df - relative_fitness,
                           np.inf if relative_rmse == 0.0 else dr - relative_rmse))
    return out


def restate(estimator, c, max_dist, max_iteration, relative_fitness, relative_rmse, n_src=None):
    """the restatement of `estimator` on the first n_src source points of the inputs `c` -> SimpleNamespace(result = (T, fitness, rmse,
    iterations), trace, conds, margins)"""
    src = c.src[:n_src]
    trace, conds = [], []
    if estimator == "point_to_point":
        res = orc.icp_point_to_point(src, c.tgt, c.T0, max_dist, max_iteration, relative_fitness, relative_rmse, trace=trace)
    elif estimator == "point_to_plane":
        res = plane.icp_point_to_plane(src, c.tgt, c.nt, c.T0, max_dist, max_iteration, relative_fitness, relative_rmse, conds=conds,
                                       trace=trace)
    else:
        res = gicp.icp_plane_to_plane(src, c.tgt, c.ns[:n_src], c.nt, c.T0, max_dist, max_iteration, relative_fitness, relative_rmse,
                                      conds=conds, trace=trace)
    return SimpleNamespace(result=res, trace=trace, conds=conds, margins=margins(trace, relative_fitness, relative_rmse))


@functools.lru_cache(maxsize=None)
def _reference(estimator, case, max_dist, max_iteration, relative_fitness, relative_rmse):
    return restate(estimator, inputs(case), max_dist, max_iteration, relative_fitness, relative_rmse)


def reference(row, swapped=False, defaults=False):
    """the restatement on a row, computed once; swapped: with the two thresholds exchanged; defaults: with both at 1e-6"""
    rel = (1e-6, 1e-6) if defaults else (row.relative_fitness, row.relative_rmse)
    return _reference(row.estimator, row.case, row.max_dist, row.max_iteration, *(rel[::-1] if swapped else rel))


# ------------------------------------------------------------------------------------------------ second stride
@functools.lru_cache(maxsize=None)
def stride_inputs(seed=0):
    """corner_case with its 2 000-point target and max(STRIDE_N_SRC) source points from the same generator (the target is the first
    draw, so it is corner_case(2000, seed)'s); source normals from normals_ref on the whole source cloud"""
    n = max(STRIDE_N_SRC)
    rng = np.random.RandomState(seed)
    tgt = plane.corner_cloud(2000, rng).astype(np.float32)
    _, tgt_same, _, nt, gt, T0 = gicp.corner(2000, seed)
    assert np.array_equal(tgt, tgt_same)
    s = plane.corner_cloud(n, rng)
    src = ((s - gt[:3, 3]) @ gt[:3, :3]).astype(np.float32)
    ns = plane.normals_ref(src, 30)[0].astype(np.float32)
    return SimpleNamespace(src=src, tgt=tgt, ns=ns, nt=nt, T0=_f32_exact(T0))


@functools.lru_cache(maxsize=None)
def stride_reference(estimator, n_src, max_iteration):
    return restate(estimator, stride_inputs(), STRIDE_MAX_DIST, max_iteration, 1e-6, 1e-6, n_src=n_src)
