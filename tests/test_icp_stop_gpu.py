"""GPU: the ICP stop rule, the state after every evaluation / update pair, the second stride of the totals loop and the host's batch
edges, for point to point, point to plane and plane to plane (one state machine, icp_step_kernel), against the fp64 restatements on
the cases of tests/icp_stop_cases.py.

The gate is the suite's own: equal iteration count, |d fitness| < 1e-12, |d rmse| < 1e-9, max |dT| < 1e-9.  What justifies it --
every stop decision of the reference at least 1e-7 from flipping, every system solved with a condition number <= 1e4 -- is asserted
on the CPU (tests/test_icp_stop_cases_cpu.py) and again here on every reference used."""
import functools

import numpy as np
import pytest
import torch

import icp_stop_cases as sc

pytestmark = pytest.mark.gpu

SUMS = {"point_to_point": 17, "point_to_plane": 29, "plane_to_plane": 29}      # IcpSums<kPlane>::kCount of csrc/icp.hip
EPSILON = 1e-3


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _device_inputs(case, gpu):
    """(src, tgt, [normals the estimators take, the source's first], T0 f32 [4,4]) on the device, uploaded once per case"""
    c = sc.stride_inputs() if case == "stride" else sc.inputs(case)
    nrm = [] if c.ns is None else [T_(c.ns, gpu), T_(c.nt, gpu)]
    return T_(c.src, gpu), T_(c.tgt, gpu), nrm, T_(c.T0.astype(np.float32), gpu)


def _normals(estimator, nrm, n_src=None):
    """the normals `estimator` takes: none, the target's, or both (the source's cut to its first n_src)"""
    if estimator == "point_to_point":
        return []
    return nrm[1:] if estimator == "point_to_plane" else [nrm[0][:n_src].contiguous(), nrm[1]]


def _sync(estimator, s, t, nrm, T0, max_dist, max_iteration, *rel):
    from umeregrobust_amd import ops
    if estimator == "point_to_point":
        return ops.icp_point_to_point(s, t, T0, max_dist, max_iteration, *rel)
    if estimator == "point_to_plane":
        return ops.icp_point_to_plane(s, t, *nrm, T0, max_dist, max_iteration, *rel)
    return ops.icp_plane_to_plane(s, t, *nrm, T0, max_dist, max_iteration, *rel, epsilon=EPSILON)


def _job(estimator, s, t, nrm, T0d, max_dist, max_iteration, *rel):
    from umeregrobust_amd import ops
    kw = dict(zip(("tgt_normals", "src_normals"), nrm[::-1]))
    return ops.IcpJob(s, t, T0d, max_dist, max_iteration, *rel, **kw)


def _bits_equal(a, b):
    return a.transformation.tobytes() == b.transformation.tobytes() and a.iterations == b.iterations \
        and np.float64(a.fitness).tobytes() == np.float64(b.fitness).tobytes() \
        and np.float64(a.inlier_rmse).tobytes() == np.float64(b.inlier_rmse).tobytes()


def _conditions(ref, tag):
    assert min(ref.margins, default=np.inf) >= sc.MARGIN_MIN, tag
    assert max(ref.conds, default=1.0) <= sc.COND_MAX, tag


def _same(out, ref, tag):
    """the gate, on a reference whose conditions hold"""
    T, fit, rmse, it = ref.result
    print(f"[{tag}] iterations {out.iterations} / {it}, d fitness {abs(out.fitness - fit):.1e}, d rmse {abs(out.inlier_rmse - rmse):.1e}, "
          f"max |dT| {np.abs(out.transformation - T).max():.1e}; stop margin >= {min(ref.margins, default=np.inf):.1e}, "
          f"cond <= {max(ref.conds, default=1.0):.0f}")
    _conditions(ref, tag)
    assert out.iterations == it, tag
    assert abs(out.fitness - fit) < 1e-12 and abs(out.inlier_rmse - rmse) < 1e-9, tag
    assert np.abs(out.transformation - T).max() < 1e-9, tag


def _three_ways(row, gpu):
    """a row through the synchronous op from a host start and from a device start and through IcpJob: each inside the gate, the job
    and the synchronous call from the same device start equal bit for bit (and the host start, which holds the same numbers)"""
    s, t, nrm, T0d = _device_inputs(row.case, gpu)
    nrm = _normals(row.estimator, nrm)
    ref = sc.reference(row)
    rel = (row.relative_fitness, row.relative_rmse)
    host = _sync(row.estimator, s, t, nrm, sc.inputs(row.case).T0, row.max_dist, row.max_iteration, *rel)
    dev = _sync(row.estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration, *rel)
    job = _job(row.estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration, *rel)
    got = job.result()
    for name, out in (("host start", host), ("device start", dev), ("job", got)):
        _same(out, ref, f"{sc.row_id(row)} {name}")
        assert out.iterations == row.iterations
    assert _bits_equal(got, dev) and _bits_equal(host, dev)
    return job


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("row", [r for r in sc.ROWS if r.kind != "never"], ids=sc.row_id)
def test_thresholds(gpu, row):
    _three_ways(row, gpu)
    if row.kind == "swap":
        # and the same pair the other way round ends where the reference says it ends, elsewhere
        s, t, nrm, T0d = _device_inputs(row.case, gpu)
        other = _sync(row.estimator, s, t, _normals(row.estimator, nrm), T0d, row.max_dist, row.max_iteration, row.relative_rmse,
                      row.relative_fitness)
        _same(other, sc.reference(row, swapped=True), f"{sc.row_id(row)} swapped")
        assert other.iterations == row.swapped != row.iterations


@pytest.mark.parametrize("row", [r for r in sc.ROWS if r.kind == "never"], ids=sc.row_id)
def test_batch_edges(gpu, row):
    """thresholds of 0 never stop a run: exactly max_iteration updates on either side of the host's batch edges (4, then 8 pairs at a
    time), and the job has enqueued what the host loop implies"""
    job = _three_ways(row, gpu)
    assert row.iterations == row.max_iteration
    assert job.launched == sc.NEVER_LAUNCHED[row.max_iteration] and job.launched in (4, 12, 20)


@pytest.mark.parametrize("estimator", sc.ESTIMATORS)
def test_jobs_with_other_thresholds_side_by_side(gpu, estimator):
    """a job with a row's thresholds next to one with the defaults on the same stream (a workspace each): each returns what it returns
    alone, and the two differ"""
    row = next(r for r in sc.ROWS if r.estimator == estimator and r.kind == "rmse_withholds")
    s, t, nrm, T0d = _device_inputs(row.case, gpu)
    nrm = _normals(estimator, nrm)
    rel = (row.relative_fitness, row.relative_rmse)
    solo_row = _job(estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration, *rel).result()
    solo_def = _job(estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration).result()
    for order in (0, 1):
        a = _job(estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration, *(rel if order == 0 else ()))
        b = _job(estimator, s, t, nrm, T0d, row.max_dist, row.max_iteration, *(() if order == 0 else rel))
        assert sorted((a.slot, b.slot)) == [0, 1]
        with_row, with_def = (a, b) if order == 0 else (b, a)
        assert _bits_equal(with_row.result(), solo_row) and _bits_equal(with_def.result(), solo_def)
    _same(solo_row, sc.reference(row), f"{estimator} row thresholds")
    _same(solo_def, sc.reference(row, defaults=True), f"{estimator} default thresholds")
    assert solo_row.iterations != solo_def.iterations


# ------------------------------------------------------------------------------------------------ trajectory
class _Chain:
    """the raw enqueue-only entry of an estimator on a row, with a workspace and a pinned state buffer of its own"""

    def __init__(self, row, gpu):
        from umeregrobust_amd import _lib, ops
        self.lib, self.call, self.gpu = _lib.load(), _lib.call, gpu
        s, t, nrm, self.T0d = _device_inputs(row.case, gpu)
        nrm = _normals(row.estimator, nrm)
        size, _, _, self.entry = ops._icp_entries(self.lib, len(nrm))
        n, m = s.shape[0], t.shape[0]
        self.ws = torch.zeros(int(size(n, m)), dtype=torch.uint8, device=gpu)
        self.n_state = int(self.lib.umereg_icp_state_bytes())
        self.state = torch.zeros(self.n_state, dtype=torch.uint8).pin_memory()
        self.head = [s.data_ptr(), t.data_ptr()] + [x.data_ptr() for x in nrm] + [n, m]
        self.par = [float(row.max_dist), int(row.max_iteration), float(row.relative_fitness), float(row.relative_rmse)] \
            + ([EPSILON] if len(nrm) == 2 else [])
        self.keep = (s, t, nrm)
        # the workspace's tail: the state (256 bytes), then one row of partial sums per 64 source points
        self.partial_bytes = -(-((n + 63) // 64) * SUMS[row.estimator] * 8 // 256) * 256
        self.state_off = self.ws.numel() - self.partial_bytes - 256

    def run(self, first, iterations):
        """-> (T [4,4], fitness, rmse, iters, done, the state's bytes) after `iterations` more pairs"""
        self.call(self.gpu, self.entry, *self.head, self.T0d.data_ptr(), *self.par, int(first), int(iterations), self.state.data_ptr(),
                  self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream(self.gpu).cuda_stream)
        torch.cuda.synchronize()
        T, fr, it = np.empty((4, 4)), np.zeros(2), np.zeros(2, np.int32)
        assert self.lib.umereg_icp_state_decode(self.state.data_ptr(), T.ctypes.data, fr.ctypes.data, fr.ctypes.data + 8, it.ctypes.data,
                                                it.ctypes.data + 4) == 0
        return T, float(fr[0]), float(fr[1]), int(it[0]), int(it[1]), self.state.numpy().tobytes()

    def device_state(self):
        return self.ws[self.state_off:self.state_off + self.n_state].cpu().numpy().tobytes()

    def partial(self):
        return self.ws[self.state_off + 256:]


@pytest.mark.parametrize("estimator", sc.ESTIMATORS)
def test_trajectory(gpu, estimator):
    """pair by pair through the enqueue-only entry.  While `done` is 0, after pair k the state holds iters = k, the k-th transform,
    and the fitness / rmse of transform k - 1 (the evaluation the update was computed from).  The pair that stops leaves the
    transform alone and holds the fitness / rmse of that transform.  From then on no queued pair writes a byte, of the state or of
    the partial sums."""
    row = sc.TRAJECTORY[estimator]
    ref = sc.reference(row)
    _conditions(ref, estimator)
    trace, K = ref.trace, ref.result[3]
    assert K == row.iterations >= 6 and len(trace) == K + 1
    chain = _Chain(row, gpu)
    after, T_before = {}, None
    for k in range(1, K + 2):
        T, fit, rmse, iters, done, raw = chain.run(k == 1, 1)
        after[k] = raw
        was = trace[k - 1]                                  # the evaluation pair k made
        print(f"[{estimator} pair {k}] iters {iters} done {done}, d fitness {abs(fit - was[1]):.1e}, d rmse {abs(rmse - was[2]):.1e}, "
              f"max |dT| {np.abs(T - trace[min(k, K)][0]).max():.1e}")
        assert abs(fit - was[1]) < 1e-12 and abs(rmse - was[2]) < 1e-9, k
        assert np.abs(T - trace[min(k, K)][0]).max() < 1e-9, k
        assert (iters, done) == ((k, 0) if k <= K else (K, 1)), k
        if k == K + 1:
            assert T.tobytes() == T_before.tobytes()          # the stopping pair does not touch the transform
        T_before = T
    final = after[K + 1]
    assert chain.device_state() == final                   # the layout this test assumes for the workspace's tail
    # the latch: the partial sums overwritten with a canary, three more single pairs and a call of no pair -- nothing moves
    chain.partial().fill_(0xA5)
    for it in (1, 1, 1, 0):
        assert chain.run(False, it)[5] == final
    assert chain.device_state() == final and bool((chain.partial() == 0xA5).all())
    # one call of k pairs ends in the bytes of k single calls: in the middle, at the stop, and beyond it
    for k in (3, K + 1, K + 4):
        assert _Chain(row, gpu).run(True, k)[5] == after[min(k, K + 1)], k
    # and the ops return that state
    out = _sync(estimator, *chain.keep[:2], chain.keep[2], chain.T0d, row.max_dist, row.max_iteration, row.relative_fitness,
                row.relative_rmse)
    T, fit, rmse, iters, done, _ = chain.run(False, 0)
    assert out.transformation.tobytes() == T.tobytes() and (out.fitness, out.inlier_rmse, out.iterations) == (fit, rmse, iters)


# ------------------------------------------------------------------------------------------------ second stride
@pytest.mark.parametrize("n_src", sc.STRIDE_N_SRC)
@pytest.mark.parametrize("estimator", sc.ESTIMATORS)
def test_totals_second_stride(gpu, estimator, n_src):
    """256, 257 and 258 rows of partial sums: thread t of icp_step_kernel sums rows t, t + 256, so threads 0 and 1 go round a second
    time for the last two counts, whose rows 256 and 257 hold one matched point each (17 sums for point to point, 29 for the two
    plane estimators, the latter fed by icp_eval_kernel's point-to-plane and plane-to-plane instantiations)"""
    s, t, nrm, T0d = _device_inputs("stride", gpu)
    s = s[:n_src].contiguous()
    nrm = _normals(estimator, nrm, n_src)
    T0 = sc.stride_inputs().T0
    for max_it in sc.STRIDE_MAX_ITERATIONS:
        ref = sc.stride_reference(estimator, n_src, max_it)
        _same(_sync(estimator, s, t, nrm, T0, sc.STRIDE_MAX_DIST, max_it), ref, f"{estimator} n_src={n_src} max_it={max_it}")
    job = _job(estimator, s, t, nrm, T0d, sc.STRIDE_MAX_DIST, max_it)
    _same(job.result(), ref, f"{estimator} n_src={n_src} max_it={max_it} job")
