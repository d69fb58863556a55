"""CPU: the table of tests/icp_stop_cases.py is what it claims to be for the fp64 restatements, the restatements' `trace` changes
nothing, and the two threshold slots of the nine ICP entries are doubles that the wrappers fill in the order (relative_fitness,
relative_rmse).  Nothing here needs a device."""
import ast
import inspect
import os
import re
import textwrap
from ctypes import c_double, c_float, c_int

import numpy as np
import pytest
import torch

import abi_headers
import icp_gicp_ref as gicp
import icp_plane_ref as plane
import icp_stop_cases as sc
from oracle import oracle as orc

KINDS = ("fitness_withholds", "rmse_withholds", "swap", "strict", "immediate", "never")


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_has_every_row_for_every_estimator():
    for est in sc.ESTIMATORS:
        rows = [r for r in sc.ROWS if r.estimator == est]
        assert {r.kind for r in rows} == set(KINDS), est
        assert sorted(r.max_iteration for r in rows if r.kind == "never") == sorted(sc.NEVER_MAX_ITERATIONS), est
        t = sc.TRAJECTORY[est]
        assert t in rows and t.iterations >= 6 and t.iterations < t.max_iteration, est      # at least 6 updates, then a threshold stop
    assert len({sc.row_id(r) for r in sc.ROWS}) == len(sc.ROWS)
    for c in ("lattice8", "corner0x3", "corner0x2", "corner1x2"):
        T0 = sc.inputs(c).T0
        assert np.array_equal(T0, T0.astype(np.float32).astype(np.float64)), c       # one start for the host and the device entry


@pytest.mark.parametrize("row", sc.ROWS, ids=sc.row_id)
def test_row_is_what_it_claims(row):
    ref = sc.reference(row)
    T, fit, rmse, it = ref.result
    tests = ref.trace[1:]                                   # one stop test per update
    print(f"[{sc.row_id(row)}] iterations {it}, smallest margin {min(ref.margins):.2e}, largest condition number "
          f"{max(ref.conds, default=1.0):.0f}")
    assert it == row.iterations and len(ref.trace) == it + 1
    # the two conditions on the inputs
    assert min(ref.margins) >= sc.MARGIN_MIN
    assert (len(ref.conds) == it and max(ref.conds) <= sc.COND_MAX) if row.estimator != "point_to_point" else not ref.conds
    # the stop is the rule's: no test before the last one stopped, the last one did unless the limit ended the run
    assert not any(t[5] for t in tests[:-1])
    rf, rr = row.relative_fitness, row.relative_rmse
    for _, _, _, df, dr, stopped in tests:
        assert stopped == (df < rf and dr < rr)
    if row.kind == "fitness_withholds":
        assert tests[-1][5] and any(dr < rr and not df < rf for _, _, _, df, dr, _ in tests[:-1])
    elif row.kind == "rmse_withholds":
        assert tests[-1][5] and any(df < rf and not dr < rr for _, _, _, df, dr, _ in tests[:-1])
    elif row.kind == "swap":
        other = sc.reference(row, swapped=True)
        assert rf != rr and tests[-1][5] and other.trace[-1][5]
        assert other.result[3] == row.swapped != it
        assert min(other.margins) >= sc.MARGIN_MIN and max(other.conds, default=1.0) <= sc.COND_MAX
    elif row.kind == "strict":
        # the fitness repeats exactly well before the limit, and the rmse half would let the run stop there: `<=` would have stopped
        first = next(k for k, t in enumerate(tests, 1) if t[3] == 0.0)
        assert rf == 0.0 and first <= it - 3 and all(t[4] < rr for t in tests)
        assert it == row.max_iteration and not tests[-1][5]
    elif row.kind == "immediate":
        assert it == 1 and tests[-1][5] and all(rf > t[3] and rr > t[4] for t in sc.reference(row, defaults=True).trace[1:])
    else:
        assert rf == 0.0 and rr == 0.0 and it == row.max_iteration and not tests[-1][5]
        assert sc.NEVER_LAUNCHED[row.max_iteration] == _launched(row.max_iteration, it)
    # non-default thresholds matter on every row that stops by them: the defaults end elsewhere or the row is not about that
    if row.kind in ("rmse_withholds", "immediate"):
        assert sc.reference(row, defaults=True).result[3] != it


def _launched(max_iteration, iterations):
    """the host loop of icp_run / IcpJob.result for a run whose stop test never fires: pairs enqueued when it ends.  `done` is set by
    the pair that finds iters >= max_iteration, pair max_iteration + 1."""
    launched = 0
    while True:
        launched += 4 if launched == 0 else 8
        done = launched >= iterations + 1
        if done or launched > max_iteration + 1:
            return launched


def test_never_launched_is_one_of_4_12_20():
    assert [sc.NEVER_LAUNCHED[m] for m in sc.NEVER_MAX_ITERATIONS] == [4, 12, 12, 12, 20, 20]
    assert [_launched(m, m) for m in sc.NEVER_MAX_ITERATIONS] == [4, 12, 12, 12, 20, 20]


@pytest.mark.parametrize("estimator", sc.ESTIMATORS)
def test_second_stride_cases(estimator):
    """the inputs' conditions, and that the rows a stride of 512 would skip carry weight: source points 16 384 and 16 448, the only
    ones of rows 256 and 257, have a correspondence at the start"""
    c = sc.stride_inputs()
    assert c.src.shape == (max(sc.STRIDE_N_SRC), 3) and c.tgt.shape == (2000, 3) and c.ns.shape == c.src.shape
    assert [(n + 63) // 64 for n in sc.STRIDE_N_SRC] == [256, 257, 258]
    idx = orc.icp_evaluate(c.src, c.tgt, c.T0, sc.STRIDE_MAX_DIST)[0]
    assert idx[16384] >= 0 and idx[16448] >= 0
    for n_src in sc.STRIDE_N_SRC:
        for max_it in sc.STRIDE_MAX_ITERATIONS:
            ref = sc.stride_reference(estimator, n_src, max_it)
            print(f"[{estimator} n_src={n_src} max_it={max_it}] iterations {ref.result[3]}, margin {min(ref.margins):.2e}, "
                  f"condition number {max(ref.conds, default=1.0):.0f}")
            assert 1 <= ref.result[3] <= max_it
            assert min(ref.margins) >= sc.MARGIN_MIN and max(ref.conds, default=1.0) <= sc.COND_MAX


# ------------------------------------------------------------------------------------------------ trace
def _bits(res):
    T, fit, rmse, it = res
    return T.tobytes(), np.float64(fit).tobytes(), np.float64(rmse).tobytes(), it


@pytest.mark.parametrize("estimator", sc.ESTIMATORS)
def test_trace_changes_nothing(estimator):
    """with and without `trace` the restatements return the same bits (at the defaults and at a row's thresholds), and what they
    return without it is a 4-tuple as before; the records are the run's own evaluations"""
    row = sc.TRAJECTORY[estimator]
    c = sc.inputs(row.case)
    for rel in ((), (row.relative_fitness, row.relative_rmse)):
        if estimator == "point_to_point":
            run = lambda **kw: orc.icp_point_to_point(c.src, c.tgt, c.T0, row.max_dist, 30, *rel, **kw)          # noqa: E731
        elif estimator == "point_to_plane":
            run = lambda **kw: plane.icp_point_to_plane(c.src, c.tgt, c.nt, c.T0, row.max_dist, 30, *rel, **kw)   # noqa: E731
        else:
            run = lambda **kw: gicp.icp_plane_to_plane(c.src, c.tgt, c.ns, c.nt, c.T0, row.max_dist, 30, *rel, **kw)   # noqa: E731
        plain, trace = run(), []
        traced = run(trace=trace)
        assert len(plain) == 4 and plain[0].shape == (4, 4) and plain[0].dtype == np.float64 and isinstance(plain[3], int)
        assert _bits(plain) == _bits(traced)
        T, fit, rmse, it = traced
        assert len(trace) == it + 1 and trace[0][3] is None and trace[0][4] is None and trace[0][5] is False
        assert np.array_equal(trace[0][0], c.T0) and np.array_equal(trace[-1][0], T) and trace[-1][1:3] == (fit, rmse)
        for prev, rec in zip(trace, trace[1:]):
            assert rec[3] == abs(prev[1] - rec[1]) and rec[4] == abs(prev[2] - rec[2])
            # a record's fitness and rmse are those of the transform it names
            assert orc.icp_evaluate(c.src, c.tgt, rec[0], row.max_dist)[1:3] == rec[1:3]
        assert trace[-1][5] and not any(r[5] for r in trace[:-1])
    # the other optional lists still work next to it
    if estimator == "plane_to_plane":
        conds, margins, trace = [], [], []
        gicp.icp_plane_to_plane(c.src, c.tgt, c.ns, c.nt, c.T0, row.max_dist, 30, row.relative_fitness, row.relative_rmse, conds=conds,
                                margins=margins, trace=trace)
        assert margins == sc.margins(trace, row.relative_fitness, row.relative_rmse) and len(conds) == len(margins)


def test_margins_ignore_a_comparison_against_zero():
    T = np.eye(4)
    trace = [(T, 1.0, 0.1, None, None, False), (T, 1.0, 0.2, 0.0, 0.1, False), (T, 0.5, 0.2, 0.5, 0.0, False)]
    assert sc.margins(trace, 0.0, 1.0) == [np.inf, np.inf]
    assert sc.margins(trace, 0.25, 0.0) == [np.inf, np.inf]
    assert sc.margins(trace, 0.25, 0.05) == [pytest.approx(0.05), pytest.approx(0.25)]
    assert sc.margins(trace[:2] + [(T, 1.0, 0.2, 0.0, 0.0, True)], 0.25, 0.05) == [pytest.approx(0.05), pytest.approx(0.05)]


# ------------------------------------------------------------------------------------------------ the threshold slots
def _tables():
    from umeregrobust_amd import _lib
    return (("umereg.h", _lib.TABLES["umereg.h"], ("umereg_icp_point_to_point_f32", "umereg_icp_point_to_point_dev_f32",
                                                   "umereg_icp_enqueue_f32")),
            ("umereg_icp_plane.h", _lib.TABLES["umereg_icp_plane.h"],
             ("umereg_icp_point_to_plane_f32", "umereg_icp_point_to_plane_dev_f32", "umereg_icp_plane_enqueue_f32")),
            ("umereg_icp_gicp.h", _lib.TABLES["umereg_icp_gicp.h"],
             ("umereg_icp_plane_to_plane_f32", "umereg_icp_plane_to_plane_dev_f32", "umereg_icp_plane_to_plane_enqueue_f32")))


def _header_params(header, name):
    """the declaration's parameters as (type, name) pairs"""
    out = []
    for p in abi_headers.params(header, name).split(","):
        words = p.replace("*", "* ").split()
        out.append((" ".join(words[:-1]).replace(" *", "*"), words[-1]))
    return out


def _threshold_slots(argtypes):
    """(index of relative_fitness, of relative_rmse) in an ICP entry's argument list: behind the distance (the first float) and
    max_iteration"""
    d = argtypes.index(c_float)
    assert argtypes[d + 1] is c_int
    return d + 2, d + 3


def test_threshold_slots_are_doubles_in_the_tables_and_the_headers():
    seen = 0
    for header, table, names in _tables():
        for name in names:
            argtypes = table[name][1]
            f, r = _threshold_slots(argtypes)
            assert argtypes[f] is c_double and argtypes[r] is c_double, name
            params = _header_params(header, name)
            assert len(params) == len(argtypes), name
            assert params[f - 1] == ("int", "max_iteration"), name
            assert params[f] == ("double", "relative_fitness") and params[r] == ("double", "relative_rmse"), name
            assert params[f - 2] == ("float", "max_correspondence_distance"), name
            seen += 1
    assert seen == 9


def test_the_definitions_hand_the_thresholds_on_in_order():
    """csrc/icp.hip: every one of the nine entries puts (relative_fitness, relative_rmse) into the call's record in that order, which
    is the order of the record's fields, and the one launch of icp_step_kernel takes them from the record in the order of its
    parameters (rel_fitness, rel_rmse)"""
    from umeregrobust_amd import _build
    text = open(os.path.join(_build.CSRC, "icp.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    pairs = re.findall(r"\b(relative_\w+)\s*,\s*(?:double\s+|m\.)?(relative_\w+)", text)
    assert len(pairs) == 9 + 9 + 1 + 1               # the entries' parameters, what they put into the record, its fields, the step launch
    assert set(pairs) == {("relative_fitness", "relative_rmse")}
    assert len(re.findall(r"\brelative_fitness\b", text)) == len(re.findall(r"\brelative_rmse\b", text)) == len(pairs)
    assert re.search(r"int max_iter, double rel_fitness, double rel_rmse,", text)
    assert len(re.findall(r"m\.max_iteration,\s*m\.relative_fitness, m\.relative_rmse, state\);", text)) == 1
    assert len(re.findall(r"\bicp_step_kernel<", text)) == 1


def test_sync_wrappers_pass_fitness_before_rmse(monkeypatch):
    """ops.icp_point_to_point / icp_point_to_plane / icp_plane_to_plane with a recording stand-in for the native call: the value given
    as relative_fitness lands in the slot the table types for it, relative_rmse in the next, both unrounded doubles"""
    from umeregrobust_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_dev", lambda t, name, dtype=torch.float32: t)
    monkeypatch.setattr(ops, "_workspace", lambda dev, nbytes, tag: torch.zeros(8, dtype=torch.uint8))
    monkeypatch.setattr(ops, "_stream_ptr", lambda dev: 0)
    monkeypatch.setattr(ops, "_icp_entries", lambda lib, n_normals: (lambda n, m: 8, "from_host", "from_dev", "enqueue"))
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(_lib, "call", lambda dev, fn, *args: calls.append((fn, args)))
    s, t = torch.zeros(5, 3), torch.zeros(7, 3)
    rf, rr = 0.1 + 2.0 ** -40, 0.3 + 2.0 ** -41                 # neither survives a trip through float
    tables = {h: (tab, names) for h, tab, names in _tables()}
    for header, run in (("umereg.h", lambda **kw: ops.icp_point_to_point(s, t, np.eye(4), 0.2, 17, **kw)),
                        ("umereg_icp_plane.h", lambda **kw: ops.icp_point_to_plane(s, t, t.clone(), np.eye(4), 0.2, 17, **kw)),
                        ("umereg_icp_gicp.h", lambda **kw: ops.icp_plane_to_plane(s, t, s.clone(), t.clone(), np.eye(4), 0.2, 17, **kw))):
        table, names = tables[header]
        f, r = _threshold_slots(table[names[0]][1])
        for kw, want in ((dict(relative_fitness=rf, relative_rmse=rr), (rf, rr)), (dict(relative_rmse=rr), (1e-6, rr)),
                         (dict(relative_fitness=rf), (rf, 1e-6)), ({}, (1e-6, 1e-6))):
            del calls[:]
            run(**kw)
            (fn, args), = calls
            assert fn == "from_host" and len(args) == len(table[names[0]][1])
            assert args[f - 1] == 17 and (args[f], args[r]) == want, (header, kw)
    # positionally, the two follow max_iteration in that order
    del calls[:]
    ops.icp_point_to_point(s, t, np.eye(4), 0.2, 17, rf, rr)
    ops.icp_point_to_plane(s, t, t.clone(), np.eye(4), 0.2, 17, rf, rr)
    ops.icp_plane_to_plane(s, t, s.clone(), t.clone(), np.eye(4), 0.2, 17, rf, rr)
    for (fn, args), header in zip(calls, ("umereg.h", "umereg_icp_plane.h", "umereg_icp_gicp.h")):
        f, r = _threshold_slots(tables[header][0][tables[header][1][0]][1])
        assert (args[f], args[r]) == (rf, rr)


def test_icp_job_passes_fitness_before_rmse():
    """IcpJob keeps (distance, max_iteration, relative_fitness, relative_rmse[, epsilon]) in self.par and unpacks it behind the start
    transform, where the enqueue-only entries expect it; its signature has the two in the order of the ops'.  Read from the source:
    the constructor needs a device."""
    from umeregrobust_amd import ops
    names = list(inspect.signature(ops.IcpJob.__init__).parameters)
    assert names[4:8] == ["max_correspondence_distance", "max_iteration", "relative_fitness", "relative_rmse"]
    for fn in (ops.icp_point_to_point, ops.icp_point_to_plane, ops.icp_plane_to_plane):
        p = list(inspect.signature(fn).parameters)
        k = p.index("max_iteration")
        assert p[k + 1:k + 3] == ["relative_fitness", "relative_rmse"]
    tree = ast.parse(textwrap.dedent(inspect.getsource(ops.IcpJob)))
    par = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "self.par"]
    assert len(par) == 1
    assert ast.unparse(par[0].value) == ("(float(max_correspondence_distance), int(max_iteration), float(relative_fitness), "
                                         "float(relative_rmse)) + eps")
    enqueue = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_enqueue")
    call, = [n for n in ast.walk(enqueue) if isinstance(n, ast.Call) and ast.unparse(n.func) == "_lib.call"]
    args = [ast.unparse(a) for a in call.args]
    k = args.index("*self.par")
    assert args[k - 1] == "_ptr(self.T0)" and args[k + 1] == "1 if first else 0" and args[k + 2] == "int(iterations)"
    assert args[k - 3:k - 1] == ["self.sp.shape[0]", "self.tp.shape[0]"]
    # result() reads the limit of its loop from the slot max_iteration has there
    assert "self.launched > self.par[1] + 1" in inspect.getsource(ops.IcpJob.result)
