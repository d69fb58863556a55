"""CPU: the C-ABI shared library builds, loads WITHOUT a GPU and exports every symbol include/umereg.h
declares; without a device every compute entry point refuses with UMEREG_ENODEV (no CPU fallback)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


import abi_headers


def _alias(attr):
    import importlib
    module, name = attr.split(".")
    return getattr(importlib.import_module("umeregrobust_amd." + module), name)


def test_library_builds_and_one_table_per_header():
    """the library builds and loads; include/ holds the seventeen headers, _lib.TABLES one table for each, no symbol in two of them"""
    import umeregrobust_amd
    from umeregrobust_amd import _lib
    assert os.path.exists(umeregrobust_amd.build_native())
    assert sorted(os.listdir(abi_headers.INCLUDE)) == sorted(abi_headers.HEADERS) == sorted(_lib.TABLES) and len(_lib.TABLES) == 17
    assert _lib.TABLES["umereg.h"] is _lib.SIGNATURES
    names = [name for table in _lib.TABLES.values() for name in table]
    assert len(names) == len(set(names)) == 130, sorted(n for n in set(names) if names.count(n) > 1)
    assert _lib.load().umereg_abi_version() == _lib.ABI_VERSION == 2


# what a declaration returns -> the restype its table entry must carry
RESTYPES = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "const char*": ctypes.c_char_p}


@pytest.mark.parametrize("header", list(abi_headers.HEADERS))
def test_table_mirrors_its_header_and_every_symbol_is_exported(header):
    """Per header: the table's keys are the header's symbols (their number pinned), the built library exports each, every
    declaration has as many parameters as the table has argtypes and returns what the table's restype says (size_t, int or
    const char*), the module's public alias IS the table, and no symbol of it is in another header's table."""
    import umeregrobust_amd
    from umeregrobust_amd import _lib
    alias, count = abi_headers.HEADERS[header]
    table = _lib.TABLES[header]
    assert _alias(alias) is table
    declared, returns = abi_headers.declarations(header), abi_headers.return_types(header)
    assert sorted(table) == sorted(declared) == sorted(returns) and len(declared) == count
    lib = ctypes.CDLL(umeregrobust_amd.build_native())
    for name, n_params in declared.items():
        assert hasattr(lib, name), f"{name} declared in include/{header} but not exported"
        assert len(table[name][1]) == n_params, name
        assert table[name][0] is RESTYPES[returns[name]], (name, returns[name])
    for other, theirs in _lib.TABLES.items():
        assert other == header or not set(table) & set(theirs), (header, other)
    assert _lib.load().umereg_abi_version() == _lib.ABI_VERSION == 2


class _Entry:
    """what `call` and `checked` need of a ctypes function: a name and a status"""

    def __init__(self, status, log):
        self.__name__, self.status, self.log = "umereg_fake_entry", status, log

    def __call__(self, *args):
        self.log.append(("call", args))
        return self.status


@pytest.fixture
def guard_log(monkeypatch):
    import torch
    log = []

    class Guard:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            log.append(("enter", self.dev))

        def __exit__(self, *exc):
            log.append(("exit", self.dev))

    monkeypatch.setattr(torch.cuda, "device", Guard)
    return log


def test_call_runs_the_entry_inside_the_guard_of_the_device_given(guard_log):
    from umeregrobust_amd import _lib
    dev = object()
    assert _lib.call(dev, _Entry(0, guard_log), 1, None, 2.5) is None
    assert guard_log == [("enter", dev), ("call", (1, None, 2.5)), ("exit", dev)] and guard_log[0][1] is dev
    del guard_log[:]
    with pytest.raises(RuntimeError, match=r"umereg_fake_entry failed \(code -3\)"):
        _lib.call(dev, _Entry(-3, guard_log), 7)
    assert guard_log == [("enter", dev), ("call", (7,)), ("exit", dev)]


def test_checked_never_enters_a_guard(guard_log):
    from umeregrobust_amd import _lib
    assert _lib.checked(_Entry(0, guard_log), 1, 2) is None
    with pytest.raises(RuntimeError, match=r"umereg_fake_entry failed \(code 5\)") as e:
        _lib.checked(_Entry(5, guard_log))
    assert e.value.code == 5
    assert guard_log == [("call", (1, 2)), ("call", ())]


# entries whose int is a value, not a status
NOT_A_STATUS = {"umereg_abi_version", "umereg_device_count", "umereg_sparse_conv_wgrad_segments"}


def test_no_status_entry_is_called_directly():
    """Every entry that returns a status goes through _lib.call / _lib.checked (which name the entry that failed and, for `call`,
    make the tensors' device current): nowhere under umeregrobust_amd/ is one called as `lib.umereg_...(`."""
    from umeregrobust_amd import _lib
    status = {name for table in _lib.TABLES.values() for name, (res, _) in table.items() if res is ctypes.c_int} - NOT_A_STATUS
    assert len(status) == 92 and NOT_A_STATUS <= {n for t in _lib.TABLES.values() for n in t}
    pkg, seen = os.path.join(REPO, "umeregrobust_amd"), 0
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                called = re.findall(r"\.(umereg_\w+)\(", open(os.path.join(root, f)).read())
                seen += len(called)
                assert not set(called) & status, f"{os.path.join(root, f)} calls {sorted(set(called) & status)} directly"
    assert seen >= 30      # (the size queries: the scan does see the package's calls)


def test_load_typed_types_a_table_once_and_names_a_missing_symbol():
    """_lib.load_typed: the loader for a table from outside the package (every module's own load_native is _lib.load)"""
    from umeregrobust_amd import _lib, gt_matches
    lib = _lib.load_typed(gt_matches.GT_MATCH_SIGNATURES)
    assert lib is _lib.load() and lib is gt_matches.load_native()
    assert lib.umereg_gt_matches_workspace_bytes.restype is ctypes.c_size_t
    assert lib.umereg_gt_matches_workspace_bytes.argtypes == [ctypes.c_int] * 3
    tables = len(_lib._typed)
    assert _lib.load_typed(gt_matches.GT_MATCH_SIGNATURES) is lib and len(_lib._typed) == tables
    with pytest.raises(_lib.NativeLibraryError, match="does not export umereg_no_such_entry"):
        _lib.load_typed({"umereg_no_such_entry": (ctypes.c_int, [])})
    assert len(_lib._typed) == tables


def test_no_cpu_fallback_without_device():
    import torch
    from umeregrobust_amd import _lib, ops
    lib = _lib.load()
    if lib.umereg_device_count(None, 0) > 0:
        pytest.skip("a HIP device is visible; this test is about the GPU-less behaviour")
    buf = (ctypes.c_float * 1024)()
    out = (ctypes.c_float * 64)()
    rc = lib.umereg_rre_deg_f32(buf, buf, 4, out, None)
    assert rc == -2 and b"no CPU fallback" in lib.umereg_last_error()          # UMEREG_ENODEV
    assert lib.umereg_match_prob_f32(buf, 16, 0.05, out, None) == -2
    # argument errors are reported before the device probe
    assert lib.umereg_rre_deg_f32(None, buf, 4, out, None) == -1
    assert b"null" in lib.umereg_last_error()
    # the torch-facing ops refuse CPU tensors instead of computing on the host
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ume_cdist(torch.zeros(1, 4, 32, 4), torch.zeros(1, 4, 32, 4))
    # size queries are pure host arithmetic and work anywhere
    assert lib.umereg_ume_moments_workspace_bytes(1, 50000) > 50000 * 32
    assert lib.umereg_qbasis_bytes(10000, 3) == 10112 * 512


# (Ns, Nt, M, flags, bytes): umereg_corr_workspace_bytes_ex of the library BEFORE the layout moved into corr_ws (corr.hip), on both
# sides of every branch of the layout.  Flag values: include/umereg.h.
_CORR_WS_BYTES = [
    (100, 100, 10, 0x0, 255744), (5000, 6000, 300, 0x0, 84728576), (5000, 6000, 300, 0xa, 84728576), (5000, 6000, 300, 0x1a, 84728576),
    (5000, 6000, 300, 0xa000a, 102078464), (5000, 6000, 300, 0x28000a, 102302976),
    (10000, 10000, 2500, 0x0, 573977088), (10000, 10000, 2500, 0x1, 4399872), (10000, 10000, 2500, 0x200000, 808176640),
    (30000, 30000, 5000, 0x0, 2548424704), (30000, 30000, 5000, 0x200000, 2567565568), (70000, 70000, 5000, 0x0, 40666880),
    # M x Ns below and at 2^17, with and without FORCE_LATTICE (2), and with the consensus pass forced on top (8)
    (1024, 2000, 127, 0x0, 579840), (1024, 2000, 127, 0x2, 12118016), (1024, 2000, 128, 0x0, 12166400), (1024, 2000, 128, 0x2, 12166400),
    (1024, 2000, 127, 0xa, 12685312), (1024, 2000, 128, 0x8, 12737792),
    # NO_LATTICE (1), whatever else is set
    (5000, 6000, 300, 0x1, 1750272), (5000, 6000, 300, 0x20000b, 1750272),
    # 16-bit list entries: Nt at 65471 and 65472
    (5000, 65471, 300, 0x0, 95243008), (5000, 65472, 300, 0x0, 12264704), (5000, 65472, 300, 0x200002, 12264704),
    # M at 255 and 256, FORCE_CONSENSUS (8) / NO_CONSENSUS (4)
    (5000, 6000, 255, 0x0, 67538944), (5000, 6000, 256, 0x0, 73323520), (5000, 6000, 255, 0x8, 73065728), (5000, 6000, 256, 0x4, 67776000),
    (5000, 6000, 256, 0x20000c, 67959552),
    # M x Ns at 2^24 - 1, 2^24, 2^25 - 1, 2^25, without and with BOUND_OUTSIDE (1 << 21)
    (4097, 6000, 4095, 0x0, 480761344), (4097, 6000, 4095, 0x200000, 482925056), (4096, 6000, 4096, 0x0, 480571136),
    (4096, 6000, 4096, 0x200000, 647366400), (18631, 20000, 1801, 0x0, 672310016), (18631, 20000, 1801, 0x200000, 976628224),
    (8192, 8000, 4096, 0x0, 968905984), (8192, 8000, 4096, 0x200000, 973182464),
    # the cell block: CELL_PASS (1 << 19) on a small job; NO_CELL_PASS (1 << 20), LEFT_COOP (1 << 16), CONSENSUS_V1 (32) on big ones
    (5000, 6000, 300, 0x80000, 102078464), (8192, 8000, 4096, 0x100000, 669007360), (8192, 8000, 4096, 0x10000, 669007360),
    (8192, 8000, 4096, 0x20, 669007360), (8192, 8000, 4096, 0x180000, 669007360), (4096, 6000, 4096, 0x300000, 482734080),
    (4096, 6000, 4096, 0x200020, 482734080),
    # NO_FLAT (16) switches the bound block off
    (8192, 8000, 4096, 0x200010, 968905984), (4096, 6000, 4096, 0x200010, 645203456), (10000, 10000, 2500, 0x200010, 804905728),
    # Ns x M >= 2^32: no cell pass (32-bit entries)
    (70000, 60000, 70000, 0x0, 55128904704), (70000, 60000, 70000, 0x200000, 55742665216), (65536, 60000, 65536, 0x80000, 48358834944),
    # flags the layout ignores (SRC_ROWS, RECORD_STAGE, DEBUG_STATS, a far margin); nothing a multiple of 64
    (10000, 10000, 2500, 0x414c0, 573977088), (513, 700, 257, 0x2, 12565248),
]


def test_corr_workspace_layout_is_the_one_python_and_the_tools_rely_on():
    """umereg_corr_workspace_bytes_ex is pure host arithmetic (corr_ws, corr.hip) and must not move: the values below are those of the
    library before the layout got its one function.  And the relation ops.corr_scores_profile, bench.py and the tools rely on: the call's 64
    header words start at bytes_ex(Ns, Nt, M, NO_LATTICE) -- everything in front of the lattice exists for every flag set, everything from
    the lattice on needs it.  So that offset does not depend on the other flags, a call without a lattice has nothing behind it, and a call
    with one has at least the header."""
    from umeregrobust_amd import _lib, ops
    lib = _lib.load()
    assert len(_CORR_WS_BYTES) >= 40 and len(set(_CORR_WS_BYTES)) == len(_CORR_WS_BYTES)
    for Ns, Nt, M, flags, want in _CORR_WS_BYTES:
        assert lib.umereg_corr_workspace_bytes_ex(Ns, Nt, M, flags) == want, (Ns, Nt, M, hex(flags))
    assert lib.umereg_corr_workspace_bytes(10000, 10000, 2500) == 573977088
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
        assert lib.umereg_corr_workspace_bytes_ex(*bad, 0) == 0
    routes = (0, 2, 8, 2 | 8, 4, 16, 32, 128, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 2 | 8 | 1 << 19 | 1 << 21, (1 << 21) | 16)
    for (Ns, Nt, M), off in (((5000, 6000, 300), 1750272), ((10000, 10000, 2500), 4399872), ((1024, 2000, 127), 579840),
                             ((5000, 65472, 300), 12264704), ((4096, 6000, 4096), 2614784), ((70000, 70000, 5000), 40666880)):
        for f in routes:
            assert lib.umereg_corr_workspace_bytes_ex(Ns, Nt, M, f | ops.CORR_NO_LATTICE) == off, (Ns, Nt, M, hex(f))
            total = lib.umereg_corr_workspace_bytes_ex(Ns, Nt, M, f)
            has_lattice = Nt <= 65471 and (M * Ns >= 1 << 17 or f & 2)
            assert (total >= off + 256) if has_lattice else (total == off), (Ns, Nt, M, hex(f), total)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under umeregrobust_amd/ may import or load it."""
    pkg = os.path.join(REPO, "umeregrobust_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(root, f)).read().lower()
                assert "oracle" not in text, f"{os.path.join(root, f)} references the oracle"


def _kernels_of(path):
    text = open(path).read()
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"__launch_bounds__\s*\([^)]*\)", "", text)
    text = re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)", "", text)
    return re.findall(r"__global__\s+void\s+(\w+)\s*\(", text)


def test_corr_kernels_are_launched_where_they_are_defined():
    """The hypothesis-selection sources are five translation units over corr_dev.h and corr_host.h: each of the 42 kernels is
    DEFINED in exactly one of corr_knn / corr_consensus / corr_lattice / corr_leftover.hip and LAUNCHED only from that unit, by the host
    launcher beside it (declared in corr_host.h) -- no kernel is declared across units, so there is no second copy of a signature that
    could disagree with the first.  corr.hip (the one call, host only) and the two headers define, declare and launch none."""
    csrc = os.path.join(REPO, "umeregrobust_amd", "csrc")
    want = {"corr_knn.hip": {"knn_points_kernel", "nn1_points_kernel", "spatial_var_kernel", "colsum_partial_kernel", "feature_weight_kernel",
                             "chunk_box_kernel", "spatial_var_coop_kernel"},
            "corr_consensus.hip": {"mean_rotation_kernel", "rotate_points_kernel", "hyp_median_kernel", "hyp_err_kernel", "hyp_order_kernel",
                                   "chunk_centroid_kernel", "hyp_order_chunk_kernel", "corr_consensus_kernel", "corr_consensus2_kernel"},
            "corr_lattice.hip": {"leftover_decide_kernel", "lattice_mark_kernel", "lattice_far_table_kernel", "lattice_mark_order_kernel",
                                 "lattice_compact_kernel", "lattice_posof_kernel", "lattice_list_kernel", "cell_apply_kernel",
                                 "cell_blockscan_kernel", "cell_scatter_kernel", "bound_pass2_gate_kernel", "far_recompute_kernel",
                                 "corr_cell_kernel"},
            "corr_leftover.hip": {"corr_score_kernel", "leftover_queue_kernel", "corr_score_fallback_kernel", "leftover_flatten_kernel",
                                  "row_norm_kernel", "flat_bound_kernel", "corr_score_flat_kernel", "bound_survivors_kernel",
                                  "corr_score_record2_kernel", "leftover_sum_kernel", "corr_val_slices_kernel", "corr_reduce_kernel",
                                  "corr_select_best_kernel"}}
    every = set().union(*want.values())
    assert len(every) == sum(len(v) for v in want.values()) == 42, "a kernel is listed for two units"
    assert not os.path.exists(os.path.join(csrc, "corr_kernels.h"))
    launches = lambda f: set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", open(os.path.join(csrc, f)).read()))
    for f, names in want.items():
        defined = _kernels_of(os.path.join(csrc, f))                  # (a list: an explicit instantiation or a declaration would repeat a name)
        assert sorted(defined) == sorted(names), f"{f} defines {sorted(defined)}"
        assert launches(f) == names, f"{f} launches {sorted(launches(f))}"
    others = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and f not in want]
    assert {"corr.hip", "corr_dev.h", "corr_host.h"} <= set(others)
    for f in others:
        assert not (set(_kernels_of(os.path.join(csrc, f))) & every), f"{f} defines or declares a kernel of another unit"
        assert not (launches(f) & every), f"{f} launches a kernel of another unit"
    for f in ["corr.hip"] + [f for f in others if f.startswith("corr") and f.endswith(".h")]:
        assert _kernels_of(os.path.join(csrc, f)) == [] and launches(f) == set(), f"{f} defines, declares or launches a kernel"
    assert "hipLaunchKernelGGL" not in open(os.path.join(csrc, "corr.hip")).read()


def test_corr_bit_contracts_are_stated_once():
    """Three bit-level contracts of hypothesis selection have ONE statement each, in corr_dev.h: the image of a source point
    under a hypothesis (hyp_image: the nested-fmaf row form, by pointer rows and by float4 rows), the score of one query from the keys
    coop_knn leaves in LDS (coop_score: the only caller of cauchy_weight_hw) and the bounded mode's slack rule (bound_eps, slack_units,
    slack_publish, slack_value: the slack unit and the sticky saturation bit).  A restated copy that drifts by one operand does not crash;
    a query lands in a lattice cell nobody marked, or a bound under-counts.  Read as text: no corr* source but corr_dev.h spells them."""
    csrc = os.path.join(REPO, "umeregrobust_amd", "csrc")
    forms = {"image, pointer rows": r"fmaf\(\s*\w+\[2\]\s*,[^;]*?fmaf\(\s*\w+\[1\]\s*,[^;]*?\w+\[0\]\s*\*",
             "image, float4 rows": r"fmaf\(\s*(\w+)\.z\s*,[^;]*?fmaf\(\s*\1\.y\s*,[^;]*?\1\.x\s*\*",
             "cauchy_weight_hw(": r"\bcauchy_weight_hw\s*\(",
             "kSlackUnit": r"\bkSlackUnit\b",
             "1ull << 63": r"\b1ull\s*<<\s*63\b"}
    # Sites left inline, {(file, form): occurrences}, each with its reason:
    allowed = {
        # the single-lane bound of corr_score_flat_kernel<3> (one query, lane 0, direct atomics): with slack_units (and with bound_eps) in
        # place of its two lines the kernel's instruction schedule changed, which the refactor that introduced the helpers did not accept
        ("corr_leftover.hip", "kSlackUnit"): 1,
    }
    files = sorted(f for f in os.listdir(csrc) if f.startswith("corr") and f.endswith((".hip", ".h")))
    assert {"corr.hip", "corr_dev.h", "corr_host.h", "corr_knn.hip", "corr_consensus.hip", "corr_lattice.hip", "corr_leftover.hip"} <= set(files)
    dev = open(os.path.join(csrc, "corr_dev.h")).read()
    for name, pat in forms.items():
        assert re.search(pat, dev), f"corr_dev.h no longer states: {name}"
    seen = {}
    for f in files:
        if f == "corr_dev.h":
            continue
        text = open(os.path.join(csrc, f)).read()
        for name, pat in forms.items():
            n = len(re.findall(pat, text))
            if n:
                seen[(f, name)] = n
    assert seen == allowed, f"restated outside corr_dev.h (or a stale exception): {seen}"


def test_match_kernels_are_launched_where_they_are_defined():
    """The matcher sources are four translation units over match_dev.h: each of the eight kernels is DEFINED in exactly
    one of them and LAUNCHED only from that unit -- no kernel is declared across units; the units call each other through the
    public umereg_* entries.  pair_match.hip (host composition) and the shared header define none; the one kernel pair_match.hip
    instantiates is the record writer, a template that grid.h defines and launches."""
    csrc = os.path.join(REPO, "umeregrobust_amd", "csrc")
    units = ("ume_dist.hip", "match_f16r.hip", "match.hip", "pair_match.hip")
    want = {"ume_dist_kernel", "ume_dist_h_kernel", "match_finalize_kernel", "ume_coarse_h_kernel", "pform_pack_kernel",
            "ume_coarse_p_kernel", "match_refine_kernel", "match_prob_kernel"}
    assert not os.path.exists(os.path.join(csrc, "subspace_dist.hip"))
    from_grid = set(_kernels_of(os.path.join(csrc, "grid.h")))
    assert "record_write_kernel" in from_grid
    defined = {f: _kernels_of(os.path.join(csrc, f)) for f in units}
    every = [n for names in defined.values() for n in names]
    assert sorted(every) == sorted(want), "a kernel is defined twice, is missing, or a new one is not listed here"
    assert defined["pair_match.hip"] == [] and _kernels_of(os.path.join(csrc, "match_dev.h")) == []
    assert set(defined["ume_dist.hip"]) == {"ume_dist_kernel", "ume_dist_h_kernel", "match_finalize_kernel"}
    assert defined["match.hip"] == ["match_prob_kernel"]
    for f in units:
        launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", open(os.path.join(csrc, f)).read()))
        assert launched <= set(defined[f]) | from_grid, f"{f} launches a kernel of another unit: {sorted(launched - set(defined[f]) - from_grid)}"
        assert set(defined[f]) <= launched, f"{f} defines a kernel it never launches: {sorted(set(defined[f]) - launched)}"
    # (no unit of the library declares one of these kernels without defining it: the definitions above are all there is)
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")) and f not in units:
            assert not (set(_kernels_of(os.path.join(csrc, f))) & want), f


def test_grid_and_ball_kernels_are_launched_where_they_are_defined():
    """The a1 / a2 sources, once one file, are cut by subject: grid.hip builds the search structure, ball_search.h is the device-inline
    search, ball_query.hip and ume_moments.hip hold the two kernels that use it.  Each of the eight kernels is DEFINED in exactly
    one unit and LAUNCHED only from that unit; every other unit of the library goes through the launchers that grid.h and
    ball_search.h declare, and neither defines, declares nor launches one of these kernels."""
    csrc = os.path.join(REPO, "umeregrobust_amd", "csrc")
    want = {"grid.hip": {"pack_points_kernel", "grid_hist_kernel", "grid_scan_kernel", "grid_scatter_kernel", "kp_order_kernel",
                         "zero_words_kernel"},
            "ball_query.hip": {"ball_query_kernel"},
            "ume_moments.hip": {"ume_moments_kernel"}}
    every = set().union(*want.values())
    assert len(every) == 8
    assert not os.path.exists(os.path.join(csrc, "ball_moment.hip"))
    launches = lambda f: set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", open(os.path.join(csrc, f)).read()))
    for f, names in want.items():
        defined = _kernels_of(os.path.join(csrc, f))
        assert sorted(defined) == sorted(names), f"{f} defines {sorted(defined)}"
        assert launches(f) == names, f"{f} launches {sorted(launches(f))}"
    assert _kernels_of(os.path.join(csrc, "ball_search.h")) == [] and launches("ball_search.h") == set()
    assert _kernels_of(os.path.join(csrc, "grid.h")) == ["record_write_kernel"]
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")) and f not in want:
            assert not (set(_kernels_of(os.path.join(csrc, f))) & every), f"{f} defines or declares a kernel of another unit"
            assert not (launches(f) & every), f"{f} launches a kernel of another unit"
