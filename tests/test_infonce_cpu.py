"""CPU: the fused InfoNCE loss without a GPU -- the header's place in the one ABI (tests/test_abi.py checks include/umereg_infonce.h against
its table), the entries' refusals without a device, the Python refusals, and the tile plan (csrc/infonce_plan.h through
tests/infonce_plan_host.cpp) against the Python restatement the GPU tests place their edges with (tests/infonce_cases.py)."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import abi_headers
import infonce_cases as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_HEADER = os.path.join(abi_headers.INCLUDE, "umereg_infonce.h")


@pytest.fixture(scope="module")
def lib():
    from umeregrobust_amd import infonce
    return infonce.load_native()


# ---- 1. the header's place ------------------------------------------------------------------------------------------------------------

def test_the_header_is_one_of_include_s_and_its_table_is_the_package_s(lib):
    from umeregrobust_amd import _build, _lib, infonce
    assert infonce.INFONCE_SIGNATURES is _lib.TABLES["umereg_infonce.h"] and infonce.load_native is _lib.load
    assert len(os.listdir(abi_headers.INCLUDE)) == len(abi_headers.HEADERS) == len(_lib.TABLES)      # the number: tests/test_abi.py
    assert API_HEADER in _build.headers()                    # part of the build hash


# ---- 2. without a device ---------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_before_the_device_probe(lib):
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) // 256 * 256
    B, N, M, S = 2, 40, 30, 20
    need = lib.umereg_infonce_workspace_bytes(B, N, M, S)
    assert 0 < need == ic.workspace_bytes(B, N, M, S) < (1 << 15)

    def fwd(src=p, pts=p, tgt=p, m=p, B=B, N=N, M=M, S=S, tau=0.1, r=5.0, stats=p, loss=p, ws=p, nws=need):
        return lib.umereg_infonce_fwd_f32(src, pts, tgt, m, B, N, M, S, tau, r, stats, loss, ws, nws, None)

    def bwd(src=p, pts=p, tgt=p, m=p, B=B, N=N, M=M, S=S, tau=0.1, r=5.0, stats=p, g=p, dsrc=p, dtgt=p, ws=p, nws=need):
        return lib.umereg_infonce_bwd_f32(src, pts, tgt, m, B, N, M, S, tau, r, stats, g, dsrc, dtgt, ws, nws, None)

    for k in ("src", "pts", "tgt", "m", "stats", "loss"):
        assert fwd(**{k: None}) == -1, k
        assert b"null pointer" in lib.umereg_last_error()
    for k in ("src", "pts", "tgt", "m", "stats", "g"):
        assert bwd(**{k: None}) == -1, k
    assert bwd(dsrc=None, dtgt=None) == -1 and b"nothing to compute" in lib.umereg_last_error()
    for kw in (dict(S=0), dict(S=ic.MAX_S + 1), dict(B=0), dict(N=0), dict(M=0), dict(tau=0.0), dict(tau=-1.0), dict(r=-1.0),
               dict(src=p + 4), dict(tgt=p + 8)):
        assert fwd(**kw) == -1 and bwd(**kw) == -1, kw
    assert bwd(dsrc=p + 4) == -1
    assert fwd(ws=None) == -3 and fwd(nws=need - 1) == -3 and bwd(nws=need - 1) == -3         # UMEREG_EWORKSPACE
    if lib.umereg_device_count(None, 0) == 0:
        assert fwd() == -2 and b"no CPU fallback" in lib.umereg_last_error()                  # UMEREG_ENODEV
        assert bwd() == -2 and b"no CPU fallback" in lib.umereg_last_error()
        assert bwd(dsrc=None) == -2 and bwd(dtgt=None) == -2


def test_the_size_query_is_zero_for_what_the_entries_refuse(lib):
    q = lib.umereg_infonce_workspace_bytes
    assert q(8, 45000, 45000, ic.MAX_S) == ic.workspace_bytes(8, 45000, 45000, ic.MAX_S) > 0
    assert q(1, 1, 1, 1) == ic.workspace_bytes(1, 1, 1, 1) > 0
    for args in ((1, 10, 10, ic.MAX_S + 1), (0, 10, 10, 5), (1, 0, 10, 5), (1, 10, 0, 5), (1, 10, 10, 0), (-1, 10, 10, 5), (1, 10, 10, -3)):
        assert q(*args) == 0 == ic.workspace_bytes(*args), args
    assert ic.MAX_S >= 8192


# ---- 3. Python refusals ---------------------------------------------------------------------------------------------------------------

def test_python_refuses_cpu_tensors_and_other_widths():
    from umeregrobust_amd import infonce, pw_loss
    inp = ic.make_inputs(0, 1, 20, 20, 5, "far")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infonce.infonce_loss(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], inp["matches"], 0.1, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pw_loss.MyInfoNCELossNoSeg()(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], inp["matches"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infonce.infonce_fwd_raw(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], inp["matches"], 0.1, 5)
    # shapes and types are judged before the device, so a wrong width is a ValueError here too
    f16 = torch.zeros(1, 20, 16)
    with pytest.raises(ValueError, match="32"):
        infonce.infonce_loss(f16, inp["src_pts"], f16, inp["matches"], 0.1, 5)
    with pytest.raises(ValueError, match="float32"):
        infonce.infonce_loss(inp["src_feat"].double(), inp["src_pts"], inp["tgt_feat"], inp["matches"], 0.1, 5)
    with pytest.raises(ValueError, match="int64"):
        infonce.infonce_loss(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], inp["matches"].int(), 0.1, 5)
    with pytest.raises(ValueError, match="expected"):
        infonce.infonce_loss(inp["src_feat"], inp["src_pts"][:, :10], inp["tgt_feat"], inp["matches"], 0.1, 5)
    with pytest.raises(ValueError, match="expected"):
        infonce.infonce_loss(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], inp["matches"][..., :1], 0.1, 5)
    with pytest.raises(ValueError, match="at most"):
        infonce.infonce_loss(inp["src_feat"], inp["src_pts"], inp["tgt_feat"], torch.zeros(1, ic.MAX_S + 1, 2, dtype=torch.int64), 0.1, 5)


def test_the_fused_class_has_the_reference_s_signature():
    from umeregrobust_amd import loss, pw_loss
    sig = inspect.signature(pw_loss.MyInfoNCELossNoSeg.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [("num_samples", 2048), ("tau", 0.1), ("match_r", 0.1),
                                                                            ("neg_euclid_dist", 5)]
    assert list(inspect.signature(pw_loss.MyInfoNCELossNoSeg.forward).parameters)[1:] == ["velo_feat", "velo_pts", "ref_feat", "matches"]
    assert sig == inspect.signature(loss.MyInfoNCELossNoSeg.__init__)
    fn = pw_loss.MyInfoNCELossNoSeg(num_samples=512, tau=0.2, neg_euclid_dist=3)
    assert (fn.num_samples, fn.tau, fn.match_r, fn.neg_euclid_dist) == (512, 0.2, 0.1, 3)
    from umeregrobust_amd import train_coloring as tc
    assert inspect.signature(tc.run).parameters["fused_pointwise"].default is False


# ---- 4. the plan header ---------------------------------------------------------------------------------------------------------------

PLAN_SIZES = [(1, 1, 1, 1), (3, 300, 260, 33), (8, 45000, 45000, 512), (8, 45000, 45000, 2048), (2, 45000, 45000, 8192), (1, 5, 5, 8193),
              (0, 5, 5, 5), (1, 0, 5, 5), (1, 5, 0, 5), (1, 5, 5, 0), (7, 9, 9, 127), (7, 9, 9, 128), (7, 9, 9, 129)]


@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's plan cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("infonce_plan") / "infonce_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "infonce_plan_host.cpp"), "-o", exe])
    text = "".join("{} {} {} {}\n".format(*s) for s in PLAN_SIZES)
    lines = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    head = lines[0].split()
    return {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}, [ln for ln in lines[1:] if ln]


def test_the_plan_header_equals_its_python_restatement(header_plan, lib):
    consts, rows = header_plan
    assert consts == {"kInfoNceD": ic.D, "kInfoNceWaves": ic.WAVES, "kInfoNceThreads": ic.THREADS, "kInfoNceRows": ic.ROWS,
                      "kInfoNceCols": ic.COLS, "kInfoNceLdsStride": ic.LDS_STRIDE, "kInfoNceMaxS": ic.MAX_S,
                      "kInfoNceScatterRows": ic.SCATTER_ROWS, "kInfoNceLdsBytes": ic.LDS_BYTES,
                      "kInfoNceScatterLdsBytes": ic.SCATTER_LDS_BYTES, "kInfoNceLdsPerCu": ic.LDS_PER_CU}
    assert len(rows) == len(PLAN_SIZES)
    for (B, N, M, S), row in zip(PLAN_SIZES, rows):
        want = ic.workspace_bytes(B, N, M, S)
        got = [int(v) for v in row.split()]
        assert lib.umereg_infonce_workspace_bytes(B, N, M, S) == want
        if not want:
            assert got == [0], (B, N, M, S)
            continue
        ok, row_blocks, col_steps, part, da, dp, nm, total = got
        assert ok == 1 and row_blocks == -(-S // ic.ROWS) and col_steps == -(-S // ic.COLS)
        assert total == want and part == 0 and da % 256 == 0 and dp % 256 == 0
        assert da >= B * row_blocks * 8 and dp - da >= B * S * 128 and nm - dp >= B * S * 128 and total - nm >= B * S * 4 and nm % 256 == 0


def test_two_workgroups_per_cu_fit_in_lds():
    assert ic.LDS_PER_CU == 160 * 1024
    assert 2 * ic.LDS_BYTES <= ic.LDS_PER_CU and 2 * ic.SCATTER_LDS_BYTES <= ic.LDS_PER_CU
    assert ic.COLS % 32 == 0 and ic.COLS // 32 == ic.WAVES and ic.ROWS == 32
    assert (ic.WAVES * 32 * 32 + 2 * ic.ROWS + 2 * ic.WAVES * 32) * 4 <= ic.COLS * ic.LDS_STRIDE * 4      # combine, coefficients, row sums: in the feature area
    assert len(set(ic.EDGE_S)) == 10
