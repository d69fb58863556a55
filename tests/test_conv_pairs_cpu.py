"""CPU: the pair-compacted convolution engine (include/umereg_sparse_conv_pairs.h, csrc/sparse_conv_pairs.hip) without a GPU --
the `conv_mode` keyword, the compaction plan's restatement (tests/conv_pairs_ref.py) against csrc/conv_pairs_plan.h, the issue
count of the plan against the union walk's on all 13 tables of the 6 000-point cloud, and the host side of the new header."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import abi_headers
import conv_pairs_ref as cpr
import featnet_ref as ref
import test_featnet_gpu as fg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the keyword -------------------------------------------------------------------------------------------------------------------

def test_conv_mode_keyword(capsys):
    import torch
    from umeregrobust_amd import evaluate, models, sparse_conv, train_coloring
    assert models.CONV_MODES == ("union", "pairs")
    assert models.ResUNetSmall2().conv_mode == "union" and models.ResUNetSmall2(conv_mode="pairs").conv_mode == "pairs"
    with pytest.raises(ValueError, match="conv_mode.*'x'"):
        models.ResUNetSmall2(conv_mode="x")
    # the mode combines with every other switch, and adds neither parameters nor buffers
    m = models.ResUNetSmall2(conv_mode="pairs", trainable=True, train_precision="f16", fused_norm=True, precision="f16")
    assert list(m.state_dict()) == list(models.ResUNetSmall2().state_dict())
    with pytest.raises(ValueError, match="conv_mode"):
        models.forward_raw(None, None, 1, None, None, None, None, conv_mode="rows")
    with pytest.raises(ValueError, match="conv_mode"):
        sparse_conv.conv_raw(torch.zeros(2, 32), torch.zeros(27, 32, 32), None, 0, conv_mode="rows")
    with pytest.raises(ValueError, match="conv_mode"):
        sparse_conv.sparse_conv(torch.zeros(2, 32), torch.zeros(27, 32, 32), None, 0, conv_mode="rows")
    for fn in (models.forward_raw, sparse_conv.conv_raw, sparse_conv.sparse_conv, evaluate.cached_pairs, train_coloring.run):
        assert inspect.signature(fn).parameters["conv_mode"].default == "union", fn
    # the pairs engine has no CPU fallback either
    from umeregrobust_amd.sparse import SparseTensor
    st = SparseTensor(torch.ones(2, 1), coordinates=torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        models.ResUNetSmall2(conv_mode="pairs").eval()(st)
    for main in (evaluate.main, train_coloring.main):
        with pytest.raises(SystemExit):
            main(["--conv-mode", "rows"])
        err = capsys.readouterr().err
        assert "--conv-mode" in err and "'union', 'pairs'" in err


# ---- the plan ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: csrc/conv_pairs_plan.h cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("conv_pairs_plan") / "conv_pairs_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "conv_pairs_plan_host.cpp"), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, check=True, text=True).stdout.split("\n")
    head = lines[0].split()
    consts = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    cols = {int(ln.split()[1]): int(ln.split()[2]) for ln in lines[1:] if ln.startswith("c ")}
    blocks = {int(ln.split()[1]): int(ln.split()[2]) for ln in lines[1:] if ln.startswith("p ")}
    return consts, cols, blocks


def test_restatement_mirrors_the_header(header_plan):
    consts, cols, blocks = header_plan
    assert consts == dict(kCpTM=cpr.TM, kCpSlots=cpr.SLOTS, kCpThreads=cpr.THREADS)
    assert cols == {c: cpr.tile_cols(c) for c in range(32, 257, 32)}
    assert blocks == {p: int(cpr.blocks(p)) for p in range(cpr.TM + 1)}
    # the tile height is a multiple of both of the union engine's: the premise of "never more issue than the union walk"
    assert all(cpr.TM % th == 0 for th in cpr.UNION_TILES.values())
    assert blocks[0] == 0 and blocks[1] == blocks[32] == 1 and blocks[33] == 2 and blocks[cpr.TM] == cpr.TM // 32


def test_plan_lists_the_active_rows_in_ascending_order():
    rng = np.random.default_rng(0)
    mask = rng.integers(0, 1 << 27, 300, dtype=np.int64).astype(np.uint32)
    mask[rng.random(300) < 0.3] = 0
    mask[128:256] |= np.uint32(1 << 13)                # a full tile at one offset
    P = cpr.active_counts(mask)
    pl = cpr.plan(mask)
    assert P.shape == (3, 27) and len(pl) == 3 and P[1, 13] == cpr.TM
    for t, tile in enumerate(pl):
        for k, blks in enumerate(tile):
            rows = np.concatenate(blks) if blks else np.zeros(0, np.int64)
            want = np.nonzero((mask[t * cpr.TM:(t + 1) * cpr.TM] >> np.uint32(k)) & np.uint32(1))[0]
            assert np.array_equal(rows, want) and len(rows) == P[t, k]
            assert len(blks) == cpr.blocks(P[t, k]) and all(len(b) == cpr.SLOTS for b in blks[:-1])
    assert cpr.pairs_blocks(mask) == sum(len(b) for tile in pl for b in tile)
    # by hand: rows 0..63 use offset 3, row 64 uses offset 3 and 5
    m = np.zeros(200, np.uint32)
    m[:65] = 8
    m[64] |= 32
    assert cpr.pairs_blocks(m) == 3 + 1 and cpr.union_blocks(m, 64) == 2 + 2 + 2 and cpr.union_blocks(m, 128) == 4 + 4
    assert cpr.useful_blocks(m) == 66 / 32


def _orders(coords):
    """the reference's own row order and a cell-sorted one (rows by 8^3 cell, as the library orders level 0)"""
    cell = ref.keys(ref.coarsen(coords, 8))
    return {"input": coords, "cells": coords[np.argsort(cell, kind="stable")]}


def test_plan_never_issues_more_blocks_than_the_union_walk():
    """All 13 tables of the 6 000-point cloud, in two row orders: sum_k ceil(P_k / 32) over tiles of 128 rows against the union walk
    with tiles of 64 and of 128 rows -- the inequality of csrc/conv_pairs_plan.h checked, not assumed."""
    coords = fg.voxel_cloud(0, "KT")[:6000]
    for name, c in _orders(coords).items():
        masks = ref.neighbour_masks(ref.levels(c))
        assert len(masks) == 13
        tot = {"pairs": 0, 64: 0, 128: 0, "useful": 0.0}
        for t, m in enumerate(masks):
            p = cpr.pairs_blocks(m)
            for th in (64, 128):
                u = cpr.union_blocks(m, th)
                assert p <= u, (name, t, th, p, u)
                tot[th] += u
            assert p >= cpr.useful_blocks(m)
            tot["pairs"] += p
            tot["useful"] += cpr.useful_blocks(m)
        print(f"[conv pairs plan, {name} order] blocks over 13 tables: pairs {tot['pairs']} union64 {tot[64]} union128 {tot[128]} "
              f"useful {tot['useful']:.0f}")
        assert tot["pairs"] < tot[64]                  # and on a real cloud it issues strictly fewer


# ---- the host side of include/umereg_sparse_conv_pairs.h ---------------------------------------------------------------------------

def test_pairs_table_mirrors_its_header():
    """(keys, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import models, sparse_conv
    header = "umereg_sparse_conv_pairs.h"
    raw = open(os.path.join(abi_headers.INCLUDE, header)).read()
    syms = ["umereg_featnet_forward_pairs", "umereg_sparse_conv_pairs"]
    assert sorted(sparse_conv.SPARSE_CONV_PAIRS_SIGNATURES) == syms
    c_int = ctypes.c_int
    for name in syms:
        assert abi_headers.params(header, name).split(",")[-1].strip() == "int f16"
    # the arguments of the union engine's entries, one to one, then `int f16`
    assert sparse_conv.SPARSE_CONV_PAIRS_SIGNATURES["umereg_featnet_forward_pairs"] == \
        (c_int, models.FEATNET_SIGNATURES["umereg_featnet_forward_f32"][1] + [c_int])
    assert sparse_conv.SPARSE_CONV_PAIRS_SIGNATURES["umereg_sparse_conv_pairs"] == \
        (c_int, sparse_conv.SPARSE_CONV_SIGNATURES["umereg_sparse_conv_f32"][1] + [c_int])
    # the older headers stay what they were
    for h in ("umereg.h", "umereg_featnet.h", "umereg_featnet_f16.h", "umereg_sparse_conv.h", "umereg_sparse_conv_f16.h"):
        assert "_pairs" not in open(os.path.join(REPO, "include", h)).read(), h
    # the header states the two allowed differences
    assert "sign of a zero" in raw and "non-finite WEIGHTS" in raw


def test_pairs_entry_points_check_arguments_and_need_a_device():
    from umeregrobust_amd import sparse_conv
    lib = sparse_conv.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    ws_bytes = lib.umereg_featnet_workspace_bytes(4, 1)
    for f16 in (0, 1):
        fwd = lambda *a: lib.umereg_featnet_forward_pairs(*a, f16)        # noqa: E731
        # argument errors come before the device probe; the codes are the union entries'
        assert fwd(None, p, 4, 1, p, p, p, p, ws_bytes, None) == -1
        assert fwd(p, None, 4, 1, p, p, p, p, ws_bytes, None) == -1 and b"null" in lib.umereg_last_error()
        assert fwd(p, p, 0, 1, p, p, p, p, ws_bytes, None) == -1
        assert fwd(p, p, 4, 0, p, p, p, p, ws_bytes, None) == -1
        assert fwd(p, p, 4, 128, p, p, p, p, ws_bytes, None) == -1
        assert fwd(p, p, 4, 1, p + 4, p, p, p, ws_bytes, None) == -1
        names = (("ws", p), ("ws_bytes", ws_bytes), ("status", p), ("n", 4), ("table", 0), ("x", p), ("ld_in", 32), ("W", p), ("cin", 32),
                 ("cout", 32), ("scale", p), ("shift", p), ("out", p), ("ld_out", 32), ("accumulate", 0), ("stream", None))

        def both(**kw):
            args = [kw.get(k, d) for k, d in names]
            union = (lib.umereg_sparse_conv_f16 if f16 else lib.umereg_sparse_conv_f32)(*args)
            assert lib.umereg_sparse_conv_pairs(*args, f16) == union, kw
            return union

        for k in ("ws", "status", "x", "W", "scale", "shift", "out"):
            assert both(**{k: None}) == -1, k
            assert b"null" in lib.umereg_last_error()
        for kw in (dict(n=0), dict(table=13), dict(table=-2), dict(cin=48), dict(cout=16), dict(cout=288), dict(ld_in=16), dict(ld_in=34),
                   dict(ld_out=8), dict(x=p + 4)):
            assert both(**kw) == -1, kw
        if not f16:
            assert both(table=-1, cin=96, ld_in=96, cout=64, ld_out=64) == -1                # the 1x1 layer is the f16 entry's
        if lib.umereg_device_count(None, 0) == 0:
            assert fwd(p, p, 4, 1, p, p, p, p, ws_bytes, None) == -2                      # UMEREG_ENODEV
            assert b"no CPU fallback" in lib.umereg_last_error()
            assert both() == -2
            if f16:
                assert both(table=-1, cin=96, ld_in=96, cout=64, ld_out=64) == -2
            assert b"no CPU fallback" in lib.umereg_last_error()
