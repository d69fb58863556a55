"""The distance backward's split plan and the inputs of tests/test_ume_grad_edges_gpu.py, without a GPU.

(i)   tests/ume_grad_cases.plan restates csrc/ume_grad_plan.h's bwd_plan; a host program (tests/ume_grad_plan_host.cpp, compiled here
      with the hipcc that builds the library) prints the header's own answer for every (rows, cols) in [1, 600]^2 and a list of large
      sizes, and the two must agree line by line.
(ii)  Every shape the GPU tests name for a feature of the plan has that feature.  A change of kRowTiles or of the split rule moves the
      features and fails here, instead of silently moving them away from the shapes that are tested.
(iii) Every ladder is what it claims: the diagonal distances sit on their rungs, the condition numbers on theirs, everything else is
      benign; the closed form for a given D is autograd's gradient; the row gate judges each row on its own scale.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ume_grad_cases as uc
import ume_grad_ref as uref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs():
    small = [(r, c) for r in range(1, 601) for c in range(1, 601)]
    side = [1, 15, 16, 17, 24, 529, 545, 560] + uc.PLAN_LARGE
    return small + [(r, c) for r in side for c in side]


@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc found: the header's bwd_plan cannot be compiled here")
    exe = str(tmp_path_factory.mktemp("ume_grad_plan") / "ume_grad_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "ume_grad_plan_host.cpp"), "-o", exe])
    pairs = _pairs()
    text = "".join(f"{r} {c}\n" for r, c in pairs)
    lines = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    head = lines[0].split()
    consts = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    rows = np.array([[int(v) for v in ln.split()] for ln in lines[1:] if ln], np.int64)
    return consts, pairs, rows


def test_plan_restates_the_header(header_plan):
    consts, pairs, rows = header_plan
    assert consts == dict(kRowTiles=uc.ROW_TILES, kRowKp=uc.ROW_KP)
    assert rows.shape == (len(pairs), 5) and len(pairs) > 360000
    mine = np.array([uc.plan(r, c) for r, c in pairs], np.int64)
    bad = np.nonzero((mine != rows).any(axis=1))[0]
    assert bad.size == 0, ([pairs[i] for i in bad[:5]], rows[bad[:5]], mine[bad[:5]])
    # what every plan must satisfy for the kernel to cover the columns once and stay inside its scratch
    n_rt, n_jt, tps, splits, n_work = rows.T
    assert (splits >= 1).all() and (splits <= 32).all() and (tps >= 1).all()
    assert ((splits - 1) * tps < n_jt).all() and (splits * tps >= n_jt).all() and (n_work == n_rt * splits).all()


def test_named_shapes_have_the_features_they_are_named_for():
    plan, last, cap = uc.plan, uc.last_split, uc.split_cap
    # where each feature first appears
    assert min(c for c in range(1, 601) if plan(40, c)[1] % plan(40, c)[2]) in range(529, 561)
    assert cap(2112) == 32 and cap(2113) == 31 and cap(65520) == 2 and cap(65521) == 1
    # today's GPU shapes reach none of them: every split is full, 32 is the cap, tiles per split stay small
    for n1, n2 in ((1, 1), (48, 48), (256, 256), (257, 130), (2048, 1536)):
        for r, c in ((n1, n2), (n2, n1)):
            assert cap(r) == 32 and last(r, c) == plan(r, c)[2] and plan(r, c)[2] <= 8
    # the pad: 15, 16, 17 on either side of 16, and a single row / column
    assert uc.PAD_SHAPES == [(15, 17), (16, 16), (17, 15), (1, 17), (17, 1)]
    assert [uc.pad_kp(n) for n in (1, 15, 16, 17)] == [16, 16, 16, 32]
    assert plan(15, 17) == (1, 4, 1, 4, 4) and plan(17, 15) == (2, 2, 1, 2, 4) and plan(1, 17) == (1, 4, 1, 4, 4) and plan(17, 1) == (2, 2, 1, 2, 4)
    # 40 x 545, side 1: n_jt = 70, 3 tiles per split, 24 splits, the last of 1 tile
    assert plan(40, 545) == (3, 70, 3, 24, 72) and last(40, 545) == 1
    # 40 x 529, side 1: n_jt = 68, the last split 2 of 3 tiles
    assert plan(40, 529)[1:4] == (68, 3, 23) and last(40, 529) == 2
    # 2120 x 560, side 1: 133 row tiles cap the splits at 31, the last split 1 tile; side 2: n_jt = 266, 9 per split, the last 5
    assert plan(2120, 560)[0] == 133 and cap(2120) == 31 and plan(2120, 560)[1:4] == (70, 3, 24) and last(2120, 560) == 1
    assert plan(560, 2120)[1:4] == (266, 9, 30) and last(560, 2120) == 5
    # 65 552 x 24, side 1: one split; side 2: 32 splits of 257 tiles, the last 227
    assert uc.TALL_SHAPE == (65552, 24)
    assert plan(65552, 24) == (4097, 4, 4, 1, 4097)
    assert plan(24, 65552) == (2, 8194, 257, 32, 64) and last(24, 65552) == 227
    assert set(uc.SPLIT_SHAPES) == {(40, 545), (40, 529), (2120, 560)}


@pytest.mark.parametrize("sin_t", uc.D_RUNGS)
def test_distance_rung_is_what_it_claims(sin_t):
    u1, u2, g_diag, g_dense = uc.distance_rung(sin_t)
    assert all(t.dtype == torch.float32 for t in (u1, u2, g_diag, g_dense)) and u1.shape == u2.shape == (1, 64, 32, 4)
    D = uref.ume_cdist(u1.double(), u2.double())[0]
    d = D.diagonal()
    off = D[~torch.eye(64, dtype=torch.bool)]
    print(f"[ume ladder] D rung {sin_t}: fp64 diagonal {float(d.min()):.6e} .. {float(d.max()):.6e}, off-diagonal min {float(off.min()):.3f}")
    if sin_t > 0:
        assert float(((d - sin_t).abs() / sin_t).max()) <= 1e-5
    else:
        assert float(d.max()) < 2e-6
    assert float(off.min()) >= 0.05
    assert bool((g_diag[0][~torch.eye(64, dtype=torch.bool)] == 0).all()) and float(g_diag[0].diagonal().min()) >= 1.0
    assert float(torch.linalg.cond(u2.double()).max()) <= 1e3         # (A_i = 3 I + randn: nothing here is ill-conditioned)


@pytest.mark.parametrize("c", uc.C_RUNGS)
def test_conditioning_rung_is_what_it_claims(c):
    u1, u2, gD = uc.cond_rung(c)
    cond = torch.linalg.cond(u1.double())
    D = uref.ume_cdist(u1.double(), u2.double())
    print(f"[ume ladder] cond rung {c:.0e}: cond {float(cond.min()):.3e} .. {float(cond.max()):.3e}, min D {float(D.min()):.3f}")
    assert u1.dtype == torch.float32 and float((cond / c - 1).abs().max()) <= 0.05
    assert float(D.min()) >= 0.05 and float(torch.linalg.cond(u2.double()).max()) <= 50


def test_mixed_case_is_what_it_claims():
    u1, u2, gD, ill = uc.mixed_case()
    cond = torch.linalg.cond(u1.double())[0]
    assert int(ill.sum()) == 4 and float((cond[ill] / 1e6 - 1).abs().max()) <= 0.05 and float(cond[~ill].max()) <= 50
    assert float(uref.ume_cdist(u1.double(), u2.double()).min()) >= 0.05
    # the case a per-tensor gate cannot judge: the fp32 helper's error on the ill-conditioned rows dwarfs every benign row's gradient error
    _, truth, yard = uc.truth_and_yard(u1, u2, gD)
    e = (yard[0].double() - truth[0]).abs().flatten(-2).max(dim=-1).values[0]
    assert float(e[ill].max()) > 100 * float(e[~ill].max())


def test_closed_form_is_autograd_s_gradient():
    u1, u2, gD = uc.dist_case(1, 48, 40, 77)
    D, truth, _ = uc.truth_and_yard(u1, u2, gD)
    a, b = uc.cdist_grads_closed(u1[0].double(), u2[0].double(), D[0], gD[0].double())
    for got, want in ((a, truth[0][0]), (b, truth[1][0])):
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-10
    # and with pairs left out
    drop = torch.rand(1, 48, 40, generator=uc.gen(5)) < 0.3
    _, ta, tb = uref.cdist_grads(u1.double(), u2.double(), gD.double(), drop)
    a, b = uc.cdist_grads_closed(u1[0].double(), u2[0].double(), D[0], gD[0].double(), ~drop[0])
    assert float((a - ta[0]).abs().max()) <= 1e-10 and float((b - tb[0]).abs().max()) <= 1e-10


def test_cut_case_is_what_it_claims():
    lo, c, hi = uc.cut_values()
    assert lo < c < hi and c == np.float32(4e-3) and np.nextafter(lo, np.float32(1)) == c and np.nextafter(hi, np.float32(0)) == c
    u1, u2, D, gD, keep, put = uc.cut_case()
    assert D.dtype == torch.float32 and tuple(D.shape) == uc.CUT_SHAPE == (48, 40)
    assert uc.pad_kp(48) == 48 and uc.pad_kp(40) == 48                  # j = 39 is the last real column, 8 padded ones behind it
    vals = {(i, j): np.float32(D[i, j]) for (i, j) in put}
    assert set(vals.values()) == {lo, c, hi}
    assert all(bool(keep[i, j]) == (v == hi) for (i, j), v in vals.items())
    assert int((~keep).sum()) == sum(v != hi for v in vals.values()) and int(keep.sum()) > 1700      # nothing else is near the cut
    assert float(D[keep].min()) == float(hi)
    assert not bool(keep[20].any()) and not bool(keep[:, 17].any())
    # one thread of cdist_bwd_kernel: rows 3 and 11 (i_local = c >> 2 of tiles t = 0, 1), columns 2 q + 1
    for i in (3, 11):
        assert {np.float32(D[i, j]) for j in (1, 3, 5, 7)} == {lo, c, hi}
    assert (47, 39) in put and np.float32(D[47, 39]) == c


def test_row_gate_judges_each_row_on_its_own_scale():
    truth = torch.ones(1, 4, 32, 4, dtype=torch.float64) * torch.tensor([1.0, 1e-3, 1.0, 1e3]).view(1, 4, 1, 1)
    yard = truth * (1 + 1e-6)
    assert torch.allclose(uc.row_rel(yard, truth), torch.full((1, 4), 1e-6, dtype=torch.float64), rtol=1e-6)
    ok = truth * (1 + 3e-6)
    assert abs(uc.row_gate(ok, truth, yard, "self-test", log=lambda s: None) - 3.0) < 1e-3
    bad = truth.clone()
    bad[0, 1] *= 1 + 1e-5                       # a small row off by 1e-8 absolute: invisible per tensor, 10 x the yardstick per row
    assert float((bad - truth).abs().max()) < float((yard - truth).abs().max())
    with pytest.raises(AssertionError):
        uc.row_gate(bad, truth, yard, "self-test", log=lambda s: None)
    groups = {"a": torch.tensor([True, True, False, False]), "b": torch.tensor([False, False, True, True])}
    yard2 = truth.clone()
    yard2[0, :2] *= 1 + 1e-6
    yard2[0, 2:] *= 1 + 1e-3
    mid = truth * (1 + 1e-4)                    # fine for group b, 100 x group a's yardstick
    uc.row_gate(mid, truth, yard2, "self-test", log=lambda s: None)
    with pytest.raises(AssertionError):
        uc.row_gate(mid, truth, yard2, "self-test", groups=groups, log=lambda s: None)
    with pytest.raises(AssertionError):
        uc.row_gate(ok, truth, yard, "self-test", bar=2e-6, log=lambda s: None)
    z = torch.zeros(1, 2, 32, 4)
    assert torch.equal(uc.row_rel(z, z), torch.zeros(1, 2, dtype=torch.float64)) and bool(torch.isinf(uc.row_rel(z + 1, z)).all())
