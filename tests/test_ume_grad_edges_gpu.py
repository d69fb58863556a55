"""GPU: the backward of the subspace distance where training drives it and where its plan changes -- near pairs down to 2 x D_MIN
and below it, the strict cut at D_MIN itself, condition numbers up to 1e7, one ill-conditioned group among benign rows, the
16-keypoint pad and every feature of the split plan -- and the moments' backward on both sides of its 64-wide chunks.

Inputs, truths and gates: tests/ume_grad_cases.py (checked on the CPU by tests/test_ume_grad_plan_cpu.py).  Truth: the fp64
restatement tests/ume_grad_ref.py through autograd.  Gate, per ROW: every 32 x 4 gradient's relative error |x_i - truth_i|_F /
|truth_i|_F <= 4 x the largest such error of the SAME helper in fp32 on the CPU over the same rows; never the GPU's own output.
Every test prints what it saw (`pytest -s`; the record is profiles/ume_grad/ladders.txt)."""
import functools

import numpy as np
import pytest
import torch

import ume_grad_cases as uc
import ume_grad_ref as uref

pytestmark = pytest.mark.gpu


def autograd_grads(gpu, u1, u2, gD):
    """(forward's D, dume1, dume2) through ume_grad.ume_cdist: what training gets"""
    from umeregrobust_amd import ume_grad
    a, b = u1.to(gpu).requires_grad_(), u2.to(gpu).requires_grad_()
    D = ume_grad.ume_cdist(a, b)
    (D * gD.to(gpu)).sum().backward()
    return D.detach().cpu(), a.grad, b.grad


def raw_grads(gpu, u1, u2, D, gD):
    """(dume1, dume2) of cdist_bwd_raw on a given f32 D: the backward's own arithmetic"""
    from umeregrobust_amd import ume_grad
    return ume_grad.cdist_bwd_raw(u1.to(gpu), u2.to(gpu), D.to(gpu), gD.to(gpu))


def test_the_cut_is_the_header_s(gpu):
    from umeregrobust_amd import ume_grad
    assert np.float32(ume_grad.D_MIN) == uc.D_MIN_F32 and min(uc.D_RUNGS_ABOVE) >= 2 * ume_grad.D_MIN > max(uc.D_RUNGS_BELOW)


# ---- 1: near pairs ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rung_truth(sin_t, dense, dropped):
    u1, u2, g_diag, g_dense = uc.distance_rung(sin_t)
    gD = g_dense if dense else g_diag
    return uc.truth_and_yard(u1, u2, gD, uc.diag_mask(64, 64) if dropped else None)


@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
@pytest.mark.parametrize("sin_t", uc.D_RUNGS_ABOVE)
def test_near_pairs_carry_their_gradient(gpu, sin_t, dense):
    """diagonal pairs at D = sin t >= 2 x D_MIN: w = dD / (2 D) up to 62, (I - Q Q^T) M cancelling by 1 / D.  (a) with the forward's
    own f32 D, (b) with the truth's D rounded to f32."""
    from umeregrobust_amd import ume_grad
    u1, u2, g_diag, g_dense = uc.distance_rung(sin_t)
    gD = g_dense if dense else g_diag
    D, truth, yard = rung_truth(sin_t, dense, False)
    Dg, a, b = autograd_grads(gpu, u1, u2, gD)
    dg = Dg[0].diagonal().double()
    print(f"[ume ladder] D = {sin_t} {'dense' if dense else 'diag'}: the forward's diagonal D {float(dg.min()):.6e} .. {float(dg.max()):.6e}, "
          f"max |D gpu - fp64| / D {float(((dg - D[0].diagonal()).abs() / D[0].diagonal()).max()):.2e}")
    assert float(dg.min()) > ume_grad.D_MIN
    name = f"D = {sin_t} {'dense' if dense else 'diag'}"
    uc.row_gate(a, truth[0], yard[0], f"{name} (a) forward's D, dume1")
    uc.row_gate(b, truth[1], yard[1], f"{name} (a) forward's D, dume2")
    a, b = raw_grads(gpu, u1, u2, D.float(), gD)
    uc.row_gate(a, truth[0], yard[0], f"{name} (b) truth's D, dume1")
    uc.row_gate(b, truth[1], yard[1], f"{name} (b) truth's D, dume2")


@pytest.mark.parametrize("sin_t", uc.D_RUNGS_BELOW)
def test_pairs_below_the_cut_carry_none(gpu, sin_t):
    """diagonal pairs at D = 0.002 and on the same subspace: the forward's D is at or below D_MIN, so an upstream gradient on the
    diagonal alone gives exactly 0 everywhere, and a dense one the truth with the diagonal pairs left out"""
    from umeregrobust_amd import ume_grad
    u1, u2, g_diag, g_dense = uc.distance_rung(sin_t)
    Dg, a, b = autograd_grads(gpu, u1, u2, g_diag)
    dg = Dg[0].diagonal()
    print(f"[ume ladder] D = {sin_t}: the forward's diagonal D {float(dg.min()):.6e} .. {float(dg.max()):.6e} (D_MIN {ume_grad.D_MIN})")
    assert float(dg.max()) <= ume_grad.D_MIN
    assert bool((a == 0).all()) and bool((b == 0).all())
    D, truth, yard = rung_truth(sin_t, True, True)
    _, a, b = autograd_grads(gpu, u1, u2, g_dense)
    uc.row_gate(a, truth[0], yard[0], f"D = {sin_t} dense, diagonal dropped, dume1")
    uc.row_gate(b, truth[1], yard[1], f"D = {sin_t} dense, diagonal dropped, dume2")


def test_the_cut_is_strict(gpu):
    """D_MIN itself, its f32 predecessor and its successor fed to cdist_bwd_raw: exactly the entries <= D_MIN are dropped, the
    others weigh dD / (2 D) with the D that was given (125 dD for the successor: a row that holds one is that term and little else).
    Truth: the closed form in fp64; yardstick: the closed form in fp32."""
    u1, u2, D, gD, keep, put = uc.cut_case()
    truth = uc.cdist_grads_closed(u1.double(), u2.double(), D.double(), gD.double(), keep)
    yard = uc.cdist_grads_closed(u1, u2, D, gD, keep)
    a, b = raw_grads(gpu, u1[None], u2[None], D[None], gD[None])
    a, b = a[0].cpu(), b[0].cpu()
    assert bool((truth[0][20] == 0).all()) and bool((truth[1][17] == 0).all())
    assert bool((a[20] == 0).all()) and bool((b[17] == 0).all()), "a row whose every pair is at or below D_MIN has a gradient"
    rows1 = torch.ones(48, dtype=torch.bool)
    rows1[20] = False
    rows2 = torch.ones(40, dtype=torch.bool)
    rows2[17] = False
    touched1 = torch.zeros(48, dtype=torch.bool)
    touched1[sorted({i for (i, j) in put if j != 17})] = True
    touched2 = torch.zeros(40, dtype=torch.bool)
    touched2[sorted({j for (i, j) in put if i != 20})] = True
    uc.row_gate(a[None], truth[0][None], yard[0][None], "strict cut dume1", groups={"rows of the directed entries": touched1 & rows1, "other rows": ~touched1 & rows1})
    uc.row_gate(b[None], truth[1][None], yard[1][None], "strict cut dume2", groups={"rows of the directed entries": touched2 & rows2, "other rows": ~touched2 & rows2})


# ---- 2: conditioning ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", uc.C_RUNGS)
def test_conditioning_rungs(gpu, c):
    """cond(ume1) = c up to 1e7: the row gate, and the sharper bar -- the kernel forms Q and R in fp64 from the f32 input, so its
    row-relative error must stay at 4 x the fp32 helper's at c = 1e1 on EVERY rung"""
    u1, u2, gD = uc.cond_rung(c)
    _, truth, yard = uc.truth_and_yard(u1, u2, gD)
    _, a, b = autograd_grads(gpu, u1, u2, gD)
    bar = uc.sharp_bar()
    uc.row_gate(a, truth[0], yard[0], f"cond = {c:.0e} dume1", bar=bar[0])
    uc.row_gate(b, truth[1], yard[1], f"cond = {c:.0e} dume2", bar=bar[1])


def test_ill_conditioned_rows_among_benign_ones(gpu):
    """4 rows at c = 1e6 among 60 benign ones in one tensor: each group against its own rows of the fp32 helper, and the sharp bar"""
    u1, u2, gD, ill = uc.mixed_case()
    _, truth, yard = uc.truth_and_yard(u1, u2, gD)
    _, a, b = autograd_grads(gpu, u1, u2, gD)
    bar = uc.sharp_bar()
    uc.row_gate(a, truth[0], yard[0], "mixed dume1", groups={"benign": ~ill, "c = 1e6": ill}, bar=bar[0])
    uc.row_gate(b, truth[1], yard[1], "mixed dume2", bar=bar[1])


# ---- 3: the plan's edges -----------------------------------------------------------------------------------------------------------

def plan_edge(gpu, n1, n2, u1, u2, gD, D, truth, yard):
    """The plan is the backward's alone, so the gate is on the backward's own arithmetic: cdist_bwd_raw on the truth's D rounded to
    f32, as route (b) of the ladder.  The route through the forward's own D is printed beside it and not gated here: the forward's
    `4 - s` noise in D (5e-6 relative at D = 0.3, 5e-5 at 0.1, gated rung by rung above against a helper whose fp32 cdist carries the
    same cancellation) is not a property of any plan, and below 26 rows torch's fp32 cdist takes direct differences and carries
    none, so there the yardstick would judge the forward and not the tiling."""
    assert float(D.min()) >= 0.05
    print(f"[ume ladder] {n1} x {n2}: plans {uc.plan(n1, n2)} / {uc.plan(n2, n1)}")
    a, b = raw_grads(gpu, u1, u2, D.float(), gD)
    _, fa, fb = autograd_grads(gpu, u1, u2, gD)
    for k, got, fwd in ((0, a, fa), (1, b, fb)):
        g_med, g_max, _, c_max = uc.row_stats(fwd, truth[k], yard[k])["rows"]
        print(f"[ume ladder] {n1} x {n2} dume{k + 1} with the forward's D (not gated): gpu row-rel median {g_med:.2e} max {g_max:.2e} | "
              f"ratio {g_max / c_max:.3f}")
        assert torch.isfinite(fwd).all()
        uc.row_gate(got, truth[k], yard[k], f"{n1} x {n2} dume{k + 1}")


@pytest.mark.parametrize("n1,n2", uc.PAD_SHAPES + uc.SPLIT_SHAPES)
def test_plan_edges(gpu, n1, n2):
    """the 16-keypoint pad on either side, short last splits, the split cap below 32 (the features: test_ume_grad_plan_cpu.py)"""
    u1, u2, gD = uc.dist_case(1, n1, n2, 9000 + 7 * n1 + n2)
    plan_edge(gpu, n1, n2, u1, u2, gD, *uc.truth_and_yard(u1, u2, gD))


def test_plan_edges_tall(gpu):
    """65 552 x 24: one split on side 1; 32 splits of 257 tiles, the last of 227, on side 2"""
    n1, n2 = uc.TALL_SHAPE
    u1, u2, gD = uc.dist_case(1, n1, n2, 9999)
    plan_edge(gpu, n1, n2, u1, u2, gD, *uc.truth_and_yard_tall(u1, u2, gD))


# ---- 4: the moments' backward at its chunk edges ----------------------------------------------------------------------------

@pytest.mark.parametrize("N,n,K", [(8000, 1, 32), (8000, 63, 32), (8000, 64, 32), (8000, 65, 32), (8000, 129, 32),
                                   (8000, 40, 1), (8000, 40, 63), (8000, 40, 64), (8000, 40, 65), (7999, 40, 32)])
def test_moments_backward_is_exact_at_chunk_edges(gpu, N, n, K):
    """test_moments_backward_is_exact_on_integers (tests/test_ume_grad_gpu.py) with n on either side of the 64 keypoints
    mom_scatter_kernel tests at a time, K on either side of the 64 entries mom_gr_kernel strides by, and B N no multiple of the four
    waves of a workgroup.  Same lattice, same integers, same 2^24 precondition; the radius grows with K so that lists reach K."""
    from umeregrobust_amd import ops, ume_grad
    g = uc.gen(300 + 1000 * n + K + N)
    B = 2
    r = 2.5 if K <= 32 else 3.5
    pts = torch.randint(-12, 13, (B, N, 3), generator=g).float()
    feat = torch.randint(-3, 4, (B, N, 32), generator=g).float()
    kp = pts[:, :n].clone()
    if n >= 4:
        kp[:, 1] = kp[:, 0]                                     # two keypoints coincide
        kp[:, 2] = torch.tensor([40.0, 40.0, 40.0])             # an empty ball
        kp[:, 3] = torch.tensor([-40.0, 0.0, 0.0])
    G = torch.randint(-3, 4, (B, n, 32, 4), generator=g).float()
    F, cnt, nn_idx = ops.ume_moments(pts.to(gpu), kp.to(gpu), feat.to(gpu), K, r, return_count=True, return_idx=True, normalize=False)
    nn_cpu = nn_idx.cpu()
    inside = ((pts[:, None] - kp[:, :, None]).norm(dim=-1) < r).sum(-1)       # [B, n]
    assert torch.equal((nn_cpu >= 0).sum(-1), torch.minimum(inside, torch.tensor(K)))
    if n >= 4:
        assert int((inside > K).sum()) >= 5 and int((inside == 0).sum()) >= 4, "the case needs saturated and empty balls"
        assert torch.equal(nn_cpu[:, 0], nn_cpu[:, 1])
        if K > 1:
            assert int(((inside > 0) & (inside < K)).sum()) >= 1, "the case needs a list shorter than K"
    else:
        assert int((inside >= 1).sum()) == B
    f = feat.to(gpu).requires_grad_()
    out = ume_grad.ume_moments(pts.to(gpu), kp.to(gpu), f, K, r, normalize=False)
    assert torch.equal(out, F)
    (out * G.to(gpu)).sum().backward()
    want = uref.moments_grad(pts.double(), feat.double(), nn_cpu, G.double(), normalize=False)
    # every partial sum stays an integer below 2^24
    h = torch.cat([torch.ones(B, N, 1), pts.abs()], -1).double()
    member = torch.zeros(B, N, dtype=torch.float64)
    for b in range(B):
        member[b].index_add_(0, nn_cpu[b][nn_cpu[b] >= 0], torch.ones(int((nn_cpu[b] >= 0).sum()), dtype=torch.float64))
    assert float((member * 3 * h.sum(-1)).max()) < 2 ** 24
    got = f.grad.cpu()
    print(f"[ume ladder] moments N = {N} n = {n} K = {K}: lists of {int((nn_cpu >= 0).sum(-1).min())} .. {int((nn_cpu >= 0).sum(-1).max())}, "
          f"{int((member > 0).sum())} points in a list, entries differing from fp64 {int((got.double() != want).sum())}")
    assert torch.equal(got.double(), want)
    in_no_ball = member == 0
    assert int(in_no_ball.sum()) > 100 and bool((got[in_no_ball] == 0).all())
    assert float(want.abs().max()) > 0
