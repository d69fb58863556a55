"""GPU: the backward passes of include/umereg_ume_grad.h and `ume_loss.UMEContrastiveLoss` on top of them -- the moments'
gradient exact on integers and gated on real features, the distance's gradient gated at tile edges, its invariance and its
D = 0 convention, both entries twice between guard bands, the loss against the reference's own class
(tests/golden/g14_ume_contrastive.npz) and a training run with the trainer's total loss.

Yardsticks: tests/ume_grad_ref.py in fp64 is the truth; the SAME helper in fp32 on the CPU sets every gate
(max |gpu - fp64| <= 4 max |fp32 helper - fp64| per tensor, ume_grad_ref.gate); never the GPU's own output."""
import os

import numpy as np
import pytest
import torch

import ume_grad_ref as uref
from test_abi_guard import Guard

pytestmark = pytest.mark.gpu

GOLDEN = "g14_ume_contrastive.npz"


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1 / 2: moments ------------------------------------------------------------------------------------------------------

def test_moments_backward_is_exact_on_integers(gpu):
    """1: lattice coordinates, integer features and integer dF in [-3, 3], raw moments, B = 2; saturated and empty balls, two
    coinciding keypoints.  Every sum is a sum of integers below 2^24, so dfeat EQUALS the fp64 restatement."""
    from umeregrobust_amd import ops, ume_grad
    g = gen(1)
    B, N, n, K, r = 2, 8000, 40, 32, 2.5
    pts = torch.randint(-12, 13, (B, N, 3), generator=g).float()
    feat = torch.randint(-3, 4, (B, N, 32), generator=g).float()
    kp = pts[:, :n].clone()
    kp[:, 1] = kp[:, 0]                                     # two keypoints coincide
    kp[:, 2] = torch.tensor([40.0, 40.0, 40.0])             # an empty ball
    kp[:, 3] = torch.tensor([-40.0, 0.0, 0.0])
    G = torch.randint(-3, 4, (B, n, 32, 4), generator=g).float()
    F, cnt, nn_idx = ops.ume_moments(pts.to(gpu), kp.to(gpu), feat.to(gpu), K, r, return_count=True, return_idx=True, normalize=False)
    nn_cpu = nn_idx.cpu()
    inside = ((pts[:, None] - kp[:, :, None]).norm(dim=-1) < r).sum(-1)       # [B, n]
    assert int((inside > K).sum()) >= 5 and int((inside == 0).sum()) >= 4, "the case needs saturated and empty balls"
    assert torch.equal((nn_cpu >= 0).sum(-1), torch.minimum(inside, torch.tensor(K)))
    assert torch.equal(nn_cpu[:, 0], nn_cpu[:, 1])
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
    assert torch.equal(got.double(), want)
    in_no_ball = member == 0
    assert int(in_no_ball.sum()) > 100 and bool((got[in_no_ball] == 0).all())
    assert float(want.abs().max()) > 0


def moments_case(n, signed):
    g = gen(100 + n + int(signed))
    N, K, r = 50000, 750, 5.0
    pts = (torch.rand(1, N, 3, generator=g) * torch.tensor([60.0, 60.0, 6.0]))
    feat = torch.rand(1, N, 32, generator=g) + 0.05
    if signed:
        feat = feat - 0.3                                   # signed entries, row sums still well away from 0
    kp = pts[:, torch.randperm(N, generator=g)[:n]].contiguous()
    G = torch.randn(1, n, 32, 4, generator=g)
    return pts, feat, kp, G, K, r


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n", [1, 256, 4096])
def test_moments_backward_normalised(gpu, n, signed):
    """2: N = 50 000, K = 750 with saturated balls, positive and signed features, gated against fp64 autograd on the forward's own
    neighbour lists"""
    from umeregrobust_amd import ops, ume_grad
    pts, feat, kp, G, K, r = moments_case(n, signed)
    f = feat.to(gpu).requires_grad_()
    out = ume_grad.ume_moments(pts.to(gpu), kp.to(gpu), f, K, r, normalize=True)
    F, cnt, nn_idx = ops.ume_moments(pts.to(gpu), kp.to(gpu), feat.to(gpu), K, r, return_count=True, return_idx=True, normalize=True)
    assert torch.equal(out, F)
    (out * G.to(gpu)).sum().backward()
    nn_cpu = nn_idx.cpu()
    sat = int(((nn_cpu >= 0).sum(-1) == K).sum())
    assert sat >= max(1, n // 4) or n == 1, f"{sat} of {n} balls saturated"
    s = torch.stack([feat[0][nn_cpu[0, i][nn_cpu[0, i] >= 0]].double().sum() for i in range(min(n, 64))])
    assert float(s.abs().min()) > 100, "|s_i| must stay away from 0"
    want = uref.moments_grad(pts.double(), feat.double(), nn_cpu, G.double())
    yard = uref.moments_grad(pts, feat, nn_cpu, G)
    uref.gate(f.grad, want, yard, f"moments backward n={n} signed={signed}")
    again = ume_grad.moments_bwd_raw(pts.to(gpu), feat.to(gpu), nn_idx, F, G.to(gpu))
    assert torch.equal(again, f.grad)


# ---- 3 / 4 / 5: the distance ----------------------------------------------------------------------------------------------

COLS = torch.tensor([1.0, 6.0, 6.0, 1.5])


def dist_case(B, n1, n2, seed, copies=0):
    """UME-like matrices (columns of different scale); the first min(n1, n2) // 2 rows of ume2 are perturbed copies of ume1's
    (small diagonal), the next `copies` exact copies"""
    g = gen(seed)
    u1 = torch.randn(B, n1, 32, 4, generator=g) * COLS + torch.tensor([2.0, 0.0, 0.0, 0.0])
    u2 = torch.randn(B, n2, 32, 4, generator=g) * COLS + torch.tensor([2.0, 0.0, 0.0, 0.0])
    m = min(n1, n2) // 2
    u2[:, :m] = u1[:, :m] + 0.08 * torch.randn(B, m, 32, 4, generator=g) * COLS
    u2[:, m:m + copies] = u1[:, m:m + copies]
    gD = torch.randn(B, n1, n2, generator=g)
    return u1, u2, gD


def dist_truth(u1, u2, gD, drop=None):
    D, a, b = uref.cdist_grads(u1.double(), u2.double(), gD.double(), drop)
    _, ya, yb = uref.cdist_grads(u1, u2, gD, drop)
    return D, (a, b), (ya, yb)


def preconditions(u1, u2, D, drop=None):
    cond = max(float(torch.linalg.cond(u.double()).max()) for u in (u1, u2))
    dmin = float(D.min() if drop is None else D[~drop].min())
    assert dmin >= 0.05 and cond <= 50, (dmin, cond)
    return dmin, cond


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n1,n2", [(1, 1), (48, 48), (256, 256), (257, 130), (2048, 1536)])
def test_distance_backward(gpu, n1, n2, B):
    """3: both gradients against fp64 autograd through the reference's own ume_cdist, at sizes that are not multiples of the tile"""
    from umeregrobust_amd import ume_grad
    u1, u2, gD = dist_case(B, n1, n2, 7 * n1 + n2 + B)
    D, truth, yard = dist_truth(u1, u2, gD)
    dmin, cond = preconditions(u1, u2, D)
    a, b = u1.to(gpu).requires_grad_(), u2.to(gpu).requires_grad_()
    Dg = ume_grad.ume_cdist(a, b)
    (Dg * gD.to(gpu)).sum().backward()
    print(f"[distance] B={B} n1={n1} n2={n2}: min D {dmin:.3f}, diagonal mean {float(D[:, :min(n1, n2) // 2].diagonal(dim1=-1, dim2=-2).mean()) if min(n1, n2) > 1 else float('nan'):.3f}, "
          f"max cond {cond:.1f}, max|D gpu - fp64| {float((Dg.detach().cpu().double() - D).abs().max()):.2e}")
    assert torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    uref.gate(a.grad, truth[0], yard[0], f"dume1 B={B} {n1}x{n2}")
    uref.gate(b.grad, truth[1], yard[1], f"dume2 B={B} {n1}x{n2}")


@pytest.mark.parametrize("side", [0, 1])
def test_distance_backward_one_side_only(gpu, side):
    from umeregrobust_amd import ume_grad
    u1, u2, gD = dist_case(2, 100, 75, 31)
    D, truth, yard = dist_truth(u1, u2, gD)
    preconditions(u1, u2, D)
    t = [u1.to(gpu), u2.to(gpu)]
    t[side].requires_grad_()
    (ume_grad.ume_cdist(*t) * gD.to(gpu)).sum().backward()
    assert t[1 - side].grad is None
    uref.gate(t[side].grad, truth[side], yard[side], f"dume{side + 1} alone")
    # and the raw entry with the other output absent gives the same bits as with both
    Dg = ume_grad.ume_cdist(u1.to(gpu), u2.to(gpu))
    both = ume_grad.cdist_bwd_raw(u1.to(gpu), u2.to(gpu), Dg, gD.to(gpu))
    one = ume_grad.cdist_bwd_raw(u1.to(gpu), u2.to(gpu), Dg, gD.to(gpu), need1=side == 0, need2=side == 1)
    assert one[1 - side] is None and torch.equal(one[side], both[side]) and torch.equal(both[side], t[side].grad)


def invariance(Q, dF):
    """max_i |Q_i^T dF_i|_F / |dF_i|_F"""
    dF = dF.detach().double().cpu()
    return float(((Q.transpose(-1, -2) @ dF).flatten(-2).norm(dim=-1) / dF.flatten(-2).norm(dim=-1)).max())


def test_distance_gradient_is_invariant_under_a_change_of_basis(gpu):
    """4: D does not change under F -> F A, so Q_i^T dF_i = 0; the GPU's residual against 4 x the fp32 helper's"""
    from umeregrobust_amd import ume_grad
    u1, u2, gD = dist_case(1, 300, 200, 41)
    D, truth, yard = dist_truth(u1, u2, gD)
    preconditions(u1, u2, D)
    a, b = u1.to(gpu).requires_grad_(), u2.to(gpu).requires_grad_()
    (ume_grad.ume_cdist(a, b) * gD.to(gpu)).sum().backward()
    for name, u, got, y, t in (("dume1", u1, a.grad, yard[0], truth[0]), ("dume2", u2, b.grad, yard[1], truth[1])):
        Q = torch.linalg.qr(u.double()).Q
        r_gpu, r_cpu, r_truth = invariance(Q, got), invariance(Q, y), invariance(Q, t)
        print(f"[invariance] {name}: |Q^T dF| / |dF|  gpu {r_gpu:.3e}  fp32 helper {r_cpu:.3e}  fp64 {r_truth:.3e}")
        assert r_truth < 1e-12 and r_gpu <= 4 * r_cpu


def test_distance_zero_has_no_gradient(gpu):
    """5: exact copies of rows of ume1 in ume2: finite gradients, equal within the gate to the truth with those pairs left out"""
    from umeregrobust_amd import ume_grad
    n1, n2, copies = 96, 80, 9
    u1, u2, gD = dist_case(2, n1, n2, 51, copies=copies)
    m = min(n1, n2) // 2
    drop = torch.zeros(2, n1, n2, dtype=torch.bool)
    idx = torch.arange(m, m + copies)
    drop[:, idx, idx] = True
    D, truth, yard = dist_truth(u1, u2, gD, drop)
    preconditions(u1, u2, D, drop)
    assert float(D[drop].max()) < 1e-7
    a, b = u1.to(gpu).requires_grad_(), u2.to(gpu).requires_grad_()
    Dg = ume_grad.ume_cdist(a, b)
    print(f"[D = 0] the forward's D on equal subspaces: max {float(Dg.detach().cpu()[drop].max()):.3e} (threshold {ume_grad.D_MIN})")
    assert float(Dg.detach().cpu()[drop].max()) <= ume_grad.D_MIN < 0.05 / 4
    (Dg * gD.to(gpu)).sum().backward()
    assert torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    uref.gate(a.grad, truth[0], yard[0], "dume1 with D = 0 pairs")
    uref.gate(b.grad, truth[1], yard[1], "dume2 with D = 0 pairs")


# ---- 6: determinism and bounds ----------------------------------------------------------------------------------------------

def test_entries_are_deterministic_between_guard_bands(gpu):
    """6: every compute entry of include/umereg_ume_grad.h twice between 4 KiB canary bands on outputs and scratch: bands intact,
    outputs byte-equal between the runs, whatever the scratch held (the two runs fill it with different bytes)"""
    from umeregrobust_amd import ops, ume_grad
    lib = ume_grad.load_native()
    g = gen(6)
    B, N, n, K, r = 2, 3001, 37, 40, 3.0
    pts = torch.rand(B, N, 3, generator=g) * torch.tensor([20.0, 20.0, 4.0])
    feat = torch.rand(B, N, 32, generator=g) + 0.1
    kp = pts[:, :n].contiguous()
    F, nn_idx = ops.ume_moments(pts.to(gpu), kp.to(gpu), feat.to(gpu), K, r, return_idx=True)
    G = torch.randn(B, n, 32, 4, generator=g)
    n1, n2 = 45, 70
    u1, u2, gD = dist_case(1, n1, n2, 61)
    D = ops.ume_cdist(u1.to(gpu), u2.to(gpu))
    outs = []
    for run in range(2):
        gd = Guard(gpu, run)
        p_pts, _ = gd.inp(pts.numpy(), "pts")
        p_feat, _ = gd.inp(feat.numpy(), "feat")
        p_nn, _ = gd.inp(nn_idx.cpu().numpy(), "nn_idx")
        p_F, _ = gd.inp(F.cpu().numpy(), "F")
        p_G, _ = gd.inp(G.numpy(), "dF")
        res = []
        for normalize in (1, 0):
            p_out, t_out = gd.out((B, N, 32), torch.float32, f"dfeat{normalize}")
            p_ws, n_ws = gd.ws(lib.umereg_ume_moments_bwd_scratch_bytes(B, N, n), "moments scratch")
            gd.call("umereg_ume_moments_bwd_f32", p_pts, p_feat if normalize else None, p_nn, p_F if normalize else None, p_G, B, N, n, K,
                    normalize, p_out, p_ws, n_ws, gd.stream)
            res.append(t_out)
        p_u1, _ = gd.inp(u1[0].numpy(), "ume1")
        p_u2, _ = gd.inp(u2[0].numpy(), "ume2")
        p_D, _ = gd.inp(D[0].cpu().numpy(), "D")
        p_g, _ = gd.inp(gD[0].numpy(), "dD")
        for want1, want2 in ((1, 1), (1, 0), (0, 1)):
            p_d1, t_d1 = gd.out((n1, 32, 4), torch.float32, "dume1")
            p_d2, t_d2 = gd.out((n2, 32, 4), torch.float32, "dume2")
            p_ws, n_ws = gd.ws(lib.umereg_ume_cdist_bwd_scratch_bytes(n1, n2), "cdist scratch")
            gd.call("umereg_ume_cdist_bwd_f32", p_u1, p_u2, p_D, p_g, n1, n2, p_d1 if want1 else None, p_d2 if want2 else None, p_ws, n_ws,
                    gd.stream)
            res += [t for t, w in ((t_d1, want1), (t_d2, want2)) if w]
            if not want1:
                gd.check()
                assert bool((t_d1.view(torch.uint8) == gd.poison).all()), "an output that was not asked for was written"
        gd.check()
        assert gd.called == {"umereg_ume_moments_bwd_f32", "umereg_ume_cdist_bwd_f32"}
        outs.append([t.clone() for t in res])
    assert len(outs[0]) == 6
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(outs[0][2], outs[0][4]) and torch.equal(outs[0][3], outs[0][5])


# ---- 7: the loss against the reference's own class ---------------------------------------------------------------------------

def test_loss_equals_the_reference_s(gpu):
    """7: the fixture.  Selection outputs with the tolerances of test_generate_ume_from_keypoints2_batch_vs_oracle; loss and both
    feature gradients within 4 x max(|reference - fp64|, |fp32 helper - fp64|), fp64 on the reference's keypoints and lists."""
    from umeregrobust_amd.ume_loss import UMEContrastiveLoss
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))
    cfg = {k: float(g[f"cfg_{k}"]) for k in ("nn_r", "tau", "tau_neg", "nn_intersection_r", "svd_thr")}
    fn = UMEContrastiveLoss(num_samples=int(g["cfg_num_samples"]), max_nn=int(g["cfg_max_nn"]), min_nn=int(g["cfg_min_nn"]),
                            flat_labels=[int(v) for v in g["cfg_flat_labels"]], **cfg)
    t = lambda k: torch.from_numpy(g[k]).to(gpu)          # noqa: E731
    vf, rf = t("velo_feat").requires_grad_(), t("ref_feat").requires_grad_()
    loss, velo_kp, ref_kp, velo_ume, ref_ume, ratio, with_kpts = fn(t("velo_pts"), t("velo_seg"), vf, t("ref_pts"), rf, t("gt_tform"))
    loss.backward()
    N_ = lambda x: x.detach().cpu().numpy()               # noqa: E731
    assert np.array_equal(N_(with_kpts), g["with_kpts"]) and np.array_equal(N_(velo_kp), g["velo_kp"])
    assert np.abs(N_(ref_kp) - g["ref_kp"]).max() < 1e-5 and np.abs(N_(ratio) - g["ratio"]).max() < 1e-6
    for a, b in ((N_(velo_ume), g["velo_ume"]), (N_(ref_ume), g["ref_ume"])):
        scale = np.abs(b).max(axis=(2, 3), keepdims=True) + 1e-30
        assert a.shape == b.shape and (np.abs(a - b) / scale).max() < 2e-4 and np.median(np.abs(a - b) / scale) < 1e-6
    args = lambda dt: (torch.from_numpy(g["velo_pts"]).to(dt), torch.from_numpy(g["velo_feat"]).to(dt),            # noqa: E731
                       torch.from_numpy(g["velo_nn_idx"]).long(), torch.from_numpy(g["ref_pts"]).to(dt),
                       torch.from_numpy(g["ref_feat"]).to(dt), torch.from_numpy(g["ref_nn_idx"]).long())
    l64, gv64, gr64, _, _ = uref.loss_and_grads(*args(torch.float64), tau=cfg["tau"], tau_neg=cfg["tau_neg"])
    l32, gv32, gr32, _, _ = uref.loss_and_grads(*args(torch.float32), tau=cfg["tau"], tau_neg=cfg["tau_neg"])
    bound = 4 * max(abs(float(g["loss"]) - float(l64)), abs(float(l32) - float(l64)))
    print(f"[loss] gpu {float(loss.detach()):.8f}  reference {float(g['loss']):.8f}  fp64 {float(l64):.8f}  fp32 helper {float(l32):.8f}; "
          f"|gpu - fp64| {abs(float(loss.detach()) - float(l64)):.2e} against {bound:.2e}")
    assert abs(float(loss.detach()) - float(l64)) <= bound
    for name, got, t64, y32 in (("grad_velo_feat", vf.grad, gv64, gv32), ("grad_ref_feat", rf.grad, gr64, gr32)):
        e_gpu = float((got.detach().cpu().double() - t64).abs().max())
        e_ref = float((torch.from_numpy(g[name]).double() - t64).abs().max())
        e_cpu = float((y32.double() - t64).abs().max())
        print(f"[loss] {name}: max|gpu - fp64| {e_gpu:.3e}  max|reference - fp64| {e_ref:.3e}  max|fp32 helper - fp64| {e_cpu:.3e}  "
              f"ratio {e_gpu / max(e_ref, e_cpu):.3f}  (max|truth| {float(t64.abs().max()):.3e})")
        assert torch.isfinite(got).all() and e_gpu <= 4 * max(e_ref, e_cpu), name


# ---- 8: it trains --------------------------------------------------------------------------------------------------------

def train_with_ume(dev, seed=0, steps=30):
    """the trainer's total loss (train_coloring.py:47-60 with use_ume_loss, ume_loss_weight 0.5, use_reg_loss false) on the twin pair
    of tests/test_sparse_grad_gpu.py"""
    from test_sparse_grad_gpu import initial_state, training_pair
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    from umeregrobust_amd.ume_loss import UMEContrastiveLoss
    src, tgt, matches = training_pair()
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True)
    m.load_state_dict(initial_state(seed))
    m = m.to(dev).train()
    point_loss = MyInfoNCELossNoSeg(tau=0.1, neg_euclid_dist=5)
    ume_loss = UMEContrastiveLoss(num_samples=64, max_nn=96, min_nn=12, nn_r=1.5, tau=0.1, tau_neg=0.1, flat_labels=[9], nn_intersection_r=0.2)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    st = [SparseTensor(torch.ones(len(c), 1, device=dev), coordinates=torch.from_numpy(c.astype(np.int32)).to(dev)) for c in (src, tgt)]
    src_pts = torch.from_numpy(src[None, :, 1:] * 0.3).float().to(dev)
    tgt_pts = torch.from_numpy(tgt[None, :, 1:] * 0.3).float().to(dev)
    seg = torch.zeros(1, len(src), 1, dtype=torch.int64, device=dev)
    gt = torch.eye(4, device=dev)[None].clone()
    gt[0, :3, 3] = torch.tensor([5.0, -3.0, 1.0], device=dev) * 0.3
    mt = torch.from_numpy(matches[None]).to(dev)
    hist, finite = [], True
    for _ in range(steps):
        opt.zero_grad()
        src_feat = torch.stack(m(st[0]).decomposed_features, dim=0)
        tgt_feat = torch.stack(m(st[1]).decomposed_features, dim=0)
        l_point = point_loss(src_feat, src_pts, tgt_feat, mt)
        l_ume, _, _, velo_ume, _, _, _ = ume_loss(src_pts, seg, src_feat, tgt_pts, tgt_feat, gt)
        loss = 0.5 * l_point + 0.5 * l_ume
        loss.backward()
        finite = finite and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        opt.step()
        hist.append((float(l_point.detach()), float(l_ume.detach()), velo_ume.shape[1]))
    return m, hist, finite


def test_it_trains(gpu):
    """8: a few tens of Adam steps: every parameter gradient finite at every step, the UME loss lower at the end than at the
    start, and two runs from the same seed end with bit-identical parameters"""
    m, hist, finite = train_with_ume(gpu)
    m2, hist2, finite2 = train_with_ume(gpu)
    print(f"[training] point loss {hist[0][0]:.4f} -> {hist[-1][0]:.4f}; UME loss {hist[0][1]:.4f} -> {hist[-1][1]:.4f}; "
          f"valid keypoints {hist[0][2]} .. {hist[-1][2]} over {len(hist)} steps")
    assert finite and finite2 and all(np.isfinite(h[1]) for h in hist)
    assert hist[0][2] >= 16
    assert hist[-1][1] < hist[0][1], hist
    assert hist == hist2
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
