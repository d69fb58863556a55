"""GPU: the backward of the RTUME solve (csrc/rtume_grad.hip over csrc/polar_grad.h) per hypothesis -- at the launch's edges, down a
ladder of gaps s2 + d s3 to 1e-6 s1, on either side of the cut UMEREG_RTUME_BWD_MIN_GAP with pairs that are exact in fp32, on exactly
repeated singular values, on a near-singular group among benign pairs, without a path through R, with masses at the size of the
reference's 1e-16 terms, and through `CubeRegistrationLoss` on both branches of its selection.

Inputs, truths and gates: tests/rtume_grad_cases.py (checked on the CPU by tests/test_rtume_grad_cases_cpu.py).  Truth: the closed
form of tests/cube_loss_ref.py in fp64 on the fp32 inputs, with the header's cut.  Gate, per HYPOTHESIS: every 32 x 4 gradient's
relative error <= 4 x the largest such error of the same closed form in fp32 on the CPU over the same rows, and <= the sharp bar
(4 x the fp32 closed form's error on the 1e-1 rung) wherever the truth itself resolves the case; never the GPU's own output.
Every test prints what it saw (`pytest -s`; the record is profiles/rtume_grad/ladders.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

import cube_loss_ref as cref
import rtume_grad_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 2, 3, 7, 8, 9, 15, 257, 4096]   # one and two hypotheses per wavefront, either side of the 8 of a workgroup, many workgroups


def op_grads(gpu, G, H, dT):
    """(T, dG, dH) through the autograd op: what training gets"""
    from umeregrobust_amd import rtume_grad
    a, b = G.to(gpu).requires_grad_(), H.to(gpu).requires_grad_()
    T = rtume_grad.rtume_solve(a, b)
    (T * dT.to(gpu)).sum().backward()
    return T.detach(), a.grad, b.grad


def raw_grads(gpu, G, H, dT):
    from umeregrobust_amd import rtume_grad
    return rtume_grad.rtume_bwd_raw(G.to(gpu), H.to(gpu), dT.to(gpu))


def both_routes(gpu, G, H, dT):
    """(T, dG, dH): the op's, after asserting that the raw entry gives the same bits and the forward is ops.rtume_solve's"""
    from umeregrobust_amd import ops
    T, dG, dH = op_grads(gpu, G, H, dT)
    rG, rH = raw_grads(gpu, G, H, dT)
    assert same_bits(rG, dG) and same_bits(rH, dH), "rtume_bwd_raw and the autograd op differ"
    assert same_bits(T, ops.rtume_solve(G.to(gpu), H.to(gpu))[0]), "the op's forward is not ops.rtume_solve's"
    return T, dG, dH


def same_bits(a, b):
    """bit for bit (a NaN equals itself here)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def norms(x):
    return x.detach().double().cpu().flatten(-2).norm(dim=-1)


def mask(n, where):
    m = torch.zeros(n, dtype=torch.bool)
    m[list(where)] = True
    return m


def test_the_cut_is_the_header_s(gpu):
    from umeregrobust_amd import rtume_grad
    assert rtume_grad.MIN_GAP == rc.MIN_GAP
    bar = rc.sharp_bar()
    rc.say(f"sharp bar: dG {bar[0]:.3e}  dH {bar[1]:.3e}")


# ---- 1: per hypothesis at the launch's edges ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_case(n, thin):
    G, H, dT = cref.ume_pairs(n, 7000 + 1000 * int(thin) + n, thin=thin)
    return (G, H, dT) + rc.truth_and_yard(G, H, dT)


@pytest.mark.parametrize("thin", [False, True], ids=["full", "thin"])
@pytest.mark.parametrize("n", SIZES)
def test_per_hypothesis_at_the_launch_edges(gpu, n, thin):
    G, H, dT, truth, yard = edge_case(n, thin)
    ratio = rc.gap_ratio(G, H)
    rc.say(f"n = {n} {'thin' if thin else 'full'}: (s2 + d s3) / s1 >= {float(ratio.min()):.3f}")
    assert float(ratio.min()) >= 0.05, "the case must not stand on the convention"
    _, dG, dH = both_routes(gpu, G, H, dT)
    bar = rc.sharp_bar()
    name = f"n = {n} {'thin' if thin else 'full'}"
    rc.row_gate(dG, truth[0], yard[0], f"{name} dG", bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], f"{name} dH", bar=bar[1])


# ---- 2: the ladder ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gap", rc.GAP_RUNGS)
def test_gap_ladder(gpu, gap):
    """d = -1 and (s2 + d s3) / s1 = gap: the derivative grows as 1 / gap, the fp32 closed form loses its digits from 1e-2 on, the
    kernel (fp64 on the fp32 inputs) must not: the sharp bar on every rung the truth resolves"""
    G, H, dT = rc.gap_rung(gap)
    truth, yard = rc.truth_and_yard(G, H, dT)
    ok = rc.eligible(gap)
    res = rc.truth_resolution()
    rc.say(f"gap {gap:.0e}: truth's resolution {'not measured (no compiler)' if res is None else format(res[gap], '.2e')}: "
           f"{'eligible' if ok else 'NOT eligible'} for the sharp bar")
    assert ok or gap not in rc.GAP_RUNGS_REQUIRED
    _, dG, dH = both_routes(gpu, G, H, dT)
    bar = rc.sharp_bar() if ok else (None, None)
    rc.row_gate(dG, truth[0], yard[0], f"gap {gap:.0e} dG", bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], f"gap {gap:.0e} dH", bar=bar[1])


# ---- 3: the cut ---------------------------------------------------------------------------------------------------------------

def test_the_cut_is_strict_and_relative(gpu):
    """the five exact pairs (7.45e-9 dropped, 1.19e-8 kept at s1 = 0.625, 1.49e-8 kept with s1 = s2, 2.98e-8 kept, 1.86e-9 dropped) among
    benign pairs: every row within the sharp bar of the truth with the header's cut -- the two sides are six orders of magnitude apart --
    and the benign rows bit-equal to a launch without the cut pairs"""
    G, H, dT = rc.cut_case()
    truth, yard = rc.truth_and_yard(G, H, dT)
    _, dG, dH = both_routes(gpu, G, H, dT)
    special = mask(rc.CUT_TOTAL, rc.CUT_WHERE)
    groups = {"exact cut pairs": special, "benign": ~special}
    bar = rc.sharp_bar()
    rc.row_gate(dG, truth[0], yard[0], "cut dG", groups=groups, bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], "cut dH", groups=groups, bar=bar[1])
    top = float(norms(dG)[~special].max())
    for w, (s1, s2, e, kept) in zip(rc.CUT_WHERE, rc.CUT_PAIRS):
        a = float(norms(dG)[w])
        rc.say(f"cut pair ({s1}, {s2}, e = {e}), ratio {rc.cut_ratio(s1, s2, e):.4e}, {'kept' if kept else 'dropped'}: |dG| gpu {a:.6e}  "
               f"truth {float(norms(truth[0])[w]):.6e}  (benign rows up to {top:.3e})")
        assert np.isfinite(a) and (kept or a < 1e4 * top) and (not kept or a > 1e4 * top)
    benign = (~special).nonzero().flatten()
    _, bG, bH = op_grads(gpu, G[benign], H[benign], dT[benign])
    assert torch.equal(dG[benign.to(gpu)], bG) and torch.equal(dH[benign.to(gpu)], bH)
    # the exact-gap-0 pair (1, 0.5, -0.5) among them: finite, and no other row moves
    G2, H2, dT2 = rc.cut_case(True)
    T2, dG2, dH2 = both_routes(gpu, G2, H2, dT2)
    assert torch.isfinite(T2).all() and torch.isfinite(dG2).all() and torch.isfinite(dH2).all()
    others = (~mask(rc.CUT_TOTAL, [rc.GAP_ZERO_WHERE])).nonzero().flatten().to(gpu)
    assert torch.equal(dG2[others], dG[others]) and torch.equal(dH2[others], dH[others])
    z = float(norms(dG2)[rc.GAP_ZERO_WHERE])
    rc.say(f"exact gap 0: |dG| gpu {z:.6e}")
    assert z < 1e4 * top


# ---- 4: repeated values -------------------------------------------------------------------------------------------------------

def test_repeated_values_are_no_singularity(gpu):
    """signed values (1, 1, 0.25), (1, 0.5, 0.5), (1, 1, 1), (1, 1, -0.25), exact in fp32, each in a wavefront with a benign pair:
    fp64 autograd through an SVD gives NaN there (tests/test_rtume_grad_cases_cpu.py); the kernel's formula has no such term"""
    G, H, dT = rc.repeated_case()
    truth, yard = rc.truth_and_yard(G, H, dT)
    _, dG, dH = both_routes(gpu, G, H, dT)
    rep = mask(8, rc.REPEATED_WHERE)
    groups = {"repeated": rep, "benign": ~rep}
    bar = rc.sharp_bar()
    rc.row_gate(dG, truth[0], yard[0], "repeated values dG", groups=groups, bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], "repeated values dH", groups=groups, bar=bar[1])


# ---- 5: mixed -----------------------------------------------------------------------------------------------------------------

def test_near_singular_pairs_among_benign_ones(gpu):
    """four pairs at gap 1e-4 in slots 5, 17, 40, 63 of 64: each group against its own rows of the fp32 closed form, and the bar"""
    G, H, dT, ill = rc.mixed_case()
    truth, yard = rc.truth_and_yard(G, H, dT)
    _, dG, dH = both_routes(gpu, G, H, dT)
    groups = {"benign": ~ill, "gap 1e-4": ill}
    bar = rc.sharp_bar()
    rc.row_gate(dG, truth[0], yard[0], "mixed dG", groups=groups, bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], "mixed dH", groups=groups, bar=bar[1])


# ---- 6: no path through R -----------------------------------------------------------------------------------------------------

def test_no_path_through_r_by_value(gpu):
    """A = 0: the forward takes R = I, the closed form gives the same convention (U = V = I, every gap 0), and the translation's terms
    that do not pass through R are compared by value"""
    Gz, Hz, dTz = rc.zero_pair()
    Gb, Hb, dTb = cref.ume_pairs(3, 7100)
    G, H, dT = torch.cat([Gb[:1], Gz, Gb[1:]]), torch.cat([Hb[:1], Hz, Hb[1:]]), torch.cat([dTb[:1], dTz, dTb[1:]])       # the zero pair in an odd slot
    truth, yard = rc.truth_and_yard(G, H, dT)
    T, dG, dH = both_routes(gpu, G, H, dT)
    assert torch.equal(T[1, :3, :3].cpu(), torch.eye(3))
    z = mask(4, [1])
    bar = rc.sharp_bar()
    rc.row_gate(dG, truth[0], yard[0], "A = 0 dG", groups={"A = 0": z, "benign": ~z}, bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], "A = 0 dH", groups={"A = 0": z, "benign": ~z}, bar=bar[1])


@pytest.mark.parametrize("slot", [0, 3])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_poisoned_pair_stays_in_its_rows(gpu, value, slot):
    """a pair with a NaN or an Inf coordinate in slot 0 and in an odd slot: every other hypothesis bit-equal to a launch without it"""
    G, H, dT = cref.ume_pairs(9, 7101)
    _, dG0, dH0 = op_grads(gpu, G, H, dT)
    Gp, Hp = rc.poisoned_pair(value)
    G, H = G.clone(), H.clone()
    G[slot], H[slot] = Gp[0], Hp[0]
    _, dG, dH = both_routes(gpu, G, H, dT)
    others = (~mask(9, [slot])).nonzero().flatten().to(gpu)
    rc.say(f"{value} in slot {slot}: finite entries in its own rows {int(torch.isfinite(dG[slot]).sum())} of 128 (dG), {int(torch.isfinite(dH[slot]).sum())} (dH)")
    assert torch.isfinite(dG[others]).all() and torch.equal(dG[others], dG0[others]) and torch.equal(dH[others], dH0[others])


# ---- 7: small masses ----------------------------------------------------------------------------------------------------------

def test_small_masses_keep_both_epsilons(gpu):
    """masses scaled by 2^-23: sum mg^2 is 4e-16, and a kernel with one 1e-16 in the left denominator where the reference has two
    would be 1e-1 row-relative from the truth (asserted on the CPU)"""
    G, H, dT = rc.small_mass_case()
    truth, yard = rc.truth_and_yard(G, H, dT)
    _, dG, dH = both_routes(gpu, G, H, dT)
    bar = rc.sharp_bar()
    rc.row_gate(dG, truth[0], yard[0], "small masses dG", bar=bar[0])
    rc.row_gate(dH, truth[1], yard[1], "small masses dH", bar=bar[1])


# ---- 8: the loss --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loss_case(name):
    g14, g15 = np.load(os.path.join(GOLDEN, "g14_ume_contrastive.npz")), np.load(os.path.join(GOLDEN, "g15_cube_registration.npz"))
    thr, scale = float(g15[f"{name}_thr"]), float(g15["cfg_cube_scale"])
    t = {k: torch.from_numpy(g14[k]) for k in ("velo_ume", "ref_ume", "gt_tform", "ratio", "with_kpts", "velo_kp", "ref_kp")}
    truth = cref.loss_and_grads(t["velo_ume"].double(), t["ref_ume"].double(), t["gt_tform"].double(), t["ratio"], t["with_kpts"], scale, thr)
    yard = cref.loss_and_grads(t["velo_ume"], t["ref_ume"], t["gt_tform"], t["ratio"], t["with_kpts"], scale, thr)
    sel = t["ratio"] >= thr
    if int(sel.sum()) == 0:
        sel = t["ratio"] >= t["ratio"].median(dim=-1, keepdim=True)[0]
    cfg = (int(g15["cfg_rtume_max_nn"]), float(g15["cfg_rtume_r_nn"]), scale, thr)
    return t, cfg, truth[3:], yard[3:], sel


@pytest.mark.parametrize("name", ["main", "median"])
def test_loss_gradients_per_keypoint(gpu, name):
    """`CubeRegistrationLoss` on the fixture, on the threshold's branch and on the fall-back to the row median: the UME gradients of
    keypoints that are not selected are exactly 0, the selected ones pass the row gate"""
    from umeregrobust_amd.cube_loss import CubeRegistrationLoss
    t, (max_nn, r_nn, scale, thr), truth, yard, sel = loss_case(name)
    fn = CubeRegistrationLoss(max_nn, r_nn, cube_scale=scale, nn_inter_ratio_thr=thr)
    a, b = t["velo_ume"].to(gpu).requires_grad_(), t["ref_ume"].to(gpu).requires_grad_()
    loss, _, _ = fn(t["velo_kp"].to(gpu), a, t["ref_kp"].to(gpu), b, t["gt_tform"].to(gpu), t["ratio"].to(gpu), t["with_kpts"].to(gpu))
    loss.backward()
    n_sel = int(sel.sum())
    rc.say(f"loss {name}: {n_sel} of {sel.numel()} keypoints selected")
    assert 0 < n_sel < sel.numel() and (name == "main") == bool((t["ratio"] >= thr).any())
    for got, t64, y32, key in zip((a.grad, b.grad), truth, yard, ("grad_src_ume", "grad_tgt_ume")):
        got = got.cpu()
        assert bool((got[~sel] == 0).all()) and bool((t64[~sel] == 0).all()), f"{key}: a keypoint that is not selected has a gradient"
        assert float(norms(got[sel]).min()) > 0
        rc.row_gate(got, t64, y32, f"loss {name} {key}", groups={"selected": sel.flatten()})
