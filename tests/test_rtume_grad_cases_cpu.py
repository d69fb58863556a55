"""The inputs of tests/test_rtume_grad_edges_gpu.py and csrc/polar_grad.h itself, without a GPU.

(i)   Every construction of tests/rtume_grad_cases.py is what it claims, asserted in fp64 on the fp32 inputs: the ladder's gaps and
      d = -1, the exact pairs' exactness, side of the cut and margin, the repeated values, the mixed group, the pair without a path
      through R, the small masses and the one-epsilon restatement they must tell from the truth.
(ii)  csrc/polar_grad.h compiled for the host (tests/polar_grad_host.cpp, with the compiler that builds the library) against the fp64
      closed form through torch.linalg.svd, 64 random frame pairs per class: 1e-12 where no gap is small; the frames' R equal to
      polar_rotation's bit for bit; the cut strict, relative to s1, and the dropped term exactly absent.  On the gap rungs the
      agreement of the two fp64 evaluations is the truth's own uncertainty: it is printed, and the rungs 1e-1 ... 1e-5 must be
      resolved to a tenth of the sharp bar, which is what lets the GPU tests hold the kernel to that bar there."""
import numpy as np
import pytest
import torch

import cube_loss_ref as cref
import rtume_grad_cases as rc


def norms(x):
    return x.flatten(-2).norm(dim=-1)


# ---- (i) the cases ------------------------------------------------------------------------------------------------------------

def test_cut_is_the_header_s_and_the_bar_binds():
    from umeregrobust_amd import rtume_grad
    assert rc.MIN_GAP == rtume_grad.MIN_GAP == 1e-8
    bar = rc.sharp_bar()
    rc.say(f"sharp bar: dG {bar[0]:.3e}  dH {bar[1]:.3e}")
    # above one fp32 rounding of the output, so that a correct kernel can pass (that it binds: test_gap_rung_is_what_it_claims)
    assert all(4 * 2.0 ** -24 < b for b in bar)


@pytest.mark.parametrize("gap", rc.GAP_RUNGS)
def test_gap_rung_is_what_it_claims(gap):
    G, H, dT = rc.gap_rung(gap)
    assert G.dtype == H.dtype == dT.dtype == torch.float32 and G.shape == H.shape == (17, 32, 4) and rc.N_RUNG == 17
    assert float(G[:, :, 0].min()) > 0 and float(H[:, :, 0].min()) > 0
    ratio, (_, d) = rc.gap_ratio(G, H), rc.signed_spectrum(G, H)
    truth, yard = rc.truth_and_yard(G, H, dT)
    e = [float(rc.row_rel(y, t).max()) for y, t in zip(yard, truth)]
    rc.say(f"gap rung {gap:.0e}: realised (s2 + d s3) / s1 {float(ratio.min()):.6e} .. {float(ratio.max()):.6e}, d = -1 on {int((d < 0).sum())} of 17, "
           f"|dG| of the truth up to {float(norms(truth[0]).max()):.3e}, fp32 closed form row-rel max {e[0]:.2e} / {e[1]:.2e}")
    assert bool((d == -1).all())
    assert float(ratio.min()) >= gap / 2 and float(ratio.max()) <= gap * 2
    assert all(torch.isfinite(t).all() for t in truth)
    if gap <= 1e-2:      # here "4 x helper" alone would let a kernel be as wrong as fp32 is: the sharp bar is the gate that binds
        assert min(e) > max(rc.sharp_bar())


def test_exact_pairs_are_exact_and_on_their_side_of_the_cut():
    q = rc.hadamard_columns()
    assert bool((q.abs() == 1).all()) and torch.equal(q.T @ q, 32 * torch.eye(3, dtype=torch.float64)) and bool((q.sum(0) == 0).all())
    for s1, s2, e, _ in rc.CUT_PAIRS:
        G64, H64 = rc.cut_pair(s1, s2, e)
        assert torch.equal(G64.float().double(), G64) and torch.equal(H64.float().double(), H64)
    G, H = rc.cut_pairs()
    sp, d = rc.signed_spectrum(G, H)
    ratio = rc.gap_ratio(G, H)
    rc.say(f"exact cut pairs: (s2 + d s3) / s1 {[f'{float(r):.4e}' for r in ratio]}  (cut {rc.MIN_GAP})")
    assert bool((d == -1).all())
    for k, (s1, s2, e, kept) in enumerate(rc.CUT_PAIRS):
        want = rc.cut_ratio(s1, s2, e)
        assert abs(float(sp[k, 0]) - s1) <= 1e-15 and abs(float(sp[k, 1]) - s2) <= 1e-15
        assert abs(float(ratio[k]) / want - 1) <= 1e-6
        assert (want > rc.MIN_GAP) == kept and abs(want / rc.MIN_GAP - 1) >= 0.15
    # the second pair is kept only by a cut that scales with s1: its s2 + d s3 itself is below 1e-8
    assert rc.CUT_PAIRS[1][3] and float(sp[1, 1] + sp[1, 2]) < rc.MIN_GAP * 0.85 and float(sp[1, 0]) == 0.625
    assert float(sp[2, 0]) == float(sp[2, 1]) == 0.5


def test_the_cut_moves_the_truth_by_orders_of_magnitude():
    G, H, dT = rc.cut_case()
    assert torch.equal(G[rc.CUT_WHERE], rc.cut_pairs()[0]) and len(set(w % 2 for w in rc.CUT_WHERE)) == 2
    (dG, dH), _ = rc.truth_and_yard(G, H, dT)
    (dG0, dH0), _ = rc.truth_and_yard(G, H, dT, min_gap=0.0)
    benign = [i for i in range(rc.CUT_TOTAL) if i not in rc.CUT_WHERE]
    assert torch.equal(dG[benign], dG0[benign]) and float(rc.gap_ratio(G, H)[benign].min()) > 0.05
    top = float(norms(dG[benign]).max())
    for w, (s1, s2, e, kept) in zip(rc.CUT_WHERE, rc.CUT_PAIRS):
        a, a0 = float(norms(dG[w])), float(norms(dG0[w]))
        rc.say(f"exact cut pair ({s1}, {s2}, e = {e}) {'kept' if kept else 'dropped'}: |dG| {a:.3e} with the cut, {a0:.3e} without (benign rows up to {top:.3e})")
        if kept:
            assert a == a0 and a > 1e4 * top
        else:
            assert a0 >= 1e4 * a and a < 1e4 * top and float(norms(dH0[w])) >= 1e4 * float(norms(dH[w]))
    # with the exact-gap-0 pair: finite truth, the other rows unchanged
    G2, H2, dT2 = rc.cut_case(True)
    sp, d = rc.signed_spectrum(G2, H2)
    assert float((sp[rc.GAP_ZERO_WHERE, 1] + sp[rc.GAP_ZERO_WHERE, 2]).abs()) <= 1e-15 and rc.GAP_ZERO_WHERE not in rc.CUT_WHERE
    (dG2, _), _ = rc.truth_and_yard(G2, H2, dT2)
    others = [i for i in range(rc.CUT_TOTAL) if i != rc.GAP_ZERO_WHERE]
    assert torch.isfinite(dG2).all() and torch.equal(dG2[others], dG[others])


def test_repeated_values_are_exact_and_autograd_through_svd_fails_there():
    G64 = [rc.hadamard_pair((1.0, 1.0, 1.0), sv) for sv in rc.REPEATED]
    assert all(torch.equal(g.float().double(), g) and torch.equal(h.float().double(), h) for g, h in G64)
    G, H, dT = rc.repeated_case()
    sp, _ = rc.signed_spectrum(G, H)
    for w, sv in zip(rc.REPEATED_WHERE, rc.REPEATED):
        assert float((sp[w] - torch.tensor(sv, dtype=torch.float64)).abs().max()) <= 1e-15, (sv, sp[w])
    assert float(rc.gap_ratio(G, H).min()) >= 0.5           # none of them is near the singularity
    (dG, dH), (yG, yH) = rc.truth_and_yard(G, H, dT)
    assert torch.isfinite(dG).all() and torch.isfinite(dH).all() and torch.isfinite(yG).all() and torch.isfinite(yH).all()
    _, aG, _ = cref.solve_grads(G.double(), H.double(), dT.double())
    off = rc.row_rel(aG, dG)
    rc.say(f"repeated values: fp64 autograd through svd, row-rel against the closed form {off[rc.REPEATED_WHERE].tolist()}; "
           f"fp32 closed form {rc.row_rel(yG, dG)[rc.REPEATED_WHERE].tolist()}")
    for w in rc.REPEATED_WHERE:
        assert not np.isfinite(float(off[w])) or float(off[w]) > rc.sharp_bar()[0]
    benign = [i for i in range(8) if i not in rc.REPEATED_WHERE]
    assert float(off[benign].max()) <= 1e-12                # and where the spectrum is separated the two agree
    assert float(rc.row_rel(yG, dG).max()) <= rc.sharp_bar()[0]


def test_mixed_case_is_what_it_claims():
    G, H, dT, ill = rc.mixed_case()
    assert ill.nonzero().flatten().tolist() == [5, 17, 40, 63] == rc.MIXED_ILL
    ratio, (_, d) = rc.gap_ratio(G, H), rc.signed_spectrum(G, H)
    assert float(ratio[ill].min()) >= 0.5e-4 and float(ratio[ill].max()) <= 2e-4 and bool((d[ill] == -1).all()) and float(ratio[~ill].min()) >= 0.1
    truth, yard = rc.truth_and_yard(G, H, dT)
    e = (yard[0].double() - truth[0]).abs().flatten(-2).max(dim=-1).values
    assert float(e[ill].max()) > 100 * float(e[~ill].max())         # a per-tensor gate cannot judge the benign rows here


def test_zero_pair_has_no_path_through_r():
    G, H, dT = rc.zero_pair()
    assert bool((G[:, :, 1:] == 0).all()) and bool((H[:, :, 1:] == 0).all()) and float(G[:, :, 0].min()) > 0 and float(H[:, :, 0].min()) > 0
    S, _ = cref.spectrum(G.double(), H.double())
    assert float(S.abs().max()) == 0
    assert torch.equal(cref.solve(G.double(), H.double())[0, :3, :3], torch.eye(3, dtype=torch.float64))
    (dG, dH), (yG, yH) = rc.truth_and_yard(G, H, dT)
    (dG1, dH1), _ = rc.truth_and_yard(G, H, dT, min_gap=0.0)
    assert torch.equal(dG, dG1) and torch.equal(dH, dH1)            # every gap is 0: no term survives, whatever the cut
    assert float(norms(dG)) > 0.1 and float(norms(dH)) > 0.1        # the translation's terms do: there is a value to compare
    assert float(rc.row_rel(yG, dG)) > 0 and float(rc.row_rel(yH, dH)) > 0


def test_small_masses_tell_one_epsilon_from_two():
    G, H, dT = rc.small_mass_case()
    G0, H0, _ = cref.ume_pairs(17, 5006)
    assert torch.equal(G[:, :, 0] * 2.0 ** rc.SMALL_MASS_SHIFT, G0[:, :, 0]) and torch.equal(G[:, :, 1:], G0[:, :, 1:])
    sq = (G[:, :, 0].double() ** 2).sum(dim=1)
    assert 1e-17 <= float(sq.min()) and float(sq.max()) <= 1e-15
    truth, yard = rc.truth_and_yard(G, H, dT)
    assert all(bool(torch.isfinite(t).all()) for t in truth + yard)                                               # (i)
    one = cref.solve_grads_closed_form(G.double(), H.double(), dT.double(), min_gap=rc.MIN_GAP, parts=rc.parts_one_epsilon)
    off = [float(rc.row_rel(o, t).min()) for o, t in zip(one, truth)]
    rc.say(f"small masses (2^-{rc.SMALL_MASS_SHIFT}): sum mg^2 {float(sq.min()):.3e} .. {float(sq.max()):.3e}, one epsilon in den_l is at least "
           f"{off[0]:.3e} / {off[1]:.3e} row-relative from the truth, the fp32 closed form at most "
           f"{float(rc.row_rel(yard[0], truth[0]).max()):.2e} / {float(rc.row_rel(yard[1], truth[1]).max()):.2e}")
    assert all(o >= 100 * b for o, b in zip(off, rc.sharp_bar()))                                                 # (ii)


# ---- (ii) csrc/polar_grad.h on the host ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    if rc.host_program() is None:
        pytest.skip("no hipcc found: csrc/polar_grad.h cannot be compiled here")
    return lambda A, gR, min_gap=rc.MIN_GAP: rc.host_polar(A, gR, min_gap)


def frames_rotation(U, V):
    """R as rtume_bwd_kernel forms it from the frames, in polar.h's own order of operations"""
    return (U[:, 0, :, None] * V[:, 0, None, :] + U[:, 1, :, None] * V[:, 1, None, :]) + U[:, 2, :, None] * V[:, 2, None, :]


def check_frames(name, has, s, R, U, V):
    """The frames give polar_rotation's R bit for bit, and s is descending, s[0] >= s[1] >= |s[2]|.  The order is the order of the
    column norms of A V; each s[i] = u_i^T A v_i is a sum of nine products of its own, so two EQUAL values may come out one rounding
    apart in either order (they do, on the repeated-value classes): the order is held to 16 x 2^-53 s[0], the rounding of those sums."""
    assert bool(has.all()), name
    assert torch.equal(frames_rotation(U, V), R), f"{name}: the frames' R is not polar_rotation's"
    tol = 16 * 2.0 ** -53 * s[:, 0]
    assert bool((s[:, 0] > 0).all()) and bool((s[:, 0] >= s[:, 1] - tol).all()) and bool((s[:, 1] >= s[:, 2].abs() - tol).all()), name
    if "repeated" not in name:
        assert bool((s[:, 0] >= s[:, 1]).all()) and bool((s[:, 1] >= s[:, 2].abs()).all()), name


def test_host_build_equals_the_closed_form_where_no_gap_is_small(host):
    for name, (A, gR, regular) in rc.host_classes().items():
        if not regular:
            continue
        has, s, gA, R, U, V = host(A, gR)
        check_frames(name, has, s, R, U, V)
        Rt, sp, gAt = rc.polar_closed_form(A, gR, rc.MIN_GAP)
        e, es = float(rc.mat_rel(gA, gAt).max()), float(((s - sp).abs().max(dim=1).values / sp[:, 0]).max())
        rc.say(f"host polar_grad.h, {name}: gA row-rel max {e:.2e}, s {es:.2e} of s1, |R - closed form| {float((R - Rt).abs().max()):.2e}")
        assert e <= 1e-12 and es <= 1e-14, name
        if not name.startswith("s3") and "rank" not in name:
            assert float((R - Rt).abs().max()) <= 1e-12, name


def test_truth_resolves_the_ladder(host):
    """the agreement of the two fp64 evaluations per rung: the truth's own uncertainty"""
    bar = min(rc.sharp_bar())
    res = rc.truth_resolution()
    for gap in rc.GAP_RUNGS:
        rc.say(f"truth's resolution at gap {gap:.0e}: {res[gap]:.2e} (bar / 10 = {bar / 10:.2e}): {'eligible' if rc.eligible(gap) else 'NOT eligible'} for the sharp bar")
        if gap in rc.GAP_RUNGS_REQUIRED:
            assert res[gap] <= bar / 10 and rc.eligible(gap)
    classes = rc.host_classes()
    for name in [k for k, v in classes.items() if not v[2]]:
        A, gR, _ = classes[name]
        has, s, gA, R, U, V = host(A, gR)
        check_frames(name, has, s, R, U, V)
        e = float(rc.mat_rel(gA, rc.polar_closed_form(A, gR, rc.MIN_GAP)[2]).max())
        rc.say(f"host polar_grad.h, {name}: gA row-rel max {e:.2e} between the two fp64 evaluations")
        assert torch.isfinite(gA).all() and np.isfinite(e)


def exact_3x3(sv, shift=1):
    """diag(sv) with its columns rolled: the cross moment of `hadamard_pair`, exactly"""
    return torch.roll(torch.diag(torch.tensor(sv, dtype=torch.float64)), shift, dims=1)[None]


def term_12(U, V):
    """gR = u1 v2^T - u2 v1^T: an upstream gradient that reaches gA through the (1, 2) term alone"""
    return U[:, 1, :, None] * V[:, 2, None, :] - U[:, 2, :, None] * V[:, 1, None, :]


def test_cut_is_strict_relative_and_the_dropped_term_exactly_absent(host):
    gR = torch.randn(1, 3, 3, generator=rc.gen(7000), dtype=torch.float64)
    for s1, s2, e, kept in rc.CUT_PAIRS:
        sv = (s1, s2, -s2 * (1.0 - 2.0 ** (-2 * e)))
        A = exact_3x3(sv)
        has, s, gA, R, U, V = host(A, gR)
        check_frames(str(sv), has, s, R, U, V)
        assert s[0].tolist() == list(sv) and float(s[0, 1] + s[0, 2]) == s2 * 2.0 ** (-2 * e)         # exact: the side is not up to rounding
        assert bool(((U == 0) | (U.abs() == 1)).all()) and bool(((V == 0) | (V.abs() == 1)).all())    # the frames are signed permutations
        only = host(A, term_12(U, V))[2]
        if kept:
            assert float(only.abs().max()) == 2.0 / (s2 * 2.0 ** (-2 * e)), sv                        # Y_12 = (1 - (-1)) / gap, exactly
        else:
            assert bool((only == 0).all()), f"{sv}: the (1, 2) term is not absent"
        assert float(rc.mat_rel(gA, rc.polar_closed_form(A, gR, rc.MIN_GAP)[2])) <= 1e-12, sv
    # strict: a gap EQUAL to min_gap * s1 is dropped (2^-27 is exact, and so is the product), a cut one ulp lower keeps it
    A = exact_3x3((1.0, 0.5, -0.5 * (1.0 - 2.0 ** -26)))
    _, s, _, _, U, V = host(A, gR)
    at = 2.0 ** -27
    assert float(s[0, 1] + s[0, 2]) == at * float(s[0, 0])
    assert bool((host(A, term_12(U, V), at)[2] == 0).all()), "a gap equal to min_gap * s1 must be dropped"
    assert float(host(A, term_12(U, V), float(np.nextafter(at, 0.0)))[2].abs().max()) == 2.0 ** 28
    # the 1.19e-8 pair with the cut set to its own ratio, where that product is exact
    A = exact_3x3((0.625, 0.5, -0.5 * (1.0 - 2.0 ** -26)))
    _, s, _, _, U, V = host(A, gR)
    own = 2.0 ** -27 / 0.625
    if own * 0.625 == 2.0 ** -27:
        assert bool((host(A, term_12(U, V), own)[2] == 0).all())
    # random frames on the dropped side: the term is absent up to the frames' own orthogonality
    A, gR64, _ = rc.host_classes()["gap 5e-9 (dropped)"]
    _, _, _, _, U, V = host(A, gR64)
    assert float(host(A, term_12(U, V))[2].abs().max()) <= 1e-12
    A, gR64, _ = rc.host_classes()["gap 2e-8 (kept)"]
    _, _, _, _, U, V = host(A, gR64)
    assert float(host(A, term_12(U, V))[2].flatten(1).norm(dim=1).min()) >= 0.5e8


def test_no_frames_and_arbitrary_frames(host):
    gR = torch.randn(4, 3, 3, generator=rc.gen(7001), dtype=torch.float64)
    A = torch.zeros(4, 3, 3, dtype=torch.float64)
    A[1:] = rc.framed((1.0, 0.5, 0.25), 7002)[0][:3]
    A[2, 1, 2], A[3, 0, 0] = float("nan"), float("inf")
    has, s, gA, R, U, V = host(A, gR)
    assert has.tolist() == [False, True, False, False]
    assert all(torch.equal(R[k], torch.eye(3, dtype=torch.float64)) for k in (0, 2, 3)) and bool((gA[[0, 2, 3]] == 0).all())
    # rank 1 and an exact gap of 0: the frames are arbitrary there, and so are torch's: finite output is all there is to ask
    line = torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64)
    A = torch.stack([line[:, None] * torch.tensor([0.5, -1.0, 3.0], dtype=torch.float64)[None, :], exact_3x3(rc.GAP_ZERO)[0]])
    has, s, gA, R, U, V = host(A, gR[:2])
    assert bool(has.all()) and all(bool(torch.isfinite(t).all()) for t in (s, gA, R, U, V))
    assert bool((host(A[1:], term_12(U[1:], V[1:]))[2] == 0).all())
