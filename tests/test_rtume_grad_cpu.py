"""CPU: the ground `cube_loss.CubeRegistrationLoss` stands on -- the host side of include/umereg_rtume_grad.h, the refusals of the
new Python entry points without a GPU, the signatures of the working class, and the fp32 / fp64 restatement
(tests/cube_loss_ref.py) against the reference's own class (tests/golden/g15_cube_registration.npz,
tools/gen_cube_loss_golden.py)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cube_loss_ref as cref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = os.path.join(REPO, "tests", "golden", "g14_ume_contrastive.npz")
G15 = os.path.join(REPO, "tests", "golden", "g15_cube_registration.npz")
HEADER = os.path.join(REPO, "include", "umereg_rtume_grad.h")


# ---- 1. the C ABI's host side -----------------------------------------------------------------------------------------------

def test_rtume_grad_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import rtume_grad
    syms = ["umereg_rtume_solve_bwd_f32"]
    assert sorted(rtume_grad.RTUME_GRAD_SIGNATURES) == syms
    umereg_h = open(os.path.join(REPO, "include", "umereg.h")).read()
    assert "rtume_grad" not in umereg_h and not any(s in umereg_h for s in syms)
    # the constant the Python side repeats, and the convention written next to it
    text = open(HEADER).read()
    assert float(re.search(r"#define UMEREG_RTUME_BWD_MIN_GAP (\S+)\n", text).group(1)) == rtume_grad.MIN_GAP == 1e-8
    before = text[:text.index("#define UMEREG_RTUME_BWD_MIN_GAP")]
    assert "contributes nothing" in before[before.rindex("/*"):]


def test_rtume_grad_entry_checks_arguments_and_needs_a_device():
    from umeregrobust_amd import rtume_grad
    lib = rtume_grad.load_native()
    buf = np.zeros(1 << 12, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    bwd = lambda **kw: lib.umereg_rtume_solve_bwd_f32(*[kw.get(k, d) for k, d in (          # noqa: E731
        ("G", p), ("H", p), ("dT", p), ("n", 3), ("dG", p), ("dH", p), ("stream", None))])
    # argument errors come before the device probe
    for k in ("G", "H", "dT"):
        assert bwd(**{k: None}) == -1, k
        assert b"null" in lib.umereg_last_error()
    assert bwd(dG=None, dH=None) == -1
    for kw in (dict(n=0), dict(n=-5), dict(G=p + 4), dict(H=p + 8), dict(dG=p + 4), dict(dH=p + 12), dict(dG=None, dH=p + 8)):
        assert bwd(**kw) == -1, kw
    if lib.umereg_device_count(None, 0) == 0:
        assert bwd() == -2                                                              # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        assert bwd(dG=None) == -2 and bwd(dH=None) == -2


# ---- 2. the Python surface without a GPU ------------------------------------------------------------------------------------

def test_python_entry_points_refuse_cpu_tensors():
    from umeregrobust_amd import cube_loss, rtume_grad
    G, H = torch.ones(2, 32, 4, requires_grad=True), torch.ones(2, 32, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rtume_grad.rtume_solve(G, H)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rtume_grad.rtume_bwd_raw(G, H, torch.ones(2, 4, 4))
    fn = cube_loss.CubeRegistrationLoss(4, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(torch.zeros(1, 2, 3), G[None], torch.zeros(1, 2, 3), H[None], torch.eye(4)[None], torch.ones(1, 2), torch.ones(1, dtype=torch.bool))


def test_loss_signature_is_the_reference_s_and_the_stub_still_refuses():
    from umeregrobust_amd import cube_loss, loss
    sig = inspect.signature(cube_loss.CubeRegistrationLoss.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("rtume_max_nn", inspect.Parameter.empty), ("rtume_r_nn", inspect.Parameter.empty), ("cube_scale", 1.0), ("nn_inter_ratio_thr", 0.75)]
    assert list(inspect.signature(cube_loss.CubeRegistrationLoss.forward).parameters)[1:] == [
        "src_pts", "src_ume", "tgt_pts", "tgt_ume", "gt_tform", "matched_nn_intersection_ratio", "valid_batch_entries"]
    fn = cube_loss.CubeRegistrationLoss(750, 5, cube_scale=2.0)
    assert fn.nn_inter_ratio_thr == 0.75 and fn.points_cube.shape == (8, 3)
    assert torch.equal(fn.points_cube, torch.tensor(cref.CUBE).float() * 2.0)
    with pytest.raises(NotImplementedError, match="out of scope.*cube_loss"):
        loss.CubeRegistrationLoss()


# ---- 3. the restatement against the reference's own class, and against itself -----------------------------------------------

def fixture(dtype):
    g14, g15 = np.load(G14), np.load(G15)
    return g15, (torch.from_numpy(g14["velo_ume"]).to(dtype), torch.from_numpy(g14["ref_ume"]).to(dtype),
                 torch.from_numpy(g14["gt_tform"]).to(dtype), torch.from_numpy(g14["ratio"]), torch.from_numpy(g14["with_kpts"]))


def test_fixture_is_the_case_it_claims_to_be():
    g15, args = fixture(torch.float64)
    assert os.path.getsize(G15) <= 1 << 20
    ratio = args[3]
    assert ratio.shape == (2, 48) and float(g15["main_thr"]) == 0.75 and float(g15["median_thr"]) == 0.99
    assert int((ratio >= 0.75).sum()) == 61 and int((ratio >= 0.99).sum()) == 0          # the main branch / the median fall-back
    cond, thin, flips = cref.conditioning(args[0].flatten(0, 1), args[1].flatten(0, 1))
    print(f"[g15] max s1 / (s2 + d s3) {cond:.2f}  max s1 / s3 {thin:.1f}  d = -1: {flips}")
    assert cond <= 20
    for name in ("main", "median"):
        assert g15[f"{name}_rre"].shape == g15[f"{name}_rte"].shape == (2, 48) and g15[f"{name}_grad_src_ume"].shape == (2, 48, 32, 4)


@pytest.mark.parametrize("name", ["main", "median"])
def test_fp32_restatement_reproduces_the_reference(name):
    """The helper in fp32 against the reference's fp32 run, in the form of test_ume_grad_cpu: neither fp32 evaluation is the
    truth, so every quantity is bounded by 4 x the helper's own fp32 error against its fp64 run, and so is the reference's
    distance to fp64."""
    g15, a32 = fixture(torch.float32)
    _, a64 = fixture(torch.float64)
    thr = float(g15[f"{name}_thr"])
    scale = float(g15["cfg_cube_scale"])
    got = cref.loss_and_grads(*a32, cube_scale=scale, thr=thr)
    truth = cref.loss_and_grads(*a64, cube_scale=scale, thr=thr)
    for x, t64, key in zip(got, truth, ("loss", "rre", "rte", "grad_src_ume", "grad_tgt_ume")):
        w = torch.from_numpy(g15[f"{name}_{key}"]).double()
        e32 = float((x.double() - t64).abs().max())
        d_ref = float((x.double() - w).abs().max())
        e_ref = float((w - t64).abs().max())
        print(f"[g15 {name}] {key}: max|helper32 - reference| {d_ref:.3e}  max|helper32 - helper64| {e32:.3e}  "
              f"max|reference - helper64| {e_ref:.3e}  (max|reference| {float(w.abs().max()):.3e})")
        assert e32 > 0 and d_ref <= 4 * e32 and e_ref <= 4 * e32, key


@pytest.mark.parametrize("thin", [False, True])
def test_closed_form_backward_equals_fp64_autograd(thin):
    """The chain written out by hand (the formula the kernel implements) against autograd through torch's SVD, in fp64: 1e-12 of
    the largest entry.  Both evaluate the same function in the same precision; autograd's 1 / (s_i^2 - s_j^2) terms lose
    s1^2 / (s_i^2 - s_j^2) ~ 1e2 of 2e-16 on these spectra, and the sums over 32 rows another 1e1."""
    G, H, dT = cref.ume_pairs(257, 7 + int(thin), thin=thin)
    cond, ratio, flips = cref.conditioning(G, H)
    print(f"[closed form] thin={thin}: max s1 / (s2 + d s3) {cond:.2f}  max s1 / s3 {ratio:.3g}  d = -1: {flips}")
    assert cond <= 20 and (not thin or (ratio >= 1e5 and flips > 0))
    _, a, b = cref.solve_grads(G.double(), H.double(), dT.double())
    ca, cb = cref.solve_grads_closed_form(G.double(), H.double(), dT.double(), min_gap=1e-8)
    for got, want, name in ((ca, a, "dG"), (cb, b, "dH")):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"[closed form] thin={thin} {name}: {err:.3e} of max|autograd|")
        assert err <= 1e-12
