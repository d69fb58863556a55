"""CPU: the ground the UME contrastive loss stands on -- the host side of include/umereg_ume_grad.h, the refusals of the new
Python entry points without a GPU, the signature of `ume_loss.UMEContrastiveLoss`, and the fp64 / fp32 restatement
(tests/ume_grad_ref.py) against the reference's own class (tests/golden/g14_ume_contrastive.npz, tools/gen_ume_loss_golden.py)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ume_grad_ref as uref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "g14_ume_contrastive.npz")


# ---- 1. the C ABI's host side -----------------------------------------------------------------------------------------------

def test_ume_grad_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import ume_grad
    syms = ["umereg_ume_cdist_bwd_f32", "umereg_ume_cdist_bwd_scratch_bytes", "umereg_ume_moments_bwd_f32",
            "umereg_ume_moments_bwd_scratch_bytes"]
    assert sorted(ume_grad.UME_GRAD_SIGNATURES) == syms
    umereg_h = open(os.path.join(REPO, "include", "umereg.h")).read()
    assert "ume_grad" not in umereg_h and not any(s in umereg_h for s in syms)
    # the constants the Python side repeats
    text = open(os.path.join(REPO, "include", "umereg_ume_grad.h")).read()
    assert float(re.search(r"#define UMEREG_UME_CDIST_BWD_DMIN (\S+?)f?\n", text).group(1)) == ume_grad.D_MIN
    assert int(re.search(r"#define UMEREG_UME_GRAD_MAX_K (\d+)", text).group(1)) == ume_grad.MAX_K


def test_scratch_sizes_are_host_arithmetic():
    from umeregrobust_amd import ume_grad
    lib = ume_grad.load_native()
    mom, cd = lib.umereg_ume_moments_bwd_scratch_bytes, lib.umereg_ume_cdist_bwd_scratch_bytes
    for B, N, n in ((1, 1, 1), (2, 1000, 48), (8, 50000, 256), (1, 50000, 4096), (1, 200000, 10000)):
        s = mom(B, N, n)
        # one fp64 per point, one fp64 [32][4] and eight words (length, bounding box) per keypoint, plus alignment
        assert B * N * 8 + B * n * (128 * 8 + 32) <= s <= B * N * 8 + B * n * (128 * 8 + 32) + 3 * 256
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 10, 10), (70000, 70000, 1)):
        assert mom(*bad) == 0
    for n1, n2 in ((1, 1), (48, 48), (257, 130), (2048, 1536), (10000, 10000), (1, 10000), (10000, 1)):
        s = cd(n1, n2)
        assert s > 0 and s % 256 == 0
        assert s >= (n1 + n2) * 128 * (4 + 4 + 8) + max(n1, n2) * 128 * 4
        assert cd(n1, n2) == s
    # the partial sums of the largest case stay far below the 16 n1 n2 floats of the intermediate that is never formed
    assert cd(10000, 10000) <= 128 << 20
    for bad in ((0, 5), (5, 0), (-3, 5), (1 << 23, 5)):
        assert cd(*bad) == 0


def test_ume_grad_entry_points_check_arguments_and_need_a_device():
    from umeregrobust_amd import ume_grad
    lib = ume_grad.load_native()
    buf = np.zeros(1 << 18, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    m_bytes = lib.umereg_ume_moments_bwd_scratch_bytes(1, 8, 2)
    c_bytes = lib.umereg_ume_cdist_bwd_scratch_bytes(3, 2)
    assert 0 < m_bytes < 1 << 19 and 0 < c_bytes < 1 << 19
    mom = lambda **kw: lib.umereg_ume_moments_bwd_f32(*[kw.get(k, d) for k, d in (          # noqa: E731
        ("pts", p), ("feat", p), ("nn_idx", p), ("F", p), ("dF", p), ("B", 1), ("N", 8), ("n", 2), ("K", 4), ("normalize", 1), ("dfeat", p),
        ("scratch", p), ("scratch_bytes", m_bytes), ("stream", None))])
    cd = lambda **kw: lib.umereg_ume_cdist_bwd_f32(*[kw.get(k, d) for k, d in (             # noqa: E731
        ("ume1", p), ("ume2", p), ("D", p), ("dD", p), ("n1", 3), ("n2", 2), ("dume1", p), ("dume2", p), ("scratch", p),
        ("scratch_bytes", c_bytes), ("stream", None))])
    # argument errors come before the device probe
    for k in ("pts", "feat", "nn_idx", "F", "dF", "dfeat", "scratch"):
        assert mom(**{k: None}) == -1, k
        assert b"null" in lib.umereg_last_error()
    for kw in (dict(B=0), dict(N=0), dict(n=0), dict(K=0), dict(K=7681), dict(scratch_bytes=m_bytes - 1), dict(scratch=p + 8),
               dict(feat=p + 4), dict(B=70000, N=70000)):
        assert mom(**kw) == -1, kw
    for k in ("ume1", "ume2", "D", "dD", "scratch"):
        assert cd(**{k: None}) == -1, k
        assert b"null" in lib.umereg_last_error()
    assert cd(dume1=None, dume2=None) == -1
    for kw in (dict(n1=0), dict(n2=0), dict(n1=-4), dict(scratch_bytes=c_bytes - 1), dict(scratch=p + 16), dict(ume1=p + 4), dict(dume2=p + 8)):
        assert cd(**kw) == -1, kw
    if lib.umereg_device_count(None, 0) == 0:
        assert mom() == -2                                                              # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        assert mom(normalize=0, feat=None, F=None) == -2
        assert cd() == -2 and cd(dume1=None) == -2 and cd(dume2=None) == -2


# ---- 2. the Python surface without a GPU ------------------------------------------------------------------------------------

def test_python_entry_points_refuse_cpu_tensors():
    from umeregrobust_amd import ume_grad, ume_loss
    pts, feat = torch.zeros(1, 8, 3), torch.ones(1, 8, 32, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ume_grad.ume_moments(pts, pts[:, :2], feat, 4, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ume_grad.ume_cdist(torch.ones(1, 2, 32, 4), torch.ones(1, 3, 32, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ume_grad.moments_bwd_raw(pts, feat, torch.zeros(1, 2, 4, dtype=torch.int64), torch.ones(1, 2, 32, 4), torch.ones(1, 2, 32, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ume_grad.cdist_bwd_raw(torch.ones(1, 2, 32, 4), torch.ones(1, 3, 32, 4), torch.ones(1, 2, 3), torch.ones(1, 2, 3))
    fn = ume_loss.UMEContrastiveLoss(num_samples=2, max_nn=4, min_nn=1, nn_r=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(pts, torch.zeros(1, 8, 1, dtype=torch.int64), feat, pts, feat, torch.eye(4)[None])


def test_loss_signature_is_the_reference_s_and_the_stub_still_refuses():
    from umeregrobust_amd import loss, ume_loss
    sig = inspect.signature(ume_loss.UMEContrastiveLoss.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("num_samples", 1024), ("max_nn", 5000), ("min_nn", 1000), ("nn_r", 10), ("tau", 0.1), ("tau_neg", 0.1), ("hd_labels_flag", False),
        ("flat_labels", []), ("nn_intersection_r", 0.6), ("svd_thr", 1e-5)]
    assert list(inspect.signature(ume_loss.UMEContrastiveLoss.forward).parameters)[1:] == [
        "velo_pts", "velo_seg", "velo_feat", "ref_pts", "ref_feat", "gt_tform"]
    fn = ume_loss.UMEContrastiveLoss()
    assert (fn.n_samples, fn.max_nn, fn.min_nn, fn.nn_r, fn.tau, fn.tau_neg, fn.svd_thr) == (1024, 5000, 1000, 10, 0.1, 0.1, 1e-5)
    with pytest.raises(NotImplementedError, match="out of scope"):
        loss.UMEContrastiveLoss()


# ---- 3. the restatement against the reference's own class ---------------------------------------------------------------

def fixture(dtype):
    g = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(g[k]).to(dtype)          # noqa: E731
    return g, (t("velo_pts"), t("velo_feat"), torch.from_numpy(g["velo_nn_idx"]).long(), t("ref_pts"), t("ref_feat"),
               torch.from_numpy(g["ref_nn_idx"]).long())


def test_fixture_is_the_case_it_claims_to_be():
    g, args = fixture(torch.float64)
    assert os.path.getsize(GOLDEN) <= 1 << 20
    assert g["velo_feat"].dtype == np.float32 and g["velo_ume"].shape == (2, 48, 32, 4) and bool(g["with_kpts"].all())
    D = uref.ume_cdist(torch.from_numpy(g["velo_ume"]).double(), torch.from_numpy(g["ref_ume"]).double())
    sv = min(float(torch.linalg.svdvals(torch.from_numpy(g[k]).double()).min()) for k in ("velo_ume", "ref_ume"))
    print(f"[g14] loss {float(g['loss']):.6f}  min D {float(D.min()):.4f}  smallest singular value {sv:.2e}")
    assert float(D.min()) >= 0.05 and sv > 10 * float(g["cfg_svd_thr"])
    # the recorded neighbour lists are the lists of the recorded keypoints: every listed point lies inside the ball
    for pts, kp, nn in ((g["velo_pts"], g["velo_kp"], g["velo_nn_idx"]), (g["ref_pts"], g["ref_kp"], g["ref_nn_idx"])):
        for b in range(2):
            d = np.linalg.norm(pts[b][np.maximum(nn[b], 0)] - kp[b][:, None], axis=-1)
            assert (d[nn[b] >= 0] < float(g["cfg_nn_r"])).all() and ((nn[b] >= 0).sum(-1) >= 1).all()
    assert ((g["velo_nn_idx"] >= 0).sum(-1) >= int(g["cfg_min_nn"])).all()          # (the density condition is on the source lists)


def test_fp32_restatement_reproduces_the_reference():
    """The helper in fp32, on the fixture's own neighbour lists, against the reference's fp32 run.  The two numbers
    test_infonce_equals_the_reference_s uses (loss within 1e-6 relative, gradients within 1e-5 of their largest entry) are not
    reachable on this case by ANY two fp32 evaluations: the helper's own fp32 run differs from its fp64 run by 1e-6 relative
    in the loss and by 9e-5 / 1.1e-4 of the largest entry in the gradients (QR of matrices with cond ~ 1e3 and a cdist over
    projector entries), and the reference's fp32 run is as far from fp64 (5e-5 / 6e-5).  So the bound is 4 x the helper's
    own fp32 error against its fp64 run, per quantity; the moment matrices, which are well conditioned, keep 1e-6."""
    g, a32 = fixture(torch.float32)
    _, a64 = fixture(torch.float64)
    tau, tau_neg = float(g["cfg_tau"]), float(g["cfg_tau_neg"])
    loss, gv, gr, vu, ru = uref.loss_and_grads(*a32, tau=tau, tau_neg=tau_neg)
    loss64, gv64, gr64, _, _ = uref.loss_and_grads(*a64, tau=tau, tau_neg=tau_neg)
    want = float(g["loss"])
    e_loss = abs(float(loss) - float(loss64))
    print(f"[g14] loss: helper fp32 {float(loss):.8f}  reference {want:.8f}  helper fp64 {float(loss64):.8f}")
    for got, name in ((vu, "velo_ume"), (ru, "ref_ume")):
        assert np.abs(got.numpy() - g[name]).max() <= 1e-6 * np.abs(g[name]).max(), name
    assert e_loss > 0 and abs(float(loss) - want) <= 4 * e_loss
    assert abs(want - float(loss64)) <= 4 * e_loss
    for got, g64, name in ((gv, gv64, "grad_velo_feat"), (gr, gr64, "grad_ref_feat")):
        w = g[name]
        scale = np.abs(w).max()
        e32 = float((got.double() - g64).abs().max())
        d_ref = np.abs(got.numpy() - w).max()
        print(f"[g14] {name}: max|helper32 - reference| {d_ref / scale:.3e}  max|helper32 - helper64| {e32 / scale:.3e}  "
              f"max|reference - helper64| {float((torch.from_numpy(w).double() - g64).abs().max()) / scale:.3e}  (of max|reference|)")
        assert scale > 0 and e32 > 0
        assert d_ref <= 4 * e32, name
        assert float((torch.from_numpy(w).double() - g64).abs().max()) <= 4 * e32, name
