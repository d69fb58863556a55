"""Regenerate tests/golden/g15_cube_registration.npz: outputs of the reference's own `CubeRegistrationLoss` (loss.py:121-190), run on
the CPU from the reference tree with MinkowskiEngine and pytorch3d replaced by the placeholders of oracle/gen_golden.py.  Only
data goes into the file.

    python tools/gen_cube_loss_golden.py [out.npz]

The inputs are what the reference's `UMEContrastiveLoss` returned on the case of tests/golden/g14_ume_contrastive.npz (the trainer
feeds one loss from the other, train_coloring.py:50-58): its UME matrices, keypoints, intersection ratio, batch mask and
`gt_tform`.  They are read from that file and not stored again.  The class runs twice: with `nn_inter_ratio_thr` = 0.75 (the main
branch: some keypoints reach it) and 0.99 (no keypoint reaches it: the fall-back to the per-row median).  Stored per run: `loss`,
`rre`, `rte` and the gradients of the loss with respect to both UME tensors.  The reference runs in fp32 only (`torch.eye`
without a dtype)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SOURCE = os.path.join(REPO, "tests", "golden", "g14_ume_contrastive.npz")
DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "g15_cube_registration.npz")
CFG = dict(rtume_max_nn=48, rtume_r_nn=2.5, cube_scale=1.0)
THRESHOLDS = {"main": 0.75, "median": 0.99}
MAX_BYTES = 1 << 20       # no committed file above 1 MiB


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    from oracle import gen_golden
    gen_golden.import_reference()
    import loss as ref_loss        # the reference's loss.py
    g = np.load(SOURCE)
    t = lambda k: torch.from_numpy(g[k])      # noqa: E731
    ratio, with_kpts, gt = t("ratio"), t("with_kpts"), t("gt_tform")
    data = {f"cfg_{k}": np.float64(v) for k, v in CFG.items()}
    for name, thr in THRESHOLDS.items():
        src_ume, tgt_ume = t("velo_ume").clone().requires_grad_(), t("ref_ume").clone().requires_grad_()
        fn = ref_loss.CubeRegistrationLoss(nn_inter_ratio_thr=thr, **CFG)
        loss, rre, rte = fn(t("velo_kp"), src_ume, t("ref_kp"), tgt_ume, gt, ratio, with_kpts)
        loss.backward()
        passed = int((ratio >= thr).sum())
        print(f"[{name}] thr {thr}: {passed} of {ratio.numel()} keypoints reach it (largest ratio {float(ratio.max()):.3f}); loss "
              f"{float(loss.detach()):.5f}; rre {float(rre.min()):.2f} .. {float(rre.max()):.2f} deg; rte {float(rte.min()):.3f} .. "
              f"{float(rte.max()):.3f}; max |grad| {float(src_ume.grad.abs().max()):.3g} / {float(tgt_ume.grad.abs().max()):.3g}")
        assert (passed > 0) == (name == "main"), "the threshold does not take the branch it is named after"
        assert all(bool(torch.isfinite(x).all()) for x in (loss, rre, rte, src_ume.grad, tgt_ume.grad))
        assert float(src_ume.grad.abs().max()) > 0 and float(tgt_ume.grad.abs().max()) > 0
        data.update({f"{name}_thr": np.float64(thr), f"{name}_loss": loss.detach().numpy(), f"{name}_rre": rre.numpy(),
                     f"{name}_rte": rte.numpy(), f"{name}_grad_src_ume": src_ume.grad.numpy(),
                     f"{name}_grad_tgt_ume": tgt_ume.grad.numpy()})
    with zipfile.ZipFile(out, "w", zipfile.ZIP_LZMA) as z:
        for k, v in data.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asarray(v), allow_pickle=False)
            z.writestr(k + ".npy", b.getvalue())
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes")
    assert size <= MAX_BYTES, "the fixture outgrew the size limit of a committed file"


if __name__ == "__main__":
    main(sys.argv)
