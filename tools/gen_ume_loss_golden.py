"""Regenerate tests/golden/g14_ume_contrastive.npz: inputs and outputs of the reference's own `UMEContrastiveLoss`
(loss.py:49-118), run on the CPU from the reference tree with MinkowskiEngine and pytorch3d replaced by the placeholders of
oracle/gen_golden.py.  Only data goes into the file: the inputs, the seven outputs, the gradients of the loss with respect to
both feature tensors, and the neighbour lists of the selected keypoints (the placeholder ball query on the keypoints the
reference returned -- the same call the reference makes).

    python tools/gen_ume_loss_golden.py [out.npz]

One case: a batch of two, 1000 source and 1100 target points in a flat 16 x 16 x 4 box, the target a rotated, shifted, noisy
copy of 80 % of the source plus unrelated points; features a smooth positive function of position plus noise (a half-trained
network: matched neighbourhoods are close, others are not).  The reference runs in fp32 only (the ball-query placeholder
returns fp32).  Preconditions asserted here, so that a regenerated case stays away from the D = 0 convention and from the
validity mask: every selected keypoint valid in both clouds, min D >= 0.05."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "g14_ume_contrastive.npz")
CFG = dict(num_samples=48, max_nn=48, min_nn=16, nn_r=2.5, tau=0.1, tau_neg=0.1, nn_intersection_r=0.6, svd_thr=1e-5)
FLAT_LABELS = [9]
MAX_BYTES = 1 << 20       # no committed file above 1 MiB


def case(rng, N=1000, M=1100):
    src = rng.uniform(-8, 8, (N, 3))
    src[:, 2] *= 0.25
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    t = np.array([1.5, -0.7, 0.2])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    keep = rng.random(N) < 0.8
    tgt = np.concatenate([src[keep] @ R.T + t + rng.normal(0, 0.03, (keep.sum(), 3)),
                          rng.uniform(-8, 8, (M - keep.sum(), 3)) * [1, 1, .25]])
    tgt = tgt[rng.permutation(M)]
    W = rng.normal(0, 1, (3, 32))
    f = lambda p: (1 + np.sin(p @ W * 0.35 + np.arange(32))) * 0.5 + 0.05      # noqa: E731
    sf = f(src) + rng.normal(0, .02, (N, 32))
    tf = f((tgt - t) @ R) + rng.normal(0, .02, (M, 32))
    seg = rng.integers(0, 12, (N, 1))
    return src.astype(np.float32), seg, sf.astype(np.float32), tgt.astype(np.float32), tf.astype(np.float32), T.astype(np.float32)


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    from oracle import gen_golden
    loc_utils, _, _ = gen_golden.import_reference()
    import loss as ref_loss        # the reference's loss.py
    from pytorch3d.ops import ball_query        # the placeholder the reference ran on
    rng = np.random.default_rng(14)
    cs = [case(rng), case(rng)]
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cs]))      # noqa: E731
    velo_pts, velo_seg, ref_pts, gt = st(0), st(1), st(3), st(5)
    velo_feat, ref_feat = st(2).requires_grad_(), st(4).requires_grad_()
    fn = ref_loss.UMEContrastiveLoss(flat_labels=FLAT_LABELS, **CFG)
    res = fn(velo_pts, velo_seg, velo_feat, ref_pts, ref_feat, gt)
    loss, velo_kp, ref_kp, velo_ume, ref_ume, ratio, with_kpts = res
    loss.backward()
    with torch.no_grad():
        D = loc_utils.ume_cdist(velo_ume, ref_ume)
        sv = torch.minimum(torch.linalg.svdvals(velo_ume).min(), torch.linalg.svdvals(ref_ume).min())
        velo_nn = ball_query(velo_kp, velo_pts, K=CFG["max_nn"], radius=CFG["nn_r"], return_nn=False).idx
        ref_nn = ball_query(ref_kp, ref_pts, K=CFG["max_nn"], radius=CFG["nn_r"], return_nn=False).idx
    diag = D.diagonal(dim1=-1, dim2=-2)
    print(f"loss {float(loss.detach()):.6f}; keypoints {tuple(velo_ume.shape)}; with_kpts {with_kpts.tolist()}; smallest singular value "
          f"{float(sv):.2e}; D diagonal {float(diag.min()):.3f} .. {float(diag.max()):.3f}, min D {float(D.min()):.3f}; "
          f"ratio mean {float(ratio.mean()):.3f}")
    assert bool(with_kpts.all()) and velo_ume.shape[1] == CFG["num_samples"], "a keypoint was dropped (batch element or validity mask)"
    assert float(sv) > 10 * CFG["svd_thr"], "a UME matrix is close to the validity threshold"
    assert float(D.min()) >= 0.05, "a pair is close to D = 0"
    assert float(velo_feat.grad.abs().max()) > 0 and float(ref_feat.grad.abs().max()) > 0
    data = {f"cfg_{k}": np.float64(v) for k, v in CFG.items()}
    data.update(cfg_flat_labels=np.asarray(FLAT_LABELS, dtype=np.int64),
                velo_pts=velo_pts.numpy(), velo_seg=velo_seg.numpy(), velo_feat=velo_feat.detach().numpy(), ref_pts=ref_pts.numpy(),
                ref_feat=ref_feat.detach().numpy(), gt_tform=gt.numpy(),
                loss=loss.detach().numpy(), velo_kp=velo_kp.numpy(), ref_kp=ref_kp.numpy(), velo_ume=velo_ume.detach().numpy(),
                ref_ume=ref_ume.detach().numpy(), ratio=ratio.numpy(), with_kpts=with_kpts.numpy(),
                grad_velo_feat=velo_feat.grad.numpy(), grad_ref_feat=ref_feat.grad.numpy(),
                velo_nn_idx=velo_nn.numpy().astype(np.int32), ref_nn_idx=ref_nn.numpy().astype(np.int32))
    # an .npz is a zip of .npy members; LZMA members (numpy.load reads them like deflated ones) keep this one under MAX_BYTES
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
