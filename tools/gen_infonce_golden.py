"""Regenerate tests/golden/g13_infonce.npz: inputs and outputs of the reference's own `MyInfoNCELossNoSeg` (loss.py:10-46),
run on the CPU from the reference tree with MinkowskiEngine and pytorch3d replaced by the placeholders of
oracle/gen_golden.py.  Only data goes into the file: per case the two feature tensors, the source points, the matches, the
loss, and its gradients with respect to both feature tensors.

    python tools/gen_infonce_golden.py [out.npz]

Two cases: `far` -- anchors on a 12 m lattice, every pair farther apart than neg_euclid_dist = 5, so every other positive is
a negative; `near` -- anchors inside a 20 m box, so that about a tenth of the pairs are closer than 5 m and the mask
matters."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "g13_infonce.npz")
TAU, NEG_DIST = 0.1, 5


def unit_rows(rng, n, d=32):
    f = rng.standard_normal((n, d))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def case(rng, kind, n_src=700, n_tgt=650, n_match=200):
    if kind == "far":
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
        pts = (g * 12.0 + rng.uniform(-1, 1, g.shape)).astype(np.float32)
    else:
        pts = rng.uniform(-10, 10, (n_src, 3)).astype(np.float32)
    src = unit_rows(rng, n_src)
    tgt = unit_rows(rng, n_tgt)
    m = np.stack([rng.choice(n_src, n_match, replace=False), rng.choice(n_tgt, n_match, replace=False)], 1).astype(np.int64)
    # correlated positives, as a half-trained network would give
    tgt[m[:, 1]] = src[m[:, 0]] + 0.5 * unit_rows(rng, n_match)
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    return src[None], pts[None], tgt[None], m[None]


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    from oracle import gen_golden
    gen_golden.import_reference()
    import loss as ref_loss        # the reference's loss.py
    fn = ref_loss.MyInfoNCELossNoSeg(tau=TAU, neg_euclid_dist=NEG_DIST)
    rng = np.random.default_rng(13)
    data = {"tau": np.float64(TAU), "neg_euclid_dist": np.float64(NEG_DIST)}
    for kind in ("far", "near"):
        src, pts, tgt, m = case(rng, kind)
        a, b = torch.from_numpy(src).requires_grad_(), torch.from_numpy(tgt).requires_grad_()
        val = fn(a, torch.from_numpy(pts), b, torch.from_numpy(m))
        val.backward()
        anchors = pts[0][m[0, :, 0]]
        dist = np.linalg.norm(anchors[:, None] - anchors[None], axis=-1)
        close = int(((dist <= NEG_DIST).sum() - len(anchors)) // 2)
        print(f"{kind}: loss {float(val.detach()):.6f}, anchor pairs within {NEG_DIST}: {close}")
        assert (close == 0) == (kind == "far")
        data.update({f"{kind}_src_feat": src, f"{kind}_src_pts": pts, f"{kind}_tgt_feat": tgt, f"{kind}_matches": m,
                     f"{kind}_loss": val.detach().numpy(), f"{kind}_grad_src": a.grad.numpy(), f"{kind}_grad_tgt": b.grad.numpy()})
    np.savez_compressed(out, **data)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv)
