"""Time the point-wise InfoNCE loss, torch class against fused class, on the same inputs in one process; one JSON line per shape.

    python tools/infonce_time.py [--out profiles/infonce/infonce_time.jsonl] [--iters 20] [--warmup 5]

Shapes (B, S): (8, 512) -- the training config; (8, 2048) -- the class's default num_samples; (2, 8192) -- the largest S the fused
kernels take; N = M = 45 000 points per cloud.  For `loss.MyInfoNCELossNoSeg` (torch) and `pw_loss.MyInfoNCELossNoSeg` (fused):

  * `fwd_ms`: the forward alone under torch.no_grad();
  * `fwd_bwd_ms`: forward + backward to both feature tensors;
  * `fwd_peak_mib`, `fwd_bwd_peak_mib`: torch.cuda.max_memory_allocated over one such call, above what was allocated before it.

Every time is the median over `--iters` calls, each bracketed by its own pair of device events on the launch stream, after `--warmup`
calls of the same shape.  Anchors lie in a 100 x 100 x 8 m box (most pairs are farther apart than neg_euclid_dist = 5, as in a scan);
features are unit rows with correlated positives."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from umeregrobust_amd.loss import MyInfoNCELossNoSeg as TorchLoss          # noqa: E402
from umeregrobust_amd.pw_loss import MyInfoNCELossNoSeg as FusedLoss       # noqa: E402

SHAPES = ((8, 512), (8, 2048), (2, 8192))
POINTS = 45000
TAU, NEG_DIST = 0.1, 5


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def inputs(dev, B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)       # noqa: E731
    src, tgt = unit(B, POINTS, 32), unit(B, POINTS, 32)
    pts = torch.rand(B, POINTS, 3, generator=g) * torch.tensor([100.0, 100.0, 8.0])
    m = torch.stack([torch.stack([torch.randperm(POINTS, generator=g)[:S], torch.randperm(POINTS, generator=g)[:S]], 1) for _ in range(B)])
    for b in range(B):
        tgt[b, m[b, :, 1]] = torch.nn.functional.normalize(src[b, m[b, :, 0]] + 0.5 * unit(S, 32), dim=-1)
    return src.to(dev), pts.to(dev), tgt.to(dev), m.to(dev)


def measure(fn, src, pts, tgt, m, iters, warmup):
    def fwd():
        with torch.no_grad():
            return fn(src, pts, tgt, m)

    def fwd_bwd():
        a, b = src.detach().requires_grad_(), tgt.detach().requires_grad_()
        loss = fn(a, pts, b, m)
        loss.backward()
        return loss.detach(), a.grad, b.grad

    out = {"fwd_ms": median_ms(fwd, iters, warmup), "fwd_bwd_ms": median_ms(fwd_bwd, iters, warmup),
           "fwd_peak_mib": peak_mib(fwd), "fwd_bwd_peak_mib": peak_mib(fwd_bwd)}
    return out, fwd_bwd()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "infonce",
                                                  "infonce_time.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infonce_time: no HIP device visible; a time is a measurement on the GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for B, S in SHAPES:
            src, pts, tgt, m = inputs(dev, B, S)
            line = dict(B=B, S=S, N=POINTS, M=POINTS, tau=TAU, neg_euclid_dist=NEG_DIST, iters=args.iters, warmup=args.warmup)
            res = {}
            for name, cls in (("torch", TorchLoss), ("fused", FusedLoss)):
                try:
                    line[name], res[name] = measure(cls(tau=TAU, neg_euclid_dist=NEG_DIST), src, pts, tgt, m, args.iters, args.warmup)
                except RuntimeError as e:       # (out of memory): reported, not hidden
                    line[name] = {"error": str(e).splitlines()[0][:200]}
                torch.cuda.empty_cache()
            if len(res) == 2:
                (lt, at, bt), (lf, af, bf) = res["torch"], res["fused"]
                line["loss_torch"], line["loss_fused"] = float(lt), float(lf)
                line["grad_src_rel_diff"] = float((af - at).abs().max() / at.abs().max())
                line["grad_tgt_rel_diff"] = float((bf - bt).abs().max() / bt.abs().max())
                line["speedup_fwd"] = line["torch"]["fwd_ms"] / line["fused"]["fwd_ms"]
                line["speedup_fwd_bwd"] = line["torch"]["fwd_bwd_ms"] / line["fused"]["fwd_bwd_ms"]
            del res
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")


if __name__ == "__main__":
    main()
