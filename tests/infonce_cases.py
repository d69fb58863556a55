"""Shared by tests/test_infonce_cpu.py and tests/test_infonce_gpu.py: the Python restatement of csrc/infonce_plan.h, the exact-mask
inputs, the fp64 truth and the gates.

Truth is the library's own torch class `loss.MyInfoNCELossNoSeg` run in fp64 on the CPU with autograd.  The gates are the project's
(tests/test_sparse_grad_cpu.py): |loss - truth| <= 1e-6 |truth|, and per gradient tensor max|got - truth| <= 1e-5 max|truth|.

Exact masks: positions come from an integer lattice, so squared distances are integers, and neg_euclid_dist = sqrt(40.5): no pair is
within rounding of the threshold, and coordinate differences and torch's matrix-product cdist agree on every `far`."""
import functools

import numpy as np
import torch

# ---- csrc/infonce_plan.h, restated (tests/test_infonce_cpu.py compares this with the header's own answers) -----------------------
D = 32
WAVES = 4
THREADS = 64 * WAVES
ROWS = 32                   # R: rows per workgroup
COLS = 32 * WAVES           # C: columns per step
LDS_STRIDE = 36
MAX_S = 8192
SCATTER_ROWS = 64
LDS_BYTES = COLS * LDS_STRIDE * 4 + COLS * 16
SCATTER_LDS_BYTES = MAX_S * 4
LDS_PER_CU = 160 * 1024


def _align(v):
    return (v + 255) // 256 * 256


def sizes_ok(B, N, M, S):
    return B >= 1 and N >= 1 and M >= 1 and 1 <= S <= MAX_S and N < 2 ** 31 and M < 2 ** 31 and B * ((S + ROWS - 1) // ROWS) <= 0x3fffffff


def workspace_bytes(B, N, M, S):
    if not sizes_ok(B, N, M, S):
        return 0
    return _align(B * ((S + ROWS - 1) // ROWS) * 8) + 2 * _align(B * S * D * 4) + _align(B * S * 4)


# the sizes at which the kernels take another path: one row, a partial / full / just-over row block, the same for a column step, more than
# two row blocks with a ragged end, and one more than a column step with ragged everything
EDGE_S = (1, 2, ROWS - 1, ROWS, ROWS + 1, COLS - 1, COLS, COLS + 1, 2 * ROWS + 1, 200)

TAU = 0.1
R2 = 40.5
NEG_DIST = float(np.sqrt(R2))
LATTICES = {"far": 12, "near": 4}       # [-L, L]^3: about 93 % / about half of the pairs are farther than sqrt(40.5)


def make_inputs(seed, B, N, M, S, lattice, scale=1.0, replace=False):
    """-> dict of CPU tensors: src_feat [B, N, 32], src_pts [B, N, 3], tgt_feat [B, M, 32] (f32), matches int64 [B, S, 2].
    Features are unit rows, the matched target rows are their source rows plus noise, renormalised (as tools/gen_infonce_golden.py
    makes them), all times `scale`.  The S anchors of a batch element sit on distinct lattice points."""
    rng = np.random.default_rng(seed)
    L = LATTICES[lattice] if isinstance(lattice, str) else int(lattice)

    def unit(n):
        f = rng.standard_normal((n, D))
        return f / np.linalg.norm(f, axis=1, keepdims=True)
    src = np.stack([unit(N) for _ in range(B)])
    tgt = np.stack([unit(M) for _ in range(B)])
    side = 2 * L + 1
    assert side ** 3 >= N
    pts = np.empty((B, N, 3))
    m = np.empty((B, S, 2), np.int64)
    for b in range(B):
        cells = rng.choice(side ** 3, N, replace=False)
        pts[b] = np.stack([cells // (side * side), cells // side % side, cells % side], 1) - L
        m[b, :, 0] = rng.choice(N, S, replace=replace)
        m[b, :, 1] = rng.choice(M, S, replace=replace)
        if not replace:
            t = src[b, m[b, :, 0]] + 0.5 * unit(S)
            tgt[b, m[b, :, 1]] = t / np.linalg.norm(t, axis=1, keepdims=True)
    f32 = lambda a: torch.from_numpy((a * scale).astype(np.float32))       # noqa: E731
    return {"src_feat": f32(src), "src_pts": torch.from_numpy(pts.astype(np.float32)), "tgt_feat": f32(tgt), "matches": torch.from_numpy(m)}


def assert_exact_mask(inp, r2=R2):
    """fp64: no off-diagonal anchor pair has a squared distance within 0.25 of r2 (two samples on one source row have distance 0)."""
    for b in range(inp["matches"].shape[0]):
        x = inp["src_pts"][b].double()[inp["matches"][b, :, 0]]
        d2 = ((x[:, None] - x[None]) ** 2).sum(-1)
        off = ~torch.eye(len(x), dtype=torch.bool)
        assert not bool(((d2 - r2).abs() < 0.25)[off].any()), "an anchor pair lies within rounding of the threshold"


def torch_class(inp, dtype, tau=TAU, neg_dist=NEG_DIST, upstream=1.0):
    """`loss.MyInfoNCELossNoSeg` on the CPU in `dtype` -> (loss, dsrc, dtgt) as fp64 numpy"""
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    fn = MyInfoNCELossNoSeg(tau=tau, neg_euclid_dist=neg_dist)
    a = inp["src_feat"].detach().clone().to(dtype).requires_grad_()        # (a copy: the shared inputs stay as they are)
    p = inp["tgt_feat"].detach().clone().to(dtype).requires_grad_()
    loss = fn(a, inp["src_pts"].to(dtype), p, inp["matches"])
    (upstream * loss).backward()
    return float(loss.detach()), a.grad.double().numpy(), p.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def case(seed, B, N, M, S, lattice, scale=1.0):
    """-> (inputs, fp64 truth, the fp32 torch class on the CPU): made once per shape and shared, never modified"""
    inp = make_inputs(seed, B, N, M, S, lattice, scale)
    assert_exact_mask(inp)
    return inp, torch_class(inp, torch.float64), torch_class(inp, torch.float32)


def loss_err(got, truth):
    return abs(got - truth) / abs(truth) if truth != 0 else abs(got)


LOSS_GATE = 1e-6
GRAD_GATE = 1e-5
ZERO_TRUTH = 1e-12      # a gradient tensor whose fp64 truth stays below this is zero up to the rounding of fp64 autograd


def grad_err(got, truth):
    """max|got - truth| / max|truth|; where the truth is zero (S = 1: a row without negatives; fp64 autograd leaves 1e-16 there),
    max|got| / 1e-2, so that the gate of 1e-5 asserts max|got| <= 1e-7"""
    top = np.abs(truth).max()
    return float(np.abs(np.asarray(got, np.float64) - truth).max() / (top if top > ZERO_TRUTH else 1e-2))


def check(tag, got, truth, f32=None, zero_truth=False):
    """got / truth / f32: (loss, dsrc, dtgt).  Prints the kernel's error beside the fp32 torch class's, then asserts the gates.
    zero_truth: the case may have no negative at all (loss and gradients exactly 0); everywhere else max|truth| > 0 is asserted."""
    el = loss_err(got[0], truth[0])
    eg = []
    for k in (1, 2):
        assert zero_truth or np.abs(truth[k]).max() > ZERO_TRUTH, f"{tag}: the truth of gradient {k} is all zero"
        eg.append(grad_err(got[k], truth[k]))
    ref = ""
    if f32 is not None:
        fl = loss_err(f32[0], truth[0]) if np.isfinite(f32[0]) else float("nan")
        ref = f" | fp32 torch class: loss {fl:.2e} dsrc {grad_err(f32[1], truth[1]):.2e} dtgt {grad_err(f32[2], truth[2]):.2e}"
    print(f"[infonce {tag}] loss {got[0]:.7f} truth {truth[0]:.7f}: err {el:.2e}; dsrc {eg[0]:.2e} dtgt {eg[1]:.2e}{ref}")
    assert np.isfinite(got[0]) and el <= LOSS_GATE, f"{tag}: loss {got[0]} vs {truth[0]} ({el:.2e})"
    assert eg[0] <= GRAD_GATE, f"{tag}: dsrc {eg[0]:.2e}"
    assert eg[1] <= GRAD_GATE, f"{tag}: dtgt {eg[1]:.2e}"
