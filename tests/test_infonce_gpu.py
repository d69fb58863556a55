"""GPU: the fused InfoNCE loss (umeregrobust_amd/infonce.py, pw_loss.py on csrc/infonce.hip) against fp64 truth -- the library's own
torch class `loss.MyInfoNCELossNoSeg` in fp64 on the CPU -- at the project's gates (tests/infonce_cases.py): every tile edge of the
plan, the reference's recorded golden, duplicate rows, determinism and batching, upstream and one-sided gradients, the range in which
the torch form overflows, an out-of-range match, guard bands around the raw calls, and the training driver with --fused-pointwise."""
import os

import numpy as np
import pytest
import torch

import infonce_cases as ic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD = 4096
CANARY = 0xA5


def fused(inp, gpu, tau=ic.TAU, neg_dist=ic.NEG_DIST, upstream=None, need=(True, True)):
    """pw_loss.MyInfoNCELossNoSeg with autograd -> (loss, dsrc, dtgt) as Python float / fp64 numpy (None for a side without grad)"""
    from umeregrobust_amd.pw_loss import MyInfoNCELossNoSeg
    fn = MyInfoNCELossNoSeg(tau=tau, neg_euclid_dist=neg_dist)
    a = inp["src_feat"].detach().to(gpu).requires_grad_(need[0])
    p = inp["tgt_feat"].detach().to(gpu).requires_grad_(need[1])
    loss = fn(a, inp["src_pts"].to(gpu), p, inp["matches"].to(gpu))
    (loss if upstream is None else upstream * loss).backward()
    g = [None if t.grad is None else t.grad.double().cpu().numpy() for t in (a, p)]
    return float(loss.detach()), g[0], g[1]


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", ["far", "near"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", ic.EDGE_S)
def test_tile_edges(gpu, S, B, lattice):
    inp, truth, f32 = ic.case(100 + S, B, 300, 260, S, lattice)
    got = fused(inp, gpu)
    if S == 1:
        assert abs(truth[0]) <= ic.ZERO_TRUTH and abs(got[0]) <= 1e-6
        assert np.abs(truth[1]).max() <= ic.ZERO_TRUTH and np.abs(truth[2]).max() <= ic.ZERO_TRUTH
        assert np.abs(got[1]).max() <= 1e-7 and np.abs(got[2]).max() <= 1e-7
    # S = 1 has no negative at all; S = 2 on the near lattice may have none
    ic.check(f"S={S} B={B} {lattice}", got, truth, f32, zero_truth=S <= 2)


# ---- golden ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["far", "near"])
def test_golden_of_the_reference(gpu, kind):
    g = np.load(os.path.join(GOLDEN, "g13_infonce.npz"))
    inp = {k: torch.from_numpy(g[f"{kind}_{k}"]) for k in ("src_feat", "src_pts", "tgt_feat", "matches")}
    # the nearest anchor pair to the threshold, in metres (fp64): coordinate differences and cdist agree on every `far`
    x = inp["src_pts"][0].double()[inp["matches"][0, :, 0]]
    gap = float(((x[:, None] - x[None]).norm(dim=-1) - float(g["neg_euclid_dist"])).abs().min())
    assert gap > 1e-3, gap
    want = (float(g[f"{kind}_loss"]), g[f"{kind}_grad_src"].astype(np.float64), g[f"{kind}_grad_tgt"].astype(np.float64))
    got = fused(inp, gpu, tau=float(g["tau"]), neg_dist=float(g["neg_euclid_dist"]))
    ic.check(f"golden {kind} (nearest pair {gap:.1e} m from the threshold)", got, want)


# ---- duplicates --------------------------------------------------------------------------------------------------------------------------

def _dup_case(S):
    inp = {k: v.clone() for k, v in ic.make_inputs(700 + S, 2, 300, 260, S, "far").items()}
    m = inp["matches"]
    m[:, S - 1, 0] = m[:, 3, 0]         # two samples name one source row (their anchors coincide: distance 0, never far)
    m[:, S - 2, 1] = m[:, 5, 1]         # two others name one target row
    m[1, 7, 0] = m[1, 3, 0]             # and a row named three times
    ic.assert_exact_mask(inp)
    return inp, ic.torch_class(inp, torch.float64), ic.torch_class(inp, torch.float32)


@pytest.mark.parametrize("S", [33, 129])
def test_duplicate_rows_are_summed_in_one_order(gpu, S):
    inp, truth, f32 = _dup_case(S)
    got = fused(inp, gpu)
    ic.check(f"duplicates S={S}", got, truth, f32)
    again = fused(inp, gpu)
    assert got[0] == again[0] and got[1].tobytes() == again[1].tobytes() and got[2].tobytes() == again[2].tobytes()


# ---- raw calls between canaries ----------------------------------------------------------------------------------------------------------

class Guard:
    def __init__(self, dev, fill):
        self.dev, self.fill, self.bufs = dev, fill, []

    def buf(self, nbytes, name):
        full = torch.empty(int(nbytes) + 2 * PAD, dtype=torch.uint8, device=self.dev)
        full[:PAD] = CANARY
        full[PAD + nbytes:] = CANARY
        full[PAD:PAD + nbytes] = self.fill
        self.bufs.append((name, full, int(nbytes)))
        return full[PAD:PAD + nbytes]

    def check(self):
        torch.cuda.synchronize()
        for name, full, n in self.bufs:
            assert bool((full[:PAD] == CANARY).all()), f"{name}: bytes BEFORE the buffer were written"
            assert bool((full[PAD + n:] == CANARY).all()), f"{name}: bytes BEHIND the buffer ({n} B) were written"


def raw_call(inp, gpu, fill, tau=ic.TAU, neg_dist=ic.NEG_DIST, upstream=1.0):
    """one raw forward + backward with every output and the workspace at exactly their stated sizes between canaries, pre-filled with
    `fill` -> {name: CPU tensor}"""
    from umeregrobust_amd import _lib, infonce
    lib = infonce.load_native()
    d = {k: v.to(gpu).contiguous() for k, v in inp.items()}
    B, N = d["src_feat"].shape[:2]
    M, S = d["tgt_feat"].shape[1], d["matches"].shape[1]
    G = Guard(gpu, fill)
    need = lib.umereg_infonce_workspace_bytes(B, N, M, S)
    assert need == ic.workspace_bytes(B, N, M, S) > 0
    ws = G.buf(need, "workspace")
    stats = G.buf(B * S * 2 * 4, "row_stats")
    loss = G.buf(4, "loss")
    dsrc = G.buf(B * N * 32 * 4, "dsrc")
    dtgt = G.buf(B * M * 32 * 4, "dtgt")
    g = torch.full((1,), upstream, dtype=torch.float32, device=gpu)
    common = (d["src_feat"].data_ptr(), d["src_pts"].data_ptr(), d["tgt_feat"].data_ptr(), d["matches"].data_ptr(), B, N, M, S, tau, neg_dist)
    st = _lib.stream_ptr(gpu)
    _lib.call(gpu, lib.umereg_infonce_fwd_f32, *common, stats.data_ptr(), loss.data_ptr(), ws.data_ptr(), need, st)
    ws[:] = fill ^ 0xFF                 # the backward must not depend on what the forward left in the workspace
    _lib.call(gpu, lib.umereg_infonce_bwd_f32, *common, stats.data_ptr(), g.data_ptr(), dsrc.data_ptr(), dtgt.data_ptr(), ws.data_ptr(), need, st)
    G.check()
    return {"row_stats": stats.view(torch.float32).view(B, S, 2).cpu(), "loss": loss.view(torch.float32).cpu(),
            "dsrc": dsrc.view(torch.float32).view(B, N, 32).cpu(), "dtgt": dtgt.view(torch.float32).view(B, M, 32).cpu()}


def same_bytes(a, b):
    return all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)


def test_guard_bands_and_run_twice(gpu):
    S = ic.ROWS + 1
    inp, truth, f32 = ic.case(100 + S, 3, 300, 260, S, "far")
    r0, r1 = raw_call(inp, gpu, 0xCD), raw_call(inp, gpu, 0x3C)
    assert same_bytes(r0, r1), "an output byte the call did not write, or a dependence on what the workspace held"
    ic.check("raw S=R+1", (float(r0["loss"]), r0["dsrc"].double().numpy(), r0["dtgt"].double().numpy()), truth, f32)
    # zero wherever no match names the row
    for side, key in ((0, "dsrc"), (1, "dtgt")):
        for b in range(3):
            named = torch.zeros(r0[key].shape[1], dtype=torch.bool)
            named[inp["matches"][b, :, side]] = True
            assert bool((r0[key][b][~named] == 0).all()) and bool((r0[key][b][named].abs().sum(-1) > 0).all())


def test_an_out_of_range_match_gives_nan_and_stays_in_bounds(gpu):
    """a refusal path that must stay in bounds: the entry is never dereferenced, its row (hence the loss) is NaN"""
    S = ic.ROWS + 1
    inp = {k: v.clone() for k, v in ic.case(100 + S, 3, 300, 260, S, "far")[0].items()}
    inp["matches"][1, 4, 0] = 300       # = N
    r = raw_call(inp, gpu, 0xCD)
    assert bool(torch.isnan(r["loss"]).all())
    assert bool(torch.isnan(r["row_stats"][1, 4]).all())
    assert bool(torch.isfinite(r["row_stats"][0]).all()) and bool(torch.isfinite(r["row_stats"][2]).all())
    keep = torch.ones(S, dtype=torch.bool)
    keep[4] = False
    assert bool(torch.isfinite(r["row_stats"][1][keep]).all()), "the sample takes no part in the other rows"
    inp["matches"][1, 4] = torch.tensor([5, -1])
    assert bool(torch.isnan(raw_call(inp, gpu, 0x3C)["loss"]).all())


# ---- determinism and batching ------------------------------------------------------------------------------------------------------------

def test_a_batch_equals_its_elements_run_alone(gpu):
    S = 200
    inp = ic.case(100 + S, 3, 300, 260, S, "near")[0]
    r0, r1 = raw_call(inp, gpu, 0xEE), raw_call(inp, gpu, 0x17)
    assert same_bytes(r0, r1)
    for b in range(3):
        one = raw_call({k: v[b:b + 1] for k, v in inp.items()}, gpu, 0x5A)
        assert one["row_stats"][0].numpy().tobytes() == r0["row_stats"][b].numpy().tobytes(), b
        # (the gradients carry 1 / (B S): a third of the element's own)
        np.testing.assert_allclose(one["dsrc"][0].numpy() / 3, r0["dsrc"][b].numpy(), rtol=1e-6, atol=1e-12)


# ---- upstream gradient, one-sided gradients, no_grad ---------------------------------------------------------------------------------------

def test_upstream_and_one_sided_gradients(gpu):
    from umeregrobust_amd.pw_loss import MyInfoNCELossNoSeg
    S = ic.COLS + 1
    inp, truth, f32 = ic.case(100 + S, 3, 300, 260, S, "near")
    scaled = ic.torch_class(inp, torch.float64, upstream=0.37)
    got = fused(inp, gpu, upstream=0.37)
    ic.check("upstream 0.37", got, scaled, ic.torch_class(inp, torch.float32, upstream=0.37))
    both = fused(inp, gpu)
    only_src = fused(inp, gpu, need=(True, False))
    only_tgt = fused(inp, gpu, need=(False, True))
    assert only_src[2] is None and only_tgt[1] is None
    assert only_src[0] == both[0] == only_tgt[0]
    assert only_src[1].tobytes() == both[1].tobytes() and only_tgt[2].tobytes() == both[2].tobytes()
    d = {k: v.to(gpu) for k, v in inp.items()}
    with torch.no_grad():
        plain = MyInfoNCELossNoSeg(tau=ic.TAU, neg_euclid_dist=ic.NEG_DIST)(d["src_feat"], d["src_pts"], d["tgt_feat"], d["matches"])
    assert not plain.requires_grad and float(plain) == both[0]
    # S = 0: NaN, as the torch class's empty mean
    empty = MyInfoNCELossNoSeg()(d["src_feat"], d["src_pts"], d["tgt_feat"], d["matches"][:, :0])
    assert empty.dim() == 0 and bool(torch.isnan(empty))


# ---- range -------------------------------------------------------------------------------------------------------------------------------

def test_logits_beyond_the_torch_form_s_range(gpu):
    """features scaled by 4: l / tau reaches 160 and the fp32 torch class overflows; the running maximum keeps the fused form finite"""
    S = 200
    inp, truth, f32 = ic.case(100 + S, 3, 300, 260, S, "far", 4.0)
    a = inp["src_feat"].double()[0][inp["matches"][0, :, 0]]
    p = inp["tgt_feat"].double()[0][inp["matches"][0, :, 1]]
    top = float((a @ p.T).max() / ic.TAU)
    assert top > 88.0 and not np.isfinite(f32[0]), (top, f32[0])
    assert np.isfinite(truth[0])
    got = fused(inp, gpu)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    ic.check(f"range (largest l / tau {top:.1f})", got, truth)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------

def test_the_trainer_with_fused_pointwise(gpu, tmp_path_factory):
    """run(..., synthetic=4, fused_pointwise=True) with the synthetic settings of main(): finite losses, the first step's point-wise
    term within 1e-6 of the torch class on the same batch, and byte-identical checkpoints from two runs of one seed"""
    import json
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.pw_loss import MyInfoNCELossNoSeg as Fused

    def config():
        args = tc.make_config("kitti", device=str(gpu), num_epochs=1, output_path=str(tmp_path_factory.getbasetemp()))
        args.ume_max_nn, args.ume_min_nn, args.ume_r_nn, args.ume_n_samples, args.num_pw_samples = 64, 8, 2.0, 32, 128
        args.eval_num_kpts, args.batch_size = 32, min(args.batch_size, 2)
        return args
    outs = []
    for run in range(2):
        out = str(tmp_path_factory.mktemp(f"fused{run}"))
        tc.run(config(), synthetic=4, out_path=out, fused_pointwise=True)
        outs.append(out)
    rows = [json.loads(ln) for ln in open(os.path.join(outs[0], "scalars.jsonl"))]
    values = [r["value"] for r in rows if "loss" in r["tag"]]
    assert values and all(np.isfinite(values)), values
    a = open(os.path.join(outs[0], "last_epoch_checkpoint.pth"), "rb").read()
    assert a == open(os.path.join(outs[1], "last_epoch_checkpoint.pth"), "rb").read()
    # the first step's point-wise term: the same first batch through both classes at the same initial state
    args = config()
    torch.manual_seed(args.random_seed)
    np.random.seed(args.random_seed)
    loader, _ = tc.make_loaders(args, 4, 3000, False)
    model = tc.ResUNetSmall2(in_channels=1, out_channels=args.out_channels, trainable=True).to(gpu).train()
    batch = tc.Batch(next(iter(loader)), gpu)
    sf, tf = tc.network_features(model, batch.src).detach(), tc.network_features(model, batch.tgt).detach()     # (as the step runs it)
    with torch.no_grad():
        kw = dict(num_samples=args.num_pw_samples, tau=args.tau, neg_euclid_dist=tc.NEG_EUCLID_DIST)
        want = float(MyInfoNCELossNoSeg(**kw)(sf, batch.src_pts, tf, batch.matches))
        got = float(Fused(**kw)(sf, batch.src_pts, tf, batch.matches))
    logged = [r["value"] for r in rows if r["tag"] == "train/pointwise_loss"][0]
    print(f"[infonce trainer] first point-wise term: logged {logged:.7f} fused {got:.7f} torch class {want:.7f}")
    assert abs(got - want) <= 1e-6 * abs(want)
    assert abs(logged - want) <= 1e-6 * abs(want)
