"""GPU: ResUNetSmall2(trainable=True, fused_norm=True) -- batch norm, residual, ReLU and the f16 gradient scale on the kernels of
include/umereg_bn_act.h -- held to the gates the unfused layer-wise path is held to: the forward and its intermediates against the
fp64 restatement (tests/test_sparse_grad_gpu.py), whole-network parameter gradients against fp64 autograd with the run's own ReLU
decisions forced (f32: test_sparse_grad_gpu.check_gradients; f16: the gates of tests/test_train_f16_gpu.py), 25 Adam steps on the
twin pair, one driver epoch, and the constructor.  Small clouds only; the truths are those the neighbouring files compute (their
module caches are shared and left unchanged)."""
import os

import numpy as np
import pytest
import torch

import featnet_f16_grad_ref as g16
import featnet_grad_ref as gref
import test_featnet_gpu as fg
import test_sparse_grad_gpu as sg
import test_train_f16_cpu as tc
import test_train_f16_gpu as t16

pytestmark = pytest.mark.gpu

_cache = {}


def model(dev, sd_np, train, fused=True, tp="f32", trainable=True):
    from umeregrobust_amd.models import ResUNetSmall2
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=trainable, train_precision=tp, fused_norm=fused)
    m.load_state_dict(fg.torch_state(sd_np))
    return m.to(dev).train(train)


def same_masks(a, b):
    return all(torch.equal(a[s], b[s]) for s in gref.RELU_SITES)


def fused_case(dev, name, train):
    """sg.grad_case with fused_norm=True: the fused GPU run (forward, two backward passes) beside the unfused case's fp64 / fp32 free
    runs; the forced-decision gradients are the unfused case's where the two runs decided every ReLU alike, else recomputed."""
    key = (name, train)
    if key in _cache:
        return _cache[key]
    base = sg.grad_case(dev, name, train)
    c = dict(base)
    m = model(dev, base["sd"], train)
    res, inter = sg.forward(m, base["coords"], dev)
    c["buffers"] = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    G = base["G"]
    (res.F * G.to(dev)).sum().backward()
    c["g_gpu"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out"], c["inter"], c["res"] = res.F.detach().cpu().double(), inter, res
    m.zero_grad(set_to_none=True)
    res2, _ = sg.forward(m, base["coords"], dev)
    (res2.F * G.to(dev)).sum().backward()
    c["g_gpu_again"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out_again"] = res2.F.detach()
    rows = c["rows"] = sg.row_maps(inter["coords"], base["tables"])
    c["gpu_named"] = sg.to_helper_rows(inter, rows)
    vals = gref.site_values(c["gpu_named"] | {"cat": [c["gpu_named"][f"cat{l}"] for l in range(4)]})
    c["masks"] = {s: vals[s] > 0 for s in gref.RELU_SITES}
    if not same_masks(c["masks"], base["masks"]):
        c["g64"] = sg.helper_grads(base["tables"], base["sd"], torch.float64, train, c["masks"], G)
        c["g32"] = sg.helper_grads(base["tables"], base["sd"], torch.float32, train, c["masks"], G)
    _cache[key] = c
    return c


# ---- 1. forward and intermediates ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_forward_and_intermediates_pass_the_unfused_path_s_gates(gpu, train):
    """a batch of two, equal parameters, fused_norm on and off: output, cat0..3, s4 and hidden within the gates of
    test_sparse_grad_gpu.forward_gates of the fp64 restatement (train: 4 x the fp32 helper's own error; eval under grad: TOL x
    magnitude), for both runs; train mode: the fused run's running statistics within 1e-5 of the fp64 helper's, as there."""
    base, c = sg.grad_case(gpu, "batch2", train), fused_case(gpu, "batch2", train)
    assert c["res"].F.requires_grad and len(set(base["coords"][:, 0])) == 2
    gates, gate_out = sg.forward_gates(base, train)
    truth, truth_out = base["free64"][1], base["free64"][0]
    for label, run in (("fused", c), ("unfused", base)):
        err = {k: float((run["gpu_named"][k] - truth[k]).abs().max()) for k in sg.TENSORS}
        err_out = float((run["out"] - truth_out).abs().max())
        print(f"[fused_norm forward {'train' if train else 'eval'} {label}] max|gpu-fp64| out={err_out:.2e} "
              + " ".join(f"{k}={v:.2e}" for k, v in err.items()) + " | gates out=%.2e " % gate_out + " ".join(f"{k}={v:.2e}" for k, v in gates.items()))
        assert err_out <= gate_out, (label, err_out, gate_out)
        for k in sg.TENSORS:
            assert err[k] <= gates[k], (label, k, err[k], gates[k])
    sd64, loaded = base["free64"][3], fg.torch_state(base["sd"])
    for k, v in c["buffers"].items():
        if not train:
            assert torch.equal(v, loaded[k].to(v.dtype)), k                  # eval mode moves nothing
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(sd64[k]) == 1, k
        else:
            assert float((v.double() - sd64[k]).abs().max() / sd64[k].abs().max()) <= 1e-5, k


# ---- 2. parameter gradients -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_f32_gradients_pass_the_unfused_path_s_gate(gpu, train):
    """test_sparse_grad_gpu.check_gradients on the fused run: legitimate ReLU decisions, e_gpu <= 4 max(e_cpu, median e_cpu) per
    parameter against fp64 autograd with the run's decisions forced, two backward passes bit for bit"""
    sg.check_gradients(fused_case(gpu, "small", train), train, f"fused_norm small {'train' if train else 'eval'}")


def test_f16_gradients_pass_the_f16_path_s_gates(gpu):
    """train_precision="f16", fused_norm=True (the scale from grad_scale_device), train mode: per parameter rms(g - G64) <= M_RMS
    rms(GE16) and max |g - G64| <= M_MAX max |GE16| (tests/test_train_f16_gpu.py: M_RMS = M_MAX = 1.7), the same truths G64 and G16
    with this run's ReLU decisions; two passes bit for bit."""
    base = t16.grad_case(gpu, "small", True)
    m = model(gpu, base["sd"], True, tp="f16")
    G = base["G"]
    runs = []
    for _ in range(2):
        m.load_state_dict(fg.torch_state(base["sd"]))
        m.zero_grad(set_to_none=True)
        res, inter = sg.forward(m, base["coords"], gpu)
        (res.F * G.to(gpu)).sum().backward()
        runs.append((res.F.detach().cpu(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    assert t16.bits(runs[0][0]).equal(t16.bits(runs[1][0]))
    for k, g in runs[0][1].items():
        assert t16.bits(g).equal(t16.bits(runs[1][1][k])), k
    named = sg.to_helper_rows(inter, sg.row_maps(inter["coords"], base["tables"]))
    vals = gref.site_values(named | {"cat": [named[f"cat{l}"] for l in range(4)]})
    masks = {s: vals[s] > 0 for s in gref.RELU_SITES}
    g64, G16 = base["g64"], base["G16"]
    if not same_masks(masks, base["masks"]):
        g64 = tc.helper_grads(gref.network, base["tables"], base["sd"], torch.float64, True, masks, G)
        G16 = tc.helper_grads(g16.network, base["tables"], base["sd"], torch.float64, True, masks, G)
    e = tc.gradient_errors(runs[0][1], g64, G16)
    print(f"[fused_norm f16 gradients] worst parameter: rms ratio {max(v[0] for v in e.values()):.3f} max ratio "
          f"{max(v[1] for v in e.values()):.3f}; median rms ratio {np.median([v[0] for v in e.values()]):.3f}")
    over = {k: v for k, v in e.items() if not (v[0] <= tc.M_RMS and v[1] <= tc.M_MAX)}
    assert not over, over


# ---- 3. Adam on the twin pair -----------------------------------------------------------------------------------------------------------

def train_25(dev, fused, steps=25):
    """test_sparse_grad_gpu.train_25 with the `fused_norm` keyword"""
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    src, tgt, matches = sg.training_pair()
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, fused_norm=fused)
    m.load_state_dict(sg.initial_state(0))
    m = m.to(dev).train()
    loss_func = MyInfoNCELossNoSeg(tau=0.1, neg_euclid_dist=5)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    st = [SparseTensor(torch.ones(len(c), 1, device=dev), coordinates=torch.from_numpy(c.astype(np.int32)).to(dev)) for c in (src, tgt)]
    src_pts = torch.from_numpy(src[None, :, 1:] * 0.3).float().to(dev)
    mt = torch.from_numpy(matches[None]).to(dev)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_func(torch.stack(m(st[0]).decomposed_features, dim=0), src_pts, torch.stack(m(st[1]).decomposed_features, dim=0), mt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return m, opt, losses


def test_it_trains_deterministically_and_the_checkpoint_is_the_unfused_one_s(gpu, tmp_path):
    """25 Adam steps on the twin pair of test_sparse_grad_gpu.py: two fused runs end in bit-identical parameters; the loss is finite and
    falls to a quarter of the first step's or below (the bound of test_a_training_step_is_a_training_step); the state dict has the
    unfused model's keys, shapes and dtypes, and loads into the fused eval network, whose forward agrees with this model's own
    layer-wise eval forward within TOL."""
    from umeregrobust_amd.datasets import checkpoint_state_dict
    from umeregrobust_amd.models import ResUNetSmall2
    (m, opt, losses), (m2, _, losses2) = train_25(gpu, True), train_25(gpu, True)
    print(f"[fused_norm training] loss {losses[0]:.4f} -> {losses[-1]:.4f} over {len(losses)} steps")
    assert len(losses) == 25 and all(np.isfinite(losses))
    assert losses[24] <= losses[0] / 4, losses
    assert losses == losses2
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    sd, plain = m.state_dict(), ResUNetSmall2(trainable=True).state_dict()
    assert list(sd) == list(plain) == list(fg.SHAPES) and {k: list(v.shape) for k, v in sd.items()} == fg.SHAPES
    assert all(sd[k].dtype == plain[k].dtype for k in sd)
    assert int(sd["norm1.bn.num_batches_tracked"]) == 50
    path = tmp_path / "checkpoint_epoch_1.pth"
    torch.save({"epoch": 1, "model_state_dict": sd, "optimizer_state_dict": opt.state_dict(), "total_loss": float(losses[-1])}, path)
    loaded = {k: v.cpu().numpy() for k, v in checkpoint_state_dict(str(path)).items()}
    fused_eval = model(gpu, loaded, False, fused=False, trainable=False)
    unfused = model(gpu, loaded, False, fused=False)                   # and a checkpoint of this path loads into the other
    src, _, _ = sg.training_pair()
    with torch.no_grad():
        a = sg.forward(fused_eval, src, gpu, debug=False).F
    b = sg.forward(m.eval(), src, gpu, debug=False).F
    c = sg.forward(unfused, src, gpu, debug=False).F
    assert b.requires_grad and c.requires_grad
    err, err_u = float((a - b.detach()).abs().max()), float((a - c.detach()).abs().max())
    print(f"[fused_norm training] fused eval forward of the saved weights against the layer-wise eval forwards: fused_norm {err:.2e}, plain {err_u:.2e}")
    assert err <= fg.TOL and err_u <= fg.TOL
    # the layer-wise eval under no_grad is the fused call whatever the switch says
    with torch.no_grad():
        assert sg.forward(m, src, gpu, debug=False).F.view(torch.int32).equal(a.view(torch.int32))


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------------

def test_driver_runs_an_epoch_with_the_switch(gpu, tmp_path):
    """`--synthetic 4 --epochs 1 --fused-norm` (main -> run(..., fused_norm=True)): the epoch completes and writes a checkpoint whose
    keys, shapes and dtypes equal the plain run's"""
    from umeregrobust_amd import train_coloring as tcol
    files = {}
    for tag, extra in (("plain", []), ("fused", ["--fused-norm"])):
        run_dir = tcol.main(["--synthetic", "4", "--epochs", "1", "--output-path", str(tmp_path / tag)] + extra)
        files[tag] = torch.load(os.path.join(run_dir, "last_epoch_checkpoint.pth"), weights_only=True)
    a, b = files["plain"], files["fused"]
    assert sorted(a) == sorted(b)
    sa, sb = a["model_state_dict"], b["model_state_dict"]
    assert list(sa) == list(sb) == list(fg.SHAPES)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape, k
        assert bool(torch.isfinite(sb[k].double()).all()), k
    assert np.isfinite(b["total_loss"]) and int(sb["norm1.bn.num_batches_tracked"]) == int(sa["norm1.bn.num_batches_tracked"]) > 0


# ---- 5. the constructor -------------------------------------------------------------------------------------------------------------------

def test_fused_norm_needs_trainable(gpu):
    from umeregrobust_amd.models import ResUNetSmall2
    with pytest.raises(ValueError, match="trainable=True"):
        ResUNetSmall2(fused_norm=True)
    with pytest.raises(ValueError, match="trainable=True"):
        ResUNetSmall2(fused_norm=True, precision="f16")
    assert ResUNetSmall2(trainable=True, fused_norm=True, train_precision="f16").fused_norm
