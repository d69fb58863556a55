"""GPU: the trainable ResUNetSmall2 -- the operators of include/umereg_sparse_conv.h one by one (exact on small integers,
within the derived rounding bound on N(0, 1) inputs, deterministic between guard bands), the layer-wise forward against the
fp64 restatements, every parameter gradient against fp64 autograd through tests/featnet_grad_ref.py with the GPU run's ReLU
decisions forced onto it, a training step that trains, and weights that the fused eval network can use.

Yardsticks: the fp64 helper is the truth; the SAME helper in fp32 on the CPU is the reference-precision run the gradient and
train-mode gates are set against (never the GPU's own output)."""
import numpy as np
import pytest
import torch

import featnet_grad_ref as gref
import featnet_ref as ref
from test_featnet_gpu import SHAPES, TOL, batch_of_two, compare, edge_cloud, f32_state, seeded, torch_state, voxel_cloud

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def small_cloud():
    """a compact slice of the KITTI-test cloud: the 6000 voxels nearest to the sensor, in the cloud's (random) row order"""
    c = voxel_cloud(0, "KT")
    near = np.sort(np.argsort((c[:, 1:] ** 2).sum(1), kind="stable")[:6000])
    return c[near]


CLOUDS = {"small": small_cloud, "batch2": batch_of_two, "KT": lambda: voxel_cloud(0, "KT"), "one_cell": lambda: edge_cloud("one_cell")}
_cache = {}


def cloud(name):
    if ("cloud", name) not in _cache:
        _cache[("cloud", name)] = CLOUDS[name]()
    return _cache[("cloud", name)]


def tables_of(name):
    if ("tables", name) not in _cache:
        _cache[("tables", name)] = gref.Tables(cloud(name))
    return _cache[("tables", name)]


def row_maps(level_coords, tables):
    """per level: helper row of every GPU row (matched by coordinate)"""
    rows = []
    for l in range(5):
        gc = level_coords[l].cpu().numpy().astype(np.int64)
        assert len(gc) == tables.sizes[l], f"level {l}: {len(gc)} rows, restatement {tables.sizes[l]}"
        idx = ref.Index(tables.levels[l]).find(gc)
        assert (idx >= 0).all() and len(np.unique(idx)) == len(idx), f"level {l}: coordinates differ"
        rows.append(torch.from_numpy(idx))
    return rows


# ---- 6 / 7: the operators ---------------------------------------------------------------------------------------------------

# (table, C_in, C_out) of every 27-offset layer of the network
OPS = [(0, 1, 32), (0, 32, 32), (0, 64, 64), (1, 64, 64), (2, 64, 64), (2, 128, 128), (3, 128, 128), (4, 256, 256), (5, 32, 64),
       (6, 64, 64), (7, 64, 128), (8, 128, 256), (9, 128, 64), (10, 192, 64), (11, 256, 128), (12, 256, 128)]


def gpu_maps(name, dev):
    from umeregrobust_amd import sparse_conv as sc
    if ("maps", name) not in _cache:
        c = cloud(name)
        C = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        maps = sc.CoordinateMaps(C, int(c[:, 0].max()) + 1)
        rows = row_maps([maps.level_coords(l) for l in range(5)], tables_of(name))
        assert np.array_equal(rows[0].numpy(), maps.perm.cpu().numpy())          # level 0 of the helper is the input order
        _cache[("maps", name)] = (maps, rows)
    return _cache[("maps", name)]


def draw(shape, lo, hi, integer, g):
    if integer:
        return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g, dtype=torch.float32)


def run_operator(name, dev, t, cin, cout, integer):
    """-> dict of (gpu, truth, abs-product sum, chain length) for `out`, `dx` (C_in > 1), `dw`, in the helper's row order"""
    from umeregrobust_amd import sparse_conv as sc
    maps, rows = gpu_maps(name, dev)
    tables = tables_of(name)
    li, lo = gref.in_level(t), gref.out_level(t)
    g = torch.Generator().manual_seed(1000 * t + cin + cout)
    x = draw((tables.sizes[li], cin), -3, 3, integer, g)
    dy = draw((tables.sizes[lo], cout), -3, 3, integer, g)
    W = draw((27, cin, cout), -2, 2, integer, g)
    # GPU, through the autograd function; rows in the GPU's level order (conv1: features in input order = the helper's level 0)
    xg = (x if cin == 1 else x[rows[li]]).to(dev).requires_grad_(cin > 1)
    Wg = W.to(dev).requires_grad_()
    y = sc.sparse_conv(xg, Wg, maps, t)
    y.backward(dy[rows[lo]].to(dev))
    got = {"out": torch.empty_like(dy).index_copy_(0, rows[lo], y.detach().cpu()), "dw": Wg.grad.cpu()}
    if cin > 1:
        got["dx"] = torch.empty_like(x).index_copy_(0, rows[li], xg.grad.cpu())
    # fp64 truth and the sums of absolute products, by autograd through the helper
    res = {}
    for key, f in (("val", lambda v: v.double()), ("abs", lambda v: v.double().abs())):
        x64, W64 = f(x).requires_grad_(), f(W).requires_grad_()
        y64 = gref.conv(x64, W64, tables, t)
        (y64 * f(dy)).sum().backward()
        res[key] = {"out": y64.detach(), "dx": x64.grad, "dw": W64.grad}
    ta, _ = gref.adjoint(t)
    L = {"out": gref.chain_lengths(tables, t, cin)[:, None].expand(-1, cout),
         "dx": gref.chain_lengths(tables, ta, cout)[:, None].expand(-1, cin),
         "dw": torch.tensor([len(o) for o, _ in tables.pairs[t]])[:, None, None].expand(-1, cin, cout)}
    return {k: (got[k], res["val"][k], res["abs"][k], L[k]) for k in got}


@pytest.mark.parametrize("name", ["small", "batch2", "KT"])
def test_operators_are_exact_on_small_integers(gpu, name):
    """X, dY in [-3, 3], W in [-2, 2], integer valued: every partial sum is an integer below 2^24, so any order of fused or
    unfused accumulation is exact and the three operators must EQUAL the fp64 restatement."""
    ops = OPS if name != "batch2" else OPS[::3]
    for t, cin, cout in ops:
        for k, (got, want, absum, _) in run_operator(name, gpu, t, cin, cout, True).items():
            assert float(absum.max()) < 2 ** 24
            assert torch.equal(got.double(), want), f"{name} table {t} {cin}->{cout} {k}: " \
                f"{int((got.double() != want).sum())} of {want.numel()} elements differ, max {float((got.double() - want).abs().max())}"


@pytest.mark.parametrize("name", ["small", "KT"])
def test_operators_stay_within_the_rounding_bound(gpu, name):
    """N(0, 1) inputs: |gpu - fp64| <= gamma(2 L + 2) sum |a_i| |b_i| per element, gamma(m) = m u / (1 - m u), u = 2^-24, L the
    products in the element's chain -- the forward bound of an inner product summed in any order, fused or not."""
    worst = {}
    for t, cin, cout in OPS:
        for k, (got, want, absum, L) in run_operator(name, gpu, t, cin, cout, False).items():
            m = (2 * L + 2).double() * U
            bound = m / (1 - m) * absum
            err = (got.double() - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst[k] = max(worst.get(k, 0.0), ratio)
            bad = err > bound
            assert not bool(bad.any()), f"{name} table {t} {cin}->{cout} {k}: {int(bad.sum())} elements over the bound, worst ratio {ratio:.3g}"
            assert bool(((L == 0) <= (got == 0)).all()), "an element without a chain is not zero"
    print(f"[sparse_conv rounding {name}] worst |err| / bound: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ---- 8: determinism and guard bands -----------------------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


def test_guard_bands_and_run_twice(gpu):
    """Every device buffer of every compute entry of include/umereg_sparse_conv.h between canaries at exactly the size the header /
    the query states; scratch pre-filled with garbage, outputs with poison; two runs with other garbage agree byte for byte."""
    from umeregrobust_amd import sparse_conv as sc
    lib = sc.load_native()
    coords = batch_of_two()[::7].copy()
    n, batch = len(coords), 2
    sizes = [len(c) for c in ref.levels(coords)]
    stream = torch.cuda.current_stream(gpu).cuda_stream
    rng = np.random.default_rng(8)
    cases = [(0, 32, 32), (2, 128, 128), (6, 64, 64), (10, 192, 64), (4, 256, 256), (0, 1, 32)]
    data = {c: (rng.standard_normal((sizes[gref.in_level(c[0])], c[1])).astype(np.float32),
                rng.standard_normal((sizes[gref.out_level(c[0])], c[2])).astype(np.float32),
                rng.standard_normal((27, c[1], c[2])).astype(np.float32)) for c in cases}
    results = []
    for poison, garbage in ((0xCD, 0xEE), (0x3C, 0x17)):
        bufs = []

        def alloc(nbytes, fill):
            full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=gpu)
            full[:PAD] = CANARY
            full[PAD + nbytes:] = CANARY
            full[PAD:PAD + nbytes] = fill
            bufs.append((full, nbytes))
            return full

        def inp(a):
            a = np.ascontiguousarray(a)
            full = alloc(a.nbytes, 0)
            full[PAD:PAD + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(gpu))
            return full.data_ptr() + PAD

        def intact():
            torch.cuda.synchronize()
            for full, nb in bufs:
                assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"

        def body(full, nbytes):
            return full[PAD:PAD + nbytes].clone()

        ws_bytes = lib.umereg_featnet_workspace_bytes(n, batch)
        ws, status = alloc(ws_bytes, garbage), alloc(8 * 4, poison)
        ws_p, st_p = ws.data_ptr() + PAD, status.data_ptr() + PAD
        assert lib.umereg_featnet_build_maps(inp(coords.astype(np.int32)), n, batch, st_p, ws_p, ws_bytes, stream) == 0
        intact()
        assert status[PAD:PAD + 32].view(torch.int32).cpu().tolist()[:6] == [0] + sizes
        ones, zeros = inp(np.ones(256, np.float32)), inp(np.zeros(256, np.float32))
        outs = []
        for (t, cin, cout), (x, dy, W) in data.items():
            rows_in, rows_out = x.shape[0], dy.shape[0]
            x_p, dy_p, W_p = inp(x), inp(dy), inp(W)
            if cin > 1:
                y = alloc(rows_out * cout * 4, poison)
                rc = lib.umereg_sparse_conv_f32(ws_p, ws_bytes, st_p, n, t, x_p, cin, W_p, cin, cout, ones, zeros, y.data_ptr() + PAD, cout,
                                                0, stream)
                assert rc == 0, lib.umereg_last_error()
                Wt = alloc(27 * cin * cout * 4, poison)
                ta, mirror = gref.adjoint(t)
                assert lib.umereg_sparse_conv_repack_f32(W_p, cin, cout, 1, int(mirror), cout, Wt.data_ptr() + PAD, stream) == 0
                dx = alloc(rows_in * cin * 4, poison)
                rc = lib.umereg_sparse_conv_f32(ws_p, ws_bytes, st_p, n, ta, dy_p, cout, Wt.data_ptr() + PAD, cout, cin, ones, zeros,
                                                dx.data_ptr() + PAD, cin, 0, stream)
                assert rc == 0, lib.umereg_last_error()
                outs += [body(y, rows_out * cout * 4), body(Wt, 27 * cin * cout * 4), body(dx, rows_in * cin * 4)]
            else:
                y = alloc(n * 32 * 4, poison)
                rc = lib.umereg_sparse_conv1_f32(ws_p, ws_bytes, st_p, n, x_p, W_p, ones, zeros, y.data_ptr() + PAD, stream)
                assert rc == 0, lib.umereg_last_error()
                outs.append(body(y, n * 32 * 4))
            sc_bytes = lib.umereg_sparse_conv_wgrad_scratch_bytes(n, cin, cout)
            assert sc_bytes == lib.umereg_sparse_conv_wgrad_segments(n, cin, cout) * 27 * cin * cout * 4 > 0
            scratch, dW = alloc(sc_bytes, garbage), alloc(27 * cin * cout * 4, poison)
            rc = lib.umereg_sparse_conv_wgrad_f32(ws_p, ws_bytes, st_p, n, t, x_p, cin, cin, dy_p, cout, cout, dW.data_ptr() + PAD,
                                                  scratch.data_ptr() + PAD, sc_bytes, stream)
            assert rc == 0, lib.umereg_last_error()
            # a scratch one byte short is refused, not overrun
            assert lib.umereg_sparse_conv_wgrad_f32(ws_p, ws_bytes, st_p, n, t, x_p, cin, cin, dy_p, cout, cout, dW.data_ptr() + PAD,
                                                    scratch.data_ptr() + PAD, sc_bytes - 1, stream) == -3
            intact()
            outs.append(body(dW, 27 * cin * cout * 4))
            assert bool(torch.isfinite(outs[-1].view(torch.float32)).all())
        results.append(outs)
    assert len(results[0]) == len(results[1]) == 5 * 4 + 2
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ---- the whole network ------------------------------------------------------------------------------------------------------

TENSORS = ["cat0", "cat1", "cat2", "cat3", "s4", "hidden"]


def tensor_of(site):
    return "s4" if site == "enc4" else "hidden" if site == "mlp1" else "cat" + site[3]


def named(inter):
    return {**{f"cat{l}": inter["cat"][l] for l in range(4)}, "s4": inter["s4"], "hidden": inter["hidden"]}


def fresh_model(dev, sd_np, train, trainable=True):
    from umeregrobust_amd.models import ResUNetSmall2
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=trainable)
    m.load_state_dict(torch_state(sd_np))
    return m.to(dev).train(train)


def forward(m, coords, dev, debug=True):
    from umeregrobust_amd.sparse import SparseTensor
    C = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(dev)
    return m(SparseTensor(torch.ones(len(C), 1, device=dev), coordinates=C), debug=debug)


def to_helper_rows(inter, rows):
    """the GPU's intermediates (its level orders) -> CPU fp64 tensors in the helper's row order"""
    out = {}
    for k, v in named(inter).items():
        l = 4 if k == "s4" else 0 if k == "hidden" else int(k[3])
        v = v.detach().cpu()
        out[k] = torch.empty_like(v).index_copy_(0, rows[l], v).double()
    return out


def helper_grads(tables, sd_np, dtype, train, masks, G):
    sd = gref.state(sd_np, dtype)
    out, _ = gref.network(tables, torch.ones(G.shape[0], 1, dtype=dtype), sd, train=train, masks=masks)
    (out * G.to(dtype)).sum().backward()
    return {k: v.grad.double() for k, v in sd.items() if v.requires_grad}


def rel_err(g, truth):
    return {k: float((g[k].double().cpu() - truth[k]).abs().max() / truth[k].abs().max()) for k in truth}


def gradient_gate(e_cpu):
    med = float(np.median(list(e_cpu.values())))
    return {k: 4 * max(v, med) for k, v in e_cpu.items()}


def grad_case(dev, name, train):
    """One cloud, one mode: the GPU's forward + two backward passes, and the helper's runs on the same weights (see the module
    docstring).  Cached: the forward and the gradient tests read the same runs."""
    key = ("case", name, train)
    if key in _cache:
        return _cache[key]
    coords, tables = cloud(name), tables_of(name)
    sd_np = f32_state(seeded())
    n = len(coords)
    G = torch.randn(n, 32, generator=torch.Generator().manual_seed(n), dtype=torch.float32)
    c = {"coords": coords, "tables": tables, "sd": sd_np, "G": G}
    m = fresh_model(dev, sd_np, train)
    res, inter = forward(m, coords, dev)
    c["buffers"] = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    (res.F * G.to(dev)).sum().backward()
    c["g_gpu"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out"], c["inter"], c["res"] = res.F.detach().cpu().double(), inter, res
    m.zero_grad(set_to_none=True)
    res2, _ = forward(m, coords, dev)
    (res2.F * G.to(dev)).sum().backward()
    c["g_gpu_again"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out_again"] = res2.F.detach()
    rows = c["rows"] = row_maps(inter["coords"], tables)
    assert np.array_equal(rows[0].numpy(), inter["perm"].cpu().numpy())
    c["gpu_named"] = to_helper_rows(inter, rows)
    vals = gref.site_values(c["gpu_named"] | {"cat": [c["gpu_named"][f"cat{l}"] for l in range(4)]})
    c["masks"] = {s: vals[s] > 0 for s in gref.RELU_SITES}
    # the helper, free running: fp64 (the truth of the forward pass) and fp32 (the reference-precision forward)
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        sd = gref.state(sd_np, dtype, requires_grad=False)
        with torch.no_grad():
            out, it = gref.network(tables, torch.ones(n, 1, dtype=dtype), sd, train=train)
        c["free" + tag] = (out.double(), {k: v.double() for k, v in named(it).items()}, it, sd)
    # the helper with the GPU's decisions forced: fp64 (the truth of the gradients), fp32 (the yardstick's precision)
    c["g64"] = helper_grads(tables, sd_np, torch.float64, train, c["masks"], G)
    c["g32"] = helper_grads(tables, sd_np, torch.float32, train, c["masks"], G)
    _cache[key] = c
    return c


def forward_gates(c, train):
    """per tensor: the gate of max |gpu - fp64| -- eval: TOL x magnitude (block5 twice); train: 4 x the fp32 helper's own error"""
    t64, t32 = c["free64"][1], c["free32"][1]
    if train:
        return {k: 4 * float((t32[k] - t64[k]).abs().max()) for k in TENSORS}, 4 * float((c["free32"][0] - c["free64"][0]).abs().max())
    return {k: TOL * max(1.0, float(t64[k].abs().max())) * (2 if k == "s4" else 1) for k in TENSORS}, TOL


@pytest.mark.parametrize("name", ["small", "batch2", "KT"])
def test_eval_forward_with_gradients_matches_the_fp64_restatement(gpu, name):
    """9(a): trainable=True, eval mode, gradients enabled (the layer-wise path) within the gates of test_featnet_gpu.py"""
    c = grad_case(gpu, name, False)
    assert c["res"].F.requires_grad and c["res"].F.grad_fn is not None
    assert torch.equal(c["res"].C.cpu(), torch.from_numpy(c["coords"].astype(np.int32)))
    want, want_inter = ref.network(c["coords"], np.ones((len(c["coords"]), 1)), c["sd"])
    err = compare(c["coords"], c["out"].numpy(), c["inter"], want, want_inter)
    scale = {k: max(1.0, float(np.abs(v).max())) for k, v in
             [("cat%d" % l, want_inter["cat"][l]) for l in range(4)] + [("s4", want_inter["s4"]), ("hidden", want_inter["hidden"])]}
    print(f"[trainable eval {name}] n={len(c['coords'])} max|gpu-fp64| " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert err["out"] <= TOL, err
    for k, s in scale.items():
        assert err[k] <= TOL * s * (2 if k == "s4" else 1), (k, err[k], s)
    parts = c["res"].decomposed_features
    assert sum(len(p) for p in parts) == len(c["coords"]) and torch.stack([p[:5] for p in parts], 0).shape[1:] == (5, 32)


@pytest.mark.parametrize("name", ["small", "batch2", "one_cell"])
def test_eval_forward_under_no_grad_is_the_fused_call(gpu, name):
    """9(b): bit-identical to a trainable=False model with the same state dict"""
    sd_np = f32_state(seeded())
    a = fresh_model(gpu, sd_np, False, trainable=True)
    b = fresh_model(gpu, sd_np, False, trainable=False)
    with torch.no_grad():
        ra, ia = forward(a, cloud(name), gpu)
        rb, ib = forward(b, cloud(name), gpu)
    assert not ra.F.requires_grad
    assert ra.F.view(torch.int32).equal(rb.F.view(torch.int32))
    for k in TENSORS:
        assert named(ia)[k].view(torch.int32).equal(named(ib)[k].view(torch.int32)), k


@pytest.mark.parametrize("name", ["small", "batch2", "KT"])
def test_train_forward_matches_the_fp64_helper(gpu, name):
    """9(c): batch statistics amplify rounding, so the gate is the helper's own fp32 error on the same input: max |gpu - fp64| <=
    4 x max |cpu fp32 - fp64| for the output and every intermediate; running statistics within 1e-5 of the fp64 helper's
    (of the tensor's largest magnitude), num_batches_tracked equal."""
    c = grad_case(gpu, name, True)
    gates, gate_out = forward_gates(c, True)
    err = {k: float((c["gpu_named"][k] - c["free64"][1][k]).abs().max()) for k in TENSORS}
    err_out = float((c["out"] - c["free64"][0]).abs().max())
    print(f"[trainable train {name}] max|gpu-fp64| out={err_out:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in err.items())
          + " | gates out=%.2e " % gate_out + " ".join(f"{k}={v:.2e}" for k, v in gates.items()))
    assert err_out <= gate_out, (err_out, gate_out)
    for k in TENSORS:
        assert err[k] <= gates[k], (k, err[k], gates[k])
    sd64 = c["free64"][3]
    worst = 0.0
    for k, v in c["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(sd64[k]) == 1, k
        else:
            e = float((v.double() - sd64[k]).abs().max() / sd64[k].abs().max())
            worst = max(worst, e)
            assert e <= 1e-5, (k, e)
    print(f"[trainable train {name}] running statistics: worst relative difference {worst:.2e}")


def check_gradients(c, train, label):
    # (a) the GPU's ReLU decisions are legitimate
    gates, _ = forward_gates(c, train)
    pre64, mask64 = c["free64"][2]["pre"], c["free64"][2]["mask"]
    flips = {}
    for s in gref.RELU_SITES:
        d = c["masks"][s] != mask64[s]
        flips[s] = int(d.sum())
        if flips[s]:
            worst = float(pre64[s][d].abs().max())
            assert worst <= gates[tensor_of(s)], f"{label} {s}: a decision differs where |fp64 pre-activation| = {worst:.3e} > {gates[tensor_of(s)]:.3e}"
    # (b) every parameter's gradient against fp64, by the yardstick of the fp32 helper
    e_gpu, e_cpu = rel_err(c["g_gpu"], c["g64"]), rel_err(c["g32"], c["g64"])
    gate = gradient_gate(e_cpu)
    assert sorted(e_gpu) == sorted(k for k in SHAPES if "running_" not in k and "num_batches" not in k)
    print(f"[gradients {label}] ReLU decisions other than fp64's: {sum(flips.values())} {({k: v for k, v in flips.items() if v})}; "
          f"e_gpu max {max(e_gpu.values()):.2e} median {np.median(list(e_gpu.values())):.2e}; "
          f"e_cpu max {max(e_cpu.values()):.2e} median {np.median(list(e_cpu.values())):.2e}")
    over = {k: (e_gpu[k], gate[k]) for k in e_gpu if not e_gpu[k] <= gate[k]}
    assert not over, over
    # (c) two backward passes, bit for bit
    assert c["out_again"].cpu().double().equal(c["out"])
    for k, g in c["g_gpu"].items():
        assert g.view(torch.int32).equal(c["g_gpu_again"][k].view(torch.int32)), k
    return e_gpu, e_cpu


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", ["small", "batch2", "KT"])
def test_gradients_match_fp64_autograd_with_the_gpu_s_relu_decisions(gpu, name, train):
    """10(a)-(c): loss (out * G).sum(), G seeded N(0, 1); gate e_gpu <= 4 max(e_cpu, median e_cpu) per parameter"""
    check_gradients(grad_case(gpu, name, train), train, f"{name} {'train' if train else 'eval'}")


def test_batch_gradient_is_the_sum_of_its_clouds(gpu):
    """10(d): eval mode, the two-cloud batch: each gradient equals the sum of the two single-cloud gradients within the gate of
    10(b) (not bit for bit: dW sums over all rows)"""
    c = grad_case(gpu, "batch2", False)
    both = c["coords"]
    total = None
    for i in range(2):
        sel = both[:, 0] == i
        one = both[sel].copy()
        one[:, 0] = 0
        m = fresh_model(gpu, c["sd"], False)
        res = forward(m, one, gpu, debug=False)
        (res.F * c["G"][torch.from_numpy(sel)].to(gpu)).sum().backward()
        g = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
        total = g if total is None else {k: total[k] + g[k] for k in g}
    gate = gradient_gate(rel_err(c["g32"], c["g64"]))
    e = rel_err(total, {k: v.cpu().double() for k, v in c["g_gpu"].items()})
    print(f"[gradients batch2 = cloud 0 + cloud 1] max relative difference {max(e.values()):.2e}")
    for k in e:
        assert e[k] <= gate[k], (k, e[k], gate[k])


def test_one_cell(gpu):
    """13: a single level-4 row -- train mode names the level, eval mode with gradients works and passes 10(b)"""
    coords = cloud("one_cell")
    m = fresh_model(gpu, f32_state(seeded()), True)
    with pytest.raises(ValueError, match="level 4"):
        forward(m, coords, gpu)
    c = grad_case(gpu, "one_cell", False)
    assert c["inter"]["levels"][4] == 1
    check_gradients(c, False, "one_cell eval")


# ---- 11 / 12: a training step is a training step, and the weights come out usable ---------------------------------------------

def training_pair():
    """source / target voxel clouds [., 4] (about 1500 voxels each: a compact piece of the KITTI-test cloud, 15 % dropped on each
    side, the target shifted by (5, -3, 1) voxels) and 256 twin matches (source row, target row)"""
    base = voxel_cloud(0, "KT")
    base = base[np.argsort((base[:, 1:] ** 2).sum(1), kind="stable")[:1765]]
    rng = np.random.default_rng(11)
    keep_s, keep_t = rng.random(len(base)) >= 0.15, rng.random(len(base)) >= 0.15
    src, tgt = base[keep_s], base[keep_t] + np.array([0, 5, -3, 1])
    src_row, tgt_row = np.cumsum(keep_s) - 1, np.cumsum(keep_t) - 1
    twins = np.nonzero(keep_s & keep_t)[0]
    pick = rng.choice(twins, 256, replace=False)
    return src, tgt, np.stack([src_row[pick], tgt_row[pick]], 1).astype(np.int64)


def initial_state(seed):
    from umeregrobust_amd.models import ResUNetSmall2
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in ResUNetSmall2(trainable=True).state_dict().items()}       # drawn on the CPU


def train_25(dev, seed=0, steps=25):
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    src, tgt, matches = training_pair()
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True)
    m.load_state_dict(initial_state(seed))
    m = m.to(dev).train()
    loss_func = MyInfoNCELossNoSeg(tau=0.1, neg_euclid_dist=5)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    st = [SparseTensor(torch.ones(len(c), 1, device=dev), coordinates=torch.from_numpy(c.astype(np.int32)).to(dev)) for c in (src, tgt)]
    src_pts = torch.from_numpy(src[None, :, 1:] * 0.3).float().to(dev)
    mt = torch.from_numpy(matches[None]).to(dev)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        src_feat = torch.stack(m(st[0]).decomposed_features, dim=0)
        tgt_feat = torch.stack(m(st[1]).decomposed_features, dim=0)
        loss = loss_func(src_feat, src_pts, tgt_feat, mt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return m, opt, losses


@pytest.fixture(scope="module")
def trained(gpu):
    return train_25(gpu), train_25(gpu)


def test_a_training_step_is_a_training_step(gpu, trained):
    """11: 25 Adam steps on a twin pair with the point-wise InfoNCE loss.  The CPU restatement in fp32 goes 5.39 -> 0.11 / 0.14 on
    two seeds; a broken gradient does not reach a quarter of the first loss, rounding cannot miss it."""
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    (m, _, losses), (m2, _, losses2) = trained
    src, tgt, matches = training_pair()
    assert 1300 <= len(src) <= 1700 and 1300 <= len(tgt) <= 1700
    # the first step's loss by the helper in fp32 from the same initial numbers
    sd_np = {k: v.numpy() for k, v in initial_state(0).items()}
    feats = []
    with torch.no_grad():
        for c in (src, tgt):
            out, _ = gref.network(gref.Tables(c), torch.ones(len(c), 1), gref.state(sd_np, torch.float32, False), train=True)
            feats.append(out[None])
        want = float(MyInfoNCELossNoSeg(tau=0.1, neg_euclid_dist=5)(feats[0], torch.from_numpy(src[None, :, 1:] * 0.3).float(), feats[1],
                                                                    torch.from_numpy(matches[None])))
    print(f"[training] loss {losses[0]:.4f} -> {losses[-1]:.4f} over {len(losses)} steps; first step by the fp32 helper {want:.6f} "
          f"(relative difference {abs(losses[0] - want) / want:.2e})")
    assert len(losses) == 25 and all(np.isfinite(losses))
    assert abs(losses[0] - want) <= 1e-4 * abs(want)
    assert losses[24] <= losses[0] / 4, losses
    assert losses == losses2
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_the_trained_weights_are_usable(gpu, trained, tmp_path):
    """12: the reference's checkpoint layout, read back into a default model: the fused eval forward agrees with the trainable
    model's layer-wise eval forward within TOL"""
    from umeregrobust_amd.datasets import checkpoint_state_dict
    (m, opt, losses), _ = trained
    sd = m.state_dict()
    assert list(sd) == list(SHAPES) and {k: list(v.shape) for k, v in sd.items()} == SHAPES
    assert int(sd["norm1.bn.num_batches_tracked"]) == 50
    path = tmp_path / "checkpoint_epoch_1.pth"
    torch.save({"epoch": 1, "model_state_dict": sd, "optimizer_state_dict": opt.state_dict(), "total_loss": float(losses[-1])}, path)
    fused = fresh_model(gpu, {k: v.cpu().numpy() for k, v in checkpoint_state_dict(str(path)).items()}, False, trainable=False)
    src, _, _ = training_pair()
    with torch.no_grad():
        a = forward(fused, src, gpu, debug=False).F
    b = forward(m.eval(), src, gpu, debug=False).F
    assert b.requires_grad
    err = float((a - b.detach()).abs().max())
    print(f"[training] fused eval forward of the saved weights against the layer-wise eval forward: max difference {err:.2e}")
    assert err <= TOL
    m.train()
