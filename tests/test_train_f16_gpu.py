"""GPU: the f16-operand training mode (include/umereg_sparse_conv_f16.h) -- `sparse_conv(..., precision="f16")` operator by
operator (exact on small integers, within the rounding bound on N(0, 1) inputs, the backward scaling exact), the raw weight
gradient at its group and segment edges, every parameter gradient of ResUNetSmall2(train_precision="f16") against fp64
autograd by the margins that tests/test_train_f16_cpu.py derives, determinism and ownership, a training run and the driver.

Yardsticks: the fp64 restatement of the contract (tests/featnet_f16_grad_ref.py) and fp64 autograd of the unrounded network
(tests/featnet_grad_ref.py); never the GPU's own output, except where two GPU runs must agree bit for bit."""
import os

import numpy as np
import pytest
import torch

import featnet_f16_grad_ref as g16
import featnet_f16_ref as f16ref
import featnet_grad_ref as gref
import featnet_ref as ref
import test_featnet_f16_gpu as f16g
import test_featnet_gpu as fg
import test_sparse_grad_gpu as sg
import test_train_f16_cpu as tc
from wgrad_cases import block_of, line          # (shared with tests/test_wgrad_edges_gpu.py)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
OPS16 = [op for op in sg.OPS if op[1] >= 32]
_cache = {}


def np16(q):
    return lambda t: torch.from_numpy(np.asarray(q(t.detach().numpy(), "x"))).to(t.dtype)


R16, T16 = np16(f16ref.r16_op), np16(f16ref.t16_op)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1, 2, 3: the operators -------------------------------------------------------------------------------------------------------

def operands(name, t, cin, cout, integer):
    tables = sg.tables_of(name)
    g = torch.Generator().manual_seed(1000 * t + cin + cout)
    x = sg.draw((tables.sizes[gref.in_level(t)], cin), -3, 3, integer, g)
    dy = sg.draw((tables.sizes[gref.out_level(t)], cout), -3, 3, integer, g)
    W = sg.draw((27, cin, cout), -2, 2, integer, g)
    return x, dy, W


def gpu_operator(name, dev, t, x, W, dys):
    """out and, per dY of `dys`, (dx, dw) of sparse_conv(..., precision="f16"), in the helper's row order (on the CPU)"""
    from umeregrobust_amd import sparse_conv as sc
    maps, rows = sg.gpu_maps(name, dev)
    li, lo = gref.in_level(t), gref.out_level(t)
    xg, Wg = x[rows[li]].to(dev).requires_grad_(), W.to(dev).requires_grad_()
    y = sc.sparse_conv(xg, Wg, maps, t, precision="f16")
    grads = []
    for dy in dys:
        dx, dw = torch.autograd.grad(y, (xg, Wg), dy[rows[lo]].to(dev), retain_graph=True)
        grads.append((torch.empty_like(x).index_copy_(0, rows[li], dx.cpu()), dw.cpu()))
    return torch.empty(len(rows[lo]), W.shape[2]).index_copy_(0, rows[lo], y.detach().cpu()), grads


def restated(name, t, x, W, dy, q=f16ref.r16_op):
    """the fp64 restatement -> (out, dx, dw)"""
    x64, W64 = x.double().requires_grad_(), W.double().requires_grad_()
    y = g16.conv(x64, W64, sg.tables_of(name), t, q)
    y.backward(dy.double())
    return y.detach(), x64.grad, W64.grad


@pytest.mark.parametrize("name", ["small", "one_cell"])
def test_operators_are_exact_on_small_integers(gpu, name):
    """X, dY in [-3, 3], W in [-2, 2], integer valued: every operand is exact in f16, dY 2^13 is below 2^15 and every sum is an
    integer below 2^24, so out, dx and dw must EQUAL the fp64 restatement.  The small cloud has 6 weight-gradient segments at
    level 0 (the segment sum); the one-cell cloud has 590 points and a single level-4 row."""
    from umeregrobust_amd import sparse_conv as sc
    assert len(sg.cloud(name)) == (6000 if name == "small" else 590)
    if name == "small":
        assert sc.load_native().umereg_sparse_conv_wgrad_segments(6000, 32, 32) == 6
    for t, cin, cout in OPS16:
        x, dy, W = operands(name, t, cin, cout, True)
        assert g16.scale_exponent(dy) == 13
        out, [(dx, dw)] = gpu_operator(name, gpu, t, x, W, [dy])
        for k, got, want in zip(("out", "dx", "dw"), (out, dx, dw), restated(name, t, x, W, dy)):
            assert float(want.abs().max()) <= max(27 * 256, 6000) * 9 < 2 ** 24       # (the sums of |products| are bounded alike)
            assert torch.equal(got.double(), want), f"{name} table {t} {cin}->{cout} {k}: " \
                f"{int((got.double() != want).sum())} of {want.numel()} elements differ, max {float((got.double() - want).abs().max())}"


def bounds(name, t, x, W, dy, q):
    """per element of (out, dx, dw): gamma(2 L + 2) sum |a_i| |b_i| over the hooked operands, plus for dx and dw the allowance
    2^-14 2^-e sum |x_i| (x_i: the operand that meets the scaled dY) -- the most that flushing a scaled dY below 2^-14 can cost"""
    tables = sg.tables_of(name)
    cin, cout = W.shape[1], W.shape[2]
    xq, Wq = q(x.double()), q(W.double())
    e = g16.scale_exponent(dy)
    dys = q(dy.double() * 2.0 ** e)
    ta, mirror = gref.adjoint(t)
    Wt = gref.repack(Wq.abs(), mirror)
    absum = {"out": gref.conv(xq.abs(), Wq.abs(), tables, t), "dx": gref.conv(dys.abs(), Wt, tables, ta) * 2.0 ** -e}
    allow = {"out": 0.0, "dx": gref.conv(torch.ones_like(dys), Wt, tables, ta) * 2.0 ** (-14 - e)}
    absum["dw"], allow["dw"] = torch.zeros_like(Wq), torch.zeros_like(Wq)
    for k in range(27):
        o, i = tables.pairs[t][k]
        if len(o):
            absum["dw"][k] = xq[i].abs().t() @ dys[o].abs() * 2.0 ** -e
            allow["dw"][k] = (xq[i].abs().sum(0) * 2.0 ** (-14 - e))[:, None]
    L = {"out": gref.chain_lengths(tables, t, cin)[:, None].expand(-1, cout),
         "dx": gref.chain_lengths(tables, ta, cout)[:, None].expand(-1, cin),
         "dw": torch.tensor([len(o) for o, _ in tables.pairs[t]])[:, None, None].expand(-1, cin, cout)}
    out = {}
    for k in absum:
        m = (2 * L[k] + 2).double() * U
        out[k] = (m / (1 - m) * absum[k] + allow[k], L[k])
    return out


def test_operators_stay_within_the_rounding_bound(gpu):
    """N(0, 1) inputs on the small cloud, against the fp64 operator on the ROUNDED operands: |gpu - fp64| <= gamma(2 L + 2)
    sum |a_i| |b_i| per element (u = 2^-24), with the allowance of `bounds` for dx and dw.  Against the fp64 operator on TRUNCATED
    operands the same bound must be exceeded somewhere: otherwise this test could not tell the roundings apart."""
    worst, truncation_seen = {}, False
    for t, cin, cout in OPS16:
        x, dy, W = operands("small", t, cin, cout, False)
        out, [(dx, dw)] = gpu_operator("small", gpu, t, x, W, [dy])
        got = {"out": out, "dx": dx, "dw": dw}
        for q, hook in ((R16, f16ref.r16_op), (T16, f16ref.t16_op)):
            want = dict(zip(("out", "dx", "dw"), restated("small", t, x, W, dy, hook)))
            for k, (bound, L) in bounds("small", t, x, W, dy, q).items():
                err = (got[k].double() - want[k]).abs()
                if hook is f16ref.t16_op:
                    truncation_seen |= bool((err > bound).any())
                    continue
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst[k] = max(worst.get(k, 0.0), ratio)
                assert not bool((err > bound).any()), f"table {t} {cin}->{cout} {k}: {int((err > bound).sum())} elements over the bound, worst ratio {ratio:.3g}"
                assert bool(((L == 0) <= (got[k] == 0)).all()), "an element without a chain is not zero"
    print("[sparse_conv f16 rounding small] worst |err| / bound: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert truncation_seen, "the bound does not tell round-to-nearest from truncation"


SCALE_OPS = [(0, 32, 32), (6, 64, 64), (10, 192, 64)]


@pytest.mark.parametrize("op", SCALE_OPS, ids=lambda op: "t%d_%d_%d" % op)
def test_backward_scaling_works_and_is_exact(gpu, op):
    """The dY of the rounding test: backward(dY 2^-40) and backward(dY 2^30) equal backward(dY) times the same power bit for bit
    (unscaled, dY 2^-40 is zero in f16); rows of dY scaled by 2^-j, j uniform in [0, 20], stay within the bound with its
    allowance; dY = 0 gives exact zeros; one infinite dY gives a non-finite gradient and a normal return."""
    t, cin, cout = op
    x, dy, W = operands("small", t, cin, cout, False)
    assert float(f16ref.r16((dy * 2.0 ** -40).numpy()).max()) == 0.0
    j = torch.randint(0, 21, (dy.shape[0], 1), generator=torch.Generator().manual_seed(t))
    rowwise = dy * torch.ldexp(torch.ones(()), -j)
    inf = dy.clone()
    inf[len(inf) // 2, 3] = float("inf")
    _, grads = gpu_operator("small", gpu, t, x, W, [dy, dy * 2.0 ** -40, dy * 2.0 ** 30, rowwise, torch.zeros_like(dy), inf])
    (dx, dw), (dx_s, dw_s), (dx_b, dw_b), (dx_r, dw_r), (dx_0, dw_0), (dx_i, dw_i) = grads
    assert float(dx.abs().max()) > 0 and float(dw.abs().max()) > 0
    for p, (a, b) in ((-40, (dx_s, dw_s)), (30, (dx_b, dw_b))):
        assert bits(a).equal(bits(dx * 2.0 ** p)) and bits(b).equal(bits(dw * 2.0 ** p)), p
    want = dict(zip(("out", "dx", "dw"), restated("small", t, x, W, rowwise)))
    for k, got in (("dx", dx_r), ("dw", dw_r)):
        bound, _ = bounds("small", t, x, W, rowwise, R16)[k]
        err = (got.double() - want[k]).abs()
        assert not bool((err > bound).any()), f"{k}: worst ratio {float((err / bound.clamp_min(1e-300)).max()):.3g}"
    for z in (dx_0, dw_0):
        assert bool((z == 0).all())
    assert not bool(torch.isfinite(dx_i).all()) and not bool(torch.isfinite(dw_i).all())


# ---- 4: groups of 16, empty offsets, one and two segments ---------------------------------------------------------------------------

EDGE_CLOUDS = {**{f"line{m}": (lambda m=m: line(m)) for m in (1, 2, 16, 17, 18, 33)}, "isolated": lambda: fg.edge_cloud("isolated"),
               "rows1024": lambda: block_of(1024), "rows1025": lambda: block_of(1025)}


@pytest.mark.parametrize("name", list(EDGE_CLOUDS))
def test_weight_gradient_at_group_and_segment_edges(gpu, name):
    """umereg_sparse_conv_wgrad_f16 over table 0, integer data: equal to fp64, and dW[k] of an offset without pairs exactly zero.
    A line of m points along x has m pairs at the centre and m - 1 at (+-1, 0, 0): both sides of one and two full groups of 16;
    isolated points have the centre only; 1 024 / 1 025 level-0 rows are one / two segments."""
    from umeregrobust_amd import sparse_conv as sc
    coords = EDGE_CLOUDS[name]()
    n = len(coords)
    tables = gref.Tables(coords, tables=[0])
    pairs = [len(o) for o, _ in tables.pairs[0]]
    if name.startswith("line"):
        assert pairs[13] == n and pairs[12] == pairs[14] == n - 1 and sum(pairs) == 3 * n - 2
    if name == "isolated":
        assert sum(pairs) == pairs[13] == n
    lib = sc.load_native()
    if name.startswith("rows"):
        assert lib.umereg_sparse_conv_wgrad_segments(n, 32, 64) == (1 if n == 1024 else 2)
    maps = sc.CoordinateMaps(torch.from_numpy(coords.astype(np.int32)).to(gpu), 1)
    perm = maps.perm.cpu()
    g = torch.Generator().manual_seed(n)
    for cin, cout in ((32, 64), (64, 32)):
        x = sg.draw((n, cin), -3, 3, True, g)
        dy = sg.draw((n, cout), -3, 3, True, g) * 2.0 ** 12                      # (scaled by the caller, as the entry expects)
        dw = sc.wgrad_raw(x[perm].to(gpu), dy[perm].to(gpu), maps, 0, precision="f16").cpu()
        for k in range(27):
            o, i = tables.pairs[0][k]
            want = x[i].double().t() @ dy[o].double() if len(o) else torch.zeros(cin, cout, dtype=torch.float64)
            assert torch.equal(dw[k].double(), want), (name, cin, cout, k, len(o))
            if not len(o):
                assert bits(dw[k]).eq(0).all()


# ---- 5: whole-network gradients -----------------------------------------------------------------------------------------------------

def model_f16(dev, sd_np, train):
    from umeregrobust_amd.models import ResUNetSmall2
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, train_precision="f16")
    m.load_state_dict(fg.torch_state(sd_np))
    return m.to(dev).train(train)


def grad_case(dev, name, train):
    """One cloud, one mode: the GPU's forward and two backward passes with train_precision="f16", and the fp64 references with
    the GPU run's ReLU decisions forced onto them.  Cached and left unchanged."""
    key = ("case", name, train)
    if key in _cache:
        return _cache[key]
    coords = tc.NET_CLOUDS[name]()
    tables, n = gref.Tables(coords), len(coords)
    sd_np = fg.f32_state(fg.seeded())
    G = torch.randn(n, 32, generator=torch.Generator().manual_seed(n), dtype=torch.float32)
    c = {"coords": coords, "tables": tables, "sd": sd_np, "G": G}
    m = model_f16(dev, sd_np, train)
    res, inter = sg.forward(m, coords, dev)
    assert res.F.requires_grad
    (res.F * G.to(dev)).sum().backward()
    c["g_gpu"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out"], c["inter"] = res.F.detach().cpu(), inter
    m.zero_grad(set_to_none=True)
    if train:                                            # (the second pass sees the same running statistics)
        m.load_state_dict(fg.torch_state(sd_np))
    res2, _ = sg.forward(m, coords, dev)
    (res2.F * G.to(dev)).sum().backward()
    c["g_gpu_again"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    c["out_again"] = res2.F.detach().cpu()
    rows = sg.row_maps(inter["coords"], tables)
    named = sg.to_helper_rows(inter, rows)
    vals = gref.site_values(named | {"cat": [named[f"cat{l}"] for l in range(4)]})
    c["masks"] = {s: vals[s] > 0 for s in gref.RELU_SITES}
    c["g64"] = tc.helper_grads(gref.network, tables, sd_np, torch.float64, train, c["masks"], G)
    c["G16"] = tc.helper_grads(g16.network, tables, sd_np, torch.float64, train, c["masks"], G)
    _cache[key] = c
    return c


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", list(tc.NET_CLOUDS))
def test_gradients_carry_the_contract_s_error(gpu, name, train):
    """Per parameter, with G64 = fp64 autograd of the unrounded network, G16 = fp64 autograd through the restatement and GE16 =
    G16 - G64:  rms(g_gpu - G64) <= M_RMS rms(GE16)  and  max |g_gpu - G64| <= M_MAX max |GE16|.
    Margins (tests/test_train_f16_cpu.py, worst parameter over the same four cases): the restatement in fp32 reaches rms 1.24 and
    max 1.41, truncated operands reach at least rms 2.23 and max 1.99; M_RMS = M_MAX = 1.7 lie between.  Measured on the MI355X:
    rms 1.08 ... 1.32, max 1.36 ... 1.60, median rms ratio 0.98 ... 1.01."""
    c = grad_case(gpu, name, train)
    assert sorted(c["g_gpu"]) == sorted(c["g64"])
    e = tc.gradient_errors(c["g_gpu"], c["g64"], c["G16"])
    r, m = max(v[0] for v in e.values()), max(v[1] for v in e.values())
    print(f"[f16 training gradients {name} {'train' if train else 'eval'}] worst parameter: rms ratio {r:.3f} max ratio {m:.3f}; median "
          f"rms ratio {np.median([v[0] for v in e.values()]):.3f}")
    over = {k: v for k, v in e.items() if not (v[0] <= tc.M_RMS and v[1] <= tc.M_MAX)}
    assert not over, over


@pytest.mark.parametrize("name", list(tc.NET_CLOUDS))
def test_layer_wise_eval_forward_carries_the_contract_s_error(gpu, name):
    """The forward of the eval-mode runs above against tests/featnet_f16_ref.py: rms <= 1.25 rms(E16), max <= 1.5 max |E16| on the
    output, cat0..3, s4 and hidden (the gates of tests/test_featnet_f16_gpu.py: the layer-wise path differs from the fused one by
    f32-sized terms only)."""
    c = grad_case(gpu, name, False)
    check_e16(c["coords"], c["out"].numpy(), c["inter"], c["sd"], f"layer-wise eval {name}")


def check_e16(coords, out, inter, sd, label):
    feat = np.ones((len(coords), 1))
    want, want_inter = ref.network(coords, feat, sd)
    w16 = f16ref.flat(*f16ref.network(coords, feat, sd))
    det = lambda v: v.detach() if torch.is_tensor(v) else v        # noqa: E731  (the layer-wise path's intermediates carry graphs)
    inter = {k: [det(t) for t in v] if isinstance(v, list) else det(v) for k, v in inter.items()}
    err, _, _ = f16g.errors(coords, out, inter, want, want_inter)
    truth = f16ref.flat(want, want_inter)
    line, fails = [], []
    for k in f16ref.NAMES:
        e16 = w16[k] - truth[k]
        r_rms, r_max = f16ref.rms(err[k]) / f16ref.rms(e16), float(np.abs(err[k]).max() / np.abs(e16).max())
        line.append(f"{k}: rms {r_rms:.4f} max {r_max:.4f}")
        if r_rms > f16g.RMS_GATE or r_max > f16g.MAX_GATE:
            fails.append((k, r_rms, r_max))
    print(f"[f16 training {label}] (gpu - fp64) / E16: " + " | ".join(line))
    assert not fails, fails


# ---- 6: determinism and ownership ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_two_backward_passes_agree_bit_for_bit(gpu, train):
    c = grad_case(gpu, "small", train)
    assert bits(c["out"]).equal(bits(c["out_again"]))
    for k, g in c["g_gpu"].items():
        assert bits(g).equal(bits(c["g_gpu_again"][k])), k


PAD, CANARY = 4096, 0xA5


def test_raw_entry_between_guard_bands_and_its_argument_errors(gpu):
    """umereg_sparse_conv_wgrad_f16 with dW and scratch between 4 KiB canaries at exactly the sizes the header states, twice with
    different garbage in the scratch: bands intact, results equal bit for bit.  C_in = 1, channel counts that are no multiple of
    32, a short scratch and a table out of range are refused before any launch: dW keeps its poison."""
    from umeregrobust_amd import sparse_conv as sc
    lib = sc.load_native()
    maps, rows = sg.gpu_maps("small", gpu)
    tables = sg.tables_of("small")
    stream = torch.cuda.current_stream(gpu).cuda_stream
    ws = (maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n)
    for t, cin, cout in ((0, 32, 32), (5, 32, 64), (10, 192, 64), (4, 256, 256)):
        g = torch.Generator().manual_seed(t)
        x = torch.randn(tables.sizes[gref.in_level(t)], cin, generator=g).to(gpu)
        dy = (torch.randn(tables.sizes[gref.out_level(t)], cout, generator=g) * 2.0 ** 12).to(gpu)
        sc_bytes, dw_bytes = lib.umereg_sparse_conv_wgrad_scratch_bytes(maps.n, cin, cout), 27 * cin * cout * 4
        assert sc_bytes == lib.umereg_sparse_conv_wgrad_segments(maps.n, cin, cout) * dw_bytes
        results = []
        for garbage in (0xEE, 0x17):
            bufs = []
            for nbytes, fill in ((dw_bytes, 0xCD), (sc_bytes, garbage)):
                full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=gpu)
                full[:PAD] = CANARY
                full[PAD + nbytes:] = CANARY
                full[PAD:PAD + nbytes] = fill
                bufs.append(full)
            dW, scratch = bufs
            call = lambda table=t, ci=cin, co=cout, ld_in=cin, sb=sc_bytes: lib.umereg_sparse_conv_wgrad_f16(        # noqa: E731
                *ws, table, x.data_ptr(), ld_in, ci, dy.data_ptr(), cout, co, dW.data_ptr() + PAD, scratch.data_ptr() + PAD, sb, stream)
            assert call(ci=1, ld_in=1) == -1 and call(ci=48) == -1 and call(co=cout + 16) == -1 and call(table=13) == -1
            assert call(table=-1) == -1 and call(sb=sc_bytes - 1) == -3
            torch.cuda.synchronize()
            assert bool((dW[PAD:PAD + dw_bytes] == 0xCD).all()), "a refused call wrote dW"
            assert call() == 0, lib.umereg_last_error()
            torch.cuda.synchronize()
            for full, nbytes in ((dW, dw_bytes), (scratch, sc_bytes)):
                assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nbytes:] == CANARY).all()), "a guard band was written"
            results.append(dW[PAD:PAD + dw_bytes].clone())
        assert torch.equal(results[0], results[1]), (t, cin, cout)
        assert bool(torch.isfinite(results[0].view(torch.float32)).all())


def test_batch_gradient_is_the_sum_of_its_clouds(gpu):
    """eval mode, the batch of two 3 000-point clouds: each gradient equals the sum of the two single-cloud gradients within the
    f32 gate of test_sparse_grad_gpu.test_batch_gradient_is_the_sum_of_its_clouds, 4 max(e_cpu, median e_cpu) with e_cpu the fp32
    helper's own relative error (a power-of-two scale commutes with the rounding, so the clouds' other exponents cost nothing)."""
    c = grad_case(gpu, "two_3000", False)
    both = c["coords"]
    total = None
    for i in range(2):
        sel = both[:, 0] == i
        one = both[sel].copy()
        one[:, 0] = 0
        m = model_f16(gpu, c["sd"], False)
        res = sg.forward(m, one, gpu, debug=False)
        (res.F * c["G"][torch.from_numpy(sel)].to(gpu)).sum().backward()
        g = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
        total = g if total is None else {k: total[k] + g[k] for k in g}
    g32 = tc.helper_grads(gref.network, c["tables"], c["sd"], torch.float32, False, c["masks"], c["G"])
    gate = sg.gradient_gate(sg.rel_err(g32, c["g64"]))
    e = sg.rel_err(total, {k: v.cpu().double() for k, v in c["g_gpu"].items()})
    print(f"[f16 training gradients two_3000 = cloud 0 + cloud 1] max relative difference {max(e.values()):.2e}")
    for k in e:
        assert e[k] <= gate[k], (k, e[k], gate[k])


# ---- 7: it trains ---------------------------------------------------------------------------------------------------------------------

def train_25(dev, train_precision, seed=0, steps=25):
    """test_sparse_grad_gpu.train_25 with the `train_precision` keyword"""
    from umeregrobust_amd.loss import MyInfoNCELossNoSeg
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    src, tgt, matches = sg.training_pair()
    m = ResUNetSmall2(in_channels=1, out_channels=32, trainable=True, train_precision=train_precision)
    m.load_state_dict(sg.initial_state(seed))
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


def test_it_trains_and_the_checkpoint_serves_f16_inference(gpu, tmp_path):
    """25 Adam steps on the twin pair of test_sparse_grad_gpu.py: two f16 runs end in bit-identical parameters, the loss is finite
    throughout, and the final loss is at most 2 x the f32 run's made here (the two roundings' trajectories diverge; the loss falls
    by a factor of about 50, so a factor of 2 still shows training).  The saved checkpoint runs in ResUNetSmall2(precision="f16")
    under no_grad within the E16 gates, as does the trained model's own layer-wise eval forward."""
    from umeregrobust_amd.datasets import checkpoint_state_dict
    from umeregrobust_amd.models import ResUNetSmall2
    (m, opt, losses), (m2, _, losses2) = train_25(gpu, "f16"), train_25(gpu, "f16")
    _, _, losses32 = train_25(gpu, "f32")
    print(f"[f16 training] loss {losses[0]:.4f} -> {losses[-1]:.4f}; f32 {losses32[0]:.4f} -> {losses32[-1]:.4f} over {len(losses)} steps")
    assert len(losses) == 25 and all(np.isfinite(losses)) and all(np.isfinite(losses32))
    assert losses == losses2
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert losses32[-1] <= losses32[0] / 4
    assert losses[-1] <= 2 * losses32[-1], (losses[-1], losses32[-1])
    sd = m.state_dict()
    assert list(sd) == list(fg.SHAPES) and all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    path = tmp_path / "checkpoint_epoch_1.pth"
    torch.save({"epoch": 1, "model_state_dict": sd, "optimizer_state_dict": opt.state_dict(), "total_loss": float(losses[-1])}, path)
    loaded = checkpoint_state_dict(str(path))
    fused = ResUNetSmall2(in_channels=1, out_channels=32, precision="f16")
    fused.load_state_dict(loaded)
    fused = fused.to(gpu).eval()
    src, _, _ = sg.training_pair()
    sd_np = fg.f32_state({k: v.cpu().numpy() for k, v in loaded.items()})
    res, inter = fg.run(fused, src, gpu, debug=True)
    check_e16(src, res.F.cpu().numpy(), inter, sd_np, "fused f16 forward of the trained checkpoint")
    res, inter = sg.forward(m.eval(), src, gpu)
    assert res.F.requires_grad
    check_e16(src, res.F.detach().cpu().numpy(), inter, sd_np, "layer-wise eval forward of the trained model")


# ---- 8: the driver --------------------------------------------------------------------------------------------------------------------

def test_driver_runs_an_epoch_with_f16_operands(gpu, tmp_path):
    """`--synthetic 4 --epochs 1 --train-precision f16` (main -> run(synthetic=4, ..., train_precision="f16")): the epoch completes
    and writes a checkpoint whose keys and dtypes equal the f32 run's"""
    from umeregrobust_amd import train_coloring as tcol
    files = {}
    for tp in ("f32", "f16"):
        run_dir = tcol.main(["--synthetic", "4", "--epochs", "1", "--output-path", str(tmp_path / tp), "--train-precision", tp])
        files[tp] = torch.load(os.path.join(run_dir, "last_epoch_checkpoint.pth"), weights_only=True)
    a, b = files["f32"], files["f16"]
    assert sorted(a) == sorted(b)
    sa, sb = a["model_state_dict"], b["model_state_dict"]
    assert list(sa) == list(sb) == list(fg.SHAPES)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape, k
        assert bool(torch.isfinite(sb[k].double()).all()), k
    assert np.isfinite(b["total_loss"])
