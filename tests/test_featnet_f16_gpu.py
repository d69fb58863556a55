"""GPU: the f16-operand inference mode of ResUNetSmall2 (include/umereg_featnet_f16.h; `precision="f16"`).

1 / 2 judge the single convolution against the fp64 restatement of the contract (operands rounded to f16, exact products):
exactly on integer data, and within the forward bound of an inner product on N(0, 1) data -- no tolerance comes from the code
under test.  3 gates the whole network against E16 = (rounded network) - (fp64 network), computed here on the CPU by
tests/featnet_f16_ref.py; the two margins (1.25 on rms, 1.5 on max) are derived in tests/test_featnet_f16_cpu.py.  4-8:
determinism, the untouched f32 path, guard bands, the range bit and the plumbing."""
import functools
import os

import numpy as np
import pytest
import torch

import featnet_f16_ref as f16ref
import featnet_ref as ref
import test_featnet_gpu as fg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMS_GATE, MAX_GATE, F32_TOL = 1.25, 1.5, 2e-6
U = 2.0 ** -24

# layer of the packed block -> neighbour table (self l = l, strided l -> l+1 = 5 + l, transposed l+1 -> l = 9 + l; -1 = the 1x1
# layer over level 0): the seventeen 27-offset layers after conv1 (every (C_in, C_out) shape of the network) and mlp1
LAYER_TABLE = {1: 0, 2: 5, 3: 1, 4: 6, 5: 2, 6: 7, 7: 3, 8: 8, 9: 4, 10: 12, 11: 3, 12: 11, 13: 2, 14: 10, 15: 1, 16: 9, 17: 0, 18: -1}


def kt6000():
    return fg.voxel_cloud(0, "KT")[:6000]


def batch2():
    return np.concatenate([fg.voxel_cloud(3, "NS")[:3000], fg.voxel_cloud(4, "KT", batch=1)[:3000]])


CASES = {"one_point": lambda: fg.edge_cloud("one_point"), "one_cell": lambda: fg.edge_cloud("one_cell"),
         "isolated": lambda: fg.edge_cloud("isolated"), "kt6000": kt6000, "batch2": batch2}
CASES.update({f"n{n}": (lambda n=n: fg.voxel_cloud(0, "KT")[:n]) for n in (63, 64, 65, 127, 128, 129)})

_f16_models = {}


def model16(dev, seed=42):
    from umeregrobust_amd.models import ResUNetSmall2
    if (dev, seed) not in _f16_models:
        m = ResUNetSmall2(in_channels=1, out_channels=32, precision="f16")
        m.load_state_dict(fg.torch_state(fg.seeded(seed)))
        _f16_models[(dev, seed)] = m.eval().to(dev)
    return _f16_models[(dev, seed)]


@functools.lru_cache(maxsize=None)
def references(case):
    """(coords, fp64 network, rounded network) of a case, computed once and left unchanged"""
    coords = CASES[case]()
    feat, sd = np.ones((len(coords), 1)), fg.f32_state(fg.seeded(42))
    return coords, ref.network(coords, feat, sd), f16ref.network(coords, feat, sd)


# ---- 1, 2: the operator -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def maps_of(name, dev):
    from umeregrobust_amd import sparse_conv as sc
    coords = {"one_cell": lambda: fg.edge_cloud("one_cell"), "kt6000": kt6000}[name]()
    assert len(coords) == (590 if name == "one_cell" else 6000)
    maps = sc.CoordinateMaps(torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(dev), 1)
    levels = [maps.level_coords(l).cpu().numpy().astype(np.int64) for l in range(5)]
    return maps, levels, [ref.Index(c) for c in levels]


def table_geometry(table):
    """-> (input level, output level, tensor stride of the offsets, transposed)"""
    if table < 0:
        return 0, 0, 1, False
    if table < 5:
        return table, table, ref.TSTRIDES[table], False
    if table < 9:
        return table - 5, table - 4, ref.TSTRIDES[table - 5], False
    return table - 8, table - 9, ref.TSTRIDES[table - 9], True


def conv64(x, W, levels, index, table):
    li, lo, ts, tr = table_geometry(table)
    return ref.conv(x, levels[li], levels[lo], W, ts, transposed=tr, index=index[li])


def conv_f16(maps, table, x, ld_in, W, cin, cout, out, ld_out, accumulate, x_col=0):
    """umereg_sparse_conv_f16 through the C ABI: x / out are [rows, ld] f32 tensors, the input slice starts at column x_col"""
    from umeregrobust_amd import _lib, sparse_conv as sc
    lib = sc.load_native()
    rc = lib.umereg_sparse_conv_f16(maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, table, x.data_ptr() + 4 * x_col,
                                    ld_in, W.data_ptr(), cin, cout, maps.ones.data_ptr(), maps.zeros.data_ptr(), out.data_ptr(), ld_out,
                                    accumulate, torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "sparse_conv_f16")


def layer_shape(layer):
    from umeregrobust_amd import models
    K, cin, cout, _, _ = models.layer_info()[layer]
    return K, cin, cout


@pytest.mark.parametrize("layer", sorted(LAYER_TABLE))
def test_operator_is_exact_on_integer_data(gpu, layer):
    """Inputs in [-8, 8], weights in [-4, 4], scale 1, shift 0: every operand is exact in f16 and every term and partial sum stays
    below 27 x 256 x 32 < 2^24, so the f32 chain is exact whatever its order and the output must EQUAL the fp64 restatement --
    a wrong row, offset, channel group or k order cannot hide.  Rows of ld_in > C_in and ld_out > C_out (the padding poisoned),
    and the same contraction cut into two channel slices with `accumulate`."""
    K, cin, cout = layer_shape(layer)
    table = LAYER_TABLE[layer]
    rng = np.random.default_rng(100 + layer)
    for name in ("one_cell", "kt6000"):
        maps, levels, index = maps_of(name, gpu)
        li, lo, _, _ = table_geometry(table)
        rows_in, rows_out = len(levels[li]), len(levels[lo])
        x = rng.integers(-8, 9, (rows_in, cin)).astype(np.float64)
        W = rng.integers(-4, 5, (K, cin, cout) if K > 1 else (cin, cout)).astype(np.float64)
        want = conv64(x, W, levels, index, table)
        assert np.abs(want).max() < 2 ** 24
        ld_in, ld_out = cin + 8, cout + 5
        xd = torch.full((rows_in, ld_in), 1e30, dtype=torch.float32, device=gpu)
        xd[:, :cin] = torch.from_numpy(x).float().to(gpu)
        Wd = torch.from_numpy(W).float().to(gpu).contiguous()
        out = torch.full((rows_out, ld_out), float("nan"), dtype=torch.float32, device=gpu)
        conv_f16(maps, table, xd, ld_in, Wd, cin, cout, out, ld_out, 0)
        got = out.cpu().numpy()
        assert np.isnan(got[:, cout:]).all(), "the padding of the output rows was written"
        assert np.array_equal(got[:, :cout].astype(np.float64), want), f"{name} layer {layer}: {cin}->{cout} over table {table}"
        if cin >= 64:           # two channel slices, each with its own contiguous kernel block, added in call order
            s0 = 32
            out2 = torch.full((rows_out, ld_out), float("nan"), dtype=torch.float32, device=gpu)
            for c0, c1, acc in ((0, s0, 0), (s0, cin, 1)):
                Ws = torch.from_numpy(np.ascontiguousarray(W[..., c0:c1, :])).float().to(gpu)
                conv_f16(maps, table, xd, ld_in, Ws, c1 - c0, cout, out2, ld_out, acc, x_col=c0)
            got2 = out2.cpu().numpy()
            assert np.isnan(got2[:, cout:]).all() and np.array_equal(got2[:, :cout].astype(np.float64), want), f"{name} layer {layer}: slices"


def test_operator_python_entry_reaches_the_f16_kernel(gpu):
    """sparse_conv.conv_raw(..., precision="f16"): the 27-offset form, the 1x1 form (table -1), and the f32 default beside it"""
    from umeregrobust_amd import sparse_conv as sc
    maps, levels, index = maps_of("one_cell", gpu)
    rng = np.random.default_rng(7)
    x = rng.integers(-8, 9, (len(levels[0]), 96)).astype(np.float64)
    W3, W1 = rng.integers(-4, 5, (27, 96, 64)).astype(np.float64), rng.integers(-4, 5, (96, 64)).astype(np.float64)
    xd = torch.from_numpy(x).float().to(gpu)
    for W, table in ((W3, 0), (W1, -1)):
        got = sc.conv_raw(xd, torch.from_numpy(W).float().to(gpu), maps, table, precision="f16").cpu().numpy().astype(np.float64)
        assert np.array_equal(got, conv64(x, W, levels, index, table))
    # a value that f16 cannot hold exactly tells the two precisions apart
    xo = torch.full_like(xd, 1.0 + 2.0 ** -12)
    a = sc.conv_raw(xo, torch.from_numpy(W3).float().to(gpu), maps, 0).cpu().numpy().astype(np.float64)
    b = sc.conv_raw(xo, torch.from_numpy(W3).float().to(gpu), maps, 0, precision="f16").cpu().numpy().astype(np.float64)
    assert np.array_equal(b, conv64(np.ones_like(x), W3, levels, index, 0)) and not np.array_equal(a, b)
    with pytest.raises(ValueError):
        sc.conv_raw(xd, torch.from_numpy(W1).float().to(gpu), maps, 0, precision="f16")


@pytest.mark.parametrize("layer", sorted(LAYER_TABLE))
def test_operator_stays_within_the_rounding_bound(gpu, layer):
    """N(0, 1) inputs, He-scaled weights, against the fp64 convolution of r16(in) and r16(W): per element |err| <= gamma(2 L + 2)
    sum |a_i| |b_i|, gamma(m) = m u / (1 - m u), u = 2^-24, L the products of the element's chain -- the forward bound of an inner
    product summed in f32 in any order (the products of two f16 values are exact in f32), so it holds whatever the 16-term
    instruction does inside.  The f32 operator's worst ratio in this form is 0.31 (tests/test_sparse_grad_gpu.py).  Operands
    rounded by truncation miss the bound on the elements with short chains (their error grows like 2^-11 sqrt(L), the bound like
    2^-23 L); that ratio is printed beside the measured one.  Measured worst ratios: DESIGN.md 4.8."""
    K, cin, cout = layer_shape(layer)
    table = LAYER_TABLE[layer]
    rng = np.random.default_rng(200 + layer)
    worst = worst_trunc = 0.0
    for name in ("one_cell", "kt6000"):
        maps, levels, index = maps_of(name, gpu)
        li, lo, _, _ = table_geometry(table)
        rows_in, rows_out = len(levels[li]), len(levels[lo])
        x = rng.standard_normal((rows_in, cin)).astype(np.float32)
        W = (rng.standard_normal((K, cin, cout) if K > 1 else (cin, cout)) * np.sqrt(2.0 / (K * cin))).astype(np.float32)
        xq, Wq = f16ref.r16(x), f16ref.r16(W)
        want = conv64(xq, Wq, levels, index, table)
        absum = conv64(np.abs(xq), np.abs(Wq), levels, index, table)
        cnt = conv64(np.ones((rows_in, 1)), np.ones((K, 1, 1) if K > 1 else (1, 1)), levels, index, table)
        m = (2 * cnt * cin + 2) * U
        bound = m / (1 - m) * absum
        out = torch.full((rows_out, cout), float("nan"), dtype=torch.float32, device=gpu)
        conv_f16(maps, table, torch.from_numpy(x).to(gpu), cin, torch.from_numpy(W).to(gpu), cin, cout, out, cout, 0)
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        # what truncated operands would leave (for the record, no gate): the elements with the shortest chains tell the roundings apart
        trunc = np.abs(conv64(f16ref.t16(x), f16ref.t16(W), levels, index, table) - want)
        worst_trunc = max(worst_trunc, float((trunc / np.maximum(bound, 1e-300)).max()))
        bad = err > bound
        assert not bad.any(), f"{name} layer {layer} {cin}->{cout}: {int(bad.sum())} elements over the bound, worst ratio {ratio:.3g}"
    print(f"[sparse_conv_f16 rounding] layer {layer} ({cin}->{cout}, table {table}): worst |err| / bound {worst:.3f} "
          f"(truncated operands on the CPU: {worst_trunc:.1f})")


# ---- 3: the network ---------------------------------------------------------------------------------------------------------------

def errors(coords, out, inter, want, want_inter):
    """{name: gpu - fp64 (rows matched by coordinate)} over the output and the intermediates, with the f32 tests' checks of the
    level row counts, the coordinates and perm"""
    d = {"out": out - want}
    rows = []
    for l in range(5):
        gc = inter["coords"][l].cpu().numpy().astype(np.int64)
        assert len(gc) == len(want_inter["coords"][l]) == inter["levels"][l], f"level {l}: {len(gc)} rows"
        idx = ref.Index(want_inter["coords"][l]).find(gc)
        assert (idx >= 0).all() and len(np.unique(idx)) == len(idx), f"level {l}: coordinates differ"
        rows.append(idx)
    for l in range(4):
        d[f"cat{l}"] = inter["cat"][l].cpu().numpy() - want_inter["cat"][l][rows[l]]
    d["s4"] = inter["s4"].cpu().numpy() - want_inter["s4"][rows[4]]
    perm = inter["perm"].cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(len(coords)))
    assert np.array_equal(inter["coords"][0].cpu().numpy(), coords[perm].astype(np.int32))
    d["hidden"] = inter["hidden"].cpu().numpy() - want_inter["hidden"][perm]
    return d, rows, perm


@pytest.mark.parametrize("case", list(CASES))
def test_network_error_is_the_contracts(gpu, case):
    """For the output and each of cat0..3, s4 and hidden: rms(gpu - fp64) <= 1.25 rms(E16) and max |gpu - fp64| <= 1.5 max |E16|,
    E16 = rounded network - fp64 network (tests/featnet_f16_ref.py; margins: tests/test_featnet_f16_cpu.py).  Where E16 is zero the
    GPU must equal fp64 within the f32 gate."""
    coords, (want, want_inter), (w16, w16_inter) = references(case)
    res, inter = fg.run(model16(gpu), coords, gpu, debug=True)
    assert torch.equal(res.C.cpu(), torch.from_numpy(coords.astype(np.int32)))
    err, _, _ = errors(coords, res.F.cpu().numpy(), inter, want, want_inter)
    e16 = {k: v - f16ref.flat(want, want_inter)[k] for k, v in f16ref.flat(w16, w16_inter).items()}
    mags = f16ref.flat(want, want_inter)
    line, fails = [], []
    for k in f16ref.NAMES:
        e_rms, e_max = f16ref.rms(err[k]), float(np.abs(err[k]).max())
        r_rms, r_max = f16ref.rms(e16[k]), float(np.abs(e16[k]).max())
        if r_max == 0.0:
            tol = F32_TOL * (1.0 if k == "out" else max(1.0, float(np.abs(mags[k]).max())))
            line.append(f"{k}: E16=0 max {e_max:.2e}")
            if e_max > tol:
                fails.append((k, e_max, tol))
        else:
            line.append(f"{k}: rms {e_rms / r_rms:.4f} max {e_max / r_max:.4f}")
            if e_rms > RMS_GATE * r_rms or e_max > MAX_GATE * r_max:
                fails.append((k, e_rms / r_rms, e_max / r_max))
    print(f"[featnet f16 {case}] n={len(coords)} levels={inter['levels']} (gpu - fp64) / E16: " + " | ".join(line)
          + f" | E16 out rms {f16ref.rms(e16['out']):.2e} max {np.abs(e16['out']).max():.2e}")
    assert not fails, fails


# ---- 4: determinism ---------------------------------------------------------------------------------------------------------------

def bits(t):
    return t.contiguous().view(torch.int32)


def test_runs_agree_a_batch_equals_its_clouds_and_rows_permute(gpu):
    m = model16(gpu)
    both = batch2()
    a, b = fg.run(m, both, gpu).F, fg.run(m, both, gpu).F
    assert bits(a).equal(bits(b))
    parts = fg.run(m, both, gpu).decomposed_features
    for i in range(2):
        one = both[both[:, 0] == i].copy()
        one[:, 0] = 0
        assert bits(fg.run(m, one, gpu).F).equal(bits(parts[i])), f"cloud {i}"
    p = np.random.default_rng(9).permutation(len(both))
    c = fg.run(m, both[p], gpu).F
    assert bits(c).equal(bits(a[torch.from_numpy(p).to(gpu)]))


# ---- 5: the f32 path is untouched -------------------------------------------------------------------------------------------------

def test_f32_forward_is_the_same_bits_around_an_f16_call(gpu):
    from umeregrobust_amd.models import ResUNetSmall2
    m = ResUNetSmall2(in_channels=1, out_channels=32)
    m.load_state_dict(fg.torch_state(fg.seeded(42)))
    m = m.eval().to(gpu)
    coords = kt6000()
    before = fg.run(m, coords, gpu).F.clone()
    assert bits(before).equal(bits(fg.run(fg.model(gpu), coords, gpu).F))
    m.precision = "f16"
    ws = next(iter(m._ws.values()))
    half = fg.run(m, coords, gpu).F.clone()
    assert len(m._ws) == 1 and next(iter(m._ws.values())) is ws, "the f16 call took another workspace"
    assert bits(half).equal(bits(fg.run(model16(gpu), coords, gpu).F)) and not bits(half).equal(bits(before))
    m.precision = "f32"
    assert bits(fg.run(m, coords, gpu).F).equal(bits(before))


# ---- 6: guard bands ---------------------------------------------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


class Guarded:
    """device buffers of exact size between 4 KiB canaries"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def alloc(self, nbytes, fill):
        full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=self.dev)
        full[:PAD] = CANARY
        full[PAD + nbytes:] = CANARY
        full[PAD:PAD + nbytes] = fill
        self.bufs.append((full, nbytes))
        return full

    def inp(self, a):
        a = np.ascontiguousarray(a)
        full = self.alloc(a.nbytes, 0)
        full[PAD:PAD + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.dev))
        return full.data_ptr() + PAD

    def check(self):
        torch.cuda.synchronize()
        for full, nb in self.bufs:
            assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"


def test_guard_bands_and_run_twice(gpu):
    """Both entry points of include/umereg_featnet_f16.h with every device buffer between canaries at exactly the size the header
    / the query states; outputs poisoned, workspace full of garbage; two runs with other poison and garbage agree byte for byte."""
    from umeregrobust_amd import models
    lib = models.load_native()
    coords = batch2()[::5].copy()
    n, batch = len(coords), 2
    params = model16(gpu).packed_parameters()
    assert params.numel() == lib.umereg_featnet_params_count()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    ws_bytes = lib.umereg_featnet_workspace_bytes(n, batch)
    rng = np.random.default_rng(3)
    cases = [(0, 32, 32), (5, 32, 64), (9, 128, 64), (-1, 96, 64)]      # (table, C_in, C_out): both tiles, all three kinds of table, 1x1
    data = {t: (rng.standard_normal((n, ci)).astype(np.float32), rng.standard_normal((27 if t >= 0 else 1, ci, co)).astype(np.float32))
            for t, ci, co in cases}
    results = []
    for poison, garbage in ((0xCD, 0xEE), (0x3C, 0x17)):
        g = Guarded(gpu)
        c_p, f_p, p_p = g.inp(coords.astype(np.int32)), g.inp(np.ones((n, 1), np.float32)), g.inp(params.cpu().numpy())
        out, status, ws = g.alloc(n * 32 * 4, poison), g.alloc(8 * 4, poison), g.alloc(ws_bytes, garbage)
        rc = lib.umereg_featnet_forward_f16(c_p, f_p, n, batch, p_p, out.data_ptr() + PAD, status.data_ptr() + PAD, ws.data_ptr() + PAD,
                                            ws_bytes, stream)
        assert rc == 0, lib.umereg_last_error()
        g.check()
        st = status[PAD:PAD + 32].view(torch.int32).cpu()
        assert int(st[0]) == 0 and int(st[1]) == n
        got = [out[PAD:PAD + n * 32 * 4].clone(), st]
        sizes = st[1:6].tolist()
        # the operator over the maps that forward left in the guarded workspace: inputs of n rows (every level has at most n)
        ones_p, zeros_p = g.inp(np.ones(256, np.float32)), g.inp(np.zeros(256, np.float32))
        for t, ci, co in cases:
            rows_out = sizes[0 if t < 0 else t if t < 5 else t - 4 if t < 9 else t - 9]
            x_p, w_p = g.inp(data[t][0]), g.inp(data[t][1])
            o = g.alloc(rows_out * co * 4, poison)
            rc = lib.umereg_sparse_conv_f16(ws.data_ptr() + PAD, ws_bytes, status.data_ptr() + PAD, n, t, x_p, ci, w_p, ci, co, ones_p,
                                            zeros_p, o.data_ptr() + PAD, co, 0, stream)
            assert rc == 0, lib.umereg_last_error()
            g.check()
            got.append(o[PAD:PAD + rows_out * co * 4].clone())
        results.append(got)
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert torch.isfinite(results[0][0].view(torch.float32)).all()


# ---- 7: the range bit -------------------------------------------------------------------------------------------------------------

def test_activations_beyond_the_f16_range_raise(gpu):
    from umeregrobust_amd import models
    from umeregrobust_amd.sparse import SparseTensor
    coords = fg.edge_cloud("one_cell")
    C = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(gpu)
    big = SparseTensor(torch.full((len(C), 1), 1e6, device=gpu), coordinates=C)
    with torch.no_grad():
        with pytest.raises(ValueError, match="precision='f16'.*f16 range"):
            model16(gpu)(big)
        out = fg.model(gpu)(big).F
    assert torch.isfinite(out).all() and float((out.norm(dim=1) - 1).abs().max()) < 1e-5
    # the bit itself, through the C ABI
    m = model16(gpu)
    ws = torch.empty(models.workspace_bytes(len(C), 1), dtype=torch.uint8, device=gpu)
    o, status = torch.empty(len(C), 32, device=gpu), torch.empty(models.N_STATUS, dtype=torch.int32, device=gpu)
    models.forward_raw(C, torch.full((len(C), 1), 1e6, device=gpu), 1, m.packed_parameters(), ws, o, status, precision="f16")
    assert int(status[0]) == models.ERR_F16_RANGE == 4
    models.forward_raw(C, torch.ones(len(C), 1, device=gpu), 1, m.packed_parameters(), ws, o, status, precision="f16")
    assert int(status[0]) == 0
    # and the model works after the refusal
    assert fg.run(model16(gpu), coords, gpu).F.shape == (len(C), 32)


# ---- 8: plumbing ------------------------------------------------------------------------------------------------------------------

def test_cached_pairs_with_f16_features(gpu, tmp_path):
    """The small synthetic cache of tests/test_featnet_gpu.py's checkpoint test (one pair of it): `feature_precision="f16"`
    features lie within the network gate of the fp64 restatement; the default is the f32 features, bit for bit."""
    import argparse
    from umeregrobust_amd import evaluate
    from umeregrobust_amd.datasets import write_cached_pair
    from umeregrobust_amd.synth import synth_pair_cfg
    from umeregrobust_amd.utils.general_utils import benchmark_config_path, update_namespace_from_yaml
    ck = tmp_path / "w.pth"
    torch.save({"epoch": 1, "model_state_dict": fg.torch_state(fg.seeded(7)), "optimizer_state_dict": {}, "total_loss": 0.0}, ck)
    p = synth_pair_cfg(20, "NS", "test", n_src=6000, n_tgt=5000)
    item = []
    for pts in (p.src_pts, p.tgt_pts):
        c = np.round(pts / 0.3).astype(np.int32)
        keep = np.sort(np.unique(c, axis=0, return_index=True)[1])
        item.append((pts[keep], np.zeros(len(keep), np.int64), c[keep]))
    (sp, ss, sc_), (tp, ts_, tc) = item
    T = p.gt_tform.astype(np.float32)
    moved = (sp @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    matches = np.stack([np.arange(min(len(sp), len(tp)))] * 2, 1).astype(np.int64)
    fields = (torch.from_numpy(sp), torch.from_numpy(ss), torch.from_numpy(sc_), torch.from_numpy(tp), torch.from_numpy(ts_),
              torch.from_numpy(tc), torch.from_numpy(moved), torch.from_numpy(T), matches)
    write_cached_pair(str(tmp_path / "plain" / "test" / "08" / "000000_000001.pickle"), fields)
    args = update_namespace_from_yaml(argparse.Namespace(benchmark="kitti_test"), benchmark_config_path("kitti_test"))
    args.max_pc_size = 100000          # no dilution: the collate only permutes
    args.split = "test"

    def pair(**kw):
        return next(iter(evaluate.cached_pairs(str(tmp_path / "plain"), None, "test", range(1), args, gpu, rng=np.random.RandomState(0),
                                               checkpoint=str(ck), **kw)))

    half, full, default = pair(feature_precision="f16"), pair(feature_precision="f32"), pair()
    sd = fg.f32_state(fg.seeded(7))
    for side, pts, c in (("src", sp, sc_), ("tgt", tp, tc)):
        assert torch.equal(full[f"{side}_feat"], default[f"{side}_feat"])
        coords = np.concatenate([np.zeros((len(c), 1), np.int64), c.astype(np.int64)], axis=1)
        want = ref.network(coords, np.ones((len(c), 1)), sd)[0]
        e16 = f16ref.network(coords, np.ones((len(c), 1)), sd)[0] - want
        got_pts = half[f"{side}_pts"][0].cpu().numpy()
        oa, ob = np.lexsort(np.asarray(pts, np.float32).T), np.lexsort(got_pts.T)
        assert np.array_equal(np.asarray(pts, np.float32)[oa], got_pts[ob])
        for name, feats, f16 in (("f16", half, True), ("f32", full, False)):
            err = feats[f"{side}_feat"][0].cpu().numpy()[ob] - want[oa]
            r_rms, r_max = f16ref.rms(err) / f16ref.rms(e16), np.abs(err).max() / np.abs(e16).max()
            print(f"[cached_pairs {name} {side}] (gpu - fp64) / E16: rms {r_rms:.4f} max {r_max:.4f}")
            if f16:
                assert r_rms <= RMS_GATE and r_max <= MAX_GATE, (side, r_rms, r_max)
                assert r_rms >= 0.5, "these are not f16-operand features"
            else:
                assert np.abs(err).max() <= F32_TOL


def test_f16_module_refuses_train_mode(gpu):
    from umeregrobust_amd.models import ResUNetSmall2
    from umeregrobust_amd.sparse import SparseTensor
    coords = fg.edge_cloud("one_cell")
    C = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(gpu)
    st = SparseTensor(torch.ones(len(C), 1, device=gpu), coordinates=C)
    for trainable in (False, True):
        m = ResUNetSmall2(precision="f16", trainable=trainable).to(gpu)
        with pytest.raises(RuntimeError, match="precision='f16'.*inference only"):
            m.train()(st)
        with pytest.raises(RuntimeError, match="precision='f16'.*inference only"):
            m.eval()(st)                      # parameters require grad and grad is enabled: the layer-wise path
        with torch.no_grad():
            assert m.eval()(st).F.shape == (len(C), 32)
