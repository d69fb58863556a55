"""GPU: the weight gradient of csrc/sparse_wgrad.hip at its group, ballot-chunk, queue and segment edges -- the f32 body (groups
of 8), the f16 body (groups of 16) and the C_in = 1 body (8 row lanes) -- on the clouds of tests/wgrad_cases.py, whose edges
tests/test_wgrad_edges_cpu.py pins without a GPU; rows with leading dimensions beyond their channel count; the kernel repack.

The truth is always x[i]^T dy[o] in fp64 per offset over the pair lists of featnet_grad_ref.Tables (wgrad_cases.truth), with
the GPU's rows mapped to the helper's by coordinate; never another GPU result, except where two runs must agree bit for bit.
Operands are integers in [-3, 3] (f16: dY times 2^12, as the entry expects), every sum an integer below 2^24: EQUALITY is
required, and an offset without pairs must come out as the bit pattern 0."""
import numpy as np
import pytest
import torch

import featnet_f16_grad_ref as g16
import featnet_grad_ref as gref
import test_sparse_grad_gpu as sg
import test_train_f16_gpu as ttf
import wgrad_cases as wc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PRECISIONS = ("f32", "f16")
F16_SCALE = 2.0 ** 12
_cache = {}

# the two clouds of the rounding test, under names of their own in the tables of test_sparse_grad_gpu: test_train_f16_gpu.bounds
# and .restated look their pair lists up by name
ROUNDING_CLOUDS = {"wgrad_edges_line129": "line129", "wgrad_edges_rows1025": "rows1025"}
for _name, _case in ROUNDING_CLOUDS.items():
    sg.CLOUDS.setdefault(_name, lambda case=_case: wc.cloud(case))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def maps_of(name, dev):
    """-> (CoordinateMaps, per level the helper row of every GPU row); level 0 is the order wgrad_cases.level0_order predicts"""
    from umeregrobust_amd import sparse_conv as sc
    if name not in _cache:
        c = wc.cloud(name)
        maps = sc.CoordinateMaps(torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev), 1)
        rows = sg.row_maps([maps.level_coords(l) for l in range(5)], wc.tables_of(name))
        perm = maps.perm.cpu().numpy()
        assert np.array_equal(rows[0].numpy(), perm) and np.array_equal(perm, wc.level0_order(c))
        _cache[name] = (maps, rows)
    return _cache[name]


def operands(name, t, cin, cout, draw=wc.integers):
    """x, dy in the helper's row order; C_in = 1: a non-constant column without zeros"""
    sizes = wc.tables_of(name).sizes
    n_in, n_out = sizes[gref.in_level(t)], sizes[gref.out_level(t)]
    seed = 100000 * t + 1000 * cin + cout + n_in
    x = draw((n_in, cin), seed) if cin > 1 or draw is not wc.integers else (1 + torch.arange(n_in) % 3).to(torch.float32)[:, None]
    return x, draw((n_out, cout), seed + 1)


def on_gpu(name, dev, t, x, dy):
    """the operands in the GPU's row orders"""
    _, rows = maps_of(name, dev)
    return x[rows[gref.in_level(t)]].to(dev), dy[rows[gref.out_level(t)]].to(dev)


def assert_exact(dw, want, scale, name, t, prec):
    """dw (CPU f32 [27, C_in, C_out]) EQUALS want (fp64) x scale; offsets without pairs are the bit pattern 0"""
    pairs = wc.pair_counts(name, t)
    label = f"{name} table {t} {dw.shape[1]}->{dw.shape[2]} {prec}"
    assert tuple(dw.shape) == tuple(want.shape), label
    assert bool(torch.isfinite(dw).all()), f"{label}: {int((~torch.isfinite(dw)).sum())} elements are not finite"
    wrong = (dw.double() != want * scale).flatten(1).sum(1)
    assert not bool(wrong.any()), f"{label}: " + ", ".join(
        f"offset {k} ({pairs[k]} pairs): {int(wrong[k])} elements differ, max {float((dw[k].double() / scale - want[k]).abs().max()):g}"
        for k in torch.nonzero(wrong).flatten().tolist())
    empty = [k for k in range(27) if not pairs[k]]
    assert bool(bits(dw[empty]).eq(0).all()), f"{label}: an offset without pairs is not the bit pattern 0"


def check_exact(name, dev, t, cin, cout, precisions=PRECISIONS):
    from umeregrobust_amd import sparse_conv as sc
    maps, _ = maps_of(name, dev)
    x, dy = operands(name, t, cin, cout)
    want = wc.truth(wc.tables_of(name), t, x, dy)
    xg, dyg = on_gpu(name, dev, t, x, dy)
    for prec in precisions:
        scale = F16_SCALE if prec == "f16" else 1.0
        dw = sc.wgrad_raw(xg, dyg * scale, maps, t, precision=prec).cpu()
        assert_exact(dw, want, scale, name, t, prec)


# ---- 1: groups, ballot chunks, carries and the ring -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.GROUP_CLOUDS)
def test_group_chunk_carry_and_ring_edges(gpu, name):
    """Every line and every cloud of pairs of two over tables 0, 5 and 9, the four <BI, BO> instantiations, both precisions; and
    C_in = 1 -> 32 over table 0 in f32 (x in level-0 order).  The lines' pair counts lie on both sides of one and two groups of
    8 and of 16, of the 64-row ballot chunk and, from 129 rows on, past position 128 of the queue ring."""
    for t in (0, 5, 9):
        for cin, cout in wc.GROUP_CHANNELS:
            check_exact(name, gpu, t, cin, cout)
    check_exact(name, gpu, 0, 1, 32, ("f32",))


@pytest.mark.parametrize("name,cin,cout", [("line17", 96, 32), ("line65", 192, 64)])
def test_more_than_one_input_tile(gpu, name, cin, cout):
    """96 -> 32: three input tiles with BI = 1; 192 -> 64: three with BI = 2"""
    for t in (0, 5, 9):
        check_exact(name, gpu, t, cin, cout)


# ---- 2: segments ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.SEGMENT_CLOUDS)
def test_one_and_two_segments(gpu, name):
    """1 024 rows are one segment, 1 025 and 1 064 two.  isolated_then_line: rows 0..1023 are the isolated points, so segment 0
    holds no pair of 26 offsets and its all-zero blocks are summed; line_then_isolated: segment 1 does."""
    from umeregrobust_amd import sparse_conv as sc
    lib = sc.load_native()
    maps, _ = maps_of(name, gpu)
    c, perm = wc.cloud(name), maps.perm.cpu().numpy()
    n = len(c)
    if name == "isolated_then_line":
        assert np.array_equal(perm, np.arange(n)) and (c[perm[:1024], 1] >= 1000).all() and (c[perm[1024:], 1] < 1000).all()
    elif name == "line_then_isolated":
        assert np.array_equal(perm, np.arange(n)) and (c[perm[:40], 1] < 1000).all() and (c[perm[40:], 1] >= 1000).all()
    else:
        assert (c[perm[:1024], 1] < 16).all() and (n == 1024 or c[perm[1024], 1] == 1000)
    for cin, cout in wc.SEGMENT_CHANNELS + [(1, 32)]:
        assert lib.umereg_sparse_conv_wgrad_segments(n, cin, cout) == (1 if name == "rows1024" else 2) == wc.plan(n, cin, cout)[1]
        check_exact(name, gpu, 0, cin, cout, PRECISIONS if cin > 1 else ("f32",))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_segments_longer_than_the_floor(gpu, prec):
    """9 217 rows, 256 -> 256: nine segments of 1 088 rows, the first plan whose segment edges are no multiples of 1 024"""
    from umeregrobust_amd import sparse_conv as sc
    assert sc.load_native().umereg_sparse_conv_wgrad_segments(9217, 256, 256) == 9 and wc.plan(9217, 256, 256)[0] == 1088
    check_exact("long_segments", gpu, 0, 256, 256, (prec,))


# ---- 3: plan segments without rows ------------------------------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


def guarded(nbytes, fill, dev):
    full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=dev)
    full[:PAD] = CANARY
    full[PAD + nbytes:] = CANARY
    full[PAD:PAD + nbytes] = fill
    return full


@pytest.mark.parametrize("t", [5, 9])
def test_segments_without_rows_are_not_read(gpu, t):
    """`deep`: 2 049 level-0 rows plan three segments; table 5 writes level 1 (257 rows: two plan segments hold no row), table 9
    writes level 0 (three real segments).  The raw entries with a scratch of exactly the queried size full of 0xFF bytes (NaN)
    between canaries: a block that is read without having been written by this call shows as NaN in dW."""
    from umeregrobust_amd import sparse_conv as sc
    lib = sc.load_native()
    maps, _ = maps_of("deep", gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    assert maps.sizes[:2] == [2049, 257]
    for cin, cout in wc.DEEP_CHANNELS:
        x, dy = operands("deep", t, cin, cout)
        want = wc.truth(wc.tables_of("deep"), t, x, dy)
        xg, dyg = on_gpu("deep", gpu, t, x, dy)
        sc_bytes, dw_bytes = lib.umereg_sparse_conv_wgrad_scratch_bytes(maps.n, cin, cout), 27 * cin * cout * 4
        assert lib.umereg_sparse_conv_wgrad_segments(maps.n, cin, cout) == 3 and sc_bytes == 3 * dw_bytes
        for prec in PRECISIONS:
            scale = F16_SCALE if prec == "f16" else 1.0
            d = (dyg * scale).contiguous()
            dW, scratch = guarded(dw_bytes, 0xFF, gpu), guarded(sc_bytes, 0xFF, gpu)
            fn = lib.umereg_sparse_conv_wgrad_f16 if prec == "f16" else lib.umereg_sparse_conv_wgrad_f32
            with torch.cuda.device(gpu):
                rc = fn(maps.ws.data_ptr(), maps.ws.numel(), maps.status.data_ptr(), maps.n, t, xg.data_ptr(), cin, cin, d.data_ptr(), cout,
                        cout, dW.data_ptr() + PAD, scratch.data_ptr() + PAD, sc_bytes, stream)
            assert rc == 0, lib.umereg_last_error()
            torch.cuda.synchronize()
            for full, nbytes in ((dW, dw_bytes), (scratch, sc_bytes)):
                assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nbytes:] == CANARY).all()), "a guard band was written"
            dw = dW[PAD:PAD + dw_bytes].view(torch.float32).reshape(27, cin, cout).cpu()
            assert_exact(dw, want, scale, "deep", t, prec)


# ---- 4: leading dimensions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["line73", "rows1025"])
def test_rows_with_leading_dimensions(gpu, name):
    """x = columns [8, 8 + C_in) of [rows, C_in + 12], dY = columns [4, 4 + C_out) of [rows, C_out + 8], every other column NaN
    (leading dimensions and column offsets multiples of 4 floats): the views reach the kernel as they are, and dW equals the
    contiguous call bit for bit and the truth exactly."""
    from umeregrobust_amd import _lib
    from umeregrobust_amd import sparse_conv as sc
    maps, _ = maps_of(name, gpu)
    for cin, cout in wc.SEGMENT_CHANNELS:
        x, dy = operands(name, 0, cin, cout)
        want = wc.truth(wc.tables_of(name), 0, x, dy)
        xg, dyg = on_gpu(name, gpu, 0, x, dy)
        for prec in PRECISIONS:
            scale = F16_SCALE if prec == "f16" else 1.0
            wide_x = torch.full((len(xg), cin + 12), float("nan"), device=gpu)
            wide_dy = torch.full((len(dyg), cout + 8), float("nan"), device=gpu)
            xv, dv = wide_x[:, 8:8 + cin], wide_dy[:, 4:4 + cout]
            xv.copy_(xg)
            dv.copy_(dyg * scale)
            assert _lib.rows(xv, "test", "input") is xv and _lib.rows(dv, "test", "output gradient") is dv
            assert xv.stride(0) == cin + 12 and dv.stride(0) == cout + 8 and not xv.is_contiguous() and not dv.is_contiguous()
            assert int(torch.isnan(wide_x).sum()) == 12 * len(xg) and int(torch.isnan(wide_dy).sum()) == 8 * len(dyg)
            dw = sc.wgrad_raw(xv, dv, maps, 0, precision=prec)
            plain = sc.wgrad_raw(xg, dyg * scale, maps, 0, precision=prec)
            assert bits(dw).equal(bits(plain)), (name, cin, cout, prec)
            assert_exact(dw.cpu(), want, scale, name, 0, prec)


# ---- 5: the kernel repack -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 192), (192, 64), (256, 128)])
def test_repack_is_the_header_formula(gpu, cin, cout):
    """umereg_sparse_conv_repack_f32 for transpose x mirror x slice in {32, 64, R}: W = 0, 1, 2, ... (all distinct, below 2^24),
    bit for bit the numpy statement of the header (wgrad_cases.repacked)"""
    from umeregrobust_amd import sparse_conv as sc
    assert 27 * cin * cout < 2 ** 24
    W = np.arange(27 * cin * cout, dtype=np.float32).reshape(27, cin, cout)
    Wg = torch.from_numpy(W).to(gpu)
    done = 0
    slices = lambda R: sorted({s for s in (32, 64, R) if R % s == 0})        # noqa: E731
    for transpose in (False, True):
        R = cout if transpose else cin
        for mirror in (False, True):
            for slice in slices(R):
                got = sc.repack_raw(Wg, transpose, mirror, slice).cpu().numpy()
                want = wc.repacked(W, transpose, mirror, slice)
                assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), (transpose, mirror, slice)
                done += 1
    assert done == 2 * (len(slices(cin)) + len(slices(cout))) >= 6


# ---- 6: rounding on N(0, 1) operands at an edge -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ROUNDING_CLOUDS))
def test_rounding_at_an_edge(gpu, name):
    """N(0, 1) operands over table 0 of line(129) and of the 1 025-row cloud.  f32: |gpu - fp64| <= gamma(2 L + 2) sum |a_i| |b_i|
    per element, L the offset's pairs (the bound of test_sparse_grad_gpu.test_operators_stay_within_the_rounding_bound); f16:
    test_train_f16_gpu.bounds against the fp64 restatement on rounded operands.  Two runs, with other garbage in the scratch,
    agree bit for bit."""
    from umeregrobust_amd import sparse_conv as sc
    case = ROUNDING_CLOUDS[name]
    maps, _ = maps_of(case, gpu)
    tables = wc.tables_of(case)
    L = torch.tensor(wc.pair_counts(case, 0))[:, None, None]
    worst = {}
    for cin, cout in wc.SEGMENT_CHANNELS + [(1, 32)]:
        x, dy = operands(case, 0, cin, cout, wc.normals)
        xg, dyg = on_gpu(case, gpu, 0, x, dy)
        runs = {}
        for prec in PRECISIONS if cin > 1 else ("f32",):
            e = g16.scale_exponent(dy) if prec == "f16" else 0
            d = dyg * 2.0 ** e
            got = sc.wgrad_raw(xg, d, maps, 0, precision=prec)
            maps.scratch(1).fill_(0x17)
            again = sc.wgrad_raw(xg, d, maps, 0, precision=prec)
            assert bits(got).equal(bits(again)), (name, cin, cout, prec)
            runs[prec] = got.cpu().double() * 2.0 ** -e
        m = (2 * L + 2).double() * U
        bound = {"f32": m / (1 - m) * wc.truth(tables, 0, x.abs(), dy.abs())}
        want = {"f32": wc.truth(tables, 0, x, dy)}
        if "f16" in runs:
            W = torch.zeros(27, cin, cout)
            want["f16"] = ttf.restated(name, 0, x, W, dy)[2]
            bound["f16"], L16 = ttf.bounds(name, 0, x, W, dy, ttf.R16)["dw"]
            assert torch.equal(L16, L.expand(-1, cin, cout))
        for prec, got in runs.items():
            err = (got - want[prec]).abs()
            ratio = float((err / bound[prec].clamp_min(1e-300)).max())
            worst[prec] = max(worst.get(prec, 0.0), ratio)
            bad = err > bound[prec]
            assert not bool(bad.any()), f"{name} {cin}->{cout} {prec}: {int(bad.sum())} elements over the bound, worst ratio {ratio:.3g}"
            assert bool(((L == 0) <= (got == 0)).all()), "an element without a chain is not zero"
    print(f"[sparse_conv wgrad rounding {case}] worst |err| / bound: " + " ".join(f"dw_{k}={v:.3f}" for k, v in worst.items()))
