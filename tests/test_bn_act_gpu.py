"""GPU: the kernels of include/umereg_bn_act.h against the fp64 restatement tests/bn_act_ref.py -- bit for bit on exact data,
within a counted rounding bound on N(0, 1) data, the statistics under cancellation, the running statistics, the ReLU edge,
determinism between guard bands, and `grad_scale_device` against `sparse_conv.grad_scale` bit for bit.

Shapes: C in {32, 64, 128, 256}; with S the plan's slab length and W the finishing step's width in slabs (csrc/bn_act_plan.h,
mirrored and checked in tests/test_bn_act_cpu.py), n in {2, 3, S - 1, S, S + 1, 2 S + 1, W S + 1}."""
import numpy as np
import pytest
import torch

import bn_act_ref as bref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def dev_t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got, want64, what):
    """the f32 result holds exactly the fp64 restatement's value"""
    got = got.detach().cpu().double().numpy()
    bad = got != want64
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} differ, max {float(np.abs(got - want64).max())}"


def run_forward(dev, x, gamma, beta, res, relu, train, eps, rm=None, rv=None, nbt=None, momentum=0.1):
    from umeregrobust_amd import bn_act
    C = x.shape[1]
    rm = dev_t(np.zeros(C) if rm is None else rm, dev)
    rv = dev_t(np.ones(C) if rv is None else rv, dev)
    nbt = torch.tensor(0 if nbt is None else nbt, dtype=torch.int64, device=dev)
    y, stats = bn_act.forward_raw(dev_t(x, dev), None if res is None else dev_t(res, dev), dev_t(gamma, dev), dev_t(beta, dev), rm, rv, nbt,
                                  train, relu, eps, momentum)
    return y, stats, (rm, rv, nbt)


# ---- 1. exact -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", bref.CHANNELS)
def test_exact_data_comes_out_bit_for_bit(gpu, C):
    """eps = 0; rows m +- 2^k, small-integer residual, gamma, beta and dy: every quantity of the forward and both parameter
    gradients are small dyadic numbers, exact in f32 and in every order of summation, so the kernels must EQUAL the restatement at
    every even n.  dx divides by n: it is compared where n is a power of two, and at every even n with a dy built so that
    dbeta = dgamma = 0 (identity activation)."""
    from umeregrobust_amd import bn_act
    checked_dx = 0
    for n in (r for r in bref.edge_rows(C) if r % 2 == 0):
        x, m, k, sign = bref.exact_cloud(n, C, 100 + n)
        gamma, beta = bref.small_ints(C, -3, 3, n + 1), bref.small_ints(C, -2, 2, n + 2)
        res, dy = bref.small_ints((n, C), -3, 3, n + 3), bref.small_ints((n, C), -3, 3, n + 4)
        for relu, use_res, grad in ((True, True, dy), (False, False, dy), (False, True, bref.balanced_dy(sign, n))):
            r = res if use_res else None
            f = bref.forward(x, gamma, beta, r, relu, True, 0.0)
            y, stats, _ = run_forward(gpu, x, gamma, beta, r, relu, True, 0.0)
            tag = f"C={C} n={n} relu={relu} res={use_res}"
            same_bits(y, f["y"], tag + " y")
            same_bits(stats[0], f["mean"], tag + " save_mean")
            same_bits(stats[1], f["invstd"], tag + " save_invstd")
            b = bref.backward(grad, x, f["y"], gamma, f["mean"], f["invstd"], True, relu)
            dx, dres, dgamma, dbeta = bn_act.backward_raw(dev_t(grad, gpu), dev_t(x, gpu), y, dev_t(gamma, gpu), stats, True, relu,
                                                          need_dres=use_res)
            same_bits(dbeta, b["dbeta"], tag + " dbeta")
            same_bits(dgamma, b["dgamma"], tag + " dgamma")
            balanced = grad is not dy
            if balanced:
                assert not b["dbeta"].any() and not b["dgamma"].any()
            if balanced or n & (n - 1) == 0:
                same_bits(dx, b["dx"], tag + " dx")
                checked_dx += 1
            if use_res:
                same_bits(dres, b["dres"], tag + " dres")
    assert checked_dx >= 4


# ---- 2. bounded ---------------------------------------------------------------------------------------------------------------------

K_FWD = 7       # roundings on the forward's path, counted below
K_BWD = 7


def bounded_shapes():
    out = [(n, C) for C in bref.CHANNELS for n in bref.edge_rows(C)]
    return out + [(256 * bref.plan(2, 256)[1] + 1, 256)]          # 4097 x 256: the slab grows to five passes (bref.plan)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_random_data_stays_within_the_counted_rounding_bound(gpu, train):
    """N(0, 1) data, eps = 1e-5.  Per element, against the fp64 restatement of the same f32 inputs:

        |y - y64|   <= K_FWD u (|x scale| + |mean scale| + |beta| + |residual|),
        |dx - dx64| <= K_BWD u (|a g| + |a dbeta / n| + |a xhat' dgamma / n| + |a mean invstd dgamma / n|),   xhat' = x invstd, a = gamma invstd,

    u = 2^-24.  The roundings of the kernel's own path (csrc/bn_act.hip; the fp64 sums contribute some 1e-16 n and are not counted):
      forward, the term through the mean: mean -> f32 (1), invstd -> f32 (1), scale = gamma invstd (1), shift = fma(-mean, scale, beta)
        (1), y = fma(x, scale, shift) (1), + residual (1): 6; the term through x alone has 4 of them.  K_FWD = 6 + 1 for the second
        order of (1 + u)^6 and for |shift| <= |beta| + |mean scale| being used in place of shift.
      backward, dx = fma(x, c2, fma(g, a, c3)) with a, c2 = -a invstd dgamma / n, c3 = -a dbeta / n - c2 mean formed in fp64 from the SAVED
        f32 mean and invstd and rounded once each: the term through the mean carries mean -> f32 (1), invstd -> f32 twice (2), c3 (1) and
        the two fma (2): 6, every other term fewer.  K_BWD = 6 + 1 as above.  (eval: dx = a g, 3 roundings.)
    The ReLU mask of the restatement's backward is the kernel's own y > 0, as in the operator's contract (it saves y)."""
    from umeregrobust_amd import bn_act
    worst = {"y": 0.0, "dx": 0.0, "dgamma": 0.0, "dbeta": 0.0}
    for n, C in bounded_shapes():
        rng = np.random.default_rng(1000 * C + n)
        x, res, dy = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(3))
        gamma, beta = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
        rm, rv = rng.standard_normal(C).astype(np.float32) * 0.3, (rng.random(C) + 0.5).astype(np.float32)
        for relu, use_res in ((True, True), (False, False)):
            r = res if use_res else None
            f = bref.forward(x, gamma, beta, r, relu, train, 1e-5, rm, rv)
            y, stats, _ = run_forward(gpu, x, gamma, beta, r, relu, train, 1e-5, rm, rv)
            bound = K_FWD * U * (np.abs(x * f["scale"]) + np.abs(f["mean"] * f["scale"]) + np.abs(beta.astype(np.float64))
                                 + (np.abs(res.astype(np.float64)) if use_res else 0.0))
            err = np.abs(y.cpu().double().numpy() - f["y"])
            ratio = float((err / bound).max())
            worst["y"] = max(worst["y"], ratio)
            assert ratio <= 1.0, f"y n={n} C={C} relu={relu}: worst |err| / bound {ratio:.3f}"
            yk = y.cpu().numpy()
            b = bref.backward(dy, x, yk, gamma, f["mean"], f["invstd"], train, relu)
            dx, dres, dgamma, dbeta = bn_act.backward_raw(dev_t(dy, gpu), dev_t(x, gpu), y, dev_t(gamma, gpu), stats, train, relu,
                                                          need_dres=use_res)
            g = b["dres"]
            a = np.abs(gamma * f["invstd"])
            terms = a * np.abs(g)
            if train:
                terms = terms + a * np.abs(b["dbeta"]) / n + a * (np.abs(x * f["invstd"]) + np.abs(f["mean"] * f["invstd"])) * np.abs(b["dgamma"]) / n
            err = np.abs(dx.cpu().double().numpy() - b["dx"])
            ratio = float((err / np.maximum(K_BWD * U * terms, 1e-300))[terms > 0].max())
            worst["dx"] = max(worst["dx"], ratio)
            assert ratio <= 1.0 and not err[terms == 0].any(), f"dx n={n} C={C} relu={relu}: worst |err| / bound {ratio:.3f}"
            if use_res:
                assert np.array_equal(dres.cpu().numpy(), g.astype(np.float32))
            # the sums: fp64 accumulation, one rounding of the result, and the saved statistics' own rounding inside xhat
            xh = np.abs(g) * (np.abs(x * f["invstd"]) + np.abs(f["mean"] * f["invstd"]))
            for key, got, absum in (("dbeta", dbeta, np.abs(g).sum(axis=0)), ("dgamma", dgamma, xh.sum(axis=0))):
                e = np.abs(got.cpu().double().numpy() - b[key])
                ratio = float((e / np.maximum(4 * U * absum, 1e-300)).max())
                worst[key] = max(worst[key], ratio)
                assert ratio <= 1.0, f"{key} n={n} C={C}: worst |err| / (4 u sum |terms|) {ratio:.3f}"
    print(f"[bn_act rounding {'train' if train else 'eval'}] worst |err| / bound: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ---- 3. cancellation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,n", [(32, 8 * 128 + 1), (256, 4097)])
def test_statistics_survive_a_mean_1e5_standard_deviations_away(gpu, C, n):
    """x = 1000 + 0.01 N(0, 1): save_mean within 2 u relative of the fp64 truth, and the variance recovered from save_invstd
    (eps = 0) within 8 u relative: one rounding of invstd (u, twice in the square: 2 u) -- the fp64 sums about the pivot contribute
    nothing at this size.  A plain f32 sum(x^2) / n - mean^2 on the same data (numpy, f32 accumulators, on the CPU; the true
    variance 1e-4 lies below the rounding step 0.06 of the 1e6-sized mean square) is off by a relative 9.6e3 = 1.6e11 u at
    1025 x 32 (47 % of the channels negative) and by 3.2e5 = 5.4e12 u at 4097 x 256 (every channel negative)."""
    rng = np.random.default_rng(C + n)
    x = (1000.0 + 0.01 * rng.standard_normal((n, C))).astype(np.float32)
    f = bref.forward(x, np.ones(C), np.zeros(C), eps=0.0)
    _, stats, _ = run_forward(gpu, x, np.ones(C, np.float32), np.zeros(C, np.float32), None, False, True, 0.0)
    mean, inv = stats[0].cpu().double().numpy(), stats[1].cpu().double().numpy()
    e_mean = float((np.abs(mean - f["mean"]) / np.abs(f["mean"])).max())
    e_var = float((np.abs(inv ** -2.0 - f["var"]) / f["var"]).max())
    naive = (x * x).sum(axis=0, dtype=np.float32) / np.float32(n) - (x.sum(axis=0, dtype=np.float32) / np.float32(n)) ** 2
    print(f"[bn_act cancellation C={C} n={n}] mean / std {float((f['mean'] / np.sqrt(f['var'])).min()):.3g}; relative error of the mean "
          f"{e_mean / U:.3f} u, of the variance {e_var / U:.3f} u; a plain f32 sum of squares: {float((np.abs(naive - f['var']) / f['var']).max()) / U:.3g} u")
    assert float((f["mean"] / np.sqrt(f["var"])).min()) > 5e4
    assert e_mean <= 2 * U and e_var <= 8 * U


# ---- 4. running statistics --------------------------------------------------------------------------------------------------------------

def test_running_statistics_follow_the_restatement(gpu):
    """three train-mode calls with other data through the autograd op: running_mean and running_var within 4 u relative of the fp64
    restatement fed the same f32 inputs (each call rounds the two buffers once: 3 u, plus the restatement's own start from f32),
    num_batches_tracked == 3; an eval-mode call moves nothing and returns the running statistics' output."""
    from umeregrobust_amd import bn_act
    C, mom = 64, 0.1
    rng = np.random.default_rng(4)
    bn = torch.nn.BatchNorm1d(C, momentum=mom).to(gpu)
    rm, rv, t = np.zeros(C), np.ones(C), 0
    for i, n in enumerate((65, 130, 257)):
        x = (rng.standard_normal((n, C)) * (1 + i) + i).astype(np.float32)
        v0 = bn.running_mean._version
        y = bn_act.batch_norm_act(dev_t(x, gpu), bn.train())
        assert bn.running_mean._version > v0                       # (keys the model's packed-parameter cache)
        f = bref.forward(x, np.ones(C), np.zeros(C))
        rm, rv, t = bref.running_update(rm, rv, t, f["mean"], f["var"], n, mom)
        assert float(np.abs(y.detach().cpu().double().numpy() - f["y"]).max()) <= 1e-5
    e_m = float((np.abs(bn.running_mean.cpu().double().numpy() - rm) / np.abs(rm)).max())
    e_v = float((np.abs(bn.running_var.cpu().double().numpy() - rv) / rv).max())
    print(f"[bn_act running statistics] relative error: mean {e_m / U:.3f} u, var {e_v / U:.3f} u")
    assert e_m <= 4 * U and e_v <= 4 * U and int(bn.num_batches_tracked) == 3 == t
    before = [b.clone() for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    x = rng.standard_normal((33, C)).astype(np.float32)
    y = bn_act.batch_norm_act(dev_t(x, gpu), bn.eval())
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)
    f = bref.forward(x, np.ones(C), np.zeros(C), train=False, running_mean=before[0].cpu().numpy(), running_var=before[1].cpu().numpy())
    assert float(np.abs(y.detach().cpu().double().numpy() - f["y"]).max()) <= 1e-5


# ---- 5. the ReLU edge -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_relu_edge_decides_on_y_greater_than_zero(gpu, train):
    """rows whose y is exactly 0 (0 + 0, v + (-v), a negative pre-activation) give dres = 0; rows whose y is the smallest positive
    f32 (2^-149), the smallest normal one (2^-126) or 1 give dres = dy.  Eval: the identity map (gamma 1, beta 0, mean 0, var 1,
    eps 0), so y = relu(x + residual) exactly, the edge value in x on odd rows and in the residual on even ones.  Train: gamma = 0
    and beta = 0 over N(0, 1) rows, so y = relu(residual) exactly."""
    from umeregrobust_amd import bn_act
    C, n = 32, 130
    tiny, fmin = np.float32(2.0 ** -149), np.float32(2.0 ** -126)
    rng = np.random.default_rng(5)
    x, res = np.zeros((n, C), np.float32), np.zeros((n, C), np.float32)
    if train:
        x, gamma = rng.standard_normal((n, C)).astype(np.float32), np.zeros(C, np.float32)
    else:
        gamma = np.ones(C, np.float32)
        x[1], res[1] = 3.0, -3.0
    want_pos = np.zeros((n, C), bool)
    for row, bump in ((10, tiny), (11, fmin), (12, np.float32(1.0)), (13, -tiny), (14, np.float32(-1.0)), (129, tiny)):
        if train or row % 2 == 0:
            res[row] = bump
        else:
            x[row] = bump
        want_pos[row] = bump > 0
    dy = rng.standard_normal((n, C)).astype(np.float32)
    dy[dy == 0] = 1.0
    y, stats, _ = run_forward(gpu, x, gamma, np.zeros(C, np.float32), res, True, train, 0.0)
    yk = y.cpu().numpy()
    assert np.array_equal(yk > 0, want_pos) and np.array_equal(yk[10], np.full(C, tiny)) and not yk[~want_pos].any()
    _, dres, _, _ = bn_act.backward_raw(dev_t(dy, gpu), dev_t(x, gpu), y, dev_t(gamma, gpu), stats, train, True, need_dres=True)
    assert np.array_equal(dres.cpu().numpy(), np.where(want_pos, dy, np.float32(0.0)))


# ---- 6. determinism and scratch hygiene -------------------------------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


def test_raw_entries_between_guard_bands_run_twice(gpu):
    """every device buffer of the three compute entries between 4 KiB canaries at exactly the size the header states; the scratch
    pre-filled with garbage and the outputs with poison; two runs with other garbage give equal bits and leave the bands intact.
    Rows with a stride (ld = C + 4) included."""
    from umeregrobust_amd import bn_act
    lib = bn_act.load_native()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    rng = np.random.default_rng(6)
    cases = [(2 * 128 + 1, 32, 36), (17, 256, 256), (8 * 128 + 1, 32, 32), (33, 96, 100)]
    results = []
    for poison, garbage in ((0xCD, 0xEE), (0x3C, 0x17)):
        bufs, outs = [], []

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

        def rows(n, C, ld):
            """a strided [n, C] matrix occupies (n - 1) ld + C elements"""
            return ((n - 1) * ld + C) * 4

        def padded(a, ld):
            out = np.zeros((a.shape[0], ld), np.float32)
            out[:, :a.shape[1]] = a
            return out.reshape(-1)[:(a.shape[0] - 1) * ld + a.shape[1]]

        rng = np.random.default_rng(6)
        for n, C, ld in cases:
            x, res, dy = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(3))
            gamma, beta = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
            need = lib.umereg_bn_act_scratch_bytes(n, C)
            assert need == bref.scratch_bytes(n, C)
            x_p, res_p, dy_p, g_p, b_p = inp(padded(x, ld)), inp(padded(res, ld)), inp(padded(dy, ld)), inp(gamma), inp(beta)
            rm, rv, nbt = alloc(C * 4, 0), inp(np.ones(C, np.float32)), alloc(8, 0)
            y, sm, si = alloc(rows(n, C, ld), poison), alloc(C * 4, poison), alloc(C * 4, poison)
            scratch = alloc(need, garbage)
            rc = lib.umereg_bn_act_forward_f32(x_p, ld, res_p, ld, n, C, g_p, b_p, rm.data_ptr() + PAD, rv, nbt.data_ptr() + PAD, 1, 1, 1e-5, 0.1,
                                               y.data_ptr() + PAD, ld, sm.data_ptr() + PAD, si.data_ptr() + PAD, scratch.data_ptr() + PAD, need,
                                               stream)
            assert rc == 0, lib.umereg_last_error()
            dx, dres, dg, db = alloc(rows(n, C, ld), poison), alloc(rows(n, C, ld), poison), alloc(C * 4, poison), alloc(C * 4, poison)
            scratch2 = alloc(need, garbage)
            rc = lib.umereg_bn_act_backward_f32(dy_p, ld, x_p, ld, y.data_ptr() + PAD, ld, n, C, g_p, sm.data_ptr() + PAD, si.data_ptr() + PAD, 1,
                                                1, dx.data_ptr() + PAD, ld, dres.data_ptr() + PAD, ld, dg.data_ptr() + PAD, db.data_ptr() + PAD,
                                                scratch2.data_ptr() + PAD, need, stream)
            assert rc == 0, lib.umereg_last_error()
            # a scratch one byte short is refused, not overrun
            assert lib.umereg_bn_act_backward_f32(dy_p, ld, x_p, ld, y.data_ptr() + PAD, ld, n, C, g_p, sm.data_ptr() + PAD, si.data_ptr() + PAD,
                                                  1, 1, dx.data_ptr() + PAD, ld, dres.data_ptr() + PAD, ld, dg.data_ptr() + PAD,
                                                  db.data_ptr() + PAD, scratch2.data_ptr() + PAD, need - 1, stream) == -3
            count = n * C if ld == C else 63
            gneed = lib.umereg_grad_scale_scratch_bytes(count)
            gout, gscr = alloc(12, poison), alloc(gneed, garbage)
            rc = lib.umereg_grad_scale_f32(dy_p, count, gout.data_ptr() + PAD, gout.data_ptr() + PAD + 4, gout.data_ptr() + PAD + 8,
                                           gscr.data_ptr() + PAD, gneed, stream)
            assert rc == 0, lib.umereg_last_error()
            torch.cuda.synchronize()
            for full, nb in bufs:
                assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"
            strided = lambda full: full[PAD:PAD + rows(n, C, ld)].view(torch.float32).cpu().numpy()         # noqa: E731
            for full in (y, dx, dres):
                flat = np.full(n * ld, np.nan, np.float32)
                flat[:(n - 1) * ld + C] = strided(full)
                outs.append(torch.from_numpy(flat.reshape(n, ld)[:, :C].copy()))
                assert bool(torch.isfinite(outs[-1]).all())
            outs += [t[PAD:PAD + nb].clone().cpu() for t, nb in ((sm, C * 4), (si, C * 4), (dg, C * 4), (db, C * 4), (rm, C * 4), (nbt, 8), (gout, 12))]
            assert int(nbt[PAD:PAD + 8].view(torch.int64)) == 1
            if ld > C:      # the gap between rows keeps its poison
                gap = y[PAD:PAD + rows(n, C, ld)].view(torch.float32).cpu().numpy()[:(n - 1) * ld].reshape(n - 1, ld)[:, C:]
                assert (np.ascontiguousarray(gap).view(np.uint8) == poison).all()
        results.append(outs)
    assert len(results[0]) == len(results[1]) == 10 * len(cases)
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)


# ---- 7. the gradient scale ----------------------------------------------------------------------------------------------------------------

def scale_cases():
    big = bref.GS_WIDTH * bref.GS_CHUNK + 1                 # one element past the finishing workgroup's first pass of partials
    places = {1: [0], 63: [0, 62], 65: [0, 63, 64], 2 * bref.GS_CHUNK + 5: [0, bref.GS_CHUNK - 1, bref.GS_CHUNK, 2 * bref.GS_CHUNK + 4],
              big: [0, bref.GS_CHUNK - 1, bref.GS_CHUNK, big - 2, big - 1]}
    return [(n, at) for n, ats in places.items() for at in ats]


@pytest.mark.parametrize("v", bref.SCALE_VALUES, ids=lambda v: f"{v:.6g}")
def test_grad_scale_device_is_grad_scale_bit_for_bit(gpu, v):
    """`v` as the only extreme value of the tensor (first and last element, both sides of a partial's edge; 1, 63, 65 and
    W x 8192 + 1 elements; positive and negative), and the empty tensor: (e, 2^e, 2^-e) equal `sparse_conv.grad_scale`'s on the GPU
    and the restatement's, bit for bit."""
    from umeregrobust_amd import bn_act
    from umeregrobust_amd import sparse_conv as sc
    fills = {}
    for n, at in scale_cases():
        if n not in fills:
            fills[n] = torch.full((n,), bref.scale_background(v), dtype=torch.float32, device=gpu)
        for sign in ((1.0, -1.0) if at == 0 or n > 65 else (1.0,)):
            dy = fills[n]
            keep = dy[at].clone()
            dy[at] = sign * v
            got = [t.cpu() for t in bn_act.grad_scale_device(dy)]
            want = [t.cpu() for t in sc.grad_scale(dy)]
            mine = bref.grad_scale(np.array([sign * v], np.float32))
            dy[at] = keep
            assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.float32] and all(t.dim() == 0 for t in got)
            for a, b, c in zip(got, want, mine):
                assert bits(a.reshape(1)).equal(bits(b.reshape(1))), (v, n, at, sign, got, want)
                assert int(bits(a.reshape(1))) == int(np.asarray(c).reshape(1).view(np.int32)[0]), (v, n, at, sign, got, mine)
    # a 2-D gradient, as the convolution's backward passes it, and the empty tensor
    dy = torch.full((70, 32), bref.scale_background(v), dtype=torch.float32, device=gpu)
    dy[69, 31] = -v
    for t in (dy, torch.zeros(0, 32, device=gpu)):
        for a, b in zip(bn_act.grad_scale_device(t), sc.grad_scale(t)):
            assert bits(a.reshape(1)).equal(bits(b.reshape(1))), (v, tuple(t.shape))
