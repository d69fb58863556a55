"""GPU: the one-launch kernels between the stages at their edges -- match_prob_kernel, hypothesis_gates_kernel, rre_kernel,
corr_select_best_kernel, colsum_partial_kernel + feature_weight_kernel.  Most are single-workgroup reductions over 1024 lanes in 16
wavefronts; each had one golden at one size.  Here: n = 1, either side of a wavefront, of 256 and of 1024 lanes, a second and a fifth
trip of the strided loop; ties, a gate met with equality, non-finite input.  Inputs and fp64 truths: tests/glue_cases.py.

Gates are never the kernel's own output: a multiple (4) of the error the reference's own fp32 statement makes on the CPU against the
fp64 truth, floored at 2^-22; exact equality where the arithmetic is exact (counts, selected index, copied rows); a derived bound of
three fp32 roundings for the weighted features."""
import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- match_prob --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", gc.MATCH_PATTERNS)
@pytest.mark.parametrize("tau", gc.MATCH_TAUS)
def test_match_prob_against_fp64_at_every_size(gpu, tau, pattern):
    from umeregrobust_amd import ops
    for n in gc.SIZES:
        d = gc.match_d(n, pattern)
        truth = gc.match_prob_truth(d, tau)
        yard = gc.match_prob_statement(d, tau).astype(np.float64)
        got = ops.match_prob(dev(d, gpu), tau).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (n,)
        got = got.astype(np.float64)
        rel = lambda p: (np.abs(p - truth) / truth).max()
        e_yard, e_got, s_yard, s_got = rel(yard), rel(got), abs(yard.sum() - 1.0), abs(got.sum() - 1.0)
        print(f"tau {tau} {pattern} n {n}: rel. error {e_got:.3g} (fp32 statement {e_yard:.3g}), |sum - 1| {s_got:.3g} ({s_yard:.3g})")
        assert np.isfinite(got).all() and (truth > 0).all()
        assert e_got <= 4 * max(e_yard, gc.EPS_FLOOR), (n, e_got, e_yard)
        assert s_got <= 4 * max(s_yard, gc.EPS_FLOOR), (n, s_got, s_yard)


def test_match_prob_overflows_as_the_reference_does(gpu):
    """tau = 0.01 and d = 0: exp(100) is inf in fp32, the reference divides inf by inf.  The same entries are NaN, the others 0."""
    from umeregrobust_amd import ops
    for n in gc.SIZES:
        d = gc.match_d(n, "uniform")
        d[n // 3] = 0.0
        want = gc.match_prob_statement(d, 0.01)
        got = ops.match_prob(dev(d, gpu), 0.01).cpu().numpy()
        assert np.isnan(want[n // 3]) and not np.isnan(want).all() or n < 3
        assert np.array_equal(np.isnan(got), np.isnan(want)), n
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), n          # a finite a over an infinite sum: 0


# ---- hypothesis_gates ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", gc.SIZES)
def test_hypothesis_gates_counts_equal_numpy(gpu, n):
    from umeregrobust_amd import ops
    counts = torch.zeros(4, dtype=torch.int64, device=gpu)
    want_total = np.zeros(4, np.int64)
    for general_gt in (False, True):
        T, gt, yard, special = gc.gates_case(n, general_gt)
        rre32, rte32, c32, o32 = gc.gates_fp32(T, gt)
        rre64, rte64, c64, o64 = gc.gates_fp64(T, gt)
        # the rows are built so that no gate hangs on a rounding: fp32 and fp64 decide every row alike
        assert np.array_equal(o32, o64) and c32 == c64
        plain = np.isfinite(rre64) & np.isfinite(rte64)
        plain[list(special.values())] = False
        for thr in (1.0, 1.5):
            assert np.abs(rre64[plain] - thr).min() >= 0.005
        if not general_gt:
            x = np.abs(T[:, :3, 3]).max(axis=1)
            assert np.array_equal(rte32[plain], x[plain]) and np.array_equal(rte64[plain], x[plain].astype(np.float64))
            if n >= 64:
                for g in (0.1, 0.3, 0.6):                                             # met with equality, and missed by one ulp
                    assert (x[plain] == np.float32(g)).any() and (x[plain] == gc._succ(g)).any()
        rre, rte = ops.hypothesis_gates(dev(T, gpu), dev(gt, gpu), counts, return_errors=True)
        rre, rte = rre.cpu().numpy(), rte.cpu().numpy()
        want_total += np.array(c64)
        print(f"n {n} general_gt {general_gt}: counts {c64}, max |rre - fp64| {np.abs(rre - rre64)[plain].max():.3g}")
        assert counts.cpu().tolist() == want_total.tolist()                            # (accumulated over the two calls)
        # errors: rre within 4 x the fp32 statement's error at that angle, rte within its three roundings
        assert np.array_equal(np.isnan(rre), np.isnan(rre64)) and np.array_equal(np.isnan(rte), np.isnan(rte64))
        assert (np.abs(rre[plain] - rre64[plain]) <= 4 * yard[plain]).all()
        assert (np.abs(rte[plain] - rte64[plain]) <= 2.0 ** -22 * rte64[plain]).all()
        if special:
            assert np.isnan(rre[special["nan"]]) and np.isnan(rte[special["nan"]])      # a NaN trace stays NaN
            assert np.isinf(rte[special["inf_t"]]) and not o64[list(special.values())].any()
            assert np.array_equal(np.isnan(rre), np.isnan(rre32))
    ops.hypothesis_gates(dev(T, gpu), dev(gt, gpu), counts)                            # without the error outputs
    assert counts.cpu().tolist() == (want_total + np.array(c64)).tolist()


# ---- rre_deg ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", (1, 255, 256, 257))
def test_rre_deg_against_fp64(gpu, b):
    from umeregrobust_amd import ops
    R, R_hat, truth, yard = gc.rre_case(b)
    got = ops.rre_deg(dev(R, gpu), dev(R_hat, gpu)).cpu().numpy()
    err = np.abs(got - truth)
    print(f"b {b}: max error / yardstick {(err / yard).max():.3g}; yardsticks (deg) "
          + ", ".join(f"{a}: {gc.rre_pool(a)[3]:.2g}" for a in gc.RRE_ANGLES))
    assert got.dtype == np.float32 and (err <= 4 * yard).all(), (err / yard).max()


@pytest.mark.parametrize("b", (1, 255, 256, 257))
def test_rre_deg_identity_pi_clamp_and_nan(gpu, b):
    from umeregrobust_amd import ops
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (b, 3, 3)).copy()
    R = gc.random_rotations(b, np.random.RandomState(b)).astype(np.float32)
    run = lambda a, c: ops.rre_deg(dev(a, gpu), dev(c, gpu)).cpu().numpy()
    assert np.array_equal(run(eye, eye), np.zeros(b, np.float32))                      # trace 3 exactly
    half = eye.copy()
    half[:, 1, 1] = half[:, 2, 2] = -1.0                                               # trace -1 exactly
    yard = max(np.abs(gc.rre_statement(eye, half) - 180.0).max(), gc.EPS_FLOOR * 180.0)
    assert np.abs(run(eye, half).astype(np.float64) - 180.0).max() <= 4 * yard
    above = eye.copy()
    above[:, 0, 0] = np.float32(1.0 + 2.0 ** -20)                                      # trace 3 + 2^-20: clamped
    assert np.array_equal(run(eye, above), np.zeros(b, np.float32))
    below = eye.copy()
    below[:, 1, 1] = below[:, 2, 2] = np.float32(-1.0 - 2.0 ** -20)                    # trace below -1: clamped
    assert np.abs(run(eye, below).astype(np.float64) - 180.0).max() <= 4 * yard
    loud = R.copy()
    loud[b // 2] = np.nan
    loud[b - 1, 2, 1] = np.nan
    got = run(R, loud)
    want = np.zeros(b, bool)
    want[[b // 2, b - 1]] = True
    assert np.array_equal(np.isnan(got), want)                                         # NaN in, NaN out -- and nowhere else


# ---- corr_select_best -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", gc.SIZES)
def test_corr_select_best_ties_and_non_finite_scores(gpu, M):
    from umeregrobust_amd import ops
    T = np.random.RandomState(M + 1).randn(M, 4, 4).astype(np.float32)
    T[M // 2, 1, 2] = -0.0
    Td = dev(T, gpu)
    names = []
    for name, s, want in gc.select_cases(M):
        assert gc.select_truth(s) == want, name
        Tb, ib = ops.corr_select_best(dev(s, gpu), Td)
        assert ib.dtype == torch.int64 and ib.cpu().tolist() == [want], (name, ib.cpu().tolist(), want)
        assert np.array_equal(Tb.cpu().numpy().view(np.int32), T[want].view(np.int32)), name      # that row, bit for bit
        names.append(name)
    print(f"M {M}: {names}")
    if M >= 2049:
        assert {"same_thread_2", "same_wave_2", "other_waves_2"} <= set(names)
    if M == 5000:
        assert len(names) == len(gc.TIES) + 5


# ---- corr_weighted_features -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", gc.WEIGHTED_SHAPES + (gc.CANCEL_SHAPE + ("cancel",),), ids=lambda s: "x".join(map(str, s)))
def test_corr_weighted_features_against_fp64(gpu, shape):
    from umeregrobust_amd import ops
    sf, tf, sw, tw, s_truth, t_truth, mean = gc.weighted_case(shape[0], shape[1], cancel=len(shape) == 3)
    so, to = ops.corr_weighted_features(dev(sf, gpu), dev(tf, gpu), dev(sw, gpu), dev(tw, gpu))
    for got, f, w, truth in ((so, sf, sw, s_truth), (to, tf, tw, t_truth)):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == f.shape
        # mean -> fp32, feat - mean, times w: three roundings of at most 2^-24 each, on values no larger than |f| + |mean|
        bound = 2.0 ** -23 * (np.abs(f.astype(np.float64)) + np.abs(mean)) * np.abs(w.astype(np.float64))[:, None]
        err = np.abs(got.astype(np.float64) - truth)
        print(f"{shape}: max error {err.max():.3g}, largest error / bound {(err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0:.3g}")
        assert (err <= bound).all()
        assert (got[w == 0] == 0).all()
