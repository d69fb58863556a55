"""orthobasis_kernel (csrc/ortho.hip, every layout), svdvals_kernel and the consumers of the bases, on the rungs of tests/ortho_cases.py.

Judged against a 50-digit truth with no conditioning mask: matrices of cond up to 7e13 (UME moments of balls far from the origin) are
held to the same bars as well-conditioned ones, because their ill-conditioning is column grading, which a Householder QR does not suffer
from.  Every bar is 4 x a yardstick computed here from the truth (ortho_cases: e_round, e_lapack), never from the kernel's output;
tests/test_ortho_cpu.py asserts without a GPU that every rung qualifies and that the oracle used for the consumers deserves the name.

Batches: the judged matrices cycled into n = 1, 2, 7, 8, 9, 127, 128, 129, 257 slots -- both halves of a wavefront, the 8-matrix
workgroup, the 16 / 32 / 128 pads of the fragment layouts.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import ortho_cases as oc
from tests.conftest import load_golden
from tests.test_gpu_parity import N_, T_
from tests.test_oracle_golden import well_conditioned

pytestmark = pytest.mark.gpu

NS = [1, 2, 7, 8, 9, 127, 128, 129, 257]
PLAIN, ROWS, COLS, ROWS_H, COLS_H = 0, 1, 2, 3, 4
_PAD = {PLAIN: 1, ROWS: 16, COLS: 32, ROWS_H: 128, COLS_H: 32}


# ------------------------------------------------------------------------------------------------ the pool and its batches
@pytest.fixture(scope="module")
def pool():
    """every judged matrix: (mats f32 [N,32,4], rung name of each, OrderedDict rung -> Yard)"""
    rungs = oc.rungs()
    mats = np.concatenate(list(rungs.values()))
    rung_of = np.concatenate([[name] * len(m) for name, m in rungs.items()])
    yard = {name: oc.rung_yardsticks(m) for name, m in rungs.items()}
    for name, y in yard.items():
        assert max(y.e_round, y.e_lapack) <= oc.JUDGED_MAX, (name, y)         # no rung is skipped, silently or otherwise
    assert len(mats) < min(n for n in NS if n > 100)                          # the large batches hold every matrix
    return mats, rung_of, yard


def _slots(n, n_pool):
    """which pool matrix sits in each of n slots: the pool cycled, from a start that moves with n (small batches differ)"""
    return (np.arange(n) + 11 * n) % n_pool


@pytest.fixture(scope="module")
def plain(gpu, pool):
    """PLAIN Q of every batch: n -> (slots, Q f32 [n,32,4]), and the canonical Q of each pool matrix (from the largest batch)"""
    from umeregrobust_amd import ops
    mats = pool[0]
    out = {}
    for n in NS:
        s = _slots(n, len(mats))
        Q = N_(ops.ume_orthobasis(T_(mats[s], gpu)))
        assert Q.shape == (n, 32, 4) and Q.dtype == np.float32
        out[n] = (s, Q)
    s, Q = out[NS[-1]]
    canon = np.empty((len(mats), 32, 4), np.float32)
    canon[s] = Q
    assert len(set(s.tolist())) == len(mats)
    return out, canon


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


# ------------------------------------------------------------------------------------------------ projector, orthonormality
def test_plain_projector_and_orthonormality_per_rung(pool, plain):
    """Every slot of every batch: max |Q Q^T - P_truth| <= 4 max(e_round, e_lapack) of the matrix's rung, and |Q^T Q - I| within the
    same multiple of the fp32-rounded truth's own (and of that bar)."""
    mats, rung_of, yard = pool
    worst = {name: [0.0, 0.0] for name in yard}
    for n, (s, Q) in plain[0].items():
        for slot, i in enumerate(s):
            w = worst[rung_of[i]]
            w[0] = max(w[0], oc.err_P(Q[slot], oc.truth(mats[i])))
            w[1] = max(w[1], oc.err_orth(Q[slot]))
    for name, y in yard.items():
        eP, eO = worst[name]
        print(f"[ortho ladder] {name:12s} e_round {y.e_round:.2e} e_lapack {y.e_lapack:.2e} orth_round {y.orth_round:.2e} | "
              f"gpu |dP| {eP:.2e} (bar {oc.bar(y):.2e}) gpu |Q^T Q - I| {eO:.2e} (bar {oc.SLACK * y.orth_round:.2e})")
    for name, y in yard.items():
        eP, eO = worst[name]
        assert eP <= oc.bar(y), (name, eP, oc.bar(y))
        assert eO <= oc.SLACK * y.orth_round, (name, eO, y.orth_round)


def test_golden_g3_unmasked(gpu):
    """The 160 matrices of golden G3, each judged whenever its own yardstick is <= 1e-6: that is every row the suite's
    well_conditioned(max_cond=1e6) mask keeps and rows it throws away; one rung, one bar."""
    from umeregrobust_amd import ops
    g = load_golden("g3_ume_cdist.npz")
    ume = np.concatenate([g["ume1"], g["ume2"]])
    Y = np.array([oc.yardsticks(u) for u in ume])
    judged = Y[:, :2].max(axis=1) <= oc.JUDGED_MAX
    wc = well_conditioned(ume)
    assert judged[wc].all() and (judged & ~wc).sum() >= 1, (judged.sum(), wc.sum())
    y = oc.Yard(*Y[judged].max(axis=0))
    Q = N_(ops.ume_orthobasis(T_(ume, gpu)))
    eP = max(oc.err_P(Q[i], oc.truth(ume[i])) for i in np.flatnonzero(judged))
    eO = max(oc.err_orth(Q[i]) for i in range(len(ume)))                    # orthonormal on all 160, rank-deficient or not
    print(f"[ortho ladder] g3 ({int(judged.sum())} of {len(ume)}; mask keeps {int(wc.sum())}) e_round {y.e_round:.2e} e_lapack {y.e_lapack:.2e} "
          f"orth_round {y.orth_round:.2e} | gpu |dP| {eP:.2e} (bar {oc.bar(y):.2e}) gpu |Q^T Q - I| {eO:.2e}")
    assert eP <= oc.bar(y), (eP, oc.bar(y))
    assert eO <= oc.SLACK * Y[:, 2].max(), (eO, Y[:, 2].max())


# ------------------------------------------------------------------------------------------------ Q as LAPACK's
def test_q_is_lapacks_signs_included(pool, plain):
    """The conventions family and the generic rungs k <= 3: Q itself within the rung's projector bar of numpy.linalg.qr's Q, column
    for column and sign for sign; every column the tau = 0 convention leaves as e_k is e_k to the bit."""
    mats, rung_of, yard = pool
    canon = plain[1]
    eye = np.eye(32, dtype=np.float32)[:, :4]
    n_exact = 0
    for i in np.flatnonzero(np.isin(rung_of, ["conventions", "generic_0", "generic_3"])):
        Qn = oc.lapack_q(mats[i])
        d = np.abs(canon[i].astype(np.float64) - Qn).max(axis=0)
        assert d.max() <= oc.bar(yard[rung_of[i]]), (rung_of[i], i, d)
        Qt = oc.truth(mats[i]).Q
        for k in range(4):
            if np.array_equal(Qt[:, k], eye[:, k].astype(oc.LD)):
                assert np.array_equal(canon[i][:, k], eye[:, k]), (i, k)
                n_exact += 1
    assert n_exact == 14                                                      # zero, top4_triu: 4 + 4; one_column_j: 0 + 1 + 2 + 3
    names = list(oc.conventions())
    first = int(np.flatnonzero(rung_of == "conventions")[0])
    assert np.array_equal(canon[first + names.index("zero")], eye) and np.array_equal(canon[first + names.index("top4_triu")], eye)


# ------------------------------------------------------------------------------------------------ slot independence
def test_same_matrix_same_bits_in_every_slot(pool, plain):
    batches, canon = plain
    for n, (s, Q) in batches.items():
        assert np.array_equal(_bits(Q), _bits(canon[s])), n


@pytest.mark.parametrize("n", [2, 9, 129])
def test_nan_and_inf_neighbours_change_no_bit(gpu, pool, plain, n):
    """A matrix with one NaN and one with one inf, in an even and an odd slot (the two halves of a wavefront): the call returns and
    every other matrix of the batch comes out bit for bit as without them, in every layout."""
    from umeregrobust_amd import ops
    mats, canon = pool[0], plain[1]
    bad = oc.nonfinite()
    for at in ([(0, 0)], [(1, 1)]) if n == 2 else ([(4, 0), (7, 1)], [(n - 1, 0), (n - 4, 1)]):
        s = _slots(n, len(mats))
        batch = mats[s].copy()
        clean = np.ones(n, bool)
        for slot, which in at:
            batch[slot] = bad[which]
            clean[slot] = False
        Q = N_(ops.ume_orthobasis(T_(batch, gpu)))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Q[clean]), _bits(canon[s][clean])), (n, at)
        for layout in (ROWS, COLS):
            Qf = orc.decode_f32_fragments(N_(ops.ume_orthobasis(T_(batch, gpu), layout)), n, layout)
            assert np.array_equal(_bits(Qf[clean]), _bits(canon[s][clean])), (n, at, layout)
        sv = N_(ops.ume_svdvals(T_(batch, gpu)))
        sv0 = N_(ops.ume_svdvals(T_(mats[s], gpu)))
        assert np.array_equal(_bits(sv[clean]), _bits(sv0[clean])), (n, at)


def test_power_of_two_column_scales_change_no_bit(gpu):
    """Q(B diag(2^k)) == Q(B) to the bit: every operation of the routine scales exactly"""
    from umeregrobust_amd import ops
    Q0 = N_(ops.ume_orthobasis(T_(oc.graded_bases(), gpu)))
    for j in range(len(oc.GRADED_EXP)):
        assert np.array_equal(_bits(N_(ops.ume_orthobasis(T_(oc.graded(j), gpu)))), _bits(Q0)), oc.GRADED_EXP[j]


# ------------------------------------------------------------------------------------------------ layouts
def _raw_orthobasis(gpu, batch, layout, guard=4096):
    """umereg_ume_orthobasis_f32 into a buffer pre-filled with 0xA5 bytes, with a guard behind it -> (bytes written to, the guard)"""
    lib = __import__("umeregrobust_amd")._lib.load()
    n = batch.shape[0]
    nbytes = lib.umereg_qbasis_bytes(n, layout)
    assert nbytes == (n + _PAD[layout] - 1) // _PAD[layout] * _PAD[layout] * 512
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    ume = T_(batch, gpu)
    rc = lib.umereg_ume_orthobasis_f32(ctypes.c_void_p(ume.data_ptr()), n, layout, ctypes.c_void_p(buf.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    out = N_(buf)
    return out[:nbytes], out[nbytes:]


@pytest.mark.parametrize("n", NS)
def test_fp32_fragment_layouts(gpu, pool, plain, n):
    """ROWS and COLS decode bit-equal to PLAIN through the restated qoff_rows / qoff_cols; the offsets of the n bases are distinct,
    every other float of umereg_qbasis_bytes is written as zero, and nothing behind the buffer is touched."""
    mats = pool[0]
    s, Qp = plain[0][n]
    for layout in (PLAIN, ROWS, COLS):
        raw, guard = _raw_orthobasis(gpu, mats[s], layout)
        assert (guard == 0xA5).all(), (n, layout)
        f = raw.view(np.float32)
        if layout == PLAIN:
            assert f.size == n * 128 and np.array_equal(_bits(f.reshape(n, 32, 4)), _bits(Qp))
            continue
        assert f.size == orc.f32_fragment_floats(n, layout)
        off = orc.f32_fragment_offsets(n, layout)
        assert np.unique(off).size == n * 128 and off.max() < f.size
        assert np.array_equal(_bits(f[off]), _bits(Qp)), (n, layout)
        rest = np.ones(f.size, bool)
        rest[off.reshape(-1)] = False
        assert rest.sum() == f.size - n * 128 and (_bits(f[rest]) == 0).all(), (n, layout)


def _half_ulp_f16(h):
    return 0.5 * np.abs(np.spacing(h.astype(np.float16))).astype(np.float64)


@pytest.mark.parametrize("n", NS)
def test_split_f16_layouts(gpu, pool, plain, n):
    """ROWS_F16X2 and COLS_F16X2: hi is Q rounded to f16 (|hi - Q| <= half an f16 ulp of hi), hi + lo is within 2^-24 of the PLAIN
    Q, the two layouts hold the same halfs, the padding is written as zero and every byte is accounted for."""
    mats = pool[0]
    s, Qp = plain[0][n]
    Q = Qp.astype(np.float64)
    planes = {}
    for layout in (ROWS_H, COLS_H):
        raw, guard = _raw_orthobasis(gpu, mats[s], layout)
        assert (guard == 0xA5).all(), (n, layout)
        h = raw.view(np.float16)
        assert h.size == orc.split_f16_halfs(n, layout)
        off = orc.split_f16_offsets(n, layout)
        assert np.unique(off).size == n * 256 and off.max() < h.size
        hi, lo = orc.decode_split_f16(h, n, layout)
        assert (np.abs(hi.astype(np.float64) - Q) <= _half_ulp_f16(hi)).all(), (n, layout)
        e = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - Q)
        assert e.max() <= 2.0 ** -24, (n, layout, e.max() / 2.0 ** -24)
        rest = np.ones(h.size, bool)
        rest[off.reshape(-1)] = False
        assert rest.sum() == h.size - n * 256 and (_bits(h[rest]) == 0).all(), (n, layout)
        planes[layout] = (hi, lo)
    assert np.array_equal(_bits(planes[ROWS_H][0]), _bits(planes[COLS_H][0]))
    assert np.array_equal(_bits(planes[ROWS_H][1]), _bits(planes[COLS_H][1]))


# ------------------------------------------------------------------------------------------------ consumers
@pytest.fixture(scope="module")
def consumers():
    src, tgt = oc.consumer_sets()
    return src, tgt, orc.ume_cdist_f64(src, tgt)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_ume_cdist_on_far_balls_unmasked(gpu, consumers, precision):
    """The distance matrix of the far rungs (cond up to 7e13) against their perturbed copies and decoys meets the project's bars --
    2e-5 where D > 0.05, 2e-3 below -- on EVERY pair: no conditioning mask."""
    from umeregrobust_amd import ops
    src, tgt, D64 = consumers
    D = N_(ops.ume_cdist(T_(src, gpu)[None], T_(tgt, gpu)[None], precision=precision)[0]).astype(np.float64)
    far = D64 > 0.05
    e = np.abs(D - D64)
    for ci, c in enumerate(oc.FAR_C):
        r = slice(ci * oc.N_PER_RUNG, (ci + 1) * oc.N_PER_RUNG)
        print(f"[ortho consumers] ume_cdist {precision} sources |c| = {c:.0e}: max |dD| {e[r][far[r]].max():.2e} at D > 0.05 "
              f"({int(far[r].sum())} pairs), {e[r][~far[r]].max() if (~far[r]).any() else 0.0:.2e} below")
    assert far.sum() >= 0.9 * far.size
    assert e[far].max() <= 2e-5, e[far].max()
    assert e.max() <= 2e-3, e.max()


def test_rtume_dist_on_far_balls(gpu, consumers):
    """rtume_solve(with_dist=True): each far source paired with its own copy and with a decoy.  dist is 0.707 sqrt(8 - 2 s) evaluated
    in fp64 and rounded once to fp32, a value <= 2: within 2^-22 (that rounding, 2^-24 .. 2^-23, doubled) of the truth for D > 0.05."""
    from umeregrobust_amd import ops
    src, tgt, D64 = consumers
    n = src.shape[0]
    gi = np.concatenate([np.arange(n), np.arange(n)])
    hi = np.concatenate([np.arange(n), n + (np.arange(n) % (tgt.shape[0] - n))])
    _, dist = ops.rtume_solve(T_(src, gpu), T_(tgt, gpu), T_(gi, gpu), T_(hi, gpu), with_dist=True)
    dist = N_(dist).astype(np.float64)
    D = D64[gi, hi]
    want = 0.707 * np.sqrt(8.0 - 2.0 * (4.0 - D * D))
    ok = D > 0.05
    e = np.abs(dist - want)
    print(f"[ortho consumers] rtume dist: {int(ok.sum())} of {ok.size} pairs at D > 0.05, max |d dist| {e[ok].max():.2e} (bar {2.0 ** -22:.2e})")
    assert ok.sum() >= 0.9 * ok.size
    assert e[ok].max() <= 2.0 ** -22, e[ok].max()


def test_ume_match_f16r_on_far_balls(gpu, consumers):
    """ume_match(precision="f16r") returns the fp64 arg-min wherever the two best d^2 are more than 2e-5 apart -- which, asserted on
    the oracle, is at least 95 % of the rows."""
    from umeregrobust_amd import ops
    src, tgt, D64 = consumers
    ref = orc.ume_match_f64(src, tgt)
    clear = ref.d2sec - ref.d2min > 2e-5
    assert clear.mean() >= 0.95, clear.mean()
    assert np.array_equal(ref.argmin, D64.argmin(axis=1))
    m, d = ops.ume_match(T_(src, gpu)[None], T_(tgt, gpu)[None], precision="f16r")
    m, d = N_(m[0]), N_(d[0])
    print(f"[ortho consumers] ume_match f16r: {int(clear.sum())} of {clear.size} rows clear, {int((m == ref.argmin).sum())} equal the fp64 arg-min")
    assert np.array_equal(m[clear], ref.argmin[clear])


# ------------------------------------------------------------------------------------------------ singular values
@pytest.fixture(scope="module")
def sv_pool(pool):
    """the matrices whose singular values are judged (every rung but the conventions) and mpmath's svd_r of each"""
    mats, rung_of, _ = pool
    keep = rung_of != "conventions"
    return mats[keep], rung_of[keep], np.stack([oc.sigma_truth(a) for a in mats[keep]])


def test_svdvals_ladders(gpu, sv_pool):
    """Graded family: every sigma within 2^-23 RELATIVE of mpmath's svd_r (one-sided Jacobi keeps small singular values to
    working precision: a host restatement of the kernel's loop plus the fp32 rounding stays below 2^-24 on them).  Generic and far
    families: within 2^-23 sigma_1 absolute.  Descending order, and the same bits in every slot of every batch size."""
    from umeregrobust_amd import ops
    mats, rung_of, S = sv_pool
    canon = N_(ops.ume_svdvals(T_(mats, gpu)))
    assert canon.shape == (len(mats), 4) and canon.dtype == np.float32
    assert (np.diff(canon, axis=1) <= 0).all() and np.isfinite(canon).all()
    rel = np.abs(canon.astype(np.float64) - S) / S
    ab = np.abs(canon.astype(np.float64) - S) / S[:, :1]
    for name in dict.fromkeys(rung_of):
        r = rung_of == name
        print(f"[ortho ladder] svdvals {name:12s} sigma4/sigma1 {(S[r, 3] / S[r, 0]).min():.1e}: max rel {rel[r].max():.2e}, "
              f"max abs / sigma1 {ab[r].max():.2e} (bar {2.0 ** -23:.2e})")
    graded = np.char.startswith(rung_of, "graded")
    assert graded.sum() == 3 * oc.N_PER_RUNG and (S[graded, 3] / S[graded, 0]).min() < 1e-9
    assert rel[graded].max() <= 2.0 ** -23, rel[graded].max()
    assert ab[~graded].max() <= 2.0 ** -23, ab[~graded].max()
    for n in NS:
        s = _slots(n, len(mats))
        assert np.array_equal(_bits(N_(ops.ume_svdvals(T_(mats[s], gpu)))), _bits(canon[s])), n


def test_svdvals_conventions(gpu):
    """An exactly zero column (of +0.0 or -0.0) gives sigma = 0 exactly, one zero per such column; entries at 1e+-18 stay finite;
    descending order throughout."""
    from umeregrobust_amd import ops
    cases = oc.conventions()
    sv = N_(ops.ume_svdvals(T_(np.stack(list(cases.values())), gpu)))
    assert np.isfinite(sv).all() and (np.diff(sv, axis=1) <= 0).all() and (sv >= 0).all()
    for i, (name, a) in enumerate(cases.items()):
        zero_cols = int((a == 0).all(axis=0).sum())
        assert int((sv[i] == 0).sum()) == zero_cols, (name, sv[i], zero_cols)
    for name in ("big_1e18", "small_1e-18", "mixed_1e+-18"):
        i = list(cases).index(name)
        S = oc.sigma_truth(cases[name])
        assert sv[i, 0] > 0 and abs(sv[i, 0] / S[0] - 1) <= 2.0 ** -23, (name, sv[i], S)
