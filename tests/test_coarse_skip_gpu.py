"""The coarse matcher's early exit and the cell-ordered pair chain: the matches are those of the exhaustive scan, bit for bit.

The pair chain (pair_match / pair_match_ragged / the capacity graph) writes its split-f16 bases in the cell order of the keypoints
(targets: a spatially uniform subsample first) and the Q-form coarse kernel drops a tile as soon as a partial sum proves that none of
its scores can reach a row's limit.  Neither may change a result: the arg-min is defined in fp64 over ALL targets, ties go to the lowest
ORIGINAL target index.  So every comparison here is array equality against (a) the same call with `force_exhaustive` (the refine kernel
scans every target of every row) and (b) the layered calls on the chain's own F, which run in the caller's order and which the existing
suite judges exactly against oracle.match_split_f64.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K_NN, R_NN, TAU = 750, 5.0, 0.05


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def _layered_stages(F, gpu):
    """orthobasis -> reset -> coarse -> refine through the public stage entries on F [2, n, 32, 4] (identity order)."""
    from umeregrobust_amd import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n = F.shape[1]
    ha = ops.ume_orthobasis(F[0], orc.QLAYOUT_ROWS_F16X2)
    hb = ops.ume_orthobasis(F[1], orc.QLAYOUT_COLS_F16X2)
    sb = lib.umereg_ume_match_q_scratch_bytes(n, n)
    scratch = torch.empty(sb, dtype=torch.uint8, device=gpu)
    scratch.fill_(0xA5)
    m = torch.empty(n, dtype=torch.int64, device=gpu)
    d = torch.empty(n, device=gpu)
    _lib.check(lib.umereg_ume_match_reset_f16(scratch.data_ptr(), sb, n, n, st), "reset")
    _lib.check(lib.umereg_ume_match_coarse_f16(ha.data_ptr(), hb.data_ptr(), n, n, scratch.data_ptr(), sb, st), "coarse")
    _lib.check(lib.umereg_ume_match_refine_f16(ha.data_ptr(), hb.data_ptr(), n, n, scratch.data_ptr(), sb, m.data_ptr(), d.data_ptr(), st),
               "refine")
    torch.cuda.synchronize()
    return m, d


def _assert_chain_exact(c, gpu, case, K=K_NN, r=R_NN, cap_graph=True):
    """c = [src_pts, tgt_pts, src_feat, tgt_feat, src_kp, tgt_kp] on the device.  Every chain form == exhaustive == layered."""
    from umeregrobust_amd import ops
    n = c[4].shape[0]
    F, m, d, prob = ops.pair_match_ragged(*c, K, r, tau=TAU)
    Fx, mx, dx, px = ops.pair_match_ragged(*c, K, r, tau=TAU, opts=ops.MatchOpts(force_exhaustive=1))
    assert torch.equal(F, Fx), case
    assert torch.equal(m, mx) and torch.equal(d, dx) and torch.equal(prob, px), (case, int((m != mx).sum()), int((d != dx).sum()))
    ml, dl = ops.ume_match(F[0:1].contiguous(), F[1:2].contiguous(), precision="f16r")
    assert torch.equal(m, ml) and torch.equal(d, dl), (case, "layered one-call", int((m != ml).sum()))
    ms, ds = _layered_stages(F, gpu)
    assert torch.equal(m[0], ms) and torch.equal(d[0], ds), (case, "layered stages", int((m[0] != ms).sum()))
    for o in (ops.MatchOpts(splits=3), ops.MatchOpts(share_mask=0), ops.MatchOpts(variant=1)):      # other plans, the P-form: same result
        _, mo, do, _ = ops.pair_match_ragged(*c, K, r, tau=TAU, opts=o)
        assert torch.equal(m, mo) and torch.equal(d, do), (case, o.key())
    if c[0].shape[0] == c[1].shape[0]:
        a = ops.pair_match(torch.stack(c[0:2]), torch.stack(c[2:4]), torch.stack(c[4:6]), K, r, tau=TAU)
        assert torch.equal(a[1], m) and torch.equal(a[2], d) and torch.equal(a[3], prob), (case, "stacked")
    if cap_graph:
        cap = max(c[0].shape[0], c[1].shape[0]) + 300
        g = ops.PairMatchCapGraph(gpu, cap, n, K, r, TAU)
        for _ in range(2):                       # a replay over a workspace the previous replay left behind
            g.launch(*c, 0, torch.cuda.current_stream(gpu).cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(g.F, F) and torch.equal(g.m, m) and torch.equal(g.d, d) and torch.equal(g.prob, prob), (case, "cap graph")
        del g
    assert int(m.min()) >= 0 and int(m.max()) < n
    return F, m, d


def _dev_pair(p, gpu):
    return [T_(x, gpu) for x in (p.src_pts, p.tgt_pts, p.src_feat, p.tgt_feat, p.src_inds, p.tgt_inds)]


@pytest.mark.parametrize("shape", ["KT", "KTr", "ROT", "NS", "SY"])
def test_chain_equals_exhaustive_and_layered_at_the_benchmark_shapes(gpu, shape):
    """The five benchmark shapes, a plain and a hard pair each (KTr: a ragged pair): on a hard pair many rows have no true match, so
    their limits stay low and nothing may be skipped for them, while their neighbours in the same wave skip."""
    from umeregrobust_amd.synth import synth_pair_cfg
    for hard in (False, True):
        if shape == "KTr":
            p = synth_pair_cfg(300 + hard, "KT", hard=hard, n_src=50000, n_tgt=41300)
        elif shape == "ROT":
            p = synth_pair_cfg(310 + hard, "KT", kind="rot", hard=hard)
        else:
            p = synth_pair_cfg(320 + hard, shape, hard=hard)
        _assert_chain_exact(_dev_pair(p, gpu), gpu, (shape, hard), cap_graph=not hard)


@pytest.mark.parametrize("n_kp", [5, 63, 64, 65, 500, 777, 1001])
def test_chain_keypoint_counts_at_the_edges_of_the_slot_order(gpu, n_kp):
    """n_kp below the ordered path (< 64: identity order), at its edge, not a multiple of 8 (the subsample's stride) or 32 (a target
    tile), and 8 k + 1 (the subsample holds one slot more than n / 8)."""
    from umeregrobust_amd.synth import synth_pair, synth_pair_hard
    for seed, f, ns, nt in ((41, synth_pair, 6000, 6000), (42, synth_pair_hard, 5121, 4000)):
        p = f(seed + n_kp, n_src=ns, n_tgt=nt, n_kp=n_kp)
        _assert_chain_exact(_dev_pair(p, gpu), gpu, (n_kp, seed))


def test_chain_degenerate_geometry(gpu):
    """All keypoints in ONE grid cell (the cell order is then whatever the scatter's atomics made of it); keypoints with nobody but
    themselves in their ball (isolated points far from the scene); the same point drawn several times as a target keypoint (exactly equal
    targets, in slots that the cell order puts side by side and the subsample tears apart: the tie goes to the lowest ORIGINAL index)."""
    from umeregrobust_amd import ops
    from umeregrobust_amd.synth import synth_pair
    rng = np.random.RandomState(7)
    # one cell: a 2 m cube, cell edge 2.5 m
    n, nk = 3000, 640
    pts = rng.uniform(-1.0, 1.0, (2, n, 3)).astype(np.float32)
    feat = rng.standard_normal((2, n, 32)).astype(np.float32)
    feat /= np.linalg.norm(feat, axis=2, keepdims=True)
    kp = np.stack([rng.choice(n, nk, replace=False), rng.choice(n, nk, replace=False)]).astype(np.int64)
    _assert_chain_exact([T_(pts[0], gpu), T_(pts[1], gpu), T_(feat[0], gpu), T_(feat[1], gpu), T_(kp[0], gpu), T_(kp[1], gpu)], gpu, "one cell")
    # isolated keypoints
    p = synth_pair(51, N=8000, n_kp=900)
    sp, tp = p.src_pts.copy(), p.tgt_pts.copy()
    lone = np.arange(40)
    sp[p.src_inds[lone]] = np.stack([400.0 + 30.0 * lone, -300.0 + 0.0 * lone, 2.0 + 0.0 * lone], axis=1)
    tp[p.tgt_inds[lone + 100]] = np.stack([-500.0 - 25.0 * lone, 350.0 + 0.0 * lone, 1.0 + 0.0 * lone], axis=1)
    cnt = orc.ume_moments(sp, sp[p.src_inds[lone]], p.src_feat, K_NN, R_NN, "f64", return_count=True)[1]
    assert (np.asarray(cnt) <= 1).all()                              # the case is what it is named for
    c = [T_(x, gpu) for x in (sp, tp, p.src_feat, p.tgt_feat, p.src_inds, p.tgt_inds)]
    _assert_chain_exact(c, gpu, "isolated")
    # repeated target keypoints: slots 3, 200, 411 and 899 are the twin of source keypoint 17
    p = synth_pair(52, N=8000, n_kp=900)
    ti = p.tgt_inds.copy()
    twin = p.tgt_twin_of_src[p.src_inds[17]] if hasattr(p, "tgt_twin_of_src") else ti[0]
    ti[[200, 3, 411, 899]] = twin
    c = [T_(x, gpu) for x in (p.src_pts, p.tgt_pts, p.src_feat, p.tgt_feat, p.src_inds, ti)]
    F, m, d = _assert_chain_exact(c, gpu, "repeated targets")
    assert torch.equal(F[1, 3], F[1, 200]) and torch.equal(F[1, 3], F[1, 899])
    hit = N_(m[0])
    assert not np.isin(hit, [200, 411, 899]).any()                  # an exact tie never goes to the later copy
    if hasattr(p, "tgt_twin_of_src"):
        assert hit[17] == 3


# ---- bases built to break the bound, through the layered matcher (the same coarse kernel, caller's order) ---------------------------
def _orthonormal(rng, n, k=6):
    """n orthonormal frames of k columns in R^32 (fp64)"""
    q = np.linalg.qr(rng.standard_normal((n, 32, k)))[0]
    return q


def _partial_scores(Qi, Qj):
    """[4] cumulative sums of |Qi^T q_jb|^2 over the target's basis columns b"""
    return np.cumsum(((Qi.T @ Qj) ** 2).sum(axis=0))


def _bound_case(name, rng, n1=256, n2=4096):
    """(u1 [n1,32,4], u2 [n2,32,4], row i's decoy and true target) -- see test_bases_built_to_break_the_bound"""
    fr = _orthonormal(rng, n1)                       # u1..u4 = the source basis, w, w2 orthogonal to it
    u, w, w2 = fr[:, :, :4], fr[:, :, 4], fr[:, :, 5]
    u1 = u.copy()
    u2 = rng.standard_normal((n2, 32, 4))
    decoy = np.arange(n1)                            # the first eight tiles
    true = n2 - 1 - 3 * np.arange(n1)                # scattered over the last quarter
    if name == "first column orthogonal":
        # decoy: shares u1, u2 and most of u3 -> s = 2.95; true best: [w, u1, u2, u3] -> s_partial(1) = 0, s = 3
        c2 = 0.95
        u2[decoy] = np.stack([u[:, :, 0], u[:, :, 1], np.sqrt(c2) * u[:, :, 2] + np.sqrt(1 - c2) * w, w2], axis=2)
        u2[true] = np.stack([w, u[:, :, 0], u[:, :, 1], u[:, :, 2]], axis=2)
    elif name == "late columns carry the score":
        # decoy s = 3.5, limits above 3 c: unrelated tiles stop at the FIRST test; true best: first column mostly outside -> 0.6 + 3
        u2[decoy] = np.stack([u[:, :, 0], u[:, :, 1], u[:, :, 2], np.sqrt(0.5) * u[:, :, 3] + np.sqrt(0.5) * w], axis=2)
        u2[true] = np.stack([np.sqrt(0.6) * u[:, :, 0] + np.sqrt(0.4) * w, u[:, :, 1], u[:, :, 2], u[:, :, 3]], axis=2)
    elif name == "low scores everywhere":
        # sources in channels 0..15, targets in 16..31 plus a little of everything: no score reaches 1, limits stay near zero
        u1 = np.zeros((n1, 32, 4)); u1[:, :16] = rng.standard_normal((n1, 16, 4))
        u2 = 0.15 * rng.standard_normal((n2, 32, 4)); u2[:, 16:] += rng.standard_normal((n2, 16, 4))
        decoy = true = None
    else:
        raise KeyError(name)
    return u1.astype(np.float32), u2.astype(np.float32), decoy, true


@pytest.mark.parametrize("name", ["first column orthogonal", "late columns carry the score", "low scores everywhere"])
def test_bases_built_to_break_the_bound(gpu, name):
    """Every row meets a good decoy in the first tiles (its limit is high from then on) and its true best late, in a tile whose first
    column says nothing (s_partial(1) = 0 of s = 3) or little (0.6 of 3.6): a test that forgot the remaining columns would drop it.
    And rows whose best score is below 1 everywhere: no tile may be dropped on their account.  The properties are checked on the CPU
    (fp64 bases of the oracle) before the GPU is asked."""
    from umeregrobust_amd import ops
    rng = np.random.RandomState(11)
    u1, u2, decoy, true = _bound_case(name, rng)
    Q1, Q2 = orc.orthobasis_f64(u1), orc.orthobasis_f64(u2)
    S = np.einsum("ika,jkb->ijab", Q1, Q2)
    S = (S ** 2).sum(axis=(2, 3))                                      # [n1, n2] scores
    if true is not None:
        rows = np.arange(u1.shape[0])
        assert np.array_equal(S.argmax(axis=1), true)                  # the late target IS the row's best ...
        second = np.sort(S, axis=1)[:, -2]
        assert np.allclose(second, S[rows, decoy]) and (S[rows, true] - second > 0.04).all()   # ... the decoy second, beyond the margin
        part = np.stack([_partial_scores(Q1[i], Q2[true[i]]) for i in rows])
        if name == "first column orthogonal":
            assert (part[:, 0] < 1e-10).all() and np.allclose(part[:, 3], 3.0) and np.allclose(S[rows, decoy], 2.95)
        else:
            assert np.allclose(part[:, 0], 0.6) and np.allclose(part[:, 3], 3.6) and np.allclose(S[rows, decoy], 3.5)
    else:
        assert S.max() < 1.0
    a, b = T_(u1, gpu)[None], T_(u2, gpu)[None]
    m, d = ops.ume_match(a, b, precision="f16r")
    mx, dx = ops.ume_match(a, b, precision="f16r", opts=ops.MatchOpts(force_exhaustive=1))
    assert torch.equal(m, mx) and torch.equal(d, dx), int((m != mx).sum())
    for o in (ops.MatchOpts(splits=1), ops.MatchOpts(splits=7), ops.MatchOpts(share_mask=0)):
        mo, do = ops.ume_match(a, b, precision="f16r", opts=o)
        assert torch.equal(mo, mx) and torch.equal(do, dx), o.key()
    if true is not None:
        assert np.array_equal(N_(m[0]), true)
    else:
        assert np.array_equal(N_(m[0]), S.argmax(axis=1))
