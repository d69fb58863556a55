"""Edge clouds and a numpy restatement of the device-side keypoint selection (umeregrobust_amd/gt_keypoints.py, csrc/gt_keypoints.hip).
Shared by tests/test_gt_keypoints_cpu.py (no GPU: the restatement against oracle.generate_ume_from_keypoints2, and that every cloud
sits on the edge it is named for) and tests/test_gt_keypoints_gpu.py (the kernels and the generator).  Test infrastructure only.

Construction.  One base cloud from tests/ball_cases.cloud(with_centres=True): M centres whose balls of radius R hold a PRESCRIBED
number of points (the centre counts), of five kinds (KINDS).  Every point is of a flat class except the ones a case names, the
target is the source under the ground-truth transform (so every source point overlaps it), hence the candidates of an element are
exactly the points the case names, in descending index order.  A `pattern` case names centres: it asks for a sequence of kinds
and takes, walking the centres from the highest index down, the next centre of the wanted kind.  A `random` case names a random
subset of ALL points; their hits are whatever the cloud gives (counted here by brute force)."""
import functools
from collections import namedtuple

import numpy as np

import ball_cases

R = 5.0
MAX_NN, MIN_NN = 64, 16
INTERSECTION_R = 0.6
FLAT, NON_FLAT = 9, 1
# kind -> points in the centre's ball, the centre included
KINDS = {"s": 3, "m": MIN_NN - 1, "d": MIN_NN, "p": MIN_NN + 1, "x": MAX_NN + 6}
DENSE = {"s": False, "m": False, "d": True, "p": True, "x": True}
PER_KIND = 44
N_TOTAL = 20 * 1024         # the base cloud is padded to this with far filler

# launch constants of csrc/gt_keypoints.hip (gt_keypoints.py restates them; the CPU test compares the two)
CAND_BLOCK, PICK_BLOCK, TEST_WAVES, MAX_TEST_WG, WORKERS_PER_SAMPLE = 256, 1024, 4, 512, 4
WG_CAP_SAMPLES = MAX_TEST_WG * TEST_WAVES // WORKERS_PER_SAMPLE     # num_samples at which the test kernel's workgroup cap sets in

Element = namedtuple("Element", "named")                    # named: int64 indices of the non-flat points (any order)
Case = namedtuple("Case", "name elements n kw error")       # n: the cloud is cut to its first n points (None = all); error: None / text


@functools.lru_cache(maxsize=1)
def base():
    kinds = [k for k in KINDS for _ in range(PER_KIND)]
    rng = np.random.RandomState(11)
    rng.shuffle(kinds)
    c = ball_cases.cloud([KINDS[k] - 1 for k in kinds], r=R, seed=3, order="random", n_total=N_TOTAL, with_centres=True)
    order = np.argsort(-c.kp_index)                          # centres from the highest index down
    return c.pts, c.kp_index[order], [kinds[i] for i in order]


def gt_tform():
    a = 0.3
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    T[:3, 3] = [1.5, -2.0, 0.25]
    return T


def pattern(seq):
    """indices of centres whose kinds, from the highest index down, spell `seq`"""
    _, idx, kinds = base()
    out, at = [], 0
    for want in seq:
        while at < len(kinds) and kinds[at] != want:
            at += 1
        assert at < len(kinds), f"the base cloud cannot spell {seq!r}"
        out.append(int(idx[at]))
        at += 1
    return Element(np.array(out, np.int64))


def walk(seq):
    """`pattern` spelled in the order the selection walks the candidates: from the LOWEST index up (the reference keeps the candidates
    in descending index order and then picks the dense POSITIONS in descending order)"""
    return pattern(seq[::-1])


def first_of(allowed, count):
    """the `count` highest-indexed centres of the kinds in `allowed`"""
    _, idx, kinds = base()
    out = [int(i) for i, k in zip(idx, kinds) if k in allowed][:count]
    assert len(out) == count
    return Element(np.array(out, np.int64))


def random_subset(count, seed, n=None):
    pts, _, _ = base()
    n = n or pts.shape[0]
    return Element(np.random.RandomState([seed, count]).choice(n, count, replace=False).astype(np.int64))


def _kw(num_samples, min_nn=MIN_NN, max_nn=MAX_NN):
    return dict(nn_r=R, max_nn=max_nn, min_nn=min_nn, num_samples=num_samples, flat_labels=[FLAT], nn_intersection_r=INTERSECTION_R)


def all_cases():
    ns = 5
    cs = [
        Case("last_candidate_completes", [walk("s" * 10 + "d" * 4 + "m" * 6 + "d")], None, _kw(ns), None),
        Case("first_candidates", [walk("d" * ns + "s" * 22)], None, _kw(ns), None),
        Case("exactly_num_samples", [walk("sdmdsdsmdsd" + "s" * 5)], None, _kw(ns), None),
        Case("num_samples_plus_one", [walk("sdmdsdsmdsd" + "s" * 5 + "p")], None, _kw(ns), None),
        Case("num_samples_minus_one", [walk("sdmdsdsmds" + "s" * 5)], None, _kw(ns), None),
        Case("dense_at_the_lowest_indices", [walk("d" * 6 + "m" * 10 + "s" * 10)], None, _kw(ns), None),
        Case("dense_at_the_highest_indices", [walk("s" * 10 + "m" * 10 + "d" * 6)], None, _kw(ns), None),
        Case("truncation_cuts_the_dense_away", [pattern("ddd" + "s" * 7), pattern("s" * 10 + "d" * 5)], None, _kw(ns), None),
        Case("one_candidate", [pattern("d")], None, _kw(1), None),
        Case("hits_around_min_nn_and_above_max_nn", [walk("mdpxsmdpxs")], None, _kw(40), None),
        Case("min_nn_zero_is_always_dense", [walk("smsms")], None, _kw(40, min_nn=0), None),
        Case("min_nn_above_max_nn", [pattern("xxdpx")], None, _kw(ns, min_nn=MAX_NN + 1), "no_keypoint"),
        Case("nothing_dense_anywhere", [pattern("smsm"), pattern("mmss")], None, _kw(ns), "no_keypoint"),
        Case("no_candidate_in_one_element", [pattern("dd"), Element(np.zeros(0, np.int64))], None, _kw(ns), "no_candidate"),
    ]
    for n in (63, 64, 65):          # one wavefront of candidates, one less, one more; fewer dense than asked for: no stop
        cs.append(Case(f"candidates_{n}", [first_of("sdm", n)], None, _kw(40), None))
    # the pick kernel's trip (PICK_BLOCK positions) and several trips: random candidates, more asked for than there are, so all are tested
    for n in (PICK_BLOCK - 1, PICK_BLOCK, PICK_BLOCK + 1, 2 * PICK_BLOCK + 1):
        cs.append(Case(f"candidates_{n}", [random_subset(n, 1)], None, _kw(n + 7, min_nn=50, max_nn=128), None))
    # nearly everything dense: the stop rule at work, at the num_samples where the workgroup cap sets in (WG_CAP_SAMPLES) and on both
    # sides of it; two elements of different lengths
    for num in (WG_CAP_SAMPLES - 1, WG_CAP_SAMPLES, WG_CAP_SAMPLES + 1):
        cs.append(Case(f"stop_at_{num}", [random_subset(2100, 2), random_subset(1500, 3)], None, _kw(num, min_nn=4, max_nn=48), None))
    # few workgroups in the test kernel (num_samples of them): most candidates wait for a second ticket
    for num in (4, 6):
        cs.append(Case(f"workers_{num}", [random_subset(300, 4)], None, _kw(num, min_nn=8, max_nn=48), None))
    # the cloud's size around the compaction's block (CAND_BLOCK rows) and its scan's slice (1024 blocks would need N > 2^18: not here)
    for n in (8 * CAND_BLOCK - 1, 8 * CAND_BLOCK, 8 * CAND_BLOCK + 1):
        cs.append(Case(f"cloud_of_{n}", [random_subset(200, 5, n)], n, _kw(20, min_nn=6, max_nn=48), None))
    return cs


def inputs(case):
    """numpy inputs of generate_ume_from_keypoints2 for the case: (src, seg, src_feat, tgt, tgt_feat, gt)."""
    pts, _, _ = base()
    n = case.n or pts.shape[0]
    pts = pts[:n]
    bs = len(case.elements)
    src = np.stack([pts] * bs)
    seg = np.full((bs, n, 1), FLAT, np.int64)
    for b, e in enumerate(case.elements):
        seg[b, e.named, 0] = NON_FLAT
    T = gt_tform()
    gt = np.stack([T] * bs)
    tgt = (src @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    feat = np.stack([ball_cases.features(n, 7)] * bs)
    return src, seg, feat, tgt, feat.copy(), gt


def hits_of(pts, index):
    """points with ((dx dx) + (dy dy)) + (dz dz) < r r, f32 with one rounding per operation, strict -- for every named index"""
    out = np.empty(len(index), np.int64)
    r2 = np.float32(R) * np.float32(R)
    for k, i in enumerate(index):
        d = pts[i][None] - pts
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[k] = int((d2 < r2).sum())
    return out


Selection = namedtuple("Selection", "cand lengths min_length hits dense kp_index record last with_kpts num_out error")


def select_ref(case):
    """The selection restated: candidates (descending), truncation to the batch minimum, density, ordered pick, record.  hits, dense and
    last are in WALK order (step 0 = the last candidate of the truncated list)."""
    pts, _, _ = base()
    n = case.n or pts.shape[0]
    pts = pts[:n]
    kw = case.kw
    ns, max_nn, min_nn = kw["num_samples"], kw["max_nn"], kw["min_nn"]
    bs = len(case.elements)
    cand = -np.ones((bs, n), np.int32)
    lengths = np.zeros(bs, np.int32)
    for b, e in enumerate(case.elements):
        c = np.sort(e.named)[::-1]
        cand[b, :len(c)] = c
        lengths[b] = len(c)
    L = int(lengths.min())
    hits, dense, last = [], [], []
    kp_index = -np.ones((bs, ns), np.int64)
    record = np.zeros((bs, 2), np.int32)
    for b in range(bs):
        order = cand[b, :L][::-1]                                   # the walk: from the end of the truncated list to its head
        h = hits_of(pts, order)
        d = np.minimum(h, max_nn) >= min_nn
        w = np.where(d)[0]
        k = min(len(w), ns)
        kp_index[b, :k] = order[w[:k]]
        record[b] = (k, lengths[b])
        hits.append(h); dense.append(d)
        last.append(int(w[k - 1]) if len(w) >= ns else L - 1)     # the last position a lazy scan needs: fewer than ns dense -> all
    with_kpts = record[:, 0] > 0
    error = "no_candidate" if L == 0 else ("no_keypoint" if not with_kpts.any() else None)
    num_out = 0 if error else int(min(record[with_kpts, 0].min(), ns))
    return Selection(cand, lengths, L, hits, dense, kp_index, record, last, with_kpts, num_out, error)


# ---- ball_any ----------------------------------------------------------------------------------------------------------------
def ball_any_ref(q, p, radius):
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros(q.shape[0], np.int32)
    for b in range(q.shape[0]):
        d = q[b][:, None, :] - p[b][None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[b] = int((d2 < r2).any(axis=1).sum())
    return out


def ball_any_inputs(Bk, K, seed, radius=INTERSECTION_R):
    """q near p (about half of the rows have a partner within the radius), the tail of p padded with the origin and the tail of q
    with one `t`-valued row, as the generator's neighbour tensors are"""
    rng = np.random.RandomState([seed, Bk, K])
    half = max(1.0, 0.5 * (3.0 * K) ** (1.0 / 3.0))            # about 0.3 strangers per ball: a row's answer is its partner's distance
    p = rng.uniform(-half, half, (Bk, K, 3)).astype(np.float32)
    q = (p[:, rng.permutation(K)] + rng.choice([0.3, 2.5], (Bk, K, 1)) * radius * rng.standard_normal((Bk, K, 3)) / np.sqrt(3)).astype(np.float32)
    pad = rng.randint(0, K // 2 + 1, Bk)
    t = np.array([1.5, -2.0, 0.25], np.float32)
    for b in range(Bk):
        if pad[b]:
            p[b, K - pad[b]:] = 0
            q[b, K - pad[b]:] = t
    return q, p


def lattice_345(K, inside):
    """p on an integer lattice, q = p + (3, 4, 0) * 0.125 * [1 or 1 - 2^-24 ...]: every q row is at EXACTLY 0.625 from its partner
    (and farther from every other p row); `inside` moves radius one ulp up, so that the strict test admits them."""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 3)[:K].astype(np.float32) * 4
    p = g[None]
    q = (g + np.array([0.375, 0.5, 0.0], np.float32))[None]
    radius = np.float32(0.625)
    if inside:
        radius = np.nextafter(radius, np.float32(1))
    return q.astype(np.float32), p.astype(np.float32), float(radius)
