"""Clouds with a PRESCRIBED number of points inside every query ball, for the ball search's top-K selection (csrc/ball_search.h),
and a Python restatement of the host rule that sizes its list (lds_plan).  Shared by tests/test_ball_plan_cpu.py (no GPU: the
restatement against the header, the switch points, and that every cloud is what it claims -- judged by the oracle's linear scan) and
tests/test_ball_search_edges_gpu.py (the kernels).  Test infrastructure only, host only.

Construction (cloud)
  centres      one per entry of `counts`, on a 3-D lattice of spacing 12 m with jitter +-0.5 m: centres are >= 11 m apart, so with r = 5
               the balls are disjoint, and so are the shells of near misses (5.75 + 5 < 11); the cloud stays compact, so the grid's
               cells stay near the radius
  inside       counts[q] points uniform in the ball of radius 0.9 r around centre q: 0.5 m inside the sphere, five orders of magnitude
               more than the fp32 rounding of coordinates ~100 m -- every arithmetic agrees that they are hits
  near misses  64 per query at distance 1.004 r .. 1.15 r (>= 2 cm outside): they lie in cells the search visits, and only the
               predicate rejects them
  order        which ORIGINAL index each point gets -- the top-K is "the first K by original index":
               random    a permutation
               scan      ascending in (z layer, y row, x): the order in which the search walks the grid, so that once a list was cut
                         to its K smallest every later arrival is above the threshold (dropped by `oi <= thr`)
               reverse   the opposite: every arrival is smaller than everything kept, every selection evicts, the threshold keeps
                         shrinking
               top       n_total = 2^k + 1 points; the balls' points take the HIGH indices, filler >= 20 m from every centre (at least half
                         of the cloud) the low ones: every hit index is >= 2^(k-1), and the single index 2^k -- the only one that needs
                         the highest bit the selection looks at -- is an inside point of query `owner`
  with_centres each centre is appended as a point of the cloud (a keypoint given as an index); its ball then has counts[q] + 1 hits
"""
import functools
from collections import namedtuple

import numpy as np

R = 5.0
SPACING = 12.0
JITTER = 0.5
NEAR_MISSES = 64
SEL_REGS = 20          # kSelRegs (ball_search.h)
SCAN_UNROLL = 4        # kScanUnroll (grid.h)
MAX_K = 7680           # kMaxBallK
WAVE = 64

# the K the GPU tests run at every plan edge, and the index orders
GPU_K = [1, 64, 65, 750, 768, 769, 960, 961, 1472, 1473, 4032, 4033, 7680]
ORDERS = ["random", "scan", "reverse"]
VALU_K = [961, 1473, 4033]          # acc="f64valu" = the default, byte for byte
MANY_K = [1473, 4032]               # 131 queries: more than one workgroup's waves
LENGTHS_K = [750, 961, 1473]
PAIR_K = [961, 1473, 4033]
TOP_K = [64, 750, 961]
TOP_BITS = [15, 16]
N_MANY = 131
N_PAIR_KP = 67


def plan(K, sel_regs=SEL_REGS, scan_unroll=SCAN_UNROLL):
    """lds_plan(K, &cap, &waves) restated: ints per wavefront's list, wavefronts per workgroup."""
    kpad = (K + 63) // 64 * 64
    reg_cap = sel_regs * WAVE
    cap_min = kpad + (scan_unroll + 1) * WAVE
    cap_big = max(2 * kpad + 64, cap_min)
    cap = min(reg_cap, cap_big) if cap_min <= reg_cap else cap_big
    waves = 4 if cap * 4 * 4 <= 48 * 1024 else (2 if cap * 4 * 2 <= 64 * 1024 else 1)
    return cap, waves


def in_registers(K, sel_regs=SEL_REGS, scan_unroll=SCAN_UNROLL):
    """keep_k_smallest's choice: the selection runs in registers iff the list fits kSelRegs entries per lane."""
    return plan(K, sel_regs, scan_unroll)[0] <= sel_regs * WAVE


def counts_for(K, cap):
    """Hits per ball that sit on every comparison of the streaming selection for this plan (negative ones dropped, repeats once)."""
    c = [0, 1, K - 1, K, K + 1,                                                     # the final `cnt > K`
         cap - 257, cap - 256, cap - 255, cap - 128, cap - 127, cap, cap + 1,       # make_room: cnt > cap - chunks * 64, chunks = 4 / 2
         2 * cap + K, 6 * cap]                                                      # several selections per ball
    j = 64
    while j <= K:                                                                   # sort_kept pads to a power of two
        c += [j - 1, j, j + 1]
        j *= 2
    out = []
    for v in c:
        if v >= 0 and v not in out:
            out.append(v)
    return out


Cloud = namedtuple("Cloud", "centres pts counts kp_index")   # counts: hits per ball (int64 [m]); kp_index: int64 [m] or None


def _lattice(m, rng):
    nz = min(4, int(np.ceil(m ** (1.0 / 3.0))))
    nxy = int(np.ceil(np.sqrt(m / nz)))
    g = np.stack(np.meshgrid(np.arange(nxy), np.arange(nxy), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)[:m]
    return (g * SPACING + rng.uniform(-JITTER, JITTER, (m, 3))).astype(np.float32)


def _shell(rng, n, lo, hi, volume):
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = rng.uniform(0.0, 1.0, (n, 1))
    rad = hi * np.cbrt(u) if volume else lo + (hi - lo) * u
    return d * rad


def cloud(counts, r=R, seed=0, order="random", n_total=None, with_centres=False, owner=0):
    counts = np.asarray(counts, np.int64)
    m = len(counts)
    rng = np.random.RandomState([seed, m, int(counts.sum()) % (1 << 31)])
    centres = _lattice(m, rng)
    c64 = centres.astype(np.float64)
    parts, ball_of = [], []
    for q in range(m):
        parts.append(c64[q] + _shell(rng, int(counts[q]), 0.0, 0.9 * r, True))
        parts.append(c64[q] + _shell(rng, NEAR_MISSES, 1.004 * r, 1.15 * r, False))
    n_ball = int(counts.sum()) + NEAR_MISSES * m
    if with_centres:
        parts.append(c64)
    n_geom = n_ball + (m if with_centres else 0)
    n_fill = 0
    if n_total is not None:
        n_fill = n_total - n_geom
        assert n_fill >= 0, (n_total, n_geom)
        # filler: a slab beyond the lattice, >= 20 m from every centre
        hi = c64.max(axis=0) + 6.0
        lo = c64.min(axis=0) - 6.0
        f = rng.uniform(0.0, 1.0, (n_fill, 3)) * np.array([20.0, hi[1] - lo[1], hi[2] - lo[2]]) + np.array([hi[0] + 20.0, lo[1], lo[2]])
        parts.append(f)
    geom = np.concatenate(parts).astype(np.float32)
    N = geom.shape[0]
    # index_of[g]: the original index of generated point g
    if order == "random":
        index_of = rng.permutation(N)
    elif order in ("scan", "reverse"):
        mn = geom.min(axis=0)
        zc = np.floor((geom[:, 2] - mn[2]) / np.float32(1.0001 * r))
        yc = np.floor((geom[:, 1] - mn[1]) / np.float32(0.50005 * r))
        walk = np.lexsort((geom[:, 0], yc, zc))          # walk[i] = the generated point visited i-th
        index_of = np.empty(N, np.int64)
        index_of[walk] = np.arange(N) if order == "scan" else N - 1 - np.arange(N)
    elif order == "top":
        assert n_total is not None and ((n_total - 1) & (n_total - 2)) == 0 and n_fill * 2 >= n_total - 1 and counts[owner] > 0
        index_of = np.empty(N, np.int64)
        index_of[n_geom:] = rng.permutation(n_fill)                      # filler: the low indices
        first_of_owner = int(counts[:owner].sum()) + NEAR_MISSES * owner    # an inside point of `owner`
        rest = np.delete(np.arange(n_geom), first_of_owner)
        index_of[rest] = n_fill + rng.permutation(n_geom - 1)
        index_of[first_of_owner] = N - 1                                 # = 2^k
    else:
        raise ValueError(order)
    pts = np.empty_like(geom)
    pts[index_of] = geom
    kp_index = None
    if with_centres:
        kp_index = index_of[n_ball:n_geom].astype(np.int64)
        assert np.array_equal(pts[kp_index], centres)
    return Cloud(centres, pts, counts + (1 if with_centres else 0), kp_index)


def features(N, seed):
    """Non-negative features (|normals|, rows normalised): the moments' normaliser does not cancel."""
    f = np.abs(np.random.RandomState([seed, N]).standard_normal((N, 32))).astype(np.float32)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f


# ------------------------------------------------------------------------------------------------ the cases the GPU tests run
Case = namedtuple("Case", "name K kwargs")     # cloud(**kwargs), searched with K


def _seed(*a):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(a)) % 100003


def edge_case(K, order):
    return Case(f"edge-{K}-{order}", K, dict(counts=tuple(counts_for(K, plan(K)[0])), seed=_seed(1, K, ORDERS.index(order)), order=order))


def many_case(K):
    cap = plan(K)[0]
    rng = np.random.RandomState([2, K])
    counts = rng.choice([K - 1, K, K + 1, cap + 1], N_MANY)
    return Case(f"many-{K}", K, dict(counts=tuple(int(c) for c in counts), seed=_seed(2, K), order="random"))


def dense_case():
    K = 750
    cap = plan(K)[0]
    counts = list(range(K - 2, K + 3)) + list(range(cap - 300, cap + 45))
    return Case("dense-750", K, dict(counts=tuple(counts), seed=_seed(3), order="random"))


def small_case(K):
    return Case(f"small-{K}", K, dict(counts=tuple(range(73)), seed=_seed(4, K), order="random"))


def top_case(K, bits, extra):
    """The ball of query 0 holds index 2^bits and has K + extra hits: extra = 0 -> 2^bits must be kept, 1 -> it is the one dropped."""
    n_total = (1 << bits) + 1
    cap = plan(K)[0]
    counts = [K + extra]
    for c in (K + 1, cap + 1, K - 1, 2 * cap + 1):
        if sum(counts) + c + NEAR_MISSES * (len(counts) + 1) <= n_total // 2:
            counts.append(c)
    return Case(f"top-{K}-{bits}-{extra}", K, dict(counts=tuple(counts), seed=_seed(5, K, bits, extra), order="top", n_total=n_total, owner=0))


def pair_case(K, side):
    """One cloud of a registration pair (side 0 = source, 1 = target): keypoints as indices, balls of counts + 1 hits."""
    cap = plan(K)[0]
    rng = np.random.RandomState([6, K, side])
    counts = rng.choice([K - 2, K - 1, K, cap, cap + 1] if side == 0 else [0, K - 2, K - 1, K, cap - 256, cap + 1], N_PAIR_KP)
    return Case(f"pair-{K}-{side}", K, dict(counts=tuple(int(c) for c in counts), seed=_seed(6, K, side), order="random", with_centres=True))


def all_cases():
    cs = [edge_case(K, o) for K in GPU_K for o in ORDERS] + [many_case(K) for K in MANY_K] + [dense_case()]
    cs += [small_case(K) for K in (750, 64)]
    cs += [top_case(K, b, e) for K in TOP_K for b in TOP_BITS for e in (0, 1)]
    cs += [pair_case(K, s) for K in PAIR_K for s in (0, 1)]
    return cs


@functools.lru_cache(maxsize=4)
def _build(name, K, items):
    return cloud(**dict(items))


def build(case):
    """The case's cloud (the last few are kept: the tests that share a cloud run next to each other)."""
    return _build(case.name, case.K, tuple(sorted(case.kwargs.items())))
