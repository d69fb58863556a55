"""Inputs, Python mirrors and fp64 truths of tests/test_voxel_key_cpu.py, tests/test_voxel_hash_edges_gpu.py and
tests/test_glue_edges_gpu.py.  Nothing here needs a device.

Voxel side: `quotients` / `keys` / `capacity` / `home_slot` restate csrc/voxel_key.h (the CPU module holds them against the header
itself); the GPU module uses them only to CHOOSE cells whose probes wrap or chain -- what it compares with is numpy's `unique` over
the fp32 quotient rows (`first_of_every_voxel`), which knows nothing about keys.

Glue side: every case is a function of its size and a seed; truths are fp64 on the fp32 inputs; "statement" functions are the
reference's own lines in fp32 on the CPU, the yardsticks the gates are multiples of."""
import functools

import numpy as np

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)

# ---- voxel keys --------------------------------------------------------------------------------------------------------------

GOLD = np.uint64(0x9E3779B97F4A7C15)
Q_MAX = 1048575                                       # |floor(p / voxel)| <= 2^20 - 1 is accepted
SWEEP_VOXELS = (0.3, 0.05, 0.6, 0.1)                  # thinning and correlation voxels of the benchmark configs
SWEEP_K = 4096
CAPACITY_N = (1, 511, 512, 513, 65536, 65537)


def capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def quotients(pts, voxel):
    """floor(p / voxel) in fp32, as torch.floor(coordinates / quantization_size): float32 [n, 3]"""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(pts, np.float32) / np.float32(voxel))


def keys(pts, voxel):
    """-> (ok bool [n], key uint64 [n], 0 where not ok)"""
    f = quotients(pts, voxel)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(f) <= np.float32(Q_MAX)).all(axis=1)
    q = (np.where(ok[:, None], f, 0).astype(np.int64) + (1 << 20)).astype(np.uint64)
    key = (q[:, 0] << np.uint64(42)) | (q[:, 1] << np.uint64(21)) | q[:, 2]
    return ok, np.where(ok, key, np.uint64(0))


def home_slot(key, cap):
    with np.errstate(over="ignore"):
        return (((np.asarray(key, np.uint64) * GOLD) >> np.uint64(32)) & np.uint64(cap - 1)).astype(np.int64)


def first_of_every_voxel(pts, voxel):
    """The lowest index of every distinct row of the fp32 quotient, ascending."""
    _, first = np.unique(quotients(pts, voxel).astype(np.int64), axis=0, return_index=True)
    return np.sort(first)


CELL_VOXEL = 0.25                                     # a power of two: (cell + 0.5) * voxel and its quotient are exact in fp32


def points_in_cells(cells):
    pts = ((np.asarray(cells, np.float64) + 0.5) * CELL_VOXEL).astype(np.float32)
    assert np.array_equal(quotients(pts, CELL_VOXEL), np.asarray(cells, np.float32))
    return pts


@functools.lru_cache(maxsize=4)
def cells_by_home_slot(cap):
    """2 M random cells of [-2000, 2000)^3, distinct, with their home slot in a table of `cap` slots."""
    rng = np.random.RandomState(cap)
    cells = np.unique(rng.randint(-2000, 2000, (2_000_000, 3)), axis=0)
    cells = cells[rng.permutation(len(cells))]
    ok, key = keys(points_in_cells(cells), CELL_VOXEL)
    assert ok.all()
    return cells, home_slot(key, cap)


def wrap_cloud():
    """600 distinct cells whose home slots are the last 6 of a 2048-slot table, in random order: the probes run past slot 2047."""
    cells, home = cells_by_home_slot(2048)
    pick = cells[home >= 2048 - 6][:600]
    assert len(pick) == 600 and capacity(600) == 2048
    return points_in_cells(pick)


def chain_cloud(cap):
    """300 cells that share the LAST home slot of a `cap`-slot table (one probe chain of 300 that starts by wrapping), padded with
    300 cells from anywhere.  cap = 2048: the chain cells twice and the padding once (900 points; all 600 cells twice would be 1200
    points and a 4096-slot table).  cap = 4096: all 600 cells twice.  Shuffled, so a second copy may sit anywhere after its first."""
    cells, home = cells_by_home_slot(cap)
    chain, rest = cells[home == cap - 1][:300], cells[home != cap - 1][:300]
    assert len(chain) == 300 and len(rest) == 300
    both = np.concatenate([chain, chain, rest] + ([rest] if cap == 4096 else []))
    assert capacity(len(both)) == cap, (len(both), cap)
    return points_in_cells(both[np.random.RandomState(cap + 1).permutation(len(both))])


def distinct_cloud(n):
    """n points, every one its own voxel, in random order."""
    rng = np.random.RandomState(n % 9973)
    flat = rng.choice(128 ** 3, n, replace=False)
    return points_in_cells(np.stack([flat % 128 - 64, (flat // 128) % 128 - 64, flat // 16384 - 64], axis=1))


def range_cloud():
    """voxel = 1: on every axis the quotients +-(2^20 - 1) and their neighbours +-(2^20 - 2), every point twice; two points that differ
    in the x field only and two that differ in the z field only; cells whose fields would carry into each other if one were a bit
    narrower or wider.  -> float32 [n, 3]"""
    cells = []
    for axis in range(3):
        for q in (Q_MAX, Q_MAX - 1, -Q_MAX, -Q_MAX + 1):
            c = [5, -7, 9]
            c[axis] = q
            cells.append(c)
    cells += [[5, -7, 9], [6, -7, 9], [5, -7, 10], [0, 0, Q_MAX], [0, 1, -Q_MAX], [0, 1, 0], [1, -Q_MAX, 0], [0, Q_MAX, 0],
              [Q_MAX, Q_MAX, Q_MAX], [-Q_MAX, -Q_MAX, -Q_MAX], [-Q_MAX, Q_MAX, -Q_MAX]]
    cells = np.array(cells + cells, np.int64)
    pts = (cells + 0.5).astype(np.float32)
    assert np.array_equal(quotients(pts, 1.0), cells.astype(np.float32))
    return pts[np.random.RandomState(20).permutation(len(pts))]


def beyond_range_point(axis, sign):
    c = np.array([[5.0, -7.0, 9.0]])
    c[0, axis] = sign * (Q_MAX + 1)
    pts = (c + 0.5).astype(np.float32)
    assert quotients(pts, 1.0)[0, axis] == sign * (Q_MAX + 1)
    return pts


def sweep_cloud(voxel, axis):
    """fl32(k v), its successor and its predecessor for k in [-SWEEP_K, SWEEP_K] on `axis`, the other two coordinates constant:
    the points at which a quotient that is not the IEEE fp32 division takes another floor.  -> float32 [3 (2 SWEEP_K + 1), 3]"""
    k = np.arange(-SWEEP_K, SWEEP_K + 1)
    x = (k * np.float64(voxel)).astype(np.float32)
    x = np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])
    pts = np.full((len(x), 3), np.float32(0.5 * voxel), np.float32)
    pts[:, axis] = x
    return pts[np.random.RandomState(int(voxel * 100)).permutation(len(x))]


def sweep_axis(i):
    return i % 3                                      # four voxel sizes on three axes: the fourth is on x again


# ---- match_prob ------------------------------------------------------------------------------------------------------------------

MATCH_TAUS = (0.05, 1.0)
MATCH_PATTERNS = ("uniform", "equal", "one_zero")
EPS_FLOOR = 2.0 ** -22


def match_d(n, pattern):
    rng = np.random.RandomState(n)
    if pattern == "uniform":
        return rng.uniform(0.0, 1.3, n).astype(np.float32)
    if pattern == "equal":
        return np.full(n, 0.7, np.float32)
    d = np.full(n, 1.3, np.float32)
    d[n // 2] = 0.0
    return d


def match_prob_truth(d, tau):
    a = np.exp((1.0 - d.astype(np.float64)) / tau)
    return a / a.sum()


def match_prob_statement(d, tau):
    """reference evaluate.py:235-236 in torch fp32 on the CPU"""
    import torch
    t = torch.from_numpy(d)
    a = torch.exp((1 - t) / tau)
    return (a / a.sum()).numpy()


# ---- rotation error and gates ------------------------------------------------------------------------------------------------------

DEG = np.float32(180.0) / np.float32(3.141592653589793)
RRE_ANGLES = (0.3, 0.95, 0.99, 1.01, 1.05, 1.2, 1.45, 1.49, 1.51, 1.55, 3.0, 30.0, 90.0, 170.0, 179.9)
DESIGNATED = (0.99, 1.01, 1.49, 1.51)                # 0.01 deg from a gate; everything else >= 0.05 deg away
POOL = 257


def _rotations(axes, angle_rad):
    u = axes / np.linalg.norm(axes, axis=1, keepdims=True)
    K = np.zeros((len(u), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -u[:, 2], u[:, 1], u[:, 2], -u[:, 0], -u[:, 1], u[:, 0]
    s, c = np.sin(angle_rad), np.cos(angle_rad)
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def random_rotations(m, rng):
    return _rotations(rng.randn(m, 3), rng.uniform(0.2, 3.0, m)[:, None, None])


def rre_truth(R, R_hat):
    """relative_rotation_error in fp64 on the fp32 inputs: degrees [b]"""
    with np.errstate(invalid="ignore"):
        tr = (R_hat.astype(np.float64) * R.astype(np.float64)).sum(axis=(1, 2))
        return np.degrees(np.arccos((np.clip(tr, -1.0, 3.0) - 1.0) / 2.0))


def rre_statement(R, R_hat):
    """reference utils/eval_utils.py:60-76 in torch fp32 on the CPU"""
    import torch
    R, R_hat = torch.from_numpy(R), torch.from_numpy(R_hat)
    tr = torch.einsum("bii->b", torch.matmul(R_hat, torch.transpose(R, 1, 2)))
    return (torch.acos((torch.clamp(tr, -1, 3) - 1) / 2) * (180 / torch.tensor(3.141592653589793))).numpy()


@functools.lru_cache(maxsize=None)
def rre_pool(angle_deg):
    """POOL pairs (R, R_hat) whose relative rotation is `angle_deg` about a random axis, both fp32; the fp64 truth on those fp32
    matrices; and the yardstick of the angle: the largest error of the fp32 statement over the pool, floored at 2^-22 of the angle
    (acosf within an ulp and one rounding of the conversion, for a trace that happens to come out exact)."""
    rng = np.random.RandomState(int(angle_deg * 100))
    R = random_rotations(POOL, rng)
    R_hat = _rotations(rng.randn(POOL, 3), np.radians(angle_deg)) @ R
    R, R_hat = R.astype(np.float32), R_hat.astype(np.float32)
    truth = rre_truth(R, R_hat)
    yard = max(np.abs(rre_statement(R, R_hat) - truth).max(), EPS_FLOOR * angle_deg)
    return R, R_hat, truth, float(yard)


def rre_case(b):
    """b pairs cycling through RRE_ANGLES -> (R, R_hat, truth, yardstick per row)"""
    R, R_hat, truth, yard = (np.empty((b, 3, 3), np.float32), np.empty((b, 3, 3), np.float32), np.empty(b), np.empty(b))
    for i in range(b):
        p = rre_pool(RRE_ANGLES[i % len(RRE_ANGLES)])
        j = (i // len(RRE_ANGLES)) % POOL
        R[i], R_hat[i], truth[i], yard[i] = p[0][j], p[1][j], p[2][j], p[3]
    return R, R_hat, truth, yard


def _succ(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


GATE_T = tuple(np.float32(v) for v in (0.0, 0.1, _succ(0.1), 0.3, _succ(0.3), 0.6, _succ(0.6), 0.05, 0.2, 0.45, 1.0))
GATE_ANGLES = tuple(a for a in RRE_ANGLES if a < 90.0)     # 11 translations x 12 angles, walked with coprime strides


def gates_case(n, general_gt):
    """n hypotheses against one ground truth -> (T float32 [n,4,4], gt float32 [4,4], yardstick of rre per row, special rows).
    general_gt = False: gt translation 0 and hypothesis translations EXACTLY on a gate (0.6f, 0.3f, 0.1f) or one ulp above it,
    along one axis with either sign, so rte = sqrtf(x x) = |x| carries no rounding.  general_gt = True: a ground truth with a
    translation of its own and hypothesis offsets 2 % off the gates.  With n >= 64 three rows are loud: all NaN (as rtume_kernel
    poisons a row), an infinite translation, an infinite rotation entry that sends the trace to -inf."""
    rng = np.random.RandomState(n + 7 * general_gt)
    gt = np.eye(4)
    gt[:3, :3] = random_rotations(1, rng)[0]
    if general_gt:
        gt[:3, 3] = rng.uniform(-20, 20, 3)
    gt = gt.astype(np.float32)
    k = np.arange(n)
    ang = np.array(GATE_ANGLES)[k % len(GATE_ANGLES)]
    T = np.zeros((n, 4, 4))
    T[:, 3, 3] = 1.0
    T[:, :3, :3] = gt[:3, :3].astype(np.float64) @ _rotations(rng.randn(n, 3), np.radians(ang)[:, None, None])
    x = np.array(GATE_T, np.float64)[(k // 2) % len(GATE_T)] * np.where(k % 2, -1.0, 1.0)
    T = T.astype(np.float32)
    if general_gt:
        off = rng.randn(n, 3)
        off *= (np.abs(x) * rng.choice([0.98, 1.02], n) / np.linalg.norm(off, axis=1))[:, None]
        T[:, :3, 3] = (gt[:3, 3].astype(np.float64) + off).astype(np.float32)
    else:
        T[k, k % 3, 3] = x.astype(np.float32)
    yard = np.array([rre_pool(a)[3] for a in GATE_ANGLES])[k % len(GATE_ANGLES)]
    special = {}
    if n >= 64:
        special = dict(nan=n - 1, inf_t=n // 2, inf_r=0)
        T[n - 1] = np.nan
        T[n // 2, 0, 3] = np.inf
        T[0, 1, 1] = -np.inf * np.sign(gt[1, 1])                                        # trace -inf: clamped to 180 degrees
    return T, gt, yard, special


G_RRE, G_RTE = (np.float32(1.5), np.float32(1.5), np.float32(1.0)), (np.float32(0.6), np.float32(0.3), np.float32(0.1))


def _counts(rre, rte):
    with np.errstate(invalid="ignore"):
        return [len(rre)] + [int(((rre <= a) & (rte <= b)).sum()) for a, b in zip(G_RRE, G_RTE)], \
            np.stack([(rre <= a) & (rte <= b) for a, b in zip(G_RRE, G_RTE)], axis=1)


def gates_fp32(T, gt):
    """hypothesis_gates in numpy fp32, operation by operation -> (rre, rte, counts, outcome bool [n,3])"""
    f = np.float32
    with np.errstate(all="ignore"):
        tr = np.zeros(len(T), f)
        for p in range(3):
            d = np.zeros(len(T), f)
            for q in range(3):
                d = d + gt[p, q] * T[:, p, q]
            tr = tr + d
        tr = np.where(tr < f(-1), f(-1), np.where(tr > f(3), f(3), tr))               # torch.clamp: NaN stays
        rre = np.arccos((tr - f(1)) / f(2)) * DEG
        dx, dy, dz = (T[:, a, 3] - gt[a, 3] for a in range(3))
        rte = np.sqrt(dx * dx + dy * dy + dz * dz)
    assert rre.dtype == f and rte.dtype == f
    return (rre, rte) + _counts(rre, rte)


def gates_fp64(T, gt):
    with np.errstate(all="ignore"):
        T64, g64 = T.astype(np.float64), gt.astype(np.float64)
        tr = (T64[:, :3, :3] * g64[:3, :3]).sum(axis=(1, 2))
        tr = np.where(tr < -1, -1.0, np.where(tr > 3, 3.0, tr))
        rre = np.degrees(np.arccos((tr - 1.0) / 2.0))
        rte = np.sqrt(((T64[:, :3, 3] - g64[:3, 3]) ** 2).sum(axis=1))
    return (rre, rte) + _counts(rre, rte)


# ---- corr_select_best --------------------------------------------------------------------------------------------------------------

TIES = {                                              # indices that share the maximum -> the least M they need
    "same_thread_2": (5, 5 + 1024), "same_thread_3": (5, 5 + 1024, 5 + 2048), "same_wave_2": (67, 104), "same_wave_3": (67, 80, 127),
    "other_waves_2": (10, 700), "other_waves_3": (10, 300, 900), "thread_and_wave": (1029, 6, 70), "last_two": (-2, -1),
}


def select_cases(M):
    """-> [(name, scores float32 [M], index the reference picks)]"""
    rng = np.random.RandomState(M)
    base = rng.uniform(-1, 1, M).astype(np.float32)
    out = []
    for name, at in TIES.items():
        at = [a % M for a in at] if min(at) < 0 else list(at)
        if max(at) < M and len(set(at)) == len(at):
            s = base.copy()
            s[at] = 2.0
            out.append((name, s, min(at)))
    out.append(("all_equal", np.full(M, 0.25, np.float32), 0))
    out.append(("all_minus_inf", np.full(M, -np.inf, np.float32), 0))
    s = base.copy(); s[M - 1] = np.inf
    out.append(("one_plus_inf", s, M - 1))
    s = base.copy(); s[0] = np.inf; s[M - 1] = np.nan
    out.append(("nan_last_beats_inf_first", s, M - 1))
    if M > 8:
        s = base.copy(); s[0] = np.inf; s[7] = np.nan; s[M - 1] = np.nan
        out.append(("lowest_nan", s, 7))
    return out


def select_truth(s):
    """torch.argmax's order: NaN above every number, the lowest index among equals"""
    nan = np.nonzero(np.isnan(s))[0]
    return int(nan[0]) if len(nan) else int(np.argmax(s))


# ---- corr_weighted_features -----------------------------------------------------------------------------------------------------------

WEIGHTED_SHAPES = ((1, 1), (7, 9), (255, 257), (256, 256), (1, 5000), (5000, 1))
CANCEL_SHAPE = (2049, 2951)


def weighted_case(Ns, Nt, cancel=False):
    """Features 100 + 1e-3 N(0,1) (their spread is 1e-5 of their size: a mean summed in fp32 would be wrong), weights in [0, 2] with
    exact zeros.  cancel: on top, +-2^27 on rows spaced so that single threads of the column sum see +2^27, a plain row, -2^27 in
    that order (5000 rows over 64 workgroups of 8 row lanes): an fp32 partial sum loses the plain row there.
    -> (src_feat, tgt_feat, src_w, tgt_w, fp64 truths of both outputs, fp64 mean [32])"""
    rng = np.random.RandomState(Ns * 31 + Nt)
    n = Ns + Nt
    feat = (100.0 + 1e-3 * rng.randn(n, 32)).astype(np.float32)
    if cancel:
        rows_per = (n + 63) // 64
        step = (np.arange(n) % rows_per) // 8
        whole = np.arange(n) // rows_per < n // rows_per                        # the last, partial workgroup stays plain: the mean stays ~100
        feat[(step == 0) & whole] += np.float32(2.0 ** 27)
        feat[(step == 2) & whole] -= np.float32(2.0 ** 27)
        assert abs(feat.astype(np.float64).mean() - 100.0) < 1.0
    w = rng.uniform(0, 2, n).astype(np.float32)
    w[rng.rand(n) < 0.2] = 0.0
    w[0] = 0.0
    w[n - 1] = 2.0
    mean = feat.astype(np.float64).mean(axis=0)
    truth = (feat.astype(np.float64) - mean) * w.astype(np.float64)[:, None]
    return feat[:Ns].copy(), feat[Ns:].copy(), w[:Ns].copy(), w[Ns:].copy(), truth[:Ns], truth[Ns:], mean
