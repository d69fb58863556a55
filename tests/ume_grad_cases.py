"""Inputs, fp64 truths and yardsticks of tests/test_ume_grad_edges_gpu.py, all of it checkable without a GPU
(tests/test_ume_grad_plan_cpu.py): the Python mirror of csrc/ume_grad_plan.h and the shapes named for its features, the distance
and conditioning ladders, the closed form of the distance's gradient for a GIVEN D, and the per-row gate.  Imports the fp64 / fp32
restatement tests/ume_grad_ref.py and nothing from the library."""
import functools

import numpy as np
import torch

import ume_grad_ref as uref

# ---- the plan (csrc/ume_grad_plan.h) ----------------------------------------------------------------------------------------

ROW_TILES = 2                   # kRowTiles
ROW_KP = 8 * ROW_TILES          # kRowKp
MAX_KP = 1 << 22                # kMaxKp of ume_grad.hip


def pad_kp(n):
    return (n + ROW_KP - 1) // ROW_KP * ROW_KP


def plan(rows, cols):
    """(n_rt, n_jt, tiles_per_split, splits, n_work) of bwd_plan(rows, cols): rows = keypoints of the side whose gradient is formed"""
    n_rt = pad_kp(rows) // ROW_KP
    n_jt = pad_kp(cols) // 8
    splits = min((4096 + n_rt - 1) // n_rt, 32, n_jt)
    tps = (n_jt + splits - 1) // splits
    splits = (n_jt + tps - 1) // tps
    return n_rt, n_jt, tps, splits, n_rt * splits


def split_cap(rows):
    """the number of splits the row count allows before the columns are looked at"""
    n_rt = pad_kp(rows) // ROW_KP
    return min((4096 + n_rt - 1) // n_rt, 32)


def last_split(rows, cols):
    """tiles of the last split"""
    _, n_jt, tps, splits, _ = plan(rows, cols)
    return n_jt - (splits - 1) * tps


PAD_SHAPES = [(15, 17), (16, 16), (17, 15), (1, 17), (17, 1)]          # the 16-keypoint pad and the 8-column tile masks, both sides
SPLIT_SHAPES = [(40, 545), (40, 529), (2120, 560)]                     # short last splits, the cap below 32
TALL_SHAPE = (65552, 24)                                               # one split on side 1, hundreds of tiles per split on side 2
PLAN_LARGE = [2112, 2113, 2120, 4096, 4097, 10000, 65520, 65521, 65552, 100000, MAX_KP - 1, MAX_KP]

# ---- inputs -----------------------------------------------------------------------------------------------------------------

N_RUNG = 64
COLS = torch.tensor([1.0, 6.0, 6.0, 1.5])
D_RUNGS = [0.3, 0.1, 0.05, 0.02, 0.01, 0.008, 0.002, 0.0]       # sin t of the diagonal pairs; 0: the same subspace
D_RUNGS_ABOVE = [d for d in D_RUNGS if d >= 0.008]              # at least 2 x D_MIN: these pairs carry a gradient
D_RUNGS_BELOW = [0.002, 0.0]                                    # at or below D_MIN in the forward: no gradient
C_RUNGS = [1e1, 1e3, 1e5, 1e6, 1e7]
D_MIN_F32 = np.float32(4e-3)                                    # UMEREG_UME_CDIST_BWD_DMIN as the kernel compares it
MIXED_ILL = [5, 17, 40, 63]                                     # the rows of the mixed case at c = 1e6


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ume_like(g, *shape):
    """f32 [*shape, 32, 4] with columns of different scale and a column of mean 2, as dist_case of tests/test_ume_grad_gpu.py"""
    return torch.randn(*shape, 32, 4, generator=g) * COLS + torch.tensor([2.0, 0.0, 0.0, 0.0])


def dist_case(B, n1, n2, seed):
    """benign UME-like matrices: the first min(n1, n2) // 2 rows of ume2 are perturbed copies of ume1's (D about 0.1 ... 0.3)"""
    g = gen(seed)
    u1, u2 = ume_like(g, B, n1), ume_like(g, B, n2)
    m = min(n1, n2) // 2
    u2[:, :m] = u1[:, :m] + 0.08 * torch.randn(B, m, 32, 4, generator=g) * COLS
    gD = torch.randn(B, n1, n2, generator=g)
    return u1, u2, gD


@functools.lru_cache(maxsize=None)
def distance_rung(sin_t):
    """(ume1, ume2, dD diagonal only, dD dense), f32, B = 1, n = 64.  span ume2_i is span ume1_i with ONE basis vector turned by
    the angle t towards a unit vector orthogonal to the span: one principal angle t, three of 0, so D_ii = sin t up to the f32
    rounding of ume2; every other pair is a pair of unrelated subspaces."""
    g = gen(1000 + int(round(sin_t * 1e4)))
    n = N_RUNG
    u1 = ume_like(g, n)
    Q = torch.linalg.qr(u1.double()).Q
    v = torch.randn(n, 32, 1, generator=g, dtype=torch.float64)
    v = v - Q @ (Q.transpose(-1, -2) @ v)
    v = v - Q @ (Q.transpose(-1, -2) @ v)                   # (twice: orthogonal to the span to the last bit)
    N = v / v.norm(dim=-2, keepdim=True)
    t = float(np.arcsin(sin_t))
    Q2 = Q.clone()
    Q2[:, :, 2] = np.cos(t) * Q[:, :, 2] + np.sin(t) * N[:, :, 0]
    # A_i = 3 I + randn(4, 4); ume2 = Q2 A rounded to f32.  The rounding turns the span a little, the more the worse A_i is
    # conditioned: a draw whose fp64 D_ii is not within half the tolerance the CPU test asserts is drawn again.
    u2 = torch.zeros(n, 32, 4)
    todo = torch.ones(n, dtype=torch.bool)
    for _ in range(50):
        k = int(todo.sum())
        A = 3.0 * torch.eye(4, dtype=torch.float64) + torch.randn(k, 4, 4, generator=g, dtype=torch.float64)
        u2[todo] = (Q2[todo] @ A).float()
        d = uref.ume_cdist(u1[None].double(), u2[None].double())[0].diagonal()
        todo = (d - sin_t).abs() > 0.5e-5 * sin_t if sin_t > 0 else d > 1e-6
        if not bool(todo.any()):
            break
    assert not bool(todo.any()), "no draw of A_i keeps D_ii on the rung"
    g_diag = torch.diag(1.0 + torch.rand(n, generator=g))
    g_dense = torch.randn(n, n, generator=g)
    return u1[None], u2[None], g_diag[None], g_dense[None]


def conditioned(g, n, c):
    """f32 [n, 32, 4] = U diag(1, c^-1/3, c^-2/3, c^-1) V^T, U and V random with orthonormal columns"""
    s = torch.tensor([1.0, c ** (-1.0 / 3.0), c ** (-2.0 / 3.0), 1.0 / c], dtype=torch.float64)
    out = torch.zeros(n, 32, 4)
    todo = torch.ones(n, dtype=torch.bool)
    for _ in range(50):     # the f32 rounding moves sigma_min = 1 / c by a few percent at c = 1e7: such a draw is drawn again
        k = int(todo.sum())
        U = torch.linalg.qr(torch.randn(k, 32, 4, generator=g, dtype=torch.float64)).Q
        V = torch.linalg.qr(torch.randn(k, 4, 4, generator=g, dtype=torch.float64)).Q
        out[todo] = ((U * s) @ V.transpose(-1, -2)).float()
        todo = (torch.linalg.cond(out.double()) / c - 1).abs() > 0.025
        if not bool(todo.any()):
            break
    assert not bool(todo.any()), "no draw keeps cond within 2.5 % of c after rounding"
    return out


@functools.lru_cache(maxsize=None)
def cond_rung(c):
    """(ume1 of condition number c, benign ume2, dense dD), f32, B = 1, n = 64"""
    g = gen(2000 + int(round(np.log10(c) * 10)))
    u1 = conditioned(g, N_RUNG, c)
    u2 = ume_like(g, N_RUNG)
    gD = torch.randn(N_RUNG, N_RUNG, generator=g)
    return u1[None], u2[None], gD[None]


@functools.lru_cache(maxsize=None)
def mixed_case():
    """(ume1, ume2, dD, ill): one tensor of 60 benign rows and 4 rows (MIXED_ILL) at c = 1e6; ill: bool [64]"""
    g = gen(2999)
    u1 = ume_like(g, N_RUNG)
    u1[MIXED_ILL] = conditioned(g, len(MIXED_ILL), 1e6)
    u2 = ume_like(g, N_RUNG)
    gD = torch.randn(N_RUNG, N_RUNG, generator=g)
    ill = torch.zeros(N_RUNG, dtype=torch.bool)
    ill[MIXED_ILL] = True
    return u1[None], u2[None], gD[None], ill


def diag_mask(n1, n2):
    m = torch.zeros(1, n1, n2, dtype=torch.bool)
    i = torch.arange(min(n1, n2))
    m[:, i, i] = True
    return m


# ---- truths -----------------------------------------------------------------------------------------------------------------

def truth_and_yard(u1, u2, gD, drop=None):
    """(D fp64, (dume1, dume2) fp64, (dume1, dume2) of the same helper in fp32): autograd through the reference's own ume_cdist"""
    D, a, b = uref.cdist_grads(u1.double(), u2.double(), gD.double(), drop)
    _, ya, yb = uref.cdist_grads(u1.float(), u2.float(), gD.float(), drop)
    return D, (a, b), (ya, yb)


def truth_and_yard_tall(u1, u2, gD, block=4096):
    """the same with ume1's rows in blocks: dume1 is separable by row, dume2 is a sum over the blocks"""
    n1 = u1.shape[1]
    out = []
    for dt in (torch.float64, torch.float32):
        a, b, D = [], torch.zeros(u2.shape, dtype=dt), []
        for i0 in range(0, n1, block):
            Di, ai, bi = uref.cdist_grads(u1[:, i0:i0 + block].to(dt), u2.to(dt), gD[:, i0:i0 + block].to(dt))
            a.append(ai)
            b += bi
            D.append(Di)
        out.append((torch.cat(D, 1), torch.cat(a, 1), b))
    return out[0][0], out[0][1:], out[1][1:]


def cdist_grads_closed(ume1, ume2, D, g, keep=None):
    """(dume1, dume2) for a GIVEN D, in the dtype of the inputs, no batch dimension: w_ij = g_ij / (2 D_ij) where `keep` (bool
    [n1, n2], default everywhere) and 0 elsewhere, M1_i = sum_j w_ij Q2_j Q2_j^T Q1_i, dF1_i = -2 (I - Q1_i Q1_i^T) M1_i R1_i^-T
    (F = Q R), roles swapped for side 2.  With D = ume_cdist(ume1, ume2) this is the gradient autograd gives (pinned on the CPU)."""
    Q1, R1 = torch.linalg.qr(ume1)
    Q2, R2 = torch.linalg.qr(ume2)
    w = g / (2 * D)
    if keep is not None:
        w = torch.where(keep, w, torch.zeros_like(w))
    S = torch.einsum("ida,jdb->ijab", Q1, Q2)                       # Q1_i^T Q2_j
    M1 = torch.einsum("ij,jdb,ijab->ida", w, Q2, S)
    M2 = torch.einsum("ij,ida,ijab->jdb", w, Q1, S)

    def finish(M, Q, R):
        Y = M - Q @ (Q.transpose(-1, -2) @ M)
        return -2 * torch.linalg.solve(R, Y.transpose(-1, -2)).transpose(-1, -2)        # X R^T = Y
    return finish(M1, Q1, R1), finish(M2, Q2, R2)


# ---- the strict cut ---------------------------------------------------------------------------------------------------------

CUT_SHAPE = (48, 40)


def cut_values():
    """(predecessor, D_MIN, successor) as f32"""
    c = D_MIN_F32
    return np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1))


@functools.lru_cache(maxsize=None)
def cut_case():
    """(ume1, ume2, D f32, dD, keep): one benign 48 x 40 case (no batch dimension) whose D is the truth's, rounded to f32, with
    chosen entries replaced by D_MIN, its f32 predecessor and its successor: in one thread's 4 x 4 blocks (a lane of
    cdist_bwd_kernel holds rows 3 and 11, columns 1, 3, 5, 7 of the first tile), in the last real row and column (i = 47; j = 39
    with 8 padded columns behind it), and a whole row (20) and a whole column (17) at or below the cut: those two matrices get
    exactly 0.  keep = D > D_MIN, the kernel's strict comparison."""
    n1, n2 = CUT_SHAPE
    u1, u2, gD = dist_case(1, n1, n2, 77)
    D64 = uref.ume_cdist(u1.double(), u2.double())[0]
    D = D64.float().clone()
    lo, c, hi = (float(v) for v in cut_values())
    put = {(3, 1): c, (3, 3): lo, (3, 5): hi, (3, 7): c, (11, 1): hi, (11, 3): c, (11, 5): lo, (11, 7): hi,
           (47, 39): c, (47, 38): lo, (46, 39): hi, (47, 0): hi, (0, 39): c, (47, 37): hi}
    for j in range(n2):
        put[(20, j)] = c if j % 2 else lo
    for i in range(n1):
        put[(i, 17)] = lo if i % 2 else c
    for (i, j), v in put.items():
        D[i, j] = v
    keep = D > float(c)
    return u1[0], u2[0], D, gD[0], keep, put


# ---- yardstick and gate -----------------------------------------------------------------------------------------------------

def row_rel(x, truth):
    """|x_i - truth_i|_F / |truth_i|_F per 32 x 4 matrix (fp64; 0 / 0 = 0, e / 0 = inf)"""
    x, truth = x.detach().double().cpu(), truth.detach().double().cpu()
    e = (x - truth).flatten(-2).norm(dim=-1)
    t = truth.flatten(-2).norm(dim=-1)
    return torch.where(t > 0, e / t.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))


def row_stats(got, truth, yard, groups=None):
    """per group of rows (default: all rows one group): (GPU median, GPU max, helper median, helper max) of the row-relative error"""
    e_gpu, e_cpu = row_rel(got, truth).flatten(), row_rel(yard, truth).flatten()
    groups = {"rows": torch.ones_like(e_gpu, dtype=torch.bool)} if groups is None else groups
    return {k: (float(e_gpu[m].median()), float(e_gpu[m].max()), float(e_cpu[m].median()), float(e_cpu[m].max())) for k, m in groups.items()}


def row_gate(got, truth, yard, name, groups=None, bar=None, log=print, tag="ume ladder"):
    """Every row's relative error of `got` (the GPU's) <= 4 x the largest row-relative error of `yard` (the fp32 helper on the CPU)
    over the same rows; `groups`: {name: bool mask over the rows}, each judged against its own rows.  `bar`: a second, absolute
    bound on the GPU's row-relative error.  Prints what it saw under `tag` and returns the largest ratio."""
    worst = 0.0
    for k, (g_med, g_max, c_med, c_max) in row_stats(got, truth, yard, groups).items():
        ratio = g_max / c_max if c_max > 0 else (0.0 if g_max == 0 else float("inf"))
        log(f"[{tag}] {name} {k}: gpu row-rel median {g_med:.2e} max {g_max:.2e} | fp32 helper median {c_med:.2e} max {c_max:.2e} | "
            f"ratio {ratio:.3f}" + ("" if bar is None else f" | bar {bar:.2e}: {g_max / bar:.3f} of it"))
        assert np.isfinite(g_max), f"{name} {k}"
        assert g_max <= 4 * c_max, f"{name} {k}: a row at {g_max:.3e} > 4 x {c_max:.3e}"
        if bar is not None:
            assert g_max <= bar, f"{name} {k}: a row at {g_max:.3e} > {bar:.3e}"
        worst = max(worst, ratio)
    return worst


@functools.lru_cache(maxsize=None)
def sharp_bar():
    """4 x the fp32 helper's largest row-relative error at the c = 1e1 rung, per side: the kernel forms Q and R in fp64 from the
    f32 input, so nothing in it should grow with cond beyond the 1 / sigma_min the truth itself carries"""
    u1, u2, gD = cond_rung(C_RUNGS[0])
    _, truth, yard = truth_and_yard(u1, u2, gD)
    return tuple(4 * float(row_rel(y, t).max()) for y, t in zip(yard, truth))
