"""The clouds, the plan mirror and the fp64 truth of the weight-gradient edge tests (tests/test_wgrad_edges_cpu.py pins every
edge a cloud is here for, tests/test_wgrad_edges_gpu.py runs csrc/sparse_wgrad.hip over them).  No GPU.

Every cloud is int64 [n, 4] (batch index 0) in a GIVEN input order: the library numbers 8^3 cells by first occurrence and keeps
the input order inside a cell (csrc/sparse_map.hip), so the input order decides which rows share a 64-row ballot chunk and a
segment of the weight gradient.  `level0_order` restates that rule."""
import numpy as np
import torch

import featnet_grad_ref as gref
import featnet_ref as ref

MAX_SEGMENTS, MIN_RPS, CHUNK, QUEUE = 64, 1024, 64, 128
GROUP = {"f32": 8, "f16": 16}           # pairs consumed at a time (wg_mfma_kernel / wg_f16_kernel)


def ceil_div(a, b):
    return -(-a // b)


def plan(n, cin, cout):
    """wg_plan of csrc/sparse_wgrad.hip -> (rows per segment, segments over [0, n))"""
    block = 27 * cin * cout
    smax = min(max((64 << 20) // (4 * block), 1), MAX_SEGMENTS)
    rps = max(MIN_RPS, ceil_div(ceil_div(n, smax), CHUNK) * CHUNK)
    return rps, ceil_div(n, rps)


def level0_order(coords):
    """input row of every level-0 row: stable by 8^3 cell, the cells numbered by first occurrence"""
    _, first, inv = np.unique(ref.keys(ref.coarsen(coords, 8)), return_index=True, return_inverse=True)
    return np.argsort(first[inv.reshape(-1)], kind="stable")


# ---- the clouds ---------------------------------------------------------------------------------------------------------------

def line(m):
    return np.stack([np.zeros(m, np.int64), np.arange(m) - 5, np.full(m, 3), np.full(m, -2)], 1)


def block_of(n):
    """n level-0 rows: a dense 16 x 8 x 8 block, and beyond 1024 isolated points far away"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    far = np.stack([1000 + 50 * np.arange(n - 1024), np.zeros(n - 1024, np.int64), np.zeros(n - 1024, np.int64)], 1)
    c = np.concatenate([g, far]).astype(np.int64)
    c = c[np.random.default_rng(n).permutation(len(c))]
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)


def pairs_of_two(m):
    """x in {3 j, 3 j + 1}, j < m: the +x (-x) neighbour exists on every other row only -- a ballot with holes"""
    x = (3 * np.arange(m)[:, None] + np.arange(2)).reshape(-1)
    return np.stack([np.zeros(2 * m, np.int64), x, np.full(2 * m, 3), np.full(2 * m, -2)], 1)


def isolated(count):
    """`count` points 50 apart along x from 1000 on: every one alone in its 8^3 cell and without a neighbour"""
    z = np.zeros(count, np.int64)
    return np.stack([z, 1000 + 50 * np.arange(count), z, z], 1)


def isolated_then_line():
    return np.concatenate([isolated(1024), line(40)])


def line_then_isolated():
    return np.concatenate([line(40), isolated(1024)])


def dense_and_far(nx, ny, nz, seed):
    """a dense nx x ny x nz block and one point far away, in a seeded random order"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    c = np.concatenate([g, [[5000, 0, 0]]]).astype(np.int64)
    c = c[np.random.default_rng(seed).permutation(len(c))]
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)


def deep():
    return dense_and_far(16, 16, 8, 2049)


def long_segments():
    return dense_and_far(24, 24, 16, 9217)


LINES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 129, 200)
TWOS = (40, 100)
CLOUDS = {**{f"line{m}": (lambda m=m: line(m)) for m in LINES}, **{f"twos{m}": (lambda m=m: pairs_of_two(m)) for m in TWOS},
          "isolated_then_line": isolated_then_line, "line_then_isolated": line_then_isolated,
          "rows1024": lambda: block_of(1024), "rows1025": lambda: block_of(1025), "deep": deep, "long_segments": long_segments}
GROUP_CLOUDS = [f"line{m}" for m in LINES] + [f"twos{m}" for m in TWOS]
SEGMENT_CLOUDS = ["rows1024", "rows1025", "isolated_then_line", "line_then_isolated"]
# (cloud, table, C_in, C_out) of every exact case of the GPU tests: the largest sum of |x| |dy| is asserted over all of them
GROUP_CHANNELS = [(32, 32), (32, 64), (64, 32), (64, 64)]
SEGMENT_CHANNELS = [(32, 64), (64, 32)]
DEEP_CHANNELS = [(32, 64), (64, 64)]
EXACT_CASES = ([(c, t) for c in GROUP_CLOUDS for t in (0, 5, 9)] + [(c, 0) for c in SEGMENT_CLOUDS] + [("long_segments", 0)]
               + [("deep", 5), ("deep", 9)])

_cache = {}


def cloud(name):
    if ("cloud", name) not in _cache:
        c = CLOUDS[name]()
        c.setflags(write=False)
        _cache[("cloud", name)] = c
    return _cache[("cloud", name)]


def tables_of(name):
    """featnet_grad_ref.Tables of a cloud with the pair lists of the tables the tests use (0, 5 and 9)"""
    if ("tables", name) not in _cache:
        _cache[("tables", name)] = gref.Tables(cloud(name), tables=[0, 5, 9])
    return _cache[("tables", name)]


def pair_counts(name, t):
    return [len(o) for o, _ in tables_of(name).pairs[t]]


# ---- operands and the truth -----------------------------------------------------------------------------------------------------

def integers(shape, seed):
    """integer-valued f32 in [-3, 3]"""
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).to(torch.float32)


def normals(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def truth(tables, t, x, dy):
    """dW [27, C_in, C_out] in fp64: x[i]^T dy[o] per offset over the table's pairs (rows in the helper's order)"""
    x, dy = x.double(), dy.double()
    dw = torch.zeros(27, x.shape[1], dy.shape[1], dtype=torch.float64)
    for k, (o, i) in enumerate(tables.pairs[t]):
        if len(o):
            dw[k] = x[i].t() @ dy[o]
    return dw


def repacked(W, transpose, mirror, slice):
    """umereg_sparse_conv_repack_f32 as include/umereg_sparse_conv.h states it, W a numpy [27, C_in, C_out] -> flat"""
    M = W.transpose(0, 2, 1) if transpose else W
    if mirror:
        M = M[::-1]
    K, R, C = M.shape
    return np.ascontiguousarray(M.reshape(K, R // slice, slice, C).transpose(1, 0, 2, 3)).reshape(-1)
