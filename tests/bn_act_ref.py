"""fp64 numpy restatement of include/umereg_bn_act.h, all from f32 inputs: y = act(batch_norm(x) [+ residual]) forward, the
running-statistics update, the backward, and the gradient-scale contract; and a Python mirror of csrc/bn_act_plan.h (checked against
the header itself by tests/test_bn_act_cpu.py through tests/bn_act_plan_host.cpp) that the GPU tests choose their shapes with."""
import math

import numpy as np

# csrc/bn_act_plan.h
THREADS, MAX_C, MIN_PASSES, MAX_SLABS, GS_CHUNK, GS_WIDTH = 256, 256, 4, 256, 8192, 256
CHANNELS = (32, 64, 128, 256)       # the network's norms
E_MAX = 126


def plan(n, C):
    """-> (unit, slab length S, slabs, finishing width W) of bn_plan(n, C)"""
    unit = THREADS // (C // 4)
    cover = unit * MAX_SLABS
    passes = max(MIN_PASSES, (n + cover - 1) // cover)
    slab = passes * unit
    return unit, slab, (n + slab - 1) // slab, THREADS // C


def scratch_bytes(n, C):
    return plan(n, C)[2] * 2 * C * 8


def gs_partials(count):
    return (count + GS_CHUNK - 1) // GS_CHUNK


def edge_rows(C):
    """the row counts the GPU tests run: with S the slab length and W the finishing width, {2, 3, S - 1, S, S + 1, 2 S + 1, W S + 1}"""
    _, S, _, W = plan(2, C)
    return sorted({2, 3, S - 1, S, S + 1, 2 * S + 1, W * S + 1})


# ---- the operator -----------------------------------------------------------------------------------------------------------------

def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def forward(x, gamma, beta, residual=None, relu=False, train=True, eps=1e-5, running_mean=None, running_var=None):
    """-> dict(y, mean, var (biased; eval: the running one), invstd), everything fp64"""
    x, gamma, beta, residual = _f64(x), _f64(gamma), _f64(beta), _f64(residual)
    if train:
        mean = x.mean(axis=0)
        var = ((x - mean) ** 2).mean(axis=0)
    else:
        mean, var = _f64(running_mean), _f64(running_var)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    y = x * scale + (beta - mean * scale)
    if residual is not None:
        y = y + residual
    if relu:
        y = np.maximum(y, 0.0)
    return dict(y=y, mean=mean, var=var, invstd=invstd, scale=scale)


def running_update(running_mean, running_var, num_batches_tracked, mean, var, n, momentum):
    """-> the three buffers after one train-mode call (var: the biased batch variance)"""
    return ((1 - momentum) * _f64(running_mean) + momentum * mean,
            (1 - momentum) * _f64(running_var) + momentum * var * (n / (n - 1)), int(num_batches_tracked) + 1)


def backward(dy, x, y, gamma, mean, invstd, train=True, relu=False):
    """-> dict(dx, dres, dgamma, dbeta) in fp64; y: the forward's output (read only with relu: the mask is y > 0); mean / invstd: the
    statistics the forward used (`forward(...)['mean']`, `['invstd']`)"""
    dy, x, gamma = _f64(dy), _f64(x), _f64(gamma)
    g = dy * (np.asarray(y) > 0) if relu else dy
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(axis=0), (g * xhat).sum(axis=0)
    n = x.shape[0]
    dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n) if train else gamma * invstd * g
    return dict(dx=dx, dres=g, dgamma=dgamma, dbeta=dbeta)


# ---- the gradient scale -------------------------------------------------------------------------------------------------------------

def pow2(e):
    return np.array((int(e) + 127) << 23, dtype=np.uint32).view(np.float32)[()]


def grad_scale(dy):
    """-> (e int32, 2^e f32, 2^-e f32): e = 14 - floor(log2(max |dy|)) held to +-126; 0 for a zero or non-finite maximum (a NaN
    anywhere counts as non-finite)"""
    a = np.abs(np.asarray(dy, dtype=np.float32)).ravel()
    e = 0
    if a.size and np.isfinite(a).all() and a.max() > 0:
        e = 14 - (math.frexp(float(a.max()))[1] - 1)          # frexp: m = f 2^ex with f in [0.5, 1)
        e = max(-E_MAX, min(E_MAX, e))
    return np.int32(e), pow2(e), pow2(-e)


SCALE_VALUES = [0.0, float("nan"), float("inf"), 2.0 ** -120, 2.0 ** -113, 2.0 ** 14, 2.0 ** 15 - 1, 2.0 ** 15,
                float(np.finfo(np.float32).max)]


def scale_background(v):
    """what the rest of a tensor holds when v is its only extreme value: a quarter of a finite positive v (exact), 1 beside
    infinity or a NaN, 0 beside 0"""
    return v / 4 if np.isfinite(v) and v > 0 else 0.0 if v == 0 else 1.0


# ---- exact-data clouds --------------------------------------------------------------------------------------------------------------

def exact_cloud(n, C, seed):
    """x f32 [n, C] (n even): half of each channel's rows are m + 2^k and half m - 2^k at permuted positions, m an integer in [-4, 4],
    k in [0, 3]: the mean is exactly m and the biased variance exactly 4^k.  -> (x, m, k, sign [n, C] of x - m)"""
    assert n % 2 == 0
    rng = np.random.default_rng(seed)
    m, k = rng.integers(-4, 5, C), rng.integers(0, 4, C)
    sign = np.empty((n, C))
    for c in range(C):
        sign[:, c] = rng.permutation(np.repeat([1.0, -1.0], n // 2))
    return (m + sign * 2.0 ** k).astype(np.float32), m, k, sign


def small_ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(np.float32)


def balanced_dy(sign, seed):
    """dy f32 of small integers with sum dy = 0 and sum dy xhat = 0 per channel (xhat = sign): inside each sign group the rows are
    paired as +v, -v (a group of odd size leaves one row 0)"""
    rng = np.random.default_rng(seed)
    dy = np.zeros(sign.shape, np.float32)
    for c in range(sign.shape[1]):
        for s in (1.0, -1.0):
            rows = rng.permutation(np.nonzero(sign[:, c] == s)[0])
            h = len(rows) // 2
            v = rng.integers(-3, 4, h)
            dy[rows[:h], c], dy[rows[h:2 * h], c] = v, -v
    return dy
