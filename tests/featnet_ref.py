"""fp64 restatement of ResUNetSmall2's forward pass (reference models.py:392-618, configuration :691-698) for the tests:
gather-form numpy -- coordinate keys sorted once, neighbours found by `searchsorted`, one matmul per kernel offset.

The MinkowskiEngine 0.5.4 semantics it restates (parity unpinned) are pinned here against torch's dense
`conv3d` / `conv_transpose3d` (tests/test_featnet_cpu.py): the restatement is the yardstick of the HIP network, torch's dense
convolutions are the yardstick of the restatement.  Rows of every level come out in sorted-key order; callers compare by
coordinate."""
import numpy as np

STRIDES = (1, 2, 2, 2, 3)
TSTRIDES = (1, 2, 4, 8, 24)
# offset index k = (dx+1) + 3(dy+1) + 9(dz+1), x fastest
OFFSETS = np.array([(k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1) for k in range(27)], dtype=np.int64)
_BIAS = 1 << 18
# the device's coordinate key and hash (csrc/sparse.h: fn_key, fn_hash, fn_ws), mirrored for the tests that aim at hash slots;
# tests/test_featnet_cpu.py pins these constants against the header
KEY_SHIFTS = (57, 38, 19, 0)        # batch 7 bits | x, y, z 19 bits each, biased by _BIAS
HASH_MUL = 0x9E3779B97F4A7C15
MIN_CAP = 1024
MAX_BATCH = 127
COORD_LIM = 1 << 17


def keys(c):
    """int [n,4] (batch, x, y, z) -> uint64 keys, ordered as (batch, x, y, z) lexicographically: the device's fn_key, bit for
    bit (batch in [0, 127], x / y / z in [-2^18, 2^18); asserted)."""
    c = np.asarray(c, dtype=np.int64).reshape(-1, 4)
    assert ((c[:, 0] >= 0) & (c[:, 0] < MAX_BATCH + 1)).all() and ((c[:, 1:] >= -_BIAS) & (c[:, 1:] < _BIAS)).all(), \
        "a coordinate outside the key's range"
    u = (c + np.array([0, _BIAS, _BIAS, _BIAS])).astype(np.uint64)
    return (u[:, 0] << np.uint64(KEY_SHIFTS[0])) | (u[:, 1] << np.uint64(KEY_SHIFTS[1])) | (u[:, 2] << np.uint64(KEY_SHIFTS[2])) | u[:, 3]


def table_cap(n):
    """slots per hash table of a pass over n points (fn_ws): the smallest power of two >= max(1024, 2 n)"""
    cap = MIN_CAP
    while cap < 2 * n:
        cap <<= 1
    return cap


def hash_slot(k, cap):
    """fn_hash: the home slot of uint64 keys in a table of `cap` slots (the product wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        return ((np.asarray(k, dtype=np.uint64) * np.uint64(HASH_MUL)) >> np.uint64(32)) & np.uint64(cap - 1)


class Index:
    """Row lookup by coordinate over one map."""

    def __init__(self, coords):
        self.k = keys(coords)
        self.order = np.argsort(self.k, kind="stable")
        self.sk = self.k[self.order]

    def find(self, q):
        """-> row index of every query coordinate, -1 where absent."""
        qk = keys(q)
        pos = np.searchsorted(self.sk, qk)
        pos_c = np.minimum(pos, len(self.sk) - 1)
        hit = self.sk[pos_c] == qk
        return np.where(hit, self.order[pos_c], -1)


def coarsen(c, t):
    c = np.array(c, dtype=np.int64, copy=True)
    c[:, 1:] = np.floor_divide(c[:, 1:], t) * t
    return c


def strided_map(c, ts_out):
    """unique(floor(c / ts_out) ts_out), batch kept; rows in sorted-key order."""
    cc = coarsen(c, ts_out)
    _, first = np.unique(keys(cc), return_index=True)
    return cc[first]


def levels(coords):
    """the five maps of a cloud: level 0 = the input rows (in input order), level l = strided_map(level l - 1, TSTRIDES[l])"""
    lv = [np.asarray(coords, dtype=np.int64)]
    for l in range(1, 5):
        lv.append(strided_map(lv[-1], TSTRIDES[l]))
    return lv


def cells(coords):
    """number of locality cells of the level-0 row order: distinct (batch, floor(c / 8)) (include/umereg_featnet.h, status[6])"""
    return len(np.unique(keys(coarsen(coords, 8))))


# the 13 neighbour tables in the header's order (UMEREG_FN_MASKS): (query level, read level, sign of the offset); the offsets
# are in units of the finer level's tensor stride
TABLES = [(l, l, 1) for l in range(5)] + [(l + 1, l, 1) for l in range(4)] + [(l, l + 1, -1) for l in range(4)]


def neighbour_masks(levels):
    """The offset masks of the 13 neighbour tables over the five maps `levels` (each in its own row order): table l (self)
    queries level l and reads level l at +off_k ts_l; 5 + l (strided) queries level l + 1 and reads level l at +off_k ts_l;
    9 + l (transposed) queries level l and reads level l + 1 at -off_k ts_l.  -> 13 uint32 arrays, one word per query row,
    bit k set exactly when a row exists at that offset (the rule of `conv`)."""
    lv = [np.asarray(c, dtype=np.int64) for c in levels]
    idx = [Index(c) for c in lv]
    out = []
    for ql, tl, sign in TABLES:
        ts = TSTRIDES[min(ql, tl)]
        mask = np.zeros(len(lv[ql]), dtype=np.uint32)
        for k in range(27):
            q = lv[ql].copy()
            q[:, 1:] += sign * OFFSETS[k] * ts
            mask |= (idx[tl].find(q) >= 0).astype(np.uint32) << np.uint32(k)
        out.append(mask)
    return out


def conv(feat, in_coords, out_coords, W, ts, transposed=False, index=None):
    """out[o] = sum_k feat[o + off_k ts] @ W[k] (transposed: feat[o - off_k ts]) over the neighbours that exist; fp64.
    W [27, C_in, C_out] or [C_in, C_out] (1x1: out[o] = feat[o] @ W, same coordinates)."""
    feat = np.asarray(feat, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 2:
        return feat @ W
    index = index or Index(in_coords)
    out = np.zeros((len(out_coords), W.shape[2]))
    sign = -1 if transposed else 1
    for k in range(27):
        q = np.array(out_coords, dtype=np.int64, copy=True)
        q[:, 1:] += sign * OFFSETS[k] * ts
        j = index.find(q)
        m = j >= 0
        if m.any():
            out[m] += feat[j[m]] @ W[k]
    return out


def batch_norm(x, sd, prefix, eps=1e-5):
    g, b = sd[prefix + ".bn.weight"], sd[prefix + ".bn.bias"]
    mu, var = sd[prefix + ".bn.running_mean"], sd[prefix + ".bn.running_var"]
    return (x - mu) / np.sqrt(var + eps) * g + b


def network(coords, feat, sd):
    """coords int [N,4], feat [N,1], sd {name: fp64 numpy} -> (out [N,32] in input order, intermediates): per level l the
    coordinates (`coords[l]`), the concatenation [decoder block | encoder block] (`cat[l]`, l < 4), block5's output (`s4`),
    mlp1's output (`hidden`, input order)."""
    relu = lambda x: np.maximum(x, 0.0)     # noqa: E731
    lv = levels(coords)
    idx = [Index(c) for c in lv]

    def block(x, l, name):
        return relu(batch_norm(conv(x, lv[l], lv[l], sd[name + ".conv1.kernel"], TSTRIDES[l], index=idx[l]), sd, name + ".norm1") + x)

    skips = []
    x = np.asarray(feat, dtype=np.float64)
    for l in range(5):
        i = l + 1
        src = lv[0] if l == 0 else lv[l - 1]
        ts_in = TSTRIDES[0] if l == 0 else TSTRIDES[l - 1]
        h = batch_norm(conv(x, src, lv[l], sd[f"conv{i}.kernel"], ts_in, index=idx[0] if l == 0 else idx[l - 1]), sd, f"norm{i}")
        x = relu(block(h, l, f"block{i}"))
        skips.append(x)
    inter = dict(coords=lv, s4=x)
    cats = [None] * 4
    for l in range(3, -1, -1):
        i = l + 1
        h = batch_norm(conv(x, lv[l + 1], lv[l], sd[f"conv{i}_tr.kernel"], TSTRIDES[l], transposed=True, index=idx[l + 1]), sd,
                       f"norm{i}_tr")
        tr = relu(block(h, l, f"block{i}_tr"))
        x = cats[l] = np.concatenate([tr, skips[l]], axis=1)
    inter["cat"] = cats
    h = relu(conv(x, None, None, sd["mlp1.kernel"], 1))
    inter["hidden"] = h
    out = conv(h, None, None, sd["final.kernel"], 1) + sd["final.bias"].reshape(1, -1)
    return out / np.linalg.norm(out, axis=1, keepdims=True), inter


def seeded_state_dict(seed, model_state):
    """Seeded weights on the reference's names and shapes (`model_state`: name -> shape): He-scaled kernels, batch norm with
    gamma ~ U(.5, 1.5), beta ~ N(0, .1), mean ~ N(0, .1), var ~ U(.5, 2), a final bias ~ N(0, .1).  -> {name: fp64 numpy}."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in model_state.items():
        shape = tuple(shape)
        if name.endswith(".kernel"):
            fan_in = shape[0] * shape[1] if len(shape) == 3 else shape[0]
            sd[name] = rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)
        elif name.endswith("bn.weight"):
            sd[name] = rng.uniform(0.5, 1.5, shape)
        elif name.endswith("bn.bias") or name.endswith("running_mean") or name == "final.bias":
            sd[name] = rng.normal(0.0, 0.1, shape)
        elif name.endswith("running_var"):
            sd[name] = rng.uniform(0.5, 2.0, shape)
        elif name.endswith("num_batches_tracked"):
            sd[name] = np.zeros(shape, dtype=np.int64)
        else:
            raise KeyError(name)
    return sd
