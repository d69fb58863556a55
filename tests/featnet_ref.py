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


def keys(c):
    """int [n,4] (batch, x, y, z) -> int64 keys, ordered as (batch, x, y, z) lexicographically."""
    c = np.asarray(c, dtype=np.int64)
    w = 2 * _BIAS
    return ((c[:, 0] * w + c[:, 1] + _BIAS) * w + c[:, 2] + _BIAS) * w + c[:, 3] + _BIAS


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
    lv = [np.asarray(coords, dtype=np.int64)]
    for l in range(1, 5):
        lv.append(strided_map(lv[-1], TSTRIDES[l]))
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
