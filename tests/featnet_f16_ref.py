"""The f16-operand contract of include/umereg_featnet_f16.h restated in fp64 for the tests: the network of
tests/featnet_ref.py (built on its `levels`, `Index`, `conv` and `batch_norm`) with an operand hook `q`.

`q(a, what)` is applied to the input (`what` = "in") and to the kernel (`what` = "w") of layers 1..18 of the packed parameter
block -- the seventeen 27-offset convolutions other than conv1, and mlp1 -- and to nothing else: conv1, `final`, batch norm,
residuals, ReLU and every stored activation stay as they are.  With `q = r16_op` it is the contract (operands rounded to f16,
to nearest even; exact products; the sums here are fp64, the device's f32); with `q = identity` it is `ref.network`."""
import numpy as np

import featnet_ref as ref


def r16(a):
    """f32 value -> f16, round to nearest even -> fp64 (the rounding the kernel applies where it stages a tile)"""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float32).astype(np.float16).astype(np.float64)


def t16(a):
    """f32 value -> f16 by truncation (round toward zero) -> fp64: the wrong rounding, for the tests that must tell it apart"""
    a32 = np.asarray(a).astype(np.float32)
    with np.errstate(over="ignore"):
        h = a32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a32)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def identity(a, what):
    return a


def r16_op(a, what):
    return r16(a)


def t16_op(a, what):
    return t16(a)


def network(coords, feat, sd, q=r16_op):
    """coords int [N,4], feat [N,1], sd {name: fp64 numpy}, q: the operand hook -> (out [N,32] in input order, intermediates)
    as `ref.network` returns them."""
    relu = lambda x: np.maximum(x, 0.0)     # noqa: E731
    lv = ref.levels(coords)
    idx = [ref.Index(c) for c in lv]
    T = ref.TSTRIDES

    def qconv(x, src, dst, W, ts, transposed=False, index=None):
        return ref.conv(q(x, "in"), src, dst, q(W, "w"), ts, transposed=transposed, index=index)

    def block(x, l, name):
        return relu(ref.batch_norm(qconv(x, lv[l], lv[l], sd[name + ".conv1.kernel"], T[l], index=idx[l]), sd, name + ".norm1") + x)

    skips = []
    x = np.asarray(feat, dtype=np.float64)
    for l in range(5):
        i = l + 1
        if l == 0:      # conv1: f32 kernel, no hook
            h = ref.conv(x, lv[0], lv[0], sd["conv1.kernel"], T[0], index=idx[0])
        else:
            h = qconv(x, lv[l - 1], lv[l], sd[f"conv{i}.kernel"], T[l - 1], index=idx[l - 1])
        x = relu(block(ref.batch_norm(h, sd, f"norm{i}"), l, f"block{i}"))
        skips.append(x)
    inter = dict(coords=lv, s4=x)
    cats = [None] * 4
    for l in range(3, -1, -1):
        i = l + 1
        h = ref.batch_norm(qconv(x, lv[l + 1], lv[l], sd[f"conv{i}_tr.kernel"], T[l], transposed=True, index=idx[l + 1]), sd,
                           f"norm{i}_tr")
        tr = relu(block(h, l, f"block{i}_tr"))
        x = cats[l] = np.concatenate([tr, skips[l]], axis=1)
    inter["cat"] = cats
    h = relu(qconv(x, None, None, sd["mlp1.kernel"], 1))
    inter["hidden"] = h
    out = ref.conv(h, None, None, sd["final.kernel"], 1) + sd["final.bias"].reshape(1, -1)      # final: f32 kernel, no hook
    return out / np.linalg.norm(out, axis=1, keepdims=True), inter


NAMES = ("out", "cat0", "cat1", "cat2", "cat3", "s4", "hidden")


def flat(out, inter):
    """{name: array} over the output and the intermediates the gates are stated for"""
    d = {"out": out, "s4": inter["s4"], "hidden": inter["hidden"]}
    d.update({f"cat{l}": inter["cat"][l] for l in range(4)})
    return d


def rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0
