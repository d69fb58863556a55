"""CPU: the f16-operand mode of the feature network (include/umereg_featnet_f16.h) -- its fp64 restatement
(tests/featnet_f16_ref.py) against tests/featnet_ref.py, the host side of the new header, the `precision` keyword, and the
derivation of the whole-network gates that tests/test_featnet_f16_gpu.py applies.

The gates.  Write E16 = (network with operands rounded to f16) - (fp64 network): the error the CONTRACT has, computed without
the code under test.  A correct kernel differs from the rounded network only by its f32 accumulation, so its error against fp64
is E16 plus an f32-sized perturbation; a kernel that rounds differently (truncation is the mildest wrong rounding) has another
error altogether.  The derivation below measures both on the CPU: the perturbation moves rms by at most 5 % and max by at most
25 %, truncation moves rms by at least 1.5 x -- so the GPU gates, rms <= 1.25 rms(E16) and max <= 1.5 max(E16), sit between."""
import json
import os
import re

import numpy as np
import pytest

import abi_headers
import featnet_f16_ref as f16ref
import featnet_ref as ref
import test_featnet_gpu as fg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = json.load(open(os.path.join(REPO, "tests", "golden", "featnet_state_dict.json")))


def test_restatement_with_identity_hook_is_the_fp64_network():
    rng = np.random.default_rng(3)
    c = np.unique(rng.integers(-40, 40, (800, 3)), axis=0)
    c = np.concatenate([(np.arange(len(c)) % 2)[:, None], c[rng.permutation(len(c))]], axis=1)
    sd = ref.seeded_state_dict(0, SHAPES)
    want, wi = ref.network(c, np.ones((len(c), 1)), sd)
    got, gi = f16ref.network(c, np.ones((len(c), 1)), sd, q=f16ref.identity)
    a, b = f16ref.flat(got, gi), f16ref.flat(want, wi)
    for k in f16ref.NAMES:
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), k
    # and the hook reaches layers 1..18 only: 18 inputs, 18 kernels, never conv1's [27, 1, 32] or final's [64, 32]
    seen = []
    f16ref.network(c, np.ones((len(c), 1)), sd, q=lambda a, what: (seen.append((what, a.shape)), a)[1])
    kernels = [s for w, s in seen if w == "w"]
    assert len(kernels) == 18 and sum(1 for w, _ in seen if w == "in") == 18
    assert (27, 1, 32) not in kernels and (64, 32) not in kernels and kernels[-1] == (96, 64)


def test_roundings():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 65504.0, 65519.0, 65520.0, 1e6, 2.0 ** -25,
                  3 * 2.0 ** -25])
    assert f16ref.r16(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 65504.0, 65504.0, np.inf, np.inf, 0.0, 2.0 ** -23]
    assert f16ref.t16(x[:6]).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 65504.0, 65504.0]


# ---- the host side of include/umereg_featnet_f16.h ----------------------------------------------------------------------------

def test_f16_table_mirrors_its_header():
    """(keys, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import models, sparse_conv
    text = abi_headers.text("umereg_featnet_f16.h")
    assert sorted(models.FEATNET_F16_SIGNATURES) == ["umereg_featnet_forward_f16", "umereg_sparse_conv_f16"]
    # the arguments of the f32 entries, one to one
    assert models.FEATNET_F16_SIGNATURES["umereg_featnet_forward_f16"] == models.FEATNET_SIGNATURES["umereg_featnet_forward_f32"]
    assert models.FEATNET_F16_SIGNATURES["umereg_sparse_conv_f16"] == sparse_conv.SPARSE_CONV_SIGNATURES["umereg_sparse_conv_f32"]
    assert int(re.search(r"#define UMEREG_FN_ERR_F16_RANGE (\d+)", text).group(1)) == models.ERR_F16_RANGE == 4
    for h in ("umereg.h", "umereg_featnet.h", "umereg_sparse_conv.h"):
        assert "f16.h" not in open(os.path.join(REPO, "include", h)).read()


def test_f16_entry_points_check_arguments_and_need_a_device():
    from umeregrobust_amd import models
    lib = models.load_native()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    ws_bytes = lib.umereg_featnet_workspace_bytes(4, 1)
    fwd = lib.umereg_featnet_forward_f16
    # argument errors come before the device probe
    assert fwd(None, p, 4, 1, p, p, p, p, ws_bytes, None) == -1
    assert fwd(p, None, 4, 1, p, p, p, p, ws_bytes, None) == -1 and b"null" in lib.umereg_last_error()
    assert fwd(p, p, 0, 1, p, p, p, p, ws_bytes, None) == -1
    assert fwd(p, p, 4, 0, p, p, p, p, ws_bytes, None) == -1
    assert fwd(p, p, 4, 128, p, p, p, p, ws_bytes, None) == -1
    assert fwd(p, p, 4, 1, p + 4, p, p, p, ws_bytes, None) == -1
    conv = lambda **kw: lib.umereg_sparse_conv_f16(*[kw.get(k, d) for k, d in (          # noqa: E731
        ("ws", p), ("ws_bytes", ws_bytes), ("status", p), ("n", 4), ("table", 0), ("x", p), ("ld_in", 32), ("W", p), ("cin", 32), ("cout", 32),
        ("scale", p), ("shift", p), ("out", p), ("ld_out", 32), ("accumulate", 0), ("stream", None))])
    for k in ("ws", "status", "x", "W", "scale", "shift", "out"):
        assert conv(**{k: None}) == -1, k
        assert b"null" in lib.umereg_last_error()
    for kw in (dict(n=0), dict(table=13), dict(table=-2), dict(cin=48), dict(cout=16), dict(cout=288), dict(ld_in=16), dict(ld_in=34),
               dict(ld_out=8), dict(x=p + 4)):
        assert conv(**kw) == -1, kw
    if lib.umereg_device_count(None, 0) == 0:
        assert fwd(p, p, 4, 1, p, p, p, p, ws_bytes, None) == -2                          # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        assert conv() == -2 and conv(table=-1, cin=96, ld_in=96, cout=64, ld_out=64) == -2
        assert b"no CPU fallback" in lib.umereg_last_error()


def test_precision_keyword(capsys):
    import torch
    from umeregrobust_amd import evaluate, models, sparse_conv
    from umeregrobust_amd.sparse import SparseTensor
    assert models.ResUNetSmall2().precision == "f32" and models.ResUNetSmall2(precision="f16").precision == "f16"
    with pytest.raises(ValueError, match="bf16"):
        models.ResUNetSmall2(precision="bf16")
    with pytest.raises(ValueError, match="bf16"):
        models.forward_raw(None, None, 1, None, None, None, None, precision="bf16")
    with pytest.raises(ValueError, match="bf16"):
        sparse_conv.conv_raw(torch.zeros(2, 32), torch.zeros(27, 32, 32), None, 0, precision="bf16")
    # an f16 module refuses the layer-wise path by name, trainable or not, before anything else
    st = SparseTensor(torch.ones(2, 1), coordinates=torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32))
    for trainable in (False, True):
        m = models.ResUNetSmall2(precision="f16", trainable=trainable)
        with pytest.raises(RuntimeError, match="precision='f16'.*inference only"):
            m.train()(st)
        with pytest.raises(RuntimeError, match="precision='f16'.*inference only"):
            m.eval()(st)                                                                  # needs gradients
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            m.eval()(st)
    # the command line and cached_pairs carry the choice; the default is f32
    import inspect
    assert inspect.signature(evaluate.cached_pairs).parameters["feature_precision"].default == "f32"
    assert inspect.signature(models.forward_raw).parameters["precision"].default == "f32"
    assert inspect.signature(sparse_conv.conv_raw).parameters["precision"].default == "f32"
    with pytest.raises(SystemExit):
        evaluate.main(["--feature-precision", "bf16"])
    err = capsys.readouterr().err
    assert "--feature-precision" in err and "'f32', 'f16'" in err


# ---- where the network gates come from ------------------------------------------------------------------------------------------

def test_network_gates_sit_between_an_f32_sized_perturbation_and_truncation():
    """On the 6 000-point KITTI-shaped cloud with the seeded weights (42) the GPU tests use.  Probes on 6 000- and 20 000-point
    clouds gave 0.994-1.001 (rms) and <= 1.08 (max) for the perturbation, 1.60 (output) and 3.7-4.1 (s4) for truncation, with E16
    itself 4-5e-5 rms and 2.5-3.3e-4 max on the unit output."""
    coords = fg.voxel_cloud(0, "KT")[:6000]
    feat = np.ones((len(coords), 1))
    sd = fg.f32_state(fg.seeded(42))
    want = f16ref.flat(*ref.network(coords, feat, sd))
    e16 = {k: v - want[k] for k, v in f16ref.flat(*f16ref.network(coords, feat, sd)).items()}
    print("[f16 gates] E16 " + " ".join(f"{k}: rms {f16ref.rms(e):.2e} max {np.abs(e).max():.2e}" for k, e in e16.items()))
    assert 1e-5 < f16ref.rms(e16["out"]) < 2e-4 and np.abs(e16["out"]).max() < 2e-3

    # (a) every rounded activation perturbed by relative N(0, 1e-6): more than the f32 kernel's observed error (2e-6 of the
    # largest magnitude of a buffer, tests/test_featnet_gpu.py) leaves on a typical element
    rng = np.random.default_rng(1)

    def perturbed(a, what):
        a = f16ref.r16(a)
        return a * (1.0 + 1e-6 * rng.standard_normal(a.shape)) if what == "in" else a

    ep = {k: v - want[k] for k, v in f16ref.flat(*f16ref.network(coords, feat, sd, q=perturbed)).items()}
    for k in f16ref.NAMES:
        r_rms, r_max = f16ref.rms(ep[k]) / f16ref.rms(e16[k]), np.abs(ep[k]).max() / np.abs(e16[k]).max()
        print(f"[f16 gates] perturbed {k}: rms ratio {r_rms:.4f} max ratio {r_max:.4f}")
        assert 0.95 <= r_rms <= 1.05 and r_max <= 1.25, (k, r_rms, r_max)

    # (b) truncation in place of round-to-nearest
    et = {k: v - want[k] for k, v in f16ref.flat(*f16ref.network(coords, feat, sd, q=f16ref.t16_op)).items()}
    ratios = {k: f16ref.rms(et[k]) / f16ref.rms(e16[k]) for k in f16ref.NAMES}
    print("[f16 gates] truncation rms ratios " + " ".join(f"{k}={v:.2f}" for k, v in ratios.items()))
    assert ratios["out"] >= 1.5 and ratios["s4"] >= 2.5, ratios
