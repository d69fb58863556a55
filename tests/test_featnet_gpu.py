"""GPU: the HIP ResUNetSmall2 (umeregrobust_amd.models, include/umereg_featnet.h) against the fp64 restatement of
tests/featnet_ref.py with seeded weights -- the normalised output and the intermediates of every level (debug hook) --
plus determinism, the error contract, guard bands around every entry point of the header, and the evaluation loop run
from a pair cache without features (`--checkpoint`)."""
import json
import os

import numpy as np
import pytest
import torch

import featnet_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = json.load(open(os.path.join(REPO, "tests", "golden", "featnet_state_dict.json")))
TOL = 2e-6


def seeded(seed=42):
    return ref.seeded_state_dict(seed, SHAPES)


def torch_state(sd):
    return {k: torch.from_numpy(np.asarray(v)).to(torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
            for k, v in sd.items()}


def f32_state(sd):
    """the weights the GPU sees, back in fp64: the restatement runs on exactly those values"""
    return {k: np.asarray(v, dtype=np.float32).astype(np.float64) if v.dtype != np.int64 else v for k, v in sd.items()}


_models = {}


def model(dev, seed=42):
    from umeregrobust_amd.models import ResUNetSmall2
    if (dev, seed) not in _models:
        m = ResUNetSmall2(in_channels=1, out_channels=32)
        m.load_state_dict(torch_state(seeded(seed)))
        _models[(dev, seed)] = m.eval().to(dev)
    return _models[(dev, seed)]


def run(m, coords, dev, debug=False):
    from umeregrobust_amd.sparse import SparseTensor
    C = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(dev)
    with torch.no_grad():
        return m(SparseTensor(torch.ones(len(C), 1, device=dev), coordinates=C), debug=debug)


def voxel_cloud(seed, config, batch=0):
    """a synthetic KITTI / nuScenes-shaped cloud as the collate hands it over: voxel coordinates round(p / 0.3), in random order"""
    from umeregrobust_amd.synth import synth_pair_cfg
    p = synth_pair_cfg(seed, config, "test")
    c = np.round(p.src_pts / 0.3).astype(np.int64)
    c = c[np.sort(np.unique(c, axis=0, return_index=True)[1])]
    c = c[np.random.default_rng(seed).permutation(len(c))]
    return np.concatenate([np.full((len(c), 1), batch), c], axis=1)


def edge_cloud(kind):
    rng = np.random.default_rng(5)
    if kind == "one_point":
        return np.array([[0, -7, 3, -1]])
    if kind == "one_cell":          # every point in the stride-24 cell [-24, 0)^3
        c = np.unique(rng.integers(-24, 0, (600, 3)), axis=0)
        return np.concatenate([np.zeros((len(c), 1), np.int64), c[rng.permutation(len(c))]], axis=1)
    if kind == "isolated":          # no point has a neighbour at any level
        g = np.stack(np.meshgrid(np.arange(-3, 3), np.arange(-3, 3), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3) * 100 + 7
        return np.concatenate([np.zeros((len(g), 1), np.int64), g], axis=1)
    raise KeyError(kind)


def batch_of_two():
    a, b = voxel_cloud(3, "NS"), voxel_cloud(4, "KT", batch=1)
    return np.concatenate([a[:20000], b[:31000]])


CASES = {
    "KT": lambda: voxel_cloud(0, "KT"),
    "NS": lambda: voxel_cloud(1, "NS"),
    "batch2": batch_of_two,
    "one_point": lambda: edge_cloud("one_point"),
    "one_cell": lambda: edge_cloud("one_cell"),
    "isolated": lambda: edge_cloud("isolated"),
}


def compare(coords, out, inter, want, want_inter):
    """-> {name: max |gpu - fp64|} over the output and every intermediate (rows matched by coordinate)"""
    err = {"out": float(np.abs(out - want).max())}
    rows = []
    for l in range(5):
        gc = inter["coords"][l].cpu().numpy().astype(np.int64)
        assert len(gc) == len(want_inter["coords"][l]), f"level {l}: {len(gc)} rows, restatement {len(want_inter['coords'][l])}"
        idx = ref.Index(want_inter["coords"][l]).find(gc)
        assert (idx >= 0).all() and len(np.unique(idx)) == len(idx), f"level {l}: coordinates differ"
        rows.append(idx)
    for l in range(4):
        err[f"cat{l}"] = float(np.abs(inter["cat"][l].cpu().numpy() - want_inter["cat"][l][rows[l]]).max())
    err["s4"] = float(np.abs(inter["s4"].cpu().numpy() - want_inter["s4"][rows[4]]).max())
    perm = inter["perm"].cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(len(coords)))
    assert np.array_equal(inter["coords"][0].cpu().numpy(), coords[perm].astype(np.int32))
    err["hidden"] = float(np.abs(inter["hidden"].cpu().numpy() - want_inter["hidden"][perm]).max())
    return err


@pytest.mark.parametrize("case", list(CASES))
def test_network_matches_the_fp64_restatement(gpu, case):
    coords = CASES[case]()
    res, inter = run(model(gpu), coords, gpu, debug=True)
    out = res.F.cpu().numpy()
    assert torch.equal(res.C.cpu(), torch.from_numpy(coords.astype(np.int32)))
    want, want_inter = ref.network(coords, np.ones((len(coords), 1)), f32_state(seeded()))
    err = compare(coords, out, inter, want, want_inter)
    scale = {k: max(1.0, float(np.abs(v).max())) for k, v in
             [("cat%d" % l, want_inter["cat"][l]) for l in range(4)] + [("s4", want_inter["s4"]), ("hidden", want_inter["hidden"])]}
    print(f"[featnet {case}] n={len(coords)} levels={inter['levels']} max|gpu-fp64| "
          + " ".join(f"{k}={v:.2e}" for k, v in err.items()) + " | magnitudes " + " ".join(f"{k}={v:.1f}" for k, v in scale.items()))
    assert err["out"] <= TOL, err
    for k, s in scale.items():
        assert err[k] <= TOL * s, (k, err[k], s)


def test_runs_are_bit_identical_and_a_batch_equals_its_clouds(gpu):
    m = model(gpu)
    both = batch_of_two()
    a = run(m, both, gpu).F
    b = run(m, both, gpu).F
    assert a.view(torch.int32).equal(b.view(torch.int32))
    parts = run(m, both, gpu).decomposed_features
    for i in range(2):
        one = both[both[:, 0] == i].copy()
        one[:, 0] = 0
        single = run(m, one, gpu).F
        assert single.view(torch.int32).equal(parts[i].contiguous().view(torch.int32)), f"cloud {i}"


def test_errors_raise(gpu):
    from umeregrobust_amd.sparse import SparseTensor
    m = model(gpu)
    c = edge_cloud("one_cell")
    with pytest.raises(ValueError, match="duplicate"):
        run(m, np.concatenate([c, c[5:6]]), gpu)
    for bad in ([0, 1 << 17, 0, 0], [0, 0, -(1 << 17) - 1, 0], [0, 0, 0, 1 << 20], [-1, 0, 0, 0]):
        with pytest.raises(ValueError, match="outside"):
            run(m, np.concatenate([c, [bad]]), gpu)
    two = np.concatenate([c[:10], c[:10] + [1, 0, 0, 0]])          # the same coordinates in two batch items are not duplicates
    assert run(m, two, gpu).F.shape == (20, 32)
    st_cpu = SparseTensor(torch.ones(len(c), 1), coordinates=torch.from_numpy(c.astype(np.int32)))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(st_cpu)
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
        m.train()(st_cpu)
    m.eval()
    st = SparseTensor(torch.ones(len(c), 1, device=gpu), coordinates=torch.from_numpy(c.astype(np.int32)).to(gpu))
    with pytest.raises(RuntimeError, match="no backward"):
        m(st)
    # and the model still works after every refusal
    assert run(m, c, gpu).F.shape == (len(c), 32)


# ---- guard bands around every entry point of include/umereg_featnet.h -------------------------------------------------------

PAD, CANARY = 4096, 0xA5


def test_guard_bands_and_run_twice(gpu):
    """Every device buffer of umereg_featnet_forward_f32 between canaries, at exactly the size the header / the query states;
    the workspace pre-filled with garbage, the outputs with poison; two runs with other garbage and poison agree byte for byte.
    (The other four entry points are host-only queries: their outputs are checked against the workspace here too.)"""
    import ctypes
    from umeregrobust_amd import models
    lib = models.load_native()
    coords = batch_of_two()[::7].copy()
    n, batch = len(coords), 2
    params = model(gpu).packed_parameters()
    assert params.numel() == lib.umereg_featnet_params_count()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    results = []
    for poison, garbage in ((0xCD, 0xEE), (0x3C, 0x17)):
        bufs = []

        def alloc(nbytes, fill):
            full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=gpu)
            full[:PAD] = CANARY
            full[PAD + nbytes:] = CANARY
            full[PAD:PAD + nbytes] = fill
            bufs.append((full, nbytes))
            return full

        def inp(a):
            a = np.ascontiguousarray(a)
            full = alloc(a.nbytes, 0)
            full[PAD:PAD + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(gpu))
            return full.data_ptr() + PAD

        c_p = inp(coords.astype(np.int32))
        f_p = inp(np.ones((n, 1), np.float32))
        p_p = inp(params.cpu().numpy())
        out = alloc(n * 32 * 4, poison)
        status = alloc(8 * 4, poison)
        ws_bytes = lib.umereg_featnet_workspace_bytes(n, batch)
        ws = alloc(ws_bytes, garbage)
        rc = lib.umereg_featnet_forward_f32(c_p, f_p, n, batch, p_p, out.data_ptr() + PAD, status.data_ptr() + PAD,
                                            ws.data_ptr() + PAD, ws_bytes, stream)
        assert rc == 0, lib.umereg_last_error()
        torch.cuda.synchronize()
        for full, nb in bufs:
            assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"
        # the maps alone, into buffers of their own
        status_m = alloc(8 * 4, poison)
        ws_m = alloc(ws_bytes, garbage)
        rc = lib.umereg_featnet_build_maps(c_p, n, batch, status_m.data_ptr() + PAD, ws_m.data_ptr() + PAD, ws_bytes, stream)
        assert rc == 0, lib.umereg_last_error()
        torch.cuda.synchronize()
        for full, nb in bufs:
            assert bool((full[:PAD] == CANARY).all()) and bool((full[PAD + nb:] == CANARY).all()), "a guard band was written"
        st = status[PAD:PAD + 32].view(torch.int32).cpu()
        assert int(st[0]) == 0 and int(st[1]) == n
        assert torch.equal(st, status_m[PAD:PAD + 32].view(torch.int32).cpu())
        results.append((out[PAD:PAD + n * 32 * 4].clone(), st))
        for which in range(models.BUF_MASKS + 1):
            off, cols = ctypes.c_size_t(), ctypes.c_int32()
            assert lib.umereg_featnet_buffer(n, batch, which, ctypes.addressof(off), ctypes.addressof(cols)) == 0
            assert off.value + n * cols.value * 4 <= ws_bytes
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


# ---- the evaluation loop from a cache without features ----------------------------------------------------------------------

def test_evaluate_with_checkpoint_equals_a_cache_with_dumped_features(gpu, tmp_path):
    """A tiny pair cache without features + a seeded checkpoint: `evaluate --checkpoint` gives the per-pair RRE / RTE of the
    same cache with the same model's features dumped into it."""
    import argparse
    from umeregrobust_amd import evaluate
    from umeregrobust_amd.datasets import write_cached_pair
    from umeregrobust_amd.synth import synth_pair_cfg
    from umeregrobust_amd.utils.general_utils import benchmark_config_path, update_namespace_from_yaml
    ck = tmp_path / "w.pth"
    torch.save({"epoch": 1, "model_state_dict": torch_state(seeded(7)), "optimizer_state_dict": {}, "total_loss": 0.0}, ck)
    m = model(gpu, seed=7)
    plain, dumped = tmp_path / "plain", tmp_path / "dumped"
    for i in range(2):
        p = synth_pair_cfg(20 + i, "NS", "test", n_src=6000, n_tgt=5000)
        item = []
        for pts in (p.src_pts, p.tgt_pts):
            c = np.round(pts / 0.3).astype(np.int32)
            keep = np.sort(np.unique(c, axis=0, return_index=True)[1])
            item.append((pts[keep], np.zeros(len(keep), np.int64), c[keep]))
        (sp, ss, sc), (tp, ts_, tc) = item
        T = p.gt_tform.astype(np.float32)
        moved = (sp @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        matches = np.stack([np.arange(min(len(sp), len(tp)))] * 2, 1).astype(np.int64)
        fields = (torch.from_numpy(sp), torch.from_numpy(ss), torch.from_numpy(sc), torch.from_numpy(tp), torch.from_numpy(ts_),
                  torch.from_numpy(tc), torch.from_numpy(moved), torch.from_numpy(T), matches)
        name = os.path.join("test", "08", f"{i:06d}_{i + 1:06d}.pickle")
        write_cached_pair(str(plain / name), fields)
        feats = [run(m, np.concatenate([np.zeros((len(c), 1), np.int64), c], 1), gpu).F.cpu() for c in (sc, tc)]
        write_cached_pair(str(dumped / name), fields, feats[0], feats[1])
    args = update_namespace_from_yaml(argparse.Namespace(benchmark="kitti_test"), benchmark_config_path("kitti_test"))
    args.max_pc_size = 100000          # no dilution: the collate only permutes, and the network is row-order invariant
    args.split = "test"

    def rre_rte(cache, checkpoint):
        rng = np.random.RandomState(0)
        pairs = list(evaluate.cached_pairs(str(cache), None, "test", range(2), args, gpu, rng=rng, checkpoint=checkpoint))
        with torch.no_grad():
            res = evaluate.evaluate_pairs(pairs, args, rng=rng, refine=False)
        return res["rre"].numpy(), res["rte"].numpy(), pairs

    rre_a, rte_a, pairs_a = rre_rte(dumped, None)
    rre_b, rte_b, pairs_b = rre_rte(plain, str(ck))
    for a, b in zip(pairs_a, pairs_b):
        assert torch.equal(a["src_feat"], b["src_feat"]) and torch.equal(a["tgt_feat"], b["tgt_feat"])
    assert np.array_equal(rre_a, rre_b) and np.array_equal(rte_a, rte_b)
    # and the cache without features is refused without a checkpoint
    with pytest.raises(KeyError, match="src_feat"):
        next(evaluate.cached_pairs(str(plain), None, "test", range(1), args, gpu))
