"""GPU: the sampling equalizer (csrc/equalize.hip) against its restatement (tests/equalizer_ref.py), stage by stage on the smallest
shapes that can still go wrong, then the whole call, the raw entries between guard bands, and the three places it plugs into.

What is exact is compared exactly: q, r2, src_index and rho2 are integers or single f32 operations; the placement is compared bit
for bit with csrc/equalize_math.h compiled for the host.  What is fp64 with another summation order is bounded:
  normals     angle <= 1e-10 / gap + sqrt(3) 2^-25 (equalizer_ref.normal_bound), gap = (l1 - l0) / l2 of the neighbourhood;
  projection  device and restatement evaluate x' = x + (m . n) n in fp64 from the same f32 inputs and the same neighbour set.  The sums
              of N <= 1 025 terms differ by N u relative (u = 2^-53), so m moves by ~1e-13 rho, n by ~1e-13 / gap, and the fp64 value by
              delta <= rho * 1e-12 * (1 + 1 / gap) + 4 u |x| (a decade of room); the device then rounds once to f32: half an ulp of the
              coordinate.  |device - restatement's fp64 value| <= ulp32(coordinate) / 2 + delta, per coordinate."""
import os

import numpy as np
import pytest
import torch

import equalizer_ref as ref
import raw_scan_ref as rref
from conftest import load_golden

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = ref.gpu_cases()
IDS = [c[0] for c in CASES]
# the share of a case's fitted normals (surfels) and moved samples (projection) whose eigen-gap is at least GAP_FLOOR: 90 %, except
# where triples of identical points sit beside distinct ones -- a point whose nearest site is a triple sees itself and two copies, a
# collinear neighbourhood with no normal to judge (restatement: 74 % of the surfels, 89 % of the moved samples clear the floor)
JUDGED_SHARE = {"duplicates": 0.7}


def dev_t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def stages(gpu):
    """every case through the three device stages, and the restatement's surfels: computed once, shared, never changed"""
    from umeregrobust_amd import equalizer
    out = {}
    for name, pts, M, knn, rmax in CASES:
        p = dev_t(pts, gpu)
        normals, r2, q = equalizer.surfels(p, knn, rmax)
        samples, src, rho2 = equalizer.sample(p, normals, r2, q, M, knn, seed=0)
        moved, cnt = equalizer.project(samples, rho2, p, return_count=True)
        torch.cuda.synchronize()
        out[name] = dict(pts=pts, M=M, knn=knn, rmax=rmax, want=ref.surfels(pts, knn, rmax),
                         normals=normals.cpu().numpy(), r2=r2.cpu().numpy(), q=q.cpu().numpy().view(np.uint32),
                         samples=samples.cpu().numpy(), src=src.cpu().numpy(), rho2=rho2.cpu().numpy(),
                         moved=moved.cpu().numpy(), cnt=cnt.cpu().numpy())
    return out


def test_the_cases_cover_the_sizes_and_are_what_they_are_named(stages):
    assert {len(c[1]) for c in CASES} == {3, 4, 63, 64, 65, 257, 1025} and {c[2] for c in CASES} == {1, 63, 64, 65, 1000, 4097}
    s = stages
    assert (s["duplicates"]["want"]["q"] == 0).sum() == 30 and (s["duplicates"]["want"]["r2"] == 0).sum() == 30
    rmax2, _ = ref.scale_of(0.01)
    assert (s["capped"]["want"]["r2"] == rmax2).all()                                     # r_max caps every support
    assert 0 < int(s["few_weights"]["want"]["q"].astype(np.int64).sum()) < s["few_weights"]["M"]       # Qt < M
    assert s["k_is_n_3"]["want"]["K"] == 3 and s["k_is_n_4"]["want"]["K"] == 4            # K = n < knn
    assert np.abs(s["far"]["pts"][:, 0]).min() >= 900.0


@pytest.mark.parametrize("name", IDS)
def test_surfels(stages, name):
    s = stages[name]
    want = s["want"]
    assert np.array_equal(s["q"], want["q"]) and np.array_equal(s["r2"].view(np.uint32), want["r2"].view(np.uint32))
    got = s["normals"].astype(np.float64)
    fixed = (want["gap"] == 0) & (want["normals"] == [0.0, 0.0, 1.0]).all(axis=1)          # a zero covariance: the rule (0, 0, 1)
    judged = ~fixed & (want["gap"] >= ref.GAP_FLOOR)
    share = float(judged.sum()) / max(int((~fixed).sum()), 1)
    err = ref.angle(got[judged], want["normals"][judged])
    room = ref.normal_bound(want["gap"][judged])
    print(f"[surfels {name}] n {len(got)}, judged {int(judged.sum())} ({100 * share:.1f} % of the fitted), smallest gap judged "
          f"{want['gap'][judged].min():.2e}, worst angle {err.max():.2e} rad, worst angle / bound {(err / room).max():.3f}")
    assert share >= JUDGED_SHARE.get(name, 0.9), "the gap gate must leave the case judged"
    assert (err <= room).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-6
    k = np.abs(got).argmax(axis=1)
    assert (got[np.arange(len(got)), k] > 0).all()                                        # canonical sign everywhere
    assert np.array_equal(got[fixed], np.tile([0.0, 0.0, 1.0], (int(fixed.sum()), 1)))


@pytest.mark.parametrize("name", IDS)
def test_sample(stages, name):
    """fed the device's own surfels: src_index and rho2 equal everywhere (the allocation is integer), positions equal bit for bit to
    the host-compiled header"""
    s = stages[name]
    if ref.host_program() is None:
        pytest.skip("no hipcc found: csrc/equalize_math.h cannot be compiled here")
    src, Qt = ref.allocate(s["q"], s["M"], seed=0)
    assert np.array_equal(s["src"], src)
    assert np.array_equal(s["rho2"].view(np.uint32), s["r2"][src].view(np.uint32))
    assert (s["q"][src] > 0).all(), "a point without area was chosen"
    _, _, x = ref.host_place(s["pts"], s["normals"], s["r2"], src, s["want"]["K"], seed=0)
    same = np.array_equal(s["samples"].view(np.uint32), x.view(np.uint32))
    print(f"[sample {name}] M {s['M']}, Qt {Qt}, distinct sources {len(set(src.tolist()))}, positions differing from the host header: "
          f"{int((s['samples'].view(np.uint32) != x.view(np.uint32)).any(axis=1).sum())}")
    assert same


@pytest.mark.parametrize("name", IDS)
def test_project(stages, name):
    s = stages[name]
    want = ref.project(s["samples"], s["rho2"], s["pts"])
    print(f"[project {name}] cut margin min |d2 - rho2| / rho2 = {want['margin']:.3e}")
    assert want["margin"] > 0.0
    assert np.array_equal(s["cnt"], want["count"])                                         # the neighbour sets are equal
    stayed = want["gap"] == 0
    assert np.array_equal(s["moved"][stayed & (want["count"] < 3)].view(np.uint32), s["samples"][stayed & (want["count"] < 3)].view(np.uint32))
    x64 = want["x"]
    rho = np.sqrt(s["rho2"].astype(np.float64))
    with np.errstate(divide="ignore"):
        delta = rho * 1e-12 * (1.0 + 1.0 / want["gap"]) + 4 * 2.0 ** -53 * np.abs(x64).max(axis=1)
    delta[stayed] = 0.0
    bound = 0.5 * np.spacing(np.abs(x64).astype(F32)).astype(np.float64) + delta[:, None]
    err = np.abs(s["moved"].astype(np.float64) - x64)
    moved = ~stayed
    well = moved & (want["gap"] >= ref.GAP_FLOOR)
    print(f"[project {name}] moved {int(moved.sum())} of {len(rho)}, gap >= {ref.GAP_FLOOR}: {int(well.sum())}, worst err / bound "
          f"{float((err / bound)[moved].max(initial=0.0)):.3f}, worst err {float(err.max()):.3e} m")
    assert (err <= bound).all()
    assert not moved.any() or well.sum() >= JUDGED_SHARE.get(name, 0.9) * moved.sum(), "the gap must leave the case judged to an ulp"


@pytest.mark.parametrize("name", ["plane", "corner", "far", "few_weights"])
def test_whole_call(gpu, stages, name):
    """equals the chained stages bit for bit; twice, on different streams and workspaces, equal bits; another seed moves the samples
    but not q"""
    from umeregrobust_amd import equalizer
    s = stages[name]
    p = dev_t(s["pts"], gpu)
    kw = dict(num_points=s["M"], knn=s["knn"], max_radius=s["rmax"])
    out, src = equalizer.equalize_cloud(p, return_index=True, **kw)
    assert out.dtype == torch.float32 and out.shape == (s["M"], 3) and src.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy().view(np.uint32), s["moved"].view(np.uint32)) and np.array_equal(src.cpu().numpy(), s["src"])
    flat = equalizer.equalize_cloud(p, project=False, **kw)
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), s["samples"].view(np.uint32))
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        again = equalizer.equalize_cloud(p, **kw)
    side.synchronize()
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    other, src2 = equalizer.equalize_cloud(p, seed=1, return_index=True, **kw)
    assert not torch.equal(other, out)
    _, _, q2 = equalizer.surfels(p, s["knn"], s["rmax"])
    assert np.array_equal(q2.cpu().numpy().view(np.uint32), s["q"])
    # the whole call against the restatement's fp64 chain: the same sources, positions to the placement's f32 roundings + the projection
    want = ref.equalize(s["pts"], s["M"], s["knn"], s["rmax"], do_project=False)
    assert np.array_equal(src.cpu().numpy(), want["src"])
    big = float(np.abs(s["pts"]).max()) + 1.0
    assert np.abs(flat.cpu().numpy().astype(np.float64) - want["x"]).max() <= 8 * float(np.spacing(F32(big)))


def test_guard_bands_run_twice_dirty_workspace(gpu):
    """every entry between 4 KiB guard bands, outputs and workspace at exactly the stated sizes, twice with another poison and another
    garbage in the workspace: the bands intact, the outputs equal byte for byte"""
    from test_abi_guard import Guard
    from umeregrobust_amd import equalizer
    lib = equalizer.load_native()
    pts = ref.corner_cloud(777, np.random.RandomState(3))
    n, M, knn = len(pts), 1301, 16
    runs = []
    for run in (0, 1):
        G = Guard(gpu, run)
        with torch.cuda.device(gpu):
            p, _ = G.inp(pts)
            nrm, t_nrm = G.out((n, 3), torch.float32, "normals")
            r2, t_r2 = G.out((n,), torch.float32, "r2")
            q, t_q = G.out((n,), torch.int32, "q")
            ws, nws = G.ws(lib.umereg_equalize_workspace_bytes(n, 1, knn), "ws_surfels")
            G.call("umereg_equalize_surfels_f32", p, n, knn, 1.0, nrm, r2, q, ws, nws, G.stream)
            x, t_x = G.out((M, 3), torch.float32, "samples")
            src, t_src = G.out((M,), torch.int64, "src_index")
            rho2, t_rho2 = G.out((M,), torch.float32, "rho2")
            tot, t_tot = G.out((1,), torch.int64, "total")
            ws, nws = G.ws(lib.umereg_equalize_workspace_bytes(n, 1, knn), "ws_sample")
            G.call("umereg_equalize_sample_f32", p, nrm, r2, q, n, M, knn, 5, x, src, rho2, tot, ws, nws, G.stream)
            y, t_y = G.out((M, 3), torch.float32, "projected")
            cnt, t_cnt = G.out((M,), torch.int32, "nb_count")
            ws, nws = G.ws(lib.umereg_equalize_workspace_bytes(n, 1, 3), "ws_project")
            G.call("umereg_equalize_project_f32", x, rho2, p, M, n, y, cnt, ws, nws, G.stream)
            z, t_z = G.out((M, 3), torch.float32, "out")
            src2, t_src2 = G.out((M,), torch.int64, "src_index")
            tot2, t_tot2 = G.out((1,), torch.int64, "total")
            ws, nws = G.ws(lib.umereg_equalize_workspace_bytes(n, M, knn), "ws_cloud")
            G.call("umereg_equalize_cloud_f32", p, n, M, knn, 1.0, 1, 5, z, src2, tot2, ws, nws, G.stream)
        G.check()
        outs = dict(normals=t_nrm, r2=t_r2, q=t_q, samples=t_x, src=t_src, rho2=t_rho2, total=t_tot, projected=t_y, count=t_cnt, out=t_z,
                    src2=t_src2, total2=t_tot2)
        runs.append({k: v.detach().cpu().clone() for k, v in outs.items()})
        del G
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), f"`{k}` differs between two runs"
    assert torch.equal(runs[0]["out"].view(torch.int32), runs[0]["projected"].view(torch.int32)) and torch.equal(runs[0]["src"], runs[0]["src2"])
    assert int(runs[0]["total"]) == int(runs[0]["q"].numpy().view(np.uint32).astype(np.int64).sum()) == int(runs[0]["total2"]) > 0


def test_refusals_are_the_hosts(gpu):
    """Qt == 0, a bad knn and sizes above 2^22 are refused on the host; an all-duplicate cloud, whose Qt is zero only on the device, is
    the ValueError of the one word read back"""
    from umeregrobust_amd import equalizer
    p = dev_t(ref.plane_cloud(50, np.random.RandomState(0)), gpu)
    with pytest.raises(ValueError, match="Qt"):
        equalizer.equalize_cloud(p[:2], num_points=10)
    with pytest.raises(ValueError, match="knn"):
        equalizer.equalize_cloud(p, knn=2)
    with pytest.raises(ValueError, match="num_points"):
        equalizer.equalize_cloud(p, num_points=(1 << 22) + 1)
    with pytest.raises(ValueError, match="Qt are 0"):
        equalizer.equalize_cloud(p[:1].repeat(40, 1), num_points=10)


# ---- in place, at reduced size ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scan_tree(tmp_path_factory):
    """two pairs (frames 0 -> 1 and 1 -> 0) of small labelled synthetic scans as a SemanticKITTI tree, the kind tests/test_raw_pair_gpu.py uses"""
    g17 = load_golden("g17_raw_scan.npz")
    root = tmp_path_factory.mktemp("raw_eq")
    (s0, w0), (s1, w1), T = rref.synth_labelled_scans(170, n=3000)
    rref.write_kitti_frame(root / "sequences", 3, 10, s0, w0)
    rref.write_kitti_frame(root / "sequences", 3, 12, s1, w1)
    tforms = np.stack([T, np.linalg.inv(T.astype(np.float64)).astype(np.float32)])
    rref.write_metadata(root / "meta", "train", np.array([[3, 10, 12], [3, 12, 10]], np.int64), tforms)
    return dict(data=str(root / "sequences"), meta=str(root / "meta"), scan=(s0, w0), lm=(g17["lm_keys"], g17["lm_values"]),
                label_config=rref.write_learning_map(root / "labels.yaml", g17["lm_keys"], g17["lm_values"]))


def test_complete_cloud_with_the_built_in(gpu, scan_tree):
    from umeregrobust_amd import equalizer, raw_scan
    lut = raw_scan.learning_map_lut(*scan_tree["lm"])
    pts, seg = raw_scan.prepare_cloud(*scan_tree["scan"], lut=lut, sem16=True, keep_unlabeled=True, device=gpu)
    new_pts, new_seg = raw_scan.complete_cloud(pts, seg, equalizer.sampling_equalizer)
    assert new_pts.shape == (125000, 3) and new_pts.dtype == torch.float32 and new_pts.device == pts.device
    assert new_seg.shape == (125000,) and new_seg.dtype == torch.int64 and bool(torch.isfinite(new_pts).all())
    assert set(np.unique(new_seg.cpu().numpy())) <= set(np.unique(seg.cpu().numpy())) | {0} and int((new_seg != 0).sum()) > 1000
    small, small_seg = raw_scan.complete_cloud(pts, seg, equalizer.make_equalizer(num_points=4000, knn=8))
    assert small.shape == (4000, 3) and small_seg.shape == (4000,)


def test_a_raw_pair_dataset_with_the_built_in(gpu, scan_tree):
    from umeregrobust_amd import equalizer
    from umeregrobust_amd.datasets import SemanticKITTIDataset
    ds = SemanticKITTIDataset(scan_tree["data"], "train", metadata_dir=scan_tree["meta"], label_config=scan_tree["label_config"], device=gpu,
                              use_pc_completion=True, completion_fn=equalizer.sampling_equalizer)
    item = ds[0]
    assert len(item) == 9 and [t.dtype for t in item] == [torch.float32, torch.int64, torch.int32] * 2 + [torch.float32, torch.float32, torch.int64]
    assert len(item[0]) > 100 and len(item[3]) > 100 and (item[1] != 0).all() and (item[4] != 0).all() and len(item[8]) > 0


def test_the_cache_command_with_the_built_in(gpu, scan_tree, tmp_path):
    from umeregrobust_amd.datasets import CachedPairDataset
    from umeregrobust_amd.datasets import sem_preprocessing as sp
    out = tmp_path / "cache"
    argv = ["--data_path", scan_tree["data"], "--output_path", str(out), "--split", "train", "--nksr", "True", "--dataset_mode", "kitti",
            "--metadata_dir", scan_tree["meta"], "--label_config", scan_tree["label_config"], "--completion",
            "umeregrobust_amd.equalizer:sampling_equalizer"]
    assert sp.main(argv) == (2, 0)
    listed = CachedPairDataset(str(out), split="train")
    assert listed.files == [(3, 10, 12), (3, 12, 10)]
    item = listed[0]
    assert len(item) == 9 and len(item[0]) > 100 and len(item[8]) > 0 and os.path.isdir(os.path.join(str(out), "train", "03"))
