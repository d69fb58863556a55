"""GPU: the device-side collate (umeregrobust_amd/collate.py on csrc/collate.hip, include/umereg_collate.h) against the reference's
own collate results (tests/golden/g10_collate.npz) and against the host collate `batch_collate_fn_dset` on constructed items: every
output equal (`array_equal`, dtype and shape), the host generator left in the same state.  No tolerance anywhere: the collate copies
values and computes indices."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

KEYS = ("src_pts", "src_seg", "src_coords", "tgt_pts", "tgt_seg", "tgt_coords", "src_pts_tform", "gt_tform", "matches")
OUT = ("src_pts", "src_seg", "src_coords", "src_feat", "tgt_pts", "tgt_seg", "tgt_coords", "tgt_feat", "src_pts_tform", "gt_tform", "matches",
       "src_net_feat", "tgt_net_feat")


def on_device(items, dev):
    return [tuple(t.to(dev) for t in it) for it in items]


def assert_same(got, want, what=""):
    """got: the device collate's tuple; want: numpy arrays or host tensors of the expected values"""
    assert len(got) == len(want), what
    for name, a, b in zip(OUT, got, want):
        b = b.numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        assert isinstance(a, torch.Tensor), (what, name)
        if name != "gt_tform":                              # (gt_tform may stay where the items had it)
            assert a.device.type == "cuda", (what, name)
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name)


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 1. the reference's golden ---------------------------------------------------------------------------------------------

def test_device_collate_equals_reference_golden(gpu):
    """both cases of tests/test_input_side.py::test_collate_equals_reference_golden, items on the device, global numpy stream"""
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    from umeregrobust_amd.datasets import batch_collate_fn_dset
    g = load_golden("g10_collate.npz")
    items = [tuple(torch.from_numpy(g[f"in{i}_{k}"]) for k in KEYS) for i in range(3)]
    for tag, data, nm, mx in (("b3", items, 60, 600), ("b1", items[1:2], 10000, 100000)):
        np.random.seed(10)
        batch_collate_fn_dset(data, num_matches=nm, max_pc_size=mx)
        host_state = np.random.get_state()
        np.random.seed(10)
        res = batch_collate_fn_dset_device(on_device(data, gpu), num_matches=nm, max_pc_size=mx)
        assert len(res) == 11
        assert_same(res, [g[f"{tag}_{name}"] for name in OUT[:11]], tag)
        assert same_state(np.random.get_state(), host_state), tag
        assert np.random.rand() == float(g[f"{tag}_next_rand"])


# ---- 2. constructed items against the host collate ---------------------------------------------------------------------------

def make_matches(rng, ns, nt, m):
    """m rows (source, target), sorted by neither column, with every rule of the match semantics in play: sources listed several
    times (one of them with three DIFFERENT targets, in unsorted file order), several sources pointing at one target"""
    rows = np.stack([rng.randint(0, ns, m), rng.randint(0, nt, m)], axis=1).astype(np.int64)
    if m >= 6 and ns >= 3 and nt >= 3:
        at = rng.choice(m, 6, replace=False)
        s0 = int(rng.randint(0, ns))
        ta, tb, tc = np.sort(rng.choice(nt, 3, replace=False))
        rows[np.sort(at[:3])] = [[s0, tb], [s0, tc], [s0, ta]]              # file order: the middle target first
        t0 = int(rng.randint(0, nt))
        sa, sb, sc = np.sort(rng.choice(ns, 3, replace=False))
        rows[np.sort(at[3:])] = [[sc, t0], [sa, t0], [sb, t0]]              # the lowest source is not the first row
    return rows


def make_item(rng, ns, nt, m, seg_dtype=np.int64, feat=False):
    def cloud(n):
        return (torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)), torch.from_numpy(rng.randint(0, 20, n).astype(seg_dtype)),
                torch.from_numpy(rng.randint(-500, 500, (n, 3)).astype(np.int32)))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = rng.standard_normal(3)
    item = cloud(ns) + cloud(nt) + (torch.from_numpy(rng.standard_normal((ns, 3)).astype(np.float32)), torch.from_numpy(T),
                                    torch.from_numpy(make_matches(rng, ns, nt, m).reshape(m, 2)))
    if feat:                                                                 # feature = original index, as tests/test_input_side.py has it
        item += (torch.arange(ns, dtype=torch.float32)[:, None].repeat(1, 4), torch.arange(nt, dtype=torch.float32)[:, None].repeat(1, 4))
    return item


# name -> (per element (source size, target size, match rows), num_matches, max_pc_size); M runs from 0 to 3 Ns
CASES = {
    "one_point": ([(1, 1, 3)], 20, 100000),
    "around_a_wave": ([(63, 65, 3 * 63), (65, 63, 40)], 20, 100000),
    "cap_binds": ([(257, 1000, 257), (1000, 257, 3000), (300, 300, 150)], 20, 256),
    "several_blocks": ([(5000, 4096, 15000), (5000, 4096, 2500)], 512, 100000),
    "an_empty_list_among_full_ones": ([(300, 280, 900), (290, 310, 0), (128, 129, 128)], 20, 200),      # M = 0: the batch keeps no match
}


@functools.lru_cache(maxsize=None)
def host_case(name):
    """-> (items on the host, the host collate's result, the generator state after it): computed once per case"""
    from umeregrobust_amd.datasets import batch_collate_fn_dset
    shapes, nm, mx = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    items = [make_item(rng, *s) for s in shapes]
    draw = np.random.RandomState(7)
    want = batch_collate_fn_dset(items, num_matches=nm, max_pc_size=mx, rng=draw)
    return items, want, draw.get_state()


@pytest.mark.parametrize("where", ["items_on_host", "items_on_device"])
@pytest.mark.parametrize("name", list(CASES))
def test_device_collate_equals_host_collate(gpu, name, where):
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    items, want, state = host_case(name)
    _, nm, mx = CASES[name]
    draw = np.random.RandomState(7)
    got = batch_collate_fn_dset_device(on_device(items, gpu) if where == "items_on_device" else items, num_matches=nm, max_pc_size=mx,
                                       rng=draw, device=gpu)
    print(f"{name}: clouds {tuple(want[0].shape)} / {tuple(want[4].shape)}, matches {tuple(want[10].shape)}")
    assert_same(got, want, name)
    assert same_state(draw.get_state(), state)
    if where == "items_on_device":
        assert got[9].device.type == "cuda"
    if name == "an_empty_list_among_full_ones":
        assert tuple(want[10].shape) == (3, 0, 2)
    elif name != "one_point":
        assert want[10].shape[1] > 0, "the case must keep some matches to say anything about them"


# ---- 3. edges --------------------------------------------------------------------------------------------------------------

def both(items, gpu, nm, mx=100000, seed=3, **kw):
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    from umeregrobust_amd.datasets import batch_collate_fn_dset
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    want = batch_collate_fn_dset(items, num_matches=nm, max_pc_size=mx, rng=a)
    got = batch_collate_fn_dset_device(on_device(items, gpu), num_matches=nm, max_pc_size=mx, rng=b, **kw)
    assert same_state(a.get_state(), b.get_state())
    return got, want


def test_an_element_without_matches_empties_the_batch(gpu):
    rng = np.random.RandomState(11)
    items = [make_item(rng, 300, 280, 900), make_item(rng, 290, 310, 0)]
    assert tuple(items[1][8].shape) == (0, 2)
    got, want = both(items, gpu, 50)
    assert tuple(got[10].shape) == (2, 0, 2) and got[10].dtype == torch.int64
    assert_same(got, want)


def test_all_matches_thinned_away(gpu):
    """every match of element 1 names a source point that its dilution drops: no survivor, k == 0, and the draw of nothing is
    still made (the generator states agree)"""
    rng = np.random.RandomState(12)
    items = [make_item(rng, 400, 400, 1200), make_item(rng, 400, 400, 0)]
    twin = np.random.RandomState(3)
    for _ in range(2):
        twin.choice(400, 40, replace=False)                                  # element 0: source draw, target draw
    dropped = np.setdiff1d(np.arange(400), twin.choice(400, 40, replace=False))
    rows = np.stack([rng.choice(dropped, 500), rng.randint(0, 400, 500)], axis=1).astype(np.int64)
    items[1] = items[1][:8] + (torch.from_numpy(rows),)
    got, want = both(items, gpu, 50, mx=40, seed=3)
    assert tuple(want[10].shape) == (2, 0, 2)
    assert_same(got, want)


def test_num_matches_above_every_survivor_count(gpu):
    rng = np.random.RandomState(13)
    items = [make_item(rng, 500, 450, 700), make_item(rng, 470, 520, 1400)]
    got, want = both(items, gpu, 10 ** 6)
    assert 0 < want[10].shape[1] < 450
    assert_same(got, want)


def test_features_follow_the_same_dilution(gpu):
    rng = np.random.RandomState(14)
    items = [make_item(rng, 300, 340, 600, feat=True), make_item(rng, 320, 310, 500, feat=True)]
    got, want = both(items, gpu, 40, mx=250)
    assert len(got) == 13 and tuple(got[11].shape) == (2, 250, 4) and tuple(got[12].shape) == (2, 250, 4)
    assert_same(got, want)
    for b in range(2):
        assert torch.equal(items[b][0][got[11][b, :, 0].long().cpu()], got[0][b].cpu())


def test_a_seg_field_of_another_integer_dtype_keeps_it(gpu):
    rng = np.random.RandomState(15)
    items = [make_item(rng, 200, 210, 300, seg_dtype=np.int32), make_item(rng, 190, 230, 300, seg_dtype=np.int32)]
    got, want = both(items, gpu, 30)
    assert got[1].dtype == torch.int32 and got[5].dtype == torch.int32
    assert_same(got, want)


def test_a_match_index_out_of_range_raises(gpu):
    from umeregrobust_amd.collate import batch_collate_fn_dset_device
    rng = np.random.RandomState(16)
    items = [make_item(rng, 200, 210, 300), make_item(rng, 190, 230, 300)]
    rows = items[1][8].clone()
    rows[17, 0] = 190                                                        # == Ns of element 1
    items[1] = items[1][:8] + (rows,)
    with pytest.raises(RuntimeError, match="element 1"):
        batch_collate_fn_dset_device(on_device(items, gpu), num_matches=30, rng=np.random.RandomState(0))
    rows[17] = torch.tensor([5, 230])                                        # == Nt
    with pytest.raises(RuntimeError, match="element 1"):
        batch_collate_fn_dset_device(on_device(items, gpu), num_matches=30, rng=np.random.RandomState(0))


# ---- 4. the raw entry between guard bands, twice -----------------------------------------------------------------------------

PAD, CANARY = 4096, 0xA5


class Guard:
    """buffers between two 4 KiB canaries (the pattern of tests/test_abi_guard.py): outputs pre-filled with poison, the workspace
    with garbage, both different in the two runs"""

    def __init__(self, dev, run):
        self.dev, self.poison, self.garbage, self.bufs = dev, (0xCD, 0x3C)[run], (0xEE, 0x17)[run], []

    def _alloc(self, nbytes, fill, name):
        full = torch.empty(nbytes + 2 * PAD, dtype=torch.uint8, device=self.dev)
        full[:PAD] = CANARY
        full[PAD + nbytes:] = CANARY
        full[PAD:PAD + nbytes] = fill
        self.bufs.append((name, full, nbytes))
        return full[PAD:PAD + nbytes]

    def inp(self, arr, name):
        a = np.ascontiguousarray(arr)
        view = self._alloc(a.nbytes, 0, name)
        view.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.dev))
        return view

    def out(self, nbytes, name):
        return self._alloc(nbytes, self.poison, name)

    def ws(self, nbytes):
        return self._alloc(nbytes, self.garbage, "workspace")

    def check(self):
        torch.cuda.synchronize()
        for name, full, n in self.bufs:
            assert bool((full[:PAD] == CANARY).all()), f"{name}: bytes BEFORE the buffer were written"
            assert bool((full[PAD + n:] == CANARY).all()), f"{name}: bytes BEHIND the buffer ({n} B) were written"


@pytest.mark.parametrize("ns,nt,n_src,n_tgt", [(63, 65, 50, 60), (5000, 4096, 4000, 3000)])
def test_raw_entry_between_guard_bands_twice(gpu, ns, nt, n_src, n_tgt):
    from umeregrobust_amd import collate
    from umeregrobust_amd.datasets.kitti_dataset import _Dilution, surviving_matches
    lib = collate.load_native()
    rng = np.random.RandomState(ns)
    item = make_item(rng, ns, nt, 3 * ns)
    m, b = 3 * ns, 5
    src, tgt = _Dilution(ns, n_src, rng), _Dilution(nt, n_tgt, rng)
    want_rows = surviving_matches(item[8].numpy(), src, tgt)
    cap = min(m, n_src, n_tgt)
    assert 0 < len(want_rows) < cap
    nws = lib.umereg_collate_workspace_bytes(ns, nt, m)
    assert nws > 0
    out_bytes = dict(src_pts=12 * n_src, src_seg=8 * n_src, src_coords=16 * n_src, src_pts_tform=12 * n_src, tgt_pts=12 * n_tgt,
                     tgt_seg=8 * n_tgt, tgt_coords=16 * n_tgt, matches=16 * cap, count=8)
    runs = []
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for run in (0, 1):
        G = Guard(gpu, run)
        ins = [G.inp(item[i].numpy(), KEYS[i]) for i in (0, 1, 2, 6, 3, 4, 5, 8)]
        ks, kt = G.inp(src.keep.astype(np.int64), "keep_src"), G.inp(tgt.keep.astype(np.int64), "keep_tgt")
        outs = {k: G.out(n, "out_" + k) for k, n in out_bytes.items()}
        ws = G.ws(nws)
        p = lambda t: t.data_ptr()                                          # noqa: E731
        with torch.cuda.device(gpu):
            rc = lib.umereg_collate_element(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), ns, p(ins[4]), p(ins[5]), p(ins[6]), nt, p(ins[7]), m,
                                            p(ks), n_src, p(kt), n_tgt, b, p(outs["src_pts"]), p(outs["src_seg"]), p(outs["src_coords"]),
                                            p(outs["src_pts_tform"]), p(outs["tgt_pts"]), p(outs["tgt_seg"]), p(outs["tgt_coords"]),
                                            p(outs["matches"]), p(outs["count"]), p(ws), nws, stream)
        assert rc == 0, lib.umereg_last_error().decode()
        G.check()
        got = {k: v.cpu().numpy().copy() for k, v in outs.items()}
        count = got["count"].view(np.int32)
        assert count[1] == 0 and count[0] == len(want_rows)
        tail = got["matches"][16 * int(count[0]):]
        assert (tail == G.poison).all(), "rows beyond out_count[0] were written"
        got["matches"] = got["matches"][:16 * int(count[0])]
        runs.append(got)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), f"output `{k}` differs between two runs (an unwritten byte, or a dependence on the workspace)"
    # ... and they are the host collate's values
    r = runs[0]
    assert np.array_equal(r["matches"].view(np.int64).reshape(-1, 2), want_rows)
    assert np.array_equal(r["src_pts"].view(np.float32).reshape(-1, 3), item[0].numpy()[src.keep])
    assert np.array_equal(r["src_seg"].view(np.int64), item[1].numpy()[src.keep])
    assert np.array_equal(r["src_pts_tform"].view(np.float32).reshape(-1, 3), item[6].numpy()[src.keep])
    assert np.array_equal(r["tgt_pts"].view(np.float32).reshape(-1, 3), item[3].numpy()[tgt.keep])
    assert np.array_equal(r["tgt_seg"].view(np.int64), item[4].numpy()[tgt.keep])
    for k, keep, coords in (("src_coords", src.keep, item[2]), ("tgt_coords", tgt.keep, item[5])):
        c = r[k].view(np.int32).reshape(-1, 4)
        assert (c[:, 0] == b).all() and np.array_equal(c[:, 1:], coords.numpy()[keep])


# ---- 5. the augmented item that stays on the device --------------------------------------------------------------------------

def test_augmented_item_stays_on_the_device(gpu):
    from umeregrobust_amd.datasets.kitti_dataset import augmented_item
    g16 = load_golden("g16_train_data.npz")
    item = tuple(torch.from_numpy(g16["item_" + k]) for k in KEYS)
    voxel, seed = float(g16["item_voxel"]), int(g16["item_seed"])
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    phases = []

    class Phase:
        def __init__(self, name):
            phases.append(name)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    host = augmented_item(item, voxel, a, gpu)
    dev = augmented_item(item, voxel, b, gpu, phase=Phase, to_host=False)
    assert same_state(a.get_state(), b.get_state()) and "to_host" not in phases and "matches" in phases
    assert len(dev) == len(host) == 9
    for name, h, d in zip(KEYS, host, dev):
        assert h.device.type == "cpu" and d.device.type == "cuda", name
        assert d.dtype == h.dtype and d.shape == h.shape and torch.equal(d.cpu(), h), name
