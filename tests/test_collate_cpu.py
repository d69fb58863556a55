"""CPU: the ground the device-side collate stands on -- the host side of include/umereg_collate.h (exports, the signature table,
the size query, argument checks before the device probe) and the refusal of the Python entry point without a GPU."""
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_collate_table_mirrors_its_header():
    """(keys, their number, exports, parameter counts, disjointness and the ABI version: tests/test_abi.py, one case per header)"""
    from umeregrobust_amd import collate
    assert sorted(collate.COLLATE_SIGNATURES) == ["umereg_collate_element", "umereg_collate_workspace_bytes"]
    umereg_h = open(os.path.join(REPO, "include", "umereg.h")).read()
    assert "umereg_collate" not in umereg_h


def test_workspace_query_is_monotone_and_refuses_bad_sizes():
    from umeregrobust_amd import collate
    q = collate.load_native().umereg_collate_workspace_bytes
    sizes = (1, 2, 63, 64, 65, 257, 1000, 1024, 1025, 4096, 5000, 50000, 100000, 2 ** 31 - 1)
    for m in (0, 1, 5000):
        last = 0
        for n in sizes:
            got = [q(n, sizes[0], m), q(sizes[0], n, m), q(n, n, m)]
            assert all(g > 0 and g % 256 == 0 for g in got), (n, m, got)
            assert got[2] >= max(got[0], got[1]) and got[2] >= last, (n, m)
            last = got[2]
    assert q(5000, 4096, 0) <= q(5000, 4096, 15000)
    # four int32 tables over the two clouds and the block counts of the scan
    assert 2 * 4 * (5000 + 4096) <= q(5000, 4096, 100) <= 2 * 4 * (5000 + 4096) + 5 * 256
    for bad in ((0, 5, 5), (5, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (2 ** 31, 5, 5), (5, 2 ** 31, 5), (5, 5, 2 ** 31),
                (2 ** 40, 5, 5), (5, 5, 2 ** 40)):
        assert q(*bad) == 0, bad
    assert collate.workspace_bytes(2 ** 31, 5, 5) == 0 and collate.workspace_bytes(5, 5, 0) > 0
    # the largest sizes the contract takes: no 32-bit wrap in the block count of the scan (2^21 blocks of 1024 targets, one more word)
    up = lambda v: (v + 255) // 256 * 256                                              # noqa: E731
    big = 2 ** 31 - 1
    want = lambda ns, nt: up(2 * up(4 * ns) + 2 * up(4 * nt) + 4 * (-(-nt // 1024) + 1))   # noqa: E731
    for ns, nt in ((big, big), (big - 1023, 7), (7, big - 1023), (7, big - 1022), (7, big), (5000, 4096)):
        assert q(ns, nt, big) == want(ns, nt), (ns, nt)


def test_collate_entry_checks_arguments_and_needs_a_device():
    from umeregrobust_amd import collate
    lib = collate.load_native()
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    names = ("src_pts", "src_seg", "src_coords", "src_pts_tform", "ns", "tgt_pts", "tgt_seg", "tgt_coords", "nt", "matches", "n_matches",
             "keep_src", "n_src", "keep_tgt", "n_tgt", "b", "out_src_pts", "out_src_seg", "out_src_coords", "out_src_pts_tform", "out_tgt_pts",
             "out_tgt_seg", "out_tgt_coords", "out_matches", "out_count", "workspace", "workspace_bytes", "stream")
    sizes = dict(ns=9, nt=8, n_matches=5, n_src=4, n_tgt=3, b=1, workspace_bytes=1 << 12, stream=None)
    call = lambda **kw: lib.umereg_collate_element(*[kw.get(k, sizes.get(k, p)) for k in names])          # noqa: E731
    # argument errors come before the device probe
    for kw in (dict(ns=0), dict(nt=0), dict(ns=-3), dict(ns=2 ** 31), dict(nt=2 ** 31), dict(n_matches=-1), dict(n_matches=2 ** 31),
               dict(n_src=0), dict(n_src=10), dict(n_tgt=0), dict(n_tgt=9), dict(b=-1), dict(keep_src=None), dict(keep_tgt=None),
               dict(out_count=None), dict(matches=None), dict(out_matches=None), dict(src_pts=None), dict(out_src_seg=None),
               dict(tgt_coords=None), dict(out_tgt_pts=None), dict(src_pts_tform=None)):
        assert call(**kw) == -1, kw                                                      # UMEREG_EINVAL
        assert lib.umereg_last_error()
    if lib.umereg_device_count(None, 0) == 0:
        assert call() == -2                                                              # UMEREG_ENODEV
        assert b"no CPU fallback" in lib.umereg_last_error()
        # a skipped field (both pointers NULL) and an empty match list are fine as arguments
        assert call(src_seg=None, out_src_seg=None) == -2
        assert call(matches=None, out_matches=None, n_matches=0) == -2
        assert call(workspace=None, workspace_bytes=0) == -2                             # (the workspace is checked after the probe)


def test_device_collate_raises_without_a_device(monkeypatch):
    from umeregrobust_amd import collate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    n = 5
    item = (torch.zeros(n, 3), torch.zeros(n, dtype=torch.int64), torch.zeros(n, 3, dtype=torch.int32)) * 2 + (
        torch.zeros(n, 3), torch.eye(4), torch.zeros(2, 2, dtype=torch.int64))
    rng = np.random.RandomState(0)
    state = rng.get_state()[1].copy()
    with pytest.raises(RuntimeError, match="needs a HIP device.*no CPU fallback"):
        collate.batch_collate_fn_dset_device([item], num_matches=4, rng=rng)
    assert np.array_equal(rng.get_state()[1], state), "the refusal must come before the first draw"


def test_device_collate_never_runs_in_a_loader_worker(monkeypatch, tmp_path):
    """a forked worker must not open the GPU: with the flag the loaders have no workers, whatever the config says (a pair cache with
    `use_aug=False` would otherwise get the config's 8), and the collate itself refuses inside a worker before it draws anything"""
    from umeregrobust_amd import collate
    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.datasets.kitti_dataset import write_cached_pair
    n = 5
    item = (torch.zeros(n, 3), torch.zeros(n, dtype=torch.int64), torch.zeros(n, 3, dtype=torch.int32)) * 2 + (
        torch.zeros(n, 3), torch.eye(4), torch.zeros(2, 2, dtype=torch.int64))
    for split in ("train", "val"):
        write_cached_pair(str(tmp_path / split / "00" / "000000_000001.pickle"), item)
    args = tc.make_config("kitti", cache_data_path=str(tmp_path), use_aug=False)
    assert args.num_workers == 8
    for loader in tc.make_loaders(args, device_collate=True):
        assert loader.num_workers == 0 and loader.pin_memory is False
        assert loader.collate_fn.func is collate.batch_collate_fn_dset_device and loader.dataset.items_on_device
    for loader in tc.make_loaders(args):                                                # the default is what it was
        assert loader.num_workers == 8 and loader.pin_memory is True and not loader.dataset.items_on_device
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    rng = np.random.RandomState(0)
    state = rng.get_state()[1].copy()
    with pytest.raises(RuntimeError, match="worker"):
        collate.batch_collate_fn_dset_device([item], num_matches=4, rng=rng)
    assert np.array_equal(rng.get_state()[1], state)


def test_driver_takes_the_flag_and_keeps_its_defaults():
    import inspect

    from umeregrobust_amd import train_coloring as tc
    from umeregrobust_amd.datasets.kitti_dataset import CachedPairDataset, augmented_item
    assert inspect.signature(tc.run).parameters["device_collate"].default is False
    assert inspect.signature(tc.make_loaders).parameters["device_collate"].default is False
    assert inspect.signature(tc.train_one_epoch).parameters["late_read"].default is False
    assert inspect.signature(augmented_item).parameters["to_host"].default is True
    assert inspect.signature(CachedPairDataset.__init__).parameters["items_on_device"].default is False
    assert inspect.signature(tc.SyntheticPairs.__init__).parameters["items_on_device"].default is False
    assert "device_collate" not in tc.DEFAULTS["kitti"]
    with pytest.raises(KeyError):
        tc.make_config("kitti", device_collate=True)
