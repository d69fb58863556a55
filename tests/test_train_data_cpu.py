"""CPU: the trainer's data side and driver, as far as they need no GPU, against tests/golden/g16_train_data.npz (the reference's own
one_side_ball_query_matches / mutual_ball_query_matches / convert_coords_to_grid_pts / cached_getitem_augmented on seeded lattice
clouds, tools/gen_train_data_golden.py):

  * the fp64 restatement of the match semantics (tests/train_data_ref.py) equals the reference's KDTree results on every source
    point whose margins exceed 1e-4 m; at most 1 % of the source cloud is excluded;
  * grid points, rotation matrices, the augmented ground truth;
  * the config parser takes every key of the reference's training configs (copies under tests/golden/ as fixtures);
  * the checkpoint dictionary and its file-name rule."""
import os

import numpy as np
import pytest
import torch

import train_data_ref as ref
from conftest import GOLDEN, load_golden

MARGIN = 1e-4       # metres: ten times the fp32 rounding of the reference's matmul transform at <= 50 m
MAX_EXCLUDED = 0.01


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_train_data.npz")


def test_restatement_equals_the_reference_matches(g16):
    src, tgt, T, r = g16["m_src"], g16["m_tgt"], g16["m_T"], float(g16["m_radius"])
    T_inv = torch.linalg.inv(torch.from_numpy(T)).numpy()
    ok = ref.decided(src, tgt, T, r, MARGIN)
    print(f"one side: {int((~ok).sum())} of {len(src)} source points inside the {MARGIN} m margin; reference rows {len(g16['m_one_side'])}")
    assert (~ok).mean() <= MAX_EXCLUDED
    assert np.array_equal(ref.rows_on(ref.one_side(src, tgt, T, r), ok), ref.rows_on(g16["m_one_side"], ok))
    # mutual: a source point is decided if its own search is and the reverse search of its target is
    ok_t = ref.decided(tgt, src, T_inv, r, MARGIN)
    j, _, _ = ref.nearest(ref.transform_f32(src, T), tgt)
    ok_m = ok & ok_t[j]
    print(f"mutual: {int((~ok_m).sum())} of {len(src)} source points excluded; reference rows {len(g16['m_mutual'])}")
    assert (~ok_m).mean() <= MAX_EXCLUDED
    assert np.array_equal(ref.rows_on(ref.mutual(src, tgt, T, T_inv, r), ok_m), ref.rows_on(g16["m_mutual"], ok_m))
    assert len(g16["m_mutual"]) > 1000


def test_restatement_tie_and_radius_rules():
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    assert np.array_equal(ref.one_side([[0.5, 0, 0], [0.25, 0, 0], [5, 5, 5]], t, None, 0.6), [[0, 0], [1, 0]])
    assert ref.one_side([[0.25, 0, 0]], t[:1], None, 0.25).shape == (0, 2)
    assert np.array_equal(ref.mutual([[0.1, 0, 0], [0.2, 0, 0]], t[:2], None, None, 0.5), [[0, 0]])
    assert ref.mutual([[9, 9, 9]], t, None, None, 0.5).shape == (0, 2)


def test_grid_points_equal_the_reference(g16):
    from umeregrobust_amd.utils.general_utils import convert_coords_to_grid_pts
    got = convert_coords_to_grid_pts(torch.from_numpy(g16["m_src"]), torch.from_numpy(g16["g_coords"]), float(g16["g_ds"]))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g16["g_grid"])


def test_rotation_and_augmented_ground_truth(g16):
    from umeregrobust_amd.datasets.kitti_dataset import augmented_gt_tform, z_rotation_matrix
    rng = np.random.RandomState(int(g16["item_seed"]))
    angles = [rng.uniform(low=-180, high=180), rng.uniform(low=-180, high=180)]
    assert np.array_equal(angles, g16["aug_angles"])
    rots = [torch.from_numpy(z_rotation_matrix(a)).float() for a in angles]
    assert np.array_equal(rots[0].numpy(), g16["aug_rot_src"]) and np.array_equal(rots[1].numpy(), g16["aug_rot_tgt"])
    assert np.array_equal(z_rotation_matrix(angles[0]), ref.z_rotation(angles[0]))
    got = augmented_gt_tform(torch.from_numpy(g16["item_gt_tform"]), rots[0], rots[1])
    assert float(np.abs(got.numpy() - g16["aug_gt_tform"]).max()) <= 1e-6


@pytest.mark.parametrize("name", ["kitti", "nuscenes"])
def test_config_takes_every_key_of_the_reference_file(name, tmp_path):
    import yaml
    from umeregrobust_amd import train_coloring as tc
    path = os.path.join(GOLDEN, f"train_{name}_config.yaml")
    keys = yaml.safe_load(open(path))
    args = tc.make_config(name, path)
    assert set(keys) == set(tc.DEFAULTS[name]), "the defaults must have exactly the reference's keys"
    for k, v in keys.items():
        assert getattr(args, k) == v, k
    # the built-in defaults ARE the reference's values, but for the two paths that were the authors' own
    for k, v in keys.items():
        if k != "data_path":
            assert tc.DEFAULTS[name][k] == v, k
    bad = tmp_path / "bad.yaml"
    bad.write_text("lr: 0.1\nlearning_rate: 0.1\n")
    with pytest.raises(KeyError, match="learning_rate"):
        tc.make_config(name, str(bad))
    assert tc.make_config(name, lr=0.5).lr == 0.5


def test_checkpoint_dictionary_and_file_name(tmp_path_factory):
    from umeregrobust_amd import train_coloring as tc
    tmp_path = tmp_path_factory.mktemp("run")         # (no "_checkpoint" in the directory's name: `resume` looks at the whole path)
    from umeregrobust_amd.datasets import checkpoint_state_dict
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=tc.WEIGHT_DECAY)
    model(torch.ones(1, 3)).sum().backward()
    opt.step()
    assert tc.checkpoint_file_name("best_total_loss.pth") == "best_total_loss_checkpoint.pth"
    assert tc.checkpoint_file_name("last_epoch.pth") == "last_epoch_checkpoint.pth"
    tc.save_checkpoint(7, 1.25, model, opt, str(tmp_path), "last_epoch.pth")
    tc.save_model(model, str(tmp_path), "weights.pth")
    assert sorted(os.listdir(tmp_path)) == ["last_epoch_checkpoint.pth", "weights.pth"]
    ck = torch.load(tmp_path / "last_epoch_checkpoint.pth", weights_only=True)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "total_loss"] and ck["epoch"] == 7 and ck["total_loss"] == 1.25
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in ck["model_state_dict"].items())
    assert ck["optimizer_state_dict"]["param_groups"][0]["weight_decay"] == 0.0
    assert sorted(checkpoint_state_dict(str(tmp_path / "last_epoch_checkpoint.pth"))) == sorted(model.state_dict())
    assert sorted(torch.load(tmp_path / "weights.pth", weights_only=True)) == sorted(model.state_dict())
    # resume: START_EPOCH is the stored epoch (the saved epoch runs again)
    m2 = torch.nn.Linear(3, 2)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3)
    assert tc.resume(str(tmp_path / "last_epoch_checkpoint.pth"), m2, o2, "cpu") == 7
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), model.state_dict().values()))
    assert tc.resume(str(tmp_path / "weights.pth"), m2, o2, "cpu") == 0
