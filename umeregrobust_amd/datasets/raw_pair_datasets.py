"""The reference's two pair datasets under their own names, `SemanticKITTIDataset` (datasets/kitti/kitti_dataset.py:317-543) and
`NuscenesDataset` (datasets/nuscenes/nuscenes_dataset.py:315-550): the pair list from the metadata files, items from the pair
cache (`cache_data_path != ""`: what `CachedPairDataset` serves, augmentation included) or, without a cache, made from the raw
scans on the GPU (`raw_scan.prepare_cloud` / `prepare_pair`), which is how the cache is written in the first place
(`python -m umeregrobust_amd.datasets.sem_preprocessing`).

Constructor arguments are the reference's, in its order; what it reads relative to its working directory is named here by
keyword: `metadata_dir` (the directory with `{split}_metadata.npy` and `{split}_gt_tforms.npy`), and for SemanticKITTI
`label_config` (a yaml with the dataset's `learning_map`; the map is the dataset's and is not shipped with this package).
`completion_fn(pts) -> new_pts` stands where the reference calls NKSR (`use_pc_completion=True`)."""
import os

import numpy as np
import torch

from .kitti_dataset import CachedPairDataset, _refuse_gpu_in_worker


class _RawPairDataset(CachedPairDataset):
    IN_VALID_IDXS = {}
    KIND = None              # "kitti" | "nuscenes": how CachedPairDataset names the sequence directory
    MAX_TRANSLATION = None   # KITTI: pairs further apart than this are left out (kitti_dataset.py:354-356)

    def __init__(self, data_path, split, voxel_size=0.3, use_pc_completion=False, cache_data_path="", dataset_size=-1,
                 use_augmentations=False, convert_points_to_grid=True, skip_invalid_entries=True, overied_cache=False, *,
                 metadata_dir=None, label_config=None, device=None, completion_fn=None, rng=np.random, items_on_device=False):
        if metadata_dir is None:
            raise ValueError(f"{type(self).__name__}: metadata_dir= must name the directory that holds {split}_metadata.npy and "
                             f"{split}_gt_tforms.npy (the reference's datasets/{self.KIND}/metadata)")
        self.data_path, self.use_pc_completion = data_path, bool(use_pc_completion)
        self.convert_points_to_grid, self.skip_invalid_entries = convert_points_to_grid, skip_invalid_entries
        self.completion_fn, self.label_config, self._lut = completion_fn, label_config, None
        files = np.load(os.path.join(metadata_dir, f"{split}_metadata.npy")).tolist()
        gt_tforms = np.load(os.path.join(metadata_dir, f"{split}_gt_tforms.npy"))
        if self.MAX_TRANSLATION is not None:
            near = np.linalg.norm(gt_tforms[:, :3, 3], axis=-1) <= self.MAX_TRANSLATION
            files, gt_tforms = np.array(files)[near].tolist(), gt_tforms[near]
        if skip_invalid_entries and cache_data_path != "":                    # pairs without matches
            valid = np.setdiff1d(np.arange(len(files)), np.array(self.IN_VALID_IDXS[split]))
            files, gt_tforms = np.array(files)[valid].tolist(), gt_tforms[valid]
        if overied_cache:
            cache_data_path = ""
        files = [self._entry(e) for e in files]
        if dataset_size != -1:
            files, gt_tforms = files[:dataset_size], gt_tforms[:dataset_size]
        self.gt_tforms = gt_tforms
        if self.use_pc_completion and completion_fn is None and cache_data_path == "":
            from ..raw_scan import completion_missing
            raise completion_missing()
        super().__init__(cache_data_path, split=split, files=files, dataset=self.KIND, use_augmentations=use_augmentations,
                         voxel_size=voxel_size, device=device, rng=rng, items_on_device=items_on_device)

    @staticmethod
    def _entry(e):
        return e

    def __getitem__(self, idx):
        if self.cache_data_path != "":
            return super().__getitem__(idx)
        return self.preprocess_getitem(idx)

    def load_cloud(self, seq_id, frame_id, device, keep_unlabeled):
        raise NotImplementedError

    def preprocess_getitem(self, idx, phase=None):
        """The item made from the two raw scans, on the GPU -> the 9-tuple (on the host unless items_on_device)."""
        from .. import raw_scan
        who = f"{type(self).__name__} without a cache"
        _refuse_gpu_in_worker(who)
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who} prepares the scans on the GPU; there is no HIP device and no CPU fallback")
        device = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        seq_id, frame0_id, frame1_id = self.files[idx]
        clouds = []
        for frame_id in (frame0_id, frame1_id):
            pts, seg = self.load_cloud(seq_id, frame_id, device, keep_unlabeled=self.use_pc_completion)
            if self.use_pc_completion:
                pts, seg = raw_scan.complete_cloud(pts, seg, self.completion_fn, self.LABEL_COPY_DIST_THR)
                pts, seg = raw_scan.drop_unlabeled(pts, seg)
            clouds.append((pts, seg))
        gt_tform = torch.from_numpy(self.gt_tforms[idx]).float()
        return raw_scan.prepare_pair(clouds[0], clouds[1], gt_tform, self.voxel_size, self.convert_points_to_grid,
                                     to_host=not self.items_on_device, phase=phase)


class SemanticKITTIDataset(_RawPairDataset):
    """Registration pairs of SemanticKITTI: `<data_path>/<seq:02d>/velodyne/<frame:06d>.bin` and `.../labels/<frame:06d>.label`."""
    LABEL_COPY_DIST_THR = 3
    IN_VALID_IDXS = {"train": [489, 3770, 5132, 5184, 7559, 9080, 9344, 11627], "val": [623], "test": [9], "lokitti": [241, 392, 530],
                     "rotkitti": [394, 441]}
    KIND = "kitti"
    MAX_TRANSLATION = 50

    def learning_map(self):
        if self._lut is None:
            if self.label_config is None:
                raise ValueError("SemanticKITTIDataset: reading raw scans needs label_config= (the dataset's yaml with its `learning_map`, "
                                 "the reference's datasets/kitti/kitti_config.yaml)")
            from ..raw_scan import load_learning_map
            self._lut = load_learning_map(self.label_config)
        return self._lut

    def load_cloud(self, seq_id, frame_id, device, keep_unlabeled=False):
        """`load_semantic_kitti_point_cloud` (kitti_dataset.py:300-314) and the unlabelled mask, on the device"""
        from .. import raw_scan
        scan = raw_scan.read_kitti_scan(os.path.join(self.data_path, f"{seq_id:02d}", "velodyne", f"{frame_id:06d}.bin"))
        labels = raw_scan.read_kitti_label(os.path.join(self.data_path, f"{seq_id:02d}", "labels", f"{frame_id:06d}.label"), len(scan))
        return raw_scan.prepare_cloud(scan, labels, lut=self.learning_map(), sem16=True, keep_unlabeled=keep_unlabeled, device=device)


class NuscenesDataset(_RawPairDataset):
    """Registration pairs of nuScenes exported in the KITTI layout: `<data_path>/<split>/sequences/<seq>/velodyne/<frame:06d>.bin`,
    labels `.../labels/<frame:06d>.npy` where they exist.  Sequence ids are strings; `rotnuscenes` reads the `test` directory."""
    LABEL_COPY_DIST_THR = 3
    IN_VALID_IDXS = {"train": [], "val": [], "test": [], "rotnuscenes": [], "lonuscenes": []}
    KIND = "nuscenes"

    velo_data_type = "bin"   # what `preprocess_getitem` reads (the reference's default); set "npy" on an instance for exported arrays

    @staticmethod
    def _entry(e):
        return (e[0].__str__(), int(e[1]), int(e[2]))                         # nuscenes_dataset.py:368

    def load_cloud(self, seq_id, frame_id, device, keep_unlabeled=False):
        """`load_nuscenes_point_cloud` (nuscenes_dataset.py:294-312), the ego box (:403-409) and the unlabelled mask, on the device"""
        from .. import raw_scan
        actual_split = "test" if self.split == "rotnuscenes" else self.split    # :390
        scan, labels = raw_scan.read_nuscenes_cloud(self.data_path, actual_split, seq_id, frame_id, self.velo_data_type)
        return raw_scan.prepare_cloud(scan, labels, ego_box=raw_scan.NUSCENES_EGO_BOX, keep_unlabeled=keep_unlabeled, device=device)
