"""Write the pair cache from raw scans: the reference's `datasets/sem_preprocessing.py` with the scans prepared on the GPU.

    python -m umeregrobust_amd.datasets.sem_preprocessing --data_path <sequences> --output_path <cache> --split train \\
        --dataset_mode kitti --metadata_dir <dir with train_metadata.npy> --label_config <kitti_config.yaml> --nksr False

The reference's arguments, defaults and output paths (`<output_path>/<split>/<seq>/<frame0:06d>_<frame1:06d>.pickle`, the nine
keys of `write_cached_pair`); a file that exists is skipped.  Added: `--metadata_dir`, `--label_config` (what the reference reads
relative to its working directory) and `--completion module:function`, the `completion_fn(pts) -> new_pts` that stands where the
reference calls NKSR.  `--nksr` keeps the reference's default, True: without a completion the command then stops with a message
rather than write clouds that were not equalised under the command line that promises them.  Values the reference parses with
`eval` (`--nksr`, `--convert_points_to_grid`, `--range_idxs`) are read as Python literals."""
import argparse
import ast
import importlib
import os
import sys


def _named_function(spec):
    module, _, name = spec.partition(":")
    if not module or not name:
        raise argparse.ArgumentTypeError(f"--completion takes module:function, got {spec!r}")
    return getattr(importlib.import_module(module), name)


def make_parser():
    parser = argparse.ArgumentParser(prog="python -m umeregrobust_amd.datasets.sem_preprocessing", description=__doc__.split("\n")[0])
    parser.add_argument("--data_path", type=str, default="")
    parser.add_argument("--output_path", type=str, default="")
    parser.add_argument("--split", type=str, default="train", choices=["train", "test", "val"])
    parser.add_argument("--nksr", type=ast.literal_eval, default=True)
    parser.add_argument("--dataset_mode", type=str, default="kitti", choices=["kitti", "nuscenes"])
    parser.add_argument("--convert_points_to_grid", type=ast.literal_eval, default=True)
    parser.add_argument("--voxel_size", type=float, default=0.3)
    parser.add_argument("--range_idxs", type=ast.literal_eval, default=[])
    parser.add_argument("--metadata_dir", type=str, default=None, help="directory with <split>_metadata.npy and <split>_gt_tforms.npy")
    parser.add_argument("--label_config", type=str, default=None, help="kitti: the dataset's yaml with its learning_map")
    parser.add_argument("--completion", type=_named_function, default=None, metavar="module:function",
                        help="completion_fn(pts) -> new_pts, used when --nksr is True")
    return parser


def main(argv=None):
    """-> (files written, files skipped)"""
    from .kitti_dataset import write_cached_pair
    from .raw_pair_datasets import NuscenesDataset, SemanticKITTIDataset
    args = make_parser().parse_args(argv)
    common = dict(data_path=args.data_path, split=args.split, use_pc_completion=args.nksr, skip_invalid_entries=False,
                  convert_points_to_grid=args.convert_points_to_grid, voxel_size=args.voxel_size, metadata_dir=args.metadata_dir,
                  completion_fn=args.completion)
    if args.dataset_mode == "nuscenes":
        dset = NuscenesDataset(**common)
    else:
        dset = SemanticKITTIDataset(label_config=args.label_config, **common)
    range_vals = range(len(dset)) if args.range_idxs == [] else range(args.range_idxs[0], args.range_idxs[1])
    written = skipped = 0
    for itr in range_vals:
        seq_id, frame0_id, frame1_id = dset.files[itr]
        save_dir_path = os.path.join(args.output_path, args.split, seq_id if args.dataset_mode == "nuscenes" else f"{seq_id:02d}")
        save_path = os.path.join(save_dir_path, f"{frame0_id:06d}_{frame1_id:06d}.pickle")
        if os.path.isfile(save_path):
            print(f"{save_path} - EXIST (Skip)")
            skipped += 1
            continue
        write_cached_pair(save_path, dset[itr])
        written += 1
    print(f"{written} written, {skipped} skipped")
    return written, skipped


if __name__ == "__main__":
    main(sys.argv[1:])
