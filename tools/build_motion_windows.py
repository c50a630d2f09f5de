#!/usr/bin/env python3
"""Raw SMPL-H motion -> the stage-2 window files and statistics the reference's AMASSDataset caches
(egoego/data/amass_diffusion_dataset.py:204-231), on the GPU, with the reference's names and joblib layouts:

    python tools/build_motion_windows.py --data train_amass_smplh_motion.p [--test_data test_amass_smplh_motion.p] \\
        --body_model smpl_models/smplh_amass --window 120 --out processed/

  --data          the training split: a joblib / pickle dict {k: {'seq_name', 'trans' [T,3], 'root_orient' [T,3], 'body_pose' [T,63], ...}}
  --test_data     optionally the test split, in the same layout
  --body_model    the SMPL-H model directory (<dir>/male/model.npz): the rest offsets come from it; or
  --rest_offsets  an .npy [22,3] of them
  --window        frames per window (120)
  --no_canonicalize   the reference's other branch: no heading canonicalisation (files without the cano_ prefix)
  --out           output directory

Writes <cano_>train_diffusion_amass_window_<W>.p (and <cano_>test_... with --test_data), <cano_>min_max_mean_std_data_window_<W>.p
(from the training split) and rest_offsets.npy.  tools/run_stage2_demo.py and tools/run_egoego_demo.py take the last two as
--stats and --rest_offsets as they are.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_any(path):
    try:
        import joblib
        return joblib.load(path)
    except Exception:
        with open(path, "rb") as f:
            return pickle.load(f)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--data", required=True)
    p.add_argument("--test_data")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--body_model")
    src.add_argument("--rest_offsets")
    p.add_argument("--window", type=int, default=120)
    p.add_argument("--no_canonicalize", action="store_true")
    p.add_argument("--out", required=True)
    opt = p.parse_args(argv)
    import joblib
    from egoego_release_amd import motion_data as MD

    if opt.rest_offsets:
        rest = np.load(opt.rest_offsets).astype(np.float32).reshape(22, 3)
    else:
        from egoego_release_amd.body import BodyModel
        rest = MD.rest_pose_offsets(BodyModel(bm_fname=os.path.join(opt.body_model, "male", "model.npz"))).cpu().numpy()
    os.makedirs(opt.out, exist_ok=True)
    prefix = "" if opt.no_canonicalize else "cano_"
    report = {"window": opt.window, "canonicalize_init_head": not opt.no_canonicalize, "files": []}

    def dump(obj, name):
        path = os.path.join(opt.out, name)
        joblib.dump(obj, path)
        report["files"].append(path)

    np.save(os.path.join(opt.out, "rest_offsets.npy"), rest)
    report["files"].append(os.path.join(opt.out, "rest_offsets.npy"))
    for split, path in (("train", opt.data), ("test", opt.test_data)):
        if path is None:
            continue
        mw = MD.build_motion_windows(load_any(path), rest, window=opt.window, canonicalize_init_head=not opt.no_canonicalize)
        dump(mw.to_window_data_dict(), f"{prefix}{split}_diffusion_amass_window_{opt.window}.p")
        report[split + "_windows"] = len(mw)
        if split == "train":
            dump(mw.stats(), f"{prefix}min_max_mean_std_data_window_{opt.window}.p")
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
