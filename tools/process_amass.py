#!/usr/bin/env python3
"""Raw AMASS -> the per-sequence files and the stage-2 motion files of the reference's
utils/data_utils/process_amass_dataset.py, on the GPU, under the reference's names:

    python tools/process_amass.py --amass_root data/amass --body_model smpl_models/smplh_amass --out data/processed_amass

  --amass_root   the raw AMASS tree: <root>/<dataset>/<subject>/*_poses.npz (poses, trans, mocap_framerate)
  --body_model   the SMPL-H model directory (<dir>/male/model.npz; every sequence uses the male skeleton at zero betas, as the
                 reference forces)
  --datasets     which datasets to process (default: every directory under --amass_root)
  --chunk_frames raw frames per GPU pass
  --out          output directory

Writes <out>/<dataset>/<subject>/<file>_<N>_frames_<fps>_fps.npz per kept sequence (the arguments of np.savez at :477-491), and
<out>/amass_smplh_motion.p, train_amass_smplh_motion.p and test_amass_smplh_motion.p (joblib, :495-588; sequences in sorted
order where the reference takes os.listdir's).  tools/build_motion_windows.py --data takes the last two as they are.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--amass_root", required=True)
    p.add_argument("--body_model", required=True)
    p.add_argument("--datasets", nargs="+")
    p.add_argument("--chunk_frames", type=int, default=None)
    p.add_argument("--out", required=True)
    opt = p.parse_args(argv)
    import joblib
    from egoego_release_amd import amass_prep as A
    from egoego_release_amd.body import BodyModel

    bm = BodyModel(bm_fname=os.path.join(opt.body_model, "male", "model.npz"))
    datasets = opt.datasets or sorted(d for d in os.listdir(opt.amass_root) if d[0] != "." and os.path.isdir(os.path.join(opt.amass_root, d)))
    report = {"sequences": 0, "kept": 0, "short": 0, "terrain": 0, "frames": 0, "files": []}
    data = {}
    for ds in datasets:
        files = sorted(glob.glob(os.path.join(opt.amass_root, ds, "*", "*_poses.npz")))
        seqs = []
        for f in files:
            with np.load(f) as z:
                seqs.append({"path": f, "poses": z["poses"], "trans": z["trans"], "mocap_framerate": z["mocap_framerate"]})
        kw = {} if opt.chunk_frames is None else {"chunk_frames": opt.chunk_frames}
        results = A.process_sequences(seqs, bm, **kw) if seqs else []
        for f, r in zip(files, results):
            report["sequences"] += 1
            if not isinstance(r, dict):
                report[r] += 1
                continue
            subject, stem = os.path.basename(os.path.dirname(f)), os.path.basename(f)[:-4]
            os.makedirs(os.path.join(opt.out, ds, subject), exist_ok=True)
            name = A.record_file_name(stem, r)
            np.savez(os.path.join(opt.out, ds, subject, name), **r)
            with np.load(os.path.join(opt.out, ds, subject, name)) as z:  # what prep_smpl_to_single_data reads back (:514)
                data["-".join((ds, subject, name))] = {k: z[k] for k in z.files}
            report["kept"] += 1
            report["frames"] += int(r["trans"].shape[0])
    os.makedirs(opt.out, exist_ok=True)
    data = A.collect(data)
    train, test = A.split(data)
    for name, obj in (("amass_smplh_motion.p", data), ("train_amass_smplh_motion.p", train), ("test_amass_smplh_motion.p", test)):
        joblib.dump(obj, os.path.join(opt.out, name))
        report["files"].append(os.path.join(opt.out, name))
    report["train"], report["test"] = len(train), len(test)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
