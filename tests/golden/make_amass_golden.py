#!/usr/bin/env python3
"""Golden records of the AMASS preprocessing, produced by running the reference's own process_seq
(utils/data_utils/process_amass_dataset.py:340-493), unmodified, on the CPU.

Runs only where the reference checkout is present ($EGOEGO_REFERENCE, default /root/reference).  What executes is the reference's
Python, unmodified, on temporary .npz files this script writes.  Not the reference's:

  get_body_model_sequence   (human_body_prior's SMPL-H and the licensed model files are absent) is replaced by one that returns Jtr
                            from tests/body_oracle.py on synthetic.make_body_model, fp64 rounded once to float32, and the first 22
                            entries of that model's kintree_table;
  pytorch3d.transforms      the scipy stand-ins of make_window_loop_golden.py;
  everything else its file imports and process_seq never reaches: the stub list of make_eval_golden.py.

Inputs: synthetic.make_eval_motion(1, T, seed, fps=..., check=False) as 66 pose columns and a translation, float32 values handed
over as float64.  One sequence each: kept at 120, 60 and 30 fps; the 240-fps and the 59-fps path corrections; a terrain discard;
a too-short sequence.  The file holds inputs and recorded results only.  The script asserts the conditions that make an exact
comparison no coin toss (synthetic.assert_eval_margins on the trimmed raw joints at the sequence's fps; consecutive output head
rotations identical or >= 0.008 rad apart; |w| >= 0.5; heading norm >= 0.5), that tests/amass_oracle.py reproduces the discrete
results exactly, and prints how far the reference's float32 results lie from the fp64 oracle, per key.

    python tests/golden/make_amass_golden.py
"""
import glob
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
OUT = os.path.join(HERE, "amass_golden.npz")
MODEL = dict(seed=0, n_verts=512, n_faces=64)  # Jtr depends on the vertices only through J_regressor: a small mesh will do
# name -> (directory the file sits in, T, seed, the labelled mocap_framerate, what happens)
SEQUENCES = {
    "kept_120": ("ACCAD/s1", 240, 5, 120.0, "kept"),
    "kept_60": ("CMU/s2", 200, 4, 60.0, "kept"),
    "kept_30": ("SFU/s3", 100, 3, 30.0, "kept"),
    "handball_240": ("BMLhandball/S01_Expert", 320, 4, 120.0, "kept"),
    "mislabeled_59": ("KIT/20160930_50032", 150, 5, 60.0, "kept"),
    "terrain": ("HumanEva/s4", 500, 0, 120.0, "terrain"),
    "short": ("MPI_mosh/s5", 100, 1, 120.0, "short"),
}


def load_reference(tr):
    import make_eval_golden
    make_eval_golden.install_stubs()
    sys.modules["pytorch3d.transforms"] = tr
    sys.modules["pytorch3d"].transforms = tr
    from utils.data_utils import process_amass_dataset as P
    P.transforms = tr
    return P


def main():
    import amass_oracle as O
    import body_oracle
    import make_window_loop_golden as W
    from egoego_release_amd import synthetic as S
    from sklearn.cluster import DBSCAN

    P = load_reference(W.transforms_module())
    model = S.make_body_model(**MODEL)
    recorded = []

    class RecordingDBSCAN(DBSCAN):
        def fit(self, X, *a, **k):
            r = super().fit(X, *a, **k)
            recorded.append(self.labels_.copy())
            return r

    class Body:
        pass

    def get_body_model_sequence(smplh_path, gender, num_frames, pose_body, pose_hand, betas, root_orient, trans):
        assert str(gender) == "male" and not np.any(betas)
        f32 = lambda a: np.asarray(torch.Tensor(a))  # noqa: E731  (the rounding of :151-156)
        pose = np.concatenate([f32(root_orient), f32(pose_body)], 1).reshape(num_frames, 22, 3)
        out = body_oracle.forward(model, pose, f32(trans), np.zeros((num_frames, 16)), dtype=torch.float64)
        body = Body()
        body.Jtr = out["Jtr"].float()
        body.v = torch.zeros(num_frames, 1, 3)
        kintree = np.asarray(model["kintree_table"])[0, :22].astype(np.int64)
        kintree[0] = -1
        return body, kintree

    P.DBSCAN = RecordingDBSCAN
    P.get_body_model_sequence = get_body_model_sequence
    P.print = lambda *a, **k: None

    out = {"names": np.array(list(SEQUENCES)), "model": np.array([MODEL["seed"], MODEL["n_verts"], MODEL["n_faces"]])}
    worst = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (folder, T, seed, fps, expect) in SEQUENCES.items():
            m = S.make_eval_motion(1, T, seed, fps=fps, check=False)
            poses, trans = m["local_aa"][0].reshape(T, 66), m["root_trans"][0]
            os.makedirs(os.path.join(tmp, "in", folder), exist_ok=True)
            os.makedirs(os.path.join(tmp, "out", folder), exist_ok=True)
            path_in = os.path.join(tmp, "in", folder, name + "_poses.npz")
            path_out = os.path.join(tmp, "out", folder, name + "_poses.npz")
            np.savez(path_in, poses=poses.astype(np.float64), trans=trans.astype(np.float64), mocap_framerate=np.float64(fps),
                     gender="female", betas=np.ones(16))
            rel_path = os.path.join(folder, name + "_poses.npz")
            out[name + "/path"], out[name + "/poses"], out[name + "/trans"] = np.array(rel_path), poses, trans
            out[name + "/mocap_framerate"] = np.float64(fps)

            recorded.clear()
            P.process_seq((path_in, path_out, "unused"))
            files = glob.glob(path_out[:-4] + "*.npz")
            rec, info = O.process_seq(model, rel_path, poses.astype(np.float64), trans.astype(np.float64), np.float64(fps))
            what = "kept" if isinstance(rec, dict) else rec
            assert what == expect and len(files) == (what == "kept"), (name, what, files)
            out[name + "/result"] = np.array(what)
            if what == "short":
                assert not recorded
                print(f"{name:14s} short")
                continue
            real_fps = O.corrected_fps(rel_path, fps)
            S.assert_eval_margins(info["raw_joints"], real_fps)
            assert np.array_equal(info["fc"]["labels"], recorded[0]), name
            out[name + "/labels"] = recorded[0].astype(np.int32)
            if what == "terrain":
                print(f"{name:14s} terrain  raw frames {info['raw_joints'].shape[0]}  n_static {recorded[0].size}")
                continue
            O.assert_head_conditions(info["head"])
            z = np.load(files[0])
            assert os.path.basename(files[0]) == name + "_poses_%d_frames_%d_fps.npz" % (rec["trans"].shape[0], int(rec["fps"]))
            assert tuple(z.files) == O.RECORD_KEYS
            for k in O.RECORD_KEYS:
                a = z[k]
                out[name + "/dtype/" + k] = np.array(str(a.dtype))
                out[name + "/ref/" + k] = a.astype(np.uint8) if k == "contacts" else a
            for k in ("fps", "floor_height", "contacts", "trans", "root_orient", "pose_body", "betas"):
                assert np.array_equal(z[k], np.asarray(rec[k])), (name, k)
            assert z["floor_height"].dtype == np.float32 and str(z["gender"]) == "male"
            same = np.append(info["head"]["same"], info["head"]["same"][-1])
            for k in O.CONTINUOUS_KEYS:
                assert z[k].shape == np.asarray(rec[k]).shape, (name, k)
                worst[k] = max(worst.get(k, 0.0), O.rel_diff(z[k], rec[k]))
            # a pair's branch shows in the reference's own rows: axis * 0 gives exact zeros
            assert np.array_equal(np.all(z["head_vels"][:, 3:] == 0, 1), same), name
            ang, w, hn = O.head_conditions(info["head"])
            print(f"{name:14s} kept  raw {info['raw_joints'].shape[0]:4d} -> {rec['trans'].shape[0]:3d} frames at {int(rec['fps'])} fps  floor "
                  f"{float(rec['floor_height']):+.6f}  head step >= {ang:.4f} rad  |w| >= {w:.3f}  heading >= {hn:.3f}  head_vels {z['head_vels'].dtype}")
    print("reference (float32 arithmetic) vs the fp64 oracle, worst relative difference per key:")
    print("REFERENCE_DISTANCE = {" + ", ".join(f'"{k}": {v:.3e}' for k, v in worst.items()) + "}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
