#!/usr/bin/env python3
"""Golden samples of HeadNet's training data, produced by running the reference's own ARESHeadPoseDataset
(egoego/data/ares_headpose_dataset.py, unmodified) on the CPU over a six-sequence tree this script writes to a temporary folder.

Runs only in the authoring container (the reference checkout present), with the stand-ins of make_stage1_golden.install_stubs()
for the modules the reference imports and this image lacks.  Window 4, D = 12; sequences of T = 6, 5, 4 (dropped by the filter),
9 (with a SLAM track of 7 rows), 8 and 7 (no SLAM file: dropped); the T = 5 sequence has a track of 8 rows, longer than itself.
Recorded, with their dtypes: the tree's arrays; per kept sequence the six whole SLAM arrays the dataset holds; every array of
every item, for_eval off (two passes, `random` seeded, every random.sample result recorded) and on.  The script asserts that
tests/head_batch_oracle.py reproduces each item bit for bit from the recorded start.

    python tests/golden/make_head_batch_golden.py
"""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

WINDOW, D = 4, 12
SRC = "/viscam/u/jiamanli/datasets/egomotion_syn_dataset/habitat_rendering_replica_all"   # the root the motion file records
# name -> (T, rows of the SLAM track or None)
TREE = {"apartment_0-seq_a": (6, 6), "apartment_0-seq_b": (5, 8), "room_1-seq_c": (4, 4), "room_1-seq_d": (9, 7),
        "office_2-seq_e": (8, 8), "office_2-seq_f": (7, None)}


def unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def write_tree(root):
    """-> {name: {head_qpos fp32, head_vels fp64, of_feats fp32, slam fp64 or None}} as written under root/data."""
    import joblib
    g = np.random.default_rng(20)
    seqs, motion = {}, {}
    for k, (name, (T, L)) in enumerate(TREE.items()):
        scene, rest = name.split("-")[0], "-".join(name.split("-")[1:])
        qpos = np.concatenate([np.cumsum(g.normal(0, 0.02, (T, 3)), 0) + [0, 0, 1.6], unit(g.normal(size=(1, 4)) + np.cumsum(
            g.normal(0, 0.05, (T, 4)), 0))], 1).astype(np.float32)
        vels = g.normal(0, 0.3, (T, 6))
        vels[-1] = vels[-2]                                            # the cloned last row the dataset removes
        feats = g.normal(size=(T - 1, D)).astype(np.float32)
        files = []
        for t in range(T - 1):
            rec = f"{SRC}/{scene}/{rest}/raft_flows/{t:05d}.npy"
            files.append(rec)
            real = rec.replace(os.path.dirname(SRC), os.path.join(root, "data", "ares")).replace("raft_flows", "raft_of_feats")
            os.makedirs(os.path.dirname(real), exist_ok=True)
            np.save(real, feats[t])
        slam = None
        if L is not None:
            slam = np.concatenate([np.cumsum(g.normal(0, 0.05, (L, 3)), 0) + g.normal(size=(1, 3)),
                                   unit(g.normal(size=(1, 4)) + np.cumsum(g.normal(0, 0.05, (L, 4)), 0))], 1)
            path = os.path.join(root, "data", "ares", "droid_slam_res", scene, rest + ".npy")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, slam)
        motion[k] = {"seq_name": name, "head_qpos": qpos, "head_vels": vels, "of_files": files}
        seqs[name] = {"head_qpos": qpos, "head_vels": vels, "of_feats": feats, "slam": slam}
    os.makedirs(os.path.join(root, "data", "ares_egoego_processed"), exist_ok=True)
    for split in ("train", "test"):
        joblib.dump(motion, os.path.join(root, "data", "ares_egoego_processed", f"{split}_ares_smplh_motion.p"))
    return seqs


def main():
    from make_stage1_golden import install_stubs
    install_stubs()
    from egoego.data.ares_headpose_dataset import ARESHeadPoseDataset
    import head_batch_oracle as O

    rec = {"window": np.int64(WINDOW), "names": np.array(list(TREE))}
    with tempfile.TemporaryDirectory() as root:
        seqs = write_tree(root)
        for name, s in seqs.items():
            for k, v in s.items():
                if v is not None:
                    rec[f"seq/{name}/{k}"] = v
        cwd = os.getcwd()
        os.chdir(root)  # the reference reads the feature files under the relative path data/ares
        try:
            draws = []
            sample = random.sample

            def recording_sample(population, k):
                got = sample(population, k)
                draws.append((len(population), got[0]))
                return got

            random.sample = recording_sample
            random.seed(7)
            for mode, for_eval, passes in (("train", False, 2), ("eval", True, 1)):
                ds = ARESHeadPoseDataset("data", train=True, window=WINDOW, for_eval=for_eval)
                kept = [ds.data_dict[i]["seq_name"] for i in range(len(ds))]
                assert kept == ["apartment_0-seq_a", "apartment_0-seq_b", "room_1-seq_d", "office_2-seq_e"], kept
                rec["kept"] = np.array(kept)
                whole = {}
                for i, name in enumerate(kept):
                    whole[name] = dict(seqs[name], **{k: ds.data_dict[i][k] for k in O.SLAM_KEYS})
                    for k in O.SLAM_KEYS:
                        rec[f"seq/{name}/{k}"] = np.asarray(ds.data_dict[i][k])
                j = 0
                for _ in range(passes):
                    for i, name in enumerate(kept):
                        del draws[:]
                        q = ds[i]
                        F = len(seqs[name]["head_qpos"]) - 1
                        if for_eval:
                            assert not draws
                            start = 0
                        else:
                            assert len(draws) == 1 and draws[0][0] == F - WINDOW + 1
                            start = draws[0][1]
                        assert q["seq_name"] == name
                        n = int(q["seq_len"])
                        assert (start, n) == O.window_of(F, F if for_eval else WINDOW, for_eval, start)
                        want = O.item(whole[name], start, n)
                        P = f"{mode}/{j}/"
                        rec[P + "seq"], rec[P + "start"], rec[P + "seq_len"] = np.array(name), np.int64(start), np.int64(n)
                        for k, w in want.items():
                            if k == "seq_len":
                                continue
                            a = np.asarray(q[k])
                            assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == np.ascontiguousarray(w).tobytes(), (P, k)
                            rec[P + k] = a
                        assert sorted(k for k in q if k != "seq_name") == sorted(want)
                        j += 1
                rec[f"{mode}/count"] = np.int64(j)
            random.sample = sample
        finally:
            os.chdir(cwd)
    out = os.path.join(HERE, "head_batch_golden.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes;", {k: str(v.dtype) for k, v in rec.items() if k.startswith("eval/0/")})


if __name__ == "__main__":
    main()
