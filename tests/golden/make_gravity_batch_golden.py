#!/usr/bin/env python3
"""Golden vectors of GravityNet's training samples, produced by running the reference's own AMASSHeadPoseDataset.__getitem__
(egoego/data/amass_headpose_dataset.py:115-165, with augment_traj :38-76 and divide_train_val :78-103) on the CPU.

Runs only in the authoring container (the reference checkout present).  What executes is the reference's Python, unmodified.  Not
the reference's (absent from this image): pytorch3d.transforms, installed by make_stage1_golden.install_stubs() and given two
stand-ins here whose bodies are pytorch3d's published formulas in torch: quaternion_to_matrix, and random_rotation (four normals o,
q = o / copysign(|o|, o_0), quaternion_to_matrix(q)), which also records the quaternion it returns.  `random`, `np.random` and torch
are seeded; the start (random.sample) and the scale (np.random.uniform) of every sample are recorded on their way through.

window = 16; sequences of 31 frames (kept by the split), 30 (dropped by it), 17, 18 and 19 (dropped too, and injected past the split
so that __getitem__ sees len - window - 1 of 0, 1 and 2) and 40 (a validation name); for_eval off and on.  The script asserts that
tests/gravity_batch_oracle.py's "ref32" mode reproduces every recorded tensor bit for bit from the recorded draws, and writes
tests/golden/gravity_batch_golden.npz.

    python tests/golden/make_gravity_batch_golden.py
"""
import os
import random
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

WINDOW = 16
SEQS = (("CMU-01_31", 31), ("KIT-02_30", 30), ("ACCAD-03_17", 17), ("EKUT-04_18", 18), ("BMLmovi-05_19", 19), ("SFU-06_40", 40))
INJECTED = ("ACCAD-03_17", "EKUT-04_18", "BMLmovi-05_19")
OUT = os.path.join(HERE, "gravity_batch_golden.npz")
TENSORS = ("ori_head_pose", "head_rot_mat", "head_trans", "aligned_rot_mat", "floor_normal")


def make_sequences():
    g = np.random.default_rng(20240)
    out = {}
    for name, n in SEQS:
        trans = np.cumsum(g.normal(0.0, 0.02, (n, 3)), 0) + g.normal(0.0, 1.0, (1, 3)) + np.array([0.0, 0.0, 1.6])
        q = g.normal(0.0, 1.0, (1, 4)) + np.cumsum(g.normal(0.0, 0.05, (n, 4)), 0)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        out[name] = {"head_pose": np.concatenate([trans, q], 1).astype(np.float32)}
    return out


def quaternion_to_matrix(quaternions):
    r, i, j, k = torch.unbind(quaternions, -1)
    two_s = 2.0 / (quaternions * quaternions).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(quaternions.shape[:-1] + (3, 3))


def main():
    import make_stage1_golden as S1
    S1.install_stubs()
    import pytorch3d.transforms as tr
    import gravity_batch_oracle as O

    rec = {}

    def random_rotation():
        o = torch.randn((1, 4))
        s = (o * o).sum(1)
        q = o / torch.where((o[:, 0] < 0), -torch.sqrt(s), torch.sqrt(s))[:, None]
        rec["normals"], rec["quat"] = o[0].numpy().copy(), q[0].numpy().copy()
        return quaternion_to_matrix(q)[0]

    tr.quaternion_to_matrix, tr.random_rotation = quaternion_to_matrix, random_rotation
    import egoego.data.amass_headpose_dataset as DS

    class Random:  # the module's `random`: the same draws, recorded
        @staticmethod
        def sample(population, k):
            got = random.sample(population, k)
            rec["start"] = int(got[0])
            return got

    DS.random = Random
    uniform = np.random.uniform

    def recording_uniform(*a, **kw):
        got = uniform(*a, **kw)
        rec["scale"] = float(np.asarray(got).reshape(-1)[0])
        return got

    np.random.uniform = recording_uniform
    seqs = make_sequences()
    out = {"window": np.int64(WINDOW), "names": np.array([n for n, _ in SEQS])}
    for name in seqs:
        out[f"pose/{name}"] = seqs[name]["head_pose"]
    worst = 0
    with tempfile.TemporaryDirectory() as folder:
        for for_eval in (False, True):
            random.seed(7)
            np.random.seed(8)
            torch.manual_seed(9)
            split = {}
            for train in (True, False):
                ds = DS.AMASSHeadPoseDataset(seqs, folder, train=train, window=WINDOW, for_eval=for_eval)
                split[train] = [ds.data_dict[k] for k in range(len(ds))]
            out["split_train"], out["split_val"] = np.array(split[True]), np.array(split[False])
            assert split[True] == ["CMU-01_31"] and split[False] == ["SFU-06_40"], split
            ds.data_dict = {k: n for k, n in enumerate(split[True] + list(INJECTED) + split[False])}
            for k in range(len(ds)):
                rec.clear()
                item = ds[k]
                name, n = item["seq_name"], int(item["seq_len"])
                length = seqs[name]["head_pose"].shape[0]
                start = rec.get("start", 0)
                case = f"{'eval' if for_eval else 'train'}/{name}"
                out[f"{case}/start"], out[f"{case}/seq_len"] = np.int64(start), np.int64(n)
                out[f"{case}/scale"], out[f"{case}/quat"], out[f"{case}/normals"] = np.float64(rec["scale"]), rec["quat"], rec["normals"]
                out[f"{case}/aligned_scale"] = np.float64(item["aligned_scale"])
                for key in TENSORS:
                    out[f"{case}/{key}"] = item[key].numpy().copy()
                # ---- the oracle's reference mode from the recorded draws: bit for bit
                q, Rr = O.random_rotation_from_normals(rec["normals"], np.float32)
                assert np.array_equal(q, rec["quat"]), case
                assert O.window_of(length, WINDOW, for_eval, start) == (start, n), case
                got = O.sample(seqs[name]["head_pose"], WINDOW, start, Rr, rec["scale"], mode="ref32")
                assert got["seq_len"] == n
                assert got["aligned_scale"] == out[f"{case}/aligned_scale"], case
                for key in TENSORS:
                    a, b = got[key], out[f"{case}/{key}"]
                    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (case, key, a.dtype, b.dtype, a.shape, b.shape)
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, key, float(np.abs(a - b).max()))
                f64 = O.sample(seqs[name]["head_pose"], WINDOW, start, Rr, np.float32(rec["scale"]), mode="fp64")
                worst = max([worst] + [O.err_units(got[key], f64[key]) for key in TENSORS[1:]])
    np.random.uniform = uniform
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays; the reference is at most {worst:.2f} eps-units from fp64")


if __name__ == "__main__":
    main()
