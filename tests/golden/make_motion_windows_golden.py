#!/usr/bin/env python3
"""Golden vectors of the STAGE-2 MOTION WINDOWS, produced by running the reference's own code.

Runs only in the authoring container (/root/reference present).  What executes here is the reference's Python, unmodified, bound
to a stand-in `self` that carries opt.canonicalize_init_head, window, data_dict, rest_human_offsets and the statistics:

  AMASSDataset.cal_normalize_data_input, process_window_data, extract_min_max_mean_std_from_data, __getitem__,
  normalize_jpos_min_max                          egoego/data/amass_diffusion_dataset.py:316-353, 409-510, 355-377, 515-538, 379-385
  local2global_pose, quat_fk_torch                egoego/data/amass_diffusion_dataset.py:92-107, 127-143
  rotate_at_frame_smplh                           egoego/lafan1/utils.py:111-137

What is NOT the reference's, as in make_window_loop_golden.py (whose stand-ins and stubs are imported, not restated): the bodies of
the pytorch3d.transforms functions, on numpy + scipy; get_smpl_parents, replaced by the 22 standard parents; the rest-pose
offsets (test_harness_golden.REST_OFFSETS).  One more patch: torch.Tensor.cuda is the identity for the run, because
process_window_data calls .cuda() on its inputs (dataset:410-412) and this container has no GPU.  rotate_at_frame_smplh is
wrapped to record the heading it returns; nothing it computes is changed.

Inputs: the demo's 140 real frames (harness_golden.npz), copies cut to 29, 30, 89, 90, 119 and 120 frames, and a copy turned 1.1 rad
about z and shifted.  Runs: window 120 and 40, both branches of canonicalize_init_head.  Every window's first-frame head x-axis is
asserted to lie well away from the vertical and its heading well away from a half turn, where the reference's heading is
ill-conditioned.

The fixture holds DATA only: the recipe (cut lengths, the turned copy), per run the window table, the statistics, the worst
absolute distance of the reference's results from tests/windows_oracle.py per output, and the reference's arrays on a subset of
rows (every window's rows t % ROW_STEP == 0 and its last two; all rows would not fit the size limit: the distances above are over
all rows).  global_jvel is not stored: the generator asserts that it is exactly the float32 difference of the stored global_jpos
with a zero last row, and the tests rebuild it so.

    python tests/golden/make_motion_windows_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
from scipy.spatial.transform import Rotation as Rot

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

CUTS = (29, 30, 89, 90, 119, 120)
TURN, SHIFT = 1.1, (0.7, -0.4, 0.0)
ROW_STEP = 8
RUNS = ((120, True), (120, False), (40, True), (40, False))
ITEM_WINDOWS = 2  # __getitem__ items stored per run: the first full window and the first padded one


def sample_rows(length, step=ROW_STEP):
    return np.array([t for t in range(length) if t % step == 0 or t >= length - 2])


def stand_in_dataset(DS, rest_offsets, data_dict, window, cano):
    """The stand-in `self`: the reference's own AMASSDataset methods bound to an object that carries what they read.
    process_window_data also returns local_rot_6d, which cal_normalize_data_input drops: it is wrapped to record it in
    ds.local6d (nothing is changed)."""
    ds = types.SimpleNamespace(opt=types.SimpleNamespace(canonicalize_init_head=cano), window=window, data_dict=data_dict,
                               rest_human_offsets=torch.from_numpy(rest_offsets).float().reshape(1, 22, 3), local6d=[])
    for name in ("cal_normalize_data_input", "process_window_data", "extract_min_max_mean_std_from_data", "__getitem__",
                 "normalize_jpos_min_max", "__len__"):
        setattr(ds, name, types.MethodType(getattr(DS.AMASSDataset, name), ds))
    pwd0 = ds.process_window_data

    def pwd_rec(*a, **k):
        q = pwd0(*a, **k)
        ds.local6d.append(q["local_rot_6d"].reshape(-1, 132).numpy().copy())
        return q
    ds.process_window_data = pwd_rec
    return ds


def record_headings(DS):
    """Wraps DS.rotate_at_frame_smplh to record the heading it returns -> the list that fills up."""
    yrots = []
    raf0 = DS.rotate_at_frame_smplh

    def raf_rec(*a, **k):
        res = raf0(*a, **k)
        yrots.append(np.array(res[2]).reshape(4))
        return res
    DS.rotate_at_frame_smplh = raf_rec
    return yrots


def main():
    from make_window_loop_golden import import_reference
    import windows_oracle as WO
    from test_harness_golden import REST_OFFSETS
    _, DS, _ = import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self  # dataset:410-412; no GPU here

    hg = np.load(os.path.join(HERE, "harness_golden.npz"))
    rz = Rot.from_rotvec([0.0, 0.0, TURN])
    out = {"cut_lengths": np.array(CUTS), "turn": np.float64(TURN), "shift": np.array(SHIFT), "row_step": np.int64(ROW_STEP),
           "turned_trans": rz.apply(hg["demo_trans"]) + np.array(SHIFT),
           "turned_root_orient": (rz * Rot.from_rotvec(hg["demo_root_orient"])).as_rotvec()}
    seqs = WO.golden_sequences(hg, out)
    data_dict = {k: {"seq_name": "seq_%d_len_%d" % (k, len(s[0])), "trans": s[0], "root_orient": s[1], "body_pose": s[2]}
                 for k, s in enumerate(seqs)}
    out["seq_names"] = np.array([data_dict[k]["seq_name"] for k in data_dict])

    yrots = record_headings(DS)
    worst = {}

    def note(key, ref, orc):
        d = float(np.abs(np.asarray(ref, np.float64) - orc).max())
        worst[key] = max(worst.get(key, 0.0), d)

    for window, cano in RUNS:
        tag = "w%d_%s" % (window, "cano" if cano else "raw")
        ds = stand_in_dataset(DS, REST_OFFSETS, data_dict, window, cano)
        local6d = ds.local6d
        del yrots[:]
        ds.cal_normalize_data_input()
        wd = ds.window_data_dict
        N = len(wd)
        assert len(local6d) == N and len(yrots) == (N if cano else 0)
        st = ds.extract_min_max_mean_std_from_data()
        for k in ("global_jpos_min", "global_jpos_max", "global_jvel_min", "global_jvel_max"):  # dataset:236-239
            setattr(ds, k, torch.from_numpy(st[k]).float().reshape(22, 3)[None])
        names = {data_dict[k]["seq_name"]: k for k in data_dict}
        table = np.array([[names[wd[i]["seq_name"]], wd[i]["start_t_idx"], wd[i]["end_t_idx"], wd[i]["global_jpos"].shape[0]] for i in range(N)])
        out[tag + "_table"] = table
        assert np.array_equal(table, WO.window_table([len(s[0]) for s in seqs], window)), tag
        _, orc = WO.build(seqs, REST_OFFSETS, window, cano)
        lengths = table[:, 3]
        ref = {k: np.zeros((N, window, w), np.float32) for k, w in (("global_jpos", 66), ("global_jvel", 66), ("global_rot_6d", 132),
                                                                    ("local_rot_6d", 132))}
        for i in range(N):
            n = lengths[i]
            assert wd[i]["global_jpos"].dtype == np.float32 and wd[i]["global_rot_6d"].shape == (n, 132)
            for k in ("global_jpos", "global_jvel", "global_rot_6d"):
                ref[k][i, :n] = wd[i][k]
            ref["local_rot_6d"][i, :n] = local6d[i]
            p = wd[i]["global_jpos"]
            assert np.array_equal(wd[i]["global_jvel"], np.concatenate([p[1:] - p[:-1], np.zeros((1, 66), np.float32)]))
            # conditioning margins, on the oracle's float64 head rotation of the first frame
            k, s = table[i, 0], table[i, 1]
            aa = np.concatenate([seqs[k][1][s:s + 1, None], seqs[k][2][s:s + 1].reshape(1, 21, 3)], 1)
            R = np.eye(3)
            for j in (0, 3, 6, 9, 12, 15):
                R = R @ WO.rodrigues(aa[0, j])
            horiz = np.hypot(R[0, 0], R[1, 0])
            assert horiz > 0.5, (tag, i, horiz)  # the head's x-axis is at most 60 degrees from the horizontal
            if cano:
                assert 1.0 + R[0, 0] / horiz > 0.1, (tag, i)  # the heading is not near a half turn
        for k in ref:
            note(k, ref[k], orc[k])
        rec = np.array(yrots) if cano else np.tile([1.0, 0.0, 0.0, 0.0], (N, 1))
        note("recover_rot_quat", rec, orc["recover_rot_quat"])
        out[tag + "_recover_rot_quat"] = rec
        so = WO.stats(orc["global_jpos"], orc["global_jvel"], lengths)
        for k in st:
            assert st[k].dtype == np.float32 and st[k].shape == (66,)
            note(k, st[k], so[k])
            out[tag + "_" + k] = st[k]
        # __getitem__ for every window against the oracle; a full and a padded window are stored
        mo = WO.motion(orc["global_jpos"], orc["global_rot_6d"], lengths, so)
        items = []
        for i in range(N):
            it = ds.__getitem__(i)
            assert it["seq_len"] == lengths[i] and it["motion"].shape == (window, 198) and it["motion"].dtype == torch.float32
            note("motion", it["motion"].numpy(), mo[i])
            items.append(it["motion"].numpy())
        pick = [int(np.flatnonzero(lengths == window)[0]), int(np.flatnonzero(lengths < window)[0])][:ITEM_WINDOWS]
        out[tag + "_item_index"] = np.array(pick)
        rows = [sample_rows(n) for n in lengths]
        out[tag + "_item_motion"] = np.concatenate([items[i][rows[i]] for i in pick])
        for k in ("global_jpos", "global_rot_6d", "local_rot_6d"):
            out[tag + "_" + k] = np.concatenate([ref[k][i, rows[i]] for i in range(N)])
        print(tag, "windows", N, "real rows", int(lengths.sum()), "stored rows", sum(len(r) for r in rows))
    # the layout of the files the reference writes (dataset:227, 231), for the tool's test
    out["file_window_keys"] = np.array(sorted(wd[0]))
    out["file_stats_keys"] = np.array(sorted(st))
    out["file_dtypes"] = np.array([str(wd[0][k].dtype) for k in ("global_jpos", "global_jvel", "global_rot_6d")] + [str(st["global_jpos_min"].dtype)])
    out["file_index_types"] = np.array([type(wd[0]["start_t_idx"]).__name__, type(wd[0]["end_t_idx"]).__name__, type(wd[0]["seq_name"]).__name__])
    keys = sorted(worst)
    out["reference_distance_keys"] = np.array(keys)
    out["reference_distance"] = np.array([worst[k] for k in keys])
    for k in keys:
        print("reference vs oracle, worst |difference| %-18s %.3e" % (k, worst[k]))
    path = os.path.join(HERE, "motion_windows_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
