#!/usr/bin/env python3
"""Golden vectors of the STAGE-2 MOTION WINDOWS at their heading and rotation edges, produced by running the reference's own code.

Runs only in the authoring container (/root/reference present).  What executes is the reference's Python, unmodified, through the
stand-ins of make_motion_windows_golden.py (imported, not restated; what they replace is listed there): cal_normalize_data_input,
process_window_data and rotate_at_frame_smplh with canonicalize_init_head on.

Inputs (tests/window_cases.py, seeded; the fixture records the recipe, not the arrays): per window W in (64, 120) the heading
sequence (22 windows, window k starting on heading case k % 21: headings up to pi - 1e-3, pitches up to 1.52) and the angle
sequence (three windows of the angle draws, up to 7 rad).  Every window's preconditions are asserted by window_cases.

The fixture holds DATA only: the recipe, per (kind, W) the window table, the reference's recover_rot_quat, its arrays on the rows
t % ROW_STEP == 0 and each window's last two, and PER WINDOW and output the reference's worst distance from tests/windows_oracle.py
over all rows.  The reference computes in float32 with a float64 detour for the heading: near a half turn and near the vertical
that distance is large, and it is recorded as it is.  global_jvel is asserted here to be the float32 difference of the reference's
own global_jpos and is not stored.

    python tests/golden/make_motion_window_edges_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

WINDOWS = (64, 120)
KINDS = ("heading", "angle")
ROW_STEP = 16
ARRAYS = ("global_jpos", "global_rot_6d", "local_rot_6d")


def main():
    from make_window_loop_golden import import_reference
    from make_motion_windows_golden import record_headings, sample_rows, stand_in_dataset
    import window_cases as WC
    from test_harness_golden import REST_OFFSETS
    _, DS, _ = import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self  # dataset:410-412; no GPU here
    yrots = record_headings(DS)

    out = {"row_step": np.int64(ROW_STEP), "windows": np.array(WINDOWS), "kinds": np.array(KINDS), "distance_keys": np.array(WC.CONTINUOUS),
           "heading_cases": np.array(WC.HEADING_CASES), "angles": WC.ANGLES_ALL,
           "seeds": np.array([WC.heading_sequence.__defaults__[0], WC.angle_sequence.__defaults__[0]])}
    for W in WINDOWS:
        for kind in KINDS:
            tag = "%s_w%d" % (kind, W)
            case = WC.rule_case(kind, W)
            seq, table, orc = case["seq"], case["table"], case["oracle"]
            if kind == "angle":
                assert not WC.holds_every_angle(seq[1], seq[2])
            ds = stand_in_dataset(DS, REST_OFFSETS, {0: {"seq_name": tag, "trans": seq[0], "root_orient": seq[1], "body_pose": seq[2]}}, W, True)
            del yrots[:]
            ds.cal_normalize_data_input()
            wd = ds.window_data_dict
            N = len(wd)
            assert len(ds.local6d) == N == len(yrots)
            got = np.array([[0, wd[i]["start_t_idx"], wd[i]["end_t_idx"], wd[i]["global_jpos"].shape[0]] for i in range(N)])
            assert np.array_equal(got, table), tag
            dist = np.zeros((N, len(WC.CONTINUOUS)))
            rows = [sample_rows(n, ROW_STEP) for n in table[:, 3]]
            kept = {k: [] for k in ARRAYS}
            for i in range(N):
                n = table[i, 3]
                p = wd[i]["global_jpos"]
                assert p.dtype == np.float32 and np.array_equal(wd[i]["global_jvel"], np.concatenate([p[1:] - p[:-1], np.zeros((1, 66), np.float32)]))
                ref = {"global_jpos": p, "global_rot_6d": wd[i]["global_rot_6d"], "local_rot_6d": ds.local6d[i]}
                for c, k in enumerate(ARRAYS):
                    assert ref[k].shape == orc[k][i, :n].shape and np.isfinite(ref[k]).all(), (tag, i, k)
                    dist[i, c] = np.abs(ref[k].astype(np.float64) - orc[k][i, :n]).max()
                    kept[k].append(np.asarray(ref[k], np.float32)[rows[i]])
                dist[i, 3] = WC.up_to_sign(yrots[i], orc["recover_rot_quat"][i]).max()
            out[tag + "_table"] = table
            out[tag + "_recover_rot_quat"] = np.array(yrots)
            out[tag + "_reference_distance"] = dist
            for k in ARRAYS:
                out[tag + "_" + k] = np.concatenate(kept[k])
            print(tag, "windows", N, "stored rows", sum(len(r) for r in rows))
            for i in range(N):
                what = "heading %.4f pitch %.2f" % WC.HEADING_CASES[i % 21] if kind == "heading" else "angle draws"
                print("  window %2d (%s): reference vs oracle" % (i, what), " ".join("%s %.2e" % kv for kv in zip(WC.CONTINUOUS, dist[i])))
    path = os.path.join(HERE, "motion_window_edges_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
