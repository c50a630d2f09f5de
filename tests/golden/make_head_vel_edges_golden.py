#!/usr/bin/env python3
"""Golden head velocities at rotation edges, produced by running the reference's own get_head_vel
(utils/data_utils/process_amass_dataset.py:111-137), unmodified, on the CPU.

Runs only where the reference checkout is present ($EGOEGO_REFERENCE, default /root/reference).  What executes is the reference's
Python, unmodified.  Not the reference's: pytorch3d.transforms (the scipy stand-ins of make_window_loop_golden.py) and everything
else its file imports and get_head_vel never reaches (the stub list of make_eval_golden.py), as in make_amass_golden.py.

Inputs: the sequences of tests/rotation_edge_cases.head_sequences() (2 and 40 frames; get_head_vel cannot take the 1-frame one:
it copies the last of no rows), as the float32 head_qpos the reference hands it (:463-466).  The file holds inputs and the
recorded head_vels only.  The script asserts that the rows whose angular part is exactly zero (axis * 0) are the pairs
tests/amass_oracle.py flags `same`, and prints how far the reference's float32 arithmetic lies from the fp64 oracle in its
float32 mode, per sequence (max |a - b| / max |b|): tests/amass_oracle.HEAD_EDGES_REFERENCE_DISTANCE.

    python tests/golden/make_head_vel_edges_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
OUT = os.path.join(HERE, "amass_head_edges.npz")


def main():
    import amass_oracle as O
    import make_amass_golden
    import make_window_loop_golden as W
    import rotation_edge_cases as RC

    P = make_amass_golden.load_reference(W.transforms_module())
    out, dist = {}, []
    for b, s in enumerate(RC.head_sequences()):
        T = s["rot"].shape[0]
        out["seq%d/head_rot" % b], out["seq%d/head_qpos" % b] = s["rot"], s["qpos32"]
        if T < 2:
            continue
        vels = np.asarray(P.get_head_vel(torch.from_numpy(s["qpos32"].copy())))
        want, same = O.head_vel(s["qpos32"], float32=True)
        assert vels.shape == want.shape == (T, 6)
        assert np.array_equal(np.all(vels[:, 3:] == 0, 1), np.append(same, same[-1])), b
        out["seq%d/head_vels" % b] = vels
        dist.append(O.rel_diff(vels, want))
        print(f"sequence {b}: {T:2d} frames  head_vels {vels.dtype}  same pairs {int(same.sum())}  reference vs the fp64 oracle {dist[-1]:.3e}")
    # (rounded up in the fourth digit: the constant is used as a bound on these very rows)
    print("HEAD_EDGES_REFERENCE_DISTANCE = (None, " + ", ".join("%.3e" % (d * 1.0005) for d in dist) + ")")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
