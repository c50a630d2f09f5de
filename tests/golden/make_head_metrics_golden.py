#!/usr/bin/env python3
"""Golden values of the stage-1 score: the reference's own egoego/eval/head_pose_metrics.py compute_head_pose_metrics, unmodified
(numpy only), run on seeded pose pairs (tests/stage1_ragged_cases.py metric_poses) at several lengths, 1 included.

Runs only where the reference checkout is present; its root is the first argument or $EGOEGO_REFERENCE.

    python tests/golden/make_head_metrics_golden.py /path/to/reference

Writes tests/golden/head_metrics_golden.npz: seed, lengths [B], pred / gt [B, Tmax, 7] float64 (xyz + quaternion w,x,y,z; rows past
a length are zero) and metrics [B, 3] = (head_dist, head_dist_rot_only, head_trans_err in mm).  The rotation matrices handed to the
reference are pytorch3d's quaternion_to_matrix formula in float64, as eval_egoego.py:298-303 builds them.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
SEED = 4711
LENGTHS = (1, 2, 63, 64, 65, 139, 300)


def main():
    import stage1_ragged_cases as K
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ["EGOEGO_REFERENCE"]
    spec = importlib.util.spec_from_file_location("ref_head_pose_metrics", os.path.join(ref_root, "egoego", "eval", "head_pose_metrics.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    B, Tmax = len(LENGTHS), max(LENGTHS)
    pred, gt = K.metric_poses(SEED, B, Tmax)
    metrics = np.zeros((B, 3))
    for b, n in enumerate(LENGTHS):
        pred[b, n:] = 0
        gt[b, n:] = 0
        metrics[b] = ref.compute_head_pose_metrics(pred[b, :n, :3], K.quat_to_matrix(pred[b, :n, 3:]), gt[b, :n, :3],
                                                   K.quat_to_matrix(gt[b, :n, 3:]))
        mine = K.head_pose_metrics_np(pred[b, :n, :3], K.quat_to_matrix(pred[b, :n, 3:]), gt[b, :n, :3], K.quat_to_matrix(gt[b, :n, 3:]))
        print(n, metrics[b], "restatement off by", np.abs(np.array(mine) - metrics[b]).max() / np.abs(metrics[b]).max())
    out = os.path.join(HERE, "head_metrics_golden.npz")
    np.savez_compressed(out, seed=SEED, lengths=np.array(LENGTHS), pred=pred, gt=gt, metrics=metrics)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
