"""numpy restatement of HeadNet's training data (the reference's ARESHeadPoseDataset, egoego/data/ares_headpose_dataset.py: the
filter of 93-109, the dropping rule of 82-89 and __getitem__ of 270-333) for GIVEN starts, and a numpy replica of the keyed draw of
egoego_s1_head_batch (include/egoego_hip.h).  tests/golden/make_head_batch_golden.py asserts that item() reproduces the reference's
items bit for bit; the kernel only selects and copies, so padded() is what it must write, bit for bit.

A sequence here is a dict: head_qpos [T, 7], head_vels [T, 6], of_feats [T - 1, D] and optionally the six SLAM arrays of SLAM_KEYS,
each [L, ...] (the whole aligned / original track).
"""
import numpy as np

from gravity_batch_oracle import MASK32, philox4x32_10

DRAW_TAG = 0x48424154  # "HBAT"
SLAM_KEYS = ("aligned_slam_trans", "aligned_slam_rot_quat", "aligned_slam_rot_mat", "ori_slam_trans", "ori_slam_rot_quat",
             "ori_slam_rot_mat")


# ---------------------------------------------------------------------------------------------- the rules
def passes_filter(T, n_of_files, window):
    """filter_data (101): the sequence stays iff it is longer than the window and has one feature file per frame but the last."""
    return T > window and T - 1 == n_of_files


def kept(sequences, window, for_eval):
    """HeadBatches' dropping rules on a list of sequence dicts -> (indices kept, {'short', 'no_slam'})."""
    any_slam = any("aligned_slam_trans" in s or s.get("slam") is not None for s in sequences)
    keep, dropped = [], {"short": 0, "no_slam": 0}
    for k, s in enumerate(sequences):
        F = len(s["head_qpos"]) - 1
        if F < (1 if for_eval else window):
            dropped["short"] += 1
        elif any_slam and not ("aligned_slam_trans" in s or s.get("slam") is not None):
            dropped["no_slam"] += 1
        else:
            keep.append(k)
    return keep, dropped


def window_of(F, window, for_eval, start):
    """(276-283) -> (start, n), or None where the kernel writes an empty sample: fewer than one feature frame, no room for a window
    in training, a start outside range(F - window + 1).  for_eval: start 0 and n = min(F, window), `window` being the padded length
    (the reference takes all F frames; Python passes the batch's largest F)."""
    if F < 1:
        return None
    if for_eval:
        return 0, min(F, window)
    room = F - window + 1
    if room < 1 or not 0 <= start < room:
        return None
    return int(start), window


# ---------------------------------------------------------------------------------------------- one sample
def item(seq, start, n):
    """The reference's query dict (without seq_name): rows start .. start + n of the pose-like arrays, start .. start + n - 1 of
    the frame-like ones; dtypes as the arrays have them."""
    q = {"head_pose": seq["head_qpos"][start:start + n + 1], "head_vels": seq["head_vels"][:-1][start:start + n],
         "of": seq["of_feats"][start:start + n], "seq_len": n}
    for k in SLAM_KEYS:
        if k in seq:
            q[k] = seq[k][start:start + n + 1]
    return q


def padded(seq, window, for_eval=False, start=0):
    """What egoego_s1_head_batch writes for one sample: item() padded with zeros to window (+ 1) rows, head_vels rounded to fp32
    once, lengths, start_t_idx and (with SLAM) pose_lengths = the rows the reference's slice of the track has."""
    W = int(window)
    w = window_of(len(seq["head_qpos"]) - 1, W, for_eval, start)
    st, n = (0, 0) if w is None else w
    q = item(seq, st, n) if w is not None else None
    D = seq["of_feats"].shape[1]

    def pad(key, rows, tail, dtype):
        out = np.zeros((rows,) + tail, dtype)
        if q is not None:
            a = np.asarray(q[key]).astype(dtype)
            out[:len(a)] = a
        return out

    out = {"head_pose": pad("head_pose", W + 1, (7,), np.float32), "head_vels": pad("head_vels", W, (6,), np.float32),
           "of": pad("of", W, (D,), np.float32), "lengths": np.int32(n), "seq_len": np.int64(n), "start_t_idx": np.int32(st)}
    if "aligned_slam_trans" in seq:
        for k in SLAM_KEYS:
            out[k] = pad(k, W + 1, seq[k].shape[1:], np.float64 if k == "ori_slam_trans" else np.float32)
        L = len(seq["aligned_slam_trans"])
        out["pose_lengths"] = np.int32(0 if w is None else min(max(L - st, 0), n + 1))
        if q is not None:
            assert out["pose_lengths"] == len(q["aligned_slam_trans"])
    return out


# ---------------------------------------------------------------------------------------------- an ARES tree for the loaders
def write_ares_tree(root, seqs, src_root, short_files=()):
    """The files ARESHeadPoseDataset reads, under `root`: both splits' motion file (of_files recorded under `src_root`, as the
    published files record them), one .npy per feature frame and the SLAM track of every sequence that has a raw `slam`.
    short_files: names whose of_files list lacks its last entry (the filter drops them)."""
    import os

    import joblib
    src = os.path.dirname(src_root)
    motion = {}
    for k, s in enumerate(seqs):
        scene, rest = s["seq_name"].split("-")[0], "-".join(s["seq_name"].split("-")[1:])
        files = [f"{src_root}/{scene}/{rest}/raft_flows/{t:05d}.npy" for t in range(len(s["of_feats"]))]
        for f, row in zip(files, s["of_feats"]):
            real = f.replace(src, os.path.join(root, "ares")).replace("raft_flows", "raft_of_feats")
            os.makedirs(os.path.dirname(real), exist_ok=True)
            np.save(real, row)
        if s["seq_name"] in short_files:
            files = files[:-1]
        if s.get("slam") is not None:
            path = os.path.join(root, "ares", "droid_slam_res", scene, rest + ".npy")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, s["slam"])
        motion[k] = {"seq_name": s["seq_name"], "head_qpos": s["head_qpos"], "head_vels": s["head_vels"], "of_files": files}
    os.makedirs(os.path.join(root, "ares_egoego_processed"), exist_ok=True)
    for split in ("train", "test"):
        joblib.dump(motion, os.path.join(root, "ares_egoego_processed", f"{split}_ares_smplh_motion.p"))


# ---------------------------------------------------------------------------------------------- the draw
def draw_start(seed, draw_ids, room):
    """(word 0 * room) >> 32 of Philox4x32-10 keyed by `seed` at the counter (draw id low, draw id high, 1, DRAW_TAG) -> int64 [n]"""
    ids = np.asarray(draw_ids, np.int64).astype(np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10((ids & MASK32, ids >> np.uint64(32), 1, DRAW_TAG), (seed & 0xFFFFFFFF, seed >> 32))[..., 0].astype(np.uint64)
    return ((w * np.uint64(room)) >> np.uint64(32)).astype(np.int64)
