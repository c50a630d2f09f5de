"""fp64 numpy restatement of the reference's process_seq (utils/data_utils/process_amass_dataset.py:340-493), written from its
lines (not from the library's kernels):

  corrected_fps, trim_range, is_short, downsample_table   the host arithmetic (:360-363, :376, :381, :427-448)
  joints_and_head_rot     Jtr[:, :22] and the global rotation of joint 15 through tests/body_oracle.forward (betas 0)
  head_tracks             :454-472 with get_head_vel (:111-137), fp64
  process_seq             the whole record, or "short" / "terrain"

The floor height, contacts and discard flag come from tests/eval_oracle.floor_and_contacts on the joints rounded to float32, as
the reference receives them (body.Jtr is float32).  Poses are rounded to float32 first, as torch.Tensor(...) does (:151-156).
"""
import numpy as np
import torch

import body_oracle
import eval_oracle

OUT_FPS = 30
HEAD = 15
RECORD_KEYS = ("fps", "gender", "floor_height", "contacts", "trans", "root_orient", "pose_body", "betas", "joints", "head_qpos",
               "head_vels", "global_head_rot_6d", "global_head_trans", "global_head_rot_6d_diff", "global_head_trans_diff")
CONTINUOUS_KEYS = ("joints", "head_qpos", "head_vels", "global_head_rot_6d", "global_head_rot_6d_diff", "global_head_trans",
                   "global_head_trans_diff")

# how far the reference's own float32 results lie from this oracle on the golden inputs, worst relative difference per key
# (max |a - b| / max |b| per sequence; printed by tests/golden/make_amass_golden.py); the GPU tests' bounds may not exceed 4 x these
REFERENCE_DISTANCE = {"joints": 6.361e-08, "head_qpos": 6.688e-08, "head_vels": 4.134e-05, "global_head_rot_6d": 2.563e-07,
                      "global_head_rot_6d_diff": 3.102e-07, "global_head_trans": 6.688e-08, "global_head_trans_diff": 2.970e-06}


# the same for head_vels on the sequences of rotation_edge_cases.head_sequences() (1, 2 and 40 frames; the reference's
# get_head_vel cannot take one frame), against head_vel(..., float32=True); printed by tests/golden/make_head_vel_edges_golden.py
HEAD_EDGES_REFERENCE_DISTANCE = (None, 1.037e-07, 1.425e-07)


def corrected_fps(path, fps):
    if path.find("BMLhandball") >= 0:
        fps = 240
    if path.find("20160930_50032") >= 0 or path.find("20161014_50033") >= 0:
        fps = 59
    return fps


def trim_range(num_frames):
    return int(0.1 * num_frames), int(0.9 * num_frames)


def is_short(num_frames, fps):
    return num_frames < 1.0 * fps


def downsample_table(num_frames, fps):
    """-> (indices into the trimmed frames, the fps that is saved): :427-448."""
    if OUT_FPS != fps and not OUT_FPS > fps:
        fps_ratio = float(OUT_FPS) / fps
        new_num_frames = int(fps_ratio * num_frames)
        return np.linspace(0, num_frames - 1, num=new_num_frames, dtype=int), OUT_FPS
    return np.arange(num_frames), fps


def joints_and_head_rot(model, root_orient, pose_body, trans):
    """float32-rounded poses -> (Jtr[:, :22] fp64, the global rotation matrix of joint 15 fp64 [N, 3, 3])."""
    ro, pb, tr = (np.asarray(a).astype(np.float32).astype(np.float64) for a in (root_orient, pose_body, trans))
    pose = np.concatenate([ro, pb], 1).reshape(-1, 22, 3)
    out = body_oracle.forward(model, pose, tr, np.zeros((pose.shape[0], 16)), dtype=torch.float64)
    return out["Jtr"][:, :22].numpy(), out["A"][:, HEAD, :, :3].numpy()


def matrix_to_quaternion(R):
    """real-first, w >= 0, fp64: the candidate of the largest component (pytorch3d's rule)."""
    R = np.asarray(R, np.float64)
    m = lambda i, j: R[..., i, j]  # noqa: E731
    qa = np.sqrt(np.maximum(np.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2),
                                      1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2)], -1), 0.0))
    cand = np.stack([np.stack([qa[..., 0] ** 2, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
                     np.stack([m(2, 1) - m(1, 2), qa[..., 1] ** 2, m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], -1),
                     np.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), qa[..., 2] ** 2, m(1, 2) + m(2, 1)], -1),
                     np.stack([m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), qa[..., 3] ** 2], -1)], -2)
    k = qa.argmax(-1)
    q = np.take_along_axis(cand, k[..., None, None], -2)[..., 0, :] / (2.0 * np.maximum(np.take_along_axis(qa, k[..., None], -1), 0.1))
    return np.where(q[..., :1] < 0, -q, q)


def _q_mul(a, b):
    return eval_oracle._q_mul(a, b)


def head_vel(head_qpos, dt=1 / 30, float32=False):
    """get_head_vel (:111-137) in fp64 -> (head_vels [T, 6], the pairs that took the |1 -+ q0| < 1e-6 branch [T - 1] bool).
    `float32` rounds head_qpos to float32 first: the reference hands get_head_vel a float32 tensor (:463-466) and the kernel
    reads its own float32 quaternion, so at a quaternion whose rounding matters (w near 0, a relative rotation near pi) this is
    the mode they are compared in.  A single frame has no pair: zero rows."""
    qp = np.asarray(head_qpos, np.float64)
    if float32:
        qp = qp.astype(np.float32).astype(np.float64)
    if qp.shape[0] < 2:
        return np.zeros((qp.shape[0], 6)), np.zeros(0, bool)
    rows, same = [], []
    for i in range(qp.shape[0] - 1):
        cur, nxt = qp[i], qp[i + 1]
        v = (nxt[:3] - cur[:3]) / dt
        hq = cur[3:7].copy()
        hq[1] = hq[2] = 0.0
        hq /= np.linalg.norm(hq)
        v = eval_oracle.quat_to_matrix(hq).T @ v
        qrel = _q_mul(nxt[3:7], cur[3:7] * np.array([1.0, -1.0, -1.0, -1.0]))
        if qrel[0] < 0:
            qrel = -qrel
        if abs(1.0 - qrel[0]) < 1e-6 or abs(1 + qrel[0]) < 1e-6:
            axis, angle = np.array([1.0, 0.0, 0.0]), 0.0
            same.append(True)
        else:
            angle = 2 * np.arccos(qrel[0])
            axis = qrel[1:4] / np.sin(angle / 2.0)
            axis = axis / np.linalg.norm(axis)
            same.append(False)
        if angle > np.pi:
            angle -= 2 * np.pi
        elif angle < -np.pi:
            angle += 2 * np.pi
        rv = eval_oracle.quat_to_matrix(cur[3:7]).T @ ((axis * angle) / dt)
        rows.append(np.concatenate((v, rv)))
    rows.append(rows[-1].copy())
    return np.vstack(rows), np.asarray(same, bool)


def head_tracks(joints, head_rot, float32=False):
    """joints [T, 22, 3] (after the floor shift and the downsampling), head_rot [T, 3, 3] -> the seven head arrays in fp64, plus
    `same` (head_vel's flags), `quat` [T, 4] and `rot` (the input rotations).  `float32`: head_vel's mode of that name (head_qpos
    itself stays unrounded)."""
    joints, R = np.asarray(joints, np.float64), np.asarray(head_rot, np.float64)
    trans = joints[:, HEAD]
    quat = matrix_to_quaternion(R)
    qpos = np.concatenate([trans, quat], -1)
    vels, same = head_vel(qpos, float32=float32)
    diff = np.swapaxes(R[:-1], -1, -2) @ R[1:]
    return {"global_head_trans": trans, "global_head_rot_6d": R[:, :2].reshape(-1, 6), "head_qpos": qpos, "head_vels": vels,
            "global_head_rot_6d_diff": diff[:, :2].reshape(-1, 6), "global_head_trans_diff": trans[1:] - trans[:-1],
            "same": same, "quat": quat, "rot": R}


def process_seq(model, path, poses, trans, mocap_framerate):
    """-> a record (RECORD_KEYS; the continuous keys in fp64), "short" or "terrain"; plus a dict of what was computed on the way
    (`raw_joints` float32 at the raw rate, `fc` the floor oracle's dict, `table`, `head` the head_tracks dict)."""
    poses, trans = np.asarray(poses), np.asarray(trans)
    fps = corrected_fps(path, mocap_framerate)
    s, e = trim_range(poses.shape[0])
    trans, root_orient, pose_body = trans[s:e].copy(), poses[s:e, :3], poses[s:e, 3:66]
    n = trans.shape[0]
    if is_short(n, fps):
        return "short", {}
    j64, R = joints_and_head_rot(model, root_orient, pose_body, trans)
    j32 = j64.astype(np.float32)
    fc = eval_oracle.floor_and_contacts(j32, fps)
    floor = fc["offset_floor_height"]
    trans[:, 2] -= floor
    table, out_fps = downsample_table(n, fps)
    info = {"raw_joints": j32, "fc": fc, "table": table}
    if fc["discard_seq"]:
        return "terrain", info
    joints = j64[table].copy()
    joints[:, :, 2] -= np.float64(floor)
    head = head_tracks(joints, R[table])
    info["head"] = head
    rec = {"fps": out_fps, "gender": "male", "floor_height": floor, "contacts": fc["contacts"][table], "trans": trans[table],
           "root_orient": root_orient[table], "pose_body": pose_body[table], "betas": np.zeros(16), "joints": joints}
    rec.update({k: head[k] for k in CONTINUOUS_KEYS if k != "joints"})
    return {k: rec[k] for k in RECORD_KEYS}, info


def rel_diff(a, b):
    """worst |a - b| over the largest |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def head_conditions(head):
    """The conditions on the inputs that make the discrete parts of the head tracks no coin toss -> (smallest angle between
    non-identical consecutive output head rotations, smallest |w|, smallest heading norm)."""
    R, q = head["rot"], head["quat"]
    ang = []
    for a, b in zip(R[:-1], R[1:]):
        if not np.array_equal(a, b):
            ang.append(float(np.arccos(np.clip((np.trace(a.T @ b) - 1) / 2, -1, 1))))
    return (min(ang) if ang else np.inf), float(np.abs(q[:, 0]).min()), float(np.sqrt(q[:, 0] ** 2 + q[:, 3] ** 2).min())


def assert_head_conditions(head):
    ang, w, hn = head_conditions(head)
    assert ang >= 0.008, f"consecutive head rotations {ang} rad apart: identical or >= 0.008 expected"
    assert w >= 0.5, f"head quaternion |w| = {w}: >= 0.5 expected"
    assert hn >= 0.5, f"heading norm {hn}: >= 0.5 expected"
