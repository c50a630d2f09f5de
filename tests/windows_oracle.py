"""fp64 numpy restatement of the reference's stage-2 window construction, written from the definitions (not from the library's
kernels); test-only, like eval_oracle.py:

  window_table            cal_normalize_data_input, amass_diffusion_dataset.py:316-335
  process_window          process_window_data, 409-510, with rotate_at_frame_smplh (lafan1/utils.py:111-137)
  build                   every window of every sequence, padded to `window` rows
  stats, motion           extract_min_max_mean_std_from_data 355-377, __getitem__ 515-538

The inputs are cast to float32 first, as the reference's .float() does; everything after is float64.  Matrices and the
reference's own formulas are used where the kernels use quaternions.
"""
import numpy as np

PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)
HEAD = 15
KEYS = ("global_jpos", "global_jvel", "global_rot_6d", "local_rot_6d", "recover_rot_quat")


def window_table(lengths, window=120, min_frames=30):
    rows = []
    for k, num_steps in enumerate(lengths):
        start = 0
        while start < num_steps:
            end = start + window - 1
            if end >= num_steps:
                end = num_steps
            if end - start >= min_frames:
                rows.append((k, start, end, len(range(num_steps)[start:end + 1])))
            start += window // 2
    return np.asarray(rows, np.int64).reshape(-1, 4)


def rodrigues(aa):
    """axis-angle [..., 3] -> rotation matrices [..., 3, 3]: I + sin(a) K + (1 - cos(a)) K^2"""
    aa = np.asarray(aa, np.float64)
    ang = np.linalg.norm(aa, axis=-1)[..., None, None]
    safe = np.where(ang < 1e-12, 1.0, ang)
    x, y, z = np.moveaxis(aa, -1, 0)
    o = np.zeros_like(x)
    K = np.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(aa.shape[:-1] + (3, 3))
    a = np.where(ang < 1e-12, 1.0, np.sin(ang) / safe)
    b = np.where(ang < 1e-12, 0.5, (1.0 - np.cos(ang)) / (safe * safe))
    return np.eye(3) + a * K + b * (K @ K)


def heading(head_rot):
    """rotate_at_frame_smplh's yrot (w, x, y, z) for the head's global rotation matrix in the first frame"""
    fwd = head_rot[:, 0] * np.array([1.0, 1.0, 0.0])  # R . x, projected
    fwd = fwd / (np.sqrt((fwd * fwd).sum()) + 1e-8)
    ex = np.array([1.0, 0.0, 0.0])
    q = np.concatenate([[np.sqrt((ex * ex).sum() * (fwd * fwd).sum()) + (ex * fwd).sum()], np.cross(ex, fwd)])
    return q / (np.sqrt((q * q).sum()) + 1e-8)


def _quat_mul_vec(q, x):
    t = 2.0 * np.cross(q[1:], x)
    return x + q[0] * t + np.cross(q[1:], t)


def _quat_to_matrix(q):
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def process_window(trans, root_orient, body_pose, rest_offsets, canonicalize=True, parents=PARENTS):
    """One window's frames [n, 3], [n, 3], [n, 63] -> dict of float64 arrays: global_jpos, global_jvel [n, 66], global_rot_6d,
    local_rot_6d [n, 132], recover_rot_quat [4]."""
    trans = np.asarray(trans, np.float32).astype(np.float64)
    aa = np.concatenate([np.asarray(root_orient, np.float32).reshape(-1, 1, 3), np.asarray(body_pose, np.float32).reshape(-1, 21, 3)], 1)
    rest = np.asarray(rest_offsets, np.float32).astype(np.float64).reshape(22, 3)
    n = aa.shape[0]
    local = rodrigues(aa)  # [n, 22, 3, 3]

    def chain(loc):
        glob = loc.copy()
        for j in range(1, 22):
            glob[:, j] = glob[:, parents[j]] @ loc[:, j]
        return glob

    yrot = np.array([1.0, 0.0, 0.0, 0.0])
    if canonicalize:
        yrot = heading(chain(local)[0, HEAD])
        inv = yrot * np.array([1.0, -1.0, -1.0, -1.0])
        local = local.copy()
        local[:, 0] = _quat_to_matrix(inv) @ local[:, 0]
        trans = np.stack([_quat_mul_vec(inv, x) for x in trans])
    glob = chain(local)
    pos = np.zeros((n, 22, 3))
    for j in range(1, 22):
        pos[:, j] = np.einsum("nab,b->na", glob[:, parents[j]], rest[j]) + pos[:, parents[j]]
    pos = pos + rest[0] + trans[:, None, :]
    move = pos[0, HEAD].copy()
    move[2] = 0.0
    pos = pos - move
    # the velocity is taken on the positions as stored (float32) and is itself a float32 difference
    p32 = pos.astype(np.float32)
    vel = np.concatenate([p32[1:] - p32[:-1], np.zeros((1, 22, 3), np.float32)], 0)
    return {"global_jpos": pos.reshape(n, 66), "global_jvel": vel.astype(np.float64).reshape(n, 66),
            "global_rot_6d": glob[:, :, :2, :].reshape(n, 132), "local_rot_6d": local[:, :, :2, :].reshape(n, 132), "recover_rot_quat": yrot}


def build(seqs, rest_offsets, window=120, canonicalize=True, min_frames=30, table=None):
    """seqs: list of (trans, root_orient, body_pose) -> (table [N, 4], dict of arrays padded with zero rows to `window`).
    `table` overrides the window rule (rows of (sequence, start, end, length))."""
    if table is None:
        table = window_table([len(s[0]) for s in seqs], window, min_frames)
    N = len(table)
    out = {"global_jpos": np.zeros((N, window, 66)), "global_jvel": np.zeros((N, window, 66)), "global_rot_6d": np.zeros((N, window, 132)),
           "local_rot_6d": np.zeros((N, window, 132)), "recover_rot_quat": np.zeros((N, 4))}
    for i, (k, start, _, length) in enumerate(table):
        if length == 0:  # an empty window (only through `table`): no first frame, so no heading; zero rows
            out["recover_rot_quat"][i] = [1.0, 0.0, 0.0, 0.0]
            continue
        w = process_window(*(a[start:start + length] for a in seqs[k]), rest_offsets, canonicalize)
        for key in KEYS[:4]:
            out[key][i, :length] = w[key]
        out["recover_rot_quat"][i] = w["recover_rot_quat"]
    return table, out


def stats(jpos, jvel, lengths):
    """min / max per coordinate over the real rows of all windows"""
    real = np.arange(jpos.shape[1])[None, :] < np.asarray(lengths)[:, None]
    p, v = jpos[real], jvel[real]
    return {"global_jpos_min": p.min(0), "global_jpos_max": p.max(0), "global_jvel_min": v.min(0), "global_jvel_max": v.max(0)}


def motion(jpos, rot6d, lengths, st):
    lo, hi = np.asarray(st["global_jpos_min"], np.float64), np.asarray(st["global_jpos_max"], np.float64)
    real = (np.arange(jpos.shape[1])[None, :] < np.asarray(lengths)[:, None])[..., None]
    return np.where(real, np.concatenate([(jpos - lo) / (hi - lo) * 2 - 1, rot6d], -1), 0.0)


def golden_sequences(hg, g):
    """The fixture's input recipe -> list of (trans, root_orient, body_pose): the demo's 140 frames (harness_golden.npz), its first
    g['cut_lengths'] frames, and the copy turned about z and shifted that the fixture carries."""
    demo = (hg["demo_trans"], hg["demo_root_orient"], hg["demo_body_pose"])
    seqs = [demo] + [tuple(a[:n] for a in demo) for n in g["cut_lengths"]]
    return seqs + [(g["turned_trans"], g["turned_root_orient"], hg["demo_body_pose"])]
