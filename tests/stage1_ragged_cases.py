"""What tests/test_stage1_ragged.py and tests/test_gpu_stage1_ragged.py share: the planar closed form of evo's Umeyama rotation
and compute_head_pose_metrics restated in numpy, the table of trajectory pairs, seeded ragged stage-1 batches and their
per-sequence oracle.  Host code only (numpy, torch on the CPU); nothing here needs a GPU."""
import functools

import numpy as np
import torch

import stage1_oracle as O

ULP32 = 2.0 ** -23  # one fp32 ulp at 1.0


# ---------------------------------------------------------------------------------------------- the planar closed form
def planar_covariance(est, ref):
    """est, ref [n, >= 2] -> A [2, 2] = (1/n) sum (ref_i - mean_ref)(est_i - mean_est)^T over xy."""
    e, r = np.asarray(est, np.float64)[:, :2], np.asarray(ref, np.float64)[:, :2]
    return (r - r.mean(0)).T.dot(e - e.mean(0)) / len(e)


def planar_umeyama(est, ref):
    """The r of evo's umeyama_alignment on points whose z is constant, without an SVD: blockdiag(Q, det Q), Q the orthogonal polar
    factor of the 2 x 2 covariance A.  det A >= 0: the rotation by atan2(A10 - A01, A00 + A11); det A < 0: the reflection
    [[e, f], [f, -e]] / hypot(e, f) with e = A00 - A11, f = A01 + A10, and -1 in the z corner.  A zero covariance gives identity."""
    A = planar_covariance(est, ref)
    rot = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0] >= 0
    e = A[0, 0] + A[1, 1] if rot else A[0, 0] - A[1, 1]
    f = A[1, 0] - A[0, 1] if rot else A[0, 1] + A[1, 0]
    h = np.hypot(e, f)
    if h == 0:
        return np.eye(3)
    c, s = e / h, f / h
    if rot:
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return np.array([[c, s, 0], [s, -c, 0], [0, 0, -1.0]])


def oracle_umeyama(est, ref):
    """stage1_oracle.umeyama_r on the xy of est / ref with z set to 1 (what HN's align_xy_plane_traj hands to evo)."""
    e, r = np.array(est, np.float64)[:, :3].copy(), np.array(ref, np.float64)[:, :3].copy()
    e[:, 2] = 1
    r[:, 2] = 1
    return O.umeyama_r(e.T, r.T)


def sigma_ratio(est, ref):
    s = np.linalg.svd(planar_covariance(est, ref), compute_uv=False)
    return s[1] / s[0] if s[0] > 0 else 0.0


def _walk(rng, n, step):
    return np.cumsum(rng.standard_normal((n, 3)) * step, 0)


def _rotz(t):
    return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]])


@functools.lru_cache(maxsize=None)
def trajectory_cases():
    """-> {"compared": [(name, est [n, 3], ref [n, 3], reflected)], "lines": [...], "single": [...]}.  A compared pair is a random
    walk and a rotated, scaled, noisy copy of it (the reflected ones mirrored in y first, so that det A < 0); `lines` are exact
    straight lines (A of rank 1: the reference's own answer is arbitrary there); `single` has one frame."""
    rng = np.random.default_rng(20240611)
    compared, lines, single = [], [], []
    for k, n in enumerate((2, 3, 7, 64, 65, 130, 513, 1100)):
        for reflected in (False, True):
            est = _walk(rng, n, 0.05) + rng.uniform(-1, 1, 3)
            if n == 3:  # three steps of a walk are close to a line; a triangle is the smallest well-conditioned case
                est = np.array([[0.0, 0.0, 0.1], [0.3, 0.05, 0.0], [0.1, 0.4, 0.2]]) + rng.uniform(-1, 1, 3)
            ref = est * (np.array([1.0, -1.0, 1.0]) if reflected else 1.0)
            ref = ref.dot(_rotz(rng.uniform(-np.pi, np.pi)).T) * rng.uniform(0.5, 2.0) + rng.uniform(-2, 2, 3)
            ref = ref + rng.standard_normal(ref.shape) * (0.0 if n <= 3 else 0.01)
            if n == 2:  # two points always lie on a line: A has rank 1 and cannot be compared
                lines.append((f"two_points_{int(reflected)}", est, ref, reflected))
                continue
            compared.append((f"walk{n}_{'mirrored' if reflected else 'plain'}", est, ref, reflected))
    for k, n in enumerate((5, 90)):
        t = np.linspace(0, 1, n)[:, None]
        d0, d1 = rng.standard_normal(3), rng.standard_normal(3)
        lines.append((f"line{n}", t * d0 + 0.3, 2 * t * d1 - 0.1, False))
    single.append(("single", rng.standard_normal((1, 3)), rng.standard_normal((1, 3)), False))
    return {"compared": compared, "lines": lines, "single": single}


# ---------------------------------------------------------------------------------------------- the stage-1 score
def quat_to_matrix(q):
    """pytorch3d's quaternion_to_matrix formula in numpy float64: q [..., 4] (w, x, y, z) -> [..., 3, 3]."""
    q = np.asarray(q, np.float64)
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s2 = 2.0 / (q * q).sum(-1)
    m = np.stack([1 - s2 * (j * j + k * k), s2 * (i * j - k * r), s2 * (i * k + j * r),
                  s2 * (i * j + k * r), 1 - s2 * (i * i + k * k), s2 * (j * k - i * r),
                  s2 * (i * k - j * r), s2 * (j * k + i * r), 1 - s2 * (i * i + j * j)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def head_pose_metrics_np(head_trans, head_rot, gt_head_trans, gt_head_rot):
    """egoego/eval/head_pose_metrics.py compute_head_pose_metrics restated: with homogeneous X = [Rp tp; 0 1], Y = [Rg tg; 0 1],
    X Y^-1 = [E, tp - E tg; 0 1] for E = Rp Rg^-1, so |I4 - X Y^-1|_F^2 = |I3 - E|_F^2 + |tp - E tg|^2.
    -> (head_dist, head_dist_rot_only, head_trans_err in mm), means over the frames."""
    tp, tg = np.asarray(head_trans, np.float64), np.asarray(gt_head_trans, np.float64)
    Rp, Rg = np.asarray(head_rot, np.float64), np.asarray(gt_head_rot, np.float64)
    E = np.einsum("tij,tjk->tik", Rp, np.linalg.inv(Rg))
    rot2 = ((np.eye(3)[None] - E) ** 2).sum((1, 2))
    tr2 = ((tp - np.einsum("tij,tj->ti", E, tg)) ** 2).sum(1)
    return (float(np.sqrt(rot2 + tr2).mean()), float(np.sqrt(rot2).mean()),
            float(np.sqrt(((tp - tg) ** 2).sum(1)).mean() * 1000))


def unit_quats(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, :1] < 0, -q, q)


def metric_poses(seed, B, T):
    """Seeded pose pairs [B, T, 7] (xyz + unit quaternion): a ground truth and a perturbed prediction."""
    rng = np.random.default_rng(seed)
    gt = np.concatenate([np.cumsum(rng.standard_normal((B, T, 3)) * 0.03, 1) + rng.uniform(-1, 1, (B, 1, 3)),
                         unit_quats(rng, B * T).reshape(B, T, 4)], -1)
    dq = unit_quats(rng, B * T).reshape(B, T, 4) * 0.2 + gt[..., 3:]
    dq /= np.linalg.norm(dq, axis=-1, keepdims=True)
    pred = np.concatenate([gt[..., :3] + rng.standard_normal((B, T, 3)) * 0.05, dq], -1)
    return pred, gt


# ---------------------------------------------------------------------------------------------- ragged stage-1 batches
def headnet_lengths(window):
    """Feature frames T per sequence around the block edges, and the pose frames L (T + 1; the fourth sequence has L = T)."""
    T = [1, window - 1, window, window + 1, 2 * window, 2 * window + 7]
    L = [t + 1 for t in T]
    L[3] = T[3]
    return T, L


def gravity_lengths(window):
    """SLAM frames L per sequence below, at and above window + 1, and reference lengths shorter and longer than them.  At least
    three frames are aligned: two points lie on a line, where the reference's rotation is arbitrary (see trajectory_cases)."""
    L = [3, window // 2, window, window + 1, window + 2, 2 * window + 5]
    R = [5, window // 2 + 3, window - 4, window + 1, window + 9, 2 * window]
    return L, R


def pad(rows, width=None, fill=0.0):
    """list of [n_b, ...] arrays -> [B, max n_b (or width), ...] padded with `fill`."""
    width = max(len(r) for r in rows) if width is None else width
    out = np.full((len(rows), width) + rows[0].shape[1:], fill, rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def stage1_sequences(seed, T, L):
    """Per sequence b: features [T_b, 512] fp32, a ground-truth head pose, an aligned SLAM walk, the original SLAM translation
    and rotation, all of L_b frames -> dict of lists."""
    rng = np.random.default_rng(seed)
    d = {k: [] for k in ("of", "head_pose", "aligned_slam_trans", "ori_slam_trans", "ori_slam_rot_mat")}
    for t, l in zip(T, L):
        d["of"].append(rng.standard_normal((t, 512)).astype(np.float32))
        hp = np.zeros((l, 7), np.float32)
        hp[:, :3] = np.cumsum(rng.standard_normal((l, 3)) * 0.02, 0)
        hp[:, 3:] = unit_quats(rng, l)
        d["head_pose"].append(hp)
        d["aligned_slam_trans"].append(np.cumsum(rng.standard_normal((l, 3)) * 0.03, 0).astype(np.float32))
        d["ori_slam_trans"].append(np.cumsum(rng.standard_normal((l, 3)) * 0.03, 0).astype(np.float32))
        d["ori_slam_rot_mat"].append(O.quat2mat(unit_quats(rng, l)).astype(np.float32))
    return d


def padded_batch(seqs, rows=None, extra=0, fill=0.0):
    """The sequences `rows` (None: all) of stage1_sequences' lists as one padded batch of CPU tensors; `extra` more padded frames
    than the longest needs; padded frames hold `fill`."""
    rows = range(len(next(iter(seqs.values())))) if rows is None else rows
    out = {}
    for k, v in seqs.items():
        sel = [v[b] for b in rows]
        out[k] = torch.from_numpy(pad(sel, max(len(r) for r in sel) + extra, fill))
    return out
