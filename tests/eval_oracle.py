"""fp64 numpy restatement of the reference's evaluation step, written from the definitions (not from the library's kernels):

  fk                      fk_smpl, amass_diffusion_dataset.py:265-293
  dbscan_1d               sklearn's DBSCAN(eps, min_samples).fit(h.reshape(-1, 1)).labels_ on the sorted line
  floor_and_contacts      determine_floor_height_and_contacts, utils/data_utils/process_amass_dataset.py:160-338
  metrics                 compute_metrics_for_smpl, kinpoly/scripts/eval_metrics_imu_rec.py:66-107, 222-342
  evaluate_samples        eval_egoego.py:369-446

Velocities, distances and sums are fp64.  The medians alone follow the reference's arithmetic (np.median on float32 heights),
because floor_height is compared bit for bit.
"""
import numpy as np

JOINTS = {"hips": 0, "leftLeg": 4, "rightLeg": 5, "leftFoot": 7, "rightFoot": 8, "leftToeBase": 10, "rightToeBase": 11, "head": 15,
          "leftHand": 20, "rightHand": 21}
FLOOR_VEL_THRESH = CONTACT_VEL_THRESH = 0.005
FLOOR_HEIGHT_OFFSET = 0.01
CONTACT_TOE_HEIGHT_THRESH, CONTACT_ANKLE_HEIGHT_THRESH = 0.04, 0.08
TERRAIN_HEIGHT_THRESH = ROOT_HEIGHT_THRESH = 0.04
CLUSTER_SIZE_THRESH = 0.25
DB_EPS, DB_MIN_SAMPLES = 0.005, 3
METRIC_KEYS = ("root_dist", "root_rot_dist", "root_trans_dist", "head_dist", "head_rot_dist", "head_trans_dist", "mpjpe",
               "mpjpe_wo_hand", "accel_pred", "accel_gt", "accel_err", "pred_fs", "gt_fs")

# how far the reference's own float32 results lie from the fp64 oracle on the golden inputs, worst relative difference per key
# (printed by make_eval_golden.py); the GPU tests' bounds may not exceed 4 x these
REFERENCE_DISTANCE = {
    "root_dist": 1.205e-15, "root_rot_dist": 1.276e-15, "root_trans_dist": 8.451e-08, "head_dist": 2.026e-15, "head_rot_dist": 2.411e-15,
    "head_trans_dist": 7.644e-08, "mpjpe": 7.099e-08, "mpjpe_wo_hand": 2.549e-07, "accel_pred": 6.481e-08, "accel_gt": 1.586e-08,
    "accel_err": 8.769e-07, "pred_fs": 1.433e-07, "gt_fs": 3.309e-08, "single_jpe": 1.679e-06}


# ---------------------------------------------------------------- forward kinematics
def _q_mul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _q_apply(q, p):
    pq = np.concatenate([np.zeros_like(p[..., :1]), p], -1)
    conj = q * np.array([1.0, -1.0, -1.0, -1.0])
    return _q_mul(_q_mul(q, pq), conj)[..., 1:]


def _std(q):
    return np.where(q[..., :1] < 0, -q, q)


def quat_to_matrix(q):
    """The rotation of q / |q|; identity below |q|^2 = 4 eps, as the reference's quaternion_matrix (transformation.py:1346-1370).
    (np.where swaps (1, 0, 0, 0) in for such a row and leaves every other row's bits as they were.)"""
    q = np.asarray(q, np.float64)
    tiny = (q * q).sum(-1, keepdims=True) < 4 * np.finfo(np.float64).eps
    q = np.where(tiny, np.array([1.0, 0.0, 0.0, 0.0]), q)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def fk(root_trans, local_aa, rest_offsets, parents):
    """root_trans [N, 3], local_aa [N, 22, 3], rest_offsets [22, 3] -> (global quaternions [N, 22, 4] with w >= 0, joints [N, 22, 3])."""
    aa = np.asarray(local_aa, np.float64)
    ang = np.linalg.norm(aa, axis=-1, keepdims=True)
    safe = np.where(ang < 1e-12, 1.0, ang)
    lq = _std(np.concatenate([np.cos(ang / 2), np.where(ang < 1e-12, 0.5, np.sin(ang / 2) / safe) * aa], -1))
    rest = np.asarray(rest_offsets, np.float64).reshape(22, 3)
    N = aa.shape[0]
    gq, gp = [lq[:, 0]], [np.broadcast_to(rest[0], (N, 3))]
    for j in range(1, 22):
        p = int(parents[j])
        gp.append(_q_apply(gq[p], np.broadcast_to(rest[j], (N, 3))) + gp[p])
        gq.append(_std(_q_mul(gq[p], lq[:, j])))
    return np.stack(gq, 1), np.stack(gp, 1) + np.asarray(root_trans, np.float64)[:, None, :]


# ---------------------------------------------------------------- DBSCAN on a line
def dbscan_1d(h, eps=DB_EPS, min_samples=DB_MIN_SAMPLES):
    """Labels of sklearn's DBSCAN for 1-D points `h` (any order), by its definition on the sorted line: a point is core when at
    least min_samples points, itself included, lie within <= eps; cores chained by gaps <= eps form a cluster; clusters are numbered
    by the smallest input index among their cores; a non-core point within eps of a core is a border point of the lowest-numbered
    such cluster; the rest is noise (-1).  Differences are taken in fp64."""
    h = np.asarray(h, np.float64).reshape(-1)
    n = h.size
    labels = np.full(n, -1, np.int64)
    if n == 0:
        return labels
    order = np.argsort(h, kind="stable")
    s = h[order]
    lo = hi = 0
    core = np.zeros(n, bool)
    for i in range(n):
        while s[i] - s[lo] > eps:
            lo += 1
        hi = max(hi, i)
        while hi + 1 < n and s[hi + 1] - s[i] <= eps:
            hi += 1
        core[i] = hi - lo + 1 >= min_samples
    cores = np.flatnonzero(core)
    if cores.size == 0:
        return labels
    raw = np.full(n, -1, np.int64)  # cluster ids left to right
    k = -1
    prev = None
    for i in cores:
        if prev is None or s[i] - s[prev] > eps:
            k += 1
        raw[i] = k
        prev = i
    first = np.full(k + 1, n, np.int64)
    np.minimum.at(first, raw[cores], order[cores])
    number = np.empty(k + 1, np.int64)
    number[np.argsort(first)] = np.arange(k + 1)
    lab_sorted = np.full(n, -1, np.int64)
    lab_sorted[cores] = number[raw[cores]]
    for i in np.flatnonzero(~core):
        a = np.searchsorted(cores, i)  # the nearest cores either side are the only candidates closest in height
        cand = []
        for c in (cores[a - 1] if a > 0 else None, cores[a] if a < cores.size else None):
            if c is not None and abs(s[i] - s[c]) <= eps:
                cand.append(lab_sorted[c])
        # every core within eps counts, not only the nearest: walk outwards while still within eps
        j = a - 2
        while j >= 0 and s[i] - s[cores[j]] <= eps:
            cand.append(lab_sorted[cores[j]])
            j -= 1
        j = a + 1
        while j < cores.size and s[cores[j]] - s[i] <= eps:
            cand.append(lab_sorted[cores[j]])
            j += 1
        if cand:
            lab_sorted[i] = min(cand)
    labels[order] = lab_sorted
    return labels


# ---------------------------------------------------------------- floor height and contacts
def _velocity(seq):
    v = np.linalg.norm(seq[1:] - seq[:-1], axis=1)
    return np.append(v, v[-1])


def floor_and_contacts(body_joint_seq, fps):
    """body_joint_seq [T, 22, 3] (float32 as the reference receives it; T >= 2) -> a dict: floor_height (np.float32),
    offset_floor_height, contacts [T, 22], discard_seq, labels (per static sample in the reference's order), n_groups,
    static_heights, static_inds, and the quantities a threshold is applied to (for margin checks): velocities [8, T],
    group_medians, group_root_medians, group_sizes."""
    x32 = np.asarray(body_joint_seq, np.float32)
    x = x32.astype(np.float64)
    T = x.shape[0]
    names = ("leftToeBase", "rightToeBase", "leftFoot", "rightFoot", "leftHand", "rightHand", "leftLeg", "rightLeg")
    vel = np.stack([_velocity(x[:, JOINTS[n]]) for n in names])
    stat_l, stat_r = vel[0] < FLOOR_VEL_THRESH, vel[1] < FLOOR_VEL_THRESH
    frames = np.arange(T)
    heights = np.append(x32[stat_l, JOINTS["leftToeBase"], 2], x32[stat_r, JOINTS["rightToeBase"], 2])  # float32
    inds = np.append(frames[stat_l], frames[stat_r])
    root_h = x32[:, 0, 2]
    out = {"velocities": vel, "static_heights": heights, "static_inds": inds}
    discard = False
    medians, root_medians, sizes = [], [], []
    if heights.size > 0:
        labels = dbscan_1d(heights)
        for lab in np.unique(labels):
            sel = labels == lab
            medians.append(np.median(heights[sel]))
            sizes.append(int(sel.sum()))
            root_medians.append(np.median(root_h[np.unique(inds[sel])]))
        best = int(np.argmin(medians))  # the first smallest, as the reference's strict <
        floor_height = medians[best]
        offset = np.float32(floor_height) - np.float32(FLOOR_HEIGHT_OFFSET)
        for rm, m, sz in zip(root_medians, medians, sizes):
            if rm > root_medians[best] + np.float32(ROOT_HEIGHT_THRESH) and m > floor_height + np.float32(TERRAIN_HEIGHT_THRESH) \
                    and sz > int(CLUSTER_SIZE_THRESH * fps):
                discard = True
                break
    else:
        labels = np.zeros(0, np.int64)
        floor_height, offset = np.float32(0.0), np.float32(0.0)
    contacts = np.zeros((T, 22))
    rel = x32[:, :, 2] - np.float32(floor_height)
    for k, n in enumerate(names):
        thr = CONTACT_TOE_HEIGHT_THRESH if k < 2 else CONTACT_ANKLE_HEIGHT_THRESH
        contacts[:, JOINTS[n]] = np.logical_and(vel[k] < CONTACT_VEL_THRESH, rel[:, JOINTS[n]] < np.float32(thr))
    out.update(floor_height=np.float32(floor_height), offset_floor_height=offset, contacts=contacts, discard_seq=bool(discard),
               labels=labels, n_groups=len(medians), group_medians=np.asarray(medians, np.float32),
               group_root_medians=np.asarray(root_medians, np.float32), group_sizes=np.asarray(sizes, np.int64),
               contact_heights=rel)
    return out


# ---------------------------------------------------------------- metrics
def _pose_matrices(pos, quat):
    n = pos.shape[0]
    m = np.zeros((n, 4, 4))
    m[:, :3, :3] = quat_to_matrix(quat)
    m[:, :3, 3] = pos
    m[:, 3, 3] = 1.0
    return m


def _frobenius(x, y, rot_only=False):
    if rot_only:
        x, y = x[:, :3, :3], y[:, :3, :3]
    err = np.eye(x.shape[-1]) - x @ np.linalg.inv(y)
    return np.sqrt((err ** 2).sum((1, 2))).mean()


def _accel(j):
    a = j[:-2] - 2 * j[1:-1] + j[2:]
    return np.linalg.norm(a, axis=2).mean(1)


def foot_sliding(jpos, floor_height):
    j = np.array(jpos, np.float64)
    T = j.shape[0]
    j[:, :, 2] -= float(floor_height)
    total = 0.0
    for idx, H in ((7, 0.08), (10, 0.04), (8, 0.08), (11, 0.04)):
        p = j[:, idx]
        disp = np.linalg.norm(p[1:, :2] - p[:-1, :2], axis=1)
        z = p[:-1, 2]
        total += np.abs(disp * (2 - 2 ** (z / H)))[z < H].sum() / T * 1000
    return total / 4.0


def metrics(gt_quat, gt_jpos, gt_floor_height, pred_quat, pred_jpos, pred_floor_height):
    """[T, 22, 4] / [T, 22, 3] each -> the reference's dictionary in fp64 (single_jpe as an array, plus jpe_0 .. jpe_21)."""
    gq, gp = np.asarray(gt_quat, np.float64), np.asarray(gt_jpos, np.float64)
    pq, pp = np.asarray(pred_quat, np.float64), np.asarray(pred_jpos, np.float64)
    res = {}
    for name, j in (("root", 0), ("head", JOINTS["head"])):
        mp, mg = _pose_matrices(pp[:, j], pq[:, j]), _pose_matrices(gp[:, j], gq[:, j])
        res[name + "_dist"] = _frobenius(mp, mg)
        res[name + "_rot_dist"] = _frobenius(mp, mg, rot_only=True)
        res[name + "_trans_dist"] = np.linalg.norm(pp[:, j] - gp[:, j], axis=1).mean() * 1000
    res["accel_pred"] = _accel(pp).mean() * 1000
    res["accel_gt"] = _accel(gp).mean() * 1000
    res["accel_err"] = np.linalg.norm((pp[:-2] - 2 * pp[1:-1] + pp[2:]) - (gp[:-2] - 2 * gp[1:-1] + gp[2:]), axis=2).mean(1).mean() * 1000
    res["pred_fs"] = foot_sliding(pp, pred_floor_height)
    res["gt_fs"] = foot_sliding(gp, gt_floor_height)
    err = np.linalg.norm((pp - pp[:, :1]) - (gp - gp[:, :1]), axis=2)
    res["mpjpe"] = err.mean() * 1000
    res["single_jpe"] = err.mean(0) * 1000
    res["mpjpe_wo_hand"] = res["single_jpe"][:18].mean()
    for i in range(22):
        res["jpe_%d" % i] = res["single_jpe"][i]
    return res


# ---------------------------------------------------------------- the driver
def evaluate_samples(rest_offsets, parents, local_aa, root_trans, gt_quat, gt_jpos, gt_floor_height=0.0, lengths=None, group=None,
                     fps=30):
    """local_aa [B, T, 22, 3], root_trans [B, T, 3], gt [T, ...] shared or [B, T, ...] -> per-sample metric dicts, floor heights
    and the best index per group.  FK is rounded to float32 once, as the library's output is, before anything is thresholded."""
    B, T = local_aa.shape[:2]
    lengths = [T] * B if lengths is None else [int(v) for v in lengths]
    group = [0] * B if group is None else [int(g) for g in group]
    gt_quat, gt_jpos = np.asarray(gt_quat), np.asarray(gt_jpos)
    res, floors = [], []
    for b in range(B):
        L = lengths[b]
        q, p = fk(root_trans[b, :L], local_aa[b, :L], rest_offsets, parents)
        q, p = q.astype(np.float32), p.astype(np.float32)
        gq = (gt_quat if gt_quat.ndim == 3 else gt_quat[b])[:L]
        gp = np.array((gt_jpos if gt_jpos.ndim == 3 else gt_jpos[b])[:L], np.float32)
        gp[:, :, :2] -= gp[0, JOINTS["head"], :2].copy()
        p[:, :, :2] -= p[0, JOINTS["head"], :2].copy()
        fc = floor_and_contacts(p, fps)
        floors.append(fc["offset_floor_height"])
        res.append(metrics(gq, gp, gt_floor_height, q, p, fc["offset_floor_height"]))
    return res, np.asarray(floors, np.float32), best_per_group([r["mpjpe"] for r in res], group)


def best_per_group(values, group):
    """eval_egoego.py:434-446: per group id the first sample with the smallest value, by the reference's strict < (a NaN that
    comes first stays, a later NaN never wins) -> {id: index}."""
    best = {}
    for b, v in enumerate(values):
        g = int(group[b])
        if g not in best or v < values[best[g]]:
            best[g] = b
    return best
