"""The rotation and length edges the body model, the evaluation and the AMASS head tracks are tested at (CPU, numpy): one set of
cases, shared by tests/test_rotation_edge_cases.py (the builders' margins, the oracles against independent references, planted
defects) and the three GPU files test_gpu_body_edges.py, test_gpu_evaluate_edges.py and test_gpu_amass_edges.py.

  axis_angles()      float32 axis-angle vectors: 13 magnitudes (zero, both sides of the a^2 < 1e-12 series switch of quat_f64.h,
                     pi, 2 pi and beyond) x 6 axes
  fk_chains()        22-joint local poses whose composed rotation passes pi and 2 pi along the spine and down a leg, so that the
                     sign standardisation of the evaluation's FK runs
  head_rotations()   float32 head rotation matrices on which each of matrix_to_quaternion's four candidates wins
  head_sequences()   those matrices ordered into sequences of 1, 2 and 40 frames with a head position walk
  metric_inputs()    joint walks and non-unit, negated, zero and tiny quaternions at lengths around the 64-lane wave and the
                     256-thread stride of the metrics kernel, and below 3 frames

Every builder asserts the margins that make the comparison at its cases no coin toss; nothing is filtered when a test runs.
"""
import functools
import math

import numpy as np

MAGNITUDES = (0.0, 1e-30, 1e-9, 9.99e-7, 1.0001e-6, 1e-4, math.pi - 1e-6, float(np.float32(math.pi)), math.pi + 1e-6,
              2 * math.pi - 1e-6, float(np.float32(2 * math.pi)), 3 * math.pi, 7.0)
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1 / math.sqrt(3),) * 3, (0.6, -0.8, 0.0), (0.36, 0.48, -0.8))
SMALL_ANGLE = 1e-4              # the magnitudes up to here make a "small-angle" frame
SPINE = (0, 3, 6, 9, 12, 15)    # root -> head
LEG = (0, 1, 4, 7, 10)          # root -> left toe
METRIC_LENGTHS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 513)
METRIC_T = 520
PAD = 7.5                       # what the padded frames hold (test_gpu_evaluate._pad)


_RECORD = {}


def record(case, **figures):
    """EGOEGO_EDGES_RECORD=<file>: every figure the three GPU files measure, with its bar, is written there as JSON, one entry per
    case (profiles/rotation_edges_error.json is such a file, from one pytest run over the three files)."""
    import json
    import os
    path = os.environ.get("EGOEGO_EDGES_RECORD")
    if not path:
        return
    clean = lambda v: {k: clean(x) for k, x in v.items()} if isinstance(v, dict) else (  # noqa: E731
        [clean(x) for x in v] if isinstance(v, (list, tuple)) else (v if isinstance(v, (str, bool, int)) or v is None else float("%.4g" % v)))
    _RECORD.setdefault(case, {}).update(clean(figures))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def axis_angles():
    """-> float32 [78, 3]: MAGNITUDES x AXES, magnitude-major (row 6 m + a), each rounded once from fp64."""
    return (np.asarray(MAGNITUDES)[:, None, None] * np.asarray(AXES)[None]).reshape(-1, 3).astype(np.float32)


def small_angle_rows():
    """The rows of axis_angles() whose magnitude is <= SMALL_ANGLE."""
    return np.flatnonzero(np.repeat(np.asarray(MAGNITUDES) <= SMALL_ANGLE, len(AXES)))


def _rot(axis, angle):
    """fp64 rotation matrix of a unit axis and an angle well away from zero, by the closed formula."""
    x, y, z = axis
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], np.float64)
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


# ------------------------------------------------------------------------------------------------ body model, AMASS joints
BODY_EDGE_JOINTS = (0, 2, 9, 16, 21, 25, 51)  # the root, four body joints, a joint of each hand
AMASS_EDGE_JOINTS = (0, 3, 12, 15)            # the root and the spine up to the head, whose global rotation is an output


@functools.lru_cache(maxsize=None)
def body_edge_poses():
    """-> dict(aa float32 [1092, 52, 3], trans float32 [1092, 3], edge [1092] bool, small [1092] bool).  Even frames: vector v of
    axis_angles() on joint j of BODY_EDGE_JOINTS (frame 2 (7 v + k)), every other joint at rest, so that a frame whose vector is
    small has every angle <= SMALL_ANGLE (`small`); odd frames: synthetic.make_body_poses, which give the project's figure (max
    |error| / max |fp64| over the call) its ordinary denominator."""
    from egoego_release_amd.synthetic import make_body_poses
    vec = axis_angles()
    n = vec.shape[0] * len(BODY_EDGE_JOINTS)
    aa, trans = make_body_poses(2 * n, 52, seed=71)
    edge = np.arange(2 * n) % 2 == 0
    small = np.zeros(2 * n, bool)
    aa[edge] = 0
    is_small = np.isin(np.arange(vec.shape[0]), small_angle_rows())
    for i in range(vec.shape[0]):
        for k, j in enumerate(BODY_EDGE_JOINTS):
            f = 2 * (len(BODY_EDGE_JOINTS) * i + k)
            aa[f, j] = vec[i]
            small[f] = is_small[i]
    assert small.sum() == 6 * len(AXES) * len(BODY_EDGE_JOINTS)
    assert np.linalg.norm(aa[small].astype(np.float64), axis=-1).max() <= SMALL_ANGLE * (1 + 1e-6)
    return {"aa": aa, "trans": trans, "edge": edge, "small": small}


@functools.lru_cache(maxsize=None)
def amass_joint_poses():
    """-> dict(root_orient float32 [312, 3], pose_body [312, 63], trans [312, 3]): vector v of axis_angles() on joint j of
    AMASS_EDGE_JOINTS (frame 4 v + k), rotations of up to 0.5 rad on the other joints."""
    from egoego_release_amd.synthetic import make_body_poses
    vec = axis_angles()
    aa, trans = make_body_poses(vec.shape[0] * len(AMASS_EDGE_JOINTS), 22, seed=72, amplitude=0.5)
    for i in range(vec.shape[0]):
        for k, j in enumerate(AMASS_EDGE_JOINTS):
            aa[len(AMASS_EDGE_JOINTS) * i + k, j] = vec[i]
    return {"root_orient": aa[:, 0].copy(), "pose_body": aa[:, 1:].reshape(-1, 63).copy(), "trans": trans}


# ------------------------------------------------------------------------------------------------ evaluation FK
@functools.lru_cache(maxsize=None)
def fk_chains():
    """-> dict(local_aa float32 [N, 22, 3], root_trans float32 [N, 3], rest_offsets, parents, flips: the number of (frame, joint)
    pairs whose unstandardised global product has w < 0, min_w: the smallest |w| of any local or global quaternion).

    Frames 0 .. 78 x 22 - 1: vector v of axis_angles() on joint j, gentle rotations (<= 0.3 rad) on the others.  Then the chains:
    per axis, per chain (SPINE, LEG) and per step 0.9, 1.1, 1.3 rad the root turns 2.5 rad and every chain joint `step` about the
    same axis, so the composed angle of joint k is 2.5 + k step: past pi from k = 1, past 2 pi from k = 3 or 4."""
    import eval_oracle as O
    from egoego_release_amd import synthetic as S
    g = np.random.default_rng(20)
    vec = axis_angles()
    frames = []
    for v in vec:
        for j in range(22):
            f = g.uniform(-1, 1, (22, 3)) * (0.3 / math.sqrt(3))
            f[j] = v
            frames.append(f)
    for ax in AXES:
        for chain in (SPINE, LEG):
            for step in (0.9, 1.1, 1.3):
                f = g.uniform(-1, 1, (22, 3)) * (0.3 / math.sqrt(3))
                f[0] = 2.5 * np.asarray(ax)
                for j in chain[1:]:
                    f[j] = step * np.asarray(ax)
                frames.append(f)
    aa = np.stack(frames).astype(np.float32)
    root = (g.standard_normal((aa.shape[0], 3)) * 1.5).astype(np.float32)
    rest, parents = np.asarray(S.EVAL_REST_OFFSETS, np.float32), np.asarray(S.EVAL_PARENTS)
    gq, gp = O.fk(root, aa, rest, parents)
    # the local quaternions and the unstandardised products, as O.fk forms them
    a64 = aa.astype(np.float64)
    ang = np.linalg.norm(a64, axis=-1, keepdims=True)
    lq = np.concatenate([np.cos(ang / 2), np.where(ang < 1e-12, 0.5, np.sin(ang / 2) / np.where(ang < 1e-12, 1.0, ang)) * a64], -1)
    raw_w = np.stack([O._q_mul(gq[:, parents[j]], O._std(lq[:, j]))[:, 0] for j in range(1, 22)], 1)
    flips = int((raw_w < 0).sum())
    min_w = float(min(np.abs(gq[..., 0]).min(), np.abs(lq[..., 0]).min()))
    assert flips >= 20, flips
    assert (lq[..., 0] < 0).sum() >= 20  # ... and the local quaternion's own flip (angles past pi)
    assert min_w >= 1e-9, min_w  # two fp64 implementations agree on the sign of such a w
    err = np.abs(gp - S.eval_fk(root, aa, rest, parents)).max()
    assert err <= 1e-12, err
    return {"local_aa": aa, "root_trans": root, "rest_offsets": rest, "parents": parents, "flips": flips, "min_w": min_w,
            "oracle_quat": gq, "oracle_jpos": gp}


# ------------------------------------------------------------------------------------------------ AMASS head tracks
def _candidates(R):
    """matrix_to_quaternion's four |components| x 2 of fp64 matrices [..., 3, 3] -> [..., 4]"""
    m = lambda i, j: R[..., i, j]  # noqa: E731
    return np.sqrt(np.maximum(np.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2),
                                        1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2)], -1), 0.0))


HALF_TURNS = (np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]))


@functools.lru_cache(maxsize=None)
def head_rotations():
    """-> dict(R float32 [25, 3, 3], names, winner [25]: the candidate matrix_to_quaternion takes on each).

    identity; the three exact half turns; 2.6, 2.85 and 3.1 rad about e_x, e_y, e_z tilted by 0.2 rad (towards e_z, e_z, e_x: a
    head that lies on its side still has a heading); eight generic rotations with w in 0.05 .. 0.3; four gentle ones (0.3 .. 1.2
    rad), so that candidate 0 wins on more than the identity."""
    import amass_oracle as A
    g = np.random.default_rng(31)
    mats, names = [np.eye(3)], ["identity"]
    for k, H in enumerate(HALF_TURNS):
        mats.append(H)
        names.append("half_turn_" + "xyz"[k])
    tilt = {0: 2, 1: 2, 2: 0}
    for k in range(3):
        axis = np.zeros(3)
        axis[k], axis[tilt[k]] = math.cos(0.2), math.sin(0.2)
        for angle in (2.6, 2.85, 3.1):
            mats.append(_rot(axis, angle))
            names.append("near_pi_%s_%.2f" % ("xyz"[k], angle))
    for i, w in enumerate(np.linspace(0.05, 0.3, 8)):
        # a seeded axis whose largest component leads the next by a clear margin
        while True:
            axis = g.standard_normal(3)
            axis /= np.linalg.norm(axis)
            top = np.sort(np.abs(axis))
            if top[2] - top[1] >= 0.1:
                break
        mats.append(_rot(axis, 2 * math.acos(w)))
        names.append("generic_w_%.3f" % w)
    for i, angle in enumerate((0.3, 0.6, 0.9, 1.2)):
        axis = g.standard_normal(3)
        mats.append(_rot(axis / np.linalg.norm(axis), angle))
        names.append("gentle_%.1f" % angle)
    R32 = np.stack(mats).astype(np.float32)
    R = R32.astype(np.float64)
    qa = _candidates(R)
    winner = qa.argmax(-1)
    order = np.sort(qa, -1)
    q = A.matrix_to_quaternion(R)
    exact_half = np.array([n.startswith("half_turn") for n in names])
    assert all((winner == k).sum() >= 3 for k in range(4)), np.bincount(winner, minlength=4)
    assert (order[~exact_half, 3] - order[~exact_half, 2]).min() >= 1e-3
    assert (q[exact_half, 0] == 0).all() and np.abs(q[~exact_half, 0]).min() >= 1e-3
    assert np.array_equal(R32[1:4], np.stack(HALF_TURNS).astype(np.float32))
    return {"R": R32, "names": names, "winner": winner}


def _walk(g, n, start):
    step = g.standard_normal((n, 3))
    step = 0.02 * step / np.linalg.norm(step, axis=1, keepdims=True)
    step[0] = 0
    return (np.asarray(start) + np.cumsum(step, 0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def head_sequences():
    """-> a list of three dicts, one per sequence of 1, 2 and 40 frames: rot float32 [T, 3, 3] (rows of head_rotations()), index
    [T] (which), joints float32 [T, 22, 3] before the floor shift (the head joint walks in 2 cm steps), floor (float32), pos
    float32 [T, 3] (the head joint with the floor taken off z in float32, as the kernel and the reference do), qpos32 float32
    [T, 7] (pos and the oracle's quaternion rounded to float32: what the reference's get_head_vel is handed), r0 [T - 1] (the
    standardised relative w of each pair, from qpos32), flipped [T - 1] (the pair's raw relative w was negative).

    The 1-frame sequence is the half turn about x and the 2-frame sequence ends on the half turn about y: both have w = z = 0,
    no heading, and may only ever be a pair's next frame.  The 40-frame sequence opens identity -> 3.1 rad -> identity ... (pairs
    3.1 rad apart) and goes on through the other matrices in a seeded order, some repeated in place (the `same` branch)."""
    import amass_oracle as A
    import eval_oracle as O
    hr = head_rotations()
    names = hr["names"]
    ix = {n: i for i, n in enumerate(names)}
    rest = [i for i, n in enumerate(names) if n not in ("identity", "half_turn_x", "half_turn_y", "near_pi_x_3.10", "near_pi_y_3.10",
                                                        "near_pi_z_3.10")]
    q_all = A.matrix_to_quaternion(hr["R"].astype(np.float64)).astype(np.float32).astype(np.float64)

    def pairs_of(order):
        cur, nxt = q_all[order[:-1]], q_all[order[1:]]
        raw = O._q_mul(nxt, cur * np.array([1.0, -1.0, -1.0, -1.0]))[:, 0]
        ident = np.array([np.array_equal(hr["R"][a], hr["R"][b]) for a, b in zip(order[:-1], order[1:])], bool)
        heading = np.sqrt(cur[:, 0] ** 2 + cur[:, 3] ** 2)
        return raw, ident, heading

    def fine(order):
        raw, ident, heading = pairs_of(order)
        r0 = np.abs(raw)
        return bool(np.all(heading >= 0.1) and np.all(np.where(ident, np.abs(1 - r0) < 2.5e-7, (r0 >= 1e-3) & (r0 <= 1 - 3e-6))))

    head = [ix["identity"], ix["near_pi_x_3.10"], ix["identity"], ix["near_pi_y_3.10"], ix["identity"], ix["near_pi_z_3.10"]]
    order40 = None
    for seed in range(200):  # the first seeded order that meets the pair conditions (they are asserted below, whatever this finds)
        g = np.random.default_rng([41, seed])
        tail = list(g.permutation(rest)) + list(g.permutation(rest)[:9])
        order = head + tail
        for at in sorted(g.choice(np.arange(5, len(order)), 6, replace=False), reverse=True):
            order.insert(at + 1, order[at])  # repeated in place: a bit-identical pair
        if len(order) == 40 and fine(np.asarray(order)):
            order40 = np.asarray(order)
            break
    assert order40 is not None
    orders = [np.asarray([ix["half_turn_x"]]), np.asarray([ix["generic_w_0.300"], ix["half_turn_y"]]), order40]
    assert set(np.concatenate(orders)) == set(range(len(names)))  # every matrix is in some sequence
    g = np.random.default_rng(43)
    out = []
    for b, order in enumerate(orders):
        T = order.size
        joints = (g.standard_normal((T, 22, 3)) * 0.4 + np.array([0.0, 0.0, 1.0])).astype(np.float32)
        joints[:, A.HEAD] = _walk(g, T, (0.3 - 0.1 * b, -0.2, 1.6))
        floor = np.float32((-0.0123, 0.0, 0.0456)[b])
        pos = joints[:, A.HEAD].copy()
        pos[:, 2] = pos[:, 2] - floor  # float32 arithmetic
        qpos32 = np.concatenate([pos, q_all[order].astype(np.float32)], 1)
        seq = {"rot": hr["R"][order], "index": order, "joints": joints, "floor": floor, "pos": pos, "qpos32": qpos32}
        if T > 1:
            raw, ident, heading = pairs_of(order)
            r0 = np.abs(raw)
            assert fine(order)
            angles = [math.acos(min(1.0, max(-1.0, (np.trace(a.T.astype(np.float64) @ b.astype(np.float64)) - 1) / 2)))
                      for a, b, same in zip(seq["rot"][:-1], seq["rot"][1:], ident) if not same]
            assert min(angles) >= 0.008  # the existing golden's condition (amass_oracle.assert_head_conditions)
            seq.update(r0=r0, flipped=raw < 0, identical=ident, heading=heading)
        out.append(seq)
    long = out[2]
    assert long["identical"].sum() == 6 and (2 * np.arccos(long["r0"][~long["identical"]]) > 3.0).sum() >= 6
    assert long["flipped"].sum() >= 5 and (~long["flipped"]).sum() >= 5  # both sides of qrel's sign standardisation
    return out


# ------------------------------------------------------------------------------------------------ evaluation metrics
def metric_oracle(inputs=None):
    """eval_oracle.metrics of every sample of metric_inputs() -> [B, 13 + 22] fp64: METRIC_KEYS, then single_jpe.  NaN where the
    reference takes the mean of no frames (accel_* below 3 frames)."""
    import warnings

    import eval_oracle as O
    m = metric_inputs() if inputs is None else inputs
    rows = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)  # "Mean of empty slice": that NaN is the expected value
        for b, L in enumerate(m["lengths"]):
            r = O.metrics(m["gt_quat"][b, :L], m["gt_jpos"][b, :L], m["gt_floor"][b], m["pred_quat"][b, :L], m["pred_jpos"][b, :L],
                          m["pred_floor"][b])
            rows.append(np.concatenate([[r[k] for k in O.METRIC_KEYS], r["single_jpe"]]))
    return np.asarray(rows, np.float64)


RESIDUE = 1e-12  # an fp64 value below this is rounding residue (the identical sample's distances): the smallest other value is 1e-6


def metric_figures(got, want, bound):
    """One sample's row against the oracle's -> {key: (figure, bar)}: the relative error against bound[key]; where the oracle's
    value is below RESIDUE, |got| against RESIDUE; where it is NaN, 0 if `got` is NaN too and inf if not.  single_jpe is the worst
    of its 22 entries."""
    import eval_oracle as O
    out = {}

    def one(g, w, bar):
        if np.isnan(w):
            return (0.0 if np.isnan(g) else np.inf), bar
        if abs(w) < RESIDUE:
            return (abs(g) if np.isfinite(g) else np.inf), RESIDUE
        return (abs(g - w) / abs(w) if np.isfinite(g) else np.inf), bar

    for i, k in enumerate(O.METRIC_KEYS):
        out[k] = one(got[i], want[i], bound[k])
    n = len(O.METRIC_KEYS)
    cells = [one(got[n + j], want[n + j], bound["single_jpe"]) for j in range(22)]
    out["single_jpe"] = max(cells, key=lambda c: c[0] / c[1])
    return out


FOOT_JOINTS = ((7, 0.08), (10, 0.04), (8, 0.08), (11, 0.04))  # compute_foot_sliding_for_smpl's ankles and toes with their heights


@functools.lru_cache(maxsize=None)
def metric_inputs():
    """-> dict of float32 arrays padded to METRIC_T with PAD: pred_jpos, gt_jpos [B, T, 22, 3], pred_quat, gt_quat [B, T, 22, 4],
    pred_floor, gt_floor [B], lengths [B]; B = 12: one sample per length of METRIC_LENGTHS and `identical` (= 11), a 65-frame
    sample whose prediction is its ground truth bit for bit.

    Quaternions start as unit ones; then every frame is scaled by 0.25 or 4, every third is negated, frames 3 and 4 (mod 11) of
    the prediction (5 and 6 of the ground truth) get norm^2 = 1e-16 (the identity branch of quaternion_matrix) and 1e-15
    (normalised), and frames 1 (mod 7) of the prediction and 2 (mod 7) of the ground truth are exact zeros.  The ankles and toes
    sit 1 m under the floor, within 0.01 m of their contact heights on either side, or well above, by a seeded choice per frame."""
    g = np.random.default_rng(57)
    lengths = list(METRIC_LENGTHS) + [65]
    B, T = len(lengths), METRIC_T
    from egoego_release_amd import synthetic
    skel = np.zeros((22, 3))
    for j in range(1, 22):
        skel[j] = skel[synthetic.EVAL_PARENTS[j]] + np.asarray(synthetic.EVAL_REST_OFFSETS[j], np.float64)
    out = {k: np.full((B, T, 22, w), PAD, np.float32) for k, w in (("pred_jpos", 3), ("gt_jpos", 3), ("pred_quat", 4), ("gt_quat", 4))}
    out["pred_floor"] = g.uniform(-0.02, 0.02, B).astype(np.float32)
    out["gt_floor"] = g.uniform(-0.02, 0.02, B).astype(np.float32)
    out["lengths"] = np.asarray(lengths, np.int32)
    out["identical"] = B - 1

    def walk(L, floor):
        root = np.cumsum(g.standard_normal((L, 3)) * 0.02, 0) + np.array([0.0, 0.0, 0.95])
        j = root[:, None] + skel[None] + g.standard_normal((L, 22, 3)) * 0.03
        for idx, H in FOOT_JOINTS:
            kind = g.integers(0, 4, L)
            near = H + g.choice([-1.0, 1.0], L) * g.uniform(0.001, 0.01, L)
            j[:, idx, 2] = float(floor) + np.where(kind == 0, -1.0, np.where(kind == 3, 0.2, near))
        return j.astype(np.float32)

    def quats(L, zero_at, tiny_at):
        q = g.standard_normal((L, 22, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        t = np.arange(L)
        scale = g.choice([0.25, 4.0], L)
        scale[t % 11 == tiny_at] = 1e-8
        scale[t % 11 == tiny_at + 1] = math.sqrt(1e-15)
        scale[t % 3 == 2] *= -1
        q = (q * scale[:, None, None]).astype(np.float32)
        q[t % 7 == zero_at] = 0
        return q

    for b, L in enumerate(lengths):
        out["pred_jpos"][b, :L] = walk(L, out["pred_floor"][b])
        out["gt_jpos"][b, :L] = walk(L, out["gt_floor"][b])
        out["pred_quat"][b, :L] = quats(L, 1, 3)
        out["gt_quat"][b, :L] = quats(L, 2, 5)
    b = out["identical"]
    out["gt_jpos"][b], out["gt_quat"][b], out["gt_floor"][b] = out["pred_jpos"][b], out["pred_quat"][b], out["pred_floor"][b]
    # margins: no foot within a relative 1e-4 of its height; the tiny quaternions well on their side of 4 eps
    for jp, fl in (("pred_jpos", "pred_floor"), ("gt_jpos", "gt_floor")):
        for b, L in enumerate(lengths):
            for idx, H in FOOT_JOINTS:
                z = out[jp][b, :L, idx, 2].astype(np.float64) - float(out[fl][b])
                assert np.abs(z - H).min() >= 1e-4 * H, (jp, b, idx)
    below = near = 0
    for k in ("pred_quat", "gt_quat"):
        for b, L in enumerate(lengths):
            n2 = (out[k][b, :L, [0, 15]].astype(np.float64) ** 2).sum(-1)
            lim = 4 * np.finfo(np.float64).eps
            assert not np.any((n2 > lim / 4) & (n2 < lim * 1.05)) and not np.any((n2 > 0) & (n2 < 0.9e-16))
            below += int(((n2 > 0) & (n2 < lim)).sum())
            near += int(((n2 >= lim) & (n2 < 2e-15)).sum())
    assert below >= 50 and near >= 50
    return out
