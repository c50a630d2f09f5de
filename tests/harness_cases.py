"""Seeded inputs for the four per-window harness kernels (egoego_convert_model_res, egoego_window_condition, egoego_window_prefix,
egoego_rot6d_to_matrix) at the rotations and shapes where they branch, and the fp64 oracle's answer for each.

Every input is built in float64, rounded ONCE to float32 (what the kernels and the float32 torch chains are given) and handed to
the oracle as the float64 view of those rounded values: the three sides see the same numbers.

Poses: every joint's local axis-angle is a draw from ANGLES x AXES x {+, -} — both sides of the 1e-6 small-angle threshold, and
angles near pi where matrix_to_quaternion leaves its w branch and w ~ 0; the root orientation cycles through identity and pi - 0.01
about x, y and z.  Head trajectories: first-frame headings up to pi - 0.05 either way (heading_quat's 1 + fx gets small towards -x),
pitches up to 1.45 (the forward direction's xy projection shrinks to 0.12).  Closer to either singularity the reference's own
formula loses digits (at a heading of pi - 0.01 its plain float32 chain is already 5e-6 off): such inputs say nothing about a kernel,
so the builders assert that there are none.

Two trees: the SMPL-H one with head 15, and a 22-joint chain with head 12 (the deepest composition there is; parents and head_idx
are inputs of the C ABI).
"""
import contextlib
import functools

import numpy as np
import torch
from scipy.spatial.transform import Rotation as Rot

from egoego_release_amd import harness
from oracle import harness_oracle as HO
from test_harness_golden import REST_OFFSETS

ANGLES = np.array([0.0, 1e-7, 3e-6, 1e-4, 0.5, np.pi / 2, 3.0, np.pi - 1e-3])
AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.6, 0.0, 0.8], [-0.48, 0.6, 0.64]], np.float64)
ROOT_ORIENTS = np.array([[0, 0, 0], [np.pi - 0.01, 0, 0], [0, np.pi - 0.01, 0], [0, 0, np.pi - 0.01]], np.float64)
RECOVER_Z = (0.0, np.pi / 2, 3.0, -3.1)
HEADINGS = (0.0, 1.0, np.pi / 2, 2.5, 3.0, np.pi - 0.05, -(np.pi - 0.05), -np.pi / 2)
PITCHES = (0.0, 1.2, 1.45)
ROLL = 0.3
MAX_HEADING = np.pi - 0.05
MIN_FORWARD_XY = 0.1
# window prefix: the key frame's head rotation is a PRODUCT of up to 13 drawn rotations, itself some 1e-7 rad off in float32, and the
# heading multiplies that by 1 / (the forward direction's xy length): already a factor 3 leaves the plain chain of the chain tree
# at 1.6e-6, next to the 2e-6 that a case group may cost it
MIN_FORWARD_XY_PREFIX = 0.5
T_POSE = 64
# the shapes the kernels are run at: rows / frames of the case batches ([4, 64] windows, [24, 120] head trajectories)
ALL = slice(None)
CONVERT_SLICES = {(1, 1): (slice(2, 3), slice(9, 10)), (4, 64): (ALL, ALL), (3, 41): (slice(1, 4), slice(23, 64))}
CONDITION_SLICES = {(24, 1): (ALL, slice(0, 1)), (24, 31): (ALL, slice(0, 31)), (5, 120): (slice(2, 24, 5), ALL)}
PREFIX_SHAPES = ((9, 64, 10), (9, 10, 10), (3, 64, 1), (70, 12, 1))
# what the plain float32 chain itself may be off the oracle for a case group to count as well-conditioned
E_PLAIN_LIMIT = {"angle": 2e-6, "root": 2e-6, "head": 2e-6, "pos": 2e-6, "6d": 2e-6, "recover": 5e-7}
TREES = {"smplh": (tuple(harness.SMPLH_PARENTS_22), 15), "chain": ((-1,) + tuple(range(21)), 12)}


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


def up(a):
    return np.asarray(a).astype(np.float64)


@contextlib.contextmanager
def head_index(head):
    """The float32 torch chains of harness.py read the head joint from the module's HEAD_IDX (the Python layer fixes 15); the
    second tree's head is another joint."""
    old = harness.HEAD_IDX
    harness.HEAD_IDX = head
    try:
        yield
    finally:
        harness.HEAD_IDX = old


def angle(aa_a, aa_b):
    """Rotation angle between two axis-angle arrays (insensitive to the sign ambiguity near pi)."""
    d = Rot.from_rotvec(up(aa_a).reshape(-1, 3)) * Rot.from_rotvec(up(aa_b).reshape(-1, 3)).inv()
    return np.abs(d.magnitude())


def up_to_sign(q_a, q_b):
    """Element-wise distance of two quaternion arrays, q and -q being one rotation."""
    a, b = up(q_a).reshape(-1, 4), up(q_b).reshape(-1, 4)
    return np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1))


def quat_branch(m):
    """Which of (w, x, y, z) matrix_to_quaternion divides by for the rotation matrices m [..., 3, 3]."""
    d0, d1, d2 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    return np.stack([1 + d0 + d1 + d2, 1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2], -1).argmax(-1)


def heading_and_forward(q0):
    """(heading [rad], length of the forward direction's xy projection) of the quaternions q0 [N, 4]."""
    f = HO.quat_mul_vec(q0, np.array([1.0, 0.0, 0.0]))
    return np.arctan2(f[:, 1], f[:, 0]), np.hypot(f[:, 0], f[:, 1])


def well_conditioned_heading(q0, min_forward_xy=MIN_FORWARD_XY):
    h, fxy = heading_and_forward(q0)
    return (np.abs(h) <= MAX_HEADING) & (fxy >= min_forward_xy)


def poses(seed, B=4, T=T_POSE):
    """(local axis-angle [B,T,22,3], root translation [B,T,3]), float64."""
    g = np.random.default_rng([int(seed), 0x9A5E])
    aa = AXES[g.integers(len(AXES), size=(B, T, 22))] * (ANGLES[g.integers(len(ANGLES), size=(B, T, 22))] * g.choice([-1.0, 1.0], size=(B, T, 22)))[..., None]
    k = np.arange(T) % 8  # half of the frames take the root orientation from ROOT_ORIENTS, the other half keep their draw
    for i, r in enumerate(ROOT_ORIENTS):
        aa[:, k == i, 0] = r
    return aa, g.standard_normal((B, T, 3))


def stats_around(pos, seed):
    """Seeded min/max statistics [22,3] that the positions pos [..., 22, 3] fit inside with 0.5 .. 1 to spare (ranges of a metre and more, like the
    real statistics: a narrow range only multiplies every error of the normalised positions); float32 values."""
    g = np.random.default_rng([int(seed), 0x57A7])
    p = pos.reshape(-1, 22, 3)
    return up(f32(p.min(0) - g.uniform(0.5, 1.0, (22, 3)))), up(f32(p.max(0) + g.uniform(0.5, 1.0, (22, 3))))


def skeletons(lo, hi, tree):
    """(the product's ds, the oracle's) over REST_OFFSETS with the tree's parents."""
    return harness.SkeletonStats(lo, hi, REST_OFFSETS, parents=TREES[tree][0]), HO.SkeletonOracle(lo, hi, REST_OFFSETS)


# ------------------------------------------------------------------------------------------ convert_model_res_to_data
@functools.lru_cache(maxsize=None)
def convert_case(tree, seed=0):
    """Model-space windows [4, 64, 198] whose answer is known: oracle FK of poses(), canonicalised by a rotation about z of
    RECOVER_Z[b], positions normalised, rotations as the first two matrix rows taken OFF the manifold (row 0 x 1.7,
    row 1 <- 0.6 row 1 + 0.3 row 0; Gram-Schmidt undoes both exactly)."""
    parents, head = TREES[tree]
    aa, root = poses(seed)
    B, T = aa.shape[:2]
    gq, gj = HO.SkeletonOracle(np.zeros(66), np.ones(66), REST_OFFSETS).fk(root.reshape(-1, 3), aa.reshape(-1, 22, 3), parents)
    gq, gj = gq.reshape(B, T, 22, 4), gj.reshape(B, T, 22, 3)
    rec = np.array([[np.cos(th / 2), 0.0, 0.0, np.sin(th / 2)] for th in RECOVER_Z]).reshape(B, 1, 1, 4)
    inv = np.broadcast_to(HO.quat_inv(rec), gq.shape)
    cj = HO.quat_mul_vec(inv, gj)
    six = HO.quat_to_mat(HO.std_mul(inv, gq))[..., :2, :].copy()
    six[..., 0, :] *= 1.7
    six[..., 1, :] = 0.6 * six[..., 1, :] + 0.3 * six[..., 0, :]
    lo, hi = stats_around(cj, seed)
    ds, dso = skeletons(lo, hi, tree)
    x = f32(np.concatenate([dso.norm(cj.reshape(-1, 22, 3)).reshape(B, T, 66), six.reshape(B, T, 132)], -1))
    assert np.abs(x[..., :66]).max() <= 1.0
    c = dict(tree=tree, parents=parents, head=head, ds=ds, dso=dso, lo=lo, hi=hi, x=x, rec=f32(rec),
             known_aa=aa, known_root=gj[:, :, 0], known_head=gj[:, :, head])
    c["aa"], c["root"], c["head_pos"] = HO.convert_model_res_to_data(dso, up(x), up(c["rec"]), parents, head)
    return c


def convert_branches(c):
    """Fractions of the four matrix_to_quaternion branches over (the window's global rotations, the un-canonicalised ones, the
    local ones), counted on the oracle's matrices, and the oracle's local rotation angles."""
    m = HO.rot6d_to_mat(up(c["x"])[..., 66:].reshape(c["x"].shape[:2] + (22, 6)))
    ori = HO.quat_to_mat(HO.std_mul(np.broadcast_to(up(c["rec"]), m.shape[:-2] + (4,)), HO.mat_to_quat(m)))
    loc = Rot.from_rotvec(c["aa"].reshape(-1, 3)).as_matrix()
    frac = [np.bincount(quat_branch(v).ravel(), minlength=4) / quat_branch(v).size for v in (m, ori, loc)]
    return frac, np.linalg.norm(c["aa"], axis=-1).ravel()


# ------------------------------------------------------------------------------------------ window condition
def oracle_condition(dso, p, q, head):
    """M:355-378 with numpy: (x_start [B,Tw,198], recover [B,1,1,4])."""
    b = p.shape[0]
    a_t, a_q, yrot = HO.rotate_at_frame_smplh(p, q, 0)
    mv = a_t[:, 0:1].copy()
    mv[:, :, 2] = 0
    want = np.zeros((b, p.shape[1], 198))
    want[:, :, 3 * head:3 * head + 3] = a_t - mv
    want[:, :, 66 + 6 * head:66 + 6 * head + 6] = HO.quat_to_mat(a_q)[..., :2, :].reshape(b, -1, 6)
    want[:, :, :66] = dso.norm(want[:, :, :66].reshape(-1, 22, 3)).reshape(b, -1, 66)
    return want, yrot


@functools.lru_cache(maxsize=None)
def condition_case(tree="smplh", seed=0, Tw=120):
    """Head trajectories [24, Tw]: one row per (heading, pitch) of the first frame, rolled by ROLL, then a smooth seeded walk
    (twice-summed small steps in rotation and position)."""
    head = TREES[tree][1]
    g = np.random.default_rng([int(seed), 0xC09D])
    hp = [(h, p) for h in HEADINGS for p in PITCHES]
    B = len(hp)
    r0 = Rot.from_euler("z", [h for h, _ in hp]) * Rot.from_euler("y", [-p for _, p in hp]) * Rot.from_euler("x", ROLL)
    turn = np.cumsum(np.cumsum(g.standard_normal((B, Tw, 3)) * 2e-3, 1), 1)
    turn -= turn[:, :1]
    quat = np.empty((B, Tw, 4))
    for b in range(B):
        qs = (r0[b] * Rot.from_rotvec(turn[b])).as_quat()
        quat[b] = np.concatenate([qs[:, 3:], qs[:, :3]], -1)
    pos = g.standard_normal((B, 1, 3)) + np.array([0.0, 0.0, 1.5]) + np.cumsum(np.cumsum(g.standard_normal((B, Tw, 3)) * 1e-3, 1), 1)
    pos, quat = f32(pos), f32(quat)
    canon, _, _ = HO.rotate_at_frame_smplh(up(pos), up(quat), 0)
    at_head = np.zeros((B, Tw, 22, 3))
    at_head[:, :, head] = canon - canon[:, :1] * np.array([1.0, 1.0, 0.0])
    lo, hi = stats_around(at_head, seed)
    ds, dso = skeletons(lo, hi, tree)
    c = dict(tree=tree, head=head, ds=ds, dso=dso, lo=lo, hi=hi, pos=pos, quat=quat)
    c["x_start"], c["recover"] = oracle_condition(dso, up(pos), up(quat), head)
    assert np.abs(c["x_start"][..., :66]).max() <= 1.0
    return c


# ------------------------------------------------------------------------------------------ window prefix
def oracle_prefix_parts(dso, aa, root, n_last, parents, head):
    """M:399-467 with numpy/scipy: (canonical joint positions [B,n_last,22,3] before normalisation, 6D [B,n_last,132], the key
    frames' head quaternions [B,4])."""
    B = aa.shape[0]
    gq, gj = dso.fk(root.reshape(-1, 3), aa.reshape(-1, 22, 3), parents)
    gq, gj = gq.reshape(B, -1, 22, 4)[:, -n_last:], gj.reshape(B, -1, 22, 3)[:, -n_last:]
    t_t, _, t_rec = HO.rotate_at_frame_smplh(gj[:, :, head], gq[:, :, head], 0)
    t_mv = t_t[:, 0:1].copy()
    t_mv[:, :, 2] = 0
    inv = np.broadcast_to(HO.quat_inv(t_rec), gq.shape)
    pj = HO.quat_mul_vec(inv, gj) - t_mv[:, :, None, :]
    return pj, HO.quat_to_mat(HO.std_mul(inv, gq))[..., :2, :].reshape(B, -1, 132), gq[:, 0, head]


def oracle_prefix(dso, aa, root, n_last, parents, head):
    pj, p6, _ = oracle_prefix_parts(dso, aa, root, n_last, parents, head)
    return np.concatenate([dso.norm(pj.reshape(-1, 22, 3)).reshape(pj.shape[0], -1, 66), p6], -1)


@functools.lru_cache(maxsize=None)
def prefix_case(tree, B, Tw, n_last, seed=0):
    """The first Tw frames of poses() for B rows.  The canonicalisation is about the HEAD's heading in frame Tw - n_last, which is
    wherever the drawn rotations compose to: a row whose key frame is nearer to a singularity than MAX_HEADING / MIN_FORWARD_XY_PREFIX is
    drawn again (from the next seed) until none is."""
    parents, head = TREES[tree]
    fk = HO.SkeletonOracle(np.zeros(66), np.ones(66), REST_OFFSETS)
    aa, root = (f32(v[:, :Tw]) for v in poses(seed, B))
    for attempt in range(1, 20):
        _, _, key = oracle_prefix_parts(fk, up(aa), up(root), n_last, parents, head)
        bad = ~well_conditioned_heading(key, MIN_FORWARD_XY_PREFIX)
        if not bad.any():
            break
        a2, r2 = (f32(v[:, :Tw]) for v in poses(seed + 1000 * attempt, B))
        aa[bad], root[bad] = a2[bad], r2[bad]
    pj, _, key = oracle_prefix_parts(fk, up(aa), up(root), n_last, parents, head)
    lo, hi = stats_around(pj, seed)
    ds, dso = skeletons(lo, hi, tree)
    c = dict(tree=tree, parents=parents, head=head, ds=ds, dso=dso, lo=lo, hi=hi, aa=aa, root=root, n_last=n_last, key_quat=key)
    c["prefix"] = oracle_prefix(dso, up(aa), up(root), n_last, parents, head)
    assert np.abs(c["prefix"][..., :66]).max() <= 1.0
    return c


# ------------------------------------------------------------------------------------------ rot6d
@functools.lru_cache(maxsize=None)
def rot6d_case(seed=0):
    """The 6D rows of convert_case("smplh") [5632, 6]: |a1| = 1.7, a2's component orthogonal to a1 0.6 long."""
    return np.ascontiguousarray(convert_case("smplh", seed)["x"][..., 66:].reshape(-1, 6))


ROT6D_EXACT = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [1, 0, 0, 2, 0, 0]], np.float32)


# ------------------------------------------------------------------------------------------ the yardstick
def bound(e_plain, largest):
    """What a kernel may be off the fp64 oracle: 4 x max(the plain float32 torch chain's own distance on the same inputs, one
    float32 ulp of the output's largest magnitude).  4: the kernel contracts to FMAs and calls the device's sinf / cosf / atan2f
    where torch calls its own; each side is one realisation of the rounding."""
    return 4.0 * max(float(e_plain), 2.0 ** -23 * float(largest))


def convert_distances(got, c, sl=(slice(None), slice(None))):
    """got = (aa, root, head) arrays for the rows/frames `sl` of convert case c -> {output: (distance from the oracle, largest
    magnitude of the oracle's output)}."""
    aa, root, head = (np.asarray(v) for v in got)
    o_aa, o_root, o_head = c["aa"][sl], c["root"][sl], c["head_pos"][sl]
    return {"angle": (angle(aa, o_aa).max(), np.linalg.norm(o_aa, axis=-1).max()),
            "root": (np.abs(up(root) - o_root).max(), np.abs(o_root).max()),
            "head": (np.abs(up(head) - o_head).max(), np.abs(o_head).max())}


def condition_distances(got, want):
    x, rec = (np.asarray(v) for v in got)
    w_x, w_rec = want
    return {"pos": (np.abs(up(x)[..., :66] - w_x[..., :66]).max(), np.abs(w_x[..., :66]).max()),
            "6d": (np.abs(up(x)[..., 66:] - w_x[..., 66:]).max(), np.abs(w_x[..., 66:]).max()),
            "recover": (up_to_sign(rec, w_rec).max(), 1.0)}


def prefix_distances(got, want):
    x = up(np.asarray(got))
    return {"pos": (np.abs(x[..., :66] - want[..., :66]).max(), np.abs(want[..., :66]).max()),
            "6d": (np.abs(x[..., 66:] - want[..., 66:]).max(), np.abs(want[..., 66:]).max())}


def plain_convert(c, sl=(slice(None), slice(None))):
    """The float32 torch chain (CPU path of harness.convert_model_res_to_data) on the rows/frames `sl`."""
    with head_index(c["head"]):
        return tuple(v.numpy() for v in harness.convert_model_res_to_data(c["ds"], torch.from_numpy(c["x"][sl]), c["rec"][sl[0]], parents=c["parents"]))


def plain_condition(c, pos, quat):
    with head_index(c["head"]):
        x, rec = harness._window_condition_torch(c["ds"], torch.from_numpy(pos), torch.from_numpy(quat))
    return x.numpy(), rec.numpy()


def plain_prefix(c):
    with head_index(c["head"]):
        return harness._window_prefix_torch(c["ds"], torch.from_numpy(c["aa"]), torch.from_numpy(c["root"]), c["n_last"], c["parents"]).numpy()
