"""Seeded inputs for the motion-window kernels (egoego_win_build, egoego_win_stats, egoego_win_motion; csrc/motion_windows.h) at the
chunk lengths, first-frame headings and joint rotations where they branch, and the CPU preconditions under which the fp64 oracle
(tests/windows_oracle.py) is a fair yardstick for them.  Pure numpy / scipy: importable without a GPU.

Every input is built in float64 and rounded ONCE to float32, which is what the kernels, the oracle and the reference are given.

Poses: every joint's local axis-angle is a draw from ANGLES_ALL x AXES x {+, -}: harness_cases.ANGLES (both sides of
qd_from_aa's a2 < 1e-12 series threshold, angles up to pi - 1e-3) and three angles that raw AMASS data can hold and the harness
never sees: 4.0, 2 pi - 1e-3 and 7.0 (cos(a / 2) < 0: qd_std flips the quaternion; 7.0 is more than a full turn).  On top of the
draws every (angle, sign) is PLANTED on the root, on a joint of the head chain and on a leaf (holds_every_angle checks it).

Edge frames: a frame whose root orientation is solved so that the HEAD's global rotation is Rz(heading) Ry(-pitch) Rx(ROLL) while
the other 21 joints keep their draws.  The 21 (heading, pitch) pairs of HEADING_CASES go up to a heading of pi - 1e-3 (heading_of's
w = |f| + f.x falls to 5e-7) and a pitch of 1.52 (the head x-axis' horizontal projection falls to 0.05, where the reference's two
1e-8 terms are 2e-7 of it).  sequence() places them every `edge_every` frames, so that with edge_every = window // 2 every window
of the reference's rule starts on one.

Preconditions (check_window, asserted for every window that is emitted): the window is not degenerate (horizontal projection
>= 0.04, 1 + f.x >= 4e-7: at the exact degeneracy the reference itself returns NaN), and the oracle agrees with scipy_window — the
same window restated on scipy.spatial.transform.Rotation quaternions, composed down the tree with from_rotvec — to 1e-3 of the GPU
bound (2 float32 ulp of the output's largest magnitude).  Measured: the two fp64 paths differ by at most 1.2e-14 (1.1e-13 on the many-rows walk).
"""
import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import windows_oracle as WO
from harness_cases import ANGLES, AXES, ROLL, f32, up
from test_harness_golden import REST_OFFSETS
from test_motion_windows import ulp32

ANGLES_ALL = np.concatenate([ANGLES, [4.0, 2 * np.pi - 1e-3, 7.0]])
HEADINGS = (0.0, np.pi / 2, -np.pi / 2, 2.5, np.pi - 0.05, -(np.pi - 0.05), np.pi - 1e-3)
PITCHES = (0.0, 1.4, 1.52)
HEADING_CASES = tuple((h, p) for h in HEADINGS for p in PITCHES)
HEAD_CHAIN = (0, 3, 6, 9, 12, 15)
LEAVES = (10, 11, 20, 21)  # feet and hands (the head, 15, is a leaf as well: it counts with its chain)
ANGLE_GROUPS = {"root": (0,), "head chain": HEAD_CHAIN[1:], "leaf": LEAVES}
MIN_FORWARD_XY = 0.04
MIN_ONE_PLUS_FX = 4e-7
CHUNK_WINDOWS = (2, 63, 64, 65, 120, 121, 128, 129, 193, 480)
CHUNK_FRAMES = 512
CHUNK_EDGE_FRAMES = 31  # the windows of the chunk sweep start in the first 31 frames, all of them edge frames
CONTINUOUS = ("global_jpos", "global_rot_6d", "local_rot_6d", "recover_rot_quat")
MANY_FRAMES, MANY_WINDOW, MANY_MIN_FRAMES = 44000, 40, 30
MOTION_GRID_CAP_ROW = 84734  # win_motion_kernel: 65535 x 256 threads; from this row count on each thread takes a second element


def gpu_bound(want):
    """What a kernel output may be off the oracle's `want`: the kernels compute in fp64 and round once to float32."""
    return 2.0 * ulp32(want)


def up_to_sign(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    return np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1))


def chunk_lengths(W):
    return sorted({min(max(n, 0), W) for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W)})


def chunk_first(length):
    """Where the window of `length` frames starts in chunk_sequence(): a function of the length alone, so that the same frames
    are one window under every W."""
    return length % CHUNK_EDGE_FRAMES


# ------------------------------------------------------------------------------------------ poses
def pose_draws(seed, T, keep=()):
    """Local axis-angle [T, 22, 3] float64: seeded draws, then every (angle, sign) planted on the root, on one joint of the head
    chain below the root and on a leaf, in the frames that are not in `keep` (the edge frames, whose root is solved)."""
    g = np.random.default_rng([int(seed), 0x3D6E])
    aa = AXES[g.integers(len(AXES), size=(T, 22))] * (ANGLES_ALL[g.integers(len(ANGLES_ALL), size=(T, 22))] * g.choice([-1.0, 1.0], size=(T, 22)))[..., None]
    free = [t for t in range(T) if t not in set(keep)]
    slots = [(a, s) for a in ANGLES_ALL for s in (1.0, -1.0)]
    for k, (t, (a, s)) in enumerate(zip(free, slots)):
        for m, joints in enumerate(ANGLE_GROUPS.values()):
            aa[t, joints[k % len(joints)]] = AXES[(k + m) % len(AXES)] * a * s
    return aa


def holds_every_angle(root_orient, body_pose):
    """{(group, angle, sign)} that the float32 batch does NOT hold: empty when every angle of ANGLES_ALL appears with both signs
    about one of AXES on the root, on the head chain below the root and on a leaf."""
    aa = np.concatenate([up(root_orient).reshape(-1, 1, 3), up(body_pose).reshape(-1, 21, 3)], 1)
    missing = set()
    for group, joints in ANGLE_GROUPS.items():
        v = aa[:, list(joints)].reshape(-1, 3)
        proj = v @ AXES.T  # [n, axes]: the signed angle where v is along that axis
        norm = np.linalg.norm(v, axis=-1)[:, None]
        for a in ANGLES_ALL:
            for s in (1.0, -1.0):
                hit = (np.abs(norm - a) <= 1e-6 * a) & (np.abs(proj - s * a) <= 1e-6 * a)
                if not hit.any():
                    missing.add((group, float(a), s))
    return missing


def head_target(heading, pitch):
    return Rot.from_euler("z", heading) * Rot.from_euler("y", -pitch) * Rot.from_euler("x", ROLL)


def sequence(seed, T, edge_every, first_case=0, edge_until=None):
    """(trans [T, 3], root_orient [T, 3], body_pose [T, 63]) float32: pose_draws with an edge frame every `edge_every` frames below
    `edge_until` (default: everywhere), the k-th taking HEADING_CASES[(first_case + k) % 21], and a smooth seeded root walk."""
    edges = list(range(0, T if edge_until is None else edge_until, edge_every))
    aa = pose_draws(seed, T, keep=edges)
    for k, t in enumerate(edges):
        below = Rot.identity()
        for j in HEAD_CHAIN[1:]:
            below = below * Rot.from_rotvec(aa[t, j])
        aa[t, 0] = (head_target(*HEADING_CASES[(first_case + k) % len(HEADING_CASES)]) * below.inv()).as_rotvec()
    g = np.random.default_rng([int(seed), 0x7A45])
    trans = g.standard_normal(3) + np.array([0.0, 0.0, 1.0]) + np.cumsum(g.standard_normal((T, 3)) * 0.02, 0)
    return f32(trans), f32(aa[:, 0]), f32(aa[:, 1:].reshape(T, 63))


def heading_sequence(W, seed=0):
    """22 windows of the reference's rule at window W, the k-th starting on heading case k % 21: 21 full ones and a half one."""
    return sequence(seed, 22 * (W // 2), W // 2)


def angle_sequence(W, seed=1):
    """One and a half windows of the angle draws: three windows of the reference's rule (W, W and W // 2 frames)."""
    return sequence(seed, W + W // 2, W // 2, first_case=3)


def chunk_sequence(seed=2):
    return sequence(seed, CHUNK_FRAMES, 1, edge_until=CHUNK_EDGE_FRAMES)


def chunk_table(W):
    """Rows (sequence 0, start, end, length) for WO.build(table=): one window per length of chunk_lengths(W)."""
    return np.array([(0, chunk_first(n), chunk_first(n) + n, n) for n in chunk_lengths(W)], np.int64)


def turned(seq, angle=2.0, shift=(0.7, -0.4, 0.0)):
    """The sequence turned about z and shifted in xy, re-rounded to float32."""
    rz = Rot.from_rotvec([0.0, 0.0, angle])
    return f32(rz.apply(up(seq[0])) + np.array(shift)), f32((rz * Rot.from_rotvec(up(seq[1]))).as_rotvec()), seq[2]


def many_rows_sequence(seed=3, T=MANY_FRAMES):
    """A smooth walk of T frames: every joint swings by at most 0.3 rad per component, the root turns about z within +-0.8 rad, so
    that a window starting at ANY frame is far from both degeneracies."""
    g = np.random.default_rng([int(seed), 0x44AA])
    t = np.arange(T)[:, None, None]
    aa = 0.3 * np.sin(g.uniform(0, 2 * np.pi, (1, 22, 3)) + t * g.uniform(0.01, 0.09, (1, 22, 3)))
    yaw = 0.8 * np.sin(2 * np.pi * np.arange(T) / 3000.0)
    aa[:, 0] = (Rot.from_euler("z", yaw) * Rot.from_rotvec(aa[:, 0])).as_rotvec()
    step = 0.01 * np.stack([np.cos(yaw), np.sin(yaw), np.zeros(T)], 1)
    trans = np.array([0.3, -0.2, 0.9]) + np.cumsum(step, 0) + 0.02 * np.sin(np.arange(T) / 7.0)[:, None]
    return f32(trans), f32(aa[:, 0]), f32(aa[:, 1:].reshape(T, 63))


# ------------------------------------------------------------------------------------------ the independent restatement
def scipy_window(trans, root_orient, body_pose, rest_offsets=REST_OFFSETS, canonicalize=True, parents=WO.PARENTS):
    """process_window_data on scipy Rotation quaternions, fp64: the same outputs as WO.process_window (without the velocity)."""
    trans = up(np.asarray(trans, np.float32))
    aa = np.concatenate([up(np.asarray(root_orient, np.float32)).reshape(-1, 1, 3), up(np.asarray(body_pose, np.float32)).reshape(-1, 21, 3)], 1)
    rest = up(np.asarray(rest_offsets, np.float32)).reshape(22, 3)
    n = aa.shape[0]
    loc = [Rot.from_rotvec(aa[:, j]) for j in range(22)]

    def chain(root):
        glob = [root]
        for j in range(1, 22):
            glob.append(glob[parents[j]] * loc[j])
        return glob

    yrot = np.array([1.0, 0.0, 0.0, 0.0])
    if canonicalize:
        f = chain(loc[0])[WO.HEAD][0].apply([1.0, 0.0, 0.0]) * np.array([1.0, 1.0, 0.0])
        f = f / (np.linalg.norm(f) + 1e-8)
        yrot = np.array([np.linalg.norm(f) + f[0], 0.0, 0.0, f[1]])  # quat_between((1, 0, 0), f)
        yrot = yrot / (np.linalg.norm(yrot) + 1e-8)
        w, u = yrot[0], -yrot[1:]  # the inverse as the reference applies it to the translation: not quite of unit length
        t = 2.0 * np.cross(u, trans)
        trans = trans + w * t + np.cross(u, t)
        loc[0] = Rot.from_quat([0.0, 0.0, -yrot[3], yrot[0]]) * loc[0]  # scipy: (x, y, z, w), normalised on entry
    glob = chain(loc[0])
    pos = np.zeros((n, 22, 3))
    for j in range(1, 22):
        pos[:, j] = glob[parents[j]].apply(rest[j]) + pos[:, parents[j]]
    pos = pos + rest[0] + trans[:, None, :]
    pos = pos - pos[0, WO.HEAD] * np.array([1.0, 1.0, 0.0])
    six = lambda rots: np.stack([r.as_matrix()[:, :2, :].reshape(n, 6) for r in rots], 1).reshape(n, 132)
    return {"global_jpos": pos.reshape(n, 66), "global_rot_6d": six(glob), "local_rot_6d": six(loc), "recover_rot_quat": yrot}


def first_head_conditioning(root_orient, body_pose):
    """(horizontal projection of the head's x-axis in the first frame, 1 + f.x of its normalised projection)."""
    aa = np.concatenate([up(root_orient)[:1].reshape(1, 3), up(body_pose)[:1].reshape(21, 3)])
    R = np.eye(3)
    for j in HEAD_CHAIN:
        R = R @ WO.rodrigues(aa[j])
    horiz = np.hypot(R[0, 0], R[1, 0])
    return horiz, 1.0 + R[0, 0] / (horiz + 1e-8)


def check_window(frames, want, canonicalize=True):
    """The preconditions of one non-empty window (`frames`: its trans, root_orient, body_pose; `want`: the oracle's process_window
    of them) -> {output: distance between the two fp64 paths}."""
    horiz, one_plus_fx = first_head_conditioning(frames[1], frames[2])
    assert horiz >= MIN_FORWARD_XY, horiz
    if canonicalize:
        assert one_plus_fx >= MIN_ONE_PLUS_FX, one_plus_fx
    other = scipy_window(*frames, canonicalize=canonicalize)
    dist = {}
    for k in CONTINUOUS:
        assert np.isfinite(want[k]).all(), k
        dist[k] = float(up_to_sign(other[k], want[k]).max() if k == "recover_rot_quat" else np.abs(other[k] - want[k]).max())
        assert dist[k] <= 1e-3 * gpu_bound(want[k]), (k, dist[k])
    return dist


def oracle_windows(seq, window, canonicalize, table):
    """WO.build for the rows of `table` over one sequence, every non-empty window checked -> (the oracle's arrays, the worst
    distance per output between the two fp64 paths)."""
    _, orc = WO.build([seq], REST_OFFSETS, window, canonicalize, table=table)
    worst = dict.fromkeys(CONTINUOUS, 0.0)
    for i, (_, start, _, n) in enumerate(table):
        if n == 0:
            continue
        want = {k: orc[k][i, :n] for k in CONTINUOUS[:3]}
        want["recover_rot_quat"] = orc["recover_rot_quat"][i]
        for k, d in check_window(tuple(a[start:start + n] for a in seq), want, canonicalize).items():
            worst[k] = max(worst[k], d)
    for a in orc.values():
        a.setflags(write=False)
    return orc, worst


# ------------------------------------------------------------------------------------------ the cases, computed once
@functools.lru_cache(maxsize=None)
def chunk_case(W, canonicalize):
    seq, table = chunk_sequence(), chunk_table(W)
    orc, worst = oracle_windows(seq, W, canonicalize, table)
    return dict(seq=seq, table=table, oracle=orc, fp64_paths=worst)


@functools.lru_cache(maxsize=None)
def rule_case(kind, W, canonicalize=True):
    """The windows the reference's rule cuts from heading_sequence(W) ('heading'), angle_sequence(W) ('angle') or its turned copy
    ('turned')."""
    seq = {"heading": heading_sequence, "angle": angle_sequence, "turned": lambda w: turned(angle_sequence(w))}[kind](W)
    table = WO.window_table([len(seq[0])], W)
    orc, worst = oracle_windows(seq, W, canonicalize, table)
    return dict(seq=seq, table=table, oracle=orc, fp64_paths=worst)


def many_rows_windows(n_windows):
    """The windows of the many-rows sequence that the oracle is run on: the first, the last, the one that holds row
    MOTION_GRID_CAP_ROW and its two neighbours."""
    k = MOTION_GRID_CAP_ROW // MANY_WINDOW
    return [0, k - 1, k, k + 1, n_windows - 1]


@functools.lru_cache(maxsize=None)
def many_rows_case():
    seq = many_rows_sequence()
    table = WO.window_table([MANY_FRAMES], MANY_WINDOW, MANY_MIN_FRAMES)
    pick = many_rows_windows(len(table))
    orc, worst = oracle_windows(seq, MANY_WINDOW, True, table[pick])
    return dict(seq=seq, table=table, pick=pick, oracle=orc, fp64_paths=worst)
