"""numpy restatement of one sample of GravityNet's training data (the reference's AMASSHeadPoseDataset.__getitem__ with
augment_traj, egoego/data/amass_headpose_dataset.py:38-76 and 115-165) for GIVEN draws, and a numpy replica of the draw mapping of
egoego_s1_gravity_batch (include/egoego_hip.h).

    sample(seq, window, start, Rr, scale, mode)   mode "fp64": every operation in float64 on the float32 inputs
                                                  mode "ref32": float32, the reference's operation order, the serial sum
    draw_start / draw_scale / draw_normals / draw_rotation   the kernel's draws for (seed, draw ids)

"ref32" reproduces the reference's tensors bit for bit (tests/golden/make_gravity_batch_golden.py asserts it): torch's CPU kernels
add the four squares of a quaternion left to right and contract a 3-vector as ((0 + a0 b0) + a1 b1) + a2 b2 without fused
multiply-adds, which is what numpy's elementwise float32 arithmetic below does.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
DRAW_TAG = 0x47424154
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PW0, PW1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- the arithmetic
def quaternion_to_matrix(q, dtype):
    """pytorch3d's published formula on [..., 4] real-first quaternions -> [..., 3, 3] in `dtype`."""
    q = np.asarray(q, dtype)
    r, i, j, k = (q[..., n] for n in range(4))
    one, two = dtype(1.0), dtype(2.0)
    two_s = two / (((r * r + i * i) + j * j) + k * k)
    o = np.stack([one - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), one - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), one - two_s * (i * i + j * j)], -1)
    return o.reshape(q.shape[:-1] + (3, 3)).astype(dtype)


def random_rotation_from_normals(o, dtype):
    """pytorch3d's random_quaternions / random_rotation from its four normals o -> (q, Rr) in `dtype`."""
    o = np.asarray(o, dtype)
    s = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]
    q = (o / np.copysign(np.sqrt(s), o[0])).astype(dtype)
    return q, quaternion_to_matrix(q, dtype)


def _dot3(A, x):
    """[..., 3, 3] times [..., 3, n] contracted as ((0 + a0 b0) + a1 b1) + a2 b2 in the arrays' dtype (the leading zero is the
    accumulator torch's matmul starts from: it only turns a sum of negative zeros into +0)."""
    zero = A.dtype.type(0.0)
    return ((zero + A[..., :, 0, None] * x[..., None, 0, :]) + A[..., :, 1, None] * x[..., None, 1, :]) + A[..., :, 2, None] * x[..., None, 2, :]


def window_of(length, window, for_eval, start):
    """dataset:121-133 -> (start, n): `start` is the draw from range(length - window - 1), used only where the reference draws."""
    room = length - window - 1
    if room <= 0:
        return 0, length
    return (0 if for_eval else int(start)), window + 1


def sample(seq, window, start, Rr, scale, mode="fp64"):
    """seq [len, 7] float32 (xyz, w,x,y,z), start/n from window_of applied by the caller: `start` is the first row.  Rr [3, 3]
    (float32 values), scale (a float32 value; "ref32" also takes the reference's float64 draw and rounds it where torch does).
    -> dict of numpy arrays with the batch's keys for one sample (no batch axis)."""
    seq = np.asarray(seq, np.float32)
    W = int(window)
    n = min(seq.shape[0] - start, W + 1) if seq.shape[0] - W - 1 > 0 else seq.shape[0]
    win = seq[start:start + n]
    dt = np.float64 if mode == "fp64" else np.float32
    Rr = np.asarray(Rr, np.float32).astype(dt)
    R = quaternion_to_matrix(win[:, 3:].astype(dt), dt)                      # [n, 3, 3]
    rot = _dot3(Rr[None], R)                                                 # Rr @ R(q_t)
    cur = (win[:, :3] - win[0:1, :3]) if mode != "fp64" else (win[:, :3].astype(dt) - win[0:1, :3].astype(dt))
    y = _dot3(Rr[None], cur[:, :, None])[:, :, 0]                            # [n, 3]
    s = dt(np.float32(scale))
    if mode == "fp64":
        x = np.empty_like(y)
        x[0] = y[0]
        for t in range(n - 1):
            x[t + 1] = x[t] + s * (y[t + 1] - y[t])
    else:
        diff = (y[1:] - y[:-1]) * s
        x = np.empty_like(y)
        x[0] = y[0]
        for t in range(n - 1):
            x[t + 1] = x[t] + diff[t]
    pad = lambda a: np.concatenate([a, np.zeros((W + 1 - n,) + a.shape[1:], a.dtype)], 0)  # noqa: E731
    return {"ori_head_pose": pad(win.astype(dt)), "head_rot_mat": pad(rot), "head_trans": pad(x), "seq_len": n,
            "aligned_rot_mat": Rr.T.copy(), "aligned_scale": np.float64(1.0) / np.float64(scale), "floor_normal": Rr[:, 2:3].copy(),
            "start_t_idx": start, "aug_scale": np.float32(scale)}


def err_units(got, want):
    """The largest distance of `got` from `want` in units of eps_fp32 * max|want| (0 for an all-zero `want` met exactly)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = float(np.abs(want).max()) if want.size else 0.0
    d = float(np.abs(got - want).max()) if want.size else 0.0
    if top == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / (EPS32 * top)


FLOAT_KEYS = ("head_rot_mat", "head_trans", "aligned_rot_mat", "aligned_scale", "floor_normal")


# ---------------------------------------------------------------------------------------------- the draws
def philox4x32_10(ctr, key):
    """Random123's Philox4x32-10: ctr four uint32 arrays (broadcast), key two uint32 -> [..., 4] uint32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PW0) & MASK32, (k1 + PW1) & MASK32
    return np.stack([c.astype(np.uint32) for c in (c0, c1, c2, c3)], -1)


def _words(seed, draw_ids, which):
    ids = np.asarray(draw_ids, np.int64).astype(np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((ids & MASK32, ids >> np.uint64(32), which, DRAW_TAG), (seed & 0xFFFFFFFF, seed >> 32))


def draw_start(seed, draw_ids, room):
    """(word 0 of draw 1 * room) >> 32 -> int64 [n]"""
    w = _words(seed, draw_ids, 1)[..., 0].astype(np.uint64)
    return ((w * np.uint64(room)) >> np.uint64(32)).astype(np.int64)


def draw_scale(seed, draw_ids):
    """0.1 + 9.9 * (word 1 of draw 1 + 0.5) * 2^-32 in float64, rounded to float32"""
    w = _words(seed, draw_ids, 1)[..., 1].astype(np.float64)
    return (0.1 + 9.9 * ((w + 0.5) * 2.0 ** -32)).astype(np.float32)


def draw_normals(seed, draw_ids):
    """common.h's philox_normal4 on draw 0: float32 steps as the kernel takes them, with log2 / sin / cos of the turns evaluated in
    float64 and rounded (the device's v_log_f32 / v_sin_f32 / v_cos_f32 are approximations of those) -> float32 [n, 4]."""
    f = np.float32
    r = _words(seed, draw_ids, 0)
    inv = f(2.3283064365386963e-10)
    u0 = np.minimum((r[..., 0].astype(f) + f(1.0)) * inv, f(1.0))
    u1 = r[..., 1].astype(f) * inv
    u2 = np.minimum((r[..., 2].astype(f) + f(1.0)) * inv, f(1.0))
    u3 = r[..., 3].astype(f) * inv
    ln2 = f(0.6931471805599453)
    ra = np.sqrt((f(-2.0) * ln2) * np.log2(u0.astype(np.float64)).astype(f))
    rb = np.sqrt((f(-2.0) * ln2) * np.log2(u2.astype(np.float64)).astype(f))
    turn = lambda fn, u: fn(2.0 * np.pi * u.astype(np.float64)).astype(f)  # noqa: E731
    return np.stack([ra * turn(np.cos, u1), ra * turn(np.sin, u1), rb * turn(np.cos, u3), rb * turn(np.sin, u3)], -1).astype(f)


def draw_rotation(seed, draw_ids):
    """The kernel's Rr: float64 from the float32 normals, rounded to float32 once -> float32 [n, 3, 3]"""
    o = draw_normals(seed, draw_ids)
    return np.stack([random_rotation_from_normals(v, np.float64)[1] for v in o.reshape(-1, 4)]).astype(np.float32)
