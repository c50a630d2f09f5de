"""tests/rotation_edge_cases.py on the CPU: the builders' margins hold, the oracles agree with independent references on the
cases, the recorded results of the reference's get_head_vel equal the oracle's float32 mode, and each planted defect, applied to
the oracle in numpy, moves some case past the bar its GPU test uses (test_gpu_body_edges.py, test_gpu_evaluate_edges.py,
test_gpu_amass_edges.py), which is what shows that those tests bite.
"""
import math
import os

import numpy as np
import pytest
import torch

import amass_oracle as AO
import body_oracle as BO
import eval_oracle as O
import rotation_edge_cases as RC
from egoego_release_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = 2.0 ** -24  # half a float32 ulp of 1: a component of a unit quaternion rounded once from fp64


# ------------------------------------------------------------------------------------------------ builders and references
def test_axis_angles_and_rodrigues_against_independent_references():
    v = RC.axis_angles()
    assert v.shape == (78, 3) and v.dtype == np.float32
    a = np.linalg.norm(v.astype(np.float64), axis=1).reshape(13, 6)
    assert np.allclose(a, np.asarray(RC.MAGNITUDES)[:, None], rtol=1e-7, atol=0)
    a2 = (v.astype(np.float64) ** 2).sum(1).reshape(13, 6)
    assert (a2[:4] < 1e-12).all() and (a2[4:] >= 1e-12).all()  # both sides of the series switch
    assert np.array_equal(v[42], [np.float32(math.pi), 0, 0]) and np.array_equal(v[60], [np.float32(2 * math.pi), 0, 0])
    R = BO.rodrigues(torch.from_numpy(v.astype(np.float64))).numpy()
    d_scipy = np.abs(R - BO.rodrigues_independent(v)).max()
    small = a.reshape(-1) < 1
    d_series = float(np.abs(R[small] - BO.rodrigues_series(v[small])).max())
    print(f"rodrigues vs scipy {d_scipy:.3e}; vs the long-double series for |v| < 1 {d_series:.3e}")
    assert d_scipy <= 4.5e-16  # four ulps of an entry next to 1 (scipy goes through a quaternion)
    assert d_series <= 2.0 ** -53  # an entry of magnitude <= 1 rounded once
    assert np.abs(R - BO.rodrigues_series(v)).max() <= 8 * 2.0 ** -53  # the halved-and-squared series, every magnitude
    assert np.array_equal(R[:6], np.broadcast_to(np.eye(3), (6, 3, 3)))  # exact at zero


def test_the_builders_margins_hold():
    fc = RC.fk_chains()
    assert fc["local_aa"].shape == (78 * 22 + 36, 22, 3) and fc["flips"] >= 20 and fc["min_w"] >= 1e-9
    hr = RC.head_rotations()
    assert hr["R"].dtype == np.float32 and all((hr["winner"] == k).sum() >= 3 for k in range(4))
    hs = RC.head_sequences()
    assert [s["rot"].shape[0] for s in hs] == [1, 2, 40]
    for s in hs[1:]:
        ok = np.where(s["identical"], np.abs(1 - s["r0"]) < 2.5e-7, (s["r0"] >= 1e-3) & (s["r0"] <= 1 - 3e-6))
        assert ok.all() and s["heading"].min() >= 0.1
        assert np.abs(np.linalg.norm(np.diff(s["joints"][:, AO.HEAD].astype(np.float64), axis=0), axis=1) - 0.02).max() < 1e-6
    m = RC.metric_inputs()
    assert tuple(m["lengths"][:-1]) == RC.METRIC_LENGTHS and m["pred_jpos"].shape == (12, RC.METRIC_T, 22, 3)
    b = m["identical"]
    assert all(m["pred_" + k][b].tobytes() == m["gt_" + k][b].tobytes() for k in ("jpos", "quat", "floor"))
    for k in ("pred_jpos", "gt_jpos", "pred_quat", "gt_quat"):
        assert all((m[k][i, L:] == RC.PAD).all() for i, L in enumerate(m["lengths"]))
    L = 513
    q = m["pred_quat"][10, :L, 0].astype(np.float64)
    n2 = (q * q).sum(-1)
    big = n2[n2 > 1e-3]
    assert (n2[1::7] == 0).all() and np.all((np.abs(big - 0.0625) < 1e-7) | (np.abs(big - 16.0) < 1e-5)) and big.size > 300
    p = RC.body_edge_poses()
    assert p["aa"].shape == (1092, 52, 3) and p["small"].sum() == 252 and not p["small"][1::2].any()
    assert RC.amass_joint_poses()["pose_body"].shape == (312, 63)


def test_fk_oracle_at_the_chains_against_the_matrix_fk():
    fc = RC.fk_chains()
    gq, gp = fc["oracle_quat"], fc["oracle_jpos"]
    assert (gq[..., 0] >= 0).all() and np.abs(np.linalg.norm(gq, axis=-1) - 1).max() < 1e-14
    assert np.abs(gp - synthetic.eval_fk(fc["root_trans"], fc["local_aa"], fc["rest_offsets"], fc["parents"])).max() <= 1e-12
    # the global rotation of each joint is the product of Rodrigues' matrices down its chain (scipy / the series, not quaternions)
    R = BO.rodrigues_independent(fc["local_aa"])
    G = [R[:, 0]]
    for j in range(1, 22):
        G.append(G[int(fc["parents"][j])] @ R[:, j])
    assert np.abs(O.quat_to_matrix(gq) - np.stack(G, 1)).max() <= 1e-13


def test_matrix_to_quaternion_oracle_against_scipy():
    from scipy.spatial.transform import Rotation
    hr = RC.head_rotations()
    R = hr["R"].astype(np.float64)
    q = AO.matrix_to_quaternion(R)
    assert (q[:, 0] >= 0).all()
    s = Rotation.from_matrix(R).as_quat()[:, [3, 0, 1, 2]]  # scipy: (x, y, z, w), and the nearest rotation of a rounded matrix
    s = np.where((s * q).sum(-1, keepdims=True) < 0, -s, s)
    assert np.abs(q - s).max() <= 8 * F32  # the matrices are float32 roundings of rotations
    assert np.array_equal(q[1:4], [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def test_quat_to_matrix_identity_branch_and_unchanged_bits():
    g = np.random.default_rng(0)
    q = g.standard_normal((500, 4)) * g.choice([1e-7, 0.25, 1.0, 4.0], (500, 1))
    old = q / np.linalg.norm(q, axis=-1, keepdims=True)  # the function as it stood, line for line
    w, x, y, z = np.moveaxis(old, -1, 0)
    old = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                    2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(500, 3, 3)
    assert O.quat_to_matrix(q).tobytes() == old.tobytes()
    u = np.array([0.5, -0.5, 0.5, 0.5])
    got = O.quat_to_matrix(np.stack([np.zeros(4), u * 1e-8, u * math.sqrt(1e-15), u]))
    assert np.array_equal(got[0], np.eye(3)) and np.array_equal(got[1], np.eye(3))
    assert np.abs(got[2] - got[3]).max() < 1e-15 and np.abs(got[3] - np.eye(3)).max() > 0.5


def test_metric_oracle_is_nan_below_three_frames_and_nowhere_else():
    want = RC.metric_oracle()
    acc = [O.METRIC_KEYS.index(k) for k in ("accel_pred", "accel_gt", "accel_err")]
    nan = np.isnan(want)
    assert nan[:2][:, acc].all() and nan.sum() == 6
    assert want[0, O.METRIC_KEYS.index("pred_fs")] == 0 and want[0, O.METRIC_KEYS.index("gt_fs")] == 0  # one frame: no step to slide
    b = RC.metric_inputs()["identical"]
    small = np.abs(want[b]) < RC.RESIDUE
    assert small[[O.METRIC_KEYS.index(k) for k in ("root_dist", "root_rot_dist", "root_trans_dist", "mpjpe", "accel_err")]].all()
    others = np.abs(want[~nan & ~(np.abs(want) < RC.RESIDUE)])
    assert others.min() > 1e-6  # nothing sits between the residue and a real value


def test_golden_head_vels_equal_the_oracles_float32_mode():
    z = np.load(os.path.join(ROOT, "tests", "golden", "amass_head_edges.npz"))
    for b, s in enumerate(RC.head_sequences()):
        assert np.array_equal(z["seq%d/head_rot" % b], s["rot"]) and np.array_equal(z["seq%d/head_qpos" % b], s["qpos32"])
        tracks = AO.head_tracks(np.where(np.arange(22)[:, None] == AO.HEAD, s["pos"][:, None].astype(np.float64), 0.0), s["rot"], float32=True)
        assert np.abs(tracks["head_qpos"] - s["qpos32"]).max() <= F32
        if b == 0:
            assert "seq0/head_vels" not in z.files and tracks["head_vels"].shape == (1, 6) and not tracks["head_vels"].any()
            continue
        d = AO.rel_diff(z["seq%d/head_vels" % b], tracks["head_vels"])
        print(f"sequence {b}: reference vs the oracle's float32 mode {d:.3e}")
        assert d <= AO.HEAD_EDGES_REFERENCE_DISTANCE[b]
        assert np.array_equal(np.all(z["seq%d/head_vels" % b][:-1, 3:] == 0, 1), tracks["same"])
        assert np.array_equal(tracks["same"], s["identical"])


# ------------------------------------------------------------------------------------------------ planted defects
def test_defect_always_candidate_zero_in_matrix_to_quaternion():
    R = RC.head_rotations()["R"].astype(np.float64)
    m = lambda i, j: R[..., i, j]  # noqa: E731
    qa0 = np.sqrt(np.maximum(1 + m(0, 0) + m(1, 1) + m(2, 2), 0.0))
    bad = np.stack([qa0 ** 2, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1) / (2.0 * np.maximum(qa0, 0.1))[:, None]
    moved = np.abs(bad - AO.matrix_to_quaternion(R)).max(-1)
    assert (moved > F32).sum() >= 6 and moved[1:4].min() > 0.9  # the half turns come out as zero quaternions


def test_defect_no_standardisation_in_fk(monkeypatch):
    fc = RC.fk_chains()
    monkeypatch.setattr(O, "_std", lambda q: q)
    bad, pos = O.fk(fc["root_trans"], fc["local_aa"], fc["rest_offsets"], fc["parents"])
    assert np.abs(pos - fc["oracle_jpos"]).max() < 1e-12  # the joints do not care: only the quaternion test can see this
    assert (np.abs(bad - fc["oracle_quat"]).max(-1) > F32).sum() >= 20 and (bad[..., 0] < 0).any()


def _metric_excess(got, want):
    from test_gpu_evaluate import BOUND
    worst = 0.0
    for b in range(want.shape[0]):
        worst = max([worst] + [f / bar for f, bar in RC.metric_figures(got[b], want[b], BOUND).values()])
    return worst


def test_defects_in_the_metrics_quaternion_matrix(monkeypatch):
    want = RC.metric_oracle()
    assert _metric_excess(want, want) < 1e-3  # (not 0: the identical sample's residue is held against RESIDUE)

    def unnormalised(q):  # quaternion_matrix without q *= sqrt(2 / n)
        q = np.asarray(q, np.float64)
        w, x, y, z = np.moveaxis(q, -1, 0)
        return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))

    def no_identity(q):  # normalises whatever it gets: 0 / 0 at a zero quaternion, a rotation at a tiny one
        q = np.asarray(q, np.float64)
        return unnormalised(q / np.linalg.norm(q, axis=-1, keepdims=True))

    for bad in (unnormalised, no_identity):
        monkeypatch.setattr(O, "quat_to_matrix", bad)
        got = RC.metric_oracle()
        assert _metric_excess(got, want) > 1, bad.__name__
    # the tiny quaternions alone (no zero ones) already tell the identity branch from a normalisation
    monkeypatch.undo()
    m = dict(RC.metric_inputs())
    for k in ("pred_quat", "gt_quat"):
        q = m[k].copy()
        q[(q == 0).all(-1)] = [1, 0, 0, 0]
        m[k] = q
    want2 = RC.metric_oracle(m)
    monkeypatch.setattr(O, "quat_to_matrix", no_identity)
    assert _metric_excess(RC.metric_oracle(m), want2) > 1


def test_defect_acceleration_divisor_at_one_frame():
    want = RC.metric_oracle()
    got = want.copy()
    for k in ("accel_pred", "accel_gt", "accel_err"):
        got[0, O.METRIC_KEYS.index(k)] = 0.0 / (1 - 2)  # the sum over no frames over L - 2 at L = 1: -0.0, not NaN
    assert _metric_excess(got, want) == np.inf
    got = want.copy()
    got[:2, O.METRIC_KEYS.index("accel_err")] = np.nan
    assert _metric_excess(got, want) < 1e-3


def test_defect_rodrigues_series_up_to_one_radian(monkeypatch):
    """The switch on a < 1e-6 * 1e6: the two-term series is then used up to 1 rad.  At the edge magnitudes themselves it is
    harmless (1e-4: a^4 / 120 = 1e-18); the rotations of up to 0.5 rad on the other joints show it."""
    p = RC.amass_joint_poses()
    model = synthetic.make_body_model(0, n_verts=512, n_faces=64)
    _, want = AO.joints_and_head_rot(model, p["root_orient"][:40], p["pose_body"][:40], p["trans"][:40])
    good = BO.rodrigues

    def bad(aa):
        x, y, z = aa.unbind(-1)
        a2 = x * x + y * y + z * z
        s, c = 1 - a2 / 6, 0.5 - a2 / 24
        R = torch.stack([1 - c * (y * y + z * z), c * x * y - s * z, c * x * z + s * y, c * x * y + s * z, 1 - c * (x * x + z * z),
                         c * y * z - s * x, c * x * z - s * y, c * y * z + s * x, 1 - c * (x * x + y * y)], -1).reshape(aa.shape[:-1] + (3, 3))
        return torch.where((a2 < 1.0)[..., None, None], R, good(aa))

    monkeypatch.setattr(BO, "rodrigues", bad)
    _, got = AO.joints_and_head_rot(model, p["root_orient"][:40], p["pose_body"][:40], p["trans"][:40])
    assert np.abs(got - want).max() > 8 * F32


@pytest.mark.parametrize("nj", [22, 52])
def test_split_offsets_of_the_body_oracle_lie_between_fp32_and_the_ceiling(nj):
    """The emulated split-bf16 contraction differs from fp64 by the operands' rounding alone: more than nothing, far under the
    project's 5e-5 ceiling; and the default path of forward keeps its bits."""
    model = synthetic.make_body_model(14, n_verts=52, n_faces=8)
    p = RC.body_edge_poses()
    aa, tr = p["aa"][:60, :nj], p["trans"][:60]
    betas = np.zeros((60, 16))
    r64 = BO.forward(model, aa, tr, betas)
    emul = BO.forward(model, aa, tr, betas, split_offsets=True)
    e = ((emul["offsets"] - r64["offsets"]).abs().max() / r64["offsets"].abs().max()).item()
    assert 0 < e < 5e-6 and torch.equal(emul["Jtr"], r64["Jtr"])
    assert torch.equal(BO.forward(model, aa, tr, betas, split_offsets=False)["v"], r64["v"])
