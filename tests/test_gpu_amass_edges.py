"""The AMASS joints and head-track kernels on the GPU (csrc/amass_prep.h) at rotation edges, against the fp64 oracle
(tests/amass_oracle.py) and the recorded results of the reference's own get_head_vel (tests/golden/amass_head_edges.npz); the
cases are tests/rotation_edge_cases.py's amass_joint_poses(), head_rotations() and head_sequences().

  joints   each vector of axis_angles() on the root and on joints 3, 12 and 15: the joints carry the bits of the body model's
           Jtr[:, :22] (test_joints_against_the_body_model's property, now at the edges), head_rot is within 8 x 2^-24 of the
           oracle's global rotation of joint 15.
  head     egoego_amass_head called directly on planted head rotations, on which each of mat_to_quat's four candidates wins
           (exact half turns among them), in sequences of 1, 2 and 40 frames whose pairs are bit-identical, up to 3.1 rad apart,
           and on both sides of qrel's sign standardisation.  `same` equals the oracle's; the quaternions are within 2^-24 of the
           oracle's and carry its sign; the two diffs are under test_gpu_amass_prep.bound; head_vels, against the oracle's
           float32 mode, under the smaller of 4 x HEAD_KERNEL_DISTANCE (MI355X) and 4 x amass_oracle.HEAD_EDGES_REFERENCE_DISTANCE
           per sequence, the rule of test_gpu_amass_prep.py; and within the reference's distance plus that bar of the reference's
           own rows (the triangle through the oracle).

Measured on an MI355X (profiles/rotation_edges_error.json; EGOEGO_EDGES_RECORD=<file> writes it): head_rot 2.979e-08 (bar
4.768e-07), joints against the oracle 4.806e-08; head quaternion components 2.835e-08 (bar 5.960e-08); head_vels 2.441e-08 and
2.957e-08 (the reference's own rows: 1.037e-07 and 1.425e-07 from the oracle, 1.073e-07 and 1.674e-07 from the kernel);
global_head_rot_6d_diff 5.067e-08, global_head_trans_diff 0.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import amass_oracle as O
import rotation_edge_cases as RC
from egoego_release_amd import _lib, amass_prep as A, body, synthetic
from test_gpu_amass_prep import bound, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = 2.0 ** -24
# worst relative difference of head_vels from the oracle's float32 mode per sequence of head_sequences(), measured on an MI355X
HEAD_KERNEL_DISTANCE = (None, 2.441e-08, 2.957e-08)


def head_vels_bar(b):
    ref = 4 * O.HEAD_EDGES_REFERENCE_DISTANCE[b]
    return ref if HEAD_KERNEL_DISTANCE[b] is None else min(4 * HEAD_KERNEL_DISTANCE[b], ref)


def test_joints_at_the_rotation_edges():
    p = RC.amass_joint_poses()
    model = synthetic.make_body_model(0, n_verts=512, n_faces=64)
    ro, pb, tr = dev(p["root_orient"]), dev(p["pose_body"]), dev(p["trans"])
    joints, head_rot = A.body_joints(ro, pb, tr, model)
    Jtr = body.BodyModel(model=model, device="cuda")(root_orient=ro, pose_body=pb, trans=tr).Jtr[:, :22]
    assert torch.equal(joints, Jtr)
    j64, R64 = O.joints_and_head_rot(model, p["root_orient"], p["pose_body"], p["trans"])
    e_rot = np.abs(head_rot.cpu().numpy() - R64).max()
    e_j = O.rel_diff(joints.cpu().numpy(), j64)
    print(f"AMASS joints at the edges: head_rot {e_rot:.3e} (bar {8 * F32:.3e}); joints vs the oracle {e_j:.3e} (bar {bound('joints'):.3e})")
    RC.record("amass_joints", head_rot=e_rot, head_rot_bar=8 * F32, joints=e_j, joints_bar=bound("joints"))
    assert e_rot <= 8 * F32
    assert e_j <= bound("joints")


@pytest.fixture(scope="module")
def head_run():
    """egoego_amass_head on the three sequences packed end to end -> (the sequences, per sequence the kernel's rows)."""
    seqs = RC.head_sequences()
    lens = [s["rot"].shape[0] for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N, B = int(off[-1]), len(seqs)
    joints = dev(np.concatenate([s["joints"] for s in seqs]))
    rot = dev(np.concatenate([s["rot"] for s in seqs]).reshape(N, 9))
    contacts = torch.zeros(N, 22, device="cuda")
    floor = dev(np.asarray([s["floor"] for s in seqs], np.float32))
    d_src, d_seq, d_oo = dev(np.arange(N, dtype=np.int32)), dev(np.repeat(np.arange(B, dtype=np.int32), lens)), dev(off)
    f32 = dict(device="cuda", dtype=torch.float32)
    out = {"joints": torch.empty(N, 22, 3, **f32), "contacts": torch.empty(N, 22, device="cuda", dtype=torch.float64),
           "global_head_trans": torch.empty(N, 3, **f32), "global_head_rot_6d": torch.empty(N, 6, **f32), "head_qpos": torch.empty(N, 7, **f32),
           "global_head_rot_6d_diff": torch.empty(N, 6, **f32), "global_head_trans_diff": torch.empty(N, 3, **f32),
           "head_vels": torch.empty(N, 6, **f32), "same": torch.empty(N, device="cuda", dtype=torch.uint8)}
    assert tuple(out) == A.HEAD_KEYS
    _lib.check_amass(_lib.load().egoego_amass_head(joints.data_ptr(), rot.data_ptr(), contacts.data_ptr(), floor.data_ptr(), d_src.data_ptr(),
                                                   d_seq.data_ptr(), d_oo.data_ptr(), N, N, B, *[out[k].data_ptr() for k in A.HEAD_KEYS],
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return seqs, [{k: v[off[b]:off[b + 1]] for k, v in host.items()} for b in range(B)]


def _oracle(s):
    shifted = s["joints"].copy()
    shifted[:, :, 2] = shifted[:, :, 2] - s["floor"]  # float32, as the kernel and the reference shift them
    assert np.array_equal(shifted[:, O.HEAD], s["pos"])
    return shifted, O.head_tracks(shifted.astype(np.float64), s["rot"], float32=True)


def test_head_quaternions_and_branches(head_run):
    seqs, rows = head_run
    worst = 0.0
    for b, (s, got) in enumerate(zip(seqs, rows)):
        shifted, want = _oracle(s)
        T = s["rot"].shape[0]
        assert np.array_equal(got["joints"], shifted) and np.array_equal(got["global_head_trans"], s["pos"])
        assert np.array_equal(got["head_qpos"][:, :3], s["pos"])
        assert np.array_equal(got["global_head_rot_6d"], s["rot"].reshape(T, 9)[:, :6])
        q = got["head_qpos"][:, 3:].astype(np.float64)
        worst = max(worst, np.abs(q - want["quat"]).max())
        assert np.abs(q - want["quat"]).max() <= F32, b
        assert (q[:, 0] >= 0).all() and not np.signbit(got["head_qpos"][:, 3]).any() and ((q * want["quat"]).sum(-1) > 0.99).all(), b
        same = np.append(want["same"], want["same"][-1:])  # a sequence's last row repeats its last pair
        assert np.array_equal(got["same"], same.astype(np.uint8) if T > 1 else np.zeros(1, np.uint8)), b
    assert np.array_equal(rows[0]["head_qpos"][0, 3:], [0, 1, 0, 0]) and np.array_equal(rows[1]["head_qpos"][1, 3:], [0, 0, 1, 0])
    assert rows[2]["same"].sum() == 6
    print(f"head quaternions at the edges: worst component difference {worst:.3e} (bar {F32:.3e})")
    RC.record("amass_head_quaternions", component=worst, bar=F32, winners=np.bincount(RC.head_rotations()["winner"], minlength=4).tolist())


def test_head_diffs_and_velocities(head_run):
    seqs, rows = head_run
    gold = np.load(os.path.join(ROOT, "tests", "golden", "amass_head_edges.npz"))
    one = rows[0]  # a single frame: no pair
    assert not one["head_vels"].any() and one["same"][0] == 0
    assert not one["global_head_rot_6d_diff"].any() and not one["global_head_trans_diff"].any()
    assert np.array_equal(rows[1]["head_vels"][0], rows[1]["head_vels"][1])  # two frames: the only pair, twice
    for b in (1, 2):
        s, got = seqs[b], rows[b]
        _, want = _oracle(s)
        fig = {k: O.rel_diff(got[k][:-1], want[k]) for k in ("global_head_rot_6d_diff", "global_head_trans_diff")}
        assert not got["global_head_rot_6d_diff"][-1].any() and not got["global_head_trans_diff"][-1].any()
        fig["head_vels"] = O.rel_diff(got["head_vels"], want["head_vels"])
        bars = {"global_head_rot_6d_diff": bound("global_head_rot_6d_diff"), "global_head_trans_diff": bound("global_head_trans_diff"),
                "head_vels": head_vels_bar(b)}
        d_gold = O.rel_diff(got["head_vels"], gold["seq%d/head_vels" % b])
        gold_bar = O.HEAD_EDGES_REFERENCE_DISTANCE[b] + head_vels_bar(b)
        print(f"sequence {b}:", {k: "%.3e / %.3e" % (fig[k], bars[k]) for k in fig}, "vs the reference's rows %.3e / %.3e" % (d_gold, gold_bar))
        RC.record(f"amass_head_sequence_{b}", figure=fig, bar=bars, vs_reference_rows=d_gold, vs_reference_rows_bar=gold_bar,
                  reference_vs_oracle=O.HEAD_EDGES_REFERENCE_DISTANCE[b])
        assert np.isfinite(got["head_vels"]).all()
        for k in fig:
            assert fig[k] <= bars[k], (b, k, fig[k], bars[k])
        assert d_gold <= gold_bar, (b, d_gold, gold_bar)
        assert np.array_equal(np.all(got["head_vels"][:, 3:] == 0, 1), got["same"].astype(bool)), b  # axis * 0: exact zeros
