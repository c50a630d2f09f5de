"""The edge cases of the motion-window kernels without a GPU (tests/window_cases.py): every emitted window meets its preconditions
(not degenerate; the fp64 oracle agrees with an independent scipy restatement to 1e-3 of the GPU bound), the batches hold what
they claim to hold, and the oracle reproduces the reference's own results on the heading and angle cases
(tests/golden/motion_window_edges_golden.npz, written by make_motion_window_edges_golden.py) within the reference's rounding.

Measured here: the two fp64 paths differ by at most 1.2e-14 on the edge cases and 1.1e-13 on the many-rows walk (positions of
hundreds of metres), against 1e-3 x bound >= 1.2e-10.  The reference's float32 result lies up to 2.3e-6 from the oracle where the
head x-axis is 1.52 rad above the horizontal, and no more than 3.6e-7 at a heading of pi - 1e-3 with a level head: its heading
takes a float64 detour, so the half turn costs it little; the steep head costs it 1 / cos(pitch)."""
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import harness_cases as HC
import window_cases as WC
import windows_oracle as WO
from test_harness_golden import REST_OFFSETS
from test_motion_windows import sample_rows, stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "motion_window_edges_golden.npz"))


def _head_x_axis(seq, t):
    aa = np.concatenate([WC.up(seq[1][t]).reshape(1, 3), WC.up(seq[2][t]).reshape(21, 3)])
    R = np.eye(3)
    for j in WC.HEAD_CHAIN:
        R = R @ WO.rodrigues(aa[j])
    return R[:, 0]


def test_the_case_lists_are_the_issues():
    assert WC.ANGLES is HC.ANGLES and list(WC.ANGLES_ALL[len(HC.ANGLES):]) == [4.0, 2 * np.pi - 1e-3, 7.0]
    assert len(WC.HEADING_CASES) == 21 and max(h for h, _ in WC.HEADING_CASES) == np.pi - 1e-3 and max(p for _, p in WC.HEADING_CASES) == 1.52
    assert WC.CHUNK_WINDOWS == (2, 63, 64, 65, 120, 121, 128, 129, 193, 480)
    assert WC.chunk_lengths(2) == [0, 1, 2] and WC.chunk_lengths(64) == [0, 1, 2, 63, 64] and WC.chunk_lengths(65) == [0, 1, 2, 63, 64, 65]
    assert WC.chunk_lengths(129) == [0, 1, 2, 63, 64, 65, 127, 128, 129] and WC.chunk_lengths(480) == [0, 1, 2, 63, 64, 65, 127, 128, 129, 479, 480]
    # both sides of qd_from_aa's series threshold (on the squared angle), the sign flip of qd_std, more than a turn
    a2 = WC.ANGLES_ALL ** 2
    assert (a2 == 0).any() and ((a2 > 0) & (a2 < 1e-12)).any() and ((a2 >= 1e-12) & (a2 < 1e-10)).any()
    assert (np.cos(WC.ANGLES_ALL / 2) < 0).sum() == 3 and (WC.ANGLES_ALL > 2 * np.pi).any()
    # a 63-frame window is the same frames under every W that holds one
    assert all(63 in WC.chunk_lengths(W) for W in (63, 64, 65, 193, 480))


@pytest.mark.parametrize("W", WC.CHUNK_WINDOWS)
def test_chunk_cases_meet_their_preconditions(W):
    for cano in (True, False):
        c = WC.chunk_case(W, cano)  # asserts the preconditions of every non-empty window
        first, length = c["table"][:, 1], c["table"][:, 3]
        assert list(length) == WC.chunk_lengths(W) and (first >= 0).all() and (first + length <= WC.CHUNK_FRAMES).all() and (length <= W).all()
        assert (first < WC.CHUNK_EDGE_FRAMES).all()
        assert max(c["fp64_paths"].values()) < 1e-13
        empty = int(np.flatnonzero(length == 0)[0])
        assert np.array_equal(c["oracle"]["recover_rot_quat"][empty], [1, 0, 0, 0]) and not c["oracle"]["global_jpos"][empty].any()


def test_edge_frames_have_the_prescribed_heading_and_pitch():
    """After the single rounding to float32: six axis-angles of up to 7 rad, each off by at most 2^-24 x 7 x sqrt(3), turn the head by
    at most 4.3e-6 rad; the heading feels that divided by cos(1.52) = 0.051."""
    for seq, every, n_edges, first_case in ((WC.heading_sequence(64), 32, 22, 0), (WC.heading_sequence(120), 60, 22, 0),
                                            (WC.chunk_sequence(), 1, WC.CHUNK_EDGE_FRAMES, 0), (WC.angle_sequence(120), 60, 3, 3)):
        for k in range(n_edges):
            heading, pitch = WC.HEADING_CASES[(first_case + k) % 21]
            x = _head_x_axis(seq, k * every)
            dh = np.arctan2(x[1], x[0]) - heading
            assert abs((dh + np.pi) % (2 * np.pi) - np.pi) <= 1e-4 and abs(np.arcsin(x[2]) - pitch) <= 1e-5, (k, heading, pitch)
    seen = {WC.HEADING_CASES[k % 21] for k in range(22)}
    assert seen == set(WC.HEADING_CASES)


def test_rule_cases_meet_their_preconditions_and_start_on_edge_frames():
    for kind, W, n in (("heading", 64, 22), ("heading", 120, 22), ("angle", 64, 3), ("angle", 120, 3), ("turned", 64, 3)):
        for cano in (True, False) if W == 64 else (True,):
            c = WC.rule_case(kind, W, cano)
            assert len(c["table"]) == n and (c["table"][:, 1] % (W // 2) == 0).all() and list(c["table"][:, 3]) == [W] * (n - 1) + [W // 2]
            assert max(c["fp64_paths"].values()) < 1e-13
    # the worst conditioning that is emitted: the issue's floor is not a formality
    worst = [WC.first_head_conditioning(*(a[t:t + 1] for a in WC.heading_sequence(64)[1:])) for t in range(0, 704, 32)]
    assert 0.04 <= min(h for h, _ in worst) < 0.06 and 4e-7 <= min(f for _, f in worst) < 6e-7


def test_the_angle_batches_hold_every_angle():
    for seq in (WC.angle_sequence(120), WC.angle_sequence(64), WC.heading_sequence(64), WC.chunk_sequence()):
        assert WC.holds_every_angle(seq[1], seq[2]) == set()
    # the check can fail: the smooth walk holds none of them, and one planted frame less leaves a hole
    walk = WC.many_rows_sequence(T=200)
    assert len(WC.holds_every_angle(walk[1], walk[2])) == 3 * 2 * len(WC.ANGLES_ALL)
    seq = WC.angle_sequence(120)
    root = seq[1].copy()
    root[np.abs(np.linalg.norm(root, axis=-1) - 7.0) < 1e-5] = 0.0  # no root of 7 rad any more
    assert WC.holds_every_angle(root, seq[2]) == {("root", 7.0, 1.0), ("root", 7.0, -1.0)}
    body = seq[2].copy().reshape(-1, 21, 3)
    body[:, [j - 1 for j in WC.LEAVES]] *= np.float32(0.5)
    assert {grp for grp, _, _ in WC.holds_every_angle(seq[1], body.reshape(-1, 63))} == {"leaf"}


def test_the_precondition_notices_a_path_that_differs():
    """A restatement that is 1e-9 rad off in one joint of one frame is outside 1e-3 of the GPU bound."""
    c = WC.rule_case("angle", 64)
    frames = tuple(a[:64] for a in c["seq"])
    want = {k: c["oracle"][k][0] for k in WC.CONTINUOUS}
    WC.check_window(frames, want)
    off = {k: v.copy() for k, v in want.items()}
    off["global_rot_6d"][5, 7] += 1e-9
    with pytest.raises(AssertionError):
        WC.check_window(frames, off)
    # exactly degenerate: the head x-axis straight up
    seq = WC.sequence(0, 4, 4)  # frame 0: heading 0, pitch 0; turned up by a quarter turn about y
    root = (Rot.from_euler("y", -np.pi / 2) * Rot.from_rotvec(WC.up(seq[1][0]))).as_rotvec()
    seq = (seq[0], WC.f32(np.concatenate([root[None], seq[1][1:]])), seq[2])
    assert WC.first_head_conditioning(seq[1], seq[2])[0] < 1e-5
    with pytest.raises(AssertionError):
        WC.check_window(seq, WO.process_window(*seq, REST_OFFSETS))


def test_many_rows_case():
    c = WC.many_rows_case()
    N = len(c["table"])
    assert N == 2199 and (c["table"][:, 3] == 40).all()
    assert N * 40 * 198 > 65535 * 256 >= (WC.MOTION_GRID_CAP_ROW - 2) * 198  # past win_motion_kernel's grid cap, and only just
    assert N * 40 // 1024 >= 85  # rows per win_minmax_kernel workgroup
    assert c["pick"] == [0, 2117, 2118, 2119, 2198] and 2118 * 40 <= WC.MOTION_GRID_CAP_ROW < 2119 * 40
    assert max(c["fp64_paths"].values()) < 1e-12


def test_oracle_equals_the_reference_on_the_edge_fixture(g):
    """The bars of test_oracle_equals_the_reference_within_its_rounding: the distance the generator recorded, and 27 float32 roundings
    of 2^-24 relative to the output's largest magnitude (at least 1).  The second is the reference's error in the head's rotation
    matrix; its heading is atan2 of two entries whose hypotenuse is the head x-axis' horizontal projection h <= 1, so whatever
    the heading turns (every output here) feels that error divided by h: at pitch 0 (h = 1) the bar is the existing one."""
    assert [str(k) for k in g["distance_keys"]] == list(WC.CONTINUOUS) and np.array_equal(g["heading_cases"], np.array(WC.HEADING_CASES))
    assert np.array_equal(g["angles"], WC.ANGLES_ALL)
    step = int(g["row_step"])
    worst = {}
    for W in g["windows"]:
        for kind in g["kinds"]:
            tag = "%s_w%d" % (kind, W)
            c = WC.rule_case(str(kind), int(W))
            table, orc = c["table"], c["oracle"]
            assert np.array_equal(g[tag + "_table"], table)
            rec = g[tag + "_reference_distance"]
            lengths = table[:, 3]
            edges = np.concatenate([[0], np.cumsum([len(sample_rows(n, step)) for n in lengths])])
            for i, (_, start, _, n) in enumerate(table):
                h, _ = WC.first_head_conditioning(c["seq"][1][start:start + 1], c["seq"][2][start:start + 1])
                assert h <= 1.0 + 1e-12
                for col, k in enumerate(WC.CONTINUOUS[:3]):
                    want = orc[k][i, sample_rows(n, step)]
                    d = np.abs(want - g[tag + "_" + k][edges[i]:edges[i + 1]]).max()
                    assert d <= rec[i, col] and d <= 27 * 2.0 ** -24 * max(1.0, np.abs(orc[k][i]).max()) / min(h, 1.0), (tag, i, k, d, h)
                d = WC.up_to_sign(g[tag + "_recover_rot_quat"][i], orc["recover_rot_quat"][i]).max()
                assert d <= rec[i, 3] <= 27 * 2.0 ** -24 / min(h, 1.0), (tag, i, d)
                key = (str(kind), "pitch %.2f" % WC.HEADING_CASES[i % 21][1] if kind == "heading" else "draws")
                worst[key] = np.maximum(worst.get(key, 0.0), rec[i])
            assert np.array_equal(stored(orc["global_jpos"], lengths, step).shape, g[tag + "_global_jpos"].shape)
    for key, v in sorted(worst.items()):
        print(key, "reference vs oracle:", " ".join("%s %.2e" % kv for kv in zip(WC.CONTINUOUS, v)))
