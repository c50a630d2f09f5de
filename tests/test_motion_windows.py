"""The stage-2 motion windows without a GPU: the window rule against the reference's recorded tables, the fp64 oracle
(tests/windows_oracle.py) against the reference's arrays (tests/golden/motion_windows_golden.npz, written by
make_motion_windows_golden.py from the reference's own methods), the window-dictionary round trip, and the public names."""
import os

import numpy as np
import pytest
import torch

import egoego_release_amd as pkg
from egoego_release_amd import _lib, motion_data as MD

import windows_oracle as WO
from test_harness_golden import REST_OFFSETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ((120, True), (120, False), (40, True), (40, False))


def tag_of(window, cano):
    return "w%d_%s" % (window, "cano" if cano else "raw")


def sample_rows(length, step):
    return np.array([t for t in range(length) if t % step == 0 or t >= length - 2])


def stored(arr, lengths, step):
    """The fixture's subset of rows of a padded [N, W, C] array, concatenated."""
    return np.concatenate([arr[i, sample_rows(n, step)] for i, n in enumerate(lengths)])


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


@pytest.fixture(scope="module")
def hg():
    return np.load(os.path.join(ROOT, "tests", "golden", "harness_golden.npz"))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "motion_windows_golden.npz"))


def test_window_table_equals_the_reference(hg, g):
    """Lengths 140, 29, 30, 89, 90, 119, 120 and 140 at window 120 and 40: the reference's own enumeration, exactly."""
    lengths = [len(s[0]) for s in WO.golden_sequences(hg, g)]
    assert lengths == [140, 29, 30, 89, 90, 119, 120, 140]
    for window, cano in RUNS:
        ref = g[tag_of(window, cano) + "_table"]
        got = np.stack(MD.window_table(lengths, window), 1)
        assert got.dtype == np.int64 and np.array_equal(got, ref)
        assert np.array_equal(WO.window_table(lengths, window), ref)
    ref = g["w120_cano_table"]
    assert not (ref[:, 0] == 1).any()  # 29 frames: skipped
    assert [tuple(r[1:]) for r in ref if r[0] == 2] == [(0, 30, 30)]  # end_t_idx = num_steps, one past the last frame
    assert [tuple(r[1:]) for r in ref if r[0] == 4] == [(0, 90, 90), (60, 90, 30)]
    assert [tuple(r[1:]) for r in ref if r[0] == 6] == [(0, 119, 120), (60, 120, 60)]  # a full window keeps end = start + 119


@pytest.mark.parametrize("window", [41, 2, 31])
def test_window_table_equals_the_oracle_rule(window):
    """window = 41: the stride is 20, not 20.5.  min_frames other than 30, empty and one-frame sequences."""
    lengths = [140, 0, 1, 29, 30, 31, 40, 41, 42, 61, 100]
    for min_frames in (30, 1, 0):
        got = np.stack(MD.window_table(lengths, window, min_frames), 1)
        assert np.array_equal(got, WO.window_table(lengths, window, min_frames))
    if window == 41:
        t = np.stack(MD.window_table([140], 41), 1)
        assert list(t[:, 1]) == [0, 20, 40, 60, 80, 100] and list(t[:, 3]) == [41, 41, 41, 41, 41, 40]


def test_oracle_equals_the_reference_within_its_rounding(hg, g):
    """The reference computes in float32 (with a float64 detour for the heading): it may lie a few float32 roundings from the fp64
    oracle.  Bound per output: the longest chain of the tree (root to hand) has 9 joints, each a float32 3 x 3 product or a rotated
    offset of 3 roundings per entry, so 27 roundings of 2^-24 relative to the output's largest magnitude (at least 1: the matrix
    entries).  The recorded distances, which the GPU tests' bounds build on, are re-measured here on the stored rows."""
    seqs = WO.golden_sequences(hg, g)
    step = int(g["row_step"])
    recorded = dict(zip(g["reference_distance_keys"], g["reference_distance"]))
    for window, cano in RUNS:
        tag = tag_of(window, cano)
        table, orc = WO.build(seqs, REST_OFFSETS, window, cano)
        lengths = table[:, 3]
        for k in ("global_jpos", "global_rot_6d", "local_rot_6d"):
            d = np.abs(stored(orc[k], lengths, step) - g[tag + "_" + k]).max()
            assert d <= recorded[k] and d <= 27 * 2.0 ** -24 * max(1.0, np.abs(orc[k]).max()), (tag, k, d)
        assert np.abs(orc["recover_rot_quat"] - g[tag + "_recover_rot_quat"]).max() <= recorded["recover_rot_quat"] < 1e-7
        st = WO.stats(orc["global_jpos"], orc["global_jvel"], lengths)
        for k in st:
            assert np.abs(st[k] - g[tag + "_" + k]).max() <= recorded[k] < 1e-6, (tag, k)
        mo = WO.motion(orc["global_jpos"], orc["global_rot_6d"], lengths, st)
        pick = g[tag + "_item_index"]
        d = np.abs(np.concatenate([mo[i, sample_rows(lengths[i], step)] for i in pick]) - g[tag + "_item_motion"]).max()
        assert d <= recorded["motion"], (tag, d)
    # the raw branch's heading is the identity
    assert np.array_equal(g["w120_raw_recover_rot_quat"], np.tile([1.0, 0, 0, 0], (12, 1)))


def test_window_data_dict_round_trip_on_numpy_data():
    rng = np.random.default_rng(0)
    lengths = [120, 31, 77]
    d = {i: {"seq_name": "s%d" % i, "start_t_idx": 60 * i, "end_t_idx": 60 * i + (119 if n == 120 else n),
             "global_jpos": rng.standard_normal((n, 66)).astype(np.float32), "global_jvel": rng.standard_normal((n, 66)).astype(np.float32),
             "global_rot_6d": rng.standard_normal((n, 132)).astype(np.float32)} for i, n in enumerate(lengths)}
    mw = MD.MotionWindows.from_window_data_dict(d)
    assert mw.window == 120 and len(mw) == 3 and mw.global_jpos.shape == (3, 120, 66) and mw.global_rot_6d.shape == (3, 120, 132)
    assert mw.seq_len.tolist() == lengths and mw.device.type == "cpu"
    assert float(mw.global_jpos[1, 31:].abs().max()) == 0.0
    back = mw.to_window_data_dict()
    assert list(back) == [0, 1, 2]
    for i in d:
        assert set(back[i]) == set(d[i])
        for k in d[i]:
            if isinstance(d[i][k], np.ndarray):
                assert back[i][k].dtype == np.float32 and np.array_equal(back[i][k], d[i][k])
            else:
                assert back[i][k] == d[i][k] and type(back[i][k]) is type(d[i][k])
    assert MD.MotionWindows.from_window_data_dict(d, window=150).global_jvel.shape == (3, 150, 66)
    with pytest.raises(ValueError, match="does not fit"):
        MD.MotionWindows.from_window_data_dict(d, window=100)
    # no CPU path for the arithmetic
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        mw.stats()
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        mw.motion()
    assert mw.padding_mask().shape == (3, 1, 121) and mw.padding_mask()[1, 0].sum() == 32


def test_public_names_import_without_a_gpu_and_the_call_raises_cleanly(hg):
    for name in ("build_motion_windows", "window_table", "MotionWindows", "MotionWindowDataset", "rest_pose_offsets"):
        assert getattr(pkg, name) is getattr(MD, name)
    if torch.cuda.is_available():
        return  # the GPU tests cover the call
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        pkg.build_motion_windows((hg["demo_trans"], hg["demo_root_orient"], hg["demo_body_pose"], [140]), REST_OFFSETS)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        pkg.build_motion_windows({0: {"trans": hg["demo_trans"], "root_orient": hg["demo_root_orient"], "body_pose": hg["demo_body_pose"],
                                      "seq_name": "demo"}}, REST_OFFSETS, device="cpu")
