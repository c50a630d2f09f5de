"""GravityNet's training batches without a GPU (egoego_release_amd/stage1_data.py, csrc/stage1_data.*): the numpy oracle against
the reference's recorded samples, the split rule, the window rule at its edges, the draw mapping on the numpy Philox replica, the
epoch bookkeeping, the ABI and the argument checks that return before any launch.  The GPU side is tests/test_gpu_stage1_data.py.
"""
import os
import re

import numpy as np
import pytest
import torch

import gravity_batch_oracle as O
from egoego_release_amd import _lib, build, stage1_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gravity_batch_golden.npz")
TENSORS = ("ori_head_pose", "head_rot_mat", "head_trans", "aligned_rot_mat", "floor_normal")
SEED = 2 ** 33 + 5


def golden_cases():
    """-> (window, [(case, seq [len, 7], dict of the recorded draws and tensors)])"""
    g = np.load(GOLDEN)
    cases = []
    for key in g.files:
        m = re.fullmatch(r"(train|eval)/([^/]+)/start", key)
        if m:
            case = f"{m.group(1)}/{m.group(2)}"
            rec = {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + "/")}
            cases.append((case, g[f"pose/{m.group(2)}"], rec))
    return int(g["window"]), cases


# ---------------------------------------------------------------------------------------------- the oracle and the golden
def test_oracle_reference_mode_is_the_reference_bit_for_bit():
    W, cases = golden_cases()
    assert len(cases) == 10 and {len(seq) for _, seq, _ in cases} == {31, 17, 18, 19, 40}
    for case, seq, rec in cases:
        q, Rr = O.random_rotation_from_normals(rec["normals"], np.float32)
        assert np.array_equal(q, rec["quat"]), case
        start, n = O.window_of(len(seq), W, case.startswith("eval"), int(rec["start"]))
        assert (start, n) == (int(rec["start"]), int(rec["seq_len"])), case
        got = O.sample(seq, W, start, Rr, float(rec["scale"]), mode="ref32")
        assert got["seq_len"] == n and got["aligned_scale"] == float(rec["aligned_scale"])
        for key in TENSORS:
            assert got[key].dtype == np.float32 and np.array_equal(got[key].view(np.uint32), rec[key].view(np.uint32)), (case, key)
        assert not rec["ori_head_pose"][n:].any() and not rec["head_rot_mat"][n:].any() and not rec["head_trans"][n:].any()


def test_oracle_fp64_mode_is_within_the_reference_s_own_rounding():
    """The reference's float32 tensors sit a few eps of the tensor's largest entry from the float64 restatement (the serial sum of
    head_trans the farthest): 16 units cover 17 frames of accumulated roundings with room to spare; a wrong formula is off by 1e5."""
    W, cases = golden_cases()
    for case, seq, rec in cases:
        _, Rr = O.random_rotation_from_normals(rec["normals"], np.float32)
        f64 = O.sample(seq, W, int(rec["start"]), Rr, np.float32(rec["scale"]), mode="fp64")
        for key in TENSORS[1:]:
            assert O.err_units(rec[key], f64[key]) <= 16.0, (case, key)
        # the telescoped form the kernel uses is the same number in exact arithmetic
        n = int(rec["seq_len"])
        p = seq[int(rec["start"]):int(rec["start"]) + n, :3].astype(np.float64)
        tele = float(np.float32(rec["scale"])) * (p - p[:1]) @ Rr.astype(np.float64).T
        assert O.err_units(tele, f64["head_trans"][:n]) <= 1e-3, case


def test_eval_mode_starts_at_zero_and_train_mode_inside_the_room():
    W, cases = golden_cases()
    for case, seq, rec in cases:
        room = len(seq) - W - 1
        if case.startswith("eval") or room <= 0:
            assert int(rec["start"]) == 0
        else:
            assert 0 <= int(rec["start"]) < room
        assert int(rec["seq_len"]) == (len(seq) if room <= 0 else W + 1)
        assert 0.1 <= float(rec["scale"]) < 10.0


# ---------------------------------------------------------------------------------------------- the split
def test_split_by_dataset_is_divide_train_val():
    g = np.load(GOLDEN)
    names = [str(n) for n in g["names"]]
    train, val = stage1_data.split_by_dataset(names)
    assert train == [n for n in names if not n.startswith("SFU")] and val == ["SFU-06_40"]
    lengths = {n: len(g[f"pose/{n}"]) for n in names}
    keep = lambda ns: [n for n in ns if lengths[n] > stage1_data.MIN_FRAMES]  # noqa: E731
    assert keep(train) == [str(n) for n in g["split_train"]] and keep(val) == [str(n) for n in g["split_val"]]
    assert stage1_data.split_by_dataset(["CMU-1", "CMUx-1", "MPI_HDM05-a", "HumanEva-b", "ACCAD", "BioMotionLab_NTroje-x-y"]) == \
        (["CMU-1", "ACCAD", "BioMotionLab_NTroje-x-y"], ["CMUx-1", "MPI_HDM05-a", "HumanEva-b"])
    assert len(stage1_data.TRAIN_DATASETS) == 9


def test_sequences_of_at_most_30_frames_are_dropped():
    poses = {"a": np.zeros((30, 7)), "b": np.zeros((31, 7)), "c": {"head_qpos": np.zeros((40, 7)), "seq_name": "CMU-c"}}
    assert [n for n, _ in stage1_data._head_poses(poses, None)] == ["b", "CMU-c"]
    assert [n for n, _ in stage1_data._head_poses(poses, ["CMU-c", "a"])] == ["CMU-c"]
    with pytest.raises(ValueError):
        stage1_data._head_poses({"a": np.zeros((40, 6))}, None)


# ---------------------------------------------------------------------------------------------- the window rule and the draws
def test_starts_at_a_room_of_0_1_and_2():
    ids = np.arange(4096)
    assert O.window_of(17, 16, False, 99) == (0, 17)                       # len - W - 1 = 0: no draw
    assert O.window_of(16, 16, False, 99) == (0, 16) and O.window_of(1, 16, False, 99) == (0, 1)
    assert set(O.draw_start(SEED, ids, 1).tolist()) == {0}
    assert set(O.draw_start(SEED, ids, 2).tolist()) == {0, 1}
    assert O.window_of(18, 16, False, 0) == (0, 17) and O.window_of(19, 16, False, 1) == (1, 17)
    assert O.window_of(19, 16, True, 1) == (0, 17)


def test_the_draw_mapping_over_4096_ids():
    ids = np.arange(4096)
    scale = O.draw_scale(SEED, ids)
    assert scale.dtype == np.float32 and float(scale.min()) >= np.float32(0.1) and float(scale.max()) < 10.0
    assert abs(float(scale.astype(np.float64).mean()) - 5.05) <= 0.22     # 5 sigma: sd 2.858 / sqrt(4096)
    Rr = O.draw_rotation(SEED, ids).astype(np.float64)
    assert np.abs(Rr @ Rr.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert np.abs(np.linalg.det(Rr) - 1.0).max() <= 1e-6
    assert np.abs(Rr.mean(0)).max() < 0.045                               # 5 sigma of sqrt(1 / 3 / 4096)
    assert set(O.draw_start(SEED, ids, 7).tolist()) == set(range(7))
    # the extremes of the two integer maps.  In float64 the scale stays below 10; the float32 it is rounded to is 10.0 for the top
    # ~200 of the 2^32 words (float32 is 9.5e-7 apart there), as the reference's own float32 product of a draw that close is.
    top = np.float64(2 ** 32 - 1)
    assert 0.1 + 9.9 * ((top + 0.5) * 2.0 ** -32) < 10.0 and np.float32(0.1 + 9.9 * ((top + 0.5) * 2.0 ** -32)) <= np.float32(10.0)
    assert np.float32(0.1 + 9.9 * (0.5 * 2.0 ** -32)) >= np.float32(0.1)
    assert ((2 ** 32 - 1) * 7) >> 32 == 6


def test_draws_depend_on_the_seed_and_the_draw_id_alone():
    a = O.draw_scale(SEED, [3, 2 ** 40 + 1, 3])
    assert a[0] == a[2] != a[1]
    assert O.draw_scale(SEED + 1, [3])[0] != a[0]
    assert np.array_equal(O.draw_normals(SEED, [5, 6])[1], O.draw_normals(SEED, [6])[0])
    # word 3 of the counter is the tag: no dropout (layer * 4 + site) or sampler (timestep) counter has it
    assert O.DRAW_TAG > 1000 and f"0x{O.DRAW_TAG:08X}u".lower() in open(
        os.path.join(ROOT, "egoego_release_amd", "csrc", "stage1_data.h")).read().lower()


# ---------------------------------------------------------------------------------------------- the epochs
def _epoch(plan):
    order, draws, batches = plan.next_epoch()
    return {int(k): int(d) for k, d in zip(order, draws)}, order, batches


def test_epoch_bookkeeping():
    S = 11
    a, b, c = (stage1_data.EpochPlan(S, bs, shuffle=sh, seed=4) for bs, sh in ((4, True), (3, True), (4, False)))
    assert (len(a), len(b), len(c)) == (3, 4, 3) and len(stage1_data.EpochPlan(8, 4)) == 2 and len(stage1_data.EpochPlan(1, 4)) == 1
    for epoch in range(3):
        da, oa, ba = _epoch(a)
        db, ob, bb = _epoch(b)
        dc, oc, bc = _epoch(c)
        assert da == db == dc == {k: epoch * S + k for k in range(S)}       # independent of batch size and shuffle
        assert sorted(oa.tolist()) == list(range(S)) and np.array_equal(oa, ob) and oc.tolist() == list(range(S))
        assert ba == [(0, 4), (4, 8), (8, 11)] and bb == [(0, 3), (3, 6), (6, 9), (9, 11)] and bc == ba
    assert a.epoch == 3
    assert not np.array_equal(oa, np.arange(S))
    assert not np.array_equal(_epoch(stage1_data.EpochPlan(S, 4, seed=5))[1], _epoch(stage1_data.EpochPlan(S, 4, seed=4))[1])


def test_state_dict_round_trip():
    a = stage1_data.EpochPlan(9, 2, seed=1)
    a.next_epoch()
    state = a.state_dict()
    assert sorted(state) == ["epoch", "generator"] and state["epoch"] == 1
    want = [a.next_epoch() for _ in range(2)]
    b = stage1_data.EpochPlan(9, 2, seed=77)
    b.load_state_dict(state)
    for w in want:
        got = b.next_epoch()
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2]
    assert b.epoch == a.epoch == 3


# ---------------------------------------------------------------------------------------------- the library and the edges
def test_abi():
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    for name in ("egoego_s1_gravity_batch", "egoego_s1_data_last_error"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, src), name
    assert "stage1_data.hip" in build.SOURCES
    assert int(re.search(r"#define EGOEGO_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8  # additive: the version stays
    build.build()
    assert hasattr(_lib.load(), "egoego_s1_gravity_batch")


def test_bad_arguments_return_before_any_launch():
    """window < 1, B < 1 and NULL pointers are refused on the host (EGOEGO_E_INVALID): nothing is launched, so no GPU is needed
    and the made-up addresses are never touched."""
    build.build()
    lib = _lib.load()
    p = 4096  # stands for a non-NULL pointer

    def call(window=16, B=2, n_rows=100, n_seqs=3, ins=(p, p, p, p), planted=(None, None, None), outs=(p,) * 9):
        return lib.egoego_s1_gravity_batch(ins[0], n_rows, ins[1], n_seqs, ins[2], ins[3], B, window, 1, 0, *planted, *outs, None)

    bad = [dict(window=0), dict(window=-3), dict(B=0), dict(B=-1), dict(n_rows=0), dict(n_seqs=0)]
    bad += [dict(ins=tuple(None if j == i else p for j in range(4))) for i in range(4)]
    bad += [dict(outs=tuple(None if j == i else p for j in range(9))) for i in range(9)]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_lib.EgoEgoHipError, match="stage-1 data"):
            _lib.check_s1_data(rc)
    assert "window = 0" in (call(window=0), _lib.check_s1_data.last_error())[1]
    assert int(re.search(r"EGOEGO_E_INVALID\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "egoego_hip.h")).read()).group(1)) == \
        call(B=0)


def test_the_python_checks_that_need_no_gpu():
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1_data.GravityBatches({"a": np.zeros((40, 7), np.float32)}, 2, device="cpu")
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1_data.gravity_batch(torch.zeros(40, 7), [0, 40], [0], [0], 16, 0)
    with pytest.raises(ValueError):
        stage1_data.EpochPlan(0, 4)
    with pytest.raises(ValueError):
        stage1_data.EpochPlan(4, 0)
