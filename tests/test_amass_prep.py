"""The AMASS preprocessing without a GPU: the fp64 oracle (tests/amass_oracle.py) against the recorded results of the
reference's own process_seq (tests/golden/amass_golden.npz), the host arithmetic of egoego_release_amd/amass_prep.py from
hand-written answers, argument validation and the exports."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amass_oracle as O  # noqa: E402
from egoego_release_amd import _lib, amass_prep as A, build, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "amass_golden.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    seed, n_verts, n_faces = (int(v) for v in z["model"])
    return z, synthetic.make_body_model(seed, n_verts=n_verts, n_faces=n_faces)


# ------------------------------------------------------------------------------------------------ oracle against golden
def test_the_fixture_is_small_and_holds_every_kind_of_sequence(gold):
    z, _ = gold
    assert os.path.getsize(GOLDEN) < 500_000
    kinds = {str(n): str(z[str(n) + "/result"]) for n in z["names"]}
    assert kinds == {"kept_120": "kept", "kept_60": "kept", "kept_30": "kept", "handball_240": "kept", "mislabeled_59": "kept",
                     "terrain": "terrain", "short": "short"}
    assert "BMLhandball" in str(z["handball_240/path"]) and "20160930_50032" in str(z["mislabeled_59/path"])
    assert float(z["handball_240/mocap_framerate"]) == 120 and float(z["mislabeled_59/mocap_framerate"]) == 60  # the labels are wrong


def test_oracle_reproduces_the_reference(gold):
    z, model = gold
    for name in (str(n) for n in z["names"]):
        poses, trans = z[name + "/poses"].astype(np.float64), z[name + "/trans"].astype(np.float64)
        rec, info = O.process_seq(model, str(z[name + "/path"]), poses, trans, z[name + "/mocap_framerate"])
        want = str(z[name + "/result"])
        assert (rec if isinstance(rec, str) else "kept") == want, name
        if want == "short":
            continue
        # the conditions that make the exact comparisons no coin toss
        synthetic.assert_eval_margins(info["raw_joints"], O.corrected_fps(str(z[name + "/path"]), float(z[name + "/mocap_framerate"])))
        assert np.array_equal(info["fc"]["labels"], z[name + "/labels"]), name
        if want == "terrain":
            continue
        O.assert_head_conditions(info["head"])
        assert tuple(rec) == O.RECORD_KEYS
        for k in ("fps", "contacts", "trans", "root_orient", "pose_body", "betas"):
            assert np.array_equal(np.asarray(rec[k]), z[name + "/ref/" + k]), (name, k)
        assert np.asarray(rec["floor_height"]).tobytes() == z[name + "/ref/floor_height"].tobytes() and rec["floor_height"].dtype == np.float32
        for k in O.CONTINUOUS_KEYS:
            ref = z[name + "/ref/" + k]
            assert ref.shape == rec[k].shape and ref.dtype == (np.float64 if k == "head_vels" and info["head"]["same"].any() else np.float32)
            assert O.rel_diff(ref, rec[k]) <= O.REFERENCE_DISTANCE[k] * (1 + 1e-3), (name, k)
        same = np.append(info["head"]["same"], info["head"]["same"][-1])
        assert np.array_equal(np.all(z[name + "/ref/head_vels"][:, 3:] == 0, 1), same), name  # the |1 -+ q0| branch, pair by pair


def test_the_oracles_joints_do_not_depend_on_the_hands(gold):
    """No joint below 22 has an ancestor at or beyond 22: the 22 joints are the same for any hand pose."""
    import body_oracle
    _, model = gold
    par = body_oracle.parents_of(model)
    assert all(par[j] < 22 for j in range(22))
    aa, tr = synthetic.make_body_poses(5, 52, 3)
    a = body_oracle.forward(model, aa, tr, np.zeros((5, 16)))["Jtr"][:, :22]
    b = body_oracle.forward(model, aa[:, :22], tr, np.zeros((5, 16)))["Jtr"][:, :22]
    assert torch.equal(a, b)
    j, R = O.joints_and_head_rot(model, aa[:, 0], aa[:, 1:22].reshape(5, 63), tr)
    assert np.array_equal(j, b.numpy()) and R.shape == (5, 3, 3)


# ------------------------------------------------------------------------------------------------ host arithmetic, by hand
def test_trim_edges():
    assert A.trim_range(10) == (1, 9)
    assert A.trim_range(7) == (0, 6)       # int(0.7) = 0, int(6.3) = 6
    assert A.trim_range(99) == (9, 89)     # int(9.9), int(89.1)
    assert A.trim_range(1300) == (130, 1170)
    assert A.trim_range(1) == (0, 0) and A.trim_range(0) == (0, 0)
    assert all(A.trim_range(n) == O.trim_range(n) for n in range(0, 3000, 7))


def test_frame_rate_corrections_by_path():
    assert A.corrected_fps("amass/BMLhandball/S01_Expert/Trial_upper_left_001_poses.npz", 120.0) == 240
    assert A.corrected_fps("amass/KIT/3/20160930_50032_walk_poses.npz", 100.0) == 59
    assert A.corrected_fps("amass/KIT/3/20161014_50033_poses.npz", 100.0) == 59
    assert A.corrected_fps("amass/KIT/3/20160930_50031_poses.npz", 100.0) == 100.0
    assert A.corrected_fps("amass/CMU/01/01_01_poses.npz", np.float64(120.0)) == 120.0


def test_the_downsample_tables():
    t, fps = A.downsample_table(10, 59)          # 30 / 59 * 10 = 5.08 -> 5 frames: 0, 2.25, 4.5, 6.75, 9 truncated
    assert t.tolist() == [0, 2, 4, 6, 9] and fps == 30 and t.dtype == np.int64
    t, fps = A.downsample_table(120, 59)         # 61.02 -> 61 frames, the step 119 / 60
    assert t.size == 61 and t[:4].tolist() == [0, 1, 3, 5] and t[-1] == 119 and fps == 30
    t, fps = A.downsample_table(8, 120)          # a quarter: 2 frames, the first and the last
    assert t.tolist() == [0, 7] and fps == 30
    t, fps = A.downsample_table(9, 60)           # int(4.5) = 4: 0, 2.67, 5.33, 8
    assert t.tolist() == [0, 2, 5, 8] and fps == 30
    t, fps = A.downsample_table(5, 30.0)         # at the output rate nothing moves and the fps stays the file's value
    assert t.tolist() == [0, 1, 2, 3, 4] and fps == 30.0 and isinstance(fps, float)
    t, fps = A.downsample_table(5, 25)           # below it: "cannot supersample", saved at the data rate
    assert t.tolist() == [0, 1, 2, 3, 4] and fps == 25
    for n, f in ((320, 120.0), (480, 240), (123, 59), (77, 100.0), (50, 30), (41, 24)):
        a, b = A.downsample_table(n, f), O.downsample_table(n, f)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_the_short_rule():
    assert A.is_short(119, 120) and not A.is_short(120, 120) and not A.is_short(121, 120)  # n < 1.0 * fps: n == fps is kept
    assert A.is_short(59, 59.94) and not A.is_short(60, 59.94)
    model = synthetic.make_body_model(0, n_verts=64, n_faces=8)
    seq = lambda T: {"name": "x", "poses": np.zeros((T, 66)), "trans": np.zeros((T, 3)), "mocap_framerate": 120.0}  # noqa: E731
    assert A.process_sequences([seq(148), seq(12)], model) == ["short", "short"]  # 148 -> [14, 133): 119 frames; needs no GPU
    assert A.trim_range(150) == (15, 135)  # 120 frames == fps: kept, and so sent to the GPU
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
            A.process_sequences([seq(150)], model)


def test_the_split_rule():
    names = ["CMU-01-a.npz", "SFU-0005-b.npz", "HumanEva-S1-c.npz", "MPI_HDM05-bk-d.npz", "BMLhandball-S01-e.npz", "KIT-3-MPI_mosh_f.npz",
             "SFU-HumanEva-g.npz", "Transitions_mocap-CMU-h.npz", "BMLmovi-S-i.npz"]
    data = {n: {"seq_name": n} for n in names}
    train, test = A.split(data)
    assert [train[i]["seq_name"] for i in range(len(train))] == ["CMU-01-a.npz", "KIT-3-MPI_mosh_f.npz", "Transitions_mocap-CMU-h.npz",
                                                                  "BMLmovi-S-i.npz"]
    assert [test[i]["seq_name"] for i in range(len(test))] == ["SFU-0005-b.npz", "HumanEva-S1-c.npz", "MPI_HDM05-bk-d.npz",
                                                                "KIT-3-MPI_mosh_f.npz", "SFU-HumanEva-g.npz", "SFU-HumanEva-g.npz",
                                                                "Transitions_mocap-CMU-h.npz"]
    assert list(train) == [0, 1, 2, 3] and list(test) == list(range(7))


def test_collect_gives_the_references_dictionary(gold):
    z, _ = gold
    rec = {k: z["kept_30/ref/" + k] for k in A.RECORD_KEYS}
    d = A.collect({"SFU-s3-kept_30_poses_80_frames_30_fps.npz": rec})
    (name, e), = d.items()
    assert list(e) == ["root_orient", "body_pose", "trans", "beta", "seq_name", "gender", "head_qpos", "head_vels", "global_head_trans",
                       "global_head_rot_6d", "global_head_rot_6d_diff", "global_head_trans_diff"]
    assert e["seq_name"] == name and str(e["gender"]) == "male" and e["beta"].shape == (16,)
    assert e["body_pose"] is not None and np.array_equal(e["body_pose"], rec["pose_body"]) and e["head_vels"].shape == (80, 6)
    assert A.record_file_name("kept_30_poses", rec) == "kept_30_poses_80_frames_30_fps.npz"


# ------------------------------------------------------------------------------------------------ validation, exports
def test_argument_validation():
    z3, z63 = torch.zeros(4, 3), torch.zeros(4, 63)
    model = synthetic.make_body_model(0, n_verts=64, n_faces=8)
    with pytest.raises(ValueError, match="pose_body"):
        A.body_joints(z3, torch.zeros(4, 62), z3, model)
    with pytest.raises(ValueError, match="disagree"):
        A.body_joints(z3, torch.zeros(5, 63), z3, model)
    j = torch.zeros(10, 22, 3)
    with pytest.raises(ValueError, match="joints"):
        A.floor_and_contacts(torch.zeros(10, 21, 3), [0, 10], 30)
    for bad in ([0, 9], [1, 10], [0, 6, 4, 10], [10]):
        with pytest.raises(ValueError, match="offsets"):
            A.floor_and_contacts(j, bad, 30)
    with pytest.raises(ValueError, match="at least 2"):
        A.floor_and_contacts(j, [0, 9, 10], 30)
    with pytest.raises(ValueError, match="fps"):
        A.floor_and_contacts(j, [0, 5, 10], [30, 60, 120])
    with pytest.raises(ValueError, match="at most 65536"):
        A.floor_and_contacts(torch.zeros(65537, 22, 3), [0, 65537], 120)
    with pytest.raises(ValueError, match="tables"):
        A.head_tracks(j, torch.zeros(10, 3, 3), torch.zeros(10, 22), torch.zeros(1), [0, 10], [np.array([0, 10])])
    with pytest.raises(ValueError, match="head_rot"):
        A.head_tracks(j, torch.zeros(9, 3, 3), torch.zeros(10, 22), torch.zeros(1), [0, 10])
    with pytest.raises(ValueError, match="name"):
        A.process_sequences([{"poses": np.zeros((300, 66)), "trans": np.zeros((300, 3)), "mocap_framerate": 30}], model)
    with pytest.raises(ValueError, match="poses"):
        A.process_sequences([{"name": "x", "poses": np.zeros((300, 60)), "trans": np.zeros((300, 3)), "mocap_framerate": 30}], model)
    with pytest.raises(ValueError, match="at most 65536"):
        A.process_sequences([{"name": "x", "poses": np.zeros((82000, 66)), "trans": np.zeros((82000, 3)), "mocap_framerate": 30}], model)
    # no CPU path: well-formed inputs on the CPU raise instead of falling back
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        A.body_joints(z3, z63, z3, model)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        A.floor_and_contacts(j, [0, 10], 30)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        A.head_tracks(j, torch.zeros(10, 3, 3), torch.zeros(10, 22), torch.zeros(1), [0, 10])


def test_skeleton_is_the_body_models_rest_joints():
    from egoego_release_amd import body
    model = synthetic.make_body_model(1, n_verts=128, n_faces=8)
    jt, par = A.skeleton(model)
    want, _ = body.regress_joints(model["J_regressor"], model["v_template"], model["shapedirs"])
    assert jt.dtype == np.float32 and np.array_equal(jt, want[:22])
    assert par == [0] + list(synthetic.body_model_parents()[1:22])
    bm = body.BodyModel(model=model, device="cpu")
    jt2, par2 = A.skeleton(bm)
    assert np.array_equal(jt2, jt) and par2 == par


def test_library_exports_the_amass_entries():
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = [n for n in _lib.EXPORTS if n.startswith("egoego_amass_")]
    assert names == ["egoego_amass_last_error", "egoego_amass_max_frames", "egoego_amass_joints", "egoego_amass_floor_workspace_bytes",
                     "egoego_amass_floor_contacts", "egoego_amass_head"]
    header = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    for n in names:
        assert hasattr(lib, n) and n + "(" in header, n
    assert "#define EGOEGO_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8
    assert "amass_prep.hip" in build.SOURCES
    lib.egoego_amass_max_frames.restype = ctypes.c_int
    lib.egoego_eval_max_frames.restype = ctypes.c_int
    assert lib.egoego_amass_max_frames() == A.MAX_FRAMES == 65536 and lib.egoego_eval_max_frames() == A.LDS_FRAMES == 4096
    L = _lib.load()
    assert L.egoego_amass_floor_workspace_bytes(0, 1) == 0 and L.egoego_amass_floor_workspace_bytes(10, 11) == 0
    assert L.egoego_amass_floor_workspace_bytes(1000, 3) == (33 * (4 * 1000 + 2 * 3) + 255) // 256 * 256
    # the entries fail on their arguments before they touch a device, each in the module's own error slot
    assert L.egoego_amass_joints(None, None, None, None, None, 1, None, None, None) == -1
    assert L.egoego_amass_last_error().decode() == "NULL argument"
    with pytest.raises(_lib.EgoEgoHipError, match="AMASS-preprocessing error -1: NULL argument"):
        _lib.check_amass(-1)
