"""The stage-2 motion windows on the GPU (egoego_win_*; egoego_release_amd/motion_data.py) against the fp64 oracle
(tests/windows_oracle.py) and the reference's own results (tests/golden/motion_windows_golden.npz), on the golden's inputs:
8 sequences of at most 140 frames, windows of 120 and 40, both branches of canonicalize_init_head.

Bound of a continuous output: 2 x the larger of (a) one float32 ulp of the output's largest magnitude in the fixture and (b) the
reference's own recorded distance from the oracle; the same bound holds against the reference's arrays."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

from egoego_release_amd import harness, motion_data as MD, synthetic
from egoego_release_amd import body as B

import windows_oracle as WO
from test_harness_golden import REST_OFFSETS
from test_motion_windows import RUNS, sample_rows, stored, tag_of, ulp32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = MD.STAT_KEYS


@pytest.fixture(scope="module")
def hg():
    return np.load(os.path.join(ROOT, "tests", "golden", "harness_golden.npz"))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "motion_windows_golden.npz"))


@pytest.fixture(scope="module")
def seqs(hg, g):
    return WO.golden_sequences(hg, g)


def _tuple(seqs, order=None):
    order = range(len(seqs)) if order is None else order
    return tuple(np.concatenate([seqs[k][c] for k in order]) for c in range(3)) + ([len(seqs[k][0]) for k in order],)


@pytest.fixture(scope="module")
def runs(seqs):
    """Per (window, canonicalize): the oracle (computed once, never modified) and the kernels' windows with their results on the host."""
    out = {}
    for window, cano in RUNS:
        table, orc = WO.build(seqs, REST_OFFSETS, window, cano)
        mw = MD.build_motion_windows(_tuple(seqs), REST_OFFSETS, window=window, canonicalize_init_head=cano)
        got = {k: getattr(mw, k).cpu().numpy() for k in WO.KEYS}
        out[(window, cano)] = (table, orc, mw, got)
    return out


def _np(t):
    return t.cpu().numpy()


def test_discrete_results_are_exact(runs, g):
    for (window, cano), (table, orc, mw, got) in runs.items():
        ref = g[tag_of(window, cano) + "_table"]
        assert np.array_equal(np.stack([mw.seq_index, mw.start_t_idx, mw.end_t_idx, mw.length], 1), ref)
        assert mw.seq_len.dtype == torch.int32 and np.array_equal(_np(mw.seq_len), ref[:, 3])
        assert mw.seq_names == [str(k) for k in ref[:, 0]]
        pad = np.arange(window)[None, :] >= ref[:, 3][:, None]
        assert pad.any()
        motion = _np(mw.motion())
        assert motion.shape == (len(ref), window, 198) and motion.dtype == np.float32
        for a in (got["global_jpos"], got["global_jvel"], got["global_rot_6d"], got["local_rot_6d"], motion):
            assert np.all(a[pad] == 0.0) and np.isfinite(a).all()
        assert np.array_equal(_np(mw.padding_mask()), _np(harness.prep_padding_mask(mw.global_jpos, mw.seq_len, window)))


def test_continuous_outputs_against_the_oracle_and_the_reference(runs, g):
    """Measured worst |kernel - oracle| on MI355X: global_jpos 5.96e-08, global_rot_6d and local_rot_6d 2.98e-08, recover_rot_quat
    2.78e-08, the statistics at most 5.73e-08; the reference's own distances are in the fixture and in DESIGN.md section 5h."""
    recorded = dict(zip(g["reference_distance_keys"], g["reference_distance"]))
    step = int(g["row_step"])
    worst = {}
    for (window, cano), (table, orc, mw, got) in runs.items():
        tag = tag_of(window, cano)
        lengths = table[:, 3]
        for k in ("global_jpos", "global_rot_6d", "local_rot_6d"):
            bound = 2 * max(ulp32(orc[k]), recorded[k])
            d = np.abs(got[k] - orc[k]).max()
            dg = np.abs(stored(got[k], lengths, step) - g[tag + "_" + k]).max()
            worst[k] = max(worst.get(k, 0), d)
            print(f"{tag} {k}: vs oracle {d:.3e}, vs reference {dg:.3e}, bound {bound:.3e}")
            assert d <= bound and dg <= bound, (tag, k, d, dg, bound)
        bound = 2 * max(ulp32(orc["recover_rot_quat"]), recorded["recover_rot_quat"])
        for want in (orc["recover_rot_quat"], g[tag + "_recover_rot_quat"]):
            d = np.minimum(np.abs(got["recover_rot_quat"] - want).max(-1), np.abs(got["recover_rot_quat"] + want).max(-1)).max()
            print(f"{tag} recover_rot_quat: {d:.3e}, bound {bound:.3e}")
            assert d <= bound, (tag, d, bound)
        so = WO.stats(orc["global_jpos"], orc["global_jvel"], lengths)
        st = mw.stats()
        assert sorted(st) == sorted(STAT_KEYS)
        for k in STAT_KEYS:
            assert st[k].dtype == np.float32 and st[k].shape == (66,)
            bound = 2 * max(ulp32(so[k]), recorded[k])
            d, dg = np.abs(st[k] - so[k]).max(), np.abs(st[k] - g[tag + "_" + k]).max()
            print(f"{tag} {k}: vs oracle {d:.3e}, vs reference {dg:.3e}, bound {bound:.3e}")
            assert d <= bound and dg <= bound, (tag, k, d, dg, bound)
    print("worst over the runs:", {k: f"{v:.3e}" for k, v in worst.items()})


def test_exact_relations_on_the_kernels_own_outputs(runs):
    for (window, cano), (table, orc, mw, got) in runs.items():
        lengths = table[:, 3]
        real = np.arange(window)[None, :] < lengths[:, None]
        p, v = got["global_jpos"], got["global_jvel"]
        want_v = np.zeros_like(v)
        want_v[:, :-1] = p[:, 1:] - p[:, :-1]  # float32
        want_v[np.arange(window)[None, :] >= lengths[:, None] - 1] = 0.0
        assert np.array_equal(v, want_v)
        st = mw.stats()
        assert np.array_equal(st["global_jpos_min"], p[real].min(0)) and np.array_equal(st["global_jpos_max"], p[real].max(0))
        assert np.array_equal(st["global_jvel_min"], v[real].min(0)) and np.array_equal(st["global_jvel_max"], v[real].max(0))
        lo, hi = (torch.from_numpy(st[k]).cuda() for k in STAT_KEYS[:2])
        want = torch.cat(((mw.global_jpos - lo) / (hi - lo) * 2 - 1, mw.global_rot_6d), -1) * torch.from_numpy(real).cuda()[..., None]
        motion = mw.motion()
        assert float((motion - want).abs().max()) <= 1e-6
        assert torch.equal(motion[..., 66:], mw.global_rot_6d)
        other = {k: v + np.float32(0.25) * (1 if k.endswith("max") else -1) for k, v in st.items()}  # statistics handed in
        lo2, hi2 = (torch.from_numpy(other[k]).cuda() for k in STAT_KEYS[:2])
        want2 = torch.cat(((mw.global_jpos - lo2) / (hi2 - lo2) * 2 - 1, mw.global_rot_6d), -1) * torch.from_numpy(real).cuda()[..., None]
        assert float((mw.motion(other) - want2).abs().max()) <= 1e-6
        head = p[:, 0, 45:47]
        assert np.abs(head).max() <= ulp32(p), np.abs(head).max()
        item = MD.MotionWindowDataset(mw, st)[1]
        assert item["seq_len"] == lengths[1] and torch.equal(item["motion"], motion[1]) and len(MD.MotionWindowDataset(mw)) == len(table)


def test_a_windows_rows_do_not_depend_on_the_batch(runs, seqs):
    table, orc, mw, got = runs[(120, True)]
    # any sequence order
    order = [5, 7, 0, 3, 6, 1, 2, 4]
    mw2 = MD.build_motion_windows(_tuple(seqs, order), REST_OFFSETS)
    t2 = np.stack([np.asarray(order)[mw2.seq_index], mw2.start_t_idx], 1)
    for i, (k, start, _, n) in enumerate(table):
        j = int(np.flatnonzero((t2[:, 0] == k) & (t2[:, 1] == start))[0])
        for key in WO.KEYS:
            assert np.array_equal(_np(getattr(mw2, key)[j]), got[key][i]), (key, i)
    # alone, and under a larger padded window: the 30 frames from frame 60 of the 90-frame sequence
    i = int(np.flatnonzero((table[:, 0] == 4) & (table[:, 1] == 60))[0])
    assert table[i, 3] == 30
    alone = tuple(a[60:90] for a in seqs[4]) + ([30],)
    for window in (120, 40, 200):
        assert np.array_equal(WO.window_table([30], window), [[0, 0, 30, 30]])  # the oracle's rule: one window holding the 30 frames
        one = MD.build_motion_windows(alone, REST_OFFSETS, window=window)
        assert len(one) == 1 and one.global_jpos.shape == (1, window, 66) and int(one.seq_len[0]) == 30
        for key in WO.KEYS[:4]:
            a = _np(getattr(one, key)[0])
            assert np.array_equal(a[:30], got[key][i, :30]) and not a[30:].any(), (key, window)
        assert np.array_equal(_np(one.recover_rot_quat[0]), got["recover_rot_quat"][i])
    # more than one 64-frame chunk either side: a 120-frame window alone
    i = int(np.flatnonzero((table[:, 0] == 7) & (table[:, 1] == 0))[0])
    one = MD.build_motion_windows(tuple(a[:120] for a in seqs[7]) + ([120],), REST_OFFSETS, window=130, min_frames=0)
    for key in WO.KEYS[:4]:
        assert np.array_equal(_np(getattr(one, key)[0, :120]), got[key][i]), key


def test_canonicalize_init_head_false(runs, g):
    """The reference's other branch (dataset:474-508): identity heading; only the first head's xy is taken off."""
    for window in (120, 40):
        table, orc, mw, got = runs[(window, False)]
        assert np.array_equal(got["recover_rot_quat"], np.tile(np.float32([1, 0, 0, 0]), (len(table), 1)))
        cano = runs[(window, True)][3]
        assert np.array_equal(got["global_jpos"][..., 2::3], cano["global_jpos"][..., 2::3]) or \
            np.abs(got["global_jpos"][..., 2::3] - cano["global_jpos"][..., 2::3]).max() <= ulp32(got["global_jpos"])  # z is untouched by a turn about z
        assert np.abs(got["local_rot_6d"][..., 6:] - cano["local_rot_6d"][..., 6:]).max() == 0.0  # only the root's local rotation turns


def test_rest_pose_offsets_equal_the_regressed_joints(seqs):
    """rest_pose_offsets(BodyModel) against J - J[parents] with J from body.regress_joints on the host.  J is the float32 joint
    template; the body kernel runs its FK on it in fp64 and rounds each joint once, and the offsets are one float32 subtraction of
    two such joints: 3 roundings of 2^-24 relative to the largest |J|, bounded here by 4 (1.5e-07 for these models).  Measured on
    MI355X: 1.49e-08 for both seeds."""
    for seed in (0, 3):
        model = synthetic.make_body_model(seed, n_verts=600, n_faces=900)
        jt, _ = B.regress_joints(model["J_regressor"], model["v_template"], model["shapedirs"][:, :, :16])
        parents = np.asarray(model["kintree_table"][0, :22]).astype(np.int64)
        parents[0] = 0
        want = jt[:22].astype(np.float64) - jt[:22][parents].astype(np.float64)
        off = MD.rest_pose_offsets(B.BodyModel(model=model))
        assert off.shape == (22, 3) and off.dtype == torch.float32 and off.is_cuda
        off = _np(off)
        d = np.abs(off - want).max()
        print(f"seed {seed}: rest offsets vs host regression {d:.3e}")
        assert d <= 4 * 2.0 ** -24 * np.abs(jt[:22]).max(), d
        assert np.all(off[0] == 0.0)
    mw = MD.build_motion_windows(_tuple(seqs[:1]), torch.from_numpy(off).cuda(), window=120)  # a device tensor is taken as it is
    assert np.isfinite(_np(mw.global_jpos)).all()


def test_end_to_end_on_the_demo_sequence(runs, hg, seqs):
    """build_motion_windows -> skeleton_stats -> convert_model_res_to_data on motion() with recover_rot_quat returns the input
    rotations and root translations (minus the first head's xy, which the canonical window does not keep: harness, M:369-373).
    Tolerances of test_convert_model_res_roundtrip_on_real_poses_cpu's product path: 2e-5 rad, 1e-5."""
    mw = MD.build_motion_windows({0: {"seq_name": "demo", "trans": hg["demo_trans"], "root_orient": hg["demo_root_orient"],
                                      "body_pose": hg["demo_body_pose"]}}, REST_OFFSETS)
    assert mw.seq_names == ["demo", "demo"] and list(mw.length) == [120, 80]
    ds = mw.skeleton_stats()
    assert isinstance(ds, harness.SkeletonStats)
    aa, root, head = harness.convert_model_res_to_data(ds, mw.motion(), mw.recover_rot_quat.reshape(-1, 1, 1, 4))
    aa, root = _np(aa), _np(root)
    _, raw = WO.build(seqs[:1], REST_OFFSETS, 120, False)  # FK minus the first head's xy, in the original heading
    aa_in = np.concatenate([hg["demo_root_orient"][:, None], hg["demo_body_pose"].reshape(-1, 21, 3)], 1)
    for i, (start, n) in enumerate(((0, 120), (60, 80))):
        d = Rot.from_rotvec(aa[i, :n].reshape(-1, 3).astype(np.float64)) * Rot.from_rotvec(aa_in[start:start + n].reshape(-1, 3)).inv()
        ang = np.abs(d.magnitude()).max()
        dr = np.abs(root[i, :n] - raw["global_jpos"][i, :n, :3]).max()
        print(f"window {i}: angle {ang:.3e} rad, root {dr:.3e}")
        assert ang < 2e-5 and dr < 1e-5


def test_the_files_the_tool_writes(hg, g, seqs, tmp_path):
    import joblib
    spec = importlib.util.spec_from_file_location("build_motion_windows_tool", os.path.join(ROOT, "tools", "build_motion_windows.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    names = [str(n) for n in g["seq_names"]]
    data = {k: {"seq_name": names[k], "trans": s[0], "root_orient": s[1], "body_pose": s[2]} for k, s in enumerate(seqs)}
    joblib.dump(data, tmp_path / "train.p")
    joblib.dump({0: data[0]}, tmp_path / "test.p")
    np.save(tmp_path / "rest.npy", REST_OFFSETS)
    rep = tool.main(["--data", str(tmp_path / "train.p"), "--test_data", str(tmp_path / "test.p"), "--rest_offsets", str(tmp_path / "rest.npy"),
                     "--window", "120", "--out", str(tmp_path / "out")])
    assert rep["train_windows"] == 12 and rep["test_windows"] == 2
    out = tmp_path / "out"
    assert sorted(os.listdir(out)) == ["cano_min_max_mean_std_data_window_120.p", "cano_test_diffusion_amass_window_120.p",
                                       "cano_train_diffusion_amass_window_120.p", "rest_offsets.npy"]
    wd = joblib.load(out / "cano_train_diffusion_amass_window_120.p")
    table = g["w120_cano_table"]
    assert list(wd) == list(range(12))
    dt = [str(x) for x in g["file_dtypes"]]
    it = [str(x) for x in g["file_index_types"]]
    for i in wd:
        assert sorted(wd[i]) == [str(k) for k in g["file_window_keys"]]
        assert wd[i]["seq_name"] == names[table[i, 0]] and wd[i]["start_t_idx"] == table[i, 1] and wd[i]["end_t_idx"] == table[i, 2]
        assert [type(wd[i][k]).__name__ for k in ("start_t_idx", "end_t_idx", "seq_name")] == it
        for k, w, d in (("global_jpos", 66, dt[0]), ("global_jvel", 66, dt[1]), ("global_rot_6d", 132, dt[2])):
            assert wd[i][k].shape == (table[i, 3], w) and str(wd[i][k].dtype) == d
    st = joblib.load(out / "cano_min_max_mean_std_data_window_120.p")
    assert sorted(st) == [str(k) for k in g["file_stats_keys"]]
    for k in st:
        assert st[k].shape == (66,) and str(st[k].dtype) == dt[3]
        assert np.abs(st[k] - g["w120_cano_" + k]).max() < 1e-6
    assert np.array_equal(np.load(out / "rest_offsets.npy"), REST_OFFSETS.astype(np.float32))
    back = MD.MotionWindows.from_window_data_dict(wd, device="cuda")  # what the reference would load, back on the device
    assert np.array_equal(back.stats()["global_jpos_max"], st["global_jpos_max"])
    rep = tool.main(["--data", str(tmp_path / "test.p"), "--rest_offsets", str(tmp_path / "rest.npy"), "--window", "40", "--no_canonicalize",
                     "--out", str(tmp_path / "out2")])
    assert sorted(os.listdir(tmp_path / "out2")) == ["min_max_mean_std_data_window_40.p", "rest_offsets.npy", "train_diffusion_amass_window_40.p"]
