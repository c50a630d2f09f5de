"""Stage 1 (HeadNet / GravityNet) on the CPU: the oracle against the reference's golden, the synthetic weights' key set, and
the host-side rules (block splitting, GravityNet truncation / padding, the demo loader, unsupported configurations)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_oracle as O
from egoego_release_amd import stage1, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"demo": dict(window=60, n_dec_layers=2, normal_window=120, normal_n_dec_layers=2),
        "default": dict(window=90, n_dec_layers=2, normal_window=90, normal_n_dec_layers=4)}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "stage1_golden.npz"))


def weights(g, tag):
    s = SETS[tag]
    sh, sg = (int(v) for v in g["seeds"])
    h = synthetic.make_stage1_weights("headnet", synthetic.Stage1Config("headnet", s["window"], s["n_dec_layers"]), sh)
    n = synthetic.make_stage1_weights("gravitynet", synthetic.Stage1Config("gravitynet", s["normal_window"],
                                                                             s["normal_n_dec_layers"]), sg)
    return h, n


@pytest.mark.parametrize("tag", list(SETS))
def test_oracle_reproduces_reference_golden(g, tag):
    s = SETS[tag]
    sd_h, sd_g = weights(g, tag)
    P = tag + "_"
    oh = O.headnet_eval(sd_h, s["window"], s["n_dec_layers"], g["of"], g["head_pose"][0, 3:], g["aligned_slam_trans"],
                        float(g["dist_scale"]))
    spans = O.block_spans(int(g["seq_len"]), s["window"])
    for b in range(len(spans)):
        L = s["n_dec_layers"] - 1
        assert torch.equal(oh["layers"][L][b], torch.from_numpy(g[P + f"h_block{b}_layer{L}"]))
    assert np.array_equal(torch.cat(oh["va"]).numpy(), g[P + "va"])
    assert np.array_equal(torch.cat(oh["dist"]).numpy(), g[P + "dist"])
    assert oh["pred_scale"] == float(g[P + "pred_scale"])
    assert np.abs(oh["head_pose"] - g[P + "headnet_head_pose"]).max() < 1e-6
    tr = g["ori_slam_trans"] - g["ori_slam_trans"][0:1]
    og = O.gravity_eval(sd_g, s["normal_window"], s["normal_n_dec_layers"], g["ori_slam_rot_mat"], tr, g["head_pose"],
                        float(g[P + "pred_scale"]))
    L = s["normal_n_dec_layers"] - 1
    assert torch.equal(og["layers"][L][0], torch.from_numpy(g[P + f"g_layer{L}"]))
    assert np.array_equal(og["pred_normal"], g[P + "pred_normal"])
    assert np.abs(og["normal_rot"] - g[P + "normal_rot"]).max() < 1e-6
    assert np.abs(og["align_rot"] - g[P + "align_rot"]).max() < 1e-6
    assert np.abs(og["head_pose"] - g[P + "gravity_head_pose"]).max() < 1e-6
    hp = O.assemble(og["head_pose"], oh["head_pose"], g["head_pose"])
    assert np.abs(hp - g[P + "head_pose"]).max() < 1e-6


@pytest.mark.parametrize("tag", list(SETS))
def test_synthetic_weights_match_reference_keys_and_shapes(g, tag):
    sd_h, sd_g = weights(g, tag)
    for sd, kind in ((sd_h, "headnet"), (sd_g, "gravity")):
        keys = [str(k) for k in g[f"{tag}_{kind}_keys"]]
        assert sorted(sd) == keys
        for k, shp in zip(keys, g[f"{tag}_{kind}_shapes"]):
            assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v > 0), k


def test_synthetic_weights_are_seeded():
    c = synthetic.Stage1Config("headnet", 60, 2)
    a, b = synthetic.make_stage1_weights("headnet", c, 3), synthetic.make_stage1_weights("headnet", c, 3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    d = synthetic.make_stage1_weights("headnet", c, 4)
    assert not torch.equal(a["action_va_fc.weight"], d["action_va_fc.weight"])


@pytest.mark.parametrize("T,window,expect", [(139, 60, [(0, 60), (60, 60), (120, 19)]), (120, 60, [(0, 60), (60, 60)]),
                                             (59, 60, [(0, 59)]), (1, 60, [(0, 1)]), (60, 60, [(0, 60)]),
                                             (180, 90, [(0, 90), (90, 90)])])
def test_block_spans_follow_the_reference(T, window, expect):
    assert stage1.block_spans(T, window) == expect
    assert O.block_spans(T, window) == expect
    # the reference's loop: T // window + 1 blocks, empty ones skipped
    ref = [(b * window, min(T, (b + 1) * window) - b * window) for b in range(T // window + 1)]
    assert [r for r in ref if r[1] > 0] == expect


@pytest.mark.parametrize("L,window,valid", [(140, 120, 120), (121, 120, 120), (120, 120, 119), (50, 120, 49), (2, 90, 1),
                                            (1, 90, 0)])
def test_gravity_truncation_and_padding(L, window, valid):
    assert stage1.gravity_valid_frames(L, window) == valid
    rng = np.random.default_rng(L)
    q = rng.standard_normal((L, 4))
    rot = O.quat2mat(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    tr = rng.standard_normal((L, 3)).astype(np.float32)
    f, n = O.gravity_features(rot, tr, window)
    assert n == valid and f.shape == (window, 18)
    assert torch.all(f[valid:] == 0)
    if valid:
        assert torch.allclose(f[0, :6], torch.from_numpy(rot[0, :2].reshape(6)))
        assert torch.allclose(f[valid - 1, 15:], torch.from_numpy(tr[valid] - tr[valid - 1]))


def test_demo_loader_matches_reference_inputs(g, tmp_path):
    root = write_demo_folder(g, tmp_path)
    b = stage1.load_ares_demo(str(root))[0]
    T = int(g["seq_len"])
    assert b["of"].shape == (1, T, 512) and b["head_pose"].shape == (1, T + 1, 7)
    assert int(b["seq_len"][0]) == T
    assert np.array_equal(b["of"][0].float().numpy(), g["of"])
    assert np.abs(b["aligned_slam_trans"][0].numpy() - g["aligned_slam_trans"]).max() < 1e-6
    assert np.abs(b["aligned_slam_rot_mat"][0].numpy() - g["aligned_slam_rot_mat"]).max() < 1e-6
    assert np.abs(b["ori_slam_rot_mat"][0].numpy() - g["ori_slam_rot_mat"]).max() < 1e-6
    assert np.array_equal(b["ori_slam_trans"][0].numpy(), g["ori_slam_trans"])


SEQ = "frl_apartment_4-MPI_HDM05_bk_HDM_bk_03-02_02_120_poses_827_frames_30_fps_b649seq0_samp_5"


def write_demo_folder(g, root):
    """The reference's test_data/ares layout from the golden's arrays (head velocities are not read by stage 1: zeros)."""
    import joblib
    scene, rest = SEQ.split("-", 1)
    fdir = root / scene / rest / "raft_of_feats"
    fdir.mkdir(parents=True)
    files = []
    for i, row in enumerate(g["of"]):
        np.save(fdir / f"{i:05d}.npy", row)
        files.append(f"/viscam/u/jiamanli/datasets/egomotion_syn_dataset/habitat_rendering_replica_all/{scene}/{rest}/raft_flows/"
                     f"{i:05d}.npy")
    T = len(files)
    (root / "droid_slam_res" / scene).mkdir(parents=True)
    np.save(root / "droid_slam_res" / scene / (rest + ".npy"), g["slam_raw"])
    joblib.dump({0: {"seq_name": SEQ, "head_qpos": g["head_pose"], "head_vels": np.zeros((T + 1, 6), np.float32),
                     "of_files": files}}, root / "demo_ares_data.p")
    return root


@pytest.mark.parametrize("bad", [dict(d_model=512), dict(window=129), dict(n_dec_layers=9), dict(d_k=128)])
def test_unsupported_configs_raise(bad):
    opt = Namespace(window=60, n_dec_layers=2, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0)
    for k, v in bad.items():
        setattr(opt, k, v)
    with pytest.raises(ValueError):
        stage1.HeadFormer(opt, "cuda:0")


def test_without_optical_flow_features_raises():
    opt = Namespace(window=60, n_dec_layers=2, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=False, dist_scale=10.0)
    with pytest.raises(NotImplementedError, match="ResNet-18"):
        stage1.HeadFormer(opt, "cuda:0")


def test_module_state_dict_uses_reference_names(g):
    opt = Namespace(window=60, n_dec_layers=2, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                    normal_window=120, normal_n_dec_layers=2, normal_n_head=4, normal_d_k=256, normal_d_v=256, normal_d_model=256)
    hn = stage1.HeadFormer(opt, "cuda:0")  # no GPU call before the first forward
    assert sorted(hn.state_dict()) == [str(k) for k in g["demo_headnet_keys"]]
    gn = stage1.HeadNormalFormer(opt, "cuda:0", eval_whole_pipeline=True)
    assert sorted(gn.state_dict()) == [str(k) for k in g["demo_gravity_keys"]]
    sd_h, _ = weights(g, "demo")
    hn.load_state_dict(sd_h)


def test_umeyama_and_normal_rotation():
    rng = np.random.default_rng(0)
    n = rng.standard_normal(3)
    R = stage1.rotation_from_floor_normal(n)
    assert np.allclose(R @ (n / np.linalg.norm(n)), [0, 0, 1]) and np.allclose(R @ R.T, np.eye(3))
    x = rng.standard_normal((50, 3))
    x[:, 2] = 1
    th = 0.7
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    y = x @ Rz.T
    y[:, 2] = 1
    assert np.allclose(stage1.umeyama_rotation(x, y), Rz)
    assert np.allclose(O.umeyama_r(x.T, y.T), Rz)
