"""Stage-1 training, the parts that need no GPU: the oracle of tests/stage1_train_oracle.py against the reference's recorded run
(tests/golden/stage1_train_golden.npz), the opt-in flag, the C ABI additions, the trainer's checkpoint keys and the refusal of CPU
tensors."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_oracle as S1
import stage1_train_oracle as O
from egoego_release_amd import _lib, stage1, stage1_train, trainer
from egoego_release_amd.synthetic import make_stage1_train_batch, make_stage1_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "stage1_train_golden.npz"))
WINDOW, LAYERS, B = 8, 1, 3
NEW = ("egoego_s1_train_last_error", "egoego_s1_train_ctx_create", "egoego_s1_train_ctx_destroy", "egoego_s1_train_workspace_bytes",
       "egoego_s1_train_saves_bytes", "egoego_s1_train_forward", "egoego_s1_train_backward", "egoego_s1_train_dropout_mask",
       "egoego_s1_train_saved", "egoego_s1_headnet_loss_workspace_bytes", "egoego_s1_headnet_loss")


def _opt(window=WINDOW, layers=LAYERS):
    w = GOLD["weights"]
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True,
                     w_rotation=float(w[0]), w_va=float(w[1]), w_dist=float(w[2]), dist_scale=float(w[3]))


def _digest(g):
    g = g.detach().double().reshape(-1)
    first = np.zeros(64)
    first[:min(64, g.numel())] = g[:64].numpy()
    return np.concatenate(([float(g.norm()), float(g.sum())], first))


def _check_digests(lv, names, want, tag):
    """The recorded digest of every parameter gradient: its L2 norm, its sum and its first 64 entries.  The reference ran in fp32
    and so does the oracle here: they differ by the order of fp32 sums only (1e-6 measured; 1e-4 of the tensor's norm allowed)."""
    total = np.sqrt((want[:, 0] ** 2).sum())
    for k, w in zip(names, want):
        got = _digest(lv[str(k)].grad)
        scale = max(w[0], 1e-6 * total)
        assert abs(got[0] - w[0]) <= 1e-4 * scale, (tag, k, got[0], w[0])
        assert np.abs(got[2:] - w[2:]).max() <= 1e-4 * scale, (tag, k)
        assert abs(got[1] - w[1]) <= 1e-4 * scale * np.sqrt(lv[str(k)].numel()), (tag, k, got[1], w[1])


def test_oracle_reproduces_the_reference_headnet():
    sd = make_stage1_weights("headnet", _opt(), int(GOLD["seeds"][0]))
    data = {"of": torch.from_numpy(GOLD["h_of"]), "head_pose": torch.from_numpy(GOLD["h_head_pose"]),
            "head_vels": torch.from_numpy(GOLD["h_head_vels"]), "seq_len": torch.from_numpy(GOLD["seq_len"])}
    ls, lv, heads, d_heads = O.headnet_step(sd, data, _opt(), LAYERS, dtype=torch.float32)
    got = np.array([float(ls[k].detach()) for k in ("loss", "orient", "va", "dist")])
    assert np.abs(got - GOLD["h_loss"]).max() <= 1e-5 * np.abs(GOLD["h_loss"]).max()
    assert O.rel_err(heads, torch.from_numpy(GOLD["h_heads"]).double()) <= 1e-5
    assert O.rel_err(d_heads, torch.from_numpy(GOLD["h_d_heads"]).double()) <= 1e-5
    assert sorted(O.trainable(sd)) == [str(k) for k in GOLD["h_names"]] and sum(lv[k].numel() for k in O.trainable(sd)) == 3155460
    assert lv["action_transformer.position_vec.weight"].grad is None
    _check_digests(lv, GOLD["h_names"], GOLD["h_digest"], "headnet")
    # fp64 agrees with the fp32 record to fp32's rounding, and the same batch comes out of the seeded generator
    ls64, _, heads64, _ = O.headnet_step(sd, data, _opt(), LAYERS)
    assert abs(float(ls64["loss"].detach()) - GOLD["h_loss"][0]) <= 1e-5 * GOLD["h_loss"][0]
    again = make_stage1_train_batch("headnet", B, WINDOW, seed=3, lengths=(8, 5, 1))
    assert all(np.array_equal(again[k].numpy(), GOLD["h_" + k]) for k in ("of", "head_pose", "head_vels"))


def test_oracle_reproduces_the_reference_gravitynet():
    sd = make_stage1_weights("gravitynet", _opt(), int(GOLD["seeds"][1]))
    rot, trans = torch.from_numpy(GOLD["g_head_rot_mat"]), torch.from_numpy(GOLD["g_head_trans"])
    feats = torch.stack([S1.gravity_features(rot[b], trans[b], WINDOW)[0] for b in range(B)])
    assert np.array_equal(feats.numpy(), GOLD["g_feats"])
    loss, lv, heads, d_heads = O.gravity_step(sd, feats, [WINDOW] * B, torch.from_numpy(GOLD["g_floor_normal"]), LAYERS, dtype=torch.float32)
    assert abs(float(loss.detach()) - GOLD["g_loss"][0]) <= 1e-5 * GOLD["g_loss"][0] and GOLD["g_loss"][0] == GOLD["g_loss"][1]
    assert O.rel_err(heads, torch.from_numpy(GOLD["g_heads"]).double()) <= 1e-5
    assert O.rel_err(d_heads, torch.from_numpy(GOLD["g_d_heads"]).double()) <= 1e-5
    _check_digests(lv, GOLD["g_names"], GOLD["g_digest"], "gravitynet")


def test_oracle_sign_forcing_and_chain_locality():
    """d q_5 / d va is non-zero in row 4 only (va2rot detaches the running rotation), and forcing the decisions the oracle took
    itself changes nothing."""
    d = make_stage1_train_batch("headnet", 2, 8, seed=5)
    va = d["head_vels"][..., 3:].double().clone().requires_grad_(True)
    quat, real = O.va2rot(d["head_pose"][:, 0, 3:].double(), va)
    quat[:, 5].sum().backward()
    rows = va.grad.abs().sum(-1) > 0
    assert rows[:, 4].all() and int(rows.sum()) == 2
    h = torch.cat((d["head_vels"][..., 3:], torch.ones(2, 8, 1)), -1)
    a, ga, r = O.headnet_loss_and_grad(h, 8, d["head_pose"], d["head_vels"], 10.0, 1.0, 1.0, 1.0)
    b, gb, _ = O.headnet_loss_and_grad(h, 8, d["head_pose"], d["head_vels"], 10.0, 1.0, 1.0, 1.0, chain_neg=r["chain_real"] < 0,
                                       diff_neg=r["diff_real"] < 0)
    assert torch.equal(a, b) and torch.equal(ga, gb)
    c, _, _ = O.headnet_loss_and_grad(h, 8, d["head_pose"], d["head_vels"], 10.0, 1.0, 1.0, 1.0, diff_neg=r["diff_real"] >= 0)
    assert torch.equal(a, c)  # |.| makes the orientation term blind to the sign of the difference quaternion


def test_the_flag_is_off_by_default_and_forward_reads_it():
    assert stage1.HeadFormer.hip_training is False and stage1.HeadNormalFormer.hip_training is False
    m = stage1.HeadFormer(_opt(), torch.device("cpu"))
    assert m.hip_training is False and m._graph() is False
    m.hip_training = True
    assert m._graph() is True
    with torch.no_grad():
        assert m._graph() is False
    # parameters on the CPU: the training path refuses, as every path of this package does
    with pytest.raises(_lib.EgoEgoHipError, match="cuda"):
        m.train_engine()
    assert "action_transformer.position_vec.weight" in dict(m.named_parameters())
    assert not m.action_transformer.position_vec.weight.requires_grad
    names = stage1_train.param_names(m.cfg)
    assert sorted(names) == sorted(m.state_dict()) and len(names) == 3 + 16 * LAYERS + 16
    g = stage1.HeadNormalFormer(_opt(), torch.device("cpu"))
    assert sorted(stage1_train.param_names(g.cfg)) == sorted(g.state_dict())
    assert [n for n, _, _ in stage1_train.head_linears(g.cfg)] == O.head_linear_names("gravitynet")
    assert [n for n, _, _ in stage1_train.head_linears(m.cfg)] == O.head_linear_names("headnet")


def test_compute_loss_on_cpu_tensors_raises():
    m = stage1.HeadFormer(_opt(), torch.device("cpu"))
    d = make_stage1_train_batch("headnet", 2, WINDOW, seed=0)
    pred = {"head_va": torch.zeros(2, WINDOW, 3), "head_dist_scalar": torch.zeros(2, WINDOW, 1)}
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        m.compute_loss(pred, d)
    g = stage1.HeadNormalFormer(_opt(), torch.device("cpu"))
    dg = make_stage1_train_batch("gravitynet", 2, WINDOW, seed=0)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        g.compute_loss({"pred_normal": torch.zeros(2, 3)}, dg)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1_train.headnet_loss(torch.zeros(2, WINDOW, 4), WINDOW, d["head_pose"], d["head_vels"], 10.0, 1.0, 1.0, 1.0)
    assert "head_rot_quat" in stage1.HeadFormer.compute_loss.__doc__ and "NOT read" in stage1.HeadFormer.compute_loss.__doc__


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in _lib.EXPORTS
    assert "#define EGOEGO_ABI_VERSION 8 " in header  # additive: the version stays
    assert header.index("egoego_s1_train_ctx egoego_s1_train_ctx;") > header.index("int egoego_optim_read_state(")  # behind everything
    assert re.search(r"EGOEGO_S1_TRAIN_SAVED_HEAD_HIDDEN\s*=\s*6", header) and _lib.S1_TRAIN_SAVED["head_hidden"] == 6
    assert {k: v for k, v in _lib.S1_TRAIN_SAVED.items() if k != "head_hidden"} == _lib.TRAIN_SAVED
    from egoego_release_amd import build
    assert "stage1_train.hip" in build.SOURCES
    if os.path.exists(_lib.LIB_PATH) and not build.is_stale():
        lib = _lib.load()
        assert len(lib.egoego_s1_train_forward.argtypes) == 14 and len(lib.egoego_s1_train_backward.argtypes) == 12
        assert len(lib.egoego_s1_headnet_loss.argtypes) == 16 and len(lib.egoego_s1_train_saved.argtypes) == 8
        assert lib.egoego_s1_headnet_loss_workspace_bytes(0) == 0 and lib.egoego_s1_headnet_loss_workspace_bytes(33) == 1024


def test_synthetic_batches_are_seeded_and_well_formed():
    a, b = make_stage1_train_batch("headnet", 3, 16, seed=1, lengths=[16, 4, 0]), make_stage1_train_batch("headnet", 3, 16, seed=1, lengths=[16, 4, 0])
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["of"].shape == (3, 16, 512) and a["head_pose"].shape == (3, 17, 7) and a["head_vels"].shape == (3, 16, 6)
    assert float((a["head_pose"][..., 3:].norm(dim=-1) - 1).abs().max()) < 1e-6
    assert float(a["of"][1, 4:].abs().max()) == 0 and float(a["of"][2].abs().max()) == 0 and float(a["of"][1, :4].abs().min()) > 0
    # predicted (integrated from the true velocities) and true rotations stay within about 1 rad of each other
    q = S1.va2rot(a["head_pose"][0, 0, 3:].numpy(), a["head_vels"][0, :, 3:].numpy())
    dot = np.abs((q * a["head_pose"][0, :, 3:].numpy()).sum(-1)).clip(0, 1)
    assert float(2 * np.arccos(dot).max()) < 1.0
    g = make_stage1_train_batch("gravitynet", 2, 16, seed=1)
    assert g["head_rot_mat"].shape == (2, 17, 3, 3) and g["head_trans"].shape == (2, 17, 3) and g["floor_normal"].shape == (2, 3, 1)
    eye = torch.matmul(g["head_rot_mat"], g["head_rot_mat"].transpose(-1, -2))
    assert float((eye - torch.eye(3)).abs().max()) < 1e-5 and float((g["floor_normal"].norm(dim=1) - 1).abs().max()) < 1e-6
    assert float(g["head_trans"][:, 0].abs().max()) == 0
    with pytest.raises(ValueError):
        make_stage1_train_batch("gravitynet", 2, 16, lengths=[3, 4])


def test_checkpoint_key_set(tmp_path):
    """Stage1Trainer.save writes the reference's keys; the state dict loads into a fresh HeadFormer and splits like a checkpoint
    that carries no CNN."""
    m = stage1.HeadFormer(_opt(), torch.device("cpu"))
    tr = trainer.Stage1Trainer(m, [], save_dir=str(tmp_path), save_interval=1)
    assert m.hip_training is True and m.training and isinstance(tr.optimizer, torch.optim.AdamW)
    assert tr.optimizer.defaults["lr"] == 1e-4 and tr.scheduler.step_size == 1000 and tr.scheduler.gamma == 0.3
    assert trainer.Stage1Trainer(stage1.HeadNormalFormer(_opt(), torch.device("cpu")), []).scheduler.step_size == 2000
    assert tr.train(2) == 2  # no batches: the epochs, the schedule and the checkpoints still run
    path = os.path.join(str(tmp_path), "weights", "train-2.pt")
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "transformer_encoder_state_dict"] and ck["epoch"] == 2
    cnn, rest = stage1.split_headnet_state_dict(ck["transformer_encoder_state_dict"])
    assert not cnn
    fresh = stage1.HeadFormer(_opt(), torch.device("cpu"))
    fresh.load_state_dict(rest)
    tr.load(path)
    assert tr.epoch == 2


def test_a_state_dict_is_tensors_only(tmp_path):
    """A stage-1 module's state_dict() pickles as plain tensors (a weights-only load takes it): no method of the module may hide
    nn.Module's `_version`, the state-dict format version that state_dict() copies into its metadata, nor `_apply`, through which
    .to() / .cuda() move the parameters."""
    from torch import nn
    for cls in (stage1.HeadFormer, stage1.HeadNormalFormer):
        m = cls(_opt(), torch.device("cpu"))
        assert cls._version == nn.Module._version and cls._apply is nn.Module._apply
        path = tmp_path / (cls.__name__ + ".pt")
        torch.save(m.state_dict(), path)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert sorted(sd) == sorted(m.state_dict())
        assert m.double().float() is m  # _apply works
