"""The optical-flow ResNet-18 feature extractor on the MI355X.

Parity, stage by stage: every (weight set, frame, stage) cell of tests/flow_cnn_cases.py is held to a bar derived from oracles,
e_hip <= 2 (e_emul + e_32) + 2^-22 with e(a) = |a - r64|_2 / |r64|_2, for the whole stage; every live channel to the same on its
own norms with the fp32-accumulation oracle's distance d_acc inside the sum (why: flow_cnn_cases.py); the other channels to the
stage's bar on the stage's norm.  Stages 1-4 and the head are isolated: all three oracle modes take the HIP
path's own previous-stage output (extract(..., stages=True), widened to fp64), so nothing accumulates across stages.  Weight
sets: the seeded initialisation and two trained-like ones (folded scales over three decades, variances under eps, negative and
zero BatchNorm weights, dead filters).  Frames: two flow fields, impulses at the corners, a constant, the all-zero flow, +-40 px
and a 20x flow.  The older test against the chained fp64 oracle with one max-norm over all frames stays beside it.

Also: bit-identity of a frame's features and stage tensors whatever the call and the chunk around it, re-packing after in-place
parameter changes, a NaN or Inf pixel (it reaches every feature of its frame, as through the reference's ops, and no other
frame), the drop-in layout and checkpoint path, the features through HIP HeadNet, and the extraction tool on an ARES demo layout.

EGOEGO_FLOW_RECORD=<file>: the measured figures of every cell are written there as JSON (profiles/flow_cnn_stage_error.json is
such a file)."""
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import flow_cnn_cases as K
import flow_cnn_oracle as O
import stage1_oracle as S1O
from egoego_release_amd import stage1, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ceilings tightened from the measured errors (stem 5.1e-6, layer1-4 9.4e-6 / 1.6e-5 / 1.9e-5 / 2.1e-5, features 7.4e-6)
STAGE_BAR = 5e-5   # per stage: max |HIP - fp64| / max |fp64|
FEAT_BAR = 2e-5    # features


def _frames():
    """8 frames: six synthetic ego-motion fields, an all-zero flow and one at +-40 px."""
    fl = np.concatenate([synthetic.make_flows(6, 21), np.zeros((1, 224, 224, 2), np.float32), synthetic.make_flows(1, 22) * 2.0])
    fl[7] = np.clip(fl[7], -40.0, 40.0)
    fl[7, 100:110, 100:110] = [40.0, -40.0]
    return fl


def _cpu(sd):
    return {k: v.cpu() for k, v in sd.items()}


@pytest.fixture(scope="module")
def model():
    m = stage1.FlowFeatureExtractor(seed=4).to("cuda:0")
    return m


def test_stagewise_parity_with_fp64_oracle(model):
    fl = _frames()
    feats, stages = model.extract(torch.from_numpy(fl), stages=True)
    ref, ref_stages = O.forward(_cpu(model.state_dict()), fl, torch.float64)
    errs = []
    for i, (got, exp) in enumerate(zip(stages, ref_stages)):
        exp = exp.permute(0, 2, 3, 1)
        e = float((got.double().cpu() - exp).abs().max() / exp.abs().max())
        errs.append(e)
    ef = float((feats.double().cpu() - ref).abs().max() / ref.abs().max())
    print("flow-CNN relative errors: stem, layer1-4", ["%.2e" % e for e in errs], "features %.2e" % ef)
    for i, e in enumerate(errs):
        assert e < STAGE_BAR, (i, e)
    assert ef < FEAT_BAR, ef
    assert torch.isfinite(feats).all()


_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_FLOW_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _module(wname):
    return stage1.FlowFeatureExtractor(state_dict={k: v.clone() for k, v in K.weights(wname).items()}).to("cuda:0")


@pytest.fixture(scope="module")
def case_frames():
    return torch.from_numpy(K.frames())


@pytest.fixture(scope="module")
def init_call(case_frames):
    """The init weights' module and its one 7-frame call with stages (shared: not modified)."""
    m = _module("init")
    feats, stages = m.extract(case_frames, stages=True)
    return m, feats, stages


@pytest.mark.parametrize("wname", K.WEIGHT_SETS)
def test_every_stage_cell_meets_the_derived_bar(wname, case_frames, init_call):
    """Measured on the MI355X (profiles/flow_cnn_stage_error.json), worst over the 126 cells, as fractions of the bar: whole stage
    0.49 (e_hip / (e_emul + e_32) = 0.99), live channels 0.72, other channels 0.92.  Without d_acc the worst live channel is at 8.4
    bars (features 7.0 to 8.4, layer4 up to 5.9, layer1-2 up to 1.4), with d_acc added once outside the factor at 1.03."""
    if wname == "init":
        _, feats, stages = init_call
    else:
        feats, stages = _module(wname).extract(case_frames, stages=True)
    sd = K.weights(wname)
    assert feats.shape == (7, 512) and [tuple(s.shape) for s in stages] == [(7,) + sh for sh in stage1.FlowCNNEngine.STAGE_SHAPES]
    outs = [K.nchw64(s) for s in stages] + [feats.double().cpu()]
    ins = [case_frames] + outs[:5]
    bad, rec = [], {}
    worst = {k: 0.0 for k in ("whole", "chan", "chan_plain", "chan_acc_once", "other", "ratio", "chan_ratio")}
    for i, sname in enumerate(K.STAGE_NAMES):
        r64, emul, f32, acc = (K.run(sd, i, ins[i], m) for m in ("f64", "emul", "f32", "acc"))
        assert torch.isfinite(outs[i]).all(), sname
        for n, fname in enumerate(K.FRAME_NAMES):
            c = K.cell(outs[i][n], r64[n], emul[n], f32[n], acc[n])
            rec[f"{sname}/{fname}"] = c
            print("%-14s %-9s %-9s e_hip %.2e e_emul %.2e e_32 %.2e  over bar: whole %.3f channel %.3f (without d_acc %.3f, d_acc "
                  "once %.3f) other %.3f  e/(e_emul+e_32): %.3f, worst channel %.3f  live %d" % (
                      wname, sname, fname, c["e_hip"], c["e_emul"], c["e_32"], c["whole"], c["chan"], c["chan_plain"],
                      c["chan_acc_once"], c["other"], c["ratio"], c["chan_ratio"], c["live"]))
            for k in worst:
                if np.isfinite(c[k]):
                    worst[k] = max(worst[k], c[k])
            if not K.passes(c):
                bad.append((sname, fname, c))
    print(wname, "worst:", {k: "%.3f" % v for k, v in worst.items()})
    _record(wname, cells=rec, worst=worst)
    assert not bad, bad


def test_stage_tensors_are_bit_identical_alone_and_across_chunks(case_frames, init_call):
    m, feats, stages = init_call
    for n in (0, 2, 6):
        f1, s1 = m.extract(case_frames[n:n + 1], stages=True)
        assert torch.equal(f1, feats[n:n + 1]), n
        for i in range(5):
            assert torch.equal(s1[i], stages[i][n:n + 1]), (n, i)
    small = stage1.FlowFeatureExtractor(state_dict=K.weights("init"), chunk_frames=3).to("cuda:0")  # chunks of 3, 3 and 1
    assert small.engine().chunk_frames == 3
    f3, s3 = small.extract(case_frames, stages=True)
    assert torch.equal(f3, feats)
    for i in range(5):
        assert torch.equal(s3[i], stages[i]), i


def test_statistics_and_weights_changed_in_place_are_repacked(case_frames):
    m = _module("init")
    fl = case_frames[:2]
    before = m.extract(fl)
    with torch.no_grad():
        m.cnn.resnet.layer2[0].bn1.running_var.mul_(0.25)
        m.cnn.resnet.layer1[1].conv2.weight.mul_(1.5)
    feats, stages = m.extract(fl, stages=True)
    assert not torch.equal(feats, before)
    fresh = stage1.FlowFeatureExtractor(state_dict={k: v.detach().clone() for k, v in m.state_dict().items()}).to("cuda:0")
    f2, s2 = fresh.extract(fl, stages=True)
    assert torch.equal(feats, f2)
    for i in range(5):
        assert torch.equal(stages[i], s2[i]), i


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_pixel_reaches_every_feature_of_its_frame_only(value, case_frames, init_call):
    """As through the reference's ops (F.relu and max_pool2d propagate NaN; the CPU side is asserted in test_flow_cnn_cases.py)."""
    m, feats, _ = init_call
    fl = case_frames[:3].clone()
    fl[1, 100, 57, 0] = value
    out = m.extract(fl)
    torch.cuda.synchronize()
    assert torch.equal(out[0], feats[0]) and torch.equal(out[2], feats[2])
    assert torch.equal(m.extract(case_frames[0:1])[0], out[0]) and torch.equal(m.extract(case_frames[2:3])[0], out[2])
    assert not torch.isfinite(out[1]).any(), int(torch.isfinite(out[1]).sum())


def test_frame_features_are_bit_identical_in_any_call(model):
    fl = torch.from_numpy(synthetic.make_flows(64, 31))
    alone = [model.extract(fl[i:i + 1]) for i in (0, 37, 63)]
    batch = model.extract(fl)
    for j, i in enumerate((0, 37, 63)):
        assert torch.equal(batch[i:i + 1], alone[j]), i
    # frame 37 at two other positions among other frames
    perm = torch.cat((fl[37:38], fl[:37], fl[38:]))
    assert torch.equal(model.extract(perm)[0], batch[37])
    assert torch.equal(model.extract(torch.cat((fl[:5], fl[37:38])))[5], batch[37])
    # a forced small chunk: 64 frames in chunks of 5 (frames 4/5, 9/10, ... straddle chunk boundaries)
    small = stage1.FlowFeatureExtractor(seed=4, chunk_frames=5).to("cuda:0")
    assert small.engine().chunk_frames == 5
    assert torch.equal(small.extract(fl), batch)
    assert small.engine().lib.egoego_flow_workspace_bytes(small.engine()._ctx, 64) < \
        model.engine().lib.egoego_flow_workspace_bytes(model.engine()._ctx, 64)


def test_forward_layout_and_checkpoint_split(model, tmp_path):
    fl = torch.from_numpy(synthetic.make_flows(6, 41)).reshape(2, 3, 224, 224, 2)
    out = model({"of": fl})
    assert out.shape == (2, 3, 512)
    assert torch.equal(out.reshape(6, 512), model.extract(fl.reshape(6, 224, 224, 2)))
    # a HeadNet checkpoint trained without input_of_feats: cnn.resnet.* beside the transformer and heads
    opt = Namespace(window=60, n_dec_layers=1, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0)
    hn = stage1.HeadFormer(opt, "cuda:0")
    torch.save({**model.state_dict(), **hn.state_dict()}, tmp_path / "headnet.pt")
    cnn_sd, head_sd = stage1.split_headnet_state_dict(torch.load(tmp_path / "headnet.pt"))
    m2 = stage1.FlowFeatureExtractor(seed=0).to("cuda:0")
    m2.load_state_dict(cnn_sd)
    hn.load_state_dict(head_sd)
    assert torch.equal(m2({"of": fl}), out)
    # parameters changed in place are re-packed
    with torch.no_grad():
        m2.cnn.resnet.fc.bias += 1.0
    assert torch.allclose(m2({"of": fl}), out + 1.0, atol=1e-5)


def test_features_through_hip_headnet():
    m = stage1.FlowFeatureExtractor(seed=5).to("cuda:0")
    T = 139
    fl = synthetic.make_flows(T, 51)
    feats = m.extract(torch.from_numpy(fl))
    ref_feats, _ = O.forward(_cpu(m.state_dict()), fl, torch.float64)
    window, n_layers = 60, 2
    opt = Namespace(window=window, n_dec_layers=n_layers, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0,
                    input_of_feats=True)
    hn = stage1.HeadFormer(opt, "cuda:0")
    sd = synthetic.make_stage1_weights("headnet", hn.cfg, 61)
    hn.load_state_dict(sd)
    rng = np.random.default_rng(7)
    q0 = rng.standard_normal(4)
    q0 = q0 / np.linalg.norm(q0) * np.sign(q0[0])
    hp = np.zeros((1, T + 1, 7), np.float32)
    hp[0, :, 3:] = q0
    slam = np.cumsum(rng.standard_normal((1, T + 1, 3)) * 0.03, 1).astype(np.float32)
    out = hn.forward_for_eval({"of": feats[None], "head_pose": torch.from_numpy(hp), "aligned_slam_trans": torch.from_numpy(slam)})
    ref = S1O.headnet_eval(sd, window, n_layers, ref_feats.float().numpy(), hp[0, 0, 3:], slam[0], 10.0)
    va, dist = torch.cat(ref["va"]).numpy(), torch.cat(ref["dist"]).numpy()
    e_va = np.abs(out["head_va"][0].cpu().numpy() - va).max() / np.abs(va).max()
    e_dist = np.abs(out["head_dist_scalar"][0].cpu().numpy() - dist).max() / np.abs(dist).max()
    e_q = np.abs(out["head_rot_quat"][0, -1].cpu().numpy() - ref["quat"][-1]).max()
    print("into HeadNet: head_va %.2e  head_dist_scalar %.2e  last quaternion %.2e" % (e_va, e_dist, e_q))
    # measured 1.2e-5 / 8.4e-6 / 9.3e-7
    assert e_va < 5e-5 and e_dist < 5e-5 and e_q < 1e-5, (e_va, e_dist, e_q)


def test_extraction_tool_writes_features_load_ares_demo_reads(model, tmp_path):
    import joblib
    root = str(tmp_path)
    T = 5
    fl = synthetic.make_flows(T + 1, 71)
    of_files = []
    for t in range(T + 1):
        rel = f"/scene0/seq0/raft_flows/{t:05d}.npy"
        os.makedirs(os.path.dirname(root + rel), exist_ok=True)
        np.save(root + rel, fl[t])
        of_files.append(stage1.ARES_SRC_ROOT + rel)
    qpos = np.zeros((T + 2, 7), np.float32)
    qpos[:, 3] = 1.0
    item = {"seq_name": "scene0-seq0", "head_vels": np.zeros((T + 1, 6), np.float32), "head_qpos": qpos, "of_files": of_files}
    joblib.dump({0: item}, os.path.join(root, "demo_ares_data.p"))
    torch.save(model.state_dict(), tmp_path / "cnn.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_flow_features.py"), "--data_root_folder", root,
                        "--checkpoint", str(tmp_path / "cnn.pt"), "--batch", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    batch = stage1.load_ares_demo(root)[0]
    assert batch["of"].shape == (1, T, 512) and batch["of"].dtype == torch.float64
    exp = model.extract(torch.from_numpy(fl)).double().cpu()
    assert torch.equal(batch["of"][0], exp[:T])
    assert np.load(os.path.join(root, "scene0/seq0/raft_of_feats/00005.npy")).dtype == np.float64
