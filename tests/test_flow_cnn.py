"""The optical-flow ResNet-18 feature extractor without a GPU: the module's reference key names and shapes, state-dict round
trips, checkpoint splitting, the refused modes, the seeded weights, the CPU oracle's own precision, and the C ABI structs."""
import os
import re
from argparse import Namespace

import pytest
import torch

import flow_cnn_oracle as O
from egoego_release_amd import _lib, stage1, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_keys():
    """torchvision resnet18 with fc = Linear(512, 512) under FeatureExtractor's cnn.resnet., spelled out."""
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    keys = [("conv1.weight", (64, 3, 7, 7))] + [(f"bn1.{s}", (64,) if s != "num_batches_tracked" else ()) for s in bn]
    cin = 64
    for li, cout in ((1, 64), (2, 128), (3, 256), (4, 512)):
        for b in (0, 1):
            p = f"layer{li}.{b}."
            c1_in = cin if b == 0 else cout
            for conv, bnn, shape in (("conv1", "bn1", (cout, c1_in, 3, 3)), ("conv2", "bn2", (cout, cout, 3, 3))):
                keys.append((p + conv + ".weight", shape))
                keys += [(p + f"{bnn}.{s}", (cout,) if s != "num_batches_tracked" else ()) for s in bn]
            if li > 1 and b == 0:
                keys.append((p + "downsample.0.weight", (cout, cin, 1, 1)))
                keys += [(p + f"downsample.1.{s}", (cout,) if s != "num_batches_tracked" else ()) for s in bn]
        cin = cout
    keys += [("fc.weight", (512, 512)), ("fc.bias", (512,))]
    return [("cnn.resnet." + k, s) for k, s in keys]


def test_state_dict_has_the_reference_keys_and_shapes():
    m = stage1.FlowFeatureExtractor()
    sd = m.state_dict()
    exp = _expected_keys()
    assert len(exp) == 122
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == exp
    assert not any("layer1.0.downsample" in k or ".1.downsample" in k for k in sd)
    assert tuple(sd["cnn.resnet.conv1.weight"].shape) == (64, 3, 7, 7)
    assert sd["cnn.resnet.bn1.num_batches_tracked"].dtype == torch.long
    assert not m.training  # eval mode from the start


def test_loads_a_state_dict_saved_from_itself(tmp_path):
    a = stage1.FlowFeatureExtractor(seed=3)
    path = tmp_path / "cnn.pt"
    torch.save(a.state_dict(), path)
    b = stage1.FlowFeatureExtractor(seed=0)
    assert not torch.equal(b.state_dict()["cnn.resnet.fc.weight"], a.state_dict()["cnn.resnet.fc.weight"])
    b.load_state_dict(torch.load(path))
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v), k


def test_split_headnet_state_dict_round_trips():
    opt = Namespace(window=60, n_dec_layers=1, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0)
    hn = stage1.HeadFormer(opt, "cuda:0")
    cnn = synthetic.make_flow_cnn_weights(5)
    full = {**cnn, **hn.state_dict()}  # what HeadFormer(input_of_feats=False) saves: cnn.resnet.* beside the transformer
    cnn_sd, head_sd = stage1.split_headnet_state_dict(full)
    assert set(cnn_sd) == set(cnn) and set(head_sd) == set(hn.state_dict())
    assert {**cnn_sd, **head_sd}.keys() == full.keys()
    m = stage1.FlowFeatureExtractor()
    m.load_state_dict(cnn_sd)
    hn.load_state_dict(head_sd)
    for k, v in cnn.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_training_mode_and_other_shapes_raise():
    m = stage1.FlowFeatureExtractor()
    m.train()
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m({"of": torch.zeros(1, 2, 224, 224, 2)})
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m.extract(torch.zeros(2, 224, 224, 2))
    m.eval()
    with pytest.raises(ValueError, match="224"):
        m({"of": torch.zeros(1, 2, 112, 112, 2)})
    with pytest.raises(ValueError, match="224"):
        m.extract(torch.zeros(2, 224, 200, 2))
    with pytest.raises(ValueError):
        m.extract(torch.zeros(2, 224, 224, 3))


def test_make_flow_cnn_weights_is_deterministic():
    a, b = synthetic.make_flow_cnn_weights(7), synthetic.make_flow_cnn_weights(7)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = synthetic.make_flow_cnn_weights(8)
    assert not torch.equal(a["cnn.resnet.layer2.0.conv1.weight"], c["cnn.resnet.layer2.0.conv1.weight"])
    assert (a["cnn.resnet.layer4.1.bn2.running_var"] > 0).all()
    f1, f2 = synthetic.make_flows(3, 1), synthetic.make_flows(3, 1)
    assert (f1 == f2).all() and f1.shape == (3, 224, 224, 2)
    assert 5.0 < abs(f1).max() < 25.0


def test_calibrated_activations_stay_order_one():
    """Running statistics from calibration keep every stage's activations O(1), unlike identity statistics."""
    sd = synthetic.make_flow_cnn_weights(0)
    _, stages = O.forward(sd, synthetic.make_flows(2, 11))
    for s in stages:
        assert 0.3 < float(s.std()) < 10.0, float(s.std())


def test_fp32_oracle_is_within_1e5_of_fp64():
    sd = synthetic.make_flow_cnn_weights(1)
    fl = synthetic.make_flows(2, 4)
    f64, _ = O.forward(sd, fl, torch.float64)
    f32, _ = O.forward(sd, fl, torch.float32)
    assert (f32.double() - f64).abs().max() / f64.abs().max() < 1e-5


def test_flow_weights_struct_matches_the_header():
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    body = src[src.index("typedef struct {", src.index("typedef struct egoego_flow_ctx")):src.index("} egoego_flow_weights;")]
    fields = re.findall(r"const float\*\s*(\w+)(?:\[(\d+)\])?;", body)
    assert [(n, int(d) if d else 1) for n, d in fields] == [
        (n, getattr(t, "_length_", 1)) for n, t in _lib.FlowWeights._fields_]
    assert all(int(n) == _lib.FLOW_N_CONV for _, n in fields[:5])
    assert int(re.search(r"#define EGOEGO_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8


def test_to_accepts_every_form_and_tracks_the_device():
    m = stage1.FlowFeatureExtractor()
    assert m.to(dtype=torch.float32) is m and m.device == torch.device("cuda")
    m.to(device="cpu")
    assert m.device == torch.device("cpu")
    m.device = torch.device("cuda:1")
    m.to(torch.zeros(1), non_blocking=False)
    assert m.device == torch.device("cpu")
    m.device = torch.device("cuda:1")
    m.cpu()
    assert m.device == torch.device("cpu") and m.cnn.resnet.fc.weight.device.type == "cpu"


def test_state_dict_argument_replaces_the_synthetic_weights():
    sd = synthetic.make_flow_cnn_weights(9)
    m = stage1.FlowFeatureExtractor(state_dict=sd)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
