"""The host plumbing the satellite modules share (csrc/host_util.h, _engine.py) on the GPU, through the smallest call of each
context engine: the workspace and not-loaded contracts of the C entries, a failed load, the grow-only workspace of the engines and
the device guard.  Every refused call returns before a launch; what is compared is bit for bit, so there is no tolerance here."""
import ctypes as C

import numpy as np
import pytest
import torch

from egoego_release_amd import _lib, body, stage1, synthetic

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE, E_WORKSPACE = -1, -3, -4  # include/egoego_hip.h
S1_CFG = synthetic.Stage1Config("headnet", 31, 1)
S1_W = 2
BODY_V = 52


class S1Case:
    """Stage1Engine (headnet, window 31, one layer) on W = 2 windows."""
    shape = (S1_W,)
    last_error = "egoego_s1_last_error"

    def __init__(self, dev, sd):
        self.eng = stage1.Stage1Engine(S1_CFG, dev)
        self.eng.load(sd)
        rng = np.random.default_rng(11)
        self.feats = torch.from_numpy(rng.standard_normal((S1_W, 31, 512)).astype(np.float32)).to(self.eng.device)
        self.valid = torch.tensor([31, 17], dtype=torch.int32, device=self.eng.device)
        self.out = torch.empty(S1_W, 31, 4, device=self.eng.device)

    def call(self, ws, n, eng=None):
        e = eng or self.eng
        return e.lib.egoego_s1_encode(e._ctx, self.feats.data_ptr(), self.valid.data_ptr(), S1_W, self.out.data_ptr(), None, ws, n,
                                      e._stream())

    def run(self):
        return (self.eng.encode(self.feats, self.valid),)


def flow_weights(sd, dev, prefix="cnn.resnet."):
    """The egoego_flow_weights struct of a state dict, as FlowCNNEngine.load fills it -> (struct, the tensors it points into)."""
    keep = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in sd.items() if v.is_floating_point()}
    p = lambda name: keep[prefix + name].data_ptr()  # noqa: E731
    w = _lib.FlowWeights()
    for i, (conv, bn, *_) in enumerate(synthetic.flow_cnn_convs()):
        w.conv_w[i] = p(conv + ".weight")
        w.bn_w[i], w.bn_b[i] = p(bn + ".weight"), p(bn + ".bias")
        w.bn_mean[i], w.bn_var[i] = p(bn + ".running_mean"), p(bn + ".running_var")
    w.fc_w, w.fc_b = p("fc.weight"), p("fc.bias")
    return w, keep


class FlowCase:
    """FlowCNNEngine (chunk 1) on N = 1 frame."""
    shape = (1,)
    last_error = "egoego_flow_last_error"

    def __init__(self, dev, sd):
        self.eng = stage1.FlowCNNEngine(dev, 1)
        self.eng.load(sd)
        self.flow = torch.from_numpy(synthetic.make_flows(1, 1)).to(self.eng.device)
        self.out = torch.empty(1, 512, device=self.eng.device)

    def call(self, ws, n, eng=None):
        e = eng or self.eng
        return e.lib.egoego_flow_features(e._ctx, self.flow.data_ptr(), 1, self.out.data_ptr(), None, ws, n, e._stream())

    def run(self):
        return (self.eng.features(self.flow),)


class BodyCase:
    """BodyEngine on a 52-vertex model (the smallest synthetic.make_body_model draws), N = 1 frame of one sequence."""
    shape = (1, 1)
    last_error = "egoego_body_last_error"

    def __init__(self, dev, arrays):
        self.eng = body.BodyEngine(dev)
        self.eng.load(arrays)
        aa, trans = synthetic.make_body_poses(1, 52, seed=4)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)  # noqa: E731
        self.root, self.body, self.hand, self.trans = t(aa[:, 0]), t(aa[:, 1:22].reshape(1, 63)), t(aa[:, 22:].reshape(1, 90)), t(trans)
        self.betas = t(np.random.default_rng(5).uniform(-2, 2, (1, 16)).astype(np.float32))
        self.seq = torch.zeros(1, dtype=torch.int32, device=self.eng.device)
        self.verts = torch.empty(1, BODY_V, 3, device=self.eng.device)
        self.joints = torch.empty(1, 52, 3, device=self.eng.device)

    def call(self, ws, n, eng=None):
        e = eng or self.eng
        return e.lib.egoego_body_forward(e._ctx, self.root.data_ptr(), self.body.data_ptr(), self.hand.data_ptr(), self.trans.data_ptr(),
                                         self.betas.data_ptr(), self.seq.data_ptr(), 1, 1, self.verts.data_ptr(),
                                         self.joints.data_ptr(), None, ws, n, e._stream())

    def run(self):
        return self.eng.forward(self.root, self.body, self.hand, self.trans, self.betas, self.seq)


@pytest.fixture(scope="module")
def weights():
    return {"s1": synthetic.make_stage1_weights("headnet", S1_CFG, 3),
            "flow": synthetic.make_flow_cnn_weights(0, calib_frames=1),
            "body": body.load_model_arrays(synthetic.make_body_model(3, n_verts=BODY_V, n_faces=16, max_weights=4))}


def make_cases(weights, dev):
    return {"s1": S1Case(dev, weights["s1"]), "flow": FlowCase(dev, weights["flow"]), "body": BodyCase(dev, weights["body"])}


@pytest.fixture(scope="module")
def cases(weights):
    """The three engines on cuda:0, each loaded once, with the results of their first call."""
    cs = make_cases(weights, "cuda:0")
    for c in cs.values():
        c.base = tuple(t.clone() for t in c.run())
    return cs


def err(case):
    return getattr(case.eng.lib, case.last_error)().decode()


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["s1", "flow", "body"])
def test_workspace_contract(cases, name):
    c = cases[name]
    need = getattr(c.eng.lib, c.eng.WORKSPACE_BYTES)(c.eng._ctx, *c.shape)
    assert need > 0
    buf = torch.empty(need + 512, dtype=torch.uint8, device=c.eng.device)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    with torch.cuda.device(c.eng.dev_index):
        for p, n in ((ws, need - 1), (ws + 16, need + 16), (None, need)):
            assert c.call(p, n) == E_WORKSPACE, (p, n)
            assert err(c).startswith("workspace:"), err(c)
        assert c.call(ws, need) == 0, err(c)  # the exact size at an aligned pointer is enough
    assert same(c.run(), c.base)


def test_a_context_that_was_never_loaded_says_so(cases):
    s1, flow = cases["s1"], cases["flow"]
    fresh = stage1.Stage1Engine(S1_CFG, "cuda:0")
    assert s1.call(None, 0, fresh) == E_STATE and fresh.lib.egoego_s1_last_error().decode() == "weights not loaded"
    fresh = stage1.FlowCNNEngine("cuda:0", 1)
    assert flow.call(None, 0, fresh) == E_STATE and fresh.lib.egoego_flow_last_error().decode() == "weights not loaded"
    fresh = body.BodyEngine("cuda:0")
    assert fresh.lib.egoego_body_workspace_bytes(fresh._ctx, 1, 1) == 0
    assert fresh.lib.egoego_body_last_error().decode() == "model not loaded"
    with pytest.raises(_lib.EgoEgoHipError, match="^model not loaded$"):
        fresh._workspace(1, 1)


def test_a_failed_load_frees_and_leaves_the_context_usable(cases, weights):
    c = cases["flow"]
    e = c.eng
    w, keep = flow_weights(weights["flow"], e.device)
    w.fc_b = None
    with torch.cuda.device(e.dev_index):
        assert e.lib.egoego_flow_load_weights(e._ctx, C.byref(w), e._stream()) == E_INVALID
        assert err(c) == "a weight pointer is NULL"
        ws, n = e._workspace(1)
        assert c.call(ws, n) == E_STATE and err(c) == "weights not loaded"
        w, keep = flow_weights(weights["flow"], e.device)
        assert e.lib.egoego_flow_load_weights(e._ctx, C.byref(w), e._stream()) == 0, err(c)
    del keep
    assert same(c.run(), c.base)


def test_the_engines_workspace_only_grows():
    e = stage1.Stage1Engine(S1_CFG, "cuda:0")
    need = lambda W: e.lib.egoego_s1_workspace_bytes(e._ctx, W)  # noqa: E731
    p4, n4 = e._workspace(4)
    first = e._ws
    assert p4 % 256 == 0 and n4 >= need(4) and first.numel() == need(4) + 256
    p8, n8 = e._workspace(8)
    grown = e._ws
    assert grown is not first and grown.numel() == need(8) + 256 and p8 % 256 == 0 and n8 >= need(8)
    p2, n2 = e._workspace(2)
    assert e._ws is grown and e._ws.data_ptr() == grown.data_ptr() and (p2, n2) == (p8, n8)
    with pytest.raises(_lib.EgoEgoHipError, match="^n_windows must be >= 1$"):
        e._workspace(0)
    e.close()
    assert not e._ctx.value
    e.close()  # a second close is a no-op


def test_the_device_guard_restores_the_callers_device(weights):
    if torch.cuda.device_count() < 2:
        pytest.skip("the device guard needs two visible devices to show; only one is visible")
    cs = make_cases(weights, "cuda:1")
    torch.cuda.set_device(0)
    for name, c in cs.items():
        assert c.eng.device == torch.device("cuda", 1) and c.eng.dev_index == 1
        ws, n = c.eng._workspace(*c.shape)
        assert c.call(ws, n) == 0, (name, err(c))
        assert torch.cuda.current_device() == 0, name
        assert c.call(ws, 1) == E_WORKSPACE and torch.cuda.current_device() == 0, name
        c.run()
        assert torch.cuda.current_device() == 0, name
        torch.cuda.synchronize(1)
        c.eng.close()
        assert torch.cuda.current_device() == 0, name
