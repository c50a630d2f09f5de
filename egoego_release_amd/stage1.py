"""Stage 1 of EgoEgo on the HIP library: HeadNet (HeadFormer) and GravityNet (HeadNormalFormer) with precomputed optical-flow
features, the ARES demo loader, and the assembly of the head pose that stage 2 consumes.

Reference files (paths relative to the reference root):
    HE = egoego/model/head_estimation_transformer.py         (HeadFormer)
    RN = egoego/model/resnet.py                              (ResNet, FeatureExtractor)
    HN = egoego/model/head_normal_estimation_transformer.py  (HeadNormalFormer)
    TM = egoego/model/transformer_module.py                  (Decoder)
    AD = egoego/data/ares_demo_dataset.py                    (ARESDemoDataset)
    RE = run_egoego.py                                        (the pipeline)

Every per-token and per-frame step runs in libegoego_hip (egoego_s1_*): the decoder and the MLP heads (split-bf16 MFMAs), the
GravityNet input features, the angular-velocity integration with the SLAM rescale, and GravityNet's trajectory.  The host keeps
what the reference itself does in numpy on 3 x 3 matrices: the rotation from the predicted floor normal (Rodrigues, HN:47-63) and
the Umeyama alignment (evo's PoseTrajectory3D.align).  torch is plumbing only; there is no fallback.

FlowFeatureExtractor turns raw optical flow into those features (RN's ResNet-18, egoego_flow_* in libegoego_hip).
"""
import ctypes as C
import os
from collections import defaultdict

import numpy as np
import torch
from torch import nn

from . import _lib, rotations
from ._engine import ContextEngine, EngineCacheMixin
from .synthetic import FLOW_FEATS, FLOW_IMG, Stage1Config, flow_cnn_convs, make_flow_cnn_weights, make_stage1_weights

MAX_WINDOW = 128


def block_spans(T, window):
    """HE:233-236: blocks [b * window, (b + 1) * window) for b < T // window + 1, the empty ones skipped -> [(start, length)]."""
    spans = []
    for b in range(T // window + 1):
        n = min(T, (b + 1) * window) - b * window
        if n > 0:
            spans.append((b * window, n))
    return spans


def gravity_valid_frames(L, window):
    """HN:122-141: a SLAM trajectory of L frames is truncated to window + 1 frames; the number of valid feature rows is L' - 1."""
    return max(min(L, window + 1) - 1, 0)


def _check_cfg(cfg, input_of_feats=True):
    if not input_of_feats:
        raise NotImplementedError("HeadFormer runs on precomputed optical-flow features only (input_of_feats): the ResNet-18 "
                                  "optical-flow CNN is not implemented inside it; extract the features first with "
                                  "FlowFeatureExtractor (split a checkpoint with split_headnet_state_dict)")
    if cfg.d_model != 256:
        raise ValueError(f"stage-1 d_model {cfg.d_model}: only 256 is supported")
    if cfg.n_head * cfg.d_k != 1024 or cfg.n_head * cfg.d_v != 1024 or cfg.n_head != 4:
        raise ValueError(f"stage-1 n_head {cfg.n_head}, d_k {cfg.d_k}, d_v {cfg.d_v}: only 4 x 256 is supported")
    if not 1 <= cfg.window <= MAX_WINDOW:
        raise ValueError(f"stage-1 window {cfg.window}: 1..{MAX_WINDOW} supported")
    if not 1 <= cfg.n_dec_layers <= 8:
        raise ValueError(f"stage-1 n_dec_layers {cfg.n_dec_layers}: 1..8 supported")


class Stage1Engine(ContextEngine):
    """One stage-1 context of libegoego_hip on one GPU."""

    NOUN = "stage 1"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_s1_ctx_create", "egoego_s1_ctx_destroy", "egoego_s1_workspace_bytes"
    CHECK = _lib.check_s1

    def __init__(self, cfg, device):
        _check_cfg(cfg)
        super().__init__(device)
        self.cfg = cfg
        kind = _lib.S1_HEADNET if cfg.kind == "headnet" else _lib.S1_GRAVITYNET
        c = _lib.S1Config(kind, cfg.d_feats, cfg.d_model, cfg.n_head, cfg.n_dec_layers, cfg.d_k, cfg.d_v, cfg.window)
        self._create(C.byref(c), self.dev_index)

    def load(self, sd, prefix=""):
        keep = []

        def p(name):
            t = sd[prefix + name].detach().to(device=self.device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        tr = "action_transformer."
        L = self.cfg.n_dec_layers
        layers = (_lib.LayerWeights * L)()
        for i in range(L):
            a, f = tr + f"layer_stack.{i}.self_attn.", tr + f"layer_stack.{i}.pos_ffn."
            lw = layers[i]
            lw.w_q, lw.b_q = p(a + "w_q.weight"), p(a + "w_q.bias")
            lw.w_k, lw.b_k = p(a + "w_k.weight"), p(a + "w_k.bias")
            lw.w_v, lw.b_v = p(a + "w_v.weight"), p(a + "w_v.bias")
            lw.w_fc, lw.b_fc = p(a + "fc.weight"), p(a + "fc.bias")
            lw.ln1_g, lw.ln1_b = p(a + "layer_norm.weight"), p(a + "layer_norm.bias")
            lw.w_1, lw.b_1 = p(f + "w_1.weight"), p(f + "w_1.bias")
            lw.w_2, lw.b_2 = p(f + "w_2.weight"), p(f + "w_2.bias")
            lw.ln2_g, lw.ln2_b = p(f + "layer_norm.weight"), p(f + "layer_norm.bias")
        w = _lib.S1Weights()
        w.start_conv_w, w.start_conv_b = p(tr + "start_conv.weight"), p(tr + "start_conv.bias")
        w.position_vec = p(tr + "position_vec.weight")
        w.layers = layers
        j = 0
        for pre, dims in self.cfg.head_dims().items():
            names = [f"{pre}_mlp.affine_layers.{k}" for k in range(len(dims) - 1)] + [f"{pre}_fc"]
            for nm in names:
                w.head_w[j], w.head_b[j] = p(nm + ".weight"), p(nm + ".bias")
                j += 1
        with torch.cuda.device(self.dev_index):
            _lib.check_s1(self.lib.egoego_s1_load_weights(self._ctx, C.byref(w), self._stream()))
        del keep

    def encode(self, feats, valid, layers=False):
        """feats [W, window, d_feats] fp32 cuda, valid int32 [W] -> heads ([W, window, 4] | [W, 3]) (+ [L, W, window, 256])."""
        cfg = self.cfg
        W = feats.shape[0]
        if tuple(feats.shape) != (W, cfg.window, cfg.d_feats):
            raise ValueError(f"features {tuple(feats.shape)} != [W, {cfg.window}, {cfg.d_feats}]")
        feats = feats.to(self.device, torch.float32).contiguous()
        valid = valid.to(self.device, torch.int32).contiguous()
        out = torch.empty((W, cfg.window, 4) if cfg.kind == "headnet" else (W, 3), device=self.device)
        dbg = torch.empty(cfg.n_dec_layers, W, cfg.window, cfg.d_model, device=self.device) if layers else None
        ws, n = self._workspace(W)
        with torch.cuda.device(self.dev_index):
            _lib.check_s1(self.lib.egoego_s1_encode(self._ctx, feats.data_ptr(), valid.data_ptr(), W, out.data_ptr(),
                                                    dbg.data_ptr() if dbg is not None else None, ws, n, self._stream()))
        return (out, dbg) if layers else out


# ------------------------------------------------------------------------------------------ parameter containers (reference names)
class _Attn(nn.Module):
    def __init__(self, dm, H, dk, dv):
        super().__init__()
        self.w_q, self.w_k, self.w_v = nn.Linear(dm, H * dk), nn.Linear(dm, H * dk), nn.Linear(dm, H * dv)
        self.fc = nn.Linear(H * dv, dm)
        self.layer_norm = nn.LayerNorm(dm)


class _FFN(nn.Module):
    def __init__(self, dm):
        super().__init__()
        self.w_1, self.w_2 = nn.Conv1d(dm, dm, 1), nn.Conv1d(dm, dm, 1)
        self.layer_norm = nn.LayerNorm(dm)


class _Layer(nn.Module):
    def __init__(self, dm, H, dk, dv):
        super().__init__()
        self.self_attn = _Attn(dm, H, dk, dv)
        self.pos_ffn = _FFN(dm)


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.start_conv = nn.Conv1d(cfg.d_feats, cfg.d_model, 1)
        self.position_vec = nn.Embedding(cfg.window + 1, cfg.d_model)
        self.position_vec.weight.requires_grad_(False)
        self.layer_stack = nn.ModuleList([_Layer(cfg.d_model, cfg.n_head, cfg.d_k, cfg.d_v) for _ in range(cfg.n_dec_layers)])


class _MLP(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.affine_layers = nn.ModuleList([nn.Linear(i, o) for o, i in dims])


class _Stage1Module(nn.Module):
    """Holds the reference's parameters under the reference's names (so a checkpoint's transformer_encoder_state_dict loads)
    and runs them on a Stage1Engine, re-packed whenever the parameters changed."""

    def __init__(self, cfg, device, input_of_feats):
        super().__init__()
        _check_cfg(cfg, input_of_feats)
        self.cfg = cfg
        self.device = device
        self.action_transformer = _Decoder(cfg)
        for pre, dims in cfg.head_dims().items():
            setattr(self, f"{pre}_mlp", _MLP(dims[:-1]))
            setattr(self, f"{pre}_fc", nn.Linear(dims[-1][1], dims[-1][0]))
        with torch.no_grad():  # deterministic start: the seeded synthetic weights (a checkpoint replaces them)
            self.load_state_dict(make_stage1_weights(cfg.kind, cfg, 0))
        self._engine = None
        self._packed = None

    def _version(self):
        return tuple((p.data_ptr(), p._version) for p in self.state_dict().values())

    def engine(self):
        if self._engine is None:
            self._engine = Stage1Engine(self.cfg, self.device)
        v = self._version()
        if v != self._packed:
            self._engine.load(self.state_dict())
            self._packed = v
        return self._engine

    @property
    def _dev(self):
        return self.engine().device


def _opt_get(opt, name, default=None):
    return getattr(opt, name, default)


class HeadFormer(_Stage1Module):
    """Drop-in for HE HeadFormer(opt, device) with input_of_feats: reads opt.window, n_dec_layers, n_head, d_k, d_v, d_model,
    input_of_feats and dist_scale."""

    def __init__(self, opt, device):
        self.opt = opt
        cfg = Stage1Config("headnet", opt.window, opt.n_dec_layers, opt.n_head, opt.d_k, opt.d_v, opt.d_model)
        super().__init__(cfg, device, bool(_opt_get(opt, "input_of_feats", False)))
        self.transformer_window_size = opt.window

    def _integrate(self, heads, T, q0, slam, W0, dist_scale):
        """heads [W, window, 4] cuda; T / W0 per sequence; q0 [B, 4]; slam [B, L, 3] -> quats [B, max T + 1, 4], trans, scale (fp64)."""
        dev = heads.device
        B = q0.shape[0]
        L = slam.shape[1]
        Qmax = int(max(T)) + 1
        quat = torch.zeros(B, Qmax, 4, dtype=torch.float64, device=dev)
        trans = torch.zeros(B, L, 3, dtype=torch.float64, device=dev)
        scale = torch.zeros(B, dtype=torch.float64, device=dev)
        Tt = torch.tensor(T, dtype=torch.int32, device=dev)
        w0 = torch.tensor(W0, dtype=torch.int32, device=dev)
        ln = torch.full((B,), L, dtype=torch.int32, device=dev)
        q0d = q0.to(dev, torch.float64).contiguous()
        sl = slam.to(dev, torch.float64).contiguous()
        eng = self.engine()
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_integrate(heads.data_ptr(), self.cfg.window, Tt.data_ptr(), w0.data_ptr(), q0d.data_ptr(),
                                                      sl.data_ptr(), ln.data_ptr(), B, L, Qmax, float(dist_scale), quat.data_ptr(),
                                                      trans.data_ptr(), scale.data_ptr(), eng._stream()))
        return quat, trans, scale

    def forward(self, data):
        """HE:123-170 on one window per sequence (T <= window tokens, data['seq_len'] valid)."""
        eng = self.engine()
        x = torch.as_tensor(data["of"]).to(eng.device).float()
        B, T, _ = x.shape
        if T > self.cfg.window:
            raise ValueError(f"forward() takes at most window = {self.cfg.window} frames, got {T} (use forward_for_eval)")
        feats = torch.zeros(B, self.cfg.window, self.cfg.d_feats, device=eng.device)
        feats[:, :T] = x
        valid = torch.as_tensor(data["seq_len"]).reshape(B).to(eng.device).to(torch.int32).clamp(0, T)
        heads = eng.encode(feats, valid)
        q0 = torch.as_tensor(data["head_pose"])[:, 0, 3:]
        slam = torch.zeros(B, 1, 3, dtype=torch.float64, device=eng.device)
        quat, _, _ = self._integrate(heads, [T] * B, q0, slam, list(range(B)), 1.0)
        out = defaultdict(list)
        out["head_va"] = heads[:, :T, :3]
        out["head_rot_quat"] = quat.to(torch.as_tensor(data["head_pose"]).dtype)
        out["head_dist_scalar"] = heads[:, :T, 3:4]
        return out

    def forward_for_eval(self, data):
        """HE:214-308 for B sequences of equal length T at once: every block of every sequence in one encode call.
        Extra keys: head_va [B, T, 3], head_dist_scalar [B, T, 1] (before / dist_scale), head_rot_quat [B, T + 1, 4]."""
        eng = self.engine()
        x = torch.as_tensor(data["of"]).to(eng.device).float()
        B, T, F = x.shape
        win = self.cfg.window
        spans = block_spans(T, win)
        nb = len(spans)
        feats = torch.zeros(B, nb * win, F, device=eng.device)
        feats[:, :T] = x
        feats = feats.reshape(B * nb, win, F)
        valid = torch.tensor([n for _, n in spans] * B, dtype=torch.int32, device=eng.device)
        heads = eng.encode(feats, valid)
        slam = torch.as_tensor(data["aligned_slam_trans"])
        q0 = torch.as_tensor(data["head_pose"])[:, 0, 3:]
        quat, trans, scale = self._integrate(heads, [T] * B, q0, slam, [b * nb for b in range(B)], self.opt.dist_scale)
        n = min(trans.shape[1], quat.shape[1])
        out = defaultdict(list)
        out["head_pose"] = torch.cat((trans[:, :n], quat[:, :n]), -1)
        out["pred_scale"] = scale[0] if B == 1 else scale
        hv = heads.reshape(B, nb * win, 4)[:, :T]
        out["head_va"] = hv[..., :3]
        out["head_dist_scalar"] = hv[..., 3:4]
        out["head_rot_quat"] = quat
        return out


# ------------------------------------------------------------------------------------------ the optical-flow CNN (RN)
class FlowCNNEngine(ContextEngine):
    """One flow-CNN context of libegoego_hip on one GPU; frames run in chunks of `chunk_frames` (0 = the library's default)."""

    NOUN = "the flow CNN"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_flow_ctx_create", "egoego_flow_ctx_destroy", "egoego_flow_workspace_bytes"
    CHECK = _lib.check_flow
    N_STAGES = 5
    STAGE_SHAPES = [(56, 56, 64), (56, 56, 64), (28, 28, 128), (14, 14, 256), (7, 7, 512)]

    def __init__(self, device, chunk_frames=0):
        super().__init__(device)
        self.chunk_frames = int(chunk_frames)
        self._create(self.dev_index, self.chunk_frames)

    def load(self, sd, prefix="cnn.resnet."):
        keep = []

        def p(name):
            t = sd[prefix + name].detach().to(device=self.device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        w = _lib.FlowWeights()
        for i, (conv, bn, *_) in enumerate(flow_cnn_convs()):
            w.conv_w[i] = p(conv + ".weight")
            w.bn_w[i], w.bn_b[i] = p(bn + ".weight"), p(bn + ".bias")
            w.bn_mean[i], w.bn_var[i] = p(bn + ".running_mean"), p(bn + ".running_var")
        w.fc_w, w.fc_b = p("fc.weight"), p("fc.bias")
        with torch.cuda.device(self.dev_index):
            _lib.check_flow(self.lib.egoego_flow_load_weights(self._ctx, C.byref(w), self._stream()))
        del keep

    def features(self, flow, stages=False):
        """flow [N, 224, 224, 2] fp32 -> [N, 512] (+ the five stage activations, NHWC, when `stages`)."""
        flow = flow.to(self.device, torch.float32).contiguous()
        N = flow.shape[0]
        out = torch.empty(N, FLOW_FEATS, device=self.device)
        dbg = None
        if stages:
            dbg = torch.empty(N * sum(h * w * c for h, w, c in self.STAGE_SHAPES), device=self.device)
        ws, n = self._workspace(N)
        with torch.cuda.device(self.dev_index):
            _lib.check_flow(self.lib.egoego_flow_features(self._ctx, flow.data_ptr(), N, out.data_ptr(),
                                                          dbg.data_ptr() if dbg is not None else None, ws, n, self._stream()))
        if not stages:
            return out
        st, o = [], 0
        for h, w, c in self.STAGE_SHAPES:
            st.append(dbg[o:o + N * h * w * c].view(N, h, w, c))
            o += N * h * w * c
        return out, st


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


class _ResNet18(nn.Module):
    """torchvision's resnet18 parameters and buffers under its names, fc = Linear(512, 512) (RN:5-23); torchvision itself is
    not needed."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for li in range(1, 5):
            cout = 64 << (li - 1)
            setattr(self, f"layer{li}", nn.Sequential(_BasicBlock(cin, cout, 1 if li == 1 else 2), _BasicBlock(cout, cout, 1)))
            cin = cout
        self.fc = nn.Linear(512, FLOW_FEATS)


class _ResNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = _ResNet18()


class FlowFeatureExtractor(EngineCacheMixin, nn.Module):
    """Drop-in for RN FeatureExtractor (lines 25-50) in eval mode: data['of'] [B, T, 224, 224, 2] -> [B, T, 512], on
    libegoego_hip (split-bf16 implicit-GEMM convolutions, BatchNorm with the running statistics).

    The reference builds its CNN from ImageNet weights (pretrained=True), which cannot be fetched here: this module starts from
    the seeded synthetic weights of make_flow_cnn_weights(seed); load a checkpoint's state dict (122 keys cnn.resnet.*, e.g.
    the first half of split_headnet_state_dict) to replace them, or pass it as `state_dict`, which skips the synthetic weights'
    calibration pass.  The module starts in eval mode.  Training mode would
    normalise with batch statistics, which is not implemented: forward() and extract() raise in train().  `chunk_frames` bounds
    the frames per pass through the workspace (0 = the library's default, 256)."""

    ENGINE = FlowCNNEngine

    def __init__(self, device=None, chunk_frames=0, seed=0, state_dict=None):
        super().__init__()
        self.cnn_fdim = FLOW_FEATS
        self.cnn = _ResNet()
        with torch.no_grad():  # a given state dict skips drawing (and calibrating) the synthetic weights
            self.load_state_dict(state_dict if state_dict is not None else make_flow_cnn_weights(seed))
        for prm in self.cnn.parameters():
            prm.requires_grad = False
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.chunk_frames = int(chunk_frames)
        self._engine = None
        self._packed = None
        self.eval()

    def cuda(self, device=None):
        super().cuda(device)
        if isinstance(device, torch.device):
            self.device = device
        else:
            self.device = torch.device("cuda", device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return self

    def cpu(self):
        super().cpu()
        self.device = torch.device("cpu")
        return self

    def _params_version(self):  # (not `_version`: nn.Module stores its state-dict format version under that name)
        return tuple((p.data_ptr(), p._version) for p in self.state_dict().values())

    def _engine_state(self):
        return self.state_dict()

    def _check(self, flow):
        if self.training:
            raise RuntimeError("FlowFeatureExtractor runs BatchNorm with its running statistics only (eval mode): call .eval() "
                               "first; training-mode batch statistics are not implemented")
        if tuple(flow.shape[-3:]) != (FLOW_IMG, FLOW_IMG, 2):
            raise ValueError(f"optical flow {tuple(flow.shape)}: [..., 224, 224, 2] expected (the reference hard-codes 224 x 224)")

    def extract(self, flow, stages=False):
        """flow [N, 224, 224, 2] (pixels, x and y) -> features [N, 512] fp32 on the module's device.  With `stages`, also the
        activations after the stem and after layer1..4 as NHWC tensors (debugging)."""
        flow = torch.as_tensor(flow)
        self._check(flow)
        if flow.dim() != 4:
            raise ValueError(f"optical flow {tuple(flow.shape)}: [N, 224, 224, 2] expected")
        if flow.shape[0] == 0:
            out = torch.empty(0, FLOW_FEATS, device=self.engine().device)
            return (out, []) if stages else out
        return self.engine().features(flow, stages)

    def forward(self, data):
        """RN:38-50: data['of'] [B, T, 224, 224, 2] -> [B, T, 512]."""
        of = torch.as_tensor(data["of"])
        self._check(of)
        if of.dim() != 5:
            raise ValueError(f"data['of'] {tuple(of.shape)}: [B, T, 224, 224, 2] expected")
        B, T = of.shape[:2]
        return self.extract(of.reshape(B * T, FLOW_IMG, FLOW_IMG, 2)).reshape(B, T, self.cnn_fdim)


def split_headnet_state_dict(sd):
    """A HeadFormer state dict saved with input_of_feats off holds its CNN as cnn.resnet.* (HE:66-72), the names of RN
    FeatureExtractor: -> (cnn_sd for FlowFeatureExtractor, the rest for HeadFormer(input_of_feats=True))."""
    cnn = {k: v for k, v in sd.items() if k.startswith("cnn.")}
    rest = {k: v for k, v in sd.items() if not k.startswith("cnn.")}
    return cnn, rest


def rotation_from_floor_normal(n):
    """HN:47-63 (numpy, float64): the rotation that takes the normal n onto +z (Rodrigues)."""
    a = np.asarray(n, np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    b = np.array([0.0, 0.0, 1.0])
    v = np.cross(a, b)
    c = np.dot(a, b)
    s = np.linalg.norm(v)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + k + k.dot(k) * ((1 - c) / (s ** 2))


def umeyama_rotation(est, ref):
    """The rotation r of evo's PoseTrajectory3D.align(ref, correct_scale=True) (Umeyama 1991, evo.core.geometry.umeyama_alignment)
    on positions [T, 3]: what HN's align_xy_plane_traj keeps (z set to 1 by the caller)."""
    x, y = np.asarray(est, np.float64).T, np.asarray(ref, np.float64).T
    m, n = x.shape
    mx, my = x.mean(axis=1), y.mean(axis=1)
    cov = (1.0 / n) * (y - my[:, None]).dot((x - mx[:, None]).T)
    u, d, v = np.linalg.svd(cov)
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[m - 1, m - 1] = -1
    return u.dot(s).dot(v)


class HeadNormalFormer(_Stage1Module):
    """Drop-in for HN HeadNormalFormer(opt, device, eval_whole_pipeline): reads opt.normal_* with eval_whole_pipeline, else
    opt.window / n_dec_layers / n_head / d_k / d_v / d_model."""

    def __init__(self, opt, device, eval_whole_pipeline=False):
        self.opt = opt
        pre = "normal_" if eval_whole_pipeline else ""
        g = lambda k: getattr(opt, pre + k)  # noqa: E731
        cfg = Stage1Config("gravitynet", g("window"), g("n_dec_layers"), g("n_head"), g("d_k"), g("d_v"), g("d_model"))
        super().__init__(cfg, device, True)
        self.transformer_window_size = cfg.window

    def _frames(self, data):
        eng = self.engine()
        rot = torch.as_tensor(data["head_rot_mat"]).to(eng.device).float()
        trans = torch.as_tensor(data["head_trans"]).to(eng.device).float()
        B, L = rot.shape[:2]
        return rot.reshape(B, L, 9).contiguous(), trans.contiguous(), torch.full((B,), L, dtype=torch.int32, device=eng.device)

    def forward(self, data):
        """HN:118-155: the floor normal of every sequence from its first window + 1 frames."""
        eng = self.engine()
        rot, trans, ln = self._frames(data)
        B, L = rot.shape[:2]
        win = self.cfg.window
        feats = torch.empty(B, win, 18, device=eng.device)
        valid = torch.empty(B, dtype=torch.int32, device=eng.device)
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_gravity_features(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, L, win,
                                                             feats.data_ptr(), valid.data_ptr(), eng._stream()))
        out = defaultdict(list)
        out["pred_normal"] = eng.encode(feats, valid)
        return out

    def _apply(self, rot, trans, ln, Rn, scale, Ral, origin):
        eng = self.engine()
        B, L = rot.shape[:2]
        pose = torch.empty(B, L, 7, dtype=torch.float64, device=eng.device)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(eng.device).contiguous()  # noqa: E731
        Rn, scale, Ral, origin = d(Rn), d(scale), d(Ral), d(origin)
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_gravity_apply(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, L, Rn.data_ptr(),
                                                          scale.data_ptr(), Ral.data_ptr(), origin.data_ptr(), pose.data_ptr(),
                                                          eng._stream()))
        return pose

    def forward_for_eval(self, data, pred_scale=None, use_gt_aligned_rot=False):
        """HN:214-294 for B sequences.  Extra keys: pred_normal [B, 3], normal_rot [B, 3, 3] (normal -> +z), align_rot [B, 3, 3]
        (the Umeyama r)."""
        normal = self.forward(data)["pred_normal"]
        rot, trans, ln = self._frames(data)
        B, L = rot.shape[:2]
        if use_gt_aligned_rot:
            Rn = torch.as_tensor(data["aligned_rot_mat"]).double().cpu().numpy().reshape(-1, 3, 3)[:1].repeat(B, 0)
        else:
            Rn = np.stack([rotation_from_floor_normal(v).astype(np.float32).astype(np.float64) for v in normal.cpu().numpy()])
        if pred_scale is not None:
            scale = torch.as_tensor(pred_scale).double().reshape(-1).cpu().numpy()
        else:
            scale = torch.as_tensor(data["aligned_scale"]).double().reshape(-1).cpu().numpy()
        scale = np.array(np.broadcast_to(scale, (B,)))
        eye = np.tile(np.eye(3), (B, 1, 1))
        est = self._apply(rot, trans, ln, Rn, scale, eye, trans[:, 0].double().cpu().numpy()).cpu().numpy()
        ref = torch.as_tensor(data["ori_head_pose"]).double().cpu().numpy()
        Ral = np.empty((B, 3, 3))
        for b in range(B):
            e, r = est[b, :min(L, ref.shape[1]), :3].copy(), ref[b, :, :3].copy()
            e[:, 2] = 1
            r[:, 2] = 1
            Ral[b] = umeyama_rotation(e, r).astype(np.float32)
        gt = torch.as_tensor(data["ori_head_pose"])
        pose = self._apply(rot, trans, ln, Rn, scale, Ral, gt[:, 0, :3].double().cpu().numpy())
        out = defaultdict(list)
        out["head_trans"] = pose[..., :3]
        out["head_rot_mat"] = rotations.quaternion_to_matrix(pose[..., 3:])
        out["head_pose"] = pose
        gq = gt[..., 3:].to(pose.device).double()
        out["gt_head_trans"] = gt[..., :3].to(pose.device).double()
        out["gt_head_rot_mat"] = rotations.quaternion_to_matrix(gq)
        out["gt_head_pose"] = torch.cat((out["gt_head_trans"], rotations.matrix_to_quaternion(out["gt_head_rot_mat"])), -1)
        out["pred_normal"] = normal
        out["normal_rot"] = torch.from_numpy(Rn)
        out["align_rot"] = torch.from_numpy(Ral)
        return out


def estimate_head_pose(headnet, gravitynet, batch, z_offset=-0.13):
    """RE:104-136: HeadNet's rotations with GravityNet's translation, moved onto the ground-truth start and shifted by z_offset
    (the reference's -0.13, "only for this sequence") -> [B, T, 7] float64 (xyz, quaternion w,x,y,z), what stage 2 takes.
    Also returns the two estimators' outputs."""
    out = headnet.forward_for_eval(batch)
    ori = torch.as_tensor(batch["ori_slam_trans"])
    normal_in = {"head_trans": ori - ori[:, 0:1, :], "head_rot_mat": torch.as_tensor(batch["ori_slam_rot_mat"]),
                 "ori_head_pose": torch.as_tensor(batch["head_pose"])}
    nout = gravitynet.forward_for_eval(normal_in, out["pred_scale"])
    n = min(nout["head_pose"].shape[1], out["head_pose"].shape[1])
    hp = torch.cat((nout["head_pose"][:, :n, :3], out["head_pose"][:, :n, 3:].to(nout["head_pose"].device)), -1).double()
    hp[:, :, :2] -= hp[:, 0:1, :2].clone()
    gt0 = torch.as_tensor(batch["head_pose"])[:, 0:1, :3].to(hp.device).double()
    hp[:, :, :3] += gt0 - hp[:, 0:1, :3]
    hp[:, :, 2] += z_offset
    return hp, out, nout


# ------------------------------------------------------------------------------------------ the ARES demo sequence (AD)
def _quat_to_mat32(q):
    return rotations.quaternion_to_matrix(torch.as_tensor(np.asarray(q, np.float32)).float()).numpy()


def load_slam(npy_path):
    """AD load_data_from_droidslam: [T, 7] (xyz, quaternion w,x,y,z) -> trans [T, 3], rot [T, 3, 3] fp32, quat [T, 4]."""
    d = np.load(npy_path)
    return d[:, :3], _quat_to_mat32(d[:, 3:]), d[:, 3:].astype(np.float32)


def load_slam_res_and_align_first(npy_path, gt_head_pose):
    """AD load_slam_res_and_align_first: rotate the SLAM trajectory so that its first rotation is the ground truth's, and move
    its first position onto the ground truth's -> aligned trans [T, 3], rot [T, 3, 3], quat [T, 4]."""
    trans, rot, _ = load_slam(npy_path)
    gt_rot0 = _quat_to_mat32(gt_head_pose[:1, 3:])[0]
    p2g = torch.from_numpy(np.matmul(gt_rot0, rot[0].T)).float()[None]
    arot = torch.matmul(p2g, torch.from_numpy(rot).float())
    aquat = rotations.matrix_to_quaternion(arot.double()).float().numpy()
    atrans = torch.matmul(p2g, torch.from_numpy(trans).float()[:, :, None])[:, :, 0].numpy()
    atrans = atrans + (gt_head_pose[0:1, :3] - atrans[0:1, :])
    return atrans, arot.numpy(), aquat


ARES_SRC_ROOT = "/viscam/u/jiamanli/datasets/egomotion_syn_dataset/habitat_rendering_replica_all"  # AD:101, of_files' root


def load_ares_demo(data_root_folder):
    """ARESDemoDataset(data_root_folder) as a list of batches of one sequence (what its DataLoader with batch_size=1 yields:
    tensors with a leading batch axis): head_pose [1, T'+1, 7], head_vels [1, T', 6], of [1, T', 512], seq_len, seq_name, and the
    aligned / original SLAM trajectories [1, T'+1, ...]."""
    import joblib
    d = joblib.load(os.path.join(data_root_folder, "demo_ares_data.p"))
    out = []
    for k in range(len(d)):
        item = d[k]
        scene = item["seq_name"].split("-")[0]
        npy = os.path.join(data_root_folder, "droid_slam_res", scene, "-".join(item["seq_name"].split("-")[1:]) + ".npy")
        head_vels = item["head_vels"][:-1]
        T = head_vels.shape[0]
        q = {"head_pose": item["head_qpos"][:T + 1], "head_vels": head_vels[:T], "seq_len": T, "seq_name": item["seq_name"]}
        ofs = []
        for f in item["of_files"][:T]:
            f = f.replace(ARES_SRC_ROOT, data_root_folder)
            ofs.append(np.load(f.replace("raft_flows", "raft_of_feats")))
        q["of"] = np.stack(ofs)
        if os.path.exists(npy):
            at, ar, aq = load_slam_res_and_align_first(npy, item["head_qpos"])
            ot, orot, oq = load_slam(npy)
            q.update(aligned_slam_trans=at[:T + 1], aligned_slam_rot_quat=aq[:T + 1], aligned_slam_rot_mat=ar[:T + 1],
                     ori_slam_trans=ot[:T + 1], ori_slam_rot_quat=oq[:T + 1], ori_slam_rot_mat=orot[:T + 1])
        batch = {}
        for kk, v in q.items():
            if isinstance(v, np.ndarray):
                batch[kk] = torch.from_numpy(np.ascontiguousarray(v))[None]
            elif isinstance(v, str):
                batch[kk] = [v]
            else:
                batch[kk] = torch.tensor([v])
        out.append(batch)
    return out
