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
GravityNet input features, the angular-velocity integration with the SLAM rescale, and GravityNet's trajectory.  In the
equal-length calls the host keeps what the reference itself does in numpy on 3 x 3 matrices: the rotation from the predicted floor
normal (Rodrigues, HN:47-63) and the Umeyama alignment (evo's PoseTrajectory3D.align); with `lengths=` (sequences of different
lengths in one call) both run in egoego_s1_gravity_align and nothing returns to the host.  compute_head_pose_metrics is the
stage-1 score (egoego/eval/head_pose_metrics.py) on the device.  torch is plumbing only; there is no fallback.

FlowFeatureExtractor turns raw optical flow into those features (RN's ResNet-18, egoego_flow_* in libegoego_hip).

Training (opt-in): with `hip_training` set, forward() of either estimator runs the training encode of stage1_train.py and its
outputs are connected to the parameters; compute_loss() is the reference's (HeadNet's on egoego_s1_headnet_loss).  DESIGN.md 5l.
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


def _host_lengths(lengths, B, hi, what, lo=1):
    """`lengths` (host integers or a CPU tensor) -> list of B ints in lo..hi.  A device tensor is refused: the pack of a ragged
    call is built on the host, and reading lengths back would wait for the device."""
    if isinstance(lengths, torch.Tensor):
        if lengths.device.type != "cpu":
            raise ValueError(f"{what} must be host integers or a CPU tensor (the ragged pack is built on the host)")
        lengths = lengths.reshape(-1).tolist()
    a = [int(v) for v in np.asarray(lengths).reshape(-1).tolist()]
    if len(a) != B:
        raise ValueError(f"{what}: {len(a)} values for {B} sequences")
    if a and (min(a) < lo or max(a) > hi):
        raise ValueError(f"{what} span {min(a)}..{max(a)}: {lo}..{hi} (the padded length) expected")
    return a


def _upload(values, dtype, device):
    """Host values -> a device tensor through pinned memory, without waiting for the device."""
    t = torch.as_tensor(np.asarray(values), dtype=dtype)
    if device.type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def _keep_rows(x, n):
    """x [B, T, ...] with rows t >= n[b] (n a device tensor [B]) set to zero, whatever they held (NaN included)."""
    m = torch.arange(x.shape[1], device=x.device)[None, :] < n[:, None]
    return torch.where(m.reshape(m.shape + (1,) * (x.dim() - 2)), x, torch.zeros((), dtype=x.dtype, device=x.device))


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
        self._train_engine = None

    # Opt-in: with hip_training set and grad mode on, forward() runs the training encode of csrc/stage1_train.* (stage1_train.py)
    # and its outputs are connected to the parameters; off (the default), forward() is the inference encode, without a graph.
    hip_training = False
    P_DROP = 0.1  # TM's dropout at its three sites, in train() mode only

    def _params_version(self):  # (not `_version`: nn.Module stores its state-dict format version under that name, and
        # state_dict() would carry the bound method, and with it the whole module, into every checkpoint)
        return tuple((p.data_ptr(), p._version) for p in self.state_dict().values())

    def invalidate_engine(self):
        """For an optimizer that writes the parameters through raw pointers (optim.FusedAdamW): no `_version` moves, so the
        inference engine's packed copy is declared stale here.  The training engine reads the live parameters and needs nothing."""
        self._packed = None

    def train_engine(self):
        """The training engine (egoego_s1_train_*), on the device of the parameters."""
        from .stage1_train import Stage1TrainEngine
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.EgoEgoHipError("hip_training needs the module's parameters on a cuda (ROCm) device (module.to(device)); "
                                      "there is no CPU path")
        if self._train_engine is None or self._train_engine.device != torch.device("cuda", dev.index if dev.index is not None
                                                                                  else torch.cuda.current_device()):
            self._train_engine = Stage1TrainEngine(self.cfg, dev)
        return self._train_engine

    def _graph(self):
        return bool(self.hip_training) and torch.is_grad_enabled()

    def _exec_engine(self):
        """The engine forward() runs on: the training engine while a graph is being built (it reads the live parameters, so an
        optimizer step costs no re-pack), else the inference engine."""
        return self.train_engine() if self._graph() else self.engine()

    def _encode(self, feats, valid):
        """The heads of W windows: the inference encode, or with hip_training and grad mode on the training encode (connected to
        the parameters; dropout P_DROP with one host-drawn seed per call in train() mode, none in eval())."""
        if not self._graph():
            return self.engine().encode(feats, valid)
        from .stage1_train import training_encode
        p_drop = self.P_DROP if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p_drop > 0 else 0
        return training_encode(self, self.train_engine(), feats, valid, p_drop, seed)

    def engine(self):
        if self._engine is None:
            self._engine = Stage1Engine(self.cfg, self.device)
        v = self._params_version()
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

    def _integrate(self, heads, T, q0, slam, W0, dist_scale, lens=None):
        """heads [W, window, 4] cuda; T / W0 per sequence; q0 [B, 4]; slam [B, L, 3] (lens: its valid frames per sequence, None =
        all L) -> quats [B, max T + 1, 4], trans, scale (fp64); rows past a sequence's end stay zero."""
        dev = heads.device
        B = q0.shape[0]
        L = slam.shape[1]
        Qmax = int(max(T)) + 1
        quat = torch.zeros(B, Qmax, 4, dtype=torch.float64, device=dev)
        trans = torch.zeros(B, L, 3, dtype=torch.float64, device=dev)
        scale = torch.zeros(B, dtype=torch.float64, device=dev)
        Tt = torch.tensor(T, dtype=torch.int32, device=dev)
        w0 = torch.tensor(W0, dtype=torch.int32, device=dev)
        ln = torch.full((B,), L, dtype=torch.int32, device=dev) if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        q0d = q0.to(dev, torch.float64).contiguous()
        sl = slam.to(dev, torch.float64).contiguous()
        eng = self._exec_engine()
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_integrate(heads.data_ptr(), self.cfg.window, Tt.data_ptr(), w0.data_ptr(), q0d.data_ptr(),
                                                      sl.data_ptr(), ln.data_ptr(), B, L, Qmax, float(dist_scale), quat.data_ptr(),
                                                      trans.data_ptr(), scale.data_ptr(), eng._stream()))
        return quat, trans, scale

    def forward(self, data):
        """HE:123-170 on one window per sequence (T <= window tokens, data['seq_len'] valid).  With hip_training set and grad mode
        on, head_va and head_dist_scalar are connected to the parameters (the training encode); head_rot_quat is what it is
        without the flag, integrated on the device and detached: the orientation term's gradient lives in compute_loss."""
        eng = self._exec_engine()
        x = torch.as_tensor(data["of"]).to(eng.device).float()
        B, T, _ = x.shape
        if T > self.cfg.window:
            raise ValueError(f"forward() takes at most window = {self.cfg.window} frames, got {T} (use forward_for_eval)")
        feats = torch.zeros(B, self.cfg.window, self.cfg.d_feats, device=eng.device)
        feats[:, :T] = x
        valid = torch.as_tensor(data["seq_len"]).reshape(B).to(eng.device).to(torch.int32).clamp(0, T)
        heads = self._encode(feats, valid)
        q0 = torch.as_tensor(data["head_pose"])[:, 0, 3:]
        slam = torch.zeros(B, 1, 3, dtype=torch.float64, device=eng.device)
        quat, _, _ = self._integrate(heads.detach(), [T] * B, q0, slam, list(range(B)), 1.0)
        out = defaultdict(list)
        out["head_va"] = heads[:, :T, :3]
        out["head_rot_quat"] = quat.to(torch.as_tensor(data["head_pose"]).dtype)
        out["head_dist_scalar"] = heads[:, :T, 3:4]
        return out

    def compute_loss(self, feature_pred, data):
        """HE:310-345: -> (loss, orient_loss, va_loss, dist_loss) from feature_pred['head_va'] [B, T, 3] and
        feature_pred['head_dist_scalar'] [B, T, 1] against data['head_pose'] [B, T + 1, 7] and data['head_vels'] [B, T, 6], with
        opt.w_rotation, w_va, w_dist and dist_scale; every mean is over all B * T frames, padded ones included.  One call of
        egoego_s1_headnet_loss (fp64 on the device).

        The rotations are recomputed from head_va inside the kernel, and feature_pred['head_rot_quat'] is NOT read: va2rot
        detaches the running rotation, so frame t's orientation term depends on head_va[:, t] alone, and the kernel returns that
        gradient with the loss.  (The values agree with head_rot_quat: both integrate the same head_va from head_pose[:, 0].)
        `loss` carries the gradient to head_va and head_dist_scalar; the three parts are reported values.  Works under no_grad
        and with hip_training off (validation).  CPU tensors raise: there is no CPU path."""
        from .stage1_train import HipHeadNetLoss
        va, dist = feature_pred["head_va"], feature_pred["head_dist_scalar"]
        if not isinstance(va, torch.Tensor) or va.device.type != "cuda" or dist.device != va.device:
            raise _lib.EgoEgoHipError("compute_loss needs the predictions on a cuda (ROCm) device; there is no CPU path")
        pose = torch.as_tensor(data["head_pose"]).to(va.device).float()
        vels = torch.as_tensor(data["head_vels"]).to(va.device).float()
        opt = self.opt
        return HipHeadNetLoss.apply(va, dist, pose, vels, float(opt.dist_scale), float(opt.w_rotation), float(opt.w_va), float(opt.w_dist))

    def forward_for_eval(self, data, lengths=None, pose_lengths=None):
        """HE:214-308 for B sequences of equal length T at once: every block of every sequence in one encode call.
        Extra keys: head_va [B, T, 3], head_dist_scalar [B, T, 1] (before / dist_scale), head_rot_quat [B, T + 1, 4].

        With `lengths` (host integers or a CPU tensor [B]) the sequences differ in length: data['of'] is [B, Tmax, 512] with
        lengths[b] feature frames, the pose-like entries (head_pose, aligned_slam_trans) are [B, Lmax, ...] with pose_lengths[b]
        frames (default lengths + 1).  Sequence b contributes len(block_spans(T_b, window)) blocks to the one encode call.  Every
        output is zero past its sequence's end; pred_scale is always [B]; out['lengths'] (CPU) = min(L_b, T_b + 1), the valid
        frames of head_pose.  What the padded frames of the inputs hold is never read."""
        if lengths is not None:
            return self._forward_for_eval_ragged(data, lengths, pose_lengths)
        if pose_lengths is not None:
            raise ValueError("pose_lengths needs lengths")
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

    def _forward_for_eval_ragged(self, data, lengths, pose_lengths):
        x = torch.as_tensor(data["of"])
        slam = torch.as_tensor(data["aligned_slam_trans"])
        hp = torch.as_tensor(data["head_pose"])
        if x.dim() != 3 or slam.dim() != 3 or hp.dim() != 3 or not x.shape[0] == slam.shape[0] == hp.shape[0]:
            raise ValueError(f"of {tuple(x.shape)}, aligned_slam_trans {tuple(slam.shape)}, head_pose {tuple(hp.shape)}: "
                             "[B, Tmax, F], [B, Lmax, 3], [B, >= 1, 7] expected")
        B, Tmax, F = x.shape
        T = _host_lengths(lengths, B, Tmax, "lengths")
        L = _host_lengths(pose_lengths if pose_lengths is not None else [t + 1 for t in T], B, slam.shape[1], "pose_lengths")
        eng = self.engine()
        dev, win = eng.device, self.cfg.window
        # the pack, from the host-side lengths: block w of the call is rows src[w] of the flattened features (a row past the
        # block's valid count repeats the sequence's first row: encode reads it as zero), token (b, t) is row back[b, t] of heads
        src, valid, win0 = [], [], []
        back = np.zeros((B, Tmax), np.int64)
        for b, Tb in enumerate(T):
            win0.append(len(valid))
            back[b, :Tb] = win0[b] * win + np.arange(Tb)
            for st, n in block_spans(Tb, win):
                r = np.full(win, b * Tmax, np.int64)
                r[:n] = b * Tmax + st + np.arange(n)
                src.append(r)
                valid.append(n)
        src = _upload(np.stack(src).reshape(-1), torch.int64, dev)
        feats = x.to(dev).float().reshape(B * Tmax, F).index_select(0, src).reshape(len(valid), win, F)
        heads = eng.encode(feats, _upload(valid, torch.int32, dev))
        quat, trans, scale = self._integrate(heads, T, hp[:, 0, 3:], slam, win0, self.opt.dist_scale, lens=L)
        n = [min(l, t + 1) for l, t in zip(L, T)]
        N = max(n)
        out = defaultdict(list)
        out["head_pose"] = _keep_rows(torch.cat((trans[:, :N], quat[:, :N]), -1), _upload(n, torch.int64, dev))
        out["pred_scale"] = scale
        hv = _keep_rows(heads.reshape(-1, 4).index_select(0, _upload(back.reshape(-1), torch.int64, dev)).reshape(B, Tmax, 4),
                        _upload(T, torch.int64, dev))
        out["head_va"] = hv[..., :3]
        out["head_dist_scalar"] = hv[..., 3:4]
        out["head_rot_quat"] = quat
        out["lengths"] = torch.tensor(n, dtype=torch.int64)
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
        eng = self._exec_engine()
        rot = torch.as_tensor(data["head_rot_mat"]).to(eng.device).float()
        trans = torch.as_tensor(data["head_trans"]).to(eng.device).float()
        B, L = rot.shape[:2]
        return rot.reshape(B, L, 9).contiguous(), trans.contiguous(), torch.full((B,), L, dtype=torch.int32, device=eng.device)

    def forward(self, data):
        """HN:118-155: the floor normal of every sequence from its first window + 1 frames.  With hip_training set and grad mode
        on, pred_normal is connected to the parameters (the training encode).  data['lengths'] (int32 [B] on the device; the
        batches of stage1_data carry it, no reference-format dict does): the frames of each padded sequence, so that the keys are
        masked by seq_len - 1 as in HN:148; without the key every sequence counts with all its rows."""
        eng = self._exec_engine()
        rot, trans, ln = self._frames(data)
        B, L = rot.shape[:2]
        if "lengths" in data:
            ln = data["lengths"]
            if not isinstance(ln, torch.Tensor) or ln.device != eng.device or ln.dtype != torch.int32 or tuple(ln.shape) != (B,):
                raise ValueError(f"lengths: an int32 [{B}] tensor on {eng.device} expected")
            ln = ln.clamp(max=L).contiguous()  # (the feature kernel reads rows below a sequence's length: never past the L it was given)
        win = self.cfg.window
        feats = torch.empty(B, win, 18, device=eng.device)
        valid = torch.empty(B, dtype=torch.int32, device=eng.device)
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_gravity_features(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, L, win,
                                                             feats.data_ptr(), valid.data_ptr(), eng._stream()))
        out = defaultdict(list)
        out["pred_normal"] = self._encode(feats, valid)
        return out

    def compute_loss(self, feature_pred, data):
        """HN:33-35, 334-342: -> (loss, normal_loss), |gt - pred| of the predicted floor normal against data['floor_normal']
        ([B, 3] or [B, 3, 1]) summed over its 3 components, mean over B.  Three torch ops on the device (the training encode's
        backward takes their gradient); works under no_grad and with hip_training off.  A CPU prediction raises."""
        pred = feature_pred["pred_normal"]
        if not isinstance(pred, torch.Tensor) or pred.device.type != "cuda":
            raise _lib.EgoEgoHipError("compute_loss needs the prediction on a cuda (ROCm) device; there is no CPU path")
        gt = torch.as_tensor(data["floor_normal"]).to(pred.device).squeeze(-1)
        normal_loss = (gt - pred).abs().sum(dim=1).mean()
        return normal_loss, normal_loss

    def _apply_pose(self, rot, trans, ln, Rn, scale, Ral, origin):  # (not `_apply`: nn.Module moves its parameters through that name)
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

    def forward_for_eval(self, data, pred_scale=None, use_gt_aligned_rot=False, lengths=None, ref_lengths=None):
        """HN:214-294 for B sequences.  Extra keys: pred_normal [B, 3], normal_rot [B, 3, 3] (normal -> +z), align_rot [B, 3, 3]
        (the Umeyama r).

        With `lengths` (host integers or a CPU tensor [B]: the SLAM frames of each sequence in the padded head_trans /
        head_rot_mat) the sequences differ in length, ref_lengths (default: lengths) counts the frames of ori_head_pose, and the
        whole call stays on the device: features, encode, egoego_s1_gravity_align (the Rodrigues rotation and the planar Umeyama
        alignment over min(length, ref_length) frames) and one egoego_s1_gravity_apply.  normal_rot and align_rot are then device
        tensors, every per-frame output is zero past its sequence's end, out['lengths'] repeats the lengths."""
        if lengths is not None:
            return self._forward_for_eval_ragged(data, pred_scale, use_gt_aligned_rot, lengths, ref_lengths)
        if ref_lengths is not None:
            raise ValueError("ref_lengths needs lengths")
        with torch.no_grad():  # evaluation never builds a graph, whatever hip_training says
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
        est = self._apply_pose(rot, trans, ln, Rn, scale, eye, trans[:, 0].double().cpu().numpy()).cpu().numpy()
        ref = torch.as_tensor(data["ori_head_pose"]).double().cpu().numpy()
        Ral = np.empty((B, 3, 3))
        for b in range(B):
            e, r = est[b, :min(L, ref.shape[1]), :3].copy(), ref[b, :, :3].copy()
            e[:, 2] = 1
            r[:, 2] = 1
            Ral[b] = umeyama_rotation(e, r).astype(np.float32)
        gt = torch.as_tensor(data["ori_head_pose"])
        pose = self._apply_pose(rot, trans, ln, Rn, scale, Ral, gt[:, 0, :3].double().cpu().numpy())
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

    def _forward_for_eval_ragged(self, data, pred_scale, use_gt_aligned_rot, lengths, ref_lengths):
        if use_gt_aligned_rot:
            raise NotImplementedError("use_gt_aligned_rot with lengths=: egoego_s1_gravity_align derives the rotation from the "
                                      "predicted normal; run the equal-length call per sequence for the debugging path")
        rot_in, trans_in, gt = (torch.as_tensor(data[k]) for k in ("head_rot_mat", "head_trans", "ori_head_pose"))
        if rot_in.dim() != 4 or trans_in.dim() != 3 or gt.dim() != 3 or not rot_in.shape[:2] == trans_in.shape[:2] or gt.shape[0] != rot_in.shape[0]:
            raise ValueError(f"head_rot_mat {tuple(rot_in.shape)}, head_trans {tuple(trans_in.shape)}, ori_head_pose "
                             f"{tuple(gt.shape)}: [B, Lmax, 3, 3], [B, Lmax, 3], [B, Rmax, 7] expected")
        B, Lmax = rot_in.shape[:2]
        Rmax = gt.shape[1]
        L = _host_lengths(lengths, B, Lmax, "lengths")
        R = _host_lengths(ref_lengths if ref_lengths is not None else L, B, Rmax, "ref_lengths")
        eng = self.engine()
        dev, win = eng.device, self.cfg.window
        ln, rl = _upload(L, torch.int32, dev), _upload(R, torch.int32, dev)
        rot = rot_in.to(dev).float().reshape(B, Lmax, 9).contiguous()
        trans = trans_in.to(dev).float().contiguous()
        ref = gt.to(dev).double().contiguous()
        src = pred_scale if pred_scale is not None else data["aligned_scale"]
        scale = torch.as_tensor(src).to(dev).double().reshape(-1).expand(B).contiguous()
        feats = torch.empty(B, win, 18, device=dev)
        valid = torch.empty(B, dtype=torch.int32, device=dev)
        Rn = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
        Ral = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
        pose = torch.zeros(B, Lmax, 7, dtype=torch.float64, device=dev)
        origin = ref[:, 0, :3].contiguous()
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_gravity_features(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, Lmax, win,
                                                             feats.data_ptr(), valid.data_ptr(), eng._stream()))
        normal = eng.encode(feats, valid)
        with torch.cuda.device(eng.dev_index):
            _lib.check_s1(eng.lib.egoego_s1_gravity_align(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, Lmax, normal.data_ptr(),
                                                          scale.data_ptr(), ref.data_ptr(), rl.data_ptr(), Rmax, Rn.data_ptr(),
                                                          Ral.data_ptr(), eng._stream()))
            _lib.check_s1(eng.lib.egoego_s1_gravity_apply(rot.data_ptr(), trans.data_ptr(), ln.data_ptr(), B, Lmax, Rn.data_ptr(),
                                                          scale.data_ptr(), Ral.data_ptr(), origin.data_ptr(), pose.data_ptr(),
                                                          eng._stream()))
        n_l, n_r = ln.long(), rl.long()
        out = defaultdict(list)
        out["head_trans"] = pose[..., :3]
        out["head_rot_mat"] = _keep_rows(rotations.quaternion_to_matrix(pose[..., 3:]), n_l)
        out["head_pose"] = pose
        out["gt_head_trans"] = _keep_rows(ref[..., :3], n_r)
        out["gt_head_rot_mat"] = _keep_rows(rotations.quaternion_to_matrix(ref[..., 3:]), n_r)
        out["gt_head_pose"] = _keep_rows(torch.cat((ref[..., :3], rotations.matrix_to_quaternion(out["gt_head_rot_mat"])), -1), n_r)
        out["pred_normal"] = normal
        out["normal_rot"] = Rn
        out["align_rot"] = Ral
        out["lengths"] = torch.tensor(L, dtype=torch.int64)
        out["ref_lengths"] = torch.tensor(R, dtype=torch.int64)
        return out


def stage1_ragged(headnet, gravitynet, batch, lengths, pose_lengths=None):
    """Both estimators on B sequences of different lengths (forward_for_eval(..., lengths=) of each, GravityNet on HeadNet's
    pred_scale) -> (GravityNet's translation with HeadNet's rotation [B, Nmax, 7] float64, unmasked past each end; HeadNet's
    output; GravityNet's output; the valid frames n_b = min(L_b, T_b + 1) as a host list)."""
    out = headnet.forward_for_eval(batch, lengths=lengths, pose_lengths=pose_lengths)
    L = pose_lengths if pose_lengths is not None else [int(t) + 1 for t in torch.as_tensor(lengths).reshape(-1).tolist()]
    ori = torch.as_tensor(batch["ori_slam_trans"])
    normal_in = {"head_trans": ori - ori[:, 0:1, :], "head_rot_mat": torch.as_tensor(batch["ori_slam_rot_mat"]),
                 "ori_head_pose": torch.as_tensor(batch["head_pose"])}
    nout = gravitynet.forward_for_eval(normal_in, out["pred_scale"], lengths=L, ref_lengths=L)
    n = out["lengths"].tolist()
    N = max(n)
    hp = torch.cat((nout["head_pose"][:, :N, :3], out["head_pose"][:, :N, 3:].to(nout["head_pose"].device)), -1).double()
    return hp, out, nout, n


def estimate_head_pose(headnet, gravitynet, batch, z_offset=-0.13, lengths=None, pose_lengths=None):
    """RE:104-136: HeadNet's rotations with GravityNet's translation, moved onto the ground-truth start and shifted by z_offset
    (the reference's -0.13, "only for this sequence") -> [B, T, 7] float64 (xyz, quaternion w,x,y,z), what stage 2 takes.
    Also returns the two estimators' outputs.

    With `lengths` (feature frames per sequence; pose_lengths defaults to lengths + 1) the batch is padded and the sequences
    differ in length: -> (poses [B, max n_b, 7], zero past n_b; the two outputs; the lengths n_b = min(L_b, T_b + 1), a CPU
    tensor), what full_body_gen_cond_head_pose_sliding_window_ragged takes as head_poses and lengths."""
    if lengths is not None:
        hp, out, nout, n = stage1_ragged(headnet, gravitynet, batch, lengths, pose_lengths)
        hp[:, :, :2] -= hp[:, 0:1, :2].clone()
        gt0 = torch.as_tensor(batch["head_pose"])[:, 0:1, :3].to(hp.device).double()
        hp[:, :, :3] += gt0 - hp[:, 0:1, :3]
        hp[:, :, 2] += z_offset
        return _keep_rows(hp, _upload(n, torch.int64, hp.device)), out, nout, out["lengths"]
    if pose_lengths is not None:
        raise ValueError("pose_lengths needs lengths")
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


# ------------------------------------------------------------------------------------------ the stage-1 score
def head_pose_metrics(pred_pose, gt_pose, lengths=None):
    """egoego/eval/head_pose_metrics.py compute_head_pose_metrics on poses [B, T, 7] (xyz + quaternion w,x,y,z) on the device ->
    float64 [B, 3] = (head_dist, head_dist_rot_only, head_trans_err in mm) over the first lengths[b] frames (None: all T)."""
    p, g = torch.as_tensor(pred_pose), torch.as_tensor(gt_pose)
    if p.dim() != 3 or p.shape[-1] != 7 or g.shape != p.shape or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"poses {tuple(p.shape)} / {tuple(g.shape)}: two [B, T, 7] tensors expected")
    if p.device.type != "cuda" or g.device != p.device:
        raise _lib.EgoEgoHipError("the head-pose metrics need tensors on one cuda (ROCm) device; there is no CPU path")
    dev = p.device
    B, T = p.shape[:2]
    if lengths is None:
        ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    elif isinstance(lengths, torch.Tensor) and lengths.device.type == "cuda":
        ln = lengths.to(dev, torch.int32).reshape(-1).contiguous()  # taken as given: the kernel clamps it to 0..T
        if ln.shape != (B,):
            raise ValueError(f"lengths {tuple(lengths.shape)}: [{B}] expected")
    else:
        ln = _upload(_host_lengths(lengths, B, T, "lengths"), torch.int32, dev)
    p, g = p.double().contiguous(), g.double().contiguous()
    out = torch.empty(B, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check_s1(_lib.load().egoego_s1_head_pose_metrics(p.data_ptr(), g.data_ptr(), ln.data_ptr(), B, T, out.data_ptr(), stream))
    return out


def compute_head_pose_metrics(head_trans, head_rot, gt_head_trans, gt_head_rot, lengths=None):
    """The reference's compute_head_pose_metrics (same argument order) on the device: translations [T, 3] or [B, T, 3], rotation
    matrices [T, 3, 3] or [B, T, 3, 3] (converted to quaternions on the device in float64) -> (head_dist, head_dist_rot_only,
    head_trans_err in mm), three float64 [B] tensors.  lengths [B]: the valid frames of each sequence (None: all T)."""
    ts = [torch.as_tensor(t) for t in (head_trans, head_rot, gt_head_trans, gt_head_rot)]
    if ts[0].dim() == 2:
        ts = [t[None] for t in ts]
    pt, pr, gt, gr = ts
    if pt.dim() != 3 or pt.shape[-1] != 3 or pr.shape != pt.shape[:2] + (3, 3) or gt.shape != pt.shape or gr.shape != pr.shape:
        raise ValueError(f"head_trans {tuple(pt.shape)}, head_rot {tuple(pr.shape)}, gt_head_trans {tuple(gt.shape)}, gt_head_rot "
                         f"{tuple(gr.shape)}: [B, T, 3] and [B, T, 3, 3] (or without B) expected")
    if any(t.device.type != "cuda" for t in ts):
        raise _lib.EgoEgoHipError("the head-pose metrics need tensors on a cuda (ROCm) device; there is no CPU path")
    pose = lambda t, r: torch.cat((t.double(), rotations.matrix_to_quaternion(r.double())), -1)  # noqa: E731
    m = head_pose_metrics(pose(pt, pr), pose(gt, gr), lengths)
    return m[:, 0], m[:, 1], m[:, 2]


# ------------------------------------------------------------------------------------------ the ARES demo sequence (AD)
def _quat_to_mat32(q):
    return rotations.quaternion_to_matrix(torch.as_tensor(np.asarray(q, np.float32)).float()).numpy()


def load_slam(npy_path):
    """AD load_data_from_droidslam: [T, 7] (xyz, quaternion w,x,y,z), a .npy path or the array itself -> trans [T, 3], rot
    [T, 3, 3] fp32, quat [T, 4]."""
    d = np.load(npy_path) if isinstance(npy_path, (str, os.PathLike)) else np.asarray(npy_path)
    return d[:, :3], _quat_to_mat32(d[:, 3:]), d[:, 3:].astype(np.float32)


def load_slam_res_and_align_first(npy_path, gt_head_pose):
    """AD load_slam_res_and_align_first: rotate the SLAM trajectory (a .npy path or the [T, 7] array) so that its first rotation
    is the ground truth's, and move its first position onto the ground truth's -> aligned trans [T, 3], rot [T, 3, 3], quat [T, 4]."""
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
