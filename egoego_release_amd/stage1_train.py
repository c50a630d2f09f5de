"""Stage-1 training on the HIP library (csrc/stage1_train.*): the training encode of HeadNet / GravityNet with the gradient of every
trainable tensor, and HeadNet's loss with its gradient with respect to the heads.

    Stage1TrainEngine  one egoego_s1_train_ctx on one GPU: forward (heads + saves), backward (gradients from any upstream), the
                       dropout masks and the saved tensors of a call
    HipStage1Encode    the torch.autograd.Function in front of it: parameters -> heads
    headnet_loss       egoego_s1_headnet_loss: heads -> (total, orient, va, dist) in fp64 and d(total) / d(heads)
    HipHeadNetLoss     the torch.autograd.Function in front of that: heads -> loss parts

The engine holds no copy of the weights: every call hands over pointers to the module's live parameter tensors, so the heads after
an optimizer step are the heads of the new weights.  There is no PyTorch fallback: a missing library or a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from ._engine import ContextEngine
from .train import _LAYER_FIELDS, SITES

TR = "action_transformer."
MAX_WINDOW = 128


def head_linears(cfg):
    """The heads' nn.Linear modules in the order of egoego_s1_weights.head_w -> [(name, out, in)]."""
    out = []
    for pre, dims in cfg.head_dims().items():
        names = [f"{pre}_mlp.affine_layers.{k}" for k in range(len(dims) - 1)] + [f"{pre}_fc"]
        out += [(nm, o, i) for nm, (o, i) in zip(names, dims)]
    return out


def param_names(cfg):
    """A stage-1 module's tensors in the order the library's structs list them."""
    names = [TR + "start_conv.weight", TR + "start_conv.bias", TR + "position_vec.weight"]
    for i in range(cfg.n_dec_layers):
        names += [TR + f"layer_stack.{i}.{n}" for _, n in _LAYER_FIELDS]
    for nm, _, _ in head_linears(cfg):
        names += [nm + ".weight", nm + ".bias"]
    return names


class Stage1TrainEngine(ContextEngine):
    """One stage-1 training context of libegoego_hip on one GPU.  `tensors` arguments are dicts name -> fp32 contiguous tensor on
    the engine's device, keyed like param_names()."""

    NOUN = "stage-1 training"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_s1_train_ctx_create", "egoego_s1_train_ctx_destroy", "egoego_s1_train_workspace_bytes"
    CHECK = _lib.check_s1_train

    def __init__(self, cfg, device):
        """cfg: a synthetic.Stage1Config."""
        super().__init__(device)
        self.cfg = cfg
        kind = _lib.S1_HEADNET if cfg.kind == "headnet" else _lib.S1_GRAVITYNET
        c = _lib.S1Config(kind, cfg.d_feats, cfg.d_model, cfg.n_head, cfg.n_dec_layers, cfg.d_k, cfg.d_v, cfg.window)
        self._create(C.byref(c), self.dev_index)
        self.names = param_names(cfg)
        self.linears = head_linears(cfg)

    # ------------------------------------------------------------------ plumbing
    def _struct(self, tensors, frozen_ok=False):
        """-> (_lib.S1Weights over the tensors' pointers, what must stay alive until the call has been issued)."""
        def ptr(name):
            t = tensors.get(name)
            if t is None:
                if frozen_ok and name.endswith("position_vec.weight"):
                    return None
                raise _lib.EgoEgoHipError(f"stage-1 training needs tensor {name}")
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.EgoEgoHipError(f"{name}: stage-1 training reads live fp32 contiguous tensors on {self.device} "
                                          f"(got {t.dtype} on {t.device}, contiguous={t.is_contiguous()}); move the module there")
            return t.data_ptr()

        n_layers = self.cfg.n_dec_layers
        layers = (_lib.LayerWeights * n_layers)()
        for i in range(n_layers):
            for field, n in _LAYER_FIELDS:
                setattr(layers[i], field, ptr(TR + f"layer_stack.{i}.{n}"))
        w = _lib.S1Weights()
        w.start_conv_w, w.start_conv_b = ptr(TR + "start_conv.weight"), ptr(TR + "start_conv.bias")
        w.position_vec = ptr(TR + "position_vec.weight")
        w.layers = layers
        for j, (nm, _, _) in enumerate(self.linears):
            w.head_w[j], w.head_b[j] = ptr(nm + ".weight"), ptr(nm + ".bias")
        return w, (layers, tensors)

    def saves_bytes(self, W):
        n = self.lib.egoego_s1_train_saves_bytes(self._ctx, W)
        if n == 0:
            raise _lib.EgoEgoHipError(_lib.check_s1_train.last_error())
        return n

    @staticmethod
    def _aligned(buf):
        off = (-buf.data_ptr()) % 256
        return buf.data_ptr() + off, buf.numel() - off

    def new_saves(self, W):
        """The buffer one forward call fills and its backward call reads (owned by whoever holds the graph)."""
        return torch.empty(self.saves_bytes(W) + 256, dtype=torch.uint8, device=self.device)

    def out_shape(self, W):
        return (W, self.cfg.window, 4) if self.cfg.kind == "headnet" else (W, 3)

    # ------------------------------------------------------------------ the two passes
    def forward(self, tensors, feats, valid, p_drop=0.0, seed=0, window_ids=None, saves=None):
        """feats [W, window, d_feats], valid int [W] -> (heads [W, window, 4] | [W, 3], saves)."""
        cfg = self.cfg
        W = feats.shape[0]
        if tuple(feats.shape) != (W, cfg.window, cfg.d_feats):
            raise ValueError(f"features {tuple(feats.shape)} != [W, {cfg.window}, {cfg.d_feats}]")
        feats = feats.to(self.device, torch.float32).contiguous()
        valid = valid.to(self.device, torch.int32).contiguous()
        if tuple(valid.shape) != (W,):
            raise ValueError(f"valid {tuple(valid.shape)} != ({W},)")
        wid = None if window_ids is None else torch.as_tensor(window_ids).to(self.device, torch.int64).contiguous()
        if saves is None:
            saves = self.new_saves(W)
        sp, sn = self._aligned(saves)
        heads = torch.empty(self.out_shape(W), dtype=torch.float32, device=self.device)
        w, keep = self._struct(tensors)
        ws, wn = self._workspace(W)
        with torch.cuda.device(self.dev_index):
            _lib.check_s1_train(self.lib.egoego_s1_train_forward(
                self._ctx, C.byref(w), feats.data_ptr(), valid.data_ptr(), float(p_drop), int(seed),
                None if wid is None else wid.data_ptr(), W, sp, sn, ws, wn, heads.data_ptr(), self._stream()))
        del keep
        return heads, saves

    def backward(self, tensors, saves, d_heads, W, p_drop=0.0, seed=0, grads=None):
        """-> dict name -> gradient (fresh tensors shaped like the parameters, or `grads` overwritten) for the upstream d_heads."""
        up = d_heads.to(self.device, torch.float32).contiguous()
        if tuple(up.shape) != self.out_shape(W):
            raise ValueError(f"upstream gradient {tuple(up.shape)} != {self.out_shape(W)}")
        if grads is None:
            grads = {n: torch.empty_like(tensors[n]) for n in self.names if not n.endswith("position_vec.weight")}
        w, keep = self._struct(tensors)
        g, gkeep = self._struct(grads, frozen_ok=True)
        sp, sn = self._aligned(saves)
        ws, wn = self._workspace(W)
        with torch.cuda.device(self.dev_index):
            _lib.check_s1_train(self.lib.egoego_s1_train_backward(self._ctx, C.byref(w), sp, sn, up.data_ptr(), C.byref(g), float(p_drop),
                                                                  int(seed), W, ws, wn, self._stream()))
        del keep, gkeep
        return grads

    # ------------------------------------------------------------------ test / debug surface
    def dropout_mask(self, p_drop, seed, layer, site, W, window_ids=None):
        """The mask (bool) a forward with these arguments applies: site "attn" [W, 4, window, window], "fc" / "ffn" [W, window, 256]."""
        L = self.cfg.window
        shape = (W, 4, L, L) if site == "attn" else (W, L, 256)
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        wid = None if window_ids is None else torch.as_tensor(window_ids).to(self.device, torch.int64).contiguous()
        ws, wn = self._workspace(W)
        with torch.cuda.device(self.dev_index):
            _lib.check_s1_train(self.lib.egoego_s1_train_dropout_mask(self._ctx, float(p_drop), int(seed), layer, SITES[site],
                                                                      None if wid is None else wid.data_ptr(), W, out.data_ptr(), ws, wn,
                                                                      self._stream()))
        return out.bool()

    def saved(self, saves, W, layer, which):
        """One saved tensor of the forward call that filled `saves` (names: _lib.S1_TRAIN_SAVED).  "head_hidden": `layer` is the
        index of the head Linear (the order of head_linears()) whose ReLU output is wanted."""
        L = self.cfg.window
        if which == "head_hidden":
            rows = (W, L) if self.cfg.kind == "headnet" else (W,)
            shape = rows + (self.linears[layer][1],)
        else:
            shape = {"attn_prob": (W, 4, L, L), "attn_out": (W, L, 1024)}.get(which, (W, L, 256))
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        sp, sn = self._aligned(saves)
        with torch.cuda.device(self.dev_index):
            _lib.check_s1_train(self.lib.egoego_s1_train_saved(self._ctx, sp, sn, W, layer, _lib.S1_TRAIN_SAVED[which], out.data_ptr(),
                                                               self._stream()))
        return out


class HipStage1Encode(torch.autograd.Function):
    """heads = HipStage1Encode.apply(engine, names, meta, *params): the forward pass keeps its saves on the autograd context (two
    graphs may be outstanding at once); the backward pass takes any upstream gradient of the heads and returns one gradient per
    parameter in its own shape (conv weights (out, in, 1)), None for a parameter that does not require one."""

    @staticmethod
    def forward(ctx, engine, names, meta, *params):
        tensors = {n: p.detach() for n, p in zip(names, params)}
        heads, saves = engine.forward(tensors, **meta)
        ctx.engine, ctx.names, ctx.saves = engine, names, saves
        ctx.call = (int(meta["feats"].shape[0]), float(meta.get("p_drop", 0.0)), int(meta.get("seed", 0)))
        ctx.save_for_backward(*params)
        return heads

    @staticmethod
    def backward(ctx, d_heads):
        params = ctx.saved_tensors
        tensors = {n: p.detach() for n, p in zip(ctx.names, params)}
        W, p_drop, seed = ctx.call
        grads = ctx.engine.backward(tensors, ctx.saves, d_heads, W, p_drop, seed)
        out = tuple(grads.get(n) if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[3:]))
        return (None, None, None) + out


def training_encode(module, engine, feats, valid, p_drop, seed, window_ids=None):
    """The heads of a stage-1 `module` on the training engine, connected to its parameters."""
    named = dict(module.named_parameters())
    params = [named[n] for n in engine.names]
    meta = dict(feats=feats, valid=valid, p_drop=p_drop, seed=seed, window_ids=window_ids)
    return HipStage1Encode.apply(engine, engine.names, meta, *params)


# ---------------------------------------------------------------------------------------------- HeadNet's loss
def headnet_loss(heads, T, head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist, want_fp64_grad=False):
    """egoego_s1_headnet_loss: heads [B, window, 4] fp32 cuda (the first T rows of each sequence count), head_pose [B, T + 1, 7],
    head_vels [B, T, 6] -> (loss fp64 [4] = total, orient, va, dist; d(total) / d(heads) fp32 [B, window, 4], rows t >= T zero;
    the same in fp64 when want_fp64_grad, else None)."""
    if heads.device.type != "cuda":
        raise _lib.EgoEgoHipError("HeadNet's loss needs tensors on a cuda (ROCm) device; there is no CPU path")
    lib = _lib.load()
    dev = heads.device
    if heads.dim() != 3 or heads.shape[-1] != 4:
        raise ValueError(f"heads {tuple(heads.shape)}: [B, window, 4] expected")
    B, window, _ = heads.shape
    T = int(T)
    if not 1 <= T <= window <= MAX_WINDOW:
        raise ValueError(f"T = {T}, window = {window}: 1 <= T <= window <= {MAX_WINDOW} expected")
    heads = heads.to(torch.float32).contiguous()
    pose = torch.as_tensor(head_pose).to(dev, torch.float32).contiguous()
    vels = torch.as_tensor(head_vels).to(dev, torch.float32).contiguous()
    if tuple(pose.shape) != (B, T + 1, 7) or tuple(vels.shape) != (B, T, 6):
        raise ValueError(f"head_pose {tuple(pose.shape)}, head_vels {tuple(vels.shape)}: [{B}, {T + 1}, 7] and [{B}, {T}, 6] expected")
    loss = torch.empty(4, dtype=torch.float64, device=dev)
    d32 = torch.empty(B, window, 4, dtype=torch.float32, device=dev)
    d64 = torch.empty(B, window, 4, dtype=torch.float64, device=dev) if want_fp64_grad else None
    n = lib.egoego_s1_headnet_loss_workspace_bytes(B)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check_s1_train(lib.egoego_s1_headnet_loss(heads.data_ptr(), window, B, T, pose.data_ptr(), vels.data_ptr(), float(dist_scale),
                                                       float(w_rotation), float(w_va), float(w_dist), loss.data_ptr(),
                                                       None if d64 is None else d64.data_ptr(), d32.data_ptr(), ws.data_ptr() + off,
                                                       ws.numel() - off, stream))
    return loss, d32, d64


class HipHeadNetLoss(torch.autograd.Function):
    """(loss, orient, va, dist) = HipHeadNetLoss.apply(head_va [B, T, 3], head_dist_scalar [B, T, 1], head_pose, head_vels,
    dist_scale, w_rotation, w_va, w_dist): fp32 scalars as the reference returns them.  Only `loss` carries a gradient (to head_va
    and head_dist_scalar); the three parts are reported values."""

    @staticmethod
    def forward(ctx, head_va, head_dist, head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist):
        heads = torch.cat((head_va, head_dist), -1)
        loss, d32, _ = headnet_loss(heads, heads.shape[1], head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist)
        ctx.save_for_backward(d32)
        parts = loss.to(torch.float32)
        total, orient, va, dist = parts[0], parts[1], parts[2], parts[3]
        ctx.mark_non_differentiable(orient, va, dist)
        return total, orient, va, dist

    @staticmethod
    def backward(ctx, g, *_):
        (d32,) = ctx.saved_tensors
        d = d32 * g  # (a power of two scales every entry exactly)
        return d[..., :3], d[..., 3:], None, None, None, None, None, None
