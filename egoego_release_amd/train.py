"""The stage-2 training step on the HIP library (csrc/train_step.*): the loss of CondGaussianDiffusion.p_losses and the gradient of
every trainable tensor of the denoiser.

    TrainEngine        one egoego_train_ctx on one GPU: forward (loss + saves), backward (gradients), the dropout masks and the
                       saved tensors of a call
    HipTrainingLoss    the torch.autograd.Function in front of it: `loss.backward(); optimizer.step()` runs unchanged
    training_loss      what CondGaussianDiffusion.p_losses calls when `hip_training` is set

The engine holds no copy of the weights: every call hands over pointers to the module's live parameter tensors, so the loss after
an optimizer step is the loss of the new weights.  There is no PyTorch fallback: a missing library or a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from ._engine import ContextEngine

SITES = {"attn": _lib.TRAIN_SITE_ATTN, "fc": _lib.TRAIN_SITE_FC, "ffn": _lib.TRAIN_SITE_FFN}
_LAYER_FIELDS = (("w_q", "self_attn.w_q.weight"), ("b_q", "self_attn.w_q.bias"), ("w_k", "self_attn.w_k.weight"),
                 ("b_k", "self_attn.w_k.bias"), ("w_v", "self_attn.w_v.weight"), ("b_v", "self_attn.w_v.bias"),
                 ("w_fc", "self_attn.fc.weight"), ("b_fc", "self_attn.fc.bias"), ("ln1_g", "self_attn.layer_norm.weight"),
                 ("ln1_b", "self_attn.layer_norm.bias"), ("w_1", "pos_ffn.w_1.weight"), ("b_1", "pos_ffn.w_1.bias"),
                 ("w_2", "pos_ffn.w_2.weight"), ("b_2", "pos_ffn.w_2.bias"), ("ln2_g", "pos_ffn.layer_norm.weight"),
                 ("ln2_b", "pos_ffn.layer_norm.bias"))
_TOP_FIELDS = (("start_conv_w", "motion_transformer.start_conv.weight"), ("start_conv_b", "motion_transformer.start_conv.bias"),
               ("position_vec", "motion_transformer.position_vec.weight"), ("linear_out_w", "linear_out.weight"),
               ("linear_out_b", "linear_out.bias"), ("time_mlp1_w", "time_mlp.1.weight"), ("time_mlp1_b", "time_mlp.1.bias"),
               ("time_mlp3_w", "time_mlp.3.weight"), ("time_mlp3_b", "time_mlp.3.bias"))


def param_names(n_layers):
    """The denoiser's tensors (names relative to `denoise_fn`) in the order the library's structs list them."""
    names = [n for _, n in _TOP_FIELDS]
    for i in range(n_layers):
        names += [f"motion_transformer.layer_stack.{i}.{n}" for _, n in _LAYER_FIELDS]
    return names


class TrainEngine(ContextEngine):
    """One training-step context of libegoego_hip on one GPU.  `tensors` arguments are dicts name -> fp32 contiguous tensor on the
    engine's device, keyed like param_names()."""

    NOUN = "the training step"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_train_ctx_create", "egoego_train_ctx_destroy", "egoego_train_workspace_bytes"
    CHECK = _lib.check_train

    def __init__(self, cfg, device):
        """cfg: the dict of precision._engine_cfg (d_feats, d_model, n_head, n_dec_layers, d_k, d_v, max_timesteps, num_timesteps)."""
        super().__init__(device)
        self.cfg = dict(cfg)
        c = _lib.Config(cfg["d_feats"], cfg["d_model"], cfg["n_head"], cfg["n_dec_layers"], cfg["d_k"], cfg["d_v"], cfg["max_timesteps"],
                        cfg["num_timesteps"], 0, _lib.PREC_BF16X3, 0)
        self._create(C.byref(c), self.dev_index)
        self.n_layers = int(cfg["n_dec_layers"])
        self.d_feats = int(cfg["d_feats"])
        self.names = param_names(self.n_layers)

    # ------------------------------------------------------------------ plumbing
    def _struct(self, tensors, frozen_ok=False):
        """-> (_lib.Weights over the tensors' pointers, what must stay alive until the call has been issued)."""
        def ptr(name):
            t = tensors.get(name)
            if t is None:
                if frozen_ok and name.endswith("position_vec.weight"):
                    return None
                raise _lib.EgoEgoHipError(f"the training step needs tensor {name}")
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.EgoEgoHipError(f"{name}: the training step reads live fp32 contiguous tensors on {self.device} "
                                          f"(got {t.dtype} on {t.device}, contiguous={t.is_contiguous()})")
            return t.data_ptr()

        layers = (_lib.LayerWeights * self.n_layers)()
        for i in range(self.n_layers):
            for field, n in _LAYER_FIELDS:
                setattr(layers[i], field, ptr(f"motion_transformer.layer_stack.{i}.{n}"))
        w = _lib.Weights()
        for field, n in _TOP_FIELDS:
            setattr(w, field, ptr(n))
        w.layers = layers
        return w, (layers, tensors)

    def saves_bytes(self, B, T):
        n = self.lib.egoego_train_saves_bytes(self._ctx, B, T)
        if n == 0:
            raise _lib.EgoEgoHipError(_lib.check_train.last_error())
        return n

    @staticmethod
    def _aligned(buf):
        off = (-buf.data_ptr()) % 256
        return buf.data_ptr() + off, buf.numel() - off

    def new_saves(self, B, T):
        """The buffer one forward call fills and its backward call reads (owned by whoever holds the graph)."""
        return torch.empty(self.saves_bytes(B, T) + 256, dtype=torch.uint8, device=self.device)

    def _f32(self, t, shape, name):
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} {tuple(t.shape)} != {tuple(shape)}")
        return t.to(self.device, torch.float32).contiguous()

    # ------------------------------------------------------------------ the two passes
    def forward(self, tensors, x_start, noise, cond_noise, cond_mask, t, row_mask, sqrt_ac, sqrt_1mac, p2w, objective="pred_x0",
                loss_type="l1", p_drop=0.0, seed=0, window_ids=None, saves=None, want_out=False):
        """-> (loss: device scalar, model_out [B, T, D] or None, saves).  Draws (noise, cond_noise, t) are the caller's."""
        B, T, D = x_start.shape
        if D != self.d_feats:
            raise ValueError(f"x_start has {D} features, the model {self.d_feats}")
        if objective not in ("pred_noise", "pred_x0"):
            raise ValueError(f"unknown objective {objective}")
        if loss_type not in ("l1", "l2"):
            raise ValueError(f"invalid loss type {loss_type}")
        xs = self._f32(x_start, (B, T, D), "x_start")
        nz = self._f32(noise, (B, T, D), "noise")
        cn = self._f32(cond_noise, (B, T, D), "cond_noise")
        cm = self._f32(cond_mask.expand(B, T, D) if cond_mask.dim() == 3 else cond_mask, (B, T, D), "cond_mask")
        tt = t.to(self.device, torch.int64).contiguous()
        if tuple(tt.shape) != (B,):
            raise ValueError(f"t {tuple(tt.shape)} != ({B},)")
        rm = None if row_mask is None else self._f32(row_mask, (B, T + 1), "row mask")
        wid = None if window_ids is None else torch.as_tensor(window_ids).to(self.device, torch.int64).contiguous()
        tabs = [self._f32(v, v.shape, "schedule table") for v in (sqrt_ac, sqrt_1mac, p2w)]
        if saves is None:
            saves = self.new_saves(B, T)
        sp, sn = self._aligned(saves)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        out = torch.empty(B, T, D, dtype=torch.float32, device=self.device) if want_out else None
        w, keep = self._struct(tensors)
        ws, wn = self._workspace(B, T)
        with torch.cuda.device(self.dev_index):
            _lib.check_train(self.lib.egoego_train_forward(
                self._ctx, C.byref(w), xs.data_ptr(), nz.data_ptr(), cn.data_ptr(), cm.data_ptr(), tt.data_ptr(),
                None if rm is None else rm.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                _lib.PRED_X0 if objective == "pred_x0" else _lib.PRED_NOISE, _lib.LOSS_L1 if loss_type == "l1" else _lib.LOSS_L2,
                float(p_drop), int(seed), None if wid is None else wid.data_ptr(), B, T, sp, sn, ws, wn, loss.data_ptr(),
                None if out is None else out.data_ptr(), self._stream()))
        del keep
        return loss, out, saves

    def backward(self, tensors, saves, upstream, B, T, p_drop=0.0, seed=0, grads=None):
        """-> dict name -> gradient of upstream * loss (fresh tensors shaped like the parameters, or `grads` overwritten).
        upstream: a device scalar."""
        up = upstream.to(self.device, torch.float32).reshape(1).contiguous()
        if grads is None:
            grads = {n: torch.empty_like(tensors[n]) for n in self.names if not n.endswith("position_vec.weight")}
        w, keep = self._struct(tensors)
        g, gkeep = self._struct(grads, frozen_ok=True)
        sp, sn = self._aligned(saves)
        ws, wn = self._workspace(B, T)
        with torch.cuda.device(self.dev_index):
            _lib.check_train(self.lib.egoego_train_backward(self._ctx, C.byref(w), sp, sn, up.data_ptr(), C.byref(g), float(p_drop), int(seed),
                                                            B, T, ws, wn, self._stream()))
        del keep, gkeep
        return grads

    # ------------------------------------------------------------------ test / debug surface
    def dropout_mask(self, p_drop, seed, layer, site, B, T, window_ids=None):
        """The mask (bool) a forward with these arguments applies: site "attn" [B, 4, T+1, T+1], "fc" / "ffn" [B, T+1, 512]."""
        L = T + 1
        shape = (B, 4, L, L) if site == "attn" else (B, L, 512)
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        wid = None if window_ids is None else torch.as_tensor(window_ids).to(self.device, torch.int64).contiguous()
        ws, wn = self._workspace(B, T)
        with torch.cuda.device(self.dev_index):
            _lib.check_train(self.lib.egoego_train_dropout_mask(self._ctx, float(p_drop), int(seed), layer, SITES[site],
                                                                None if wid is None else wid.data_ptr(), B, T, out.data_ptr(), ws, wn,
                                                                self._stream()))
        return out.bool()

    def saved(self, saves, B, T, layer, which):
        """One saved tensor of one layer of the forward call that filled `saves` (names: _lib.TRAIN_SAVED)."""
        L = T + 1
        shape = {"attn_prob": (B, 4, L, L), "attn_out": (B, L, 1024)}.get(which, (B, L, 512))
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        sp, sn = self._aligned(saves)
        with torch.cuda.device(self.dev_index):
            _lib.check_train(self.lib.egoego_train_saved(self._ctx, sp, sn, B, T, layer, _lib.TRAIN_SAVED[which], out.data_ptr(), self._stream()))
        return out


class HipTrainingLoss(torch.autograd.Function):
    """loss = HipTrainingLoss.apply(engine, names, meta, *params): the forward pass keeps its saves on the autograd context (two graphs
    may be outstanding at once); the backward pass multiplies by the incoming gradient on the device and returns one gradient per
    parameter in its own shape (conv weights (out, in, 1)), None for a parameter that does not require one."""

    @staticmethod
    def forward(ctx, engine, names, meta, *params):
        tensors = {n: p.detach() for n, p in zip(names, params)}
        loss, _, saves = engine.forward(tensors, **meta)
        ctx.engine, ctx.names, ctx.saves = engine, names, saves
        ctx.call = (int(meta["x_start"].shape[0]), int(meta["x_start"].shape[1]), float(meta.get("p_drop", 0.0)), int(meta.get("seed", 0)))
        ctx.save_for_backward(*params)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        params = ctx.saved_tensors
        tensors = {n: p.detach() for n, p in zip(ctx.names, params)}
        B, T, p_drop, seed = ctx.call
        grads = ctx.engine.backward(tensors, ctx.saves, grad_loss, B, T, p_drop, seed)
        out = tuple(grads.get(n) if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[3:]))
        return (None, None, None) + out


def _dropout_p(denoise_fn):
    """The module's dropout probability (0 in eval mode); the three sites of every layer share it, as in the reference."""
    if not denoise_fn.training:
        return 0.0
    ps = {float(m.p_drop) for layer in denoise_fn.motion_transformer.layer_stack for m in (layer.self_attn, layer.pos_ffn)}
    if len(ps) != 1:
        raise _lib.EgoEgoHipError(f"the HIP training step applies one dropout probability to every site; the module has {sorted(ps)}")
    return ps.pop()


def training_loss(model, engine, x_start, cond_mask, t, noise, cond_noise, padding_mask, seed):
    """p_losses on the HIP path for a CondGaussianDiffusion `model`; every random tensor is the caller's draw."""
    d = model.denoise_fn
    named = dict(d.named_parameters())
    names = engine.names
    params = [named[n] for n in names]
    meta = dict(x_start=x_start, noise=noise, cond_noise=cond_noise, cond_mask=cond_mask, t=t,
                row_mask=None if padding_mask is None else padding_mask[:, 0, :],
                sqrt_ac=model.sqrt_alphas_cumprod, sqrt_1mac=model.sqrt_one_minus_alphas_cumprod, p2w=model.p2_loss_weight,
                objective=model.objective, loss_type=model.loss_type, p_drop=_dropout_p(d), seed=seed)
    return HipTrainingLoss.apply(engine, names, meta, *params)
