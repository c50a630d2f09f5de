"""The parameter update of stage-2 training on the HIP library (csrc/optim_step.*): gradient norm, NaN skip, unscale, Adam, EMA and
gradient clearing in one call that keeps its counters on the device and reads nothing back.

    UpdateEngine   one egoego_optim_ctx over a list of tensors, with its state block (counters + descriptor tables)
    FusedAdam      torch.optim.Adam's constructor, param_groups and state_dict layout in front of it
    FusedAdamW     torch.optim.AdamW's (decoupled weight decay), with clip_grad_norm_ inside the step: stage-1 training's update
    EMA            what the reference constructs from ema-pytorch: .ema_model, .online_model, .update(), the same state_dict keys

`fused=False` is the plain path of both classes: torch.optim.Adam inside and ema-pytorch's three-line lerp, on any device, with
the same skip rule (it reads the decision back every step).  The HIP path has no fallback: off the GPU it raises.
"""
import copy
import ctypes as C

import torch
from torch import nn

from . import _lib
from ._engine import ContextEngine

_HDR = {n: getattr(_lib.OptimState, n).offset for n, _ in _lib.OptimState._fields_}
_HDR_BYTES = C.sizeof(_lib.OptimState)


def ema_decay(step, beta=0.995, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0):
    """ema-pytorch's get_current_decay at counter value `step` (the value AFTER update() has advanced it)."""
    e = max(step - update_after_step - 1, 0)
    if e <= 0:
        return 0.0
    return min(max(1.0 - (1.0 + e / inv_gamma) ** -power, min_value), beta)


def ema_action(step, initted, update_every=10, update_after_step=100):
    """What update() does when it reads counter value `step`: "none", "copy" or "lerp" (the first call past update_after_step
    copies and sets `initted`)."""
    if step % update_every != 0:
        return "none"
    if step <= update_after_step or not initted:
        return "copy"
    return "lerp"


class UpdateEngine(ContextEngine):
    """One fused-update context on one GPU over parallel lists of fp32 contiguous tensors."""

    NOUN = "the fused parameter update"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_optim_ctx_create", "egoego_optim_ctx_destroy", "egoego_optim_workspace_bytes"
    CHECK = _lib.check_optim

    def __init__(self, counts, device):
        super().__init__(device)
        self.counts = [int(c) for c in counts]
        arr = (C.c_int64 * len(self.counts))(*self.counts)
        self._create(self.dev_index, len(self.counts), arr)
        n = self.lib.egoego_optim_state_bytes(self._ctx)
        if n == 0:
            raise _lib.EgoEgoHipError(_lib.check_optim.last_error())
        buf = torch.zeros(n + 256, dtype=torch.uint8, device=self.device)
        off = (-buf.data_ptr()) % 256
        self.state = buf[off:off + n]  # zeroed: every counter starts at 0
        self._ptrs = None
        h = self.state
        self.adam_step = h[_HDR["adam_step"]:_HDR["adam_step"] + 8].view(torch.int64)
        self.last_grad_norm = h[_HDR["total_norm_f32"]:_HDR["total_norm_f32"] + 4].view(torch.float32)[0]
        self.last_skipped = h[_HDR["last_skip"]:_HDR["last_skip"] + 4].view(torch.int32)[0]
        self.last_clip_coef = h[_HDR["clip_coef"]:_HDR["clip_coef"] + 4].view(torch.float32)[0]

    def _check(self, name, lst):
        for i, (t, n) in enumerate(zip(lst, self.counts)):
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise _lib.EgoEgoHipError(f"{name}[{i}]: the fused update takes fp32 contiguous tensors of {n} elements on {self.device} "
                                          f"(got {tuple(t.shape)} {t.dtype} on {t.device}, contiguous={t.is_contiguous()})")

    def set_tensors(self, p, g=None, m=None, v=None, ema=None):
        """Refreshes the descriptor tables when a data_ptr has changed since the last call (a few launches; otherwise nothing)."""
        lists = (p, g, m, v, ema)
        ptrs = tuple(None if lst is None else tuple(t.data_ptr() for t in lst) for lst in lists)
        if ptrs == self._ptrs:
            return
        for name, lst in zip(("parameter", "gradient", "exp_avg", "exp_avg_sq", "EMA tensor"), lists):
            if lst is not None:
                if len(lst) != len(self.counts):
                    raise _lib.EgoEgoHipError(f"{len(lst)} {name}s for {len(self.counts)} tensors")
                self._check(name, lst)
        arrs = [None if q is None else (C.c_void_p * len(q))(*q) for q in ptrs]
        with torch.cuda.device(self.dev_index):
            _lib.check_optim(self.lib.egoego_optim_set_tensors(self._ctx, *arrs, self.state.data_ptr(), self.state.numel(), self._stream()))
        self._ptrs = ptrs

    def step(self, hyper=None, ema=None, losses=(), inv_scale=None, found_inf=None, skip_on="nan", zero_grads=False, decoupled=False,
             max_norm=None, clip_eps=1e-6):
        """hyper: (lr, beta1, beta2, eps, weight_decay) or None (the EMA alone); ema: an _lib.OptimEma or None.  decoupled:
        weight_decay in torch.optim.AdamW's form; max_norm: clip_grad_norm_'s, inside the step (<= 0: none).  With neither
        (max_norm None) the call is egoego_optim_step, else egoego_optimw_step."""
        wide = bool(decoupled) or max_norm is not None
        fn = self.lib.egoego_optimw_step if wide else self.lib.egoego_optim_step
        if hyper is None:
            h = None
        elif wide:
            h = _lib.OptimHyperW(*[float(x) for x in hyper], int(bool(decoupled)), 0.0 if max_norm is None else float(max_norm), float(clip_eps))
        else:
            h = _lib.OptimHyper(*[float(x) for x in hyper])
        losses = [l for l in losses]
        for l in losses + [t for t in (inv_scale, found_inf) if t is not None]:
            if l.device != self.device or l.dtype != torch.float32 or l.numel() != 1:
                raise _lib.EgoEgoHipError(f"losses, inv_scale and found_inf are fp32 device scalars on {self.device} (got {tuple(l.shape)} {l.dtype} on {l.device})")
        if len(losses) > _lib.OPTIM_MAX_LOSSES:
            raise _lib.EgoEgoHipError(f"{len(losses)} loss scalars: at most {_lib.OPTIM_MAX_LOSSES}")
        larr = (C.c_void_p * len(losses))(*[l.data_ptr() for l in losses]) if losses else None
        ws, wn = self._workspace() if h is not None else (None, 0)
        with torch.cuda.device(self.dev_index):
            _lib.check_optim(fn(
                self._ctx, None if h is None else C.byref(h), None if ema is None else C.byref(ema), larr, len(losses),
                None if inv_scale is None else inv_scale.data_ptr(), None if found_inf is None else found_inf.data_ptr(),
                _lib.OPTIM_SKIP[skip_on], int(bool(zero_grads)), int(h is not None), int(ema is not None),
                self.state.data_ptr(), self.state.numel(), ws, wn, self._stream()))

    def read_state(self):
        """-> dict of the state header's fields (one synchronisation)."""
        out = torch.empty(_HDR_BYTES, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.dev_index):
            _lib.check_optim(self.lib.egoego_optim_read_state(self._ctx, self.state.data_ptr(), self.state.numel(), out.data_ptr(), self._stream()))
        st = _lib.OptimState.from_buffer_copy(out.cpu().numpy().tobytes())
        return {n: getattr(st, n) for n, _ in _lib.OptimState._fields_}


def _invalidate(modules):
    for m in modules:
        if hasattr(m, "invalidate_engine"):
            m.invalidate_engine()


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad off) whose step is one fused call on the HIP library.

    step(ema=None, losses=None): `losses` are the micro-batches' loss scalars (device tensors): a NaN among them, a NaN gradient
    norm or the GradScaler's found_inf skips the step on the device — parameters, moments, EMA and the step counter stay as they
    are — and nothing is read back.  `ema`: an EMA over the same model, updated in the same call.  `modules`: the nn.Modules that
    own the parameters; invalidate_engine() is called on each after every step, because the write goes through raw pointers and
    bumps no `_version` (the sampler's packed weights would go stale).

    max_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_grad_norm, error_if_nonfinite=False) inside the step, after the
    unscale.  The update uses the clipped values, but the gradients in memory are NOT rewritten with them (torch clips in place;
    the plain path does too): after a fused step `.grad` holds what backward left, or zeros with zero_grads.  `last_grad_norm` is
    the norm before clipping, which is what clip_grad_norm_ returns; `last_clip_coef` the factor used (1 when nothing was clipped
    or the step was skipped).  Both are device scalars.  None (the default) is the path without clipping, unchanged."""

    _TORCH, _DECOUPLED = torch.optim.Adam, False  # the optimizer whose group keys, state dict and plain path this class has

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, fused=True,
                 modules=(), skip_on="nan", zero_grads=False, max_grad_norm=None):
        name = type(self).__name__
        if amsgrad or maximize:
            raise ValueError(f"{name} serves amsgrad=False, maximize=False")
        if max_grad_norm is not None and not (0.0 < float(max_grad_norm) < float("inf")):
            raise ValueError(f"max_grad_norm is None or a positive finite number, not {max_grad_norm!r}")
        if skip_on not in _lib.OPTIM_SKIP:
            raise ValueError(f"skip_on is 'nan' or 'nonfinite', not {skip_on!r}")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError(f"invalid lr {lr}, betas {betas}, eps {eps} or weight_decay {weight_decay}")
        # the keys of torch.optim.Adam's (AdamW's) groups, so that a state dict saved from one loads into the other (`fused` here
        # is torch's)
        defaults = dict(self._TORCH([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"{name} takes one param group")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_clip_coef = None
        self.hip = bool(fused)
        self.modules = tuple(modules)
        self.skip_on, self.zero_grads = skip_on, bool(zero_grads)
        self._step_supports_amp_scaling = True
        self._engine = None
        self._ema_pairs = {}
        self._plain = None
        self._host = {"applied": 0, "skipped": 0}
        self.last_grad_norm = None
        self.last_skipped = None
        if not self.hip:
            self._make_plain()

    # ------------------------------------------------------------------ shared
    def _params(self):
        return [p for p in self.param_groups[0]["params"] if p.requires_grad]

    def _grads(self, params):
        for p in params:
            if p.grad is None:
                raise RuntimeError(f"{type(self).__name__}.step(): a parameter that requires a gradient has none; run backward before the first step")
        return [p.grad for p in params]

    def zero_grad(self, set_to_none=False):
        """Clears the gradients in place (their pointers stay put); nothing to do when step() already cleared them."""
        if self.hip and self.zero_grads:
            return
        for p in self._params():
            if p.grad is not None:
                p.grad.detach_()
                p.grad.zero_()

    # ------------------------------------------------------------------ the plain path
    def _make_plain(self):
        self._plain = self._TORCH(self.param_groups[0]["params"], foreach=False)
        self._plain.param_groups, self._plain.state = self.param_groups, self.state

    def _step_plain(self, ema, losses):
        params = self._params()
        grads = self._grads(params)
        scale = getattr(self, "grad_scale", None)
        if scale is not None:
            inv = scale.double().reciprocal().float()
            for g in grads:
                g.mul_(inv.to(g.device))
        norm = torch.norm(torch.stack([torch.norm(g.detach(), 2.0) for g in grads]), 2.0)
        bad = torch.isnan(norm) if self.skip_on == "nan" else ~torch.isfinite(norm)
        for l in losses or ():
            bad = bad | (torch.isnan(l.detach()) if self.skip_on == "nan" else ~torch.isfinite(l.detach())).reshape(()).to(bad.device)
        found = getattr(self, "found_inf", None)
        if found is not None:
            bad = bad | (found.reshape(()) != 0).to(bad.device)
        self.last_grad_norm, self.last_skipped = norm, bad.to(torch.int32)
        if bool(bad):  # (the plain path reads its decision back)
            self._host["skipped"] += 1
        else:
            self._host["applied"] += 1
            if self.max_grad_norm is not None:  # in place, as torch does: the plain path leaves clipped gradients behind
                torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm, error_if_nonfinite=False, foreach=False)
                self.last_clip_coef = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
            self._plain.step()
            if ema is not None:
                ema.update()
        if self.zero_grads:
            for g in grads:
                g.zero_()
        _invalidate(self.modules)

    # ------------------------------------------------------------------ the HIP path
    def _hip_engine(self, params):
        if self._engine is None:
            dev = params[0].device
            if dev.type != "cuda":
                raise _lib.EgoEgoHipError(f"FusedAdam(fused=True) runs on the MI355X HIP path only (the parameters are on {dev}); "
                                          "fused=False is the plain path")
            self._engine = UpdateEngine([p.numel() for p in params], dev)
            self.last_grad_norm, self.last_skipped = self._engine.last_grad_norm, self._engine.last_skipped
            self.last_clip_coef = self._engine.last_clip_coef
            self._push_step()
        return self._engine

    def _moments(self, params):
        for p in params:
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return [self.state[p]["exp_avg"] for p in params], [self.state[p]["exp_avg_sq"] for p in params]

    def _push_step(self):
        """The `step` of the loaded / fresh state -> the device counter."""
        steps = {int(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam keeps one step counter for all parameters; the state has {sorted(steps)}")
        if self._engine is not None:
            self._engine.adam_step.fill_(steps.pop() if steps else 0)

    def _pull_step(self):
        if self._engine is not None and self.state:
            k = float(self._engine.adam_step.item())
            for st in self.state.values():
                if "step" in st:
                    st["step"] = torch.tensor(k, dtype=torch.float32)

    def _ema_tensors(self, ema, params):
        key = id(ema)
        if key not in self._ema_pairs:
            names = {id(p): n for n, p in ema.online_model.named_parameters()}
            shadow = dict(ema.ema_model.named_parameters())
            try:
                self._ema_pairs = {key: [shadow[names[id(p)]].data for p in params]}
            except KeyError:
                raise ValueError("step(ema=...): the EMA's online model does not own every parameter of this optimizer") from None
        return self._ema_pairs[key]

    @torch.no_grad()
    def step(self, closure=None, ema=None, losses=None):
        if closure is not None:
            raise ValueError("FusedAdam.step() takes no closure")
        if not self.hip:
            return self._step_plain(ema, losses)
        if ema is not None and not ema.hip:
            raise ValueError("step(ema=...) on the HIP path needs an EMA(fused=True)")
        params = self._params()
        eng = self._hip_engine(params)
        grads = self._grads(params)
        m, v = self._moments(params)
        shadow = None if ema is None else self._ema_tensors(ema, params)
        eng.set_tensors([p.data for p in params], grads, m, v, shadow)
        g = self.param_groups[0]
        inv = None
        scale = getattr(self, "grad_scale", None)
        if scale is not None:
            inv = scale.double().reciprocal().float().reshape(())
        found = getattr(self, "found_inf", None)
        eng.step((g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]), None if ema is None else ema._schedule(),
                 [l.detach().reshape(()) for l in (losses or ())], inv, None if found is None else found.reshape(()),
                 self.skip_on, self.zero_grads, self._DECOUPLED, self.max_grad_norm)
        _invalidate(self.modules)
        if ema is not None:
            _invalidate([ema.ema_model])

    def counters(self):
        """-> {'adam_step', 'applied', 'skipped', 'total_norm', 'last_skip', ...} (the HIP path: one synchronisation)."""
        if self.hip:
            if self._engine is None:
                return {"adam_step": 0, "applied": 0, "skipped": 0, "total_norm": 0.0, "last_skip": 0}
            return self._engine.read_state()
        steps = [int(st["step"]) for st in self.state.values() if "step" in st]
        return {"adam_step": steps[0] if steps else 0, **self._host,
                "total_norm": 0.0 if self.last_grad_norm is None else float(self.last_grad_norm),
                "last_skip": 0 if self.last_skipped is None else int(self.last_skipped)}

    # ------------------------------------------------------------------ torch.optim.Adam's state dict
    def state_dict(self):
        if self.hip:
            self._pull_step()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.hip:
            for p, st in self.state.items():  # the fused update takes contiguous moments; `step` stays a host scalar
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in st:
                        st[k] = st[k].contiguous()
                if "step" in st:
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).reshape(()).cpu()
            self._push_step()
        else:
            self._plain.param_groups, self._plain.state = self.param_groups, self.state


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW (amsgrad off) on the same fused call: p *= 1 - lr * weight_decay first, then Adam without the L2 term;
    torch.optim.AdamW's constructor (weight_decay = 1e-2), group keys and state dict, so a state dict goes either way.  One param
    group.  `lr` is read from param_groups[0] at every step, so torch's lr schedulers (StepLR) drive it unchanged.  fused=False is
    the unscale, clip_grad_norm_(error_if_nonfinite=False) and torch.optim.AdamW(foreach=False), under FusedAdam's skip rule."""

    _TORCH, _DECOUPLED = torch.optim.AdamW, True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, fused=True,
                 modules=(), skip_on="nan", zero_grads=False, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, fused=fused, modules=modules, skip_on=skip_on,
                         zero_grads=zero_grads, max_grad_norm=max_grad_norm)


class EMA(nn.Module):
    """ema-pytorch's EMA as the reference constructs it: EMA(model, beta=0.995, update_every=10).  `ema_model` is a deep copy with
    requires_grad off, `online_model` the model itself, `step` and `initted` are buffers, so state_dict() has the keys
    'ema_model.*', 'online_model.*', 'initted', 'step' (what harness.load_stage2_checkpoint reads).

    The warm-up schedule is restated from ema-pytorch 0.0.10's description and is NOT pinned against that package (it is not a
    dependency): every value of it is a constructor argument.  Only trainable tensors are touched: buffers and frozen parameters
    are equal in both models, and the lerp of equal values is exact."""

    def __init__(self, model, ema_model=None, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2.0 / 3.0,
                 min_value=0.0, fused=True):
        super().__init__()
        self.beta, self.update_after_step, self.update_every = float(beta), int(update_after_step), int(update_every)
        self.inv_gamma, self.power, self.min_value = float(inv_gamma), float(power), float(min_value)
        self.hip = bool(fused)
        self.online_model = model
        self.ema_model = copy.deepcopy(model) if ema_model is None else ema_model
        self.ema_model.requires_grad_(False)
        # the HIP path keeps both counters beside the parameters from the start: moved there by the first update instead, that
        # copy from host memory would be a synchronisation inside a training step
        dev = next(model.parameters()).device if self.hip else torch.device("cpu")
        dev = dev if dev.type == "cuda" else torch.device("cpu")
        self.register_buffer("initted", torch.Tensor([False]).to(dev))
        self.register_buffer("step", torch.tensor([0]).to(dev))
        self._engine = None

    def _pairs(self):
        shadow = dict(self.ema_model.named_parameters())
        return [(shadow[n], p) for n, p in self.online_model.named_parameters() if p.requires_grad]

    def _schedule(self):
        """The schedule and the two counters as the library takes them (the HIP path: counters on the parameters' device)."""
        dev = next(self.online_model.parameters()).device
        if self.step.device != dev or self.initted.device != dev:
            self.step.data, self.initted.data = self.step.data.to(dev), self.initted.data.to(dev)
        if self.step.dtype != torch.int64 or self.initted.dtype != torch.float32:
            raise _lib.EgoEgoHipError(f"EMA counters: step {self.step.dtype}, initted {self.initted.dtype}; int64 and float32 expected")
        return _lib.OptimEma(self.beta, self.inv_gamma, self.power, self.min_value, self.update_every, self.update_after_step,
                             self.step.data_ptr(), self.initted.data_ptr())

    def get_current_decay(self):
        return ema_decay(int(self.step.item()), self.beta, self.update_after_step, self.inv_gamma, self.power, self.min_value)

    def copy_params_from_model_to_ema(self):
        for e, p in self._pairs():
            e.data.copy_(p.data)
        _invalidate([self.ema_model])

    @torch.no_grad()
    def update(self):
        pairs = self._pairs()
        if self.hip:
            dev = pairs[0][1].device
            if dev.type != "cuda":
                raise _lib.EgoEgoHipError(f"EMA(fused=True) runs on the MI355X HIP path only (the model is on {dev}); fused=False is the plain path")
            if self._engine is None or self._engine.device != dev:
                self._engine = UpdateEngine([p.numel() for _, p in pairs], dev)
            self._engine.set_tensors([p.data for _, p in pairs], ema=[e.data for e, _ in pairs])
            self._engine.step(None, self._schedule())
            _invalidate([self.ema_model])
            return
        step = int(self.step.item())
        self.step += 1
        action = ema_action(step, bool(self.initted.item()), self.update_every, self.update_after_step)
        if action == "none":
            return
        if action == "copy":
            self.copy_params_from_model_to_ema()
            if step > self.update_after_step:
                self.initted.data.fill_(1.0)
            return
        decay = self.get_current_decay()
        for e, p in pairs:
            difference = e.data - p.data
            difference.mul_(1.0 - decay)
            e.data.sub_(difference)
        _invalidate([self.ema_model])

    def __call__(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)
