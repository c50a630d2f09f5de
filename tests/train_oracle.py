"""A functional restatement of CondGaussianDiffusion.p_losses for the training-step tests: explicit draws, explicit dropout masks,
optional FORCED ReLU masks and l1 signs, any dtype, any product.  Host code only.

Three uses of one function, `p_losses`:
    fp64, exact products                        the reference value (g64)
    fp64, every product as split-bf16           `mm=split_mm`: what three bf16 MFMAs per product compute, forward and backward, with
                                                an exact accumulation (e_emul)
    fp32, exact products                        the plain torch path's rounding (e_32)
tests/test_train.py pins the first, with nothing forced, to the module's own plain path.

Why forcing: a ReLU decision (and the sign of out - target under l1) is a kink.  A forward pass that differs from fp64 by 1e-5 flips
the few decisions whose pre-activation is smaller than that, and each flip moves the gradients by far more than the rounding of
the products does.  A test of the products therefore reads the decisions the code under test took, checks that every one that
differs from fp64 sits inside the forward error, and hands them to this function as forced.
"""
import math

import torch

N_HEAD, D_K = 4, 256
TR = "denoise_fn.motion_transformer."


def trainable(sd):
    """The names of the trainable tensors of a state dict (the position table is frozen, the schedule buffers are no parameters)."""
    return [k for k in sd if k.startswith("denoise_fn.") and not k.endswith("position_vec.weight")]


# ------------------------------------------------------------------------------------------------ products
def exact_mm(a, b):
    return a @ b


def _split(x):
    """fp64 -> (hi, lo) in fp64: the two bf16 numbers a split-bf16 MFMA reads of the fp32 value."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


def _split_product(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bh + al @ bh + ah @ bl


class _SplitMM(torch.autograd.Function):
    """a @ b with every product as hi*hi + lo*hi + hi*lo, and the same for the two products of its backward pass."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _split_product(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _split_product(g, b.transpose(-1, -2)), _split_product(a.transpose(-1, -2), g)


def split_mm(a, b):
    return _SplitMM.apply(a, b)


# ------------------------------------------------------------------------------------------------ the model
def time_embedding(t):
    """SinusoidalPosEmb(64) exactly as the module computes it in fp32 (frequencies and angles are fp32 values)."""
    half = 32
    freqs = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    ang = t.to(torch.float32)[:, None] * freqs[None, :]
    return ang, freqs


def _layer_norm(z, g, b):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + 1e-5) * g + b


def _linear(mm, x, w, b):
    """x [R, K], w [N, K(, 1)]"""
    w = w[:, :, 0] if w.dim() == 3 else w
    return mm(x, w.transpose(0, 1)) + b


def _drop(x, mask, p):
    return x if mask is None else x * mask.to(x.dtype) / (1.0 - p)


def p_losses(sd, x_start, noise, cond_noise, cond_mask, t, tables, row_mask=None, objective="pred_x0", loss_type="l1", p_drop=0.0,
             drop_masks=None, relu_masks=None, loss_sign=None, mm=exact_mm, dtype=torch.float64):
    """sd: name -> tensor (leaves of `dtype` that require grad where a gradient is wanted).  tables: (sqrt_alphas_cumprod,
    sqrt_one_minus_alphas_cumprod, p2_loss_weight).  row_mask [B, T+1] or None.  drop_masks: {(layer, "attn" | "fc" | "ffn"): bool
    mask} ([B, 4, L, L] / [B, L, 512]) or None.  relu_masks: per layer a bool [B, L, 512] that REPLACES the ReLU decision, or None.
    loss_sign: [B, T, D] in {-1, 0, 1} that REPLACES sign(out - target) under l1, or None.
    -> dict(loss, out [B, T, D], ffn_pre: per layer the pre-activation [B, L, 512], diff = out - target)."""
    B, T, D = x_start.shape
    L = T + 1
    c = lambda v: v.to(dtype)
    xs, nz, cn, cm = c(x_start), c(noise), c(cond_noise), c(cond_mask.expand(B, T, D))
    a1, a2, p2w = (c(v)[t] for v in tables)
    x = a1[:, None, None] * xs + a2[:, None, None] * nz
    x_cond = xs * (1.0 - cm) + cm * cn
    ang = time_embedding(t)[0].to(dtype)
    emb = torch.cat((ang.sin(), ang.cos()), -1)
    h1 = _linear(mm, emb, sd["denoise_fn.time_mlp.1.weight"], sd["denoise_fn.time_mlp.1.bias"])
    gl = 0.5 * h1 * (1.0 + torch.erf(h1 / math.sqrt(2.0)))
    tok = _linear(mm, gl, sd["denoise_fn.time_mlp.3.weight"], sd["denoise_fn.time_mlp.3.bias"])
    e = _linear(mm, torch.cat((x, x_cond), -1).reshape(B * T, 2 * D), sd[TR + "start_conv.weight"], sd[TR + "start_conv.bias"])
    h = torch.cat((tok[:, None, :], e.reshape(B, T, -1)), 1) + c(sd[TR + "position_vec.weight"])[1:L + 1][None]
    keep = None if row_mask is None else c(row_mask)[:, :, None]
    n_layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(TR + "layer_stack."))
    dm = (lambda l, s: None) if drop_masks is None else (lambda l, s: drop_masks[(l, s)])
    ffn_pre = []
    for l in range(n_layers):
        a, f = TR + f"layer_stack.{l}.self_attn.", TR + f"layer_stack.{l}.pos_ffn."
        hr = h.reshape(B * L, -1)
        q, k, v = (_linear(mm, hr, sd[a + n + ".weight"], sd[a + n + ".bias"]).reshape(B, L, N_HEAD, D_K).transpose(1, 2)
                   for n in ("w_q", "w_k", "w_v"))
        p = torch.softmax(mm(q, k.transpose(-1, -2)) / math.sqrt(D_K), dim=-1)
        p = _drop(p, dm(l, "attn"), p_drop)
        o = mm(p, v).transpose(1, 2).reshape(B * L, N_HEAD * D_K)
        y = _linear(mm, o, sd[a + "fc.weight"], sd[a + "fc.bias"]).reshape(B, L, -1)
        h = _layer_norm(_drop(y, dm(l, "fc"), p_drop) + h, sd[a + "layer_norm.weight"], sd[a + "layer_norm.bias"])
        if keep is not None:
            h = h * keep
        pre = _linear(mm, h.reshape(B * L, -1), sd[f + "w_1.weight"], sd[f + "w_1.bias"])
        ffn_pre.append(pre.reshape(B, L, -1))
        hid = torch.relu(pre) if relu_masks is None else pre * relu_masks[l].reshape(B * L, -1).to(dtype)
        y = _linear(mm, hid, sd[f + "w_2.weight"], sd[f + "w_2.bias"]).reshape(B, L, -1)
        h = _layer_norm(_drop(y, dm(l, "ffn"), p_drop) + h, sd[f + "layer_norm.weight"], sd[f + "layer_norm.bias"])
        if keep is not None:
            h = h * keep
    out = _linear(mm, h[:, 1:].reshape(B * T, -1), sd["denoise_fn.linear_out.weight"], sd["denoise_fn.linear_out.bias"]).reshape(B, T, D)
    target = xs if objective == "pred_x0" else nz
    diff = out - target
    if loss_type == "l2":
        el = diff ** 2
    elif loss_sign is None:
        el = diff.abs()
    else:
        el = diff * c(loss_sign)
    if row_mask is not None:
        el = el * c(row_mask)[:, 1:, None]
    loss = (el.flatten(1).mean(1) * p2w).mean()
    return dict(loss=loss, out=out, ffn_pre=ffn_pre, diff=diff)


def leaves(sd, dtype=torch.float64):
    """A copy of a state dict as autograd leaves of `dtype` (the frozen position table without a gradient)."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("denoise_fn."):
            continue
        t = v.detach().to("cpu", dtype).clone()
        if not k.endswith("position_vec.weight"):
            t.requires_grad_(True)
        out[k] = t
    return out


def loss_and_grads(sd, *args, dtype=torch.float64, **kw):
    """p_losses on fresh leaves of `dtype` -> (the result dict with everything detached, {name: gradient in fp64})."""
    lv = leaves(sd, dtype)
    r = p_losses(lv, *args, dtype=dtype, **kw)
    r["loss"].backward()
    grads = {k: lv[k].grad.to(torch.float64) for k in trainable(lv)}
    res = dict(loss=r["loss"].detach(), out=r["out"].detach(), ffn_pre=[p.detach() for p in r["ffn_pre"]], diff=r["diff"].detach())
    return res, grads


def rel_err(g, ref):
    return float((g.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))
