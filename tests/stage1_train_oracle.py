"""A functional restatement of stage-1 training for its tests: HeadFormer / HeadNormalFormer forward + compute_loss under autograd
(HE = egoego/model/head_estimation_transformer.py:97-178, 310-345; HN = egoego/model/head_normal_estimation_transformer.py:118-155,
334-342; TM = egoego/model/transformer_module.py), with explicit dropout masks, optional FORCED ReLU masks and quaternion sign
decisions, any dtype, any product.  Host code only.  Built on stage1_oracle (the names, the inference restatement it is pinned to)
and on train_oracle's products: exact_mm (fp64 / fp32) and split_mm (every product as three bf16 products, forward and backward).

The four pytorch3d.transforms functions the reference calls are written here from their published formulas as differentiable torch
code; tests/golden/make_stage1_train_golden.py runs the reference's own modules on them and asserts that this file reproduces the
reference's loss parts, heads and gradients.
"""
import math

import torch

import stage1_oracle as S1
from train_oracle import _drop, _layer_norm, _linear, exact_mm, rel_err, split_mm  # noqa: F401  (re-exported for the tests)

TR = S1.TR
N_HEAD, D_K = 4, 256
HEADS = {"headnet": (("action_va", 3), ("action_dist", 3)), "gravitynet": (("action_normal", 2),)}


# ------------------------------------------------------------------------------------------------ pytorch3d.transforms stand-ins
def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    ow = aw * bw - ax * bx - ay * by - az * bz
    ox = aw * bx + ax * bw + ay * bz - az * by
    oy = aw * by - ax * bz + ay * bw + az * bx
    oz = aw * bz + ax * by - ay * bx + az * bw
    return torch.stack((ow, ox, oy, oz), -1)


def standardize_quaternion(q, negative=None):
    """negative: a bool tensor [...] that REPLACES the decision q[..., 0] < 0, or None."""
    neg = q[..., 0:1] < 0 if negative is None else negative[..., None]
    return torch.where(neg, -q, q)


def quaternion_multiply(a, b, negative=None):
    return standardize_quaternion(quaternion_raw_multiply(a, b), negative)


def quaternion_invert(q):
    return q * q.new_tensor([1, -1, -1, -1])


def quaternion_apply(q, p):
    real = p.new_zeros(p.shape[:-1] + (1,))
    out = quaternion_raw_multiply(quaternion_raw_multiply(q, torch.cat((real, p), -1)), quaternion_invert(q))
    return out[..., 1:]


def axis_angle_to_quaternion(aa):
    angles = torch.norm(aa, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    eps = 1e-6
    small = angles.abs() < eps
    s = torch.empty_like(angles)
    s[~small] = torch.sin(half[~small]) / angles[~small]
    s[small] = 0.5 - (angles[small] * angles[small]) / 48
    return torch.cat((torch.cos(half), aa * s), -1)


# ------------------------------------------------------------------------------------------------ HeadNet's loss
def va2rot(q0, va, chain_neg=None, dt=1 / 30):
    """HE:97-119: q0 [B, 4], va [B, T, 3] -> [B, T + 1, 4]; the running rotation is detached.  chain_neg [B, T] forces the sign
    standardisation of every chain product.  Also returns the real parts of the chain products before standardisation."""
    q = q0
    seq, reals = [q], []
    for t in range(va.shape[1]):
        angv = quaternion_apply(q.detach(), va[:, t])
        raw = quaternion_raw_multiply(axis_angle_to_quaternion(angv * dt), q.detach())
        reals.append(raw[:, 0].detach())
        new = standardize_quaternion(raw, None if chain_neg is None else chain_neg[:, t])
        q = new / torch.norm(new, dim=1).reshape(-1, 1)
        seq.append(q)
    return torch.stack(seq, 1), torch.stack(reals, 1)


def headnet_loss(va, dist, head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist, chain_neg=None, diff_neg=None):
    """HE:310-345 on va [B, T, 3], dist [B, T, 1] (any dtype; the targets are cast to it) -> dict(loss, orient, va, dist,
    chain_real [B, T], diff_real [B, T]): the two real parts are those the sign decisions read."""
    dt_ = va.dtype
    B, T, _ = va.shape
    pose, vels = head_pose.to(dt_), head_vels.to(dt_)
    quat, chain_real = va2rot(pose[:, 0, 3:], va, chain_neg)
    pred_q = quat[:, 1:].reshape(B * T, 4)
    gt_q = pose[:, 1:, 3:].reshape(B * T, 4)
    raw = quaternion_raw_multiply(gt_q, quaternion_invert(pred_q))
    d = standardize_quaternion(raw, None if diff_neg is None else diff_neg.reshape(B * T))
    iden = d.new_tensor([1.0, 0.0, 0.0, 0.0])
    orient = (d.abs() - iden).pow(2).sum(1).mean()
    va_l = (vels[:, :, 3:].reshape(B * T, 3) - va.reshape(B * T, 3)).pow(2).sum(1).mean()
    gt_d = dist_scale * torch.linalg.vector_norm(pose[:, 1:, :3] - pose[:, :-1, :3], dim=-1).reshape(B * T, 1)
    dist_l = (dist.reshape(B * T, 1) - gt_d).pow(2).sum(1).mean()
    loss = w_rotation * orient + w_va * va_l + w_dist * dist_l
    return dict(loss=loss, orient=orient, va=va_l, dist=dist_l, chain_real=chain_real, diff_real=raw[:, 0].detach().reshape(B, T))


def headnet_loss_and_grad(heads, T, head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist, **kw):
    """The fp64 reference of egoego_s1_headnet_loss on fp32 inputs: heads [B, window, 4] -> (loss parts fp64 [4], d(total) /
    d(heads) fp64 [B, window, 4] with rows t >= T zero, the result dict)."""
    h = heads.detach().to("cpu", torch.float64).clone().requires_grad_(True)
    r = headnet_loss(h[:, :T, :3], h[:, :T, 3:4], head_pose.cpu().float(), head_vels.cpu().float(), dist_scale, w_rotation, w_va, w_dist, **kw)
    r["loss"].backward()
    parts = torch.stack([r[k].detach() for k in ("loss", "orient", "va", "dist")])
    return parts, h.grad, r


def gravity_loss(pred, floor_normal):
    """HN:33-35, 334-342."""
    gt = floor_normal.to(pred.dtype).squeeze(-1)
    return (gt - pred).abs().sum(1).mean()


# ------------------------------------------------------------------------------------------------ the training encode
def head_linear_names(kind):
    out = []
    for pre, nh in HEADS[kind]:
        out += [f"{pre}_mlp.affine_layers.{j}" for j in range(nh)] + [f"{pre}_fc"]
    return out


def encode(sd, kind, feats, valid, n_layers, p_drop=0.0, drop_masks=None, relu_masks=None, head_masks=None, mm=exact_mm,
           dtype=torch.float64):
    """TM:188-225 (use_full_attention) + the MLP heads on feats [W, L, F] with rows t >= valid[w] as zero rows.  sd: name -> tensor
    (leaves of `dtype`).  drop_masks {(layer, "attn" | "fc" | "ffn"): bool [W, 4, L, L] / [W, L, 256]} or None; relu_masks: per layer
    a bool [W, L, 256] that REPLACES the FFN's ReLU decision; head_masks {linear name: bool [rows, width]} that REPLACES a head's.
    -> dict(heads [W, L, 4] | [W, 3], ffn_pre: per layer [W, L, 256], head_pre {linear name: pre-activation})."""
    W, L, _ = feats.shape
    keep = (torch.arange(L)[None, :] < torch.as_tensor(valid).reshape(-1)[:, None]).to(dtype)[:, :, None]
    x = torch.where(keep > 0, feats.to(dtype), torch.zeros((), dtype=dtype))
    h = _linear(mm, x.reshape(W * L, -1), sd[TR + "start_conv.weight"], sd[TR + "start_conv.bias"]).reshape(W, L, -1)
    h = h + sd[TR + "position_vec.weight"].to(dtype)[1:L + 1][None]
    dm = (lambda l, s: None) if drop_masks is None else (lambda l, s: drop_masks[(l, s)])
    ffn_pre = []
    for l in range(n_layers):
        a, f = TR + f"layer_stack.{l}.self_attn.", TR + f"layer_stack.{l}.pos_ffn."
        hr = h.reshape(W * L, -1)
        q, k, v = (_linear(mm, hr, sd[a + n + ".weight"], sd[a + n + ".bias"]).reshape(W, L, N_HEAD, D_K).transpose(1, 2)
                   for n in ("w_q", "w_k", "w_v"))
        p = torch.softmax(mm(q, k.transpose(-1, -2)) / math.sqrt(D_K), dim=-1)
        p = _drop(p, dm(l, "attn"), p_drop)
        o = mm(p, v).transpose(1, 2).reshape(W * L, N_HEAD * D_K)
        y = _linear(mm, o, sd[a + "fc.weight"], sd[a + "fc.bias"]).reshape(W, L, -1)
        h = _layer_norm(_drop(y, dm(l, "fc"), p_drop) + h, sd[a + "layer_norm.weight"], sd[a + "layer_norm.bias"]) * keep
        pre = _linear(mm, h.reshape(W * L, -1), sd[f + "w_1.weight"], sd[f + "w_1.bias"])
        ffn_pre.append(pre.reshape(W, L, -1))
        hid = torch.relu(pre) if relu_masks is None else pre * relu_masks[l].reshape(W * L, -1).to(dtype)
        y = _linear(mm, hid, sd[f + "w_2.weight"], sd[f + "w_2.bias"]).reshape(W, L, -1)
        h = _layer_norm(_drop(y, dm(l, "ffn"), p_drop) + h, sd[f + "layer_norm.weight"], sd[f + "layer_norm.bias"]) * keep
    rows = h.reshape(W * L, -1) if kind == "headnet" else h[:, 0]
    head_pre, outs = {}, []
    for pre_, nh in HEADS[kind]:
        z = rows
        for j in range(nh):
            nm = f"{pre_}_mlp.affine_layers.{j}"
            pz = _linear(mm, z, sd[nm + ".weight"], sd[nm + ".bias"])
            head_pre[nm] = pz
            z = torch.relu(pz) if head_masks is None else pz * head_masks[nm].reshape(pz.shape).to(dtype)
        outs.append(_linear(mm, z, sd[pre_ + "_fc.weight"], sd[pre_ + "_fc.bias"]))
    heads = torch.cat(outs, -1)
    heads = heads.reshape(W, L, 4) if kind == "headnet" else heads
    return dict(heads=heads, ffn_pre=ffn_pre, head_pre=head_pre)


def trainable(sd):
    return [k for k in sd if not k.endswith("position_vec.weight")]


def leaves(sd, dtype=torch.float64):
    """A copy of a state dict as autograd leaves of `dtype` (the frozen position table without a gradient)."""
    out = {}
    for k, v in sd.items():
        t = v.detach().to("cpu", dtype).clone()
        if not k.endswith("position_vec.weight"):
            t.requires_grad_(True)
        out[k] = t
    return out


def heads_and_grads(sd, kind, feats, valid, n_layers, upstream, dtype=torch.float64, **kw):
    """encode on fresh leaves of `dtype`, backward from the upstream gradient of the heads -> (the result dict, detached;
    {name: gradient in fp64})."""
    lv = leaves(sd, dtype)
    r = encode(lv, kind, feats, valid, n_layers, dtype=dtype, **kw)
    r["heads"].backward(upstream.to(dtype))
    grads = {k: lv[k].grad.to(torch.float64) for k in trainable(lv)}
    res = dict(heads=r["heads"].detach(), ffn_pre=[p.detach() for p in r["ffn_pre"]], head_pre={k: v.detach() for k, v in r["head_pre"].items()})
    return res, grads


def headnet_step(sd, data, opt, n_layers, dtype=torch.float64, mm=exact_mm):
    """HeadFormer forward + compute_loss on a reference-format batch -> (the loss dict, the leaves with .grad after backward, the
    heads, d loss / d heads)."""
    lv = leaves(sd, dtype)
    of = data["of"].to(dtype)
    r = encode(lv, "headnet", of, data["seq_len"], n_layers, mm=mm, dtype=dtype)
    heads = r["heads"]
    heads.retain_grad()
    ls = headnet_loss(heads[..., :3], heads[..., 3:4], data["head_pose"].float(), data["head_vels"].float(), opt.dist_scale,
                      opt.w_rotation, opt.w_va, opt.w_dist)
    ls["loss"].backward()
    return ls, lv, heads.detach(), heads.grad


def gravity_step(sd, feats, valid, floor_normal, n_layers, dtype=torch.float64, mm=exact_mm):
    lv = leaves(sd, dtype)
    r = encode(lv, "gravitynet", feats.to(dtype), valid, n_layers, mm=mm, dtype=dtype)
    heads = r["heads"]
    heads.retain_grad()
    loss = gravity_loss(heads, floor_normal)
    loss.backward()
    return loss, lv, heads.detach(), heads.grad
