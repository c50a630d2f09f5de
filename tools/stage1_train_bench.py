#!/usr/bin/env python3
"""Time one stage-1 training step — forward + loss + backward + clip_grad_norm_ + AdamW.step() — on the HIP path (hip_training:
egoego_s1_train_forward / egoego_s1_headnet_loss / egoego_s1_train_backward) against a plain fp32 torch module that restates the
reference step by step on the same parameters and the same GPU, its Python frame loops included (HeadFormer.va2rot and
get_dist_scalar: one iteration per frame, a dozen small quaternion ops each, under autograd).

    python tools/stage1_train_bench.py --out profiles/stage1_train_bench.json     HeadNet 90 x 2, GravityNet 120 x 2; B = 32, 128
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stage1_train_bench.py --only hip --kind headnet --batch 32 --rounds 1
                                                                                   (kernel shares: a run of its own)

Both paths are warmed at every shape, then timed in alternating rounds (hip, plain, hip, plain, ...) with device events around
`steps` whole steps each, so that a drift of the shared host hits both alike; the median round and the spread are reported.
The two paths see the same batch; their dropout masks differ (torch's generator against in-kernel Philox).  A GPU is required.
"""
import argparse
import json
import math
import os
import statistics
import sys
from argparse import Namespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import rotations as R3, stage1  # noqa: E402
from egoego_release_amd.synthetic import make_stage1_train_batch  # noqa: E402

SHAPES = {"headnet": (90, 2), "gravitynet": (120, 2)}  # the reference's defaults: window x layers


def opt_for(kind):
    window, layers = SHAPES[kind]
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                     w_rotation=1.0, w_va=1.0, w_dist=1.0)


def build(kind, hip):
    cls = stage1.HeadFormer if kind == "headnet" else stage1.HeadNormalFormer
    m = cls(opt_for(kind), torch.device("cuda")).cuda()
    m.hip_training = hip
    m.train()
    return m, torch.optim.AdamW(m.parameters(), lr=1e-4)


# ------------------------------------------------------------------------------------------------ the plain path
def plain_decoder(m, x, valid, p_drop):
    """TM:188-225 (use_full_attention) with torch ops on the module's own parameters: x [B, L, F] -> [B, L, 256]."""
    dec = m.action_transformer
    B, L, _ = x.shape
    keep = (torch.arange(L, device=x.device)[None, :] < valid[:, None]).float()[:, :, None]
    h = F.conv1d(x.transpose(1, 2), dec.start_conv.weight, dec.start_conv.bias).transpose(1, 2)
    h = h + dec.position_vec.weight[1:L + 1][None]
    for layer in dec.layer_stack:
        a, f = layer.self_attn, layer.pos_ffn
        q, k, v = (lin(h).view(B, L, 4, 256).transpose(1, 2) for lin in (a.w_q, a.w_k, a.w_v))
        p = F.dropout(torch.softmax(q @ k.transpose(-1, -2) / 16.0, dim=-1), p_drop, m.training)
        o = (p @ v).transpose(1, 2).reshape(B, L, 1024)
        h = a.layer_norm(F.dropout(a.fc(o), p_drop, m.training) + h) * keep
        y = F.conv1d(F.relu(F.conv1d(h.transpose(1, 2), f.w_1.weight, f.w_1.bias)), f.w_2.weight, f.w_2.bias).transpose(1, 2)
        h = f.layer_norm(F.dropout(y, p_drop, m.training) + h) * keep
    return h


def plain_mlp(m, pre, x):
    for lin in getattr(m, pre + "_mlp").affine_layers:
        x = torch.relu(lin(x))
    return getattr(m, pre + "_fc")(x)


def plain_headnet_loss(m, data):
    """HE:131-178 + 310-345, frame loops and all."""
    opt = m.opt
    x = data["of"].float()
    B, T, _ = x.shape
    h = plain_decoder(m, x, data["seq_len"], m.P_DROP)
    va, dist = plain_mlp(m, "action_va", h), plain_mlp(m, "action_dist", h)
    curr = data["head_pose"][:, 0, 3:]
    seq = [curr]
    for t in range(T):  # va2rot
        angv = R3.quaternion_apply(curr.detach().float(), va[:, t].float())
        new = R3.quaternion_multiply(R3.axis_angle_to_quaternion(angv * (1 / 30)), curr.detach())
        curr = new / torch.norm(new, dim=1).reshape(-1, 1)
        seq.append(curr)
    quat = torch.stack(seq, 1)
    lens = []
    for t in range(T):  # get_dist_scalar
        lens.append(torch.linalg.vector_norm(data["head_pose"][:, t + 1, :3] - data["head_pose"][:, t, :3], dim=1))
    gt_dist = opt.dist_scale * torch.stack(lens).transpose(0, 1).reshape(B * T, 1).float()
    pred_q, gt_q = quat[:, 1:].reshape(B * T, 4), data["head_pose"][:, 1:, 3:].reshape(B * T, 4).float()
    d = R3.quaternion_multiply(gt_q, R3.quaternion_invert(pred_q))
    iden = torch.tensor([1.0, 0.0, 0.0, 0.0], device=d.device).repeat(B * T, 1)
    orient = (torch.abs(d) - iden).pow(2).sum(dim=1).mean()
    va_l = (data["head_vels"][:, :, 3:].reshape(B * T, 3).float() - va.reshape(B * T, 3)).pow(2).sum(dim=1).mean()
    dist_l = (dist.reshape(B * T, 1) - gt_dist).pow(2).sum(dim=1).mean()
    return opt.w_rotation * orient + opt.w_va * va_l + opt.w_dist * dist_l


def plain_gravity_loss(m, data):
    """HN:118-165 + 334-342."""
    rot, trans = data["head_rot_mat"].float(), data["head_trans"].float()
    B, L = rot.shape[:2]
    d6 = rot[:, :, :2, :].reshape(B, L, 6)
    diff = torch.matmul(rot[:, 1:], rot[:, :-1].transpose(2, 3))
    x = torch.cat((d6[:, :-1], trans[:, :-1], diff[:, :, :2, :].reshape(B, L - 1, 6), trans[:, 1:] - trans[:, :-1]), -1)
    h = plain_decoder(m, x, data["seq_len"] - 1, m.P_DROP)
    pred = plain_mlp(m, "action_normal", h[:, 0])
    return (data["floor_normal"].squeeze(-1) - pred).abs().sum(dim=1).mean()


def one_step(m, opt, data, hip):
    if hip:
        loss = m.compute_loss(m(data), data)[0]
    else:
        loss = (plain_headnet_loss if m.cfg.kind == "headnet" else plain_gravity_loss)(m, data)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0, error_if_nonfinite=False)
    opt.step()
    return loss


def timed(m, opt, data, hip, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        one_step(m, opt, data, hip)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", nargs="+", default=["headnet", "gravitynet"], choices=("headnet", "gravitynet"))
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--steps", type=int, default=10, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "plain"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage1_train_bench needs a ROCm GPU: timings are not taken on the CPU")
    paths = [p for p in ("hip", "plain") if args.only in (None, p)]
    res = {"device": torch.cuda.get_device_name(0), "steps_per_round": args.steps, "rounds": args.rounds,
           "what": "forward + loss + backward + clip_grad_norm_ + AdamW.step(), ms per step, train() mode (dropout 0.1)", "cases": {}}
    for kind in args.kind:
        window, layers = SHAPES[kind]
        for B in args.batch:
            data = {k: v.cuda() for k, v in make_stage1_train_batch(kind, B, window, seed=1).items()}
            rigs = {p: build(kind, p == "hip") for p in paths}
            torch.manual_seed(0)
            first = {}
            for p in paths:
                first[p] = float(one_step(*rigs[p], data, p == "hip").detach())
                for _ in range(args.warmup - 1):
                    one_step(*rigs[p], data, p == "hip")
            if len(paths) == 2 and not math.isclose(first["hip"], first["plain"], rel_tol=0.3):
                raise SystemExit(f"{kind} B={B}: the two paths' first losses disagree: {first}")
            times = {p: [] for p in paths}
            for _ in range(args.rounds):
                for p in paths:
                    times[p].append(timed(*rigs[p], data, p == "hip", args.steps))
            row = {p: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "first_loss": first[p]} for p, v in times.items()}
            if len(paths) == 2:
                row["hip_over_plain"] = row["hip"]["median_ms"] / row["plain"]["median_ms"]
            res["cases"][f"{kind} window {window} x {layers} layers, B = {B}"] = row
            print(json.dumps({"kind": kind, "B": B, **row}), flush=True)
            del rigs
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
