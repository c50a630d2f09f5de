#!/usr/bin/env python3
"""Stage-1 timing: HeadNet (window 60, 2 layers) + GravityNet (window 120, 2 layers) on B sequences of 139 frames, the demo
shapes, through the HIP library against the same fp32 computation as stock torch ops on the GPU.

    python tools/stage1_bench.py [--batches 1,64,256] [--iters 50] [--out stage1_bench.json]

Times (CUDA events, median of --iters after warm-up) cover the device work of one call per stage: HeadNet's encode of every block
of every sequence plus its integration kernel, GravityNet's feature kernel plus its encode.  The host steps the reference keeps in
numpy (Rodrigues, Umeyama on 3 x 3) are not included.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import _lib, stage1, synthetic  # noqa: E402

T_FRAMES = 139


def torch_decoder(sd, feats, valid, n_layers, n_head=4):
    """TM Decoder (use_full_attention) as batched fp32 torch ops: the stock-PyTorch baseline."""
    tr = "action_transformer."
    W, T, _ = feats.shape
    mask = (torch.arange(T, device=feats.device)[None, :] < valid[:, None]).float()[..., None]
    out = F.conv1d((feats * mask).transpose(1, 2), sd[tr + "start_conv.weight"], sd[tr + "start_conv.bias"]).transpose(1, 2)
    out = out + sd[tr + "position_vec.weight"][1:T + 1][None]
    for i in range(n_layers):
        a, f = tr + f"layer_stack.{i}.self_attn.", tr + f"layer_stack.{i}.pos_ffn."
        q = F.linear(out, sd[a + "w_q.weight"], sd[a + "w_q.bias"]).view(W, T, n_head, -1).transpose(1, 2)
        k = F.linear(out, sd[a + "w_k.weight"], sd[a + "w_k.bias"]).view(W, T, n_head, -1).transpose(1, 2)
        v = F.linear(out, sd[a + "w_v.weight"], sd[a + "w_v.bias"]).view(W, T, n_head, -1).transpose(1, 2)
        att = torch.softmax(q @ k.transpose(-1, -2) / 16.0, -1)
        o = (att @ v).transpose(1, 2).reshape(W, T, -1)
        o = F.layer_norm(F.linear(o, sd[a + "fc.weight"], sd[a + "fc.bias"]) + out, (256,), sd[a + "layer_norm.weight"],
                         sd[a + "layer_norm.bias"]) * mask
        h = F.linear(F.relu(F.linear(o, sd[f + "w_1.weight"][..., 0], sd[f + "w_1.bias"])), sd[f + "w_2.weight"][..., 0], sd[f + "w_2.bias"])
        out = F.layer_norm(h + o, (256,), sd[f + "layer_norm.weight"], sd[f + "layer_norm.bias"]) * mask
    return out


def torch_heads(sd, x, prefix, n):
    for j in range(n):
        x = torch.relu(F.linear(x, sd[f"{prefix}_mlp.affine_layers.{j}.weight"], sd[f"{prefix}_mlp.affine_layers.{j}.bias"]))
    return F.linear(x, sd[f"{prefix}_fc.weight"], sd[f"{prefix}_fc.bias"])


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    hcfg, gcfg = synthetic.Stage1Config("headnet", 60, 2), synthetic.Stage1Config("gravitynet", 120, 2)
    hsd = {k: v.to(dev) for k, v in synthetic.make_stage1_weights("headnet", hcfg, 0).items()}
    gsd = {k: v.to(dev) for k, v in synthetic.make_stage1_weights("gravitynet", gcfg, 0).items()}
    he, ge = stage1.Stage1Engine(hcfg, dev), stage1.Stage1Engine(gcfg, dev)
    he.load(hsd)
    ge.load(gsd)
    lib = _lib.load()
    spans = stage1.block_spans(T_FRAMES, 60)
    rows = []
    for B in [int(v) for v in opt.batches.split(",")]:
        g = torch.Generator(device="cpu").manual_seed(B)
        of = torch.randn(B, len(spans) * 60, 512, generator=g)
        of[:, T_FRAMES:] = 0
        hfeats = of.reshape(B * len(spans), 60, 512).to(dev)
        hvalid = torch.tensor([n for _, n in spans] * B, dtype=torch.int32, device=dev)
        q0 = torch.tensor([[1.0, 0, 0, 0]] * B, dtype=torch.float64, device=dev)
        slam = torch.cumsum(torch.randn(B, T_FRAMES + 1, 3, generator=g, dtype=torch.float64) * 0.01, 1).to(dev)
        L = T_FRAMES + 1
        quat = torch.empty(B, L, 4, dtype=torch.float64, device=dev)
        trans = torch.empty(B, L, 3, dtype=torch.float64, device=dev)
        scale = torch.empty(B, dtype=torch.float64, device=dev)
        Tt = torch.full((B,), T_FRAMES, dtype=torch.int32, device=dev)
        w0 = torch.arange(B, dtype=torch.int32, device=dev) * len(spans)
        ln = torch.full((B,), L, dtype=torch.int32, device=dev)
        qr = torch.randn(B, L, 4, generator=g)
        from egoego_release_amd import rotations
        rot = rotations.quaternion_to_matrix(qr / qr.norm(dim=-1, keepdim=True)).float().reshape(B, L, 9).contiguous().to(dev)
        gtr = slam.float().contiguous()
        gfeats = torch.empty(B, 120, 18, device=dev)
        gvalid = torch.empty(B, dtype=torch.int32, device=dev)

        def hip_call():
            heads = he.encode(hfeats, hvalid)
            _lib.check_s1(lib.egoego_s1_integrate(heads.data_ptr(), 60, Tt.data_ptr(), w0.data_ptr(), q0.data_ptr(), slam.data_ptr(),
                                                  ln.data_ptr(), B, L, L, 10.0, quat.data_ptr(), trans.data_ptr(), scale.data_ptr(),
                                                  he._stream()))
            _lib.check_s1(lib.egoego_s1_gravity_features(rot.data_ptr(), gtr.data_ptr(), ln.data_ptr(), B, L, 120, gfeats.data_ptr(),
                                                         gvalid.data_ptr(), ge._stream()))
            ge.encode(gfeats, gvalid)

        def hip_head():
            he.encode(hfeats, hvalid)

        def hip_grav():
            ge.encode(gfeats, gvalid)

        def torch_call():
            x = torch_decoder(hsd, hfeats, hvalid, 2)
            torch_heads(hsd, x, "action_va", 3)
            torch_heads(hsd, x, "action_dist", 3)
            y = torch_decoder(gsd, gfeats, gvalid, 2)
            torch_heads(gsd, y[:, 0], "action_normal", 2)

        with torch.no_grad():
            r = {"B": B, "windows_headnet": B * len(spans), "windows_gravitynet": B,
                 "hip_us": timed(hip_call, opt.iters), "hip_headnet_encode_us": timed(hip_head, opt.iters),
                 "hip_gravitynet_encode_us": timed(hip_grav, opt.iters), "torch_fp32_networks_us": timed(torch_call, opt.iters),
                 "launches_per_call": (1 + 3 * 2 + 4) + 1 + 1 + (1 + 3 * 2 + 3)}
        r["speedup_vs_torch"] = r["torch_fp32_networks_us"] / (r["hip_headnet_encode_us"] + r["hip_gravitynet_encode_us"])
        rows.append(r)
    res = {"workload": f"stage 1 demo shapes: HeadNet 60x2 + GravityNet 120x2, {T_FRAMES} frames per sequence", "rows": rows}
    line = json.dumps(res)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
