#!/usr/bin/env python3
"""Flow-CNN timing: FlowFeatureExtractor.extract (egoego/model/resnet.py FeatureExtractor on libegoego_hip) on 139, 8 x 139 and
64 x 139 frames of 224 x 224 optical flow, against the same network as stock fp32 torch ops on the GPU (F.conv2d etc., the
reference's input prep, eval-mode BatchNorm).

    python tools/flow_cnn_bench.py [--frames 139,1112,8896] [--iters 3] [--out profiles/flow_cnn_bench.json]

Times are CUDA events around one call (median of --iters after one warm-up), input already on the GPU.  FLOPs are algorithmic:
2 * MACs of every convolution with the 2 real input channels of conv1 (K = 98), plus fc.  The fraction of peak is against the
bf16 dense peak (2.5 PFLOP/s); split-bf16 issues three MFMAs per product, so the matrix pipe's busy fraction is three times that.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import stage1, synthetic  # noqa: E402

BF16_PEAK = 2.5e15
LAUNCHES_PER_CHUNK = 23  # stem conv, max-pool, 19 block convolutions (16 3 x 3 + 3 downsample), average pool, fc


def flops_per_frame():
    """2 * MACs of every convolution at its own input size (conv1 with its 2 real input channels) plus fc."""
    total, hw = 2 * 112 * 112 * 64 * 2 * 7 * 7, 56  # conv1; the max-pool leaves 56 x 56
    for conv, _, cin, cout, k, s, p in synthetic.flow_cnn_convs()[1:]:
        if conv.endswith("conv1"):
            block_in = hw  # a block's conv1 and its downsample read the block's input
        src = mid if conv.endswith("conv2") else block_in
        oh = (src + 2 * p - k) // s + 1
        total += 2 * oh * oh * cout * cin * k * k
        if conv.endswith("conv1"):
            mid = oh
        elif conv.endswith("conv2"):
            hw = oh
    return total + 2 * 512 * 512


def torch_resnet(sd, flow, chunk=512):
    """The reference's forward as fp32 torch ops on the GPU, in chunks of `chunk` frames."""
    g = lambda k: sd["cnn.resnet." + k]  # noqa: E731

    def bn(x, n):
        return F.batch_norm(x, g(n + ".running_mean"), g(n + ".running_var"), g(n + ".weight"), g(n + ".bias"), False, 0.0, 1e-5)

    outs = []
    for i in range(0, flow.shape[0], chunk):
        of = flow[i:i + chunk]
        of = torch.cat((of, torch.zeros(of.shape[:-1] + (1,), device=of.device)), -1).permute(0, 3, 1, 2)
        x = F.max_pool2d(F.relu(bn(F.conv2d(of, g("conv1.weight"), stride=2, padding=3), "bn1")), 3, 2, 1)
        for li in range(1, 5):
            for b in range(2):
                p = f"layer{li}.{b}."
                s = 2 if li > 1 and b == 0 else 1
                h = F.relu(bn(F.conv2d(x, g(p + "conv1.weight"), stride=s, padding=1), p + "bn1"))
                h = bn(F.conv2d(h, g(p + "conv2.weight"), padding=1), p + "bn2")
                idn = bn(F.conv2d(x, g(p + "downsample.0.weight"), stride=2), p + "downsample.1") if s == 2 else x
                x = F.relu(h + idn)
        outs.append(F.linear(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1), g("fc.weight"), g("fc.bias")))
    return torch.cat(outs)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="139,1112,8896")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "flow_cnn_bench.json"))
    a = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    m = stage1.FlowFeatureExtractor(seed=0).to("cuda:0")
    sd = {k: v.to("cuda:0") for k, v in m.state_dict().items()}
    base = torch.from_numpy(synthetic.make_flows(139, 1)).to("cuda:0")
    fpf = flops_per_frame()
    chunk = m.engine().chunk_frames or 256
    res = {"flops_per_frame": fpf, "bf16_peak": BF16_PEAK, "chunk_frames": chunk, "launches_per_chunk": LAUNCHES_PER_CHUNK,
           "sizes": []}
    for n in [int(v) for v in a.frames.split(",")]:
        flow = base.repeat((n + 138) // 139, 1, 1, 1)[:n].contiguous()
        t_hip = timed(lambda: m.extract(flow), a.iters)
        row = {"frames": n, "hip_ms": round(t_hip, 3), "chunks": (n + chunk - 1) // chunk,
               "launches": LAUNCHES_PER_CHUNK * ((n + chunk - 1) // chunk),
               "hip_tflops": round(fpf * n / t_hip / 1e9, 1), "bf16_peak_fraction": round(fpf * n / (t_hip * 1e-3) / BF16_PEAK, 4)}
        row["matrix_pipe_fraction"] = round(3 * row["bf16_peak_fraction"], 4)
        if not a.no_torch:
            with torch.no_grad():
                t_t = timed(lambda: torch_resnet(sd, flow), a.iters)
                e = float((torch_resnet(sd, flow[:139]) - m.extract(flow[:139])).abs().max())
            row.update(torch_fp32_ms=round(t_t, 3), speedup=round(t_t / t_hip, 2), max_abs_diff_vs_torch=e)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
