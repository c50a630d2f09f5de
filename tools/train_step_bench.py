#!/usr/bin/env python3
"""Time one stage-2 training step — forward + backward + Adam.step() — on the HIP training step (CondGaussianDiffusion.hip_training)
against the plain-PyTorch fp32 path of the same module on the same GPU.

    python tools/train_step_bench.py --out profiles/train_step_bench.json                 T = 120, B = 32, 64, 128
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train_step_bench.py --only hip --batch 32 --rounds 1
                                                                                           (kernel shares: a run of its own)

Both paths are warmed at every shape, then timed in alternating rounds (hip, plain, hip, plain, ...) with device events around
`steps` whole steps each, so that a drift of the shared host hits both alike; the median round and the spread are reported.
The two paths draw the same t and noises; their dropout masks differ (torch's generator against in-kernel Philox).  A GPU is required:
there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import ModelConfig, make_weights, head_condition_mask  # noqa: E402
from egoego_release_amd.synthetic import make_motion_windows  # noqa: E402


def build(hip, T, seed=0):
    from egoego_release_amd.model import CondGaussianDiffusion
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(make_weights(cfg, seed), strict=False)
    m = m.cuda()
    m.hip_training = hip
    m.train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-4)


def run_steps(m, opt, data, mask, n):
    for i in range(n):
        loss = m(data, mask)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return loss


def timed(m, opt, data, mask, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run_steps(m, opt, data, mask, n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "plain"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench needs a ROCm GPU: timings are not taken on the CPU")
    T = args.window
    paths = [p for p in ("hip", "plain") if args.only in (None, p)]
    res = {"device": torch.cuda.get_device_name(0), "T": T, "steps_per_round": args.steps, "rounds": args.rounds, "what": "forward + backward + Adam.step(), ms per step",
           "batches": {}}
    for B in args.batch:
        data = make_motion_windows(B, T, seed=1, device="cuda")
        mask = head_condition_mask((B, T, 198), device="cuda")
        rigs = {p: build(p == "hip", T) for p in paths}
        torch.manual_seed(0)
        for p in paths:
            run_steps(*rigs[p], data, mask, args.warmup)
        times = {p: [] for p in paths}
        for _ in range(args.rounds):
            for p in paths:
                times[p].append(timed(*rigs[p], data, mask, args.steps))
        row = {p: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for p, v in times.items()}
        if len(paths) == 2:
            row["hip_over_plain"] = row["hip"]["median_ms"] / row["plain"]["median_ms"]
        res["batches"][str(B)] = row
        print(json.dumps({"B": B, **row}), flush=True)
        del rigs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
