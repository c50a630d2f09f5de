#!/usr/bin/env python3
"""Time the stage-2 parameter update — the fused HIP call (optim.FusedAdam + optim.EMA) against torch.optim.Adam's default device
path plus `_foreach` EMA ops plus zero_grad(set_to_none=False) — and the whole training iteration around it.

    python tools/optim_step_bench.py --out profiles/optim_step_bench.json

The method of tools/train_step_bench.py: both sides are warmed, then timed in alternating rounds with device events around `steps`
calls each; the median round and the spread are reported.  Two parts, both at the stage-2 model's parameter list:
    update     the update alone, on fixed gradients: fused with the EMA written every call, fused without an EMA, and torch's
    iteration  Stage2Trainer: two micro-batches at B=32, T=120, hip_training on and off; fused=True, host_check=50 against
               fused=False, host_check=1
A GPU is required: there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import ModelConfig, make_weights  # noqa: E402
from egoego_release_amd.synthetic import make_motion_windows  # noqa: E402

HBM_TBPS = 6.3  # the ceiling the byte floors are quoted against


def build_model(T, hip=False, seed=0):
    from egoego_release_amd.model import CondGaussianDiffusion
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(make_weights(cfg, seed), strict=False)
    m = m.cuda()
    m.hip_training = hip
    m.train()
    return m


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def rounds(sides, steps, n_rounds, warmup):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(n_rounds):
        for k, fn in sides.items():
            times[k].append(timed(fn, steps))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def fill_grads(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        if p.requires_grad:
            p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3


def bench_update(T, steps, n_rounds, warmup):
    from egoego_release_amd.optim import EMA, FusedAdam
    sides = {}
    # fused, the EMA written on every call (update_every = 1, past the warm-up: a lerp each time), gradients cleared
    m1 = build_model(T)
    fill_grads(m1, 1)
    ema1 = EMA(m1, beta=0.995, update_every=1, update_after_step=0)
    opt1 = FusedAdam(m1.parameters(), lr=1e-4, zero_grads=True)
    sides["fused_ema"] = lambda: opt1.step(ema=ema1)
    m2 = build_model(T)
    fill_grads(m2, 1)
    opt2 = FusedAdam(m2.parameters(), lr=1e-4, zero_grads=True)
    sides["fused"] = lambda: opt2.step()
    # torch: Adam's default device path, the EMA as three _foreach ops over the trainable tensors, zero_grad in place
    m3 = build_model(T)
    fill_grads(m3, 1)
    opt3 = torch.optim.Adam(m3.parameters(), lr=1e-4)
    online = [p.data for p in m3.parameters() if p.requires_grad]
    shadow = [p.clone() for p in online]

    def torch_ema():
        opt3.step()
        d = torch._foreach_sub(shadow, online)
        torch._foreach_mul_(d, 1.0 - 0.995)
        torch._foreach_sub_(shadow, d)
        opt3.zero_grad(set_to_none=False)

    def torch_plain():
        opt3.step()
        opt3.zero_grad(set_to_none=False)

    sides["torch_ema"] = torch_ema
    sides["torch"] = torch_plain
    res = rounds(sides, steps, n_rounds, warmup)
    n = sum(p.numel() for p in m1.parameters() if p.requires_grad)
    res["n_values"] = n
    res["floor_us"] = {"norm": 4 * n / (HBM_TBPS * 1e6), "apply_adam_zero": 4 * n * 8 / (HBM_TBPS * 1e6),
                       "apply_adam_zero_ema": 4 * n * 10 / (HBM_TBPS * 1e6)}
    res["fused_ema_over_torch_ema"] = res["fused_ema"]["median_ms"] / res["torch_ema"]["median_ms"]
    res["fused_over_torch"] = res["fused"]["median_ms"] / res["torch"]["median_ms"]
    return res


def bench_iteration(T, B, steps, n_rounds, warmup, hip):
    from egoego_release_amd.trainer import Stage2Trainer
    data = make_motion_windows(4 * B, T, seed=1, device="cuda")
    batches = [{"motion": data[i * B:(i + 1) * B], "seq_len": torch.full((B,), T)} for i in range(4)]
    tmp = tempfile.mkdtemp(prefix="optim_step_bench_")
    rigs = {"fused_check50": Stage2Trainer(build_model(T, hip), batches, fused=True, host_check=50, results_folder=tmp),
            "plain_check1": Stage2Trainer(build_model(T, hip), batches, fused=False, host_check=1, results_folder=tmp)}
    torch.manual_seed(0)
    res = rounds({k: (lambda t=t: t.train(1)) for k, t in rigs.items()}, steps, n_rounds, warmup)
    res["fused_over_plain"] = res["fused_check50"]["median_ms"] / res["plain_check1"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("update", "iteration"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench needs a ROCm GPU: timings are not taken on the CPU")
    res = {"device": torch.cuda.get_device_name(0), "T": args.window, "B": args.batch, "steps_per_round": args.steps, "rounds": args.rounds,
           "what": "ms per call (update) / per iteration of two micro-batches (iteration); medians of the rounds"}
    if args.only in (None, "update"):
        res["update"] = bench_update(args.window, args.steps, args.rounds, args.warmup)
        print(json.dumps({"update": res["update"]}), flush=True)
    if args.only in (None, "iteration"):
        res["iteration"] = {}
        for hip in (False, True):
            key = "hip_training" if hip else "plain_loss"
            res["iteration"][key] = bench_iteration(args.window, args.batch, args.steps, args.rounds, args.warmup, hip)
            print(json.dumps({key: res["iteration"][key]}), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
