#!/usr/bin/env python3
"""What the parameter update costs in stage-1 training, and what the fused clip + AdamW call (optim.FusedAdamW) saves.

    python tools/stage1_update_bench.py --out profiles/stage1_update_bench.json

Both nets at their real sizes (HeadNet window 90 x 2 layers, GravityNet window 120 x 2 layers), two measurements, each in one
process with alternating rounds (torch, fused, torch, fused, ...) and medians, because the nodes of a pool differ by several
percent:

  (a) the update alone on the module's own parameter list: torch's clip_grad_norm_ + AdamW.step + zero_grad(set_to_none=False)
      against one FusedAdamW.step with zero_grads (norm, clip, decay, Adam and the gradients' zeros), device events around
      `calls` calls.  After the first call both sides work on zero gradients; neither path's cost depends on the values.
  (b) a whole trainer.Stage1Trainer.step (forward, loss, backward, update) with fused_update off and on, at B = 32 and 128.

The baseline is torch's update, which is what Stage1Trainer does by default.  The byte floor of the update is 32 B per parameter:
the norm reads g; the update reads p, g, m, v and writes p, m, v and the zeros of g.  A GPU is required.
"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import optim, stage1  # noqa: E402
from egoego_release_amd.synthetic import make_stage1_train_batch  # noqa: E402
from egoego_release_amd.trainer import Stage1Trainer  # noqa: E402

SHAPES = {"headnet": (90, 2), "gravitynet": (120, 2)}  # the reference's defaults: window x layers
PEAK_TBS = 8.0  # the MI355X's HBM3E peak, for the byte floor's time


def module(kind):
    window, layers = SHAPES[kind]
    o = Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                  w_rotation=1.0, w_va=1.0, w_dist=1.0)
    cls = stage1.HeadFormer if kind == "headnet" else stage1.HeadNormalFormer
    return cls(o, torch.device("cuda")).cuda()


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def update_alone(kind, calls, rounds, warmup):
    sides = {}
    for name in ("torch", "fused"):
        m = module(kind)
        params = [p for p in m.parameters() if p.requires_grad]
        gen = torch.Generator(device="cuda").manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 0.1
        if name == "torch":
            opt = torch.optim.AdamW(params, lr=1e-4)

            def call(params=params, opt=opt):
                torch.nn.utils.clip_grad_norm_(params, 1.0, error_if_nonfinite=False)
                opt.step()
                opt.zero_grad(set_to_none=False)
        else:
            opt = optim.FusedAdamW(params, lr=1e-4, max_grad_norm=1.0, modules=(m,), zero_grads=True, skip_on="nonfinite")
            call = opt.step
        for _ in range(warmup):
            call()
        sides[name] = (call, m, opt)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, (call, _, _) in sides.items():
            times[name].append(events(call, calls) * 1e3)
    params = [p for p in sides["torch"][1].parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    row = {"tensors": len(params), "parameters": n, "byte_floor_bytes": 32 * n, "byte_floor_us_at_8_TB_s": 32 * n / (PEAK_TBS * 1e12) * 1e6,
           "torch_us": summary(times["torch"]), "fused_us": summary(times["fused"])}
    row["torch_over_fused"] = row["torch_us"]["median"] / row["fused_us"]["median"]
    return row


def whole_step(kind, B, steps, rounds, warmup):
    window, _ = SHAPES[kind]
    data = {k: v.cuda() for k, v in make_stage1_train_batch(kind, B, window, seed=1).items()}
    sides = {name: Stage1Trainer(module(kind), [], fused_update=name == "fused") for name in ("torch", "fused")}
    for tr in sides.values():
        for _ in range(warmup):
            tr.step(data)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, tr in sides.items():
            times[name].append(events(lambda tr=tr: tr.step(data), steps))
    row = {"torch_ms": summary(times["torch"]), "fused_ms": summary(times["fused"])}
    row["saved_us"] = (row["torch_ms"]["median"] - row["fused_ms"]["median"]) * 1e3
    row["torch_over_fused"] = row["torch_ms"]["median"] / row["fused_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", nargs="+", default=["headnet", "gravitynet"], choices=tuple(SHAPES))
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--calls", type=int, default=10, help="update calls (a) and trainer steps (b) per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage1_update_bench needs a ROCm GPU: timings are not taken on the CPU")
    res = {"device": torch.cuda.get_device_name(0), "calls_per_round": args.calls, "rounds": args.rounds,
           "what": {"update_alone": "clip_grad_norm_ + AdamW.step + zero_grad(set_to_none=False) against FusedAdamW.step(zero_grads), us per call",
                    "trainer_step": "Stage1Trainer.step with fused_update off (torch) and on (fused), ms per step, train() mode"},
           "update_alone": {}, "trainer_step": {}}
    for kind in args.kind:
        window, layers = SHAPES[kind]
        tag = f"{kind} window {window} x {layers} layers"
        res["update_alone"][tag] = update_alone(kind, args.calls, args.rounds, args.warmup)
        print(json.dumps({"update_alone": tag, **res["update_alone"][tag]}), flush=True)
        for B in args.batch:
            res["trainer_step"][f"{tag}, B = {B}"] = whole_step(kind, B, args.calls, args.rounds, args.warmup)
            print(json.dumps({"trainer_step": tag, "B": B, **res["trainer_step"][f"{tag}, B = {B}"]}), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
