#!/usr/bin/env python3
"""Ragged stage 1 against the loop of one-sequence calls: 64 sequences of 40..400 feature frames through
estimate_head_pose(..., lengths=) in one call, and through the existing equal-length estimate_head_pose one sequence at a time,
on the same GPU in the same process, in the demo shapes (HeadNet 60 x 2, GravityNet 120 x 2) and the default shapes (90 x 2,
90 x 4).

    python tools/stage1_ragged_bench.py [--rounds 15] [--out profiles/stage1_ragged_bench.json]
    python tools/stage1_ragged_bench.py --only ragged --shapes demo --rounds 5      (for a kernel trace of the ragged call alone)

Inputs are device tensors (the loop's per-sequence slices are cut before timing).  Each round times the ragged call and then the
loop (alternating, after two warm-up rounds) with a pair of device events around the whole call and with the host clock after a
device synchronisation; the medians over the rounds are reported.  The one-sequence path copies the normal and the trajectory to
the host for its numpy steps, so its event time includes those waits; the ragged call has none.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import rotations, stage1, synthetic  # noqa: E402

SHAPES = {"demo": dict(window=60, n_dec_layers=2, normal_window=120, normal_n_dec_layers=2),
          "default": dict(window=90, n_dec_layers=2, normal_window=90, normal_n_dec_layers=4)}
N_SEQ, T_MIN, T_MAX = 64, 40, 400


def nets(s, dev):
    opt = Namespace(window=s["window"], n_dec_layers=s["n_dec_layers"], n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0,
                    input_of_feats=True, normal_window=s["normal_window"], normal_n_dec_layers=s["normal_n_dec_layers"],
                    normal_n_head=4, normal_d_k=256, normal_d_v=256, normal_d_model=256)
    hn = stage1.HeadFormer(opt, dev)
    hn.load_state_dict(synthetic.make_stage1_weights("headnet", hn.cfg, 1))
    gn = stage1.HeadNormalFormer(opt, dev, eval_whole_pipeline=True)
    gn.load_state_dict(synthetic.make_stage1_weights("gravitynet", gn.cfg, 2))
    return hn, gn


def make_batch(dev):
    g = torch.Generator().manual_seed(0)
    T = torch.linspace(T_MIN, T_MAX, N_SEQ).round().long()
    T = T[torch.randperm(N_SEQ, generator=g)].tolist()
    Tm, Lm = max(T), max(T) + 1
    q = torch.randn(N_SEQ, Lm, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    hp = torch.cat((torch.cumsum(torch.randn(N_SEQ, Lm, 3, generator=g) * 0.02, 1), rotations.standardize_quaternion(q)), -1)
    rq = torch.randn(N_SEQ, Lm, 4, generator=g)
    batch = {"of": torch.randn(N_SEQ, Tm, 512, generator=g), "head_pose": hp,
             "aligned_slam_trans": torch.cumsum(torch.randn(N_SEQ, Lm, 3, generator=g) * 0.03, 1),
             "ori_slam_trans": torch.cumsum(torch.randn(N_SEQ, Lm, 3, generator=g) * 0.03, 1),
             "ori_slam_rot_mat": rotations.quaternion_to_matrix(rq / rq.norm(dim=-1, keepdim=True))}
    batch = {k: v.to(dev) for k, v in batch.items()}
    singles = [{k: (v[b:b + 1, :T[b]] if k == "of" else v[b:b + 1, :T[b] + 1]).contiguous() for k, v in batch.items()}
               for b in range(N_SEQ)]
    return T, batch, singles


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--shapes", default="demo,default")
    ap.add_argument("--only", default="", choices=["", "ragged", "loop"])
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    T, batch, singles = make_batch(dev)
    rows = []
    for tag in opt.shapes.split(","):
        hn, gn = nets(SHAPES[tag], dev)

        def ragged():
            return stage1.estimate_head_pose(hn, gn, batch, lengths=T)[0]

        def loop():
            return [stage1.estimate_head_pose(hn, gn, s)[0] for s in singles]

        with torch.no_grad():
            times = {"ragged": [], "loop": []}
            for r in range(opt.rounds + 2):
                for name, fn in (("ragged", ragged), ("loop", loop)):
                    if opt.only in ("", name):
                        t = timed(fn)
                        if r >= 2:
                            times[name].append(t)
            row = {"shapes": tag, **SHAPES[tag], "rounds": opt.rounds}
            for name, ts in times.items():
                if ts:
                    row[name + "_event_ms"] = float(np.median([t[0] for t in ts]))
                    row[name + "_host_ms"] = float(np.median([t[1] for t in ts]))
            if not opt.only:
                hp, one = ragged(), loop()
                row["max_abs_pose_difference"] = max(float((hp[b, :T[b] + 1] - one[b][0]).abs().max()) for b in range(N_SEQ))
                row["speedup_event"] = row["loop_event_ms"] / row["ragged_event_ms"]
                row["speedup_host"] = row["loop_host_ms"] / row["ragged_host_ms"]
        rows.append(row)
    res = {"workload": f"stage 1, {N_SEQ} sequences of {T_MIN}..{T_MAX} feature frames ({sum(T)} in all): estimate_head_pose(lengths=) "
                       f"in one call against {N_SEQ} one-sequence calls", "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(res)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
