#!/usr/bin/env python3
"""Evaluation timing: evaluate.evaluate_samples (FK, xy shift, floor heights and contacts, metrics, root to the floor, best
sample) for 256 samples x 139 frames and 256 x 2048 frames on libegoego_hip, against the reference's algorithm run per sample on
the host.

    python tools/eval_bench.py [--shapes 256x139,256x2048] [--iters 5] [--host-samples 4] [--out profiles/eval_bench.json]

Device times are CUDA events around one call, inputs already on the GPU: after one warm-up call of the same shape, --iters calls
are timed one by one; the median is reported with the smallest and largest next to it (nothing is pinned).  The motions are
synthetic.make_eval_motion walks: 8 distinct samples, repeated to fill the batch.

The host baseline is tests/eval_oracle.py, the fp64 numpy restatement of fk_smpl, determine_floor_height_and_contacts (its DBSCAN
a sorted-line pass with Python loops, not sklearn's) and compute_metrics_for_smpl, one sample at a time as eval_egoego.py:393-446
loops: --host-samples samples are timed with the wall clock and the per-sample mean is reported; `host_ms_batch_extrapolated`
is that mean times the batch, labelled as what it is.  Prints one JSON line per shape and writes everything to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from egoego_release_amd import evaluate, harness, synthetic  # noqa: E402
import eval_oracle as O  # noqa: E402

DISTINCT = 8


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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="256x139,256x2048")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup_calls": 1, "host_samples": a.host_samples,
           "host_baseline": "tests/eval_oracle.py per sample (fp64 numpy, Python-loop DBSCAN), wall clock", "shapes": []}
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        m = synthetic.make_eval_motion(DISTINCT, T, seed=1, check=False)
        rep = (B + DISTINCT - 1) // DISTINCT
        aa_np, root_np = np.tile(m["local_aa"], (rep, 1, 1, 1))[:B], np.tile(m["root_trans"], (rep, 1, 1))[:B]
        gq, gp = O.fk(m["gt_root_trans"], m["gt_local_aa"], m["rest_offsets"], m["parents"])
        gq, gp = gq.astype(np.float32), gp.astype(np.float32)
        ds = harness.SkeletonStats(np.zeros(66), np.ones(66), m["rest_offsets"], m["parents"])
        aa, root = torch.from_numpy(aa_np).to(dev), torch.from_numpy(root_np).to(dev)
        gq_d, gp_d = torch.from_numpy(gq).to(dev), torch.from_numpy(gp).to(dev)
        out = {}

        def call():
            out["r"] = evaluate.evaluate_samples(ds, aa, root, gq_d, gp_d)

        t_med, t_lo, t_hi = timed(call, a.iters)
        n_host = min(a.host_samples, B)
        t0 = time.perf_counter()
        want, floors, best = O.evaluate_samples(m["rest_offsets"], m["parents"], aa_np[:n_host], root_np[:n_host], gq, gp)
        host_ms = (time.perf_counter() - t0) * 1e3 / n_host
        got = out["r"]
        row = {"samples": B, "frames": T, "hip_ms": round(t_med, 3), "hip_ms_min": round(t_lo, 3), "hip_ms_max": round(t_hi, 3),
               "samples_per_s": round(B / t_med * 1e3), "host_ms_per_sample": round(host_ms, 2),
               "host_ms_batch_extrapolated": round(host_ms * B, 1), "ratio_extrapolated": round(host_ms * B / t_med, 1),
               "max_floor_diff_vs_host": float(np.abs(got["floor_height"][:n_host].cpu().numpy() - floors).max()),
               "max_rel_mpjpe_diff_vs_host": float(max(abs(float(got["metrics"]["mpjpe"][b]) - want[b]["mpjpe"]) / want[b]["mpjpe"]
                                                       for b in range(n_host)))}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
