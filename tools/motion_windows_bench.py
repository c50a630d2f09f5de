#!/usr/bin/env python3
"""Motion-window timing: motion_data.build_motion_windows + .stats() + .motion() on libegoego_hip for seeded random-walk motion
at two sizes, one of them AMASS-like in window count, next to the per-window cost of the test oracle on the host.

    python tools/motion_windows_bench.py [--shapes 64x300,8000x300] [--iters 5] [--host-windows 4] [--out profiles/motion_windows_bench.json]

A shape is sequences x frames; at window 120 a 300-frame sequence gives 5 windows.  Device times are CUDA events around one call
(host arrays in, device tensors out: the upload of the raw motion is inside): after one warm-up call of the same shape, --iters
calls are timed one by one; the median is reported with the smallest and largest next to it (nothing is pinned).  16 distinct
sequences are repeated to fill the batch.

The host column is tests/windows_oracle.py (fp64 numpy) on --host-windows windows, wall clock, per window; the reference handles
one window at a time in the same way (a dozen small torch launches and a numpy detour each).  `host_ms_all_windows_product` is
that mean TIMES the window count: a product, not a measurement.  Prints one JSON line per shape and writes everything to --out."""
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
from egoego_release_amd import motion_data as MD, synthetic  # noqa: E402
import windows_oracle as WO  # noqa: E402

DISTINCT = 16


def random_walk(n_seq, frames, seed=0):
    g = np.random.default_rng([seed, 0x3D0])
    trans = np.cumsum(g.standard_normal((n_seq, frames, 3)) * 0.01, 1) + np.array([0.0, 0.0, 0.9])
    root = np.cumsum(g.standard_normal((n_seq, frames, 3)) * 0.01, 1) + g.standard_normal((n_seq, 1, 3)) * 0.3
    body = np.cumsum(g.standard_normal((n_seq, frames, 63)) * 0.005, 1) + g.standard_normal((n_seq, 1, 63)) * 0.2
    return trans.astype(np.float32), root.astype(np.float32), body.astype(np.float32)


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
    ap.add_argument("--shapes", default="64x300,8000x300")
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-windows", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_windows_bench.json"))
    a = ap.parse_args()
    rest = synthetic.EVAL_REST_OFFSETS
    res = {"device": torch.cuda.get_device_name(0), "window": a.window, "iters": a.iters, "warmup_calls": 1, "host_windows": a.host_windows,
           "host_baseline": "tests/windows_oracle.py per window (fp64 numpy), wall clock",
           "note": "host_ms_all_windows_product = host_ms_per_window x windows: a product, not a measurement", "shapes": []}
    for shape in a.shapes.split(","):
        S, T = (int(v) for v in shape.split("x"))
        t, r, b = random_walk(DISTINCT, T)
        rep = (S + DISTINCT - 1) // DISTINCT
        seqs = tuple(np.tile(x, (rep, 1, 1))[:S].reshape(S * T, -1) for x in (t, r, b)) + ([T] * S,)
        out = {}

        def call():
            mw = MD.build_motion_windows(seqs, rest, window=a.window)
            mw._stats = None
            out["mw"], out["stats"], out["motion"] = mw, mw.stats(), mw.motion()

        t_med, t_lo, t_hi = timed(call, a.iters)
        mw = out["mw"]
        N = len(mw)
        n_host = min(a.host_windows, N)
        t0 = time.perf_counter()
        for i in range(n_host):
            k, s, n = int(mw.seq_index[i]), int(mw.start_t_idx[i]), int(mw.length[i])
            w = WO.process_window(t[k % DISTINCT, s:s + n], r[k % DISTINCT, s:s + n], b[k % DISTINCT, s:s + n], rest)
            d = float(np.abs(mw.global_jpos[i, :n].cpu().numpy() - w["global_jpos"]).max())
        host_ms = (time.perf_counter() - t0) * 1e3 / n_host
        row = {"sequences": S, "frames": T, "windows": N, "hip_ms": round(t_med, 3), "hip_ms_min": round(t_lo, 3), "hip_ms_max": round(t_hi, 3),
               "windows_per_s": round(N / t_med * 1e3), "host_ms_per_window": round(host_ms, 2),
               "host_ms_all_windows_product": round(host_ms * N, 1), "ratio_product": round(host_ms * N / t_med, 1),
               "max_jpos_diff_vs_host_last_window": d}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del out, mw
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
