#!/usr/bin/env python3
"""Ragged sliding-window timing: a seeded set of head trajectories of different lengths sampled (a) by ONE call of
harness.full_body_gen_cond_head_pose_sliding_window_ragged — every window index runs once, as one ragged batch over all
sequences — and (b) by the loop it replaces, one harness.full_body_gen_cond_head_pose_sliding_window call per sequence
(samples_per_sequence windows per step, what eval_egoego.py:358-446 does with sample_bs).

    python tools/ragged_harness_bench.py [--sequences 64] [--min-frames 40] [--max-frames 400] [--samples 4] [--window 120]
                                         [--steps 1000] [--precision auto] [--out profiles/ragged_harness_bench.json]

Random-init weights (make_weights, seed 0), in-kernel Philox noise in both paths, x_T and the condition noise injected so that both
sample the same chains; sequence s of the loop gets window_offset = s * samples, the ids the ragged call gives its pairs.  Each
path runs once untimed (precision plan, captured graphs and workspaces are then in place) and once timed with the wall clock around
a device synchronisation.  `max_abs_root_diff` compares the two results: a sequence's full windows are the same bits in both, its
short last window runs padded to the window length in the ragged call and at its own length in the loop (other kernels, so equal
to rounding only, and the chain carries that forward).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egoego_release_amd import ModelConfig, harness, make_weights  # noqa: E402


def make_sequences(n, lo, hi, seed):
    """n head trajectories [T, 7] with lengths spread evenly over lo..hi (shuffled): a slow random walk at head height and smoothly
    turning unit quaternions (w >= 0)."""
    rng = np.random.default_rng(seed)
    frames = np.linspace(lo, hi, n).round().astype(int)
    rng.shuffle(frames)
    out = []
    for T in frames:
        pos = np.cumsum(rng.standard_normal((T, 3)) * 0.01, 0) + np.array([0.0, 0.0, 1.5])
        q = np.cumsum(rng.standard_normal((T, 4)) * 0.02, 0) + np.array([1.0, 0.0, 0.0, 0.0])
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        q = np.where(q[:, :1] < 0, -q, q)
        out.append(torch.from_numpy(np.concatenate([pos, q], -1)).float())
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--min-frames", type=int, default=40)
    ap.add_argument("--max-frames", type=int, default=400)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--precision", default="auto")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_harness_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = harness.build_stage2_model(window=a.window)
    model.load_state_dict(make_weights(ModelConfig(max_timesteps=a.window + 1), 0), strict=False)
    model = model.to(dev)
    model.num_timesteps = a.steps
    model.sampling_rng = "philox"
    model.philox_seed = a.seed
    model.hip_precision = a.precision if a.precision == "auto" else int(a.precision)
    rng = np.random.default_rng(1)
    rest = rng.uniform(-0.2, 0.2, (22, 3))
    rest[0] = 0
    ds = harness.SkeletonStats(rng.uniform(-2.0, -1.0, (22, 3)), rng.uniform(1.0, 2.0, (22, 3)), rest)
    poses = [p.to(dev) for p in make_sequences(a.sequences, a.min_frames, a.max_frames, a.seed)]
    g = torch.Generator().manual_seed(a.seed)
    draws = []
    for p in poses:
        T = int(p.shape[0])
        draws.append({"x_all": torch.randn(a.samples, T, 198, generator=g),
                      "cond": [torch.randn(a.samples, n, 198, generator=g) for _, n in harness.window_spans(T, a.window)]})

    def ragged():
        return harness.full_body_gen_cond_head_pose_sliding_window_ragged(model, ds, poses, samples_per_sequence=a.samples, noise=draws)

    def loop():
        res = []
        for s, p in enumerate(poses):
            hp = p[None].repeat_interleave(a.samples, 0)
            res.append(harness.full_body_gen_cond_head_pose_sliding_window(model, ds, hp, noise=draws[s], window_offset=s * a.samples))
        return res

    ragged()
    (aa, root, out_len), t_ragged = wall(ragged)
    prec_ragged = model.hip_precision_used
    loop()
    per_seq, t_loop = wall(loop)
    prec_loop = model.hip_precision_used
    diff = 0.0
    for s, (_, r) in enumerate(per_seq):
        n = int(out_len[s * a.samples])
        assert r.shape[1] == n
        diff = max(diff, float((root[s * a.samples:(s + 1) * a.samples, :n] - r).abs().max()))
    frames = [int(p.shape[0]) for p in poses]
    windows = a.samples * sum(len(harness.window_spans(T, a.window)) for T in frames)
    table = harness.ragged_window_table(frames, a.window)
    res = {"device": torch.cuda.get_device_name(0), "sequences": a.sequences, "frames_min": min(frames), "frames_max": max(frames),
           "samples_per_sequence": a.samples, "window": a.window, "diffusion_steps": a.steps, "windows_total": windows,
           "windows_per_ragged_batch": [a.samples * len(e["sequences"]) for e in table], "weights": "make_weights(seed 0), random init",
           "precision": a.precision, "precision_used_ragged": prec_ragged, "precision_used_loop": prec_loop,
           "ragged_seconds": round(t_ragged, 3), "loop_seconds": round(t_loop, 3), "loop_over_ragged": round(t_loop / t_ragged, 2),
           "max_abs_root_diff": diff, "timing": "wall clock around one call after one untimed call of the same path"}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
