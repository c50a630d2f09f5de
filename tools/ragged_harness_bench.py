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
to rounding only, and the chain carries that forward).  Prints one JSON line and writes it to --out.

    python tools/ragged_harness_bench.py --ddim_steps 50 [--ddim_eta 0.0] [--out profiles/ragged_harness_ddim_bench.json]

The same workload through the ragged call with sampler="ddim" (the strided sampler over --ddim_steps timesteps per window), next to
the ancestral ragged call of the same process.  The timed call is split into the seconds INSIDE the sampler calls (device time
between two events around every engine loop call) and the rest — the per-window glue: condition, conversion, prefix, stitching,
the host between the launches and the end-of-chain guard's read-back.  `parent_ragged_seconds` is the figure of the committed
profiles/ragged_harness_bench.json (the ancestral chain at the commit before the strided harness)."""
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
from egoego_release_amd.engine import HipEngine  # noqa: E402


class SamplerClock:
    """Device seconds inside HipEngine.sample_loop_ / ddim_loop_ while active: an event pair around every call, read after the
    timed call's final synchronisation."""

    def __init__(self):
        self.pairs = []

    def __enter__(self):
        self.saved = {n: getattr(HipEngine, n) for n in ("sample_loop_", "ddim_loop_")}
        for name, fn in self.saved.items():
            def timed(eng, *a, _fn=fn, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(eng, *a, **kw)
                e1.record()
                self.pairs.append((e0, e1))
                return out
            setattr(HipEngine, name, timed)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(HipEngine, name, fn)

    def seconds(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.pairs) * 1e-3


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
    ap.add_argument("--ddim_steps", type=int, default=0, help="N > 0: time the ragged call with the strided sampler over N timesteps per window")
    ap.add_argument("--ddim_eta", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="default: profiles/ragged_harness_bench.json, or ragged_harness_ddim_bench.json with --ddim_steps")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ragged_harness_ddim_bench.json" if a.ddim_steps else "ragged_harness_bench.json")
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

    frames = [int(p.shape[0]) for p in poses]
    windows = a.samples * sum(len(harness.window_spans(T, a.window)) for T in frames)
    table = harness.ragged_window_table(frames, a.window)
    if a.ddim_steps:
        return ddim_main(a, model, poses, draws, ragged, frames, windows, table, ds)
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
    res = {"device": torch.cuda.get_device_name(0), "sequences": a.sequences, "frames_min": min(frames), "frames_max": max(frames),
           "samples_per_sequence": a.samples, "window": a.window, "diffusion_steps": a.steps, "windows_total": windows,
           "windows_per_ragged_batch": [a.samples * len(e["sequences"]) for e in table], "weights": "make_weights(seed 0), random init",
           "precision": a.precision, "precision_used_ragged": prec_ragged, "precision_used_loop": prec_loop,
           "ragged_seconds": round(t_ragged, 3), "loop_seconds": round(t_loop, 3), "loop_over_ragged": round(t_loop / t_ragged, 2),
           "max_abs_root_diff": diff, "timing": "wall clock around one call after one untimed call of the same path"}
    emit(res, a.out)


def emit(res, out):
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def ddim_main(a, model, poses, draws, ragged, frames, windows, table, ds):
    def ragged_ddim():
        return harness.full_body_gen_cond_head_pose_sliding_window_ragged(model, ds, poses, samples_per_sequence=a.samples, noise=draws,
                                                                          sampler="ddim", n_steps=a.ddim_steps, eta=a.ddim_eta)

    def split(fn):
        fn()  # untimed: precision plan, captured graphs and workspaces
        with SamplerClock() as clock:
            res, total = wall(fn)
        return res, total, clock.seconds()

    (_, root_d, _), t_ddim, s_ddim = split(ragged_ddim)
    prec_ddim = model.hip_precision_used
    (_, root_a, _), t_anc, s_anc = split(ragged)
    prec_anc = model.hip_precision_used
    parent = None
    ref = os.path.join(ROOT, "profiles", "ragged_harness_bench.json")
    if os.path.exists(ref):
        with open(ref) as f:
            committed = json.loads(f.readline())
        same = all(committed.get(k) == v for k, v in (("sequences", a.sequences), ("samples_per_sequence", a.samples), ("window", a.window),
                                                      ("diffusion_steps", a.steps), ("windows_total", windows)))
        parent = committed["ragged_seconds"] if same else None
    ts = model.ddim_timesteps(a.ddim_steps)
    res = {"device": torch.cuda.get_device_name(0), "sequences": a.sequences, "frames_min": min(frames), "frames_max": max(frames),
           "samples_per_sequence": a.samples, "window": a.window, "windows_total": windows,
           "windows_per_ragged_batch": [a.samples * len(e["sequences"]) for e in table], "weights": "make_weights(seed 0), random init",
           "precision": a.precision, "precision_used_ddim": prec_ddim, "precision_used_ancestral": prec_anc,
           "ddim_steps": len(ts), "ddim_eta": a.ddim_eta, "ancestral_steps": a.steps,
           "ddim_seconds": round(t_ddim, 4), "ddim_sampler_seconds": round(s_ddim, 4), "ddim_glue_seconds": round(t_ddim - s_ddim, 4),
           "ddim_glue_share": round((t_ddim - s_ddim) / t_ddim, 3),
           "ancestral_seconds": round(t_anc, 4), "ancestral_sampler_seconds": round(s_anc, 4), "ancestral_glue_seconds": round(t_anc - s_anc, 4),
           "ancestral_over_ddim": round(t_anc / t_ddim, 2),
           "parent_ragged_seconds": parent, "parent_over_ddim": None if parent is None else round(parent / t_ddim, 2),
           "max_abs_root_diff_to_ancestral": float((root_d - root_a).abs().max()),
           "timing": "wall clock around one ragged call after one untimed call of the same path; sampler seconds: device time between "
                     "events around every engine loop call; glue = wall - sampler (condition, conversion, prefix, stitching, host, guard read-back); "
                     "parent_ragged_seconds: profiles/ragged_harness_bench.json (same workload, ancestral chain, the commit before)"}
    emit(res, a.out)


if __name__ == "__main__":
    main()
