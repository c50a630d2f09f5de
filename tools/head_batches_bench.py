#!/usr/bin/env python3
"""What HeadNet's training batches cost: D = 512 and (B, window) = (8, 60) (the reference's recipe), (32, 90) and (128, 90), seeded
sequences of window + 1 .. window + 400 frames with SLAM tracks.

  1. device time per batch of stage1_data.head_batch (egoego_s1_head_batch: one launch), device events, and the bytes per second
     it reaches against the copy's own byte count (every output byte written once and counted once more as read);
  2. the same batch from a torch restatement on the device: one index_select per table, the starts given;
  3. host time per batch of the reference's __getitem__ + default collate + upload restated over one .npy file per feature frame
     in a temporary tree (page cache warm), in ONE process; the reference runs 8 DataLoader workers, so the figure divided by 8 is
     reported as its best case;
  4. a Stage1Trainer HeadNet step (forward + loss + backward + clip + AdamW) over HeadBatches against the same step over a
     pre-built list of the same batches on the device (the existing path, the baseline).

Every pair is timed in alternating rounds after a warm-up; medians and the spread are reported.  A GPU is required.

    python tools/head_batches_bench.py --out profiles/head_batches_bench.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch
from torch.utils.data import default_collate

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import stage1, stage1_data  # noqa: E402
from egoego_release_amd.trainer import Stage1Trainer  # noqa: E402

D = 512
SHAPES = ((8, 60), (32, 90), (128, 90))


def make_sequences(n, window, seed):
    g = np.random.default_rng(seed)
    out = []
    for k in range(n):
        T = int(g.integers(window + 1, window + 401))
        q = g.normal(0.0, 1.0, (1, 4)) + np.cumsum(g.normal(0.0, 0.05, (T, 4)), 0)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        pose = np.concatenate([np.cumsum(g.normal(0.0, 0.02, (T, 3)), 0) + np.array([0.0, 0.0, 1.6]), q], 1).astype(np.float32)
        out.append({"seq_name": f"scene-{k:05d}", "head_qpos": pose, "head_vels": g.normal(0.0, 0.3, (T, 6)),
                    "of_feats": g.normal(size=(T - 1, D)).astype(np.float32),
                    "slam": np.concatenate([np.cumsum(g.normal(0.0, 0.05, (T, 3)), 0), q[::-1]], 1)})
    return out


def copy_bytes(B, W):
    """Bytes the kernel writes for full windows, and as many read: features, poses, velocities, the six SLAM arrays."""
    out = B * (W * D * 4 + (W + 1) * 7 * 4 + W * 6 * 4 + (W + 1) * (29 * 4 + 3 * 8)) + 3 * B * 4
    return 2 * out


def torch_batch(t, ids, starts, W):
    """The same select-and-copy from torch ops on the device, for given starts (full windows)."""
    off = t["offsets"].long()[ids.long()]
    rows = (off + starts)[:, None] + torch.arange(W + 1, device=ids.device)[None]
    frows = (off - ids + starts)[:, None] + torch.arange(W, device=ids.device)[None]
    srows = (t["slam_offsets"].long()[ids.long()] + starts)[:, None] + torch.arange(W + 1, device=ids.device)[None]
    B = ids.numel()
    s32 = t["slam32"].index_select(0, srows.reshape(-1)).reshape(B, W + 1, 29)
    return {"head_pose": t["pose"].index_select(0, rows.reshape(-1)).reshape(B, W + 1, 7),
            "head_vels": t["vels"].index_select(0, rows[:, :W].reshape(-1)).reshape(B, W, 6),
            "of": t["feats"].index_select(0, frows.reshape(-1)).reshape(B, W, D),
            "aligned_slam_trans": s32[..., :3].contiguous(), "aligned_slam_rot_quat": s32[..., 3:7].contiguous(),
            "aligned_slam_rot_mat": s32[..., 7:16].reshape(B, W + 1, 3, 3), "ori_slam_rot_quat": s32[..., 16:20].contiguous(),
            "ori_slam_rot_mat": s32[..., 20:].reshape(B, W + 1, 3, 3),
            "ori_slam_trans": t["slam_trans64"].index_select(0, srows.reshape(-1)).reshape(B, W + 1, 3)}


# ------------------------------------------------------------------------------------------------ the reference's item, restated
def write_feature_files(root, seqs):
    files = []
    for s in seqs:
        d = os.path.join(root, s["seq_name"])
        os.makedirs(d)
        fs = []
        for t, row in enumerate(s["of_feats"]):
            fs.append(os.path.join(d, f"{t:05d}.npy"))
            np.save(fs[-1], row)
        files.append(fs)
    return files


def reference_item(s, files, slam, W):
    """ares_headpose_dataset.py:270-333, op for op: a random window, one np.load per feature frame, the slices."""
    vels = s["head_vels"][:-1]
    t0 = random.sample(list(range(vels.shape[0] - W + 1)), 1)[0]
    t1 = t0 + W
    q = {"head_pose": s["head_qpos"][t0:t1 + 1], "head_vels": vels[t0:t1], "of": np.stack([np.load(f) for f in files[t0:t1]]),
         "seq_name": s["seq_name"], "seq_len": W}
    for k, v in slam.items():
        q[k] = v[t0:t1 + 1]
    return q


def host_batch_ms(seqs, files, slams, ks, W, dev):
    t0 = time.perf_counter()
    batch = default_collate([reference_item(seqs[k], files[k], slams[k], W) for k in ks])
    batch = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ------------------------------------------------------------------------------------------------ the device side
def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def epoch_ms(tr, batches, limit):
    """tr.step over the first `limit` of `batches` (a HeadBatches builds each batch on the way) -> ms per step, device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    n = 0
    for batch in batches:
        tr.step(batch)
        n += 1
        if n == limit:
            break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="batches per epoch / launches per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host_rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_batches_bench needs a ROCm GPU: timings are not taken on the CPU")
    res = {"device": torch.cuda.get_device_name(0), "D": D, "steps_per_round": args.steps, "rounds": args.rounds,
           "frames": "window + 1 .. window + 400 per sequence, seeded", "reference_workers": 8, "cases": {}}
    rigs = {}
    for B, W in SHAPES:
        seqs = make_sequences(B * args.steps, W, seed=B)
        hb = stage1_data.HeadBatches(seqs, B, window=W, seed=1)
        ids = torch.arange(B, dtype=torch.int32, device=hb.device)
        draws = torch.arange(B, dtype=torch.int64, device=hb.device)
        build = lambda hb=hb, ids=ids, draws=draws, W=W: stage1_data.head_batch(hb.tables, ids, draws, W, 1)  # noqa: E731
        starts = build()["start_t_idx"].long()
        restated = lambda hb=hb, ids=ids, starts=starts, W=W: torch_batch(hb.tables, ids, starts, W)  # noqa: E731
        got, want = build(), restated()
        assert all(torch.equal(got[k], want[k]) for k in want), "the torch restatement builds another batch"
        opt = Namespace(window=W, n_dec_layers=2, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                        w_rotation=1.0, w_va=1.0, w_dist=1.0)
        torch.manual_seed(0)
        model = stage1.HeadFormer(opt, torch.device("cuda")).cuda()
        tr = Stage1Trainer(model, hb, save_dir=os.devnull)
        prebuilt = [{k: v for k, v in b.items() if k in ("of", "head_pose", "head_vels", "seq_len")} for b in hb]
        for _ in range(2):  # warm-up: both ways of feeding the step, and the two builds alone
            epoch_ms(tr, prebuilt, 3)
            events(build, 3)
            events(restated, 3)
        epoch_ms(tr, hb, args.steps)
        rigs[(B, W)] = (seqs, hb, build, restated, tr, prebuilt)
    names = ("build", "torch_restatement_on_device", "step_over_head_batches", "step_over_prebuilt_list")
    times = {k: {n: [] for n in names} for k in rigs}
    for _ in range(args.rounds):  # alternating: every quantity of every shape once per round
        for key, (seqs, hb, build, restated, tr, prebuilt) in rigs.items():
            times[key]["build"].append(events(build, args.steps))
            times[key]["torch_restatement_on_device"].append(events(restated, args.steps))
            times[key]["step_over_head_batches"].append(epoch_ms(tr, hb, args.steps))
            times[key]["step_over_prebuilt_list"].append(epoch_ms(tr, prebuilt, args.steps))
    for (B, W), (seqs, hb, *_rest) in rigs.items():
        row = {k: summary(v) for k, v in times[(B, W)].items()}
        row["copy_bytes"] = copy_bytes(B, W)
        row["build_gb_per_s"] = row["copy_bytes"] / (row["build"]["median_ms"] * 1e-3) / 1e9
        by = {s["seq_name"]: s for s in seqs}
        picked = [by[n] for n in hb.names[:B * (args.host_rounds + 1)]]
        slams = []
        for s in picked:
            at, ar, aq = stage1.load_slam_res_and_align_first(s["slam"], s["head_qpos"])
            ot, orot, oq = stage1.load_slam(s["slam"])
            slams.append({"aligned_slam_trans": at, "aligned_slam_rot_quat": aq, "aligned_slam_rot_mat": ar, "ori_slam_trans": ot,
                          "ori_slam_rot_quat": oq, "ori_slam_rot_mat": orot})
        with tempfile.TemporaryDirectory() as root:
            files = write_feature_files(root, picked)
            random.seed(1)
            host_batch_ms(picked, files, slams, range(B), W, hb.device)  # (warm: the files of every later batch are in the page cache too)
            host = [host_batch_ms(picked, files, slams, range(k * B, (k + 1) * B), W, hb.device) for k in range(1, args.host_rounds + 1)]
        row["reference_host_one_process"] = summary(host)
        row["reference_host_over_8_workers_ms"] = row["reference_host_one_process"]["median_ms"] / 8
        live, pre = row["step_over_head_batches"], row["step_over_prebuilt_list"]
        row["build_share_of_step"] = (live["median_ms"] - pre["median_ms"]) / pre["median_ms"]
        row["step_difference_ms"] = live["median_ms"] - pre["median_ms"]
        row["step_spread_ms"] = max(live["max_ms"] - live["min_ms"], pre["max_ms"] - pre["min_ms"])
        row["host_threads"] = torch.get_num_threads()
        res["cases"][f"B = {B}, window = {W}"] = row
        print(json.dumps({"B": B, "window": W, **row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
