#!/usr/bin/env python3
"""What GravityNet's training batches cost: window 120, B = 32 and 128, seeded sequences of 200..2000 frames.

  1. device time per batch of stage1_data.gravity_batch (egoego_s1_gravity_batch: one launch), device events;
  2. host time per batch of a torch restatement of the reference's AMASSHeadPoseDataset.__getitem__ (its Python loop of `window`
     torch.cat-appended adds included) plus the default collate, in ONE process; the reference runs 8 DataLoader workers, so the
     figure divided by 8 is reported as its best case;
  3. a Stage1Trainer GravityNet step (forward + loss + backward + clip + AdamW) over GravityBatches against the same step over a
     pre-built list of the same batches.

Every pair is timed in alternating rounds after a warm-up; medians and the spread are reported.  A GPU is required.

    python tools/stage1_data_bench.py --out profiles/stage1_data_bench.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch
from torch.utils.data import default_collate

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import rotations, stage1, stage1_data  # noqa: E402
from egoego_release_amd.trainer import Stage1Trainer  # noqa: E402

WINDOW = 120


def make_sequences(n, seed):
    g = np.random.default_rng(seed)
    out = {}
    for k in range(n):
        T = int(g.integers(200, 2001))
        trans = np.cumsum(g.normal(0.0, 0.02, (T, 3)), 0) + np.array([0.0, 0.0, 1.6])
        q = g.normal(0.0, 1.0, (1, 4)) + np.cumsum(g.normal(0.0, 0.05, (T, 4)), 0)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        out[f"CMU-{k:05d}"] = np.concatenate([trans, q], 1).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the reference's item, restated
def reference_item(pose, window):
    """amass_headpose_dataset.py:115-165 with augment_traj, op for op, on one [T, 7] numpy array."""
    seq = torch.from_numpy(pose).float()
    n = seq.shape[0]
    if n - window - 1 <= 0:
        t0, t1 = 0, n
    else:
        t0 = random.sample(list(range(n - window - 1)), 1)[0]
        t1 = t0 + window + 1
    win = seq[t0:t1]
    rot = rotations.quaternion_to_matrix(win[:, 3:])
    o = torch.randn((1, 4))
    q = o / torch.where(o[:, 0] < 0, -torch.sqrt((o * o).sum(1)), torch.sqrt((o * o).sum(1)))[:, None]
    rr = rotations.quaternion_to_matrix(q)
    aug_rot = torch.matmul(rr, rot)
    cur = win[:, :3] - win[0:1, :3]
    aug_trans = torch.matmul(rr, cur[:, :, None])[:, :, 0]
    normal = torch.matmul(rr[0], torch.from_numpy(np.asarray([0, 0, 1])).float()[:, None])
    scale = np.random.uniform(low=0.1, high=10, size=(1))[0]
    diff = (aug_trans[1:] - aug_trans[:-1]) * scale
    acc = [aug_trans[0:1]]
    for t in range(aug_trans.shape[0] - 1):
        acc.append(acc[-1] + diff[t:t + 1])
    aug_trans = torch.cat(acc, dim=0)
    m = win.shape[0]
    if m < window + 1:
        win = torch.cat((win, torch.zeros(window + 1 - m, 7)), dim=0)
        aug_rot = torch.cat((aug_rot, torch.zeros(window + 1 - m, 3, 3)), dim=0)
        aug_trans = torch.cat((aug_trans, torch.zeros(window + 1 - m, 3)), dim=0)
    return {"ori_head_pose": win, "head_rot_mat": aug_rot, "head_trans": aug_trans, "seq_len": m, "aligned_rot_mat": rr[0].T,
            "aligned_scale": 1.0 / scale, "floor_normal": normal}


def host_batch_ms(poses, names, B):
    t0 = time.perf_counter()
    default_collate([reference_item(poses[n], WINDOW) for n in names[:B]])
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


def epoch_ms(tr, batches):
    """One pass of tr.step over `batches` (a GravityBatches builds each batch on the way) -> ms per step, device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    n = 0
    for batch in batches:
        tr.step(batch)
        n += 1
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--steps", type=int, default=10, help="batches per epoch / launches per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host_rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage1_data_bench needs a ROCm GPU: timings are not taken on the CPU")
    res = {"device": torch.cuda.get_device_name(0), "window": WINDOW, "steps_per_round": args.steps, "rounds": args.rounds,
           "frames": "200..2000 per sequence, seeded", "reference_workers": 8, "cases": {}}
    opt = Namespace(window=WINDOW, n_dec_layers=2, n_head=4, d_k=256, d_v=256, d_model=256)
    rigs = {}
    for B in args.batch:
        poses = make_sequences(B * args.steps, seed=B)
        gb = stage1_data.GravityBatches(poses, B, window=WINDOW, seed=1)
        ids = torch.arange(B, dtype=torch.int32, device=gb.device)
        draws = torch.arange(B, dtype=torch.int64, device=gb.device)
        build = lambda gb=gb, ids=ids, draws=draws: stage1_data.gravity_batch(gb.pose, gb.offsets, ids, draws, WINDOW, 1)  # noqa: E731
        torch.manual_seed(0)
        model = stage1.HeadNormalFormer(opt, torch.device("cuda")).cuda()
        tr = Stage1Trainer(model, gb, save_dir=os.devnull)
        prebuilt = [{k: v for k, v in b.items() if k != "lengths"} for b in gb]  # the parent's way: a list of reference-format dicts
        for _ in range(2):  # warm-up: both ways of feeding the step, and the launch alone
            epoch_ms(tr, prebuilt[:3])
            events(build, 3)
        epoch_ms(tr, gb)
        rigs[B] = (poses, gb, build, tr, prebuilt)
    times = {B: {"build": [], "step_over_gravity_batches": [], "step_over_prebuilt_list": []} for B in args.batch}
    for _ in range(args.rounds):  # alternating: every quantity of every batch size once per round
        for B in args.batch:
            poses, gb, build, tr, prebuilt = rigs[B]
            times[B]["build"].append(events(build, args.steps))
            times[B]["step_over_gravity_batches"].append(epoch_ms(tr, gb))
            times[B]["step_over_prebuilt_list"].append(epoch_ms(tr, prebuilt))
    for B in args.batch:
        poses = rigs[B][0]
        names = list(poses)
        random.seed(1)
        np.random.seed(2)
        torch.manual_seed(3)
        host_batch_ms(poses, names, B)
        host = [host_batch_ms(poses, names[k * B:], B) for k in range(args.host_rounds)]
        row = {k: summary(v) for k, v in times[B].items()}
        row["reference_host_one_process"] = summary(host)
        row["reference_host_over_8_workers_ms"] = row["reference_host_one_process"]["median_ms"] / 8
        live, pre = row["step_over_gravity_batches"]["median_ms"], row["step_over_prebuilt_list"]["median_ms"]
        row["build_share_of_step"] = (live - pre) / pre
        row["host_threads"] = torch.get_num_threads()
        res["cases"][f"B = {B}"] = row
        print(json.dumps({"B": B, **row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
