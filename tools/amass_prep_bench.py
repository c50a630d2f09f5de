#!/usr/bin/env python3
"""AMASS preprocessing timing: amass_prep's three stages (body_joints, floor_and_contacts, head_tracks) on packed sequences on
libegoego_hip, against the same steps run per sequence on the host.

    python tools/amass_prep_bench.py [--shapes 64x1500,8x12000,1x80000] [--fps 120] [--iters 5] [--host-sequences 1] \\
        [--out profiles/amass_prep_bench.json]

A shape BxT is B sequences of T raw frames (synthetic.make_eval_motion walks, 4 distinct ones repeated) at --fps; the middle 80 %
is processed, as process_seq trims.  Up to 4096 trimmed frames a sequence runs the floor kernel's LDS path, beyond that its
workspace path.  Device times are CUDA events around the three stage calls, the poses already on the GPU (the calls upload their
small host tables: offsets, thresholds, the downsample table): after one warm-up call of the same shape, --iters calls are timed
one by one; the median is reported with the smallest and largest next to it (nothing is pinned).  `process_sequences_ms` is
one wall-clock call of the whole driver, host arrays in, records out, copies included.

The host baseline is tests/amass_oracle.py per sequence, wall clock: an fp64 numpy restatement of process_seq (the 22 joints
through tests/body_oracle.py on a 64-vertex synthetic model, the DBSCAN a sorted-line pass with Python loops, the head
velocities a Python loop over frames).  It is NOT the reference's path, which runs a 6890-vertex SMPL-H forward and sklearn:
--host-sequences sequences are timed and the per-sequence mean is reported; `host_ms_batch_extrapolated` is that mean times
the batch, labelled as what it is.  Prints one JSON line per shape and writes everything to --out."""
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
from egoego_release_amd import amass_prep as A, synthetic  # noqa: E402
import amass_oracle as O  # noqa: E402

DISTINCT = 4


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
    ap.add_argument("--shapes", default="64x1500,8x12000,1x80000")
    ap.add_argument("--fps", type=float, default=120.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-sequences", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amass_prep_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = synthetic.make_body_model(0, n_verts=64, n_faces=8)  # the joints need J_regressor only; the host oracle still skins every vertex
    skel = A.skeleton(model)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup_calls": 1, "fps": a.fps, "host_sequences": a.host_sequences,
           "host_baseline": "tests/amass_oracle.py per sequence (fp64 numpy restatement, Python-loop DBSCAN and head velocities; not the "
                            "reference's SMPL-H + sklearn path), wall clock", "shapes": []}
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        distinct = min(DISTINCT, B)
        seqs = []
        for k in range(distinct):
            m = synthetic.make_eval_motion(1, T, seed=k + 1, check=False)
            seqs.append({"name": "seq%d" % k, "poses": m["local_aa"][0].reshape(T, 66).astype(np.float64),
                         "trans": m["root_trans"][0].astype(np.float64), "mocap_framerate": a.fps})
        seqs = [seqs[b % distinct] for b in range(B)]
        lo, hi = A.trim_range(T)
        n = hi - lo
        offsets = np.arange(B + 1) * n
        ro, pb, tr = (torch.from_numpy(np.concatenate([s[k][lo:hi, c0:c1].astype(np.float32) for s in seqs])).to(dev)
                      for k, c0, c1 in (("poses", 0, 3), ("poses", 3, 66), ("trans", 0, 3)))
        tables = [A.downsample_table(n, a.fps)[0]] * B
        out = {}

        def call():
            joints, head_rot = A.body_joints(ro, pb, tr, skel)
            floor, contacts, discard = A.floor_and_contacts(joints, offsets, a.fps)
            out["floor"], out["discard"] = floor, discard
            out["head"] = A.head_tracks(joints, head_rot, contacts, floor, offsets, tables)[0]

        t_med, t_lo, t_hi = timed(call, a.iters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = A.process_sequences(seqs, model)
        drv_ms = (time.perf_counter() - t0) * 1e3
        n_host = min(a.host_sequences, B)
        t0 = time.perf_counter()
        want = [O.process_seq(model, s["name"], s["poses"], s["trans"], a.fps) for s in seqs[:n_host]]
        host_ms = (time.perf_counter() - t0) * 1e3 / n_host
        floors = out["floor"].cpu().numpy()
        row = {"sequences": B, "raw_frames": T, "trimmed_frames": n, "floor_path": "lds" if n <= A.LDS_FRAMES else "workspace",
               "output_frames": int(tables[0].size), "hip_ms": round(t_med, 3), "hip_ms_min": round(t_lo, 3), "hip_ms_max": round(t_hi, 3),
               "raw_frames_per_s": round(B * n / t_med * 1e3), "process_sequences_ms": round(drv_ms, 1),
               "host_ms_per_sequence": round(host_ms, 1), "host_ms_batch_extrapolated": round(host_ms * B, 1),
               "ratio_extrapolated": round(host_ms * B / t_med, 1),
               "floor_bits_equal_host": bool(all(floors[b].tobytes() == np.float32(want[b][1]["fc"]["offset_floor_height"]).tobytes()
                                                 for b in range(n_host))),
               "discard_equal_host": bool(all(bool(out["discard"][b]) == want[b][1]["fc"]["discard_seq"] for b in range(n_host))),
               "kept": sum(isinstance(r, dict) for r in recs)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
