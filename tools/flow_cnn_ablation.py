#!/usr/bin/env python3
"""Ablation timing of the flow CNN's convolution main loop: time one 256-frame chunk of
FlowFeatureExtractor.extract on the product library or on a variant built with parts of flow_conv_kernel's K loop removed
(EGOEGO_FLOW_ABLATE in csrc/flow_cnn.h; a variant's features are wrong by design).

    python -m egoego_release_amd.build --variant -DEGOEGO_FLOW_ABLATE=6 --tag=fa6     # builds tools/_build/..._fa6.so
    python tools/flow_cnn_ablation.py [--tag fa6] [--frames 256] [--iters 5]
    python tools/flow_cnn_ablation.py --summarize DIR                                  # DIR/<tag>/*kernel_stats.csv -> table

Run each tag under `rocprofv3 --kernel-trace --stats` for per-kernel times; --summarize tabulates them (kernel time per call in
microseconds, per template: <TN, STEM>).  Prints one JSON line per run."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import _lib  # noqa: E402

MASKS = {"": "product", "fa1": "no MFMA", "fa2": "no global loads", "fa6": "no global loads, no LDS writes",
         "fa14": "no global loads, no LDS writes, no barrier (fragment reads + MFMA only)"}


def summarize(root):
    rows = {}
    for d in sorted(glob.glob(os.path.join(root, "*"))):
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not f:
            continue
        tag = os.path.basename(d)
        tag = "" if tag == "product" else tag
        rows[tag] = {r["Name"].split("(")[0].replace("void fcnn::", ""): float(r["TotalDurationNs"]) / 1e3
                     for r in csv.DictReader(open(f[0])) if "flow_" in r["Name"]}
    print(json.dumps({"variant_us_total": {MASKS.get(t, t): v for t, v in rows.items()}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    if a.tag:
        _lib.use_perfdebug_build(a.tag)
    import numpy as np
    import torch
    from egoego_release_amd import stage1, synthetic
    m = stage1.FlowFeatureExtractor(seed=0).to("cuda:0")
    flow = torch.from_numpy(synthetic.make_flows(8, 1)).to("cuda:0").repeat(a.frames // 8 + 1, 1, 1, 1)[:a.frames].contiguous()
    m.extract(flow)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.extract(flow)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(json.dumps({"variant": MASKS.get(a.tag, a.tag), "tag": a.tag, "frames": a.frames, "ms": round(float(np.median(ts)), 3)}))


if __name__ == "__main__":
    main()
