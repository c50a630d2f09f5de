#!/usr/bin/env python3
"""Turn an ARES demo layout's raw RAFT flows into the optical-flow features stage 1 reads (egoego/model/resnet.py
FeatureExtractor on the MI355X, egoego_release_amd.stage1.FlowFeatureExtractor):

    python tools/extract_flow_features.py --data_root_folder test_data/ares [--checkpoint stage1_headnet.pt]

For every of_files entry of every sequence in <data_root_folder>/demo_ares_data.p, reads .../raft_flows/NNNNN.npy ([224, 224, 2])
and writes .../raft_of_feats/NNNNN.npy ((512,) float64, the dtype of the demo's own files), which is where load_ares_demo and
tools/run_egoego_demo.py --input_of_feats look for them.
  --checkpoint  a FeatureExtractor state dict (cnn.resnet.*), or a HeadNet checkpoint trained without input_of_feats (its
                cnn.resnet.* part is used); without one the extractor's seeded synthetic weights (--seed) are used.
Prints one JSON line: frames, files written, seconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from egoego_release_amd import stage1  # noqa: E402


def load_cnn_state_dict(path):
    ck = torch.load(path, map_location="cpu")
    for k in ("transformer_encoder_state_dict", "model", "state_dict"):
        if isinstance(ck, dict) and k in ck and isinstance(ck[k], dict):
            ck = ck[k]
            break
    cnn, _ = stage1.split_headnet_state_dict(ck)
    if not cnn:
        raise SystemExit(f"{path}: no cnn.resnet.* tensors")
    return cnn


def flow_files(data_root_folder):
    """[(raft_flows path, raft_of_feats path)] of every of_files entry, in order, without repeats."""
    import joblib
    d = joblib.load(os.path.join(data_root_folder, "demo_ares_data.p"))
    out, seen = [], set()
    for k in range(len(d)):
        for f in d[k]["of_files"]:
            f = f.replace(stage1.ARES_SRC_ROOT, data_root_folder)
            if f not in seen:
                seen.add(f)
                out.append((f, f.replace("raft_flows", "raft_of_feats")))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--data_root_folder", required=True)
    p.add_argument("--checkpoint", default=None)
    p.add_argument("--seed", type=int, default=0, help="synthetic weights' seed when there is no checkpoint")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--batch", type=int, default=256, help="frames per extract call")
    a = p.parse_args(argv)
    t0 = time.time()
    sd = load_cnn_state_dict(a.checkpoint) if a.checkpoint else None
    m = stage1.FlowFeatureExtractor(seed=a.seed, state_dict=sd).to(a.device)
    files = flow_files(a.data_root_folder)
    for i in range(0, len(files), a.batch):
        part = files[i:i + a.batch]
        flow = torch.from_numpy(np.stack([np.load(src).astype(np.float32) for src, _ in part]))
        feats = m.extract(flow).double().cpu().numpy()
        for (_, dst), f in zip(part, feats):
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            np.save(dst, f)
    print(json.dumps({"frames": len(files), "written": len(files), "seconds": round(time.time() - t0, 3)}))


if __name__ == "__main__":
    main()
