#!/usr/bin/env python3
"""Score stage 1 on a whole ARES split: a HeadNet checkpoint and a GravityNet checkpoint over stage1_data.HeadBatches(for_eval=True)
(whole sequences from frame 0, a few ragged batches instead of one call per sequence) -> stage1.estimate_head_pose(lengths=,
pose_lengths=) -> stage1.head_pose_metrics against the batch's head_pose.  Prints one JSON line with the three means the
reference's eval_egoego.py:308-312 collects per sequence (s1_head_dist, s1_head_dist_rot_only, s1_head_trans_err in mm) and the
number of sequences.

    python tools/eval_stage1.py --data_root data --headnet runs/headnet/weights/train-20.pt --gravitynet runs/g/weights/train-20.pt \\
        --window 60 --normal_window 120 --normal_n_dec_layers 2 [--split test] [--feature_cache feats]

The estimate is moved onto the ground truth's first position, as estimate_head_pose does for stage 2 (--z_offset, default 0, is
its height shift); both trajectories then start at the same point, which is what the reference's subtraction of each one's first
xy gives in the plane.  A checkpoint that is not given is replaced by seeded synthetic weights, and the line says so.  A GPU is
required: there is no CPU path.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import stage1  # noqa: E402
from egoego_release_amd.stage1_data import HeadBatches, load_ares_split  # noqa: E402
from egoego_release_amd.synthetic import make_stage1_weights  # noqa: E402


def parse_opt(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_root", required=True, help="the folder that holds ares_egoego_processed/ and ares/")
    p.add_argument("--split", choices=("train", "test"), default="test")
    p.add_argument("--feature_cache", default=None, help="keep the arrays read in PATH.<split>.npz (tools/train_stage1.py's files)")
    p.add_argument("--headnet", default=None, help="a HeadNet checkpoint of tools/train_stage1.py")
    p.add_argument("--gravitynet", default=None, help="a GravityNet checkpoint of tools/train_stage1.py")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--z_offset", type=float, default=0.0)
    p.add_argument("--window", type=int, default=90)
    p.add_argument("--n_dec_layers", type=int, default=2)
    p.add_argument("--n_head", type=int, default=4)
    p.add_argument("--d_k", type=int, default=256)
    p.add_argument("--d_v", type=int, default=256)
    p.add_argument("--d_model", type=int, default=256)
    p.add_argument("--dist_scale", type=float, default=10.0)
    p.add_argument("--normal_window", type=int, default=90)
    p.add_argument("--normal_n_dec_layers", type=int, default=4)
    p.add_argument("--normal_n_head", type=int, default=4)
    p.add_argument("--normal_d_k", type=int, default=256)
    p.add_argument("--normal_d_v", type=int, default=256)
    p.add_argument("--normal_d_model", type=int, default=256)
    p.add_argument("--device", default="cuda")
    opt = p.parse_args(argv)
    opt.input_of_feats = True
    return opt


def main(argv=None):
    opt = parse_opt(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_stage1 needs a ROCm GPU: there is no CPU path")
    dev = torch.device(opt.device)
    hn = stage1.HeadFormer(opt, dev).to(dev)
    gn = stage1.HeadNormalFormer(opt, dev, eval_whole_pipeline=True).to(dev)
    notes = {}
    for m, path, seed, tag in ((hn, opt.headnet, 0, "headnet"), (gn, opt.gravitynet, 1, "gravitynet")):
        if path:
            m.load_state_dict(torch.load(path, map_location="cpu")["transformer_encoder_state_dict"])
            notes[tag] = path
        else:
            m.load_state_dict(make_stage1_weights(m.cfg.kind, m.cfg, seed))
            notes[tag] = f"not given: synthetic seeded weights (seed {seed})"
        m.eval()
    cache = f"{opt.feature_cache}.{opt.split}.npz" if opt.feature_cache else None
    seqs = load_ares_split(opt.data_root, opt.split == "train", opt.window, cache)
    batches = HeadBatches(seqs, opt.batch_size, window=opt.window, train=False, for_eval=True, shuffle=False, device=dev)
    got = []
    with torch.no_grad():
        for batch in batches:
            pose, _, _, n = stage1.estimate_head_pose(hn, gn, batch, z_offset=opt.z_offset, lengths=batch["lengths_host"],
                                                      pose_lengths=batch["pose_lengths_host"])
            gt = batch["head_pose"][:, :pose.shape[1]].to(pose.device).double()
            got.append(stage1.head_pose_metrics(pose, gt, n.tolist()))
    m = torch.cat(got).mean(0).tolist()  # the one read-back
    print(json.dumps({"split": opt.split, "sequences": len(batches.names), "dropped": batches.n_dropped, "s1_head_dist": m[0],
                      "s1_head_dist_rot_only": m[1], "s1_head_trans_err_mm": m[2], "weights": notes}))


if __name__ == "__main__":
    main()
