#!/usr/bin/env python3
"""Train a stage-1 estimator on the HIP path: the reference's trainer_head_estimation.py (HeadNet) or trainer_amass_head_gravity_
normal_estimation.py (GravityNet) loop through egoego_release_amd.trainer.Stage1Trainer, without wandb and plots.

    python tools/train_stage1.py --kind headnet --epochs 20 --save_dir runs/headnet             seeded synthetic batches
    python tools/train_stage1.py --kind gravitynet --batches train.pt --val_batches val.pt ...  torch.save'd lists of batch dicts
    python tools/train_stage1.py --kind gravitynet --motion train_amass_smplh_motion.p [--val_motion test_amass_smplh_motion.p] ...
                                                      GravityNet on the head poses of a motion file (tools/process_amass.py)
    python tools/train_stage1.py --kind headnet --data_root data --window 60 --batch_size 8 [--feature_cache feats.npz] ...
                                                      HeadNet on the ARES files (the reference's scripts/train_headnet_on_ares.sh)

A batch dict is what the reference's DataLoader yields (synthetic.make_stage1_train_batch documents the keys).  --motion builds
GravityNet's batches on the GPU (egoego_release_amd.stage1_data.GravityBatches: random windows, one random rotation and scale per
sample) from the file's `head_qpos`; without --val_motion the file is split by dataset name as the reference's divide_train_val
does.  --data_root builds HeadNet's batches on the GPU (stage1_data.HeadBatches over stage1_data.load_ares_split: the train split's
motion file, feature files and SLAM tracks under DIR; random windows) and validates on the test split's, unshuffled, as the
reference's trainer does; --feature_cache PATH keeps the arrays read in PATH.train.npz / PATH.test.npz, so that a later run opens
those two files only.  Checkpoints <save_dir>/weights/train-<epoch>.pt hold the reference's keys ('epoch',
'transformer_encoder_state_dict', 'optimizer_state_dict', 'loss'): HeadFormer.load_state_dict and tools/run_egoego_demo.py take them.
A GPU is required: there is no CPU path.
"""
import argparse
import json
import os
import pickle
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import stage1  # noqa: E402
from egoego_release_amd.synthetic import make_stage1_train_batch  # noqa: E402
from egoego_release_amd.trainer import Stage1Trainer  # noqa: E402


def parse_opt(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--kind", choices=("headnet", "gravitynet"), default="headnet")
    p.add_argument("--save_dir", default="runs/stage1")
    p.add_argument("--batches", default=None, help="a torch.save'd list of training batch dicts (default: seeded synthetic batches)")
    p.add_argument("--val_batches", default=None)
    p.add_argument("--motion", default=None, help="gravitynet: a motion file (joblib / pickle) whose entries hold head_qpos [T, 7]")
    p.add_argument("--val_motion", default=None, help="a second motion file for validation (default: --motion split by dataset name)")
    p.add_argument("--data_root", default=None, help="headnet: the folder that holds ares_egoego_processed/ and ares/ (the ARES files)")
    p.add_argument("--feature_cache", default=None, help="--data_root: keep the arrays read in PATH.train.npz and PATH.test.npz")
    p.add_argument("--data_seed", type=int, default=0, help="--motion / --data_root: the seed of the shuffle and of the draws")
    p.add_argument("--synthetic_batches", type=int, default=8, help="synthetic batches per epoch when --batches is not given")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--epochs", type=int, default=1000)
    p.add_argument("--save_interval", type=int, default=50)
    p.add_argument("--validation_iter", type=int, default=1)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--window", type=int, default=None, help="default: 90 (HeadNet) / 120 (GravityNet)")
    p.add_argument("--n_dec_layers", type=int, default=2)
    p.add_argument("--n_head", type=int, default=4)
    p.add_argument("--d_k", type=int, default=256)
    p.add_argument("--d_v", type=int, default=256)
    p.add_argument("--d_model", type=int, default=256)
    p.add_argument("--w_rotation", type=float, default=1.0)
    p.add_argument("--w_va", type=float, default=1.0)
    p.add_argument("--w_dist", type=float, default=1.0)
    p.add_argument("--dist_scale", type=float, default=10.0)
    p.add_argument("--resume", default=None, help="a checkpoint to continue from")
    p.add_argument("--fused_update", action="store_true",
                   help="clip + AdamW in one fused call (optim.FusedAdamW); a step with a non-finite gradient norm is skipped")
    p.add_argument("--device", default="cuda")
    opt = p.parse_args(argv)
    if opt.window is None:
        opt.window = 90 if opt.kind == "headnet" else 120
    opt.input_of_feats = True
    if opt.motion and opt.kind != "gravitynet":
        p.error("--motion feeds GravityNet only (HeadNet's data needs optical-flow features)")
    if opt.val_motion and not opt.motion:
        p.error("--val_motion needs --motion")
    if opt.data_root and opt.kind != "headnet":
        p.error("--data_root feeds HeadNet only (GravityNet trains from --motion)")
    if opt.feature_cache and not opt.data_root:
        p.error("--feature_cache needs --data_root")
    return opt


def load_any(path):
    try:
        import joblib
        return joblib.load(path)
    except Exception:
        with open(path, "rb") as f:
            return pickle.load(f)


def motion_batches(opt, dev):
    """-> (train, val) GravityBatches of --motion / --val_motion (val None when the split leaves no validation sequence)."""
    from egoego_release_amd.stage1_data import GravityBatches, _head_poses, split_by_dataset
    kw = dict(window=opt.window, seed=opt.data_seed, device=dev)
    data = load_any(opt.motion)
    if opt.val_motion:
        return (GravityBatches(data, opt.batch_size, **kw),
                GravityBatches(load_any(opt.val_motion), opt.batch_size, train=False, shuffle=False, **kw))
    train_names, val_names = split_by_dataset([n for n, _ in _head_poses(data, None)])
    if not train_names:
        raise SystemExit(f"{opt.motion}: no sequence of a training dataset (stage1_data.TRAIN_DATASETS); give --val_motion to train on all of it")
    train = GravityBatches(data, opt.batch_size, names=train_names, **kw)
    return train, (GravityBatches(data, opt.batch_size, train=False, shuffle=False, names=val_names, **kw) if val_names else None)


def ares_batches(opt, dev):
    """-> (train, val) HeadBatches of --data_root's train and test splits (val None when the test split has no motion file)."""
    from egoego_release_amd.stage1_data import HeadBatches, load_ares_split
    cache = lambda split: f"{opt.feature_cache}.{split}.npz" if opt.feature_cache else None  # noqa: E731
    kw = dict(window=opt.window, seed=opt.data_seed, device=dev)
    train = HeadBatches(load_ares_split(opt.data_root, True, opt.window, cache("train")), opt.batch_size, **kw)
    test_file = os.path.join(opt.data_root, "ares_egoego_processed", "test_ares_smplh_motion.p")
    if not (os.path.exists(test_file) or (cache("test") and os.path.exists(cache("test")))):
        return train, None
    val = load_ares_split(opt.data_root, False, opt.window, cache("test"))
    return train, (HeadBatches(val, opt.batch_size, train=False, shuffle=False, **kw) if val else None)


def main(argv=None):
    opt = parse_opt(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_stage1 needs a ROCm GPU: there is no CPU path")
    dev = torch.device(opt.device)
    cls = stage1.HeadFormer if opt.kind == "headnet" else stage1.HeadNormalFormer
    model = cls(opt, dev).to(dev)
    load = lambda path: torch.load(path, map_location="cpu")  # noqa: E731
    if opt.motion:
        train, val = motion_batches(opt, dev)
    elif opt.data_root:
        train, val = ares_batches(opt, dev)
    elif opt.batches:
        train, val = load(opt.batches), (load(opt.val_batches) if opt.val_batches else None)
    else:
        train = [make_stage1_train_batch(opt.kind, opt.batch_size, opt.window, seed=s) for s in range(opt.synthetic_batches)]
        val = [make_stage1_train_batch(opt.kind, opt.batch_size, opt.window, seed=10_000 + s) for s in range(2)]
    tr = Stage1Trainer(model, train, val, lr=opt.learning_rate, validation_iter=opt.validation_iter, save_interval=opt.save_interval,
                       save_dir=opt.save_dir, fused_update=opt.fused_update)
    if opt.resume:
        tr.load(opt.resume)
    os.makedirs(opt.save_dir, exist_ok=True)
    with open(os.path.join(opt.save_dir, "opt.json"), "w") as f:
        json.dump(vars(opt), f, indent=1, sort_keys=True)
    for _ in range(opt.epochs):
        tr.train(1)
        line = {"epoch": tr.epoch, "train": tr.history[-1] if tr.history else None}
        if tr.val_history and tr.val_history[-1]["epoch"] == tr.epoch:
            line["val"] = tr.val_history[-1]
        print(json.dumps(line), flush=True)
    if tr.epoch % opt.save_interval != 0:
        tr.save(tr.epoch)
    print(json.dumps({"checkpoint": tr._path(tr.epoch)}))


if __name__ == "__main__":
    main()
