#!/usr/bin/env python3
"""Stage-2 entry point: head-pose trajectory -> full-body SMPL-H motion through the MI355X diffusion sampler.

The counterpart, for the stage this repo accelerates, of the reference's drivers
    eval_stage2.py:58-222 (test_diffusion / full_body_gen_cond_head_pose_sliding_window on ground-truth head poses)
    run_egoego.py:55-192  (the same call on stage-1 head poses, then fk_smpl and the MPJPE of
                           kinpoly/scripts/eval_metrics_imu_rec.py:297-301)
with the reference's `--diffusion_*` flags (eval_stage2.py:395-404).  Stage 1 (HeadNet / GravityNet on precomputed optical-flow
features) is egoego_release_amd.stage1; DROID-SLAM, RAFT, the AMASS / ARES datasets, SMPL-H and the pretrained weights are not part
of this repo: every asset is an input file, and without `--weight` the run uses the seeded synthetic weights.

    python tools/run_stage2_demo.py --head_pose head_qpos.npy --stats cano_min_max_mean_std_data_window_120.p \\
        --rest_offsets rest_offsets.npy [--weight model-10.pt] [--gt_jpos gt.npy] --diffusion_window 120 --out out.npz

  --head_pose     .npy [T,7] or [B,T,7]: xyz + quaternion (w,x,y,z), what trainer.full_body_gen_cond_head_pose_sliding_window
                  takes (trainer_amass_cond_motion_diffusion.py:261-276); or the reference's demo pickle
                  (test_data/ares/demo_ares_data.p: its 'head_qpos').  SEVERAL files (trajectories of any lengths, each [T,7]):
                  they are sampled together through the ragged sliding-window call
                  (harness.full_body_gen_cond_head_pose_sliding_window_ragged: one batch per window index over all of them, in-kernel
                  Philox noise); the outputs are then padded to the longest result, with "out_lengths" giving each one's frames
  --stats         the dataset's min/max statistics pickle (global_jpos_min / global_jpos_max, amass_diffusion_dataset.py:232-239;
                  tools/build_motion_windows.py writes it from the raw motion)
  --rest_offsets  .npy [22,3] rest-pose joint offsets (AMASSDataset.rest_human_offsets; tools/build_motion_windows.py writes it
                  from the licensed SMPL-H model); --parents optionally overrides the SMPL-H kintree
  --gt_jpos       optional .npy [T,22,3] ground-truth global joints -> MPJPE (mm) and, under "metrics", the position keys of
                  compute_metrics_for_smpl per sample (egoego_release_amd.evaluate, on the device; the foot sliding of the samples
                  is measured from each sample's own floor height, the ground truth's from 0)
  --gt_quat       optional .npy [T,22,4] ground-truth global rotations (w,x,y,z): adds the root / head rotation keys
  --ddim_steps N  N > 0: every window runs the strided DDIM sampler over N timesteps (model.ddim_timesteps) instead of the
                  reference's ancestral chain over all --timesteps (0, the default); --ddim_eta in [0, 1] weights its per-step
                  noise (0 = deterministic; > 0 draws in-kernel, so it needs --sampling_rng philox).  Not in the reference
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import harness, make_weights, ModelConfig  # noqa: E402


def mpjpe_mm(pred_global_jpos, gt_global_jpos):
    """kinpoly/scripts/eval_metrics_imu_rec.py:297-301: root-relative mean per-joint position error in millimetres.
    pred / gt: [T, J, 3] (arrays or tensors)."""
    p = torch.as_tensor(pred_global_jpos, dtype=torch.float64)
    g = torch.as_tensor(gt_global_jpos, dtype=torch.float64)
    p = p - p[:, 0:1]
    g = g - g[:, 0:1]
    return float(torch.linalg.norm(p - g, dim=2).mean() * 1000.0)


def _load_any(path):
    if path.endswith(".npy"):
        return np.load(path)
    try:
        import joblib
        return joblib.load(path)
    except Exception:
        with open(path, "rb") as f:
            return pickle.load(f)


def load_head_pose(path):
    d = _load_any(path)
    if isinstance(d, dict):  # the reference's demo pickle: {0: {'head_qpos': (T,7), ...}}
        d = d[sorted(d.keys())[0]] if "head_qpos" not in d else d
        d = d["head_qpos"]
    hp = torch.as_tensor(np.asarray(d), dtype=torch.float32)
    return hp[None] if hp.dim() == 2 else hp


def parse_opt(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--device", default="0", help="cuda device")
    p.add_argument("--weight", default="", help="reference checkpoint ({'step','model','ema','scaler'}); empty = synthetic weights")
    # the reference's diffusion flags (eval_stage2.py:395-404)
    p.add_argument("--diffusion_window", type=int, default=120, help="horizon")
    p.add_argument("--diffusion_batch_size", type=int, default=1, help="samples drawn per trajectory (sample_bs, run_egoego.py:146)")
    p.add_argument("--diffusion_n_dec_layers", type=int, default=4)
    p.add_argument("--diffusion_n_head", type=int, default=4)
    p.add_argument("--diffusion_d_k", type=int, default=256)
    p.add_argument("--diffusion_d_v", type=int, default=256)
    p.add_argument("--diffusion_d_model", type=int, default=512)
    p.add_argument("--use_min_max", action="store_true", help="accepted for flag compatibility (always on in the shipped configs)")
    p.add_argument("--canonicalize_init_head", action="store_true", help="accepted for flag compatibility (always on)")
    # assets
    p.add_argument("--head_pose", required=True, nargs="+", help="one trajectory file, or several (sampled together, ragged)")
    p.add_argument("--stats", required=True)
    p.add_argument("--rest_offsets", required=True)
    p.add_argument("--parents", default="", help="comma-separated 22 parent indices (default: SMPL-H kintree)")
    p.add_argument("--gt_jpos", default="")
    p.add_argument("--gt_quat", default="")
    p.add_argument("--timesteps", type=int, default=1000, help="diffusion steps (lower = truncated chain, for smoke runs)")
    p.add_argument("--sampling_rng", default="torch", choices=("torch", "philox"))
    p.add_argument("--ddim_steps", type=int, default=0, help="N > 0: the strided DDIM sampler over N timesteps per window (0 = the ancestral chain)")
    p.add_argument("--ddim_eta", type=float, default=0.0, help="DDIM noise weight in [0, 1]; > 0 needs --sampling_rng philox")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--noise", default="", help="torch-saved dict {'x_all','cond','steps'} of injected draws (harness.py "
                                               "p_sample_loop_sliding_window_w_canonical): reproducibility / parity runs")
    p.add_argument("--gpus", type=int, default=0,
                   help="N >= 1: shard the (trajectory, sample) pairs over N GPUs by SEQUENCE (egoego_release_amd.dist.harness_sharded: "
                        "Philox draws keyed by the global pair index, one all_gather of the result; the output does not depend on N). "
                        "N > 1 starts its own ranks (a child `python -m torch.distributed.run`); EGOEGO_DIST_BACKEND=gloo lets ranks share a GPU. "
                        "0 (default): the single-process path with the reference's RNG order")
    p.add_argument("--out", default="stage2_out.npz")
    return p.parse_args(argv)


def self_launch(n, argv):
    """`--gpus N` outside a launcher: run this very command under torch.distributed.run in a CHILD process (never an exec)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(proc.stdout)
    sys.stdout.flush()
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    if proc.returncode != 0 or not lines:
        raise SystemExit(proc.returncode or 1)
    return json.loads(lines[-1])


def main(argv=None):
    opt = parse_opt(argv)
    several = len(opt.head_pose) > 1
    if several and (opt.gpus >= 1 or opt.gt_jpos or opt.noise):
        raise SystemExit("several --head_pose files run the single-process ragged call: --gpus, --gt_jpos and --noise take one trajectory")
    if not several:
        opt.head_pose = opt.head_pose[0]
    if opt.ddim_steps < 0 or not 0.0 <= opt.ddim_eta <= 1.0:
        raise SystemExit("--ddim_steps must be >= 0 and --ddim_eta in [0, 1]")
    if opt.ddim_steps and opt.ddim_eta > 0 and opt.sampling_rng != "philox" and not several and not (opt.noise and opt.gpus < 1):
        raise SystemExit("--ddim_eta > 0 draws its per-step noise in-kernel: add --sampling_rng philox")
    sampler = dict(sampler="ddim", n_steps=opt.ddim_steps, eta=opt.ddim_eta) if opt.ddim_steps else {}
    if opt.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(opt.gpus, sys.argv[1:] if argv is None else argv)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("EGOEGO_DIST_BACKEND", "nccl")
        ndev = torch.cuda.device_count()
        if backend == "nccl" and world > ndev:
            raise SystemExit(f"{world} ranks over RCCL need {world} GPUs, {ndev} visible (EGOEGO_DIST_BACKEND=gloo shares GPUs between ranks)")
        opt.device = str(int(os.environ.get("LOCAL_RANK", "0")) % max(1, ndev))
        torch.cuda.set_device(int(opt.device))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", int(opt.device)))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", int(opt.device))
    stats = _load_any(opt.stats)
    rest = np.load(opt.rest_offsets)
    parents = tuple(int(v) for v in opt.parents.split(",")) if opt.parents else harness.SMPLH_PARENTS_22
    ds = harness.SkeletonStats(stats["global_jpos_min"], stats["global_jpos_max"], rest, parents)

    model_kw = dict(window=opt.diffusion_window, d_model=opt.diffusion_d_model, n_head=opt.diffusion_n_head,
                    n_dec_layers=opt.diffusion_n_dec_layers, d_k=opt.diffusion_d_k, d_v=opt.diffusion_d_v)
    if opt.weight:
        model, info = harness.load_stage2_checkpoint(opt.weight, device=dev, **model_kw)
    else:
        model = harness.build_stage2_model(device=None, **model_kw)
        cfg = ModelConfig(max_timesteps=opt.diffusion_window + 1, d_model=opt.diffusion_d_model, n_head=opt.diffusion_n_head,
                          n_dec_layers=opt.diffusion_n_dec_layers, d_k=opt.diffusion_d_k, d_v=opt.diffusion_d_v)
        model.load_state_dict(make_weights(cfg, 0), strict=False)
        model = model.to(dev)
        info = {"step": None, "missing": [], "unexpected": [], "note": "synthetic seeded weights"}
    model.num_timesteps = opt.timesteps
    model.sampling_rng = opt.sampling_rng
    model.philox_seed = opt.seed

    torch.manual_seed(opt.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if opt.gpus >= 1:
        # sequence-sharded: every (trajectory, sample) pair stays on one rank (its windows depend on each other), one all_gather at the end
        from egoego_release_amd import dist as D
        head_pose = load_head_pose(opt.head_pose)
        aa, root = D.harness_sharded(model, ds, head_pose, sample_bs=opt.diffusion_batch_size, seed=opt.seed, parents=parents, **sampler)
        head_pose = head_pose.repeat_interleave(opt.diffusion_batch_size, 0)
    elif several:
        # trajectories of different lengths: every window index runs once for all of them (the per-step draws are in-kernel Philox)
        poses = []
        for path in opt.head_pose:
            hp = load_head_pose(path)
            if hp.shape[0] != 1:
                raise SystemExit(f"{path}: one [T,7] trajectory per file expected when several files are given, got {tuple(hp.shape)}")
            poses.append(hp[0].to(dev))
        model.sampling_rng = "philox"
        aa, root, out_lengths = harness.full_body_gen_cond_head_pose_sliding_window_ragged(model, ds, poses,
                                                                                           samples_per_sequence=opt.diffusion_batch_size, **sampler)
    else:
        head_pose = load_head_pose(opt.head_pose).repeat_interleave(opt.diffusion_batch_size, 0).to(dev)
        noise = torch.load(opt.noise, map_location="cpu") if opt.noise else None
        aa, root = harness.full_body_gen_cond_head_pose_sliding_window(model, ds, head_pose, noise=noise, **sampler)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        if rank != 0:
            dist.destroy_process_group()
            return None
    # global joints through FK, as run_egoego.py:152-158 does with ds.fk_smpl
    b, t = aa.shape[:2]
    gq, gj = ds.fk_smpl(root.reshape(-1, 3), aa.reshape(-1, 22, 3))
    gj = gj.reshape(b, t, 22, 3)
    out = {"local_aa": aa.cpu().numpy(), "root_trans": root.cpu().numpy(), "global_jpos": gj.cpu().numpy()}
    if several:
        keep = (torch.arange(t)[None, :] < out_lengths[:, None]).numpy()
        out["global_jpos"] = out["global_jpos"] * keep[:, :, None, None]  # (FK of the zero rows past a result's end is not a pose)
        out["out_lengths"] = out_lengths.numpy()
        rep = {"frames": [int(v) for v in out_lengths], "samples": int(b), "sequences": len(poses),
               "windows": sum(len(harness.window_spans(int(p.shape[0]), opt.diffusion_window)) for p in poses) * opt.diffusion_batch_size,
               "diffusion_steps": opt.timesteps, "ddim_steps": opt.ddim_steps, "ddim_eta": opt.ddim_eta, "seconds": round(el, 3), "checkpoint": info, "ranks": world, "sharding": None,
               "ragged": True}
        np.savez_compressed(opt.out, **out)
        print(json.dumps(rep), flush=True)
        return rep
    rep = {"frames": int(t), "samples": int(b), "windows": len(range(0, head_pose.shape[1], opt.diffusion_window - harness.OVERLAP)),
           "diffusion_steps": opt.timesteps, "ddim_steps": opt.ddim_steps, "ddim_eta": opt.ddim_eta, "seconds": round(el, 3), "checkpoint": info, "ranks": world,
           "sharding": "by sequence (dist.harness_sharded)" if opt.gpus >= 1 else None}
    if opt.gt_jpos:
        gt = np.load(opt.gt_jpos)
        from egoego_release_amd import evaluate
        n = min(t, gt.shape[0])
        edev = gj.device if gj.is_cuda else torch.device("cuda", torch.cuda.current_device())
        pj, pq = gj[:, :n].float().contiguous().to(edev), gq.reshape(b, t, 22, 4)[:, :n].float().contiguous().to(edev)
        gt_j = torch.as_tensor(gt[:n], dtype=torch.float32, device=edev)
        if opt.gt_quat:
            gt_q = torch.as_tensor(np.load(opt.gt_quat)[:n], dtype=torch.float32, device=edev)
        else:  # without rotations to compare against, the samples' own stand in and the rotation keys are left out
            gt_q, gt_j = pq, gt_j[None].expand(b, -1, -1, -1)
        floor = evaluate.determine_floor_height_and_contacts(pj, 30)[0] if 2 <= n <= evaluate.MAX_FRAMES else 0.
        m = evaluate.compute_metrics_for_smpl(gt_q, gt_j, 0., pq, pj, floor)
        skip = () if opt.gt_quat else ("root_dist", "root_rot_dist", "head_dist", "head_rot_dist")
        # (mpjpe_mm keeps the ground truth file's own precision; "metrics" holds what the device computes from float32 tensors)
        rep["mpjpe_mm"] = [mpjpe_mm(gj[i, : gt.shape[0]].cpu(), gt[:t]) for i in range(b)]
        rep["metrics"] = {k: m[k].tolist() for k in evaluate.METRIC_KEYS + ("single_jpe",) if k not in skip}
    np.savez_compressed(opt.out, **out)
    print(json.dumps(rep), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    return rep


if __name__ == "__main__":
    main()
