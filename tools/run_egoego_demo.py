#!/usr/bin/env python3
"""The whole EgoEgo pipeline of run_egoego.py:55-192 on the MI355X: precomputed optical-flow features and a DROID-SLAM trajectory
-> HeadNet / GravityNet (egoego_release_amd.stage1) -> the head pose -> stage 2's sliding-window sampler -> forward kinematics.

    python tools/run_egoego_demo.py --data_root_folder test_data/ares --weight_root_folder pretrained_models \\
        --stats cano_min_max_mean_std_data_window_120.p --rest_offsets rest_offsets.npy \\
        --window 60 --normal_window 120 --normal_n_dec_layers 2 --input_of_feats --diffusion_window 120 --out egoego_out.npz

  --data_root_folder    the reference's ARES demo layout (demo_ares_data.p, droid_slam_res/, <scene>/<seq>/raft_of_feats/)
  --weight_root_folder  stage1_headnet_ares_250.pt, stage1_gravitynet_2000.pt, stage2_diffusion_4.pt (run_egoego.py:57-85); a
                        missing file means seeded synthetic weights for that network (listed in the report)
  --stats / --rest_offsets / --timesteps / --seed / --ddim_steps / --ddim_eta  as in tools/run_stage2_demo.py (--ddim_eta > 0
                        switches stage 2's per-step noise to the in-kernel Philox stream keyed by --seed)

Writes an npz with the stage-1 head pose [B, T, 7], the local axis-angle [B, T', 22, 3], the root [B, T', 3] and the global joints
[B, T', 22, 3], and prints one JSON line with the stage-1 and stage-2 wall times.  The floor-height shift of run_egoego.py:161-173
runs on the device (egoego_release_amd.evaluate): the npz also holds floor_height [B] (determine_floor_height_and_contacts at 30 fps
on the joints moved so that the first frame's head is at x = y = 0) and root_trans_floor [B, T', 3], the moved root joint with that
height taken off z.  Not done: get_head_vel (computed but never used by the reference) and, without --body_model, the visualisation.
The meshes of --gen_vis keep their placement (mesh_shift); take floor_height off their z to stand them on the floor.

  --body_model DIR      the reference's smpl_models/smplh_amass layout (male/model.npz, female/model.npz).  With --gen_vis, the
                        first sample of every sequence goes through the SMPL-H body model as in gen_full_body_vis (male, zero
                        betas; run_egoego.py:161-166 first moves the first frame's head to x = y = 0): the npz gains mesh_verts
                        [T', V, 3], mesh_jnts [T', 22, 3] and mesh_shift [3] (the translation applied) of the first sequence,
                        and <--vis_folder>/<sequence>/objs gets one OBJ file per frame.  Blender rendering stays not done.
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
sys.path.insert(0, HERE)
from egoego_release_amd import evaluate, harness, make_weights, ModelConfig, stage1  # noqa: E402
from egoego_release_amd.synthetic import make_stage1_weights  # noqa: E402
import run_stage2_demo as S2  # noqa: E402

HEADNET_FILE, GRAVITYNET_FILE, DIFFUSION_FILE = "stage1_headnet_ares_250.pt", "stage1_gravitynet_2000.pt", "stage2_diffusion_4.pt"


def parse_opt(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--device", default="0", help="cuda device")
    p.add_argument("--workers", type=int, default=0, help="accepted for flag compatibility")
    # HeadNet (run_egoego.py parse_opt)
    p.add_argument("--window", type=int, default=90)
    p.add_argument("--n_dec_layers", type=int, default=2)
    p.add_argument("--n_head", type=int, default=4)
    p.add_argument("--d_k", type=int, default=256)
    p.add_argument("--d_v", type=int, default=256)
    p.add_argument("--d_model", type=int, default=256)
    p.add_argument("--dist_scale", type=float, default=10.0)
    p.add_argument("--freeze_of_cnn", action="store_true", help="accepted for flag compatibility")
    p.add_argument("--input_of_feats", action="store_true")
    # GravityNet
    p.add_argument("--normal_window", type=int, default=90)
    p.add_argument("--normal_n_dec_layers", type=int, default=4)
    p.add_argument("--normal_n_head", type=int, default=4)
    p.add_argument("--normal_d_k", type=int, default=256)
    p.add_argument("--normal_d_v", type=int, default=256)
    p.add_argument("--normal_d_model", type=int, default=256)
    # stage 2
    p.add_argument("--diffusion_window", type=int, default=80)
    p.add_argument("--diffusion_batch_size", type=int, default=1, help="samples per trajectory (sample_bs, run_egoego.py:146)")
    p.add_argument("--diffusion_n_dec_layers", type=int, default=4)
    p.add_argument("--diffusion_n_head", type=int, default=4)
    p.add_argument("--diffusion_d_k", type=int, default=256)
    p.add_argument("--diffusion_d_v", type=int, default=256)
    p.add_argument("--diffusion_d_model", type=int, default=512)
    p.add_argument("--use_min_max", action="store_true", help="accepted for flag compatibility")
    p.add_argument("--canonicalize_init_head", action="store_true", help="accepted for flag compatibility")
    p.add_argument("--gen_vis", action="store_true", help="with --body_model: write the body meshes (otherwise accepted and ignored)")
    p.add_argument("--body_model", default="", help="folder with male/model.npz (SMPL-H); enables --gen_vis")
    p.add_argument("--vis_folder", default="", help="where the OBJ folders go (default: egoego_demo_on_ares next to --out)")
    # assets
    p.add_argument("--data_root_folder", required=True)
    p.add_argument("--weight_root_folder", default="")
    p.add_argument("--stats", required=True)
    p.add_argument("--rest_offsets", required=True)
    p.add_argument("--timesteps", type=int, default=1000, help="diffusion steps (lower = truncated chain, for smoke runs)")
    p.add_argument("--ddim_steps", type=int, default=0, help="N > 0: the strided DDIM sampler over N timesteps per window (0 = the ancestral chain)")
    p.add_argument("--ddim_eta", type=float, default=0.0, help="DDIM noise weight in [0, 1]; > 0 draws in-kernel Philox noise keyed by --seed")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default="egoego_out.npz")
    return p.parse_args(argv)


def _weight(opt, name):
    path = os.path.join(opt.weight_root_folder, name) if opt.weight_root_folder else ""
    return path if path and os.path.exists(path) else None


def build_stage1(opt, dev):
    hn = stage1.HeadFormer(opt, dev)
    gn = stage1.HeadNormalFormer(opt, dev, eval_whole_pipeline=True)
    notes = {}
    for m, fname, seed in ((hn, HEADNET_FILE, 0), (gn, GRAVITYNET_FILE, 1)):
        path = _weight(opt, fname)
        if path:
            m.load_state_dict(torch.load(path, map_location="cpu")["transformer_encoder_state_dict"])
            notes[fname] = path
        else:
            m.load_state_dict(make_stage1_weights(m.cfg.kind, m.cfg, seed))
            notes[fname] = f"missing: synthetic seeded weights (seed {seed})"
    return hn, gn, notes


def build_stage2(opt, dev):
    kw = dict(window=opt.diffusion_window, d_model=opt.diffusion_d_model, n_head=opt.diffusion_n_head,
              n_dec_layers=opt.diffusion_n_dec_layers, d_k=opt.diffusion_d_k, d_v=opt.diffusion_d_v)
    path = _weight(opt, DIFFUSION_FILE)
    if path:
        model, _ = harness.load_stage2_checkpoint(path, device=dev, **kw)
        note = path
    else:
        model = harness.build_stage2_model(device=None, **kw)
        cfg = ModelConfig(max_timesteps=opt.diffusion_window + 1, d_model=opt.diffusion_d_model, n_head=opt.diffusion_n_head,
                          n_dec_layers=opt.diffusion_n_dec_layers, d_k=opt.diffusion_d_k, d_v=opt.diffusion_d_v)
        model.load_state_dict(make_weights(cfg, 0), strict=False)
        model = model.to(dev)
        note = "missing: synthetic seeded weights (seed 0)"
    model.num_timesteps = opt.timesteps
    return model, note


def gen_full_body_vis(bm_dict, root_trans, local_aa, mesh_folder):
    """trainer_amass_cond_motion_diffusion.py:348-382 without the rendering: root_trans [T, 3], local_aa [T, 22, 3] -> mesh joints
    [T, 22, 3], vertices [T, V, 3]; the OBJ files go to `mesh_folder`."""
    from egoego_release_amd import body
    betas = torch.zeros(1, 16, device=root_trans.device)
    jnts, verts, faces = body.run_smpl_model(root_trans[None].float(), local_aa[None].float(), betas, ["male"], bm_dict)
    body.save_verts_faces_to_mesh_file(verts[0].cpu().numpy(), faces.cpu().numpy(), mesh_folder)
    return jnts[0], verts[0]


def main(argv=None):
    opt = parse_opt(argv)
    if opt.ddim_steps < 0 or not 0.0 <= opt.ddim_eta <= 1.0:
        raise SystemExit("--ddim_steps must be >= 0 and --ddim_eta in [0, 1]")
    sampler = dict(sampler="ddim", n_steps=opt.ddim_steps, eta=opt.ddim_eta) if opt.ddim_steps else {}
    dev = torch.device("cuda", int(opt.device))
    torch.cuda.set_device(dev)
    hn, gn, notes = build_stage1(opt, dev)
    model, notes[DIFFUSION_FILE] = build_stage2(opt, dev)
    if opt.ddim_steps and opt.ddim_eta > 0:  # (the strided sampler has no reference draw order to reproduce: its noise is drawn in-kernel)
        model.sampling_rng, model.philox_seed = "philox", opt.seed
    stats = S2._load_any(opt.stats)
    ds = harness.SkeletonStats(stats["global_jpos_min"], stats["global_jpos_max"], np.load(opt.rest_offsets), harness.SMPLH_PARENTS_22)
    batches = stage1.load_ares_demo(opt.data_root_folder)
    torch.manual_seed(opt.seed)
    out = {"head_pose": [], "local_aa": [], "root_trans": [], "global_jpos": [], "floor_height": [], "root_trans_floor": []}
    vis = bool(opt.body_model and opt.gen_vis)
    mesh, mesh_folders, t3 = {}, [], 0.0
    if vis:
        from egoego_release_amd import body
        bm_dict = {"male": body.BodyModel(os.path.join(opt.body_model, "male", "model.npz"), num_betas=16, device=dev)}
        vis_folder = opt.vis_folder or os.path.join(os.path.dirname(os.path.abspath(opt.out)), "egoego_demo_on_ares")
    t1 = t2 = 0.0
    names = []
    for batch in batches:
        names += list(batch["seq_name"])
        torch.cuda.synchronize()
        a = time.perf_counter()
        with torch.no_grad():
            hp, _, _ = stage1.estimate_head_pose(hn, gn, batch)
        torch.cuda.synchronize()
        b = time.perf_counter()
        rep_hp = hp.repeat_interleave(opt.diffusion_batch_size, 0)  # run_egoego.py:147
        aa, root = harness.full_body_gen_cond_head_pose_sliding_window(model, ds, rep_hp, **sampler)
        n, t = aa.shape[:2]
        _, gj = ds.fk_smpl(root.reshape(-1, 3), aa.reshape(-1, 22, 3))
        gj = gj.reshape(n, t, 22, 3)
        # run_egoego.py:161-173: the first frame's head to x = y = 0, then the root down by the floor height
        moved = evaluate.shift_xy_(gj.float().clone())
        floor, _, _ = evaluate.determine_floor_height_and_contacts(moved, 30)
        root_floor = evaluate.root_to_floor(moved, floor)
        torch.cuda.synchronize()
        c = time.perf_counter()
        t1, t2 = t1 + (b - a), t2 + (c - b)
        for k, v in (("head_pose", hp), ("local_aa", aa), ("root_trans", root), ("global_jpos", gj), ("floor_height", floor),
                     ("root_trans_floor", root_floor)):
            out[k].append(v.detach().cpu().numpy())
        if vis:
            move = gj[:, 0:1, 15:16, :].clone()  # run_egoego.py:161-166: the first frame's head to x = y = 0
            move[..., 2] = 0
            # run_egoego.py:166 takes the root JOINT position of the moved FK result (pred_fk_jpos[:, :, 0, :], rest offset
            # included) and :191 hands it to gen_full_body_vis as root_trans, so the body model adds its own J_0 on top: the
            # mesh sits J_0 away from the FK skeleton.  Kept as the reference does it, so the OBJ files agree with its output.
            vis_root = (gj - move)[0, :, 0, :]
            folder = os.path.join(vis_folder, str(batch["seq_name"][0]).replace(" ", ""), "objs")
            jn, vt = gen_full_body_vis(bm_dict, vis_root, aa[0], folder)
            torch.cuda.synchronize()
            t3 += time.perf_counter() - c
            mesh_folders.append(folder)
            if not mesh:
                mesh = {"mesh_verts": vt.cpu().numpy(), "mesh_jnts": jn.cpu().numpy(), "mesh_shift": -move[0, 0, 0].cpu().numpy()}
    np.savez_compressed(opt.out, **{k: np.concatenate(v) for k, v in out.items()}, **mesh)
    rep = {"sequences": names, "frames": int(out["head_pose"][0].shape[1]), "samples": opt.diffusion_batch_size,
           "stage1_seconds": round(t1, 4), "stage2_seconds": round(t2, 4), "diffusion_steps": opt.timesteps, "ddim_steps": opt.ddim_steps,
           "ddim_eta": opt.ddim_eta, "weights": notes,
           "not_done": ["get_head_vel", "visualisation"],
           "out": opt.out}
    if vis:
        rep["not_done"][1] = "Blender rendering of the meshes"
        rep.update(mesh_seconds=round(t3, 4), mesh_folders=mesh_folders)
    print(json.dumps(rep), flush=True)
    return rep


if __name__ == "__main__":
    main()
