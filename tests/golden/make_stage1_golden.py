#!/usr/bin/env python3
"""Golden vectors of STAGE 1 (HeadNet / GravityNet with precomputed optical-flow features), produced by running the reference's
own modules on the CPU with seeded synthetic weights (egoego_release_amd.synthetic.make_stage1_weights).

Runs only in the authoring container (the reference checkout present).  What executes is the reference's Python, unmodified:
    ARESDemoDataset                  egoego/data/ares_demo_dataset.py   (the demo sequence: 139 features, 140 SLAM frames)
    HeadFormer.forward_for_eval      egoego/model/head_estimation_transformer.py:214-308
    HeadNormalFormer.forward_for_eval egoego/model/head_normal_estimation_transformer.py:214-294 (eval_whole_pipeline=True)
    and the assembly of run_egoego.py:104-136 (restated: it sits inside test(), which also loads stage 2).
Not the reference's (absent from this image): pytorch3d.transforms (make_window_loop_golden.py's scipy stand-ins plus
axis_angle_to_quaternion), evo's PoseTrajectory3D.align / sync.associate_trajectories (evo's published Umeyama algorithm; the two
trajectories share their timestamps, so association is the identity), torchvision and cv2 (never reached with input_of_feats).

Two shape sets: the demo's (HeadNet window 60 x 2 layers, GravityNet 120 x 2 layers: scripts/test_egoego_pipeline.sh) and the
defaults of run_egoego.py's parse_opt (90 x 2, 90 x 4).  The script also asserts that tests/stage1_oracle.py reproduces them.

    python tests/golden/make_stage1_golden.py
"""
import os
import sys
import types
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
REF = "/root/reference"
DATA = os.path.join(REF, "test_data", "ares")
SETS = {"demo": dict(window=60, n_dec_layers=2, normal_window=120, normal_n_dec_layers=2),
        "default": dict(window=90, n_dec_layers=2, normal_window=90, normal_n_dec_layers=4)}
SEED_HEAD, SEED_NORMAL, DIST_SCALE = 11, 12, 10.0


def install_stubs():
    import make_window_loop_golden as W
    from scipy.spatial.transform import Rotation as Rot

    tr = W.transforms_module()

    def axis_angle_to_quaternion(aa):
        a = W._np(aa)
        return W._like(W._wxyz(Rot.from_rotvec(a.reshape(-1, 3)), a.shape[:-1]), aa)

    tr.axis_angle_to_quaternion = axis_angle_to_quaternion

    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("pytorch3d", transforms=tr)
    sys.modules["pytorch3d.transforms"] = tr
    stub("cv2")
    tv = stub("torchvision", models=types.SimpleNamespace())
    stub("torchvision.models")
    del tv

    def umeyama_alignment(x, y, with_scale=False):  # evo.core.geometry.umeyama_alignment
        m, n = x.shape
        mean_x, mean_y = x.mean(axis=1), y.mean(axis=1)
        sigma_x = 1.0 / n * (np.linalg.norm(x - mean_x[:, np.newaxis]) ** 2)
        outer_sum = np.zeros((m, m))
        for i in range(n):
            outer_sum += np.outer((y[:, i] - mean_y), (x[:, i] - mean_x))
        cov_xy = np.multiply(1.0 / n, outer_sum)
        u, d, v = np.linalg.svd(cov_xy)
        s = np.eye(m)
        if np.linalg.det(u) * np.linalg.det(v) < 0.0:
            s[m - 1, m - 1] = -1
        r = u.dot(s).dot(v)
        c = 1 / sigma_x * np.trace(np.diag(d).dot(s)) if with_scale else 1.0
        t = mean_y - np.multiply(c, r.dot(mean_x))
        return r, t, c

    class PoseTrajectory3D:
        def __init__(self, positions_xyz=None, orientations_quat_wxyz=None, timestamps=None):
            self._positions_xyz = np.array(positions_xyz, dtype=np.float64)
            self._orientations_quat_wxyz = np.array(orientations_quat_wxyz, dtype=np.float64)
            self.timestamps = np.array(timestamps)

        def align(self, traj_ref, correct_scale=False, correct_only_scale=False, n=-1):
            with_scale = correct_scale or correct_only_scale
            r, t, s = umeyama_alignment(self._positions_xyz.T, traj_ref._positions_xyz.T, with_scale)
            if not correct_only_scale:  # evo transforms the trajectory in place (not read by the caller beyond positions)
                self._positions_xyz = (s * r.dot(self._positions_xyz.T)).T + t
            return r, t, s

    tmod = stub("evo.core.trajectory", PoseTrajectory3D=PoseTrajectory3D)
    smod = stub("evo.core.sync", associate_trajectories=lambda a, b, *args, **kw: (a, b))
    core = stub("evo.core", trajectory=tmod, sync=smod, lie_algebra=types.SimpleNamespace(),
                metrics=types.SimpleNamespace(PoseRelation=None))
    sys.modules["evo.core.lie_algebra"] = core.lie_algebra
    stub("evo.core.metrics", PoseRelation=None)
    tools = stub("evo.tools", file_interface=types.SimpleNamespace())
    sys.modules["evo.tools.file_interface"] = tools.file_interface
    stub("evo.main_ape")
    stub("evo", core=core, tools=tools)
    sys.path.insert(0, REF)


def opt_for(s):
    return Namespace(window=s["window"], n_dec_layers=s["n_dec_layers"], n_head=4, d_k=256, d_v=256, d_model=256,
                     dist_scale=DIST_SCALE, input_of_feats=True, freeze_of_cnn=True,
                     normal_window=s["normal_window"], normal_n_dec_layers=s["normal_n_dec_layers"], normal_n_head=4,
                     normal_d_k=256, normal_d_v=256, normal_d_model=256)


def main():
    install_stubs()
    from egoego.data.ares_demo_dataset import ARESDemoDataset
    from egoego.model.head_estimation_transformer import HeadFormer
    from egoego.model.head_normal_estimation_transformer import HeadNormalFormer
    from egoego_release_amd.synthetic import make_stage1_weights
    import stage1_oracle as O

    torch.set_grad_enabled(False)
    ds = ARESDemoDataset(DATA)
    item = ds[0]
    batch = {k: (torch.from_numpy(np.ascontiguousarray(v))[None] if isinstance(v, np.ndarray) else
                 ([v] if isinstance(v, str) else torch.tensor([v]))) for k, v in item.items()}
    rec = {"of": batch["of"][0].float().numpy(), "head_pose": item["head_pose"], "slam_raw": np.load(os.path.join(
        DATA, "droid_slam_res", item["seq_name"].split("-")[0], "-".join(item["seq_name"].split("-")[1:]) + ".npy")),
        "aligned_slam_trans": item["aligned_slam_trans"], "ori_slam_trans": item["ori_slam_trans"],
        "ori_slam_rot_mat": item["ori_slam_rot_mat"], "aligned_slam_rot_mat": item["aligned_slam_rot_mat"],
        "seq_len": np.int64(item["seq_len"]), "dist_scale": np.float64(DIST_SCALE),
        "seeds": np.array([SEED_HEAD, SEED_NORMAL])}
    worst = 0.0
    for tag, s in SETS.items():
        opt = opt_for(s)
        hn = HeadFormer(opt, "cpu")
        sd_h = make_stage1_weights("headnet", Namespace(window=opt.window, n_dec_layers=opt.n_dec_layers, n_head=4, d_k=256,
                                                        d_v=256, d_model=256), SEED_HEAD)
        assert sorted(hn.state_dict()) == sorted(sd_h), "HeadNet state_dict keys"
        for k, v in hn.state_dict().items():
            assert tuple(v.shape) == tuple(sd_h[k].shape), k
        hn.load_state_dict(sd_h)
        hn.eval()
        gn = HeadNormalFormer(opt, "cpu", eval_whole_pipeline=True)
        sd_g = make_stage1_weights("gravitynet", Namespace(window=opt.normal_window, n_dec_layers=opt.normal_n_dec_layers,
                                                           n_head=4, d_k=256, d_v=256, d_model=256), SEED_NORMAL)
        assert sorted(gn.state_dict()) == sorted(sd_g), "GravityNet state_dict keys"
        for k, v in gn.state_dict().items():
            assert tuple(v.shape) == tuple(sd_g[k].shape), k
        gn.load_state_dict(sd_g)
        gn.eval()
        rec[f"{tag}_headnet_keys"] = np.array(sorted(hn.state_dict()))
        rec[f"{tag}_headnet_shapes"] = np.array([list(hn.state_dict()[k].shape) + [0] * (3 - hn.state_dict()[k].dim())
                                                  for k in sorted(hn.state_dict())])
        rec[f"{tag}_gravity_keys"] = np.array(sorted(gn.state_dict()))
        rec[f"{tag}_gravity_shapes"] = np.array([list(gn.state_dict()[k].shape) + [0] * (3 - gn.state_dict()[k].dim())
                                                  for k in sorted(gn.state_dict())])

        # instrument the decoders to record every layer's output
        seen = {"h": [], "g": []}

        def hook(key):
            def f(mod, inp, out):
                seen[key].append(out[0].detach().clone())
            return f

        hh = [l.register_forward_hook(hook("h")) for l in hn.action_transformer.layer_stack]
        gh = [l.register_forward_hook(hook("g")) for l in gn.action_transformer.layer_stack]
        out_h = hn.forward_for_eval(batch)
        pred_scale = out_h["pred_scale"]
        normal_in = {"head_trans": batch["ori_slam_trans"] - batch["ori_slam_trans"][:, 0:1, :],
                     "head_rot_mat": batch["ori_slam_rot_mat"], "ori_head_pose": batch["head_pose"],
                     "seq_len": torch.tensor(batch["ori_slam_trans"].shape[1]).float()[None]}
        # the Rodrigues and Umeyama results, recorded through the module's own calls
        import egoego.model.head_normal_estimation_transformer as HNM
        got = {}
        orig_rot, orig_align = HNM.cal_rotation_from_floor_normal, gn.align_xy_plane_traj

        def rec_rot(n):
            got["pred_normal"] = np.array(n, np.float32)
            got["normal_rot"] = orig_rot(n)
            return got["normal_rot"]

        def rec_align(e, r):
            res = orig_align(e, r)
            got["align_rot"] = res[0]
            return res

        HNM.cal_rotation_from_floor_normal = rec_rot
        gn.align_xy_plane_traj = rec_align
        out_g = gn.forward_for_eval(normal_in, pred_scale)
        HNM.cal_rotation_from_floor_normal = orig_rot
        for h in hh + gh:
            h.remove()
        # run_egoego.py:104-136
        hp = torch.cat((out_g["head_pose"][:, :, :3], out_h["head_pose"][:, :, 3:]), -1).double()
        hp[0, :, :2] -= hp[0, 0:1, :2].clone()
        hp[0, :, :3] += batch["head_pose"][0, 0:1, :3].double() - hp[0, 0:1, :3]
        hp[0, :, 2] -= 0.13

        nb = len(seen["h"]) // opt.n_dec_layers
        T = int(item["seq_len"])
        spans = O.block_spans(T, opt.window)
        assert nb == len(spans)
        P = f"{tag}_"
        # the last layer's output of every window is recorded (the size limit of a fixture); the oracle is asserted below to
        # reproduce EVERY layer bit for bit, and the GPU tests compare each layer with it
        Lh, Lg = opt.n_dec_layers - 1, opt.normal_n_dec_layers - 1
        for b, (st, n) in enumerate(spans):
            rec[P + f"h_block{b}_layer{Lh}"] = seen["h"][b * opt.n_dec_layers + Lh][0].numpy()
        rec[P + f"g_layer{Lg}"] = seen["g"][Lg][0].numpy()
        # per-block va / dist from the module's own heads on the recorded last-layer outputs
        vas, dists = [], []
        for b, (st, n) in enumerate(spans):
            x = seen["h"][b * opt.n_dec_layers + opt.n_dec_layers - 1][:, :n]
            vas.append(hn.action_va_fc(hn.action_va_mlp(x))[0].numpy())
            dists.append(hn.action_dist_fc(hn.action_dist_mlp(x))[0].numpy())
        rec[P + "va"] = np.concatenate(vas)
        rec[P + "dist"] = np.concatenate(dists)
        rec[P + "headnet_head_pose"] = out_h["head_pose"][0].numpy()
        rec[P + "pred_scale"] = np.array(pred_scale.numpy())
        rec[P + "pred_normal"] = got["pred_normal"]
        rec[P + "normal_rot"] = got["normal_rot"]
        rec[P + "align_rot"] = got["align_rot"]
        rec[P + "gravity_head_pose"] = out_g["head_pose"][0].numpy()
        rec[P + "head_pose"] = hp[0].numpy()

        # the oracle must reproduce all of it
        oh = O.headnet_eval(sd_h, opt.window, opt.n_dec_layers, rec["of"], item["head_pose"][0, 3:], item["aligned_slam_trans"],
                            DIST_SCALE)
        for b in range(nb):
            for l in range(opt.n_dec_layers):
                e = (oh["layers"][l][b] - seen["h"][b * opt.n_dec_layers + l][0]).abs().max().item()
                assert e == 0.0, (tag, b, l, e)
        assert np.array_equal(torch.cat(oh["va"]).numpy(), rec[P + "va"]), tag
        assert np.array_equal(torch.cat(oh["dist"]).numpy(), rec[P + "dist"]), tag
        errs = {"quat": np.abs(oh["quat"][:len(rec[P + "headnet_head_pose"])] - rec[P + "headnet_head_pose"][:, 3:]).max(),
                "scale": abs(oh["pred_scale"] - float(rec[P + "pred_scale"])) / abs(float(rec[P + "pred_scale"])),
                "hn_pose": np.abs(oh["head_pose"] - rec[P + "headnet_head_pose"]).max()}
        og = O.gravity_eval(sd_g, opt.normal_window, opt.normal_n_dec_layers, normal_in["head_rot_mat"][0].numpy(),
                            normal_in["head_trans"][0].numpy(), item["head_pose"], float(rec[P + "pred_scale"]))
        for l in range(opt.normal_n_dec_layers):
            e = (og["layers"][l][0] - seen["g"][l][0]).abs().max().item()
            assert e == 0.0, (tag, "g", l, e)
        assert np.array_equal(og["pred_normal"], rec[P + "pred_normal"]), tag
        errs["normal_rot"] = np.abs(og["normal_rot"] - rec[P + "normal_rot"].astype(np.float32)).max()
        errs["align_rot"] = np.abs(og["align_rot"] - rec[P + "align_rot"].astype(np.float32)).max()
        errs["g_pose"] = np.abs(og["head_pose"] - rec[P + "gravity_head_pose"]).max()
        errs["pose"] = np.abs(O.assemble(og["head_pose"], oh["head_pose"], item["head_pose"]) - rec[P + "head_pose"]).max()
        print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
        worst = max(worst, max(errs.values()))
    assert worst < 1e-6, worst
    out = os.path.join(HERE, "stage1_golden.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
