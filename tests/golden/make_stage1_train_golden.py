#!/usr/bin/env python3
"""Golden vectors of STAGE-1 TRAINING, produced by running the reference's own modules on the CPU with seeded synthetic weights:
    HeadFormer.forward, compute_loss, backward          egoego/model/head_estimation_transformer.py:97-178, 310-345
    HeadNormalFormer.forward, compute_loss, backward    egoego/model/head_normal_estimation_transformer.py:118-165, 334-342
Runs only where the reference checkout is present.  What executes is the reference's Python, unmodified.  Not the reference's
(absent from this image): the bodies of the four pytorch3d.transforms functions its training path calls (quaternion_apply,
axis_angle_to_quaternion, quaternion_multiply, quaternion_invert): tests/stage1_train_oracle.py's differentiable torch code from
the published formulas; the other stand-ins are make_stage1_golden.py's.

Shapes: window 8, 1 layer, B = 3, HeadNet's seq_len (8, 5, 1), GravityNet's sequences whole, eval() mode (no dropout), fp32.  Recorded: the inputs, the loss parts, the
heads, d loss / d heads, and per parameter gradient a digest (L2 norm, sum, first 64 entries; whole gradients are about 13 MB).
The script asserts that tests/stage1_train_oracle.py reproduces all of it.

    python tests/golden/make_stage1_train_golden.py
"""
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
WINDOW, LAYERS, B = 8, 1, 3
SEQ_LEN = (8, 5, 1)
SEED_HEAD, SEED_NORMAL = 21, 22
DIGEST = 64


def digest(g):
    """[L2 norm, sum, the first 64 entries (zero padded when the tensor is smaller)]"""
    g = g.detach().double().reshape(-1)
    first = np.zeros(DIGEST)
    first[:min(DIGEST, g.numel())] = g[:DIGEST].numpy()
    return np.concatenate(([float(g.norm()), float(g.sum())], first))


def worst_grad_err(O, lv, named, names):
    """The largest relative error of the oracle's gradients (leaves lv) against the module's; the w_k.bias gradients are
    identically zero in exact arithmetic (softmax does not see a shift of all keys of a query) and are judged against the whole."""
    total = float(torch.sqrt(sum(named[k].grad.double().norm() ** 2 for k in names)))
    worst = 0.0
    for k in names:
        ref = named[k].grad.double()
        if k.endswith("w_k.bias"):
            assert float(ref.norm()) <= 1e-6 * total and float(lv[k].grad.norm()) <= 1e-6 * total, k
            continue
        worst = max(worst, O.rel_err(lv[k].grad.reshape(ref.shape), ref))
    return worst


def main():
    import make_stage1_golden as G
    import stage1_oracle as S1
    import stage1_train_oracle as O
    from egoego_release_amd.synthetic import make_stage1_train_batch, make_stage1_weights

    G.install_stubs()
    tr = sys.modules["pytorch3d.transforms"]
    for name in ("quaternion_apply", "axis_angle_to_quaternion", "quaternion_multiply", "quaternion_invert"):
        setattr(tr, name, getattr(O, name))
    from egoego.model.head_estimation_transformer import HeadFormer
    from egoego.model.head_normal_estimation_transformer import HeadNormalFormer

    opt = Namespace(window=WINDOW, n_dec_layers=LAYERS, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0, input_of_feats=True,
                    freeze_of_cnn=True, w_rotation=1.0, w_va=0.7, w_dist=0.4)
    cfg = Namespace(window=WINDOW, n_dec_layers=LAYERS, n_head=4, d_k=256, d_v=256, d_model=256)
    rec = {"seq_len": np.array(SEQ_LEN), "weights": np.array([opt.w_rotation, opt.w_va, opt.w_dist, opt.dist_scale]),
           "seeds": np.array([SEED_HEAD, SEED_NORMAL])}

    # ---- HeadNet
    sd = make_stage1_weights("headnet", cfg, SEED_HEAD)
    m = HeadFormer(opt, "cpu")
    m.load_state_dict(sd)
    m.eval()
    data = make_stage1_train_batch("headnet", B, WINDOW, seed=3, lengths=SEQ_LEN)
    out = m(data)
    out["head_va"].retain_grad()
    out["head_dist_scalar"].retain_grad()
    loss, orient, va, dist = m.compute_loss(out, data)
    loss.backward()
    loss, orient, va, dist = (v.detach() for v in (loss, orient, va, dist))
    named = dict(m.named_parameters())
    frozen = [k for k, p in named.items() if p.grad is None]
    assert frozen == ["action_transformer.position_vec.weight"], frozen
    n_train = sum(p.numel() for k, p in named.items() if p.grad is not None)
    print("HeadNet trainable parameters:", n_train)
    heads = torch.cat((out["head_va"], out["head_dist_scalar"]), -1).detach()
    d_heads = torch.cat((out["head_va"].grad, out["head_dist_scalar"].grad), -1)
    for k in ("of", "head_pose", "head_vels"):
        rec["h_" + k] = data[k].numpy()
    rec["h_loss"] = np.array([float(loss), float(orient), float(va), float(dist)])
    rec["h_heads"], rec["h_d_heads"] = heads.numpy(), d_heads.numpy()
    rec["h_names"] = np.array(sorted(k for k in named if k not in frozen))
    rec["h_digest"] = np.stack([digest(named[k].grad) for k in rec["h_names"]])

    ls, lv, oh, od = O.headnet_step(sd, data, opt, LAYERS, dtype=torch.float32)
    e = {"heads": O.rel_err(oh, heads.double()), "d_heads": O.rel_err(od, d_heads.double()),
         "loss": max(abs(float(ls[k]) - float(r)) / abs(float(r)) for k, r in zip(("loss", "orient", "va", "dist"), (loss, orient, va, dist))),
         "grads": worst_grad_err(O, lv, named, rec["h_names"])}
    print("HeadNet, oracle fp32 against the reference:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["heads"] < 1e-5 and e["loss"] < 1e-5 and e["d_heads"] < 1e-5 and e["grads"] < 1e-4, e
    # the inference restatement agrees on the heads too
    lay = S1.decoder(sd, data["of"], data["seq_len"], LAYERS)[-1]
    va1, d1 = S1.headnet_heads(sd, lay)
    assert float((torch.cat((va1, d1), -1) - heads).abs().max()) < 1e-5

    # ---- GravityNet
    sd = make_stage1_weights("gravitynet", cfg, SEED_NORMAL)
    m = HeadNormalFormer(opt, "cpu")
    m.load_state_dict(sd)
    m.eval()
    data = make_stage1_train_batch("gravitynet", B, WINDOW, seed=4)
    # (every sequence has its window + 1 frames: the reference builds GravityNet's features from every frame it is given, so a
    # shorter seq_len would leave non-zero feature rows behind the mask, which no call of this package produces)
    out = m(data)
    out["pred_normal"].retain_grad()
    loss, nl = m.compute_loss(out, data)
    loss.backward()
    loss, nl = loss.detach(), nl.detach()
    named = dict(m.named_parameters())
    frozen = [k for k, p in named.items() if p.grad is None]
    assert frozen == ["action_transformer.position_vec.weight"], frozen
    for k in ("head_rot_mat", "head_trans", "floor_normal"):
        rec["g_" + k] = data[k].numpy()
    rec["g_loss"] = np.array([float(loss), float(nl)])
    rec["g_heads"], rec["g_d_heads"] = out["pred_normal"].detach().numpy(), out["pred_normal"].grad.numpy()
    rec["g_names"] = np.array(sorted(k for k in named if k not in frozen))
    rec["g_digest"] = np.stack([digest(named[k].grad) for k in rec["g_names"]])
    feats = torch.stack([S1.gravity_features(data["head_rot_mat"][b], data["head_trans"][b], WINDOW)[0] for b in range(B)])
    rec["g_feats"] = feats.numpy()
    gl, lv, oh, od = O.gravity_step(sd, feats, [WINDOW] * B, data["floor_normal"], LAYERS, dtype=torch.float32)
    e = {"heads": O.rel_err(oh, out["pred_normal"].detach().double()), "d_heads": O.rel_err(od, out["pred_normal"].grad.double()),
         "loss": abs(float(gl) - float(loss)) / abs(float(loss)), "grads": worst_grad_err(O, lv, named, rec["g_names"])}
    print("GravityNet, oracle fp32 against the reference:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["heads"] < 1e-5 and e["loss"] < 1e-5 and e["d_heads"] < 1e-5 and e["grads"] < 1e-4, e

    path = os.path.join(HERE, "stage1_train_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
