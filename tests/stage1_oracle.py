"""fp32 CPU restatement of the stage-1 estimators (HeadFormer / HeadNormalFormer with input_of_feats) on a state dict.

Paths are relative to the reference root: HE = egoego/model/head_estimation_transformer.py, HN =
egoego/model/head_normal_estimation_transformer.py, TM = egoego/model/transformer_module.py.  The decoder and heads use the same
torch ops as the reference (so they match it bit for bit on the CPU); the rotation steps are numpy float64.
tests/golden/make_stage1_golden.py asserts that this file reproduces the reference's own modules.
"""
import numpy as np
import torch
import torch.nn.functional as F

TR = "action_transformer."


def decoder(sd, feats, valid, n_layers, n_head=4):
    """TM:188-225 with use_full_attention: feats [W, window, F] (rows past valid[w] zeroed), valid [W] -> outputs of every layer
    ([W, window, 256] each).  One window at a time, as the reference runs them (so the CPU results are the reference's bits)."""
    valid = torch.as_tensor(valid).reshape(-1)
    per = [_decoder1(sd, feats[w:w + 1], valid[w:w + 1], n_layers, n_head) for w in range(feats.shape[0])]
    return [torch.cat([p[l] for p in per]) for l in range(n_layers)]


def _decoder1(sd, feats, valid, n_layers, n_head):
    W, T, _ = feats.shape
    valid = torch.as_tensor(valid)
    mask = (torch.arange(T)[None, :] < valid[:, None]).float()  # [W, T]
    x = feats.clone().float() * mask[..., None]
    emb = F.conv1d(x.transpose(1, 2), sd[TR + "start_conv.weight"], sd[TR + "start_conv.bias"]).transpose(1, 2)
    pos = sd[TR + "position_vec.weight"][torch.arange(T) + 1]
    out = emb + pos[None]
    outs = []
    for i in range(n_layers):
        a, f = TR + f"layer_stack.{i}.self_attn.", TR + f"layer_stack.{i}.pos_ffn."
        dk = sd[a + "w_q.weight"].shape[0] // n_head
        res = out
        q = F.linear(out, sd[a + "w_q.weight"], sd[a + "w_q.bias"]).view(W, T, n_head, dk).permute(2, 0, 1, 3).reshape(-1, T, dk)
        k = F.linear(out, sd[a + "w_k.weight"], sd[a + "w_k.bias"]).view(W, T, n_head, dk).permute(2, 0, 1, 3).reshape(-1, T, dk)
        v = F.linear(out, sd[a + "w_v.weight"], sd[a + "w_v.bias"]).view(W, T, n_head, dk).permute(2, 0, 1, 3).reshape(-1, T, dk)
        att = torch.bmm(q, k.transpose(1, 2)) / np.power(dk, 0.5)
        att = F.softmax(att, dim=2)
        o = torch.bmm(att, v).view(n_head, W, T, dk).permute(1, 2, 0, 3).reshape(W, T, -1)
        o = F.layer_norm(F.linear(o, sd[a + "fc.weight"], sd[a + "fc.bias"]) + res, (res.shape[-1],),
                         sd[a + "layer_norm.weight"], sd[a + "layer_norm.bias"])
        o = o * mask[..., None]
        res = o
        h = F.conv1d(F.relu(F.conv1d(o.transpose(1, 2), sd[f + "w_1.weight"], sd[f + "w_1.bias"])), sd[f + "w_2.weight"],
                     sd[f + "w_2.bias"]).transpose(1, 2)
        o = F.layer_norm(h + res, (res.shape[-1],), sd[f + "layer_norm.weight"], sd[f + "layer_norm.bias"])
        out = o * mask[..., None]
        outs.append(out)
    return outs


def mlp_head(sd, prefix, x, n_hidden):
    for j in range(n_hidden):
        x = torch.relu(F.linear(x, sd[f"{prefix}_mlp.affine_layers.{j}.weight"], sd[f"{prefix}_mlp.affine_layers.{j}.bias"]))
    return F.linear(x, sd[f"{prefix}_fc.weight"], sd[f"{prefix}_fc.bias"])


def headnet_heads(sd, x):
    """-> va [.., 3], dist [.., 1]"""
    return mlp_head(sd, "action_va", x, 3), mlp_head(sd, "action_dist", x, 3)


def gravity_head(sd, x0):
    return mlp_head(sd, "action_normal", x0, 2)


def block_spans(T, window):
    return [(b * window, min(T, (b + 1) * window) - b * window) for b in range(T // window + 1) if min(T, (b + 1) * window) > b * window]


# ---------------------------------------------------------------------------------------------- rotations (numpy float64)
def qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def qrot(q, v):
    u, w = q[1:], q[0]
    c1 = np.cross(u, v)
    return v + 2 * (w * c1 + np.cross(u, c1))


def va2rot(q0, va, dt=1.0 / 30):
    """HE:97-119: [T+1, 4]."""
    q = np.asarray(q0, np.float64)
    out = [q]
    for v in np.asarray(va, np.float64):
        a = qrot(q, v) * dt
        ang = np.linalg.norm(a)
        s = 0.5 - ang * ang / 48 if ang < 1e-6 else np.sin(ang / 2) / ang
        n = qmul(np.concatenate([[np.cos(ang / 2)], a * s]), q)
        n = -n if n[0] < 0 else n
        q = n / np.linalg.norm(n)
        out.append(q)
    return np.stack(out)


def mat2quat(m):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(np.asarray(m, np.float64).reshape(-1, 3, 3)).as_quat()
    q = np.concatenate([q[:, 3:], q[:, :3]], -1)
    return np.where(q[:, :1] < 0, -q, q)


def quat2mat(q):
    from scipy.spatial.transform import Rotation
    q = np.asarray(q, np.float64).reshape(-1, 4)
    return Rotation.from_quat(np.concatenate([q[:, 1:], q[:, :1]], -1)).as_matrix()


def rotation_from_floor_normal(n):
    a = np.asarray(n, np.float64) / np.linalg.norm(n)
    b = np.array([0.0, 0.0, 1.0])
    v, c = np.cross(a, b), a.dot(b)
    s = np.linalg.norm(v)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + k + k.dot(k) * ((1 - c) / s ** 2)


def umeyama_r(x, y):
    """evo.core.geometry.umeyama_alignment(x [3, n], y [3, n], with_scale) -> r."""
    m, n = x.shape
    mx, my = x.mean(1), y.mean(1)
    cov = (y - my[:, None]).dot((x - mx[:, None]).T) / n
    u, d, v = np.linalg.svd(cov)
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(v) < 0:
        s[-1, -1] = -1
    return u.dot(s).dot(v)


# ---------------------------------------------------------------------------------------------- the two estimators
def headnet_eval(sd, window, n_layers, feats, q0, slam, dist_scale):
    """HE:214-308 for one sequence: feats [T, 512] float32, q0 [4], slam [L, 3] -> dict."""
    feats = torch.as_tensor(feats).float()
    T = feats.shape[0]
    spans = block_spans(T, window)
    blocks = torch.zeros(len(spans), window, feats.shape[1])
    for i, (s, n) in enumerate(spans):
        blocks[i, :n] = feats[s:s + n]
    valid = torch.tensor([n for _, n in spans])
    layers = decoder(sd, blocks, valid, n_layers)
    hd = [headnet_heads(sd, layers[-1][i:i + 1, :n]) for i, (_, n) in enumerate(spans)]
    va_l = [h[0][0] for h in hd]
    dist_l = [h[1][0] for h in hd]
    va_all = torch.cat(va_l).numpy()
    quat = va2rot(q0, va_all)
    # HE:180-212 in the slam trajectory's dtype, step by step as the reference
    d = torch.cat(dist_l)[:, 0] / dist_scale
    sl = torch.as_tensor(np.asarray(slam))
    steps = torch.stack([torch.linalg.norm(sl[i + 1] - sl[i]) for i in range(sl.shape[0] - 1)])
    m = min(len(steps), d.shape[0])
    scale_t = d[:m].mean() / steps[:m].mean()
    tr = [sl[0]]
    for i in range(sl.shape[0] - 1):
        tr.append(tr[-1] + scale_t * (sl[i + 1] - sl[i]))
    trans = torch.stack(tr).double().numpy()
    scale = float(scale_t)
    n = min(len(trans), len(quat))
    return {"layers": layers, "valid": valid, "va": va_l, "dist": dist_l, "quat": quat, "pred_scale": scale,
            "head_pose": np.concatenate([trans[:n], quat[:n]], -1)}


def gravity_features(rot, trans, window):
    """HN:118-145: rot [L, 3, 3], trans [L, 3] -> feats [window, 18] float32, valid."""
    rot = torch.as_tensor(rot).float()
    trans = torch.as_tensor(trans).float()
    if rot.shape[0] > window:
        rot, trans = rot[:window + 1], trans[:window + 1]
    n = rot.shape[0] - 1
    d6 = rot[:, :2, :].reshape(-1, 6)
    diff = torch.matmul(rot[1:], rot[:-1].transpose(1, 2))
    f = torch.cat((d6[:-1], trans[:-1], diff[:, :2, :].reshape(-1, 6), trans[1:] - trans[:-1]), -1)
    out = torch.zeros(window, 18)
    out[:n] = f
    return out, max(n, 0)


def gravity_eval(sd, window, n_layers, rot, trans, gt_pose, pred_scale):
    """HN:214-294 for one sequence: rot [L, 3, 3], trans [L, 3] (first frame at the origin), gt_pose [L', 7]."""
    feats, n = gravity_features(rot, trans, window)
    layers = decoder(sd, feats[None], torch.tensor([n]), n_layers)
    normal = gravity_head(sd, layers[-1][:, 0])[0]
    Rn = rotation_from_floor_normal(normal.numpy()).astype(np.float32).astype(np.float64)
    rot = np.asarray(rot, np.float64)
    trans = np.asarray(trans, np.float32).astype(np.float64)
    a = np.concatenate([trans[:1], trans[:1] + np.cumsum(pred_scale * (trans[1:] - trans[:-1]).dot(Rn.T), 0)])
    arot = np.einsum("ij,tjk->tik", Rn, rot)
    est = a[:len(gt_pose)].copy()
    ref = np.asarray(gt_pose, np.float64)[:, :3].copy()
    est[:, 2] = 1
    ref[:, 2] = 1
    r = umeyama_r(est.T, ref.T).astype(np.float32).astype(np.float64)
    drot = np.einsum("ij,tjk->tik", r, arot)
    dtrans = (a - a[:1]).dot(r.T) + np.asarray(gt_pose, np.float64)[:1, :3]
    return {"layers": layers, "valid": n, "pred_normal": normal.numpy(), "normal_rot": Rn, "align_rot": r,
            "head_pose": np.concatenate([dtrans, mat2quat(drot)], -1)}


def assemble(gravity_pose, headnet_pose, gt_pose, z_offset=-0.13):
    """run_egoego.py:104-136."""
    n = min(len(gravity_pose), len(headnet_pose))
    hp = np.concatenate([gravity_pose[:n, :3], headnet_pose[:n, 3:]], -1).astype(np.float64)
    hp[:, :2] -= hp[0:1, :2]
    hp[:, :3] += np.asarray(gt_pose, np.float64)[0:1, :3] - hp[0:1, :3]
    hp[:, 2] += z_offset
    return hp
