"""Deterministic synthetic weights and head-pose windows.

The reference ships no pretrained weights, datasets or tests, so
parity fixtures, the GPU parity tests and bench.py all use seeded random
weights in the reference's checkpoint layout
(/root/reference/egoego/model/transformer_cond_diffusion_model.py:143-214 and
egoego/model/transformer_module.py:36-186 define the tensors and their init
scales).  Values come from numpy's PCG64 keyed by (seed, tensor name), so the
same state dict can be rebuilt anywhere without shipping 44 MB of weights.
"""
import math
import zlib

import numpy as np
import torch


class ModelConfig:
    """Shapes of the stage-2 denoiser as run_egoego.py / eval_stage2.py build it
    (/root/reference/trainer_amass_cond_motion_diffusion.py:458-475)."""

    def __init__(self, d_feats=198, d_model=512, n_head=4, n_dec_layers=4, d_k=256, d_v=256,
                 max_timesteps=121, timesteps=1000, objective="pred_x0"):
        self.d_feats, self.d_model, self.n_head = d_feats, d_model, n_head
        self.n_dec_layers, self.d_k, self.d_v = n_dec_layers, d_k, d_v
        self.max_timesteps, self.timesteps, self.objective = max_timesteps, timesteps, objective

    def ctor_kwargs(self):
        return dict(d_feats=self.d_feats, d_model=self.d_model, n_head=self.n_head,
                    n_dec_layers=self.n_dec_layers, d_k=self.d_k, d_v=self.d_v,
                    max_timesteps=self.max_timesteps, out_dim=self.d_feats,
                    timesteps=self.timesteps, objective=self.objective)


def _rng(seed, name):
    return np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))


def _normal(seed, name, shape, std):
    return torch.from_numpy((_rng(seed, name).standard_normal(shape) * std).astype(np.float32))


def _uniform(seed, name, shape, bound):
    return torch.from_numpy(_rng(seed, name).uniform(-bound, bound, shape).astype(np.float32))


def sinusoid_position_table(n_position, d_hid):
    """Frozen table of transformer_module.py:6-24 (float64 math, row 0 zeroed)."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)[None, :]
    ang = pos / np.power(10000, 2 * (j // 2) / d_hid)
    tab = np.where(j % 2 == 0, np.sin(ang), np.cos(ang))
    tab[0] = 0.0
    return torch.from_numpy(tab.astype(np.float32))


def make_weights(cfg, seed=0):
    """Learnable tensors + the frozen position table, keyed like the reference state dict
    (without the 13 schedule buffers, which the module computes itself)."""
    D, dm, H = cfg.d_feats, cfg.d_model, cfg.n_head
    sd = {}
    tr = "denoise_fn.motion_transformer."

    def lin(name, out_f, in_f, conv=False):
        b = 1.0 / np.sqrt(in_f)  # PyTorch default kaiming_uniform(a=sqrt(5)) bound
        shape = (out_f, in_f, 1) if conv else (out_f, in_f)
        sd[name + ".weight"] = _uniform(seed, name + ".weight", shape, b)
        sd[name + ".bias"] = _uniform(seed, name + ".bias", (out_f,), b)

    lin(tr + "start_conv", dm, 2 * D, conv=True)
    sd[tr + "position_vec.weight"] = sinusoid_position_table(cfg.max_timesteps + 1, dm)
    for i in range(cfg.n_dec_layers):
        a = tr + f"layer_stack.{i}.self_attn."
        for nm, dd in (("w_q", cfg.d_k), ("w_k", cfg.d_k), ("w_v", cfg.d_v)):
            sd[a + nm + ".weight"] = _normal(seed, a + nm + ".weight", (H * dd, dm), np.sqrt(2.0 / (dm + dd)))
            sd[a + nm + ".bias"] = _uniform(seed, a + nm + ".bias", (H * dd,), 1.0 / np.sqrt(dm))
        sd[a + "fc.weight"] = _normal(seed, a + "fc.weight", (dm, H * cfg.d_v), np.sqrt(2.0 / (dm + H * cfg.d_v)))
        sd[a + "fc.bias"] = _uniform(seed, a + "fc.bias", (dm,), 1.0 / np.sqrt(H * cfg.d_v))
        f = tr + f"layer_stack.{i}.pos_ffn."
        lin(f + "w_1", dm, dm, conv=True)
        lin(f + "w_2", dm, dm, conv=True)
        for ln in (a + "layer_norm", f + "layer_norm"):
            # perturbed affine so a gamma/beta mix-up cannot hide behind the 1/0 default init
            sd[ln + ".weight"] = 1.0 + _normal(seed, ln + ".weight", (dm,), 0.1)
            sd[ln + ".bias"] = _normal(seed, ln + ".bias", (dm,), 0.1)
    lin("denoise_fn.linear_out", D, dm)
    lin("denoise_fn.time_mlp.1", 256, 64)
    lin("denoise_fn.time_mlp.3", dm, 256)
    return sd


def head_condition_mask(shape, device="cpu"):
    """1 on dims the model must synthesise, 0 on the head joint's position (45:48) and 6D
    rotation (156:162) — trainer_amass_cond_motion_diffusion.py:210-221."""
    m = torch.ones(shape, device=device)
    m[..., 45:48] = 0
    m[..., 156:162] = 0
    return m


def make_head_windows(B, T, seed=0, d_feats=198):
    """Synthetic normalised head-pose windows: zeros except a clipped random
    walk on the head position dims and the first two rows of random rotations on the head
    rot6d dims.  Returns (x_start [B,T,D], cond_mask [B,T,D])."""
    g = np.random.Generator(np.random.PCG64([seed, 7]))
    x = np.zeros((B, T, d_feats), dtype=np.float32)
    walk = np.cumsum(g.standard_normal((B, T, 3)) * 0.02, axis=1) + g.uniform(-0.5, 0.5, (B, 1, 3))
    x[..., 45:48] = np.clip(walk, -1, 1)
    q = g.standard_normal((B, T, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, a, b, c = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r0 = np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1)
    r1 = np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1)
    x[..., 156:159], x[..., 159:162] = r0, r1
    xs = torch.from_numpy(x)
    return xs, head_condition_mask(xs.shape)


# ------------------------------------------------------------------------------------------ synthetic motion (training-like data)
# first 22 entries of the SMPL-H kintree (harness.SMPLH_PARENTS_22)
_PARENTS_22 = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)


def make_motion_windows(B, T, seed=0, device="cpu", d_feats=198):
    """Seeded synthetic full-body windows in the model's data layout: [B, T, 198] = 22 normalised
    global joint positions + 22 global rotations as 6D.  NOT real motion — the reference's AMASS data cannot ship — but it has
    the structure a denoiser can learn from: a fixed seeded skeleton driven through forward kinematics by smooth per-joint
    rotations (a few low-frequency sinusoids per axis) on a smooth root walk, the head at the xy origin in the first frame
    like the reference's canonicalised windows (lafan1/utils.py:111-137), positions min/max-normalised to about [-1, 1] and 6D =
    the first two rows of each global rotation (amass_diffusion_dataset.py:446-447).  Used to optimise the module's own training
    loss for a few thousand steps (tools/make_trained_like_checkpoint.py): weights that are no longer the initialisation."""
    assert d_feats == 198
    dev = torch.device(device)
    g = torch.Generator(device="cpu").manual_seed(int(seed) * 7919 + 13)
    sk = np.random.Generator(np.random.PCG64([1234, 22]))  # the skeleton is the same for every seed
    offs = sk.standard_normal((22, 3))
    offs = offs / np.linalg.norm(offs, axis=1, keepdims=True) * sk.uniform(0.08, 0.35, (22, 1))
    offs[0] = 0.0
    offs = torch.from_numpy(offs.astype(np.float32)).to(dev)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def uni(*shape):
        return torch.rand(*shape, generator=g).to(dev)

    tt = torch.arange(T, device=dev, dtype=torch.float32) / max(T, 1)
    freqs = torch.tensor([0.5, 1.0, 2.0], device=dev)
    amp = 0.35 * rnd(B, 22, 3, 3) / freqs                                         # [B, joint, axis, harmonic]
    ph = 2 * math.pi * uni(B, 22, 3, 3)
    aa = (amp[..., None] * torch.sin(2 * math.pi * freqs[:, None] * tt + ph[..., None])).sum(-2)  # [B, 22, 3, T]
    aa = aa.permute(0, 3, 1, 2).contiguous()                                      # [B, T, 22, 3]
    aa[:, :, 0, 2] += 2 * math.pi * uni(B, 1)                                      # random heading of the root
    ang = aa.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    ax = aa / ang
    K = torch.zeros(B, T, 22, 3, 3, device=dev)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    eye = torch.eye(3, device=dev).expand(B, T, 22, 3, 3)
    # batched matmul in pieces: one call over B*T*22 > 2^24 matrices faults inside the BLAS on this stack (4096 x 196 x 22, measured)
    KK = torch.cat([k @ k for k in K.split(512)])
    Rl = eye + torch.sin(ang)[..., None] * K + (1 - torch.cos(ang))[..., None] * KK  # Rodrigues
    step = 0.01 * rnd(B, T, 3)
    step = torch.nn.functional.avg_pool1d(step.transpose(1, 2), 9, 1, 4, count_include_pad=False).transpose(1, 2)
    root = torch.cumsum(step, dim=1) * 3.0
    root[..., 2] = 0.9 + 0.05 * torch.sin(2 * math.pi * (tt[None] + uni(B, 1)))
    Rg, pos = [Rl[:, :, 0]], [root]
    for j in range(1, 22):
        p = _PARENTS_22[j]
        Rg.append(Rg[p] @ Rl[:, :, j])
        pos.append(pos[p] + (Rg[p] @ offs[j][None, None, :, None])[..., 0])
    Rg, pos = torch.stack(Rg, 2), torch.stack(pos, 2)                               # [B, T, 22, 3, 3], [B, T, 22, 3]
    shift = pos[:, :1, 15:16, :].clone()
    shift[..., 2] = 0
    pos = pos - shift
    lo = torch.tensor([-1.5, -1.5, 0.0], device=dev)
    hi = torch.tensor([1.5, 1.5, 2.0], device=dev)
    pos = ((pos - lo) / (hi - lo) * 2 - 1).clamp(-1, 1)
    return torch.cat((pos.reshape(B, T, 66), Rg[..., :2, :].reshape(B, T, 132)), -1).float()


# ------------------------------------------------------------------------------------------ stage 1 (HeadNet / GravityNet)
class Stage1Config:
    """Shapes of a stage-1 estimator: HeadFormer (kind 'headnet', head_estimation_transformer.py:48-95) or HeadNormalFormer
    (kind 'gravitynet', head_normal_estimation_transformer.py:65-110).  d_feats: 512 optical-flow features / 18 SLAM features."""

    def __init__(self, kind, window, n_dec_layers, n_head=4, d_k=256, d_v=256, d_model=256):
        if kind not in ("headnet", "gravitynet"):
            raise ValueError(f"unknown stage-1 kind {kind!r}")
        self.kind, self.window, self.n_dec_layers = kind, window, n_dec_layers
        self.n_head, self.d_k, self.d_v, self.d_model = n_head, d_k, d_v, d_model
        self.d_feats = 512 if kind == "headnet" else 18

    def head_dims(self):
        """{prefix: [(out, in), ...]} of the MLP heads (egoego/model/mlp.py) and their final Linear."""
        dm = self.d_model
        if self.kind == "headnet":
            return {"action_va": [(1024, dm), (512, 1024), (256, 512), (3, 256)],
                    "action_dist": [(1024, dm), (512, 1024), (256, 512), (1, 256)]}
        return {"action_normal": [(512, dm), (256, 512), (3, 256)]}


def make_stage1_weights(kind, cfg, seed=0):
    """Seeded synthetic state dict of a stage-1 estimator, keyed like the reference module's (`kind`: 'headnet' |
    'gravitynet'; cfg: Stage1Config or anything with window / n_dec_layers / n_head / d_k / d_v / d_model).  Init scales are
    the reference's (transformer_module.py:44-55 and PyTorch's defaults); LayerNorm affines are perturbed like make_weights'."""
    if not isinstance(cfg, Stage1Config):
        cfg = Stage1Config(kind, cfg.window, cfg.n_dec_layers, cfg.n_head, cfg.d_k, cfg.d_v, cfg.d_model)
    dm, H, dk, dv = cfg.d_model, cfg.n_head, cfg.d_k, cfg.d_v
    sd = {}
    tr = "action_transformer."

    def lin(name, out_f, in_f, conv=False):
        b = 1.0 / np.sqrt(in_f)
        sd[name + ".weight"] = _uniform(seed, name + ".weight", (out_f, in_f, 1) if conv else (out_f, in_f), b)
        sd[name + ".bias"] = _uniform(seed, name + ".bias", (out_f,), b)

    lin(tr + "start_conv", dm, cfg.d_feats, conv=True)
    sd[tr + "position_vec.weight"] = sinusoid_position_table(cfg.window + 1, dm)
    for i in range(cfg.n_dec_layers):
        a = tr + f"layer_stack.{i}.self_attn."
        for nm, dd in (("w_q", dk), ("w_k", dk), ("w_v", dv)):
            sd[a + nm + ".weight"] = _normal(seed, a + nm + ".weight", (H * dd, dm), np.sqrt(2.0 / (dm + dd)))
            sd[a + nm + ".bias"] = _uniform(seed, a + nm + ".bias", (H * dd,), 1.0 / np.sqrt(dm))
        sd[a + "fc.weight"] = _normal(seed, a + "fc.weight", (dm, H * dv), np.sqrt(2.0 / (dm + H * dv)))
        sd[a + "fc.bias"] = _uniform(seed, a + "fc.bias", (dm,), 1.0 / np.sqrt(H * dv))
        f = tr + f"layer_stack.{i}.pos_ffn."
        lin(f + "w_1", dm, dm, conv=True)
        lin(f + "w_2", dm, dm, conv=True)
        for ln in (a + "layer_norm", f + "layer_norm"):
            sd[ln + ".weight"] = 1.0 + _normal(seed, ln + ".weight", (dm,), 0.1)
            sd[ln + ".bias"] = _normal(seed, ln + ".bias", (dm,), 0.1)
    for prefix, dims in cfg.head_dims().items():
        for j, (o, i_) in enumerate(dims[:-1]):
            lin(f"{prefix}_mlp.affine_layers.{j}", o, i_)
        lin(f"{prefix}_fc", *dims[-1])
    return sd


def _np_qmul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def _np_aa2q(a):
    ang = np.linalg.norm(a, axis=-1, keepdims=True)
    s = np.where(ang < 1e-6, 0.5 - ang * ang / 48, np.sin(ang / 2) / np.maximum(ang, 1e-300))
    return np.concatenate((np.cos(ang / 2), a * s), -1)


def _np_q2mat(q):
    w, x, y, z = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), -1).reshape(q.shape[:-1] + (3, 3))


def make_stage1_train_batch(kind, B, window, seed=0, lengths=None):
    """A seeded reference-format training batch of a stage-1 estimator (what its DataLoader yields), for tests and benchmarks.

    'headnet' (HE:131-178, 310-345): of [B, window, 512], head_pose [B, window + 1, 7] (xyz, unit quaternion w,x,y,z), head_vels
    [B, window, 6] (linear | angular velocity), seq_len [B] (`lengths`, default window).  A smooth angular velocity (a few
    sinusoids, up to about 1.5 rad/s) is integrated the way va2rot does; the ground-truth rotations are that chain times a small
    random rotation (up to 0.3 rad) and the ground-truth velocities the smooth ones plus noise, so predicted and true rotations
    stay within about 1 rad of each other.  The features are a fixed random projection of (angular velocity, step length) plus
    noise: there is something to learn.  Feature rows past seq_len are zero; poses and velocities are given for every frame.
    'gravitynet' (HN:118-155, 334-342): head_rot_mat [B, window + 1, 3, 3], head_trans [B, window + 1, 3] (from the origin), both
    in a frame tilted against gravity by up to 0.5 rad, floor_normal [B, 3, 1] (the unit normal in that frame), seq_len [B] =
    window + 1 (`lengths` is not supported: the reference pads GravityNet's input for single sequences only)."""
    if kind not in ("headnet", "gravitynet"):
        raise ValueError(f"unknown stage-1 kind {kind!r}")
    r = _rng(seed, f"stage1_train_batch.{kind}")
    T = window
    t = np.arange(T + 1)[None, :, None] / 30.0
    amp, freq, ph = r.uniform(0.1, 0.5, (B, 1, 3, 3)), r.uniform(0.3, 2.0, (B, 1, 3, 3)), r.uniform(0, 2 * np.pi, (B, 1, 3, 3))
    va = (amp * np.sin(2 * np.pi * freq * t[..., None] + ph)).sum(-1)  # [B, T + 1, 3], body frame
    q = r.standard_normal((B, 4))
    q[:, 0] = np.abs(q[:, 0]) + 1.0
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    chain = [q]
    for i in range(T):
        zero = np.zeros((B, 1))
        conj = q * np.array([1.0, -1.0, -1.0, -1.0])
        angv = _np_qmul(_np_qmul(q, np.concatenate((zero, va[:, i]), -1)), conj)[:, 1:]
        n = _np_qmul(_np_aa2q(angv / 30.0), q)
        n = np.where(n[:, :1] < 0, -n, n)
        q = n / np.linalg.norm(n, axis=-1, keepdims=True)
        chain.append(q)
    chain = np.stack(chain, 1)  # [B, T + 1, 4]
    speed = r.uniform(0.2, 1.5, (B, 1, 1)) * (1 + 0.5 * np.sin(2 * np.pi * r.uniform(0.2, 1.0, (B, 1, 1)) * t + r.uniform(0, 6, (B, 1, 1))))
    heading = r.uniform(0, 2 * np.pi, (B, 1, 1)) + r.uniform(-1, 1, (B, 1, 1)) * t
    vel = np.concatenate((speed * np.cos(heading), speed * np.sin(heading), 0.05 * np.sin(3 * t + r.uniform(0, 6, (B, 1, 1)))), -1)
    trans = np.concatenate((np.zeros((B, 1, 3)), np.cumsum(vel[:, :-1], 1) / 30.0), 1)
    trans[..., 2] += 1.6
    if kind == "headnet":
        axis = r.standard_normal((B, T + 1, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        gt_q = _np_qmul(chain, _np_aa2q(axis * r.uniform(0.0, 0.3, (B, T + 1, 1))))
        gt_q[:, 0] = chain[:, 0]
        gt_q /= np.linalg.norm(gt_q, axis=-1, keepdims=True)
        head_vels = np.concatenate((vel[:, :T], va[:, :T] + 0.05 * r.standard_normal((B, T, 3))), -1)
        step = np.linalg.norm(trans[:, 1:] - trans[:, :-1], axis=-1, keepdims=True)
        proj = _rng(0, "stage1_train_batch.projection").standard_normal((4, 512)) * 0.5
        of = np.concatenate((va[:, :T], 30.0 * step), -1) @ proj + 0.3 * r.standard_normal((B, T, 512))
        seq_len = np.full(B, T) if lengths is None else np.asarray(lengths).reshape(B)
        if seq_len.min() < 0 or seq_len.max() > T:
            raise ValueError(f"lengths span {seq_len.min()}..{seq_len.max()}: 0..{T} expected")
        of = of * (np.arange(T)[None, :, None] < seq_len[:, None, None])  # feature rows past a sequence's end are zero padding
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
        return {"of": f32(of), "head_pose": f32(np.concatenate((trans, gt_q), -1)), "head_vels": f32(head_vels),
                "seq_len": torch.from_numpy(seq_len.astype(np.int64))}
    if lengths is not None:
        raise ValueError("lengths: GravityNet's training batches have window + 1 frames each")
    axis = r.standard_normal((B, 3))
    axis[:, 2] = 0.0
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    G = _np_q2mat(_np_aa2q(axis * r.uniform(0.05, 0.5, (B, 1))))  # the tilt of the SLAM frame against gravity
    rot = np.einsum("bij,btjk->btik", G, _np_q2mat(chain))
    tr0 = trans - trans[:, :1]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return {"head_rot_mat": f32(rot), "head_trans": f32(np.einsum("bij,btj->bti", G, tr0)),
            "floor_normal": f32(G[:, :, 2])[:, :, None], "seq_len": torch.full((B,), T + 1, dtype=torch.int64)}


# ------------------------------------------------------------------------------------------ stage 1's optical-flow CNN (ResNet-18)
FLOW_IMG = 224
FLOW_FEATS = 512


def flow_cnn_convs():
    """The 20 convolutions of torchvision's resnet18 in the order of the C ABI (egoego_flow_weights):
    [(conv name, BatchNorm name, c_in, c_out, kernel, stride, padding)] under the state-dict prefix of ResNet.resnet."""
    out = [("conv1", "bn1", 3, 64, 7, 2, 3)]
    cin = 64
    for li in range(1, 5):
        cout = 64 << (li - 1)
        for b in range(2):
            p = f"layer{li}.{b}."
            s = 2 if li > 1 and b == 0 else 1
            out.append((p + "conv1", p + "bn1", cin if b == 0 else cout, cout, 3, s, 1))
            out.append((p + "conv2", p + "bn2", cout, cout, 3, 1, 1))
            if li > 1 and b == 0:
                out.append((p + "downsample.0", p + "downsample.1", cin, cout, 1, 2, 0))
        cin = cout
    return out


def make_flows(n, seed=0):
    """n smooth ego-motion-like optical-flow fields [n, 224, 224, 2] float32 (pixels): a global translation, an in-plane rotation
    and a divergence (forward motion) about a random centre, plus three low-frequency sinusoids per channel; |flow| up to ~20 px."""
    g = np.random.default_rng([int(seed), 0xF10])
    ax = np.arange(FLOW_IMG, dtype=np.float64)
    yy, xx = np.meshgrid(ax, ax, indexing="ij")
    out = np.empty((n, FLOW_IMG, FLOW_IMG, 2), np.float32)
    for i in range(n):
        cx, cy = g.uniform(60, 164, 2)
        t = g.uniform(-6, 6, 2)
        w, d = g.uniform(-0.04, 0.04), g.uniform(-0.05, 0.05)
        u = t[0] - w * (yy - cy) + d * (xx - cx)
        v = t[1] + w * (xx - cx) + d * (yy - cy)
        for f in (u, v):
            for _ in range(3):
                a, fx, fy, ph = g.uniform(-1.5, 1.5), g.uniform(0.5, 2.0), g.uniform(0.5, 2.0), g.uniform(0, 2 * np.pi)
                f += a * np.sin(2 * np.pi * (fx * xx + fy * yy) / FLOW_IMG + ph)
        out[i, ..., 0], out[i, ..., 1] = u, v
    return out


def _flow_cnn_calibrate(sd, flows):
    """Set every BatchNorm's running statistics to the statistics of its input over `flows` (fp64 torch ops, eval-mode forward
    with the statistics already set upstream), so that the activations stay O(1) through the network as in a trained one."""
    F = torch.nn.functional
    x = torch.from_numpy(flows).double()
    x = torch.cat((x, torch.zeros(x.shape[:-1] + (1,), dtype=x.dtype)), -1).permute(0, 3, 1, 2)

    def conv_bn(x, conv, bn, stride, pad, relu):
        y = F.conv2d(x, sd[conv + ".weight"].double(), stride=stride, padding=pad)
        mean = y.mean(dim=(0, 2, 3))
        var = y.var(dim=(0, 2, 3), unbiased=True)
        sd[bn + ".running_mean"] = mean.float()
        sd[bn + ".running_var"] = var.float()
        y = F.batch_norm(y, mean.float().double(), var.float().double(), sd[bn + ".weight"].double(), sd[bn + ".bias"].double(),
                         False, 0.0, 1e-5)
        return F.relu(y) if relu else y

    convs = {c[0]: c for c in flow_cnn_convs()}
    x = F.max_pool2d(conv_bn(x, "conv1", "bn1", 2, 3, True), 3, 2, 1)
    for li in range(1, 5):
        for b in range(2):
            p = f"layer{li}.{b}."
            _, _, _, _, _, s, _ = convs[p + "conv1"]
            h = conv_bn(x, p + "conv1", p + "bn1", s, 1, True)
            h = conv_bn(h, p + "conv2", p + "bn2", 1, 1, False)
            idn = conv_bn(x, p + "downsample.0", p + "downsample.1", 2, 0, False) if (p + "downsample.0") in convs else x
            x = F.relu(h + idn)


def make_flow_cnn_weights(seed=0, prefix="cnn.resnet.", calib_frames=2):
    """Seeded synthetic state dict of the reference's FeatureExtractor (resnet.py; 122 keys under `prefix`).  The reference
    starts from ImageNet weights, which cannot be downloaded here.  Convolutions use torchvision's init (Kaiming normal, fan_out,
    ReLU gain); BatchNorm affines are perturbed like make_stage1_weights' LayerNorms (1 + N(0, 0.1), N(0, 0.1)); the running
    statistics are calibrated on make_flows(calib_frames) (fp64 torch ops); fc has PyTorch's default Linear init."""
    sd = {}
    for conv, bn, cin, cout, k, _, _ in flow_cnn_convs():
        sd[conv + ".weight"] = _normal(seed, "flow." + conv, (cout, cin, k, k), np.sqrt(2.0 / (cout * k * k)))
        sd[bn + ".weight"] = 1.0 + _normal(seed, "flow." + bn + ".weight", (cout,), 0.1)
        sd[bn + ".bias"] = _normal(seed, "flow." + bn + ".bias", (cout,), 0.1)
        sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    b = 1.0 / np.sqrt(FLOW_FEATS)
    sd["fc.weight"] = _uniform(seed, "flow.fc.weight", (FLOW_FEATS, FLOW_FEATS), b)
    sd["fc.bias"] = _uniform(seed, "flow.fc.bias", (FLOW_FEATS,), b)
    _flow_cnn_calibrate(sd, make_flows(calib_frames, 1000 + seed))
    return {prefix + k: v for k, v in sd.items()}


# ------------------------------------------------------------------------------------------ the SMPL-H body model
BODY_N_JOINTS = 52
_SMPLH_PARENTS_22 = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)
# rest offsets of the 22 body joints from their parents (metres, z up, arms along +-x): a rough adult in T-pose
_BODY_OFFSETS_22 = (
    (0, 0, 0.92), (0.07, 0, -0.09), (-0.07, 0, -0.09), (0, -0.02, 0.12), (0.03, 0, -0.39), (-0.03, 0, -0.39), (0, 0.02, 0.14),
    (-0.01, -0.03, -0.41), (0.01, -0.03, -0.41), (0, 0.01, 0.06), (0.02, 0.12, -0.06), (-0.02, 0.12, -0.06), (0, -0.02, 0.21),
    (0.08, -0.02, 0.12), (-0.08, -0.02, 0.12), (0, 0.04, 0.09), (0.10, -0.01, 0.04), (-0.10, -0.01, 0.04), (0.26, -0.01, -0.01),
    (-0.26, -0.01, -0.01), (0.25, 0, 0), (-0.25, 0, 0))


def body_model_parents():
    """The 52 parents of the SMPL-H tree: the 22 body joints, then 15 joints per hand (five fingers of three joints, each finger
    a chain from the wrist: joints 22-36 from the left wrist 20, joints 37-51 from the right wrist 21)."""
    par = list(_SMPLH_PARENTS_22)
    for wrist in (20, 21):
        for _ in range(5):
            par += [wrist, len(par), len(par) + 1]
    return np.asarray(par, np.int64)


def make_body_model(seed=0, n_verts=6890, n_faces=13776, max_weights=4):
    """A seeded model in the layout of SMPL-H's model.npz (the licensed files cannot be shipped), as a dict of numpy arrays:
    v_template (V, 3), shapedirs (V, 3, 16), posedirs (V, 3, 459), J_regressor (52, V), weights (V, 52), kintree_table (2, 52)
    uint32 and f (n_faces, 3) uint32.  The vertices sit around the bones of a 1.7 m T-pose skeleton; posedirs and shapedirs
    are uniform in +-1e-2; each J_regressor row averages a few vertices near its joint (rows sum to 1); every vertex has between
    1 and `max_weights` non-zero skinning weights (its own joint, then joints up and down the tree) that sum to 1, and vertex 0
    has exactly `max_weights`."""
    V, NJ = int(n_verts), BODY_N_JOINTS
    if V < NJ or not 1 <= max_weights <= NJ:
        raise ValueError("make_body_model: n_verts >= 52 and 1 <= max_weights <= 52 expected")
    g = np.random.default_rng([int(seed), 0xB0D1])
    par = body_model_parents()
    J = np.zeros((NJ, 3))
    for j in range(NJ):
        if j < 22:
            off = np.asarray(_BODY_OFFSETS_22[j], np.float64)
        else:  # fingers fan out from the wrist along the arm's direction
            side = 1.0 if j < 37 else -1.0
            k = (j - 22) % 15
            off = np.array([side * (0.035 if k % 3 else 0.08), 0.012 * (k // 3 - 2) if k % 3 == 0 else 0.0, 0.0])
        J[j] = off + (J[par[j]] if j else 0.0)
    owner = np.concatenate([np.arange(NJ), g.integers(0, NJ, V - NJ)])  # every joint owns at least one vertex
    radius = np.where(owner < 22, 0.06, 0.008)[:, None]
    along = g.uniform(0, 1, (V, 1)) * (J[owner] - J[np.maximum(par[owner], 0)]) * (owner > 0)[:, None]
    v_template = J[owner] - 0.5 * along + g.standard_normal((V, 3)) * radius
    shapedirs = g.uniform(-1e-2, 1e-2, (V, 3, 16))
    posedirs = g.uniform(-1e-2, 1e-2, (V, 3, 9 * (NJ - 1))).astype(np.float32)
    # J_regressor: up to eight of the vertices each joint owns
    J_regressor = np.zeros((NJ, V))
    for j in range(NJ):
        mine = np.flatnonzero(owner == j)[:8]
        w = g.uniform(0.5, 1.5, mine.size)
        J_regressor[j, mine] = w / w.sum()
    # skinning weights: the owner first, then its ancestors, then the remaining joints, in a seeded order
    weights = np.zeros((V, NJ))
    count = g.integers(1, max_weights + 1, V)
    count[0] = max_weights
    for v in range(V):
        chain, j = [], owner[v]
        while j >= 0:
            chain.append(j)
            j = par[j]
        if count[v] > len(chain):
            rest = np.setdiff1d(np.arange(NJ), chain)
            chain += list(g.permutation(rest))
        js = np.asarray(chain[:count[v]])
        w = g.uniform(0.2, 1.0, js.size) * np.r_[2.0, np.ones(js.size - 1)]
        weights[v, js] = w / w.sum()
    w32 = weights.astype(np.float32)
    f = g.integers(0, V, (int(n_faces), 3)).astype(np.uint32)
    kintree = np.stack([par, np.arange(NJ)]).astype(np.uint32)  # parents[0] = 2^32 - 1, as in the real file
    return {"v_template": v_template.astype(np.float32), "shapedirs": shapedirs.astype(np.float32), "posedirs": posedirs,
            "J_regressor": J_regressor.astype(np.float32), "weights": w32, "kintree_table": kintree, "f": f}


def make_body_poses(n_frames, n_joints=52, seed=0, amplitude=math.pi / 2, trans_scale=3.0):
    """Seeded poses for the body model: axis-angle [n_frames, n_joints, 3] with every component uniform in +-amplitude / sqrt(3)
    (angles up to `amplitude`) and translations [n_frames, 3] of a few metres, float32."""
    g = np.random.default_rng([int(seed), 0xB0D2])
    aa = g.uniform(-1, 1, (n_frames, n_joints, 3)) * (amplitude / math.sqrt(3.0))
    return aa.astype(np.float32), (g.standard_normal((n_frames, 3)) * trans_scale).astype(np.float32)


# ---------------------------------------------------------------- evaluation inputs
EVAL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)
# a stand-in 22-joint skeleton, z up, metres: the toes of the rest pose sit 0.93 below the hips
EVAL_REST_OFFSETS = (
    (0, 0, 0), (0.07, 0, -0.09), (-0.07, 0, -0.09), (0, 0, 0.11), (0, 0, -0.38), (0, 0, -0.38), (0, 0, 0.13), (0, 0, -0.40),
    (0, 0, -0.40), (0, 0, 0.05), (0, 0.12, -0.06), (0, 0.12, -0.06), (0, 0, 0.21), (0.08, 0, 0.12), (-0.08, 0, 0.12), (0, 0, 0.09),
    (0.10, 0, 0.03), (-0.10, 0, 0.03), (0.26, 0, 0), (-0.26, 0, 0), (0.25, 0, 0), (-0.25, 0, 0))
EVAL_CONTACT_JOINTS = (10, 11, 7, 8, 20, 21, 4, 5)  # toes, feet, hands, legs: the joints with a contact channel


def eval_fk(root_trans, local_aa, rest_offsets=EVAL_REST_OFFSETS, parents=EVAL_PARENTS):
    """fp64 forward kinematics by rotation matrices: root_trans [N, 3], local_aa [N, 22, 3] -> joints [N, 22, 3]."""
    aa = np.asarray(local_aa, np.float64)
    ang = np.linalg.norm(aa, axis=-1)[..., None, None]
    ax = aa / np.where(ang[..., 0] == 0, 1.0, ang[..., 0])
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    rest = np.asarray(rest_offsets, np.float64)
    G, P = [R[:, 0]], [np.broadcast_to(rest[0], (aa.shape[0], 3))]
    for j in range(1, 22):
        p = parents[j]
        P.append(np.einsum("nab,b->na", G[p], rest[j]) + P[p])
        G.append(G[p] @ R[:, j])
    return np.stack(P, 1) + np.asarray(root_trans, np.float64)[:, None]


def _eval_dbscan(h, eps=0.005, min_samples=3):
    """DBSCAN for 1-D points by its textbook definition (neighbour lists, clusters grown from the cores in input order), fp64."""
    n = h.size
    near = np.abs(h[:, None] - h[None, :]) <= eps
    core = near.sum(1) >= min_samples
    labels = np.full(n, -1)
    k = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = k
        stack = [i]
        while stack:
            c = stack.pop()
            if core[c]:
                for j in np.flatnonzero(near[c] & (labels == -1)):
                    labels[j] = k
                    stack.append(j)
        k += 1
    return labels


def assert_eval_margins(joints, fps=30, rel=1e-4):
    """Asserts, in fp64, that nothing determine_floor_height_and_contacts thresholds on `joints` [T, 22, 3] (float32 values) lies
    within a relative `rel` of its threshold, so that an exact comparison of its discrete outputs is no coin toss: the eight
    velocities against 0.005; every pairwise gap of static toe heights against eps = 0.005; the two smallest group medians against
    each other; the contact heights against 0.04 / 0.08; the terrain, root and size tests of the discard flag.  Returns the fp64
    floor height (None without a static sample)."""
    x = np.asarray(joints, np.float32).astype(np.float64)
    T = x.shape[0]
    assert T >= 2

    def clear(v, thr, what):
        v = np.asarray(v, np.float64)
        bad = np.abs(v - thr) < rel * abs(thr)
        assert not bad.any(), f"{what}: {v[bad][:3]} within {rel} of the threshold {thr}"

    vel = []
    for j in EVAL_CONTACT_JOINTS:
        v = np.linalg.norm(x[1:, j] - x[:-1, j], axis=1)
        vel.append(np.append(v, v[-1]))
    vel = np.stack(vel)
    clear(vel, 0.005, "a joint velocity")
    frames = np.arange(T)
    h = np.append(x[vel[0] < 0.005, 10, 2], x[vel[1] < 0.005, 11, 2])
    idx = np.append(frames[vel[0] < 0.005], frames[vel[1] < 0.005])
    if h.size == 0:
        floor = 0.0
    else:
        s = np.sort(h)
        for k in range(1, min(s.size, 64)):  # gaps of sorted samples k apart; they only grow with k
            g = s[k:] - s[:-k]
            clear(g, 0.005, "a gap of static heights")
            if g.min() > 0.005 * (1 + rel):
                break
        else:
            clear(np.abs(h[:, None] - h[None, :]), 0.005, "a gap of static heights")
        labels = _eval_dbscan(h)
        groups = np.unique(labels)
        med = np.array([np.median(h[labels == g]) for g in groups])
        root_med = np.array([np.median(x[np.unique(idx[labels == g]), 0, 2]) for g in groups])
        size = np.array([(labels == g).sum() for g in groups])
        order = np.argsort(med, kind="stable")
        floor = med[order[0]]
        if med.size > 1:
            assert med[order[1]] - floor > rel * max(abs(floor), 0.005), "the two smallest group medians are closer than the margin"
        clear(med - floor, 0.04, "a group median above the floor")
        clear(root_med - root_med[order[0]], 0.04, "a group's root median above the floor group's")
        assert not np.any(size == int(0.25 * fps) + 0.5)
    for k, j in enumerate(EVAL_CONTACT_JOINTS):
        clear(x[:, j, 2] - floor, 0.04 if k < 2 else 0.08, "a contact height")
    return floor if h.size else None


def make_eval_motion(B, T, seed=0, noise=0.05, fps=30, lengths=None, check=True):
    """Walking-like motions for the evaluation tests: a ground-truth sequence and B samples around it, as local axis-angle
    [.., T, 22, 3] and root translation [.., T, 3] over EVAL_REST_OFFSETS.  The body alternates stance phases (pose and root held
    for 4-9 frames, so the toes rest at the height the held pose gives them) and steps (linear moves of 5-9 frames, at least 4 cm
    per frame).  Sample b adds `noise` * (b + 1) / B of a seeded perturbation to the key poses and roots.

    Asserts (assert_eval_margins, on the fp64 joints rounded to float32, after the xy shift by the first frame's head, over each
    sample's `lengths[b]` frames) that no thresholded quantity lies within a relative 1e-4 of its threshold, and that the two
    smallest mpjpe values differ by more than that (`check=False` skips both, for timing runs: long sequences hold too many
    static samples for every pairwise gap to clear eps by chance).  Returns a dict of float32 numpy arrays: local_aa, root_trans, gt_local_aa,
    gt_root_trans, rest_offsets, and parents."""
    g = np.random.default_rng([int(seed), 0xE7A1])
    seg = []
    t = 0
    while t < T:
        hold, move = int(g.integers(4, 10)), int(g.integers(5, 10))
        seg.append((t, hold, move))
        t += hold + move
    nk = len(seg) + 1
    amp = np.full((22, 1), 0.12)
    amp[[1, 2, 4, 5, 7, 8]] = 0.3
    key_aa = g.uniform(-1, 1, (nk, 22, 3)) * amp
    key_root = np.zeros((nk, 3))
    key_root[:, 1] = np.arange(nk) * 0.45 + g.uniform(-0.05, 0.05, nk)
    key_root[:, 0] = g.uniform(-0.1, 0.1, nk)
    key_root[:, 2] = 0.93 + g.uniform(-0.02, 0.02, nk)
    d_aa, d_root = g.standard_normal((B, nk, 22, 3)), g.standard_normal((B, nk, 3))

    def expand(ka, kr):
        aa, root = np.zeros((T, 22, 3)), np.zeros((T, 3))
        for k, (t0, hold, move) in enumerate(seg):
            for i in range(hold + move):
                if t0 + i >= T:
                    break
                w = 0.0 if i < hold else (i - hold + 1) / (move + 1)
                aa[t0 + i] = (1 - w) * ka[k] + w * ka[k + 1]
                root[t0 + i] = (1 - w) * kr[k] + w * kr[k + 1]
        return aa.astype(np.float32), root.astype(np.float32)

    gt_aa, gt_root = expand(key_aa, key_root)
    aa, root = np.zeros((B, T, 22, 3), np.float32), np.zeros((B, T, 3), np.float32)
    lengths = [T] * B if lengths is None else [int(v) for v in lengths]
    rest32 = np.asarray(EVAL_REST_OFFSETS, np.float32)  # what a caller passes on
    gt_j = eval_fk(gt_root, gt_aa, rest32).astype(np.float32)
    gt_j[:, :, :2] -= gt_j[0, 15, :2].copy()
    mpjpe = []
    for b in range(B):
        s = noise * (b + 1) / B
        aa[b], root[b] = expand(key_aa + s * d_aa[b] * amp, key_root + s * 0.3 * d_root[b])
        if not check:
            continue
        L = lengths[b]
        j = eval_fk(root[b, :L], aa[b, :L], rest32).astype(np.float32)
        j[:, :, :2] -= j[0, 15, :2].copy()
        assert_eval_margins(j, fps)
        e = (j.astype(np.float64) - j[:, :1]) - (gt_j[:L].astype(np.float64) - gt_j[:L, :1])
        mpjpe.append(np.linalg.norm(e, axis=2).mean() * 1000)
    if B > 1 and check:
        lo = np.sort(mpjpe)[:2]
        assert lo[1] - lo[0] > 1e-4 * lo[1], "the two smallest mpjpe values are closer than the margin"
    return {"local_aa": aa, "root_trans": root, "gt_local_aa": gt_aa, "gt_root_trans": gt_root,
            "rest_offsets": rest32, "parents": EVAL_PARENTS}
