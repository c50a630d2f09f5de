"""Stage-1 training on the GPU (egoego_s1_train_*, egoego_s1_headnet_loss; egoego_release_amd/stage1_train.py): the loss kernel on
planted heads, the training encode and its gradients against the oracle of tests/stage1_train_oracle.py, the run-to-run and
batch-composition properties, the modules' hip_training path, and a short run of Stage1Trainer.  (The side-stream check is
tests/test_gpu_streams_stage1_train.py.)

The loss kernel and the oracle are both fp64 on the same fp32 inputs: loss parts and d_heads agree within 1e-9 of each tensor's
largest magnitude (three orders above the fp64 rounding of a few hundred operations).  A gradient comparison means nothing at the
two sign kinks (the standardisation of a chain product, and of the difference quaternion), so every fixture asserts on the CPU that
both real parts stay at least 1e-3 away from zero.

The gradient bar of the encode, per parameter tensor p, for the same inputs and the HIP path's ReLU and dropout decisions forced:
    e_hip(p) <= 2 * (e_emul(p) + e_32(p)),     e(p) = |g(p) - g64(p)|_2 / |g64(p)|_2
(e_emul: every product of the oracle as split-bf16, forward and backward; e_32: the oracle in fp32), the bar of test_gpu_train.py.
A tensor whose exact gradient is zero (w_k.bias always: softmax does not see a shift of all keys of a query; the whole query / key
projection at window 1) is judged by |g_hip(p)| <= 1e-6 |g64|_global.

EGOEGO_S1_TRAIN_RECORD=<file>: the measured ratios, forward errors and the two loss curves are written there as JSON
(profiles/stage1_train_grad_error.json is such a file).
"""
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_train_oracle as O
from egoego_release_amd import _lib, stage1, stage1_train
from egoego_release_amd.synthetic import make_stage1_train_batch
from egoego_release_amd.trainer import Stage1Trainer

pytestmark = pytest.mark.gpu

_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_S1_TRAIN_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _opt(window, layers):
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                     w_rotation=1.0, w_va=0.7, w_dist=0.4)


def _module(kind, window, layers):
    cls = stage1.HeadFormer if kind == "headnet" else stage1.HeadNormalFormer
    return cls(_opt(window, layers), torch.device("cuda")).cuda()


# ================================================================================================ the loss kernel alone
W_ROT, W_VA, W_DIST, DIST_SCALE = 1.0, 0.7, 0.4, 10.0


def _planted(B, window, T, seed):
    """Planted heads around a synthetic batch's own velocities and step lengths: (heads [B, window, 4] with garbage past T, head_pose
    [B, T + 1, 7], head_vels [B, T, 6]), fp32 on the CPU."""
    d = make_stage1_train_batch("headnet", B, max(T, 2), seed=seed)
    pose, vels = d["head_pose"][:, :T + 1].clone(), d["head_vels"][:, :T].clone()
    g = torch.Generator().manual_seed(100 + seed)
    heads = torch.randn(B, window, 4, generator=g)
    heads[:, :T, :3] = vels[..., 3:] + 0.3 * torch.randn(B, T, 3, generator=g)
    heads[:, :T, 3] = DIST_SCALE * (pose[:, 1:, :3] - pose[:, :-1, :3]).norm(dim=-1) + 0.2 * torch.randn(B, T, generator=g)
    return heads, pose, vels


def _check_loss(name, heads, pose, vels, T):
    B, window, _ = heads.shape
    ref, dref, r = O.headnet_loss_and_grad(heads, T, pose, vels, DIST_SCALE, W_ROT, W_VA, W_DIST)
    # the two sign kinks (CPU preconditions)
    assert float(r["chain_real"].abs().min()) >= 1e-3, ("chain product too close to a sign flip", float(r["chain_real"].abs().min()))
    assert float(r["diff_real"].abs().min()) >= 1e-3, ("difference quaternion too close to a sign flip", float(r["diff_real"].abs().min()))
    loss, d32, d64 = stage1_train.headnet_loss(heads.cuda(), T, pose.cuda(), vels.cuda(), DIST_SCALE, W_ROT, W_VA, W_DIST, want_fp64_grad=True)
    loss, d32, d64 = loss.cpu(), d32.cpu(), d64.cpu()
    e_loss = float((loss - ref).abs().max() / ref.abs().max())
    e_grad = float((d64 - dref).abs().max() / dref.abs().max())
    print(f"{name}: loss parts {loss.tolist()}  rel err {e_loss:.2e}; d_heads rel err {e_grad:.2e}")
    _record("loss " + name, loss_err=e_loss, grad_err=e_grad)
    assert e_loss <= 1e-9 and e_grad <= 1e-9
    assert torch.equal(d64[:, T:], torch.zeros_like(d64[:, T:])) and torch.equal(d32[:, T:], torch.zeros_like(d32[:, T:]))
    assert torch.equal(d32, d64.float())
    return loss, d64


@pytest.mark.parametrize("name,B,window,T", [("T=1", 3, 4, 1), ("T=window=128", 2, 128, 128), ("T<window", 3, 16, 9), ("B=1", 1, 12, 12),
                                              ("B=33", 33, 10, 7)])
def test_headnet_loss_on_planted_heads(name, B, window, T):
    heads, pose, vels = _planted(B, window, T, seed=1)
    heads[:, T:] = float("nan")  # rows past T are never read
    _check_loss(name, heads, pose, vels, T)


def test_headnet_loss_zero_and_tiny_angular_velocity():
    """A frame with va exactly 0 and one whose rotation angle is below axis_angle_to_quaternion's 1e-6 threshold (its Taylor branch):
    loss and gradient against the oracle; the gradient at va = 0 is not zero (d(a * s)/da = s = 1/2 there)."""
    heads, pose, vels = _planted(2, 8, 8, seed=2)
    heads[0, 3, :3] = 0.0
    heads[1, 5, :3] = torch.tensor([1e-6, -2e-6, 5e-7])  # angle = |va| / 30 < 1e-6
    _, d = _check_loss("zero / tiny va", heads, pose, vels, 8)
    assert float(d[0, 3, :3].abs().max()) > 0 and bool(torch.isfinite(d).all())


def test_headnet_loss_negated_ground_truth_is_the_same_rotation():
    heads, pose, vels = _planted(3, 8, 8, seed=3)
    a, da = _check_loss("gt", heads, pose, vels, 8)
    neg = pose.clone()
    neg[:, 1:, 3:] = -neg[:, 1:, 3:]
    b, db = _check_loss("gt = -q", heads, neg, vels, 8)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()) and float((da - db).abs().max()) <= 1e-12 * float(da.abs().max())


def test_headnet_loss_is_repeatable_and_refuses_bad_shapes():
    heads, pose, vels = _planted(5, 16, 9, seed=4)
    a = stage1_train.headnet_loss(heads.cuda(), 9, pose.cuda(), vels.cuda(), DIST_SCALE, W_ROT, W_VA, W_DIST, want_fp64_grad=True)
    b = stage1_train.headnet_loss(heads.cuda(), 9, pose.cuda(), vels.cuda(), DIST_SCALE, W_ROT, W_VA, W_DIST, want_fp64_grad=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        stage1_train.headnet_loss(heads.cuda(), 17, pose.cuda(), vels.cuda(), DIST_SCALE, W_ROT, W_VA, W_DIST)
    with pytest.raises(_lib.EgoEgoHipError):
        stage1_train.headnet_loss(heads, 9, pose, vels, DIST_SCALE, W_ROT, W_VA, W_DIST)


# ================================================================================================ the training encode
class Rig:
    """One module on the GPU with its training engine; sd = the CPU state dict of its parameters."""

    def __init__(self, kind, window, layers):
        self.kind, self.window, self.layers = kind, window, layers
        self.model = _module(kind, window, layers)
        self.sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        self.engine = self.model.train_engine()
        self.d_feats = self.model.cfg.d_feats

    def tensors(self):
        return {n: p.detach() for n, p in self.model.named_parameters()}

    def step(self, feats, valid, upstream, p_drop=0.0, seed=0, window_ids=None, saves=None):
        """forward + backward on the engine -> (heads, grads, saves)"""
        ts = self.tensors()
        heads, saves = self.engine.forward(ts, feats.cuda(), torch.as_tensor(valid).cuda(), p_drop, seed, window_ids, saves)
        grads = self.engine.backward(ts, saves, upstream.cuda(), feats.shape[0], p_drop, seed)
        return heads, grads, saves


_RIGS = {}


def rig(kind, window, layers):
    key = (kind, window, layers)
    if key not in _RIGS:
        _RIGS[key] = Rig(kind, window, layers)
    return _RIGS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_rigs():
    yield
    _RIGS.clear()


def inputs(kind, W, window, valid=None, seed=0):
    """(feats [W, window, F] with NaN in the rows past valid, valid [W], a random upstream gradient of the heads), on the CPU."""
    g = torch.Generator().manual_seed(500 + seed)
    F = 512 if kind == "headnet" else 18
    feats = torch.randn(W, window, F, generator=g)
    valid = torch.tensor([window] * W if valid is None else valid, dtype=torch.int32)
    feats[torch.arange(window)[None, :] >= valid[:, None]] = float("nan")  # what the padded rows hold is never read
    up = torch.randn((W, window, 4) if kind == "headnet" else (W, 3), generator=g)
    return feats, valid, up


def _decisions(on_hip_values, pre64):
    """The HIP path's ReLU decisions against fp64's: every one that differs sits inside the forward error of its tensor.
    -> (mask, flips, count)"""
    h = on_hip_values.double()
    on_hip, on_64 = h > 0, pre64 > 0
    both = on_hip & on_64
    err = float((h - pre64)[both].abs().max()) if both.any() else 0.0
    flip = on_hip != on_64
    if flip.any():
        assert float(pre64[flip].abs().max()) <= max(err, 1e-6), err
    return on_hip, int(flip.sum()), flip.numel()


def check_parity(name, kind, W, window, layers, valid=None, p_drop=0.0):
    R = rig(kind, window, layers)
    eng = R.engine
    feats, valid, up = inputs(kind, W, window, valid)
    seed = 4242
    heads, grads, saves = R.step(feats, valid, up, p_drop, seed)
    masks = None
    if p_drop > 0:
        masks = {(l, s): eng.dropout_mask(p_drop, seed, l, s, W).cpu() for l in range(layers) for s in ("attn", "fc", "ffn")}
    hidden = [eng.saved(saves, W, l, "ffn_hidden").cpu() for l in range(layers)]
    lin = O.head_linear_names(kind)
    head_hidden = {nm: eng.saved(saves, W, j, "head_hidden").cpu() for j, nm in enumerate(lin) if not nm.endswith("_fc")}
    heads = heads.cpu().double()
    grads = {k: v.cpu().double() for k, v in grads.items()}
    clean = torch.nan_to_num(feats, nan=0.0)
    kw = dict(p_drop=p_drop, drop_masks=masks)

    # ---- forward: fp64, nothing forced
    with torch.no_grad():
        r64 = O.encode(O.leaves(R.sd), kind, clean, valid, layers, **kw)
    e_fwd = float((heads - r64["heads"]).abs().max() / r64["heads"].abs().max())
    print(f"{name}: max|heads - heads64| / max|heads64| = {e_fwd:.3e}")
    assert e_fwd < 1e-4

    # ---- the kinks
    relu_masks, head_masks, n_flip, n_all = [], {}, 0, 0
    for l in range(layers):
        m, f, n = _decisions(hidden[l], r64["ffn_pre"][l])
        relu_masks.append(m)
        n_flip, n_all = n_flip + f, n_all + n
    for nm, h in head_hidden.items():
        m, f, n = _decisions(h.reshape(r64["head_pre"][nm].shape), r64["head_pre"][nm])
        head_masks[nm] = m
        n_flip, n_all = n_flip + f, n_all + n
    print(f"{name}: {n_flip} of {n_all} ReLU decisions differ from fp64")
    assert n_flip <= 1e-4 * n_all + 1

    # ---- gradients with the HIP decisions forced: fp64, emulated split-bf16, fp32
    kw.update(relu_masks=relu_masks, head_masks=head_masks)
    args = (R.sd, kind, clean, valid, layers, up)
    _, g64 = O.heads_and_grads(*args, **kw)
    _, gem = O.heads_and_grads(*args, mm=O.split_mm, **kw)
    _, g32 = O.heads_and_grads(*args, dtype=torch.float32, **kw)
    assert sorted(g64) == sorted(grads)
    total = math.sqrt(sum(float(g.norm()) ** 2 for g in g64.values()))
    ratios, over = {}, []
    for k, ref in g64.items():
        g = grads[k].reshape(ref.shape)
        assert bool(torch.isfinite(g).all()), k
        if float(ref.norm()) <= 1e-9 * total:  # zero in exact arithmetic
            assert k.endswith("w_k.bias") or window == 1 or int(valid.max()) == 0, k
            ratios[k] = float(g.norm()) / total
            if not float(g.norm()) <= 1e-6 * total:
                over.append((k, ratios[k]))
            continue
        e_hip, e_em, e_32 = O.rel_err(g, ref), O.rel_err(gem[k], ref), O.rel_err(g32[k], ref)
        ratios[k] = e_hip / (e_em + e_32)
        if not e_hip <= 2 * (e_em + e_32):
            over.append((k, e_hip, e_em, e_32))
    worst = sorted(((v, k) for k, v in ratios.items()), reverse=True)[:3]
    print(f"{name}: worst e_hip / (e_emul + e_32): " + ", ".join(f"{k} {v:.2f}" for v, k in worst))
    _record(name, heads_err=e_fwd, decisions_flipped=n_flip, decisions=n_all, ratios=ratios)
    assert not over, over


# name: (kind, W, window, layers, valid)
CASES = {
    "h 3x11": ("headnet", 3, 11, 2, [0, 1, 11]),    # valid of 0, 1 and window in one batch; 33 rows: no multiple of 8
    "h 2x33": ("headnet", 2, 33, 2, [33, 20]),      # crosses a 32-row tile
    "h 2x65": ("headnet", 2, 65, 1, None),          # the softmax's second 64-key strip
    "h 1x128": ("headnet", 1, 128, 1, None),        # the longest window
    "h 5x1": ("headnet", 5, 1, 1, None),            # one token: softmax over one key
    "h 19x27": ("headnet", 19, 27, 1, None),        # 513 rows: one past a gradient chunk
    "h 257x2": ("headnet", 257, 2, 1, None),        # 514 rows: two past
    "g 3x11": ("gravitynet", 3, 11, 2, [0, 1, 11]),  # d_feats 18: k no multiple of 8, rows not 16-byte aligned
    "g 2x120": ("gravitynet", 2, 120, 1, [120, 47]),
}


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("name", ["h 3x11", "h 2x33", "g 3x11", "g 2x120"])
def test_parity(name, p_drop):
    kind, W, window, layers, valid = CASES[name]
    check_parity(f"{name} p={p_drop}", kind, W, window, layers, valid, p_drop)


@pytest.mark.parametrize("name", ["h 2x65", "h 1x128", "h 5x1"])
def test_parity_window_edges(name):
    kind, W, window, layers, valid = CASES[name]
    check_parity(name, kind, W, window, layers, valid, 0.1 if name == "h 2x65" else 0.0)


@pytest.mark.parametrize("name", ["h 19x27", "h 257x2"])
def test_parity_past_a_gradient_chunk(name):
    kind, W, window, layers, valid = CASES[name]
    assert W * window == _lib.TRAIN_GRAD_CHUNK + (1 if name == "h 19x27" else 2)
    check_parity(name, kind, W, window, layers, valid)


# ------------------------------------------------------------------------------------------------ properties
def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind", ["headnet", "gravitynet"])
def test_bitwise_repeatable_and_workspace_blind(kind):
    """Two runs give the same bits, and so does a run whose workspace and saves held a NaN pattern on entry."""
    R = rig(kind, 11, 2)
    feats, valid, up = inputs(kind, 3, 11, [11, 4, 0])
    h0, g0, _ = R.step(feats, valid, up, 0.1, 9)
    h1, g1, _ = R.step(feats, valid, up, 0.1, 9)
    assert torch.equal(h0, h1) and _same(g0, g1)
    R.engine._ws.fill_(0xFF)
    saves = R.engine.new_saves(3).fill_(0xFF)
    h2, g2, _ = R.step(feats, valid, up, 0.1, 9, saves=saves)
    assert bool(torch.isfinite(h2).all()) and torch.equal(h0, h2) and _same(g0, g2)
    h3, _, _ = R.step(feats, valid, up, 0.1, 10)
    assert not torch.equal(h0, h3)


@pytest.mark.parametrize("kind", ["headnet", "gravitynet"])
def test_a_window_does_not_depend_on_the_batch(kind):
    """A window's rows of the heads are the same bits alone, in a pair and in the batch (under its own dropout stream); its
    contribution to the gradients (the upstream zero elsewhere) is that of the window alone up to the order of fp32 sums."""
    R = rig(kind, 11, 2)
    feats, valid, up = inputs(kind, 3, 11, [11, 5, 8])
    ids = [7, 3, 2 ** 40 + 1]
    heads, _, _ = R.step(feats, valid, up, 0.1, 5, window_ids=ids)
    for b in range(3):
        alone, g_alone, _ = R.step(feats[b:b + 1], valid[b:b + 1], up[b:b + 1], 0.1, 5, window_ids=ids[b:b + 1])
        assert torch.equal(alone[0], heads[b]), b
        only = torch.zeros_like(up)
        only[b] = up[b]
        _, g_in, _ = R.step(feats, valid, only, 0.1, 5, window_ids=ids)
        total = math.sqrt(sum(float(g.double().norm()) ** 2 for g in g_alone.values()))
        for k in g_alone:
            assert float((g_in[k].double() - g_alone[k].double()).norm()) <= 1e-5 * max(float(g_alone[k].double().norm()), 1e-3 * total), (b, k)
    pair, _, _ = R.step(feats[[2, 0]], valid[[2, 0]], up[[2, 0]], 0.1, 5, window_ids=[ids[2], ids[0]])
    assert torch.equal(pair[0], heads[2]) and torch.equal(pair[1], heads[0])


def test_upstream_gradient_scales_exactly():
    R = rig("headnet", 11, 2)
    feats, valid, up = inputs("headnet", 3, 11, [11, 5, 1])
    _, g1, _ = R.step(feats, valid, up, 0.1, 1)
    _, g2, _ = R.step(feats, valid, up * 65536.0, 0.1, 1)
    for k in g1:
        assert torch.equal(g1[k] * 65536.0, g2[k]), k


# ------------------------------------------------------------------------------------------------ dropout masks
M0, M1, PW0, PW1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(ctr, key):
    """Random123's Philox4x32-10: ctr four uint32 arrays (broadcast), key two uint32 -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PW0) & MASK32, (k1 + PW1) & MASK32
    return np.stack([c.astype(np.uint32) for c in (c0, c1, c2, c3)], -1)


def _keyed_mask(p, seed, layer, site, wid, n):
    """keep flags of elements 0..n-1 of window `wid`: draw (e >> 2; wid; layer * 4 + site) under the seed, word e & 3, kept when
    it is at least p * 2^32."""
    thr = np.uint32(int(float(np.float32(p)) * 4294967296.0))
    e4 = np.arange((n + 3) // 4, dtype=np.uint64)
    r = _philox4x32_10((e4, wid & 0xFFFFFFFF, wid >> 32, layer * 4 + site), (seed & 0xFFFFFFFF, seed >> 32))
    return (r.reshape(-1)[:n] >= thr)


def test_dropout_masks_are_the_keyed_philox_draw():
    R = rig("headnet", 11, 2)
    eng, W, L, p = R.engine, 3, 11, 0.1
    ids = [5, 900, 2 ** 40 + 1]
    seed = 2 ** 33 + 17
    for layer, site in ((0, "attn"), (0, "fc"), (1, "ffn")):
        m = eng.dropout_mask(p, seed, layer, site, W, window_ids=ids).cpu()
        assert m.shape == ((W, 4, L, L) if site == "attn" else (W, L, 256))
        for b in range(W):
            want = _keyed_mask(p, seed, layer, stage1_train.SITES[site], ids[b], m[b].numel())
            assert np.array_equal(m[b].numpy().reshape(-1), want), (layer, site, b)
            kept = float(m[b].float().mean())
            assert abs(kept - 0.9) <= 4 * math.sqrt(0.09 / m[b].numel())
    assert torch.equal(eng.dropout_mask(p, 1, 0, "fc", 2).cpu()[1], eng.dropout_mask(p, 1, 0, "fc", 1, window_ids=[1]).cpu()[0])
    assert bool(eng.dropout_mask(0.0, 1, 0, "fc", W).all())  # p = 0: every value kept
    # (that the forward and backward passes apply exactly these masks is test_parity's p = 0.1 half: the oracle is handed them)


# ------------------------------------------------------------------------------------------------ the modules
def _grads(m):
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


@pytest.mark.parametrize("kind", ["headnet", "gravitynet"])
def test_module_backward_fills_every_trainable_gradient(kind):
    """hip_training = True; out = m(data); loss, *_ = m.compute_loss(out, data); loss.backward(): .grad of every trainable tensor,
    against the fp64 oracle's forward + compute_loss + backward on the same batch (eval(): no dropout)."""
    window, layers, B = 8, 1, 3
    m = _module(kind, window, layers)
    m.hip_training = True
    m.eval()
    data = make_stage1_train_batch(kind, B, window, seed=3, lengths=(8, 5, 1) if kind == "headnet" else None)
    out = m(data)
    parts = m.compute_loss(out, data)
    parts[0].backward()
    got = _grads(m)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert sorted(got) == sorted(O.trainable(sd)) and m.action_transformer.position_vec.weight.grad is None
    if kind == "headnet":
        ls, lv, heads, _ = O.headnet_step(sd, data, m.opt, layers)
        ref = [ls[k] for k in ("loss", "orient", "va", "dist")]
        assert not out["head_rot_quat"].requires_grad and out["head_va"].requires_grad and out["head_dist_scalar"].requires_grad
    else:
        import stage1_oracle as S1
        feats = torch.stack([S1.gravity_features(data["head_rot_mat"][b], data["head_trans"][b], window)[0] for b in range(B)])
        loss, lv, heads, _ = O.gravity_step(sd, feats, [window] * B, data["floor_normal"], layers)
        ref = [loss, loss]
    # the heads are within 1e-4 of their largest value (the forward bar); a loss part is a mean of at most quadratic terms of them
    for a, b in zip(parts, ref):
        a, b = float(a.detach()), float(b.detach())
        assert abs(a - b) <= 1e-3 * abs(b), (a, b)
    total = math.sqrt(sum(float(lv[k].grad.norm()) ** 2 for k in got))
    err2, worst = 0.0, 0.0
    for k, g in got.items():
        r = lv[k].grad
        assert g.shape == m.state_dict()[k].shape and bool(torch.isfinite(g).all()), k
        err2 += float((g.double().cpu().reshape(r.shape) - r).norm()) ** 2
        if float(r.norm()) > 1e-9 * total:
            worst = max(worst, O.rel_err(g.reshape(r.shape), r))
    print(f"{kind}: gradient error against fp64: whole {math.sqrt(err2) / total:.2e}, worst tensor {worst:.2e}")
    # The per-tensor bar with forced decisions is test_parity's.  Here nothing is forced: beside the products' rounding (1e-5 to
    # 1e-4) a handful of the 1e4 ReLU decisions may differ from fp64, each moving the gradient by the order of its share; the
    # whole gradient is held to 1e-2 of its norm and every tensor to 1e-1 of its own, which a wrong or missing term cannot meet.
    assert math.sqrt(err2) <= 1e-2 * total and worst <= 1e-1


def test_two_graphs_outstanding():
    """Two forwards, then the two backwards in either order, accumulate what two sequential steps do; loss / 2 halves."""
    m = _module("headnet", 8, 1)
    m.hip_training = True
    m.eval()
    d1, d2 = make_stage1_train_batch("headnet", 3, 8, seed=1), make_stage1_train_batch("headnet", 3, 8, seed=2)
    loss = lambda d: m.compute_loss(m(d), d)[0]  # noqa: E731
    la = loss(d1); la.backward(); lb = loss(d2); lb.backward()
    seq = _grads(m)
    for order in ((0, 1), (1, 0)):
        ls = [loss(d1), loss(d2)]
        assert torch.equal(ls[0], la) and torch.equal(ls[1], lb)
        for i in order:
            ls[i].backward()
        assert _same(seq, _grads(m)), order
    (loss(d1) / 2).backward()
    half = _grads(m)
    loss(d1).backward()
    full = _grads(m)
    assert all(torch.equal(half[k] * 2, full[k]) for k in full)


def test_optimizer_step_is_seen_and_eval_mode_has_no_dropout():
    m = _module("headnet", 8, 1)
    m.hip_training = True
    m.eval()
    d = make_stage1_train_batch("headnet", 3, 8, seed=1)
    ev = dict(d, aligned_slam_trans=d["head_pose"][..., :3])
    with torch.no_grad():
        e0 = m.forward_for_eval(ev)["head_va"].clone()  # packs the inference engine's copy of the initial weights
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    l0 = m.compute_loss(m(d), d)[0]
    assert torch.equal(l0, m.compute_loss(m(d), d)[0])  # eval(): no dropout, the same bits
    l0.backward()
    opt.step()
    l1 = m.compute_loss(m(d), d)[0]
    assert float(l1.detach()) < float(l0.detach())  # one step on the same batch
    fresh = _module("headnet", 8, 1)
    fresh.load_state_dict(m.state_dict())
    fresh.hip_training = True
    fresh.eval()
    assert torch.equal(fresh.compute_loss(fresh(d), d)[0], l1)  # no stale copy of the old weights anywhere
    with torch.no_grad():
        e1 = m.forward_for_eval(ev)["head_va"]
        assert not torch.equal(e0, e1) and torch.equal(e1, fresh.forward_for_eval(ev)["head_va"])
        # validation: compute_loss under no_grad, on the inference encode
        lv = m.compute_loss(m(d), d)
        assert not lv[0].requires_grad and abs(float(lv[0]) - float(l1.detach())) <= 1e-3 * float(l1.detach())
    m.train()
    a, b = m(d)["head_va"], m(d)["head_va"]
    assert not torch.equal(a, b)  # dropout on, one fresh seed per forward
    m.hip_training = False
    assert not m(d)["head_va"].requires_grad


# ------------------------------------------------------------------------------------------------ a short run
def _oracle_run(sd, batches, opt, layers, steps, lr=1e-4):
    lv = O.leaves(sd)
    params = [lv[k] for k in O.trainable(lv)]
    optim = torch.optim.AdamW(params, lr=lr)
    curve = []
    for it in range(steps):
        d = batches[it % len(batches)]
        r = O.encode(lv, "headnet", d["of"].double(), d["seq_len"], layers)
        h = r["heads"]
        ls = O.headnet_loss(h[..., :3], h[..., 3:4], d["head_pose"], d["head_vels"], opt.dist_scale, opt.w_rotation, opt.w_va, opt.w_dist)
        optim.zero_grad()
        ls["loss"].backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0, error_if_nonfinite=False)
        optim.step()
        curve.append(float(ls["loss"].detach()))
    return curve


def test_forty_steps_of_the_trainer(tmp_path):
    """B = 4, window 16, 1 layer, eval() mode (no dropout), Stage1Trainer: the loss falls by at least half of what the fp64 oracle's
    run falls on the same data (a sanity condition, not a measurement); the checkpoint loads into a fresh HeadFormer."""
    window, layers, steps = 16, 1, 40
    m = _module("headnet", window, layers)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    batches = [make_stage1_train_batch("headnet", 4, window, seed=s) for s in range(4)]
    tr = Stage1Trainer(m, batches, save_dir=str(tmp_path), save_interval=10)
    m.eval()
    curve = []
    for ep in range(steps // len(batches)):
        tr.epoch += 1
        for d in batches:
            curve.append(tr.step(d)[0])
    curve = torch.stack(curve).cpu().tolist()
    ref = _oracle_run(sd, batches, m.opt, layers, steps)
    k = len(batches)
    first, last = sum(curve[:k]) / k, sum(curve[-k:]) / k
    rfirst, rlast = sum(ref[:k]) / k, sum(ref[-k:]) / k
    print(f"HIP: {first:.4f} -> {last:.4f}; fp64 oracle: {rfirst:.4f} -> {rlast:.4f}")
    _record("forty steps", hip=curve, oracle=ref)
    assert rlast < rfirst and first - last >= 0.5 * (rfirst - rlast)
    path = tr.save(tr.epoch)
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "transformer_encoder_state_dict"]
    fresh = stage1.HeadFormer(_opt(window, layers), torch.device("cuda"))
    fresh.load_state_dict(ck["transformer_encoder_state_dict"])


def test_the_training_tool_writes_a_loadable_checkpoint(tmp_path, capsys):
    """tools/train_stage1.py on seeded synthetic batches (in this process: the test is about the tool's loop, not its start-up)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_stage1_tool", os.path.join(root, "tools", "train_stage1.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for kind in ("headnet", "gravitynet"):
        out = tmp_path / kind
        tool.main(["--kind", kind, "--save_dir", str(out), "--epochs", "2", "--window", "8", "--n_dec_layers", "1", "--batch_size", "2",
                   "--synthetic_batches", "2", "--save_interval", "2"])
        lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
        assert [l["epoch"] for l in lines[:2]] == [1, 2] and lines[1]["train"]["loss"] < lines[0]["train"]["loss"] and "val" in lines[0]
        ck = torch.load(out / "weights" / "train-2.pt", map_location="cpu", weights_only=True)
        assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "transformer_encoder_state_dict"]
        cls = stage1.HeadFormer if kind == "headnet" else stage1.HeadNormalFormer
        cls(_opt(8, 1), torch.device("cuda")).load_state_dict(ck["transformer_encoder_state_dict"])
