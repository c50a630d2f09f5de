"""GravityNet's training batches on the GPU (egoego_s1_gravity_batch; egoego_release_amd/stage1_data.py): planted draws against the
fp64 oracle of tests/gravity_batch_oracle.py, the Philox draws against its numpy replica, batch independence, HeadNormalFormer's
forward with `lengths`, and Stage1Trainer over GravityBatches.  (The side-stream check is tests/test_gpu_streams_stage1_data.py.)

The bar of every float output, per tensor and sample: with e(x) the largest distance of x from the fp64 oracle in units of
eps_fp32 * max|tensor|,
    e_hip <= 2 * e_ref32 + 1,
e_ref32 being the oracle's reference mode (fp32, the reference's operation order, the serial sum) on the same inputs.  seq_len,
start_t_idx, aug_scale, ori_head_pose and the padding's zeros are exact.

EGOEGO_S1_DATA_RECORD=<file>: the measured e values are written there as JSON (profiles/stage1_data_error.json is such a file).
"""
import ctypes as C
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import gravity_batch_oracle as O
import stage1_oracle as S1
import stage1_train_oracle as TO
from egoego_release_amd import _lib, stage1, stage1_data
from egoego_release_amd.trainer import Stage1Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gravity_batch_golden.npz")
SEED = 2 ** 33 + 5
_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_S1_DATA_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------- fixtures
def make_seq(n, seed, qnorm=1.0):
    """[n, 7] float32: a random walk of positions around head height and of quaternions of norm `qnorm`."""
    g = np.random.default_rng(1000 + seed)
    trans = np.cumsum(g.normal(0.0, 0.02, (n, 3)), 0) + g.normal(0.0, 1.0, (1, 3)) + np.array([0.0, 0.0, 1.6])
    q = g.normal(0.0, 1.0, (1, 4)) + np.cumsum(g.normal(0.0, 0.05, (n, 4)), 0)
    q *= qnorm / np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([trans, q], 1).astype(np.float32)


def random_rr(n, seed):
    g = np.random.default_rng(2000 + seed)
    return np.stack([O.random_rotation_from_normals(g.normal(size=4), np.float64)[1] for _ in range(n)]).astype(np.float32)


def pack(seqs):
    """-> (pose [N, 7] on the GPU, offsets as a host list)"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    return torch.from_numpy(np.concatenate(seqs, 0)).cuda(), off.tolist()


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items() if isinstance(v, torch.Tensor)}


def check_planted(name, seqs, W, starts, Rr, scales, seq_ids=None):
    """One launch over the samples (sample b: sequence seq_ids[b], default b) with planted draws; every sample against the oracle.
    -> the worst (e_hip, e_ref32) per float key."""
    B = len(starts)
    seq_ids = list(range(B)) if seq_ids is None else list(seq_ids)
    pose, off = pack(seqs)
    got = host(stage1_data.gravity_batch(pose, off, seq_ids, np.arange(B), W, SEED, start=starts, rot=Rr, scale=scales))
    assert got["seq_len"].dtype == np.int64 and got["lengths"].dtype == np.int32 and got["start_t_idx"].dtype == np.int32
    assert got["head_rot_mat"].shape == (B, W + 1, 3, 3) and got["floor_normal"].shape == (B, 3, 1) and got["aligned_scale"].shape == (B,)
    worst, over = {k: (0.0, 0.0) for k in O.FLOAT_KEYS}, []
    for b in range(B):
        seq = seqs[seq_ids[b]]
        start, n = O.window_of(len(seq), W, False, starts[b])
        f64 = O.sample(seq, W, start, Rr[b], np.float32(scales[b]), "fp64")
        r32 = O.sample(seq, W, start, Rr[b], np.float32(scales[b]), "ref32")
        assert n == f64["seq_len"] == got["seq_len"][b] == got["lengths"][b] and got["start_t_idx"][b] == start, (name, b)
        assert got["aug_scale"][b] == np.float32(scales[b])
        assert np.array_equal(got["ori_head_pose"][b].view(np.uint32), r32["ori_head_pose"].view(np.uint32)), (name, b)
        for k in ("head_rot_mat", "head_trans"):
            assert not got[k][b, n:].any(), (name, b, k)                   # the padding: exact zeros
        for k in O.FLOAT_KEYS:
            e_hip, e_ref = O.err_units(got[k][b], f64[k]), O.err_units(r32[k], f64[k])
            if e_hip > worst[k][0]:
                worst[k] = (e_hip, e_ref)
            if not e_hip <= 2 * e_ref + 1:
                over.append((b, k, e_hip, e_ref))
    print(f"{name}: worst e_hip (its e_ref32): " + ", ".join(f"{k} {a:.2f} ({r:.2f})" for k, (a, r) in worst.items()))
    _record(name, **{k: {"e_hip": a, "e_ref32": r} for k, (a, r) in worst.items()})
    assert not over, over[:5]
    return worst


# ---------------------------------------------------------------------------------------------- planted draws
def test_planted_draws_from_the_golden():
    """The reference's own recorded samples (window 16; 31, 17, 18, 19 and 40 frames; for_eval off and on) in one launch, with its
    recorded start, rotation and scale planted.  The recorded tensors themselves are the oracle's reference mode bit for bit
    (tests/test_stage1_data.py), so e_ref32 here is the reference's own distance from fp64."""
    g = np.load(GOLDEN)
    W = int(g["window"])
    cases = sorted(k[:-len("/start")] for k in g.files if k.endswith("/start"))
    names = sorted({c.split("/")[1] for c in cases})
    seqs = [g[f"pose/{n}"] for n in names]
    ids = [names.index(c.split("/")[1]) for c in cases]
    Rr = np.stack([O.random_rotation_from_normals(g[f"{c}/normals"], np.float32)[1] for c in cases])
    for c, R in zip(cases, Rr):
        assert np.array_equal(R.T, g[f"{c}/aligned_rot_mat"])
    starts = [int(g[f"{c}/start"]) for c in cases]
    scales = [np.float32(g[f"{c}/scale"]) for c in cases]
    assert len(cases) == 10
    check_planted("golden", seqs, W, starts, Rr, scales, ids)
    # and against the recorded tensors directly: the distance of the two from each other is at most the sum of their distances
    # from fp64, e_hip + e_ref32 <= 3 * e_ref32 + 1 (measured for the golden: e_ref32 <= 2.4)
    pose, off = pack(seqs)
    got = host(stage1_data.gravity_batch(pose, off, ids, np.arange(10), W, SEED, start=starts, rot=Rr, scale=scales))
    for b, c in enumerate(cases):
        assert got["seq_len"][b] == int(g[f"{c}/seq_len"])
        assert np.array_equal(got["ori_head_pose"][b], g[f"{c}/ori_head_pose"])
        for k in ("head_rot_mat", "head_trans", "aligned_rot_mat", "floor_normal"):
            assert O.err_units(got[k][b], g[f"{c}/{k}"]) <= 3 * 2.4 + 1, (c, k)


def test_lengths_around_the_window_in_one_batch():
    lens = [1, 2, 16, 17, 18, 19, 1000]
    seqs = [make_seq(n, i) for i, n in enumerate(lens)]
    starts = [0, 0, 0, 0, 0, 1, 982]                                       # the last start of a room of 2 and of 983
    w = check_planted("lengths 1..1000", seqs, 16, starts, random_rr(7, 1), np.linspace(0.3, 7.0, 7))
    assert w["head_trans"][0] > 0                                          # (the comparison is not vacuous)


@pytest.mark.parametrize("B", [1, 33, 257])
def test_batch_sizes(B):
    g = np.random.default_rng(B)
    lens = g.integers(2, 60, B).tolist()
    seqs = [make_seq(n, 50 + i) for i, n in enumerate(lens)]
    starts = [int(g.integers(0, max(n - 17, 1))) for n in lens]
    check_planted(f"B = {B}", seqs, 16, starts, random_rr(B, B), g.uniform(0.1, 10.0, B))


def test_window_edges():
    """window 1; window 120 at 121 frames (no room: all of them) and 122 (a room of 1); window 128, whose 129 rows are one more
    than a workgroup has threads."""
    seqs = [make_seq(n, 80 + n) for n in (1, 2, 3, 5)]
    check_planted("window 1", seqs, 1, [0, 0, 0, 2], random_rr(4, 3), [0.5, 1.0, 2.0, 9.0])
    seqs = [make_seq(n, 90 + n) for n in (121, 122, 300)]
    check_planted("window 120", seqs, 120, [0, 0, 178], random_rr(3, 4), [0.7, 3.0, 6.0])
    seqs = [make_seq(n, 95 + n) for n in (129, 300, 128)]
    check_planted("window 128", seqs, 128, [0, 170, 0], random_rr(3, 5), [0.7, 3.0, 6.0])


def test_value_edges():
    """Quaternions of norm 0.5 and 2 (two_s carries the norm), the ends of the scale's range, Rr the identity and a turn by pi."""
    seqs = [make_seq(40, 1, qnorm=0.5), make_seq(40, 2, qnorm=2.0), make_seq(40, 3), make_seq(40, 4), make_seq(40, 5), make_seq(40, 6)]
    Rr = random_rr(6, 7)
    Rr[4] = np.eye(3, dtype=np.float32)
    Rr[5] = np.diag([1.0, -1.0, -1.0]).astype(np.float32)
    w = check_planted("value edges", seqs, 16, [3, 22, 0, 5, 7, 9], Rr, [1.5, 2.5, 0.1, 10.0, 4.0, 4.0])
    pose, off = pack(seqs)
    got = host(stage1_data.gravity_batch(pose, off, [4], [0], 16, SEED, start=[7], rot=Rr[4:5], scale=[1.0]))
    assert np.array_equal(got["head_trans"][0], seqs[4][7:24, :3] - seqs[4][7:8, :3])  # identity and scale 1: the differences as they are
    assert w["aligned_scale"][0] <= 0.5


# ---------------------------------------------------------------------------------------------- the Philox draws
def test_draws_are_the_keyed_philox_draws():
    ids = [0, 5, 2 ** 40 + 1]
    lens = [40, 100, 1000]
    seqs = [make_seq(n, 30 + i) for i, n in enumerate(lens)]
    pose, off = pack(seqs)
    W = 16
    got = host(stage1_data.gravity_batch(pose, off, [0, 1, 2], ids, W, SEED))
    ev = host(stage1_data.gravity_batch(pose, off, [0, 1, 2], ids, W, SEED, for_eval=True))
    normals = O.draw_normals(SEED, ids)
    for b in range(3):
        room = lens[b] - W - 1
        want = int(O.draw_start(SEED, [ids[b]], room)[0])
        assert got["start_t_idx"][b] == want and 0 <= want < room and ev["start_t_idx"][b] == 0
        assert got["seq_len"][b] == W + 1
        scale = O.draw_scale(SEED, [ids[b]])
        assert got["aug_scale"][b:b + 1].view(np.uint32) == scale.view(np.uint32) and ev["aug_scale"][b] == got["aug_scale"][b]
        _, R64 = O.random_rotation_from_normals(normals[b], np.float64)
        _, R32 = O.random_rotation_from_normals(normals[b], np.float32)
        e_hip, e_ref = O.err_units(got["aligned_rot_mat"][b], R64.T), O.err_units(R32.T, R64.T)
        print(f"draw id {ids[b]}: start {want}, scale {float(scale[0]):.6f}, aligned_rot_mat e_hip {e_hip:.2f}, e_ref32 {e_ref:.2f}")
        _record(f"philox draw {ids[b]}", aligned_rot_mat={"e_hip": e_hip, "e_ref32": e_ref})
        assert e_hip <= 2 * e_ref + 1, (ids[b], e_hip, e_ref)
        assert np.array_equal(got["floor_normal"][b, :, 0], got["aligned_rot_mat"][b][2]) and \
            np.array_equal(ev["aligned_rot_mat"][b], got["aligned_rot_mat"][b])
        # the rest of the sample is what the planted path gives for these very draws
        planted = host(stage1_data.gravity_batch(pose, off, [b], [0], W, 0, start=[want], rot=got["aligned_rot_mat"][b].T[None],
                                                 scale=got["aug_scale"][b:b + 1]))
        for k in ("ori_head_pose", "head_rot_mat", "head_trans", "aligned_scale"):
            assert np.array_equal(planted[k][0], got[k][b]), k
    other = host(stage1_data.gravity_batch(pose, off, [0, 1, 2], ids, W, SEED + 1))
    assert not np.array_equal(other["aug_scale"], got["aug_scale"])


# ---------------------------------------------------------------------------------------------- batch independence
def _raw(pose, off, sid, did, W, fill):
    """The C entry point on buffers pre-filled with `fill` -> dict of host arrays."""
    B = len(sid)
    dev = pose.device
    d_off = torch.tensor(off, dtype=torch.int32, device=dev)
    d_sid, d_did = torch.tensor(sid, dtype=torch.int32, device=dev), torch.tensor(did, dtype=torch.int64, device=dev)
    f = lambda *s: torch.full(s, fill, dtype=torch.float32, device=dev)  # noqa: E731
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"ori_head_pose": f(B, W + 1, 7), "head_rot_mat": f(B, W + 1, 9), "head_trans": f(B, W + 1, 3), "seq_len": i(B),
           "aligned_rot_mat": f(B, 9), "aligned_scale": f(B), "floor_normal": f(B, 3), "start_t_idx": i(B), "aug_scale": f(B)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check_s1_data(_lib.load().egoego_s1_gravity_batch(pose.data_ptr(), pose.shape[0], d_off.data_ptr(), len(off) - 1, d_sid.data_ptr(),
                                                           d_did.data_ptr(), B, W, SEED, 0, None, None, None,
                                                           *[out[k].data_ptr() for k in out], stream))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_a_sample_does_not_depend_on_its_batch_nor_on_what_the_outputs_held():
    lens = [17, 40, 25] + [31 + i for i in range(30)]
    seqs = [make_seq(n, 300 + i) for i, n in enumerate(lens)]
    pose, off = pack(seqs)
    W, sid, did = 16, 1, 123456789012
    alone = _raw(pose, off, [sid], [did], W, float("nan"))
    assert all(np.isfinite(v).all() for v in alone.values())               # every output written whole
    again = _raw(pose, off, [sid], [did], W, 3.0)
    assert _same_bits(alone, again)
    pair = _raw(pose, off, [0, sid], [7, did], W, float("nan"))
    big_ids = list(range(33))
    big = _raw(pose, off, big_ids[::-1], [did if k == sid else 1000 + k for k in big_ids[::-1]], W, float("nan"))
    at = big_ids[::-1].index(sid)
    for other, b in ((pair, 1), (big, at)):
        assert _same_bits(alone, {k: v[b:b + 1] for k, v in other.items()})
    assert all(np.isfinite(v).all() for v in big.values())
    through_python = host(stage1_data.gravity_batch(pose, off, [sid], [did], W, SEED))
    for k in alone:
        assert np.array_equal(through_python["lengths" if k == "seq_len" else k].reshape(alone[k].shape), alone[k]), k


def test_ids_that_do_not_fit_give_empty_samples_and_host_ids_raise():
    seqs = [make_seq(40, 1), make_seq(17, 2)]
    pose, off = pack(seqs)
    with pytest.raises(ValueError):
        stage1_data.gravity_batch(pose, off, [2], [0], 16, SEED)
    with pytest.raises(ValueError):
        stage1_data.gravity_batch(pose, [0, 40, 40, 57], [0], [0], 16, SEED)   # a sequence of no frames
    ids = torch.tensor([0, 5, -1, 1], dtype=torch.int32, device="cuda")        # a device tensor is not read back: the kernel guards
    got = host(stage1_data.gravity_batch(pose, off, ids, [0, 1, 2, 3], 16, SEED, start=[22, 0, 0, 0]))
    assert got["seq_len"].tolist() == [17, 0, 0, 17]
    assert not got["head_rot_mat"][1:3].any() and not got["ori_head_pose"][1:3].any() and np.isfinite(got["aligned_rot_mat"]).all()
    got = host(stage1_data.gravity_batch(pose, off, [0, 0, 1], [0, 1, 2], 16, SEED, start=[23, -1, 1]))  # rooms of 23, 23 and 0
    assert got["seq_len"].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- forward with lengths
def _opt(window, layers):
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256)


def _gravity_module(window, layers, seed=0):
    torch.manual_seed(seed)
    m = stage1.HeadNormalFormer(_opt(window, layers), torch.device("cuda")).cuda()
    m.hip_training = True
    m.eval()  # no dropout: the same bits on every call
    return m


def _padded_batch(lens, W, fill):
    seqs = [make_seq(n, 400 + i) for i, n in enumerate(lens)]
    pose, off = pack(seqs)
    B = len(lens)
    b = stage1_data.gravity_batch(pose, off, list(range(B)), list(range(B)), W, SEED)
    rows = torch.arange(W + 1, device="cuda")[None, :] >= b["lengths"][:, None]
    b["head_rot_mat"][rows] = fill                                         # what the padding holds must not matter
    b["head_trans"][rows] = fill
    return b


def test_forward_with_lengths_is_each_sequence_alone():
    W, layers, lens = 16, 2, (17, 9, 2)
    m = _gravity_module(W, layers)
    data = _padded_batch(lens, W, 7.0)
    assert data["lengths"].tolist() == list(lens)
    singles = [{"head_rot_mat": data["head_rot_mat"][b:b + 1, :n].contiguous(), "head_trans": data["head_trans"][b:b + 1, :n].contiguous()}
               for b, n in enumerate(lens)]
    pred = m(data)["pred_normal"]
    assert pred.requires_grad and pred.shape == (3, 3)
    for b in range(3):
        assert torch.equal(m(singles[b])["pred_normal"][0], pred[b]), b      # the training encode: the same bits
    with torch.no_grad():
        inf = m(data)["pred_normal"]
        for b in range(3):
            assert torch.equal(m(singles[b])["pred_normal"][0], inf[b]), b   # the inference encode
    no_key = {k: v for k, v in data.items() if k != "lengths"}
    assert not torch.equal(m(no_key)["pred_normal"][1:], pred[1:])          # (the padding counts without the key)


def test_forward_without_lengths_is_the_call_with_full_lengths():
    W = 16
    m = _gravity_module(W, 1)
    data = _padded_batch((40, 31, 17), W, 0.0)
    no_key = {k: v for k, v in data.items() if k != "lengths"}
    full = dict(no_key, lengths=torch.full((3,), W + 1, dtype=torch.int32, device="cuda"))
    assert torch.equal(m(no_key)["pred_normal"], m(full)["pred_normal"])
    with torch.no_grad():
        assert torch.equal(m(no_key)["pred_normal"], m(full)["pred_normal"])
    for bad in (full["lengths"].long(), full["lengths"].cpu(), full["lengths"][:2]):
        with pytest.raises(ValueError):
            m(dict(no_key, lengths=bad))


def test_gradients_with_lengths_are_the_sum_of_the_single_runs():
    """The batch (17, 9, 2) through the module with `lengths`, backward from a random upstream: the gradients are the training
    engine's on the features and valid counts the module built (the same bits), and meet the bar of DESIGN.md 5l,
    e_hip <= 2 (e_emul + e_32), against the SUM over the three sequences of the oracle's single runs (each sequence alone at its
    own length, the HIP path's ReLU decisions forced, as in tests/test_gpu_stage1_train.py; the fp32 oracle adds its three runs in
    fp32, as an fp32 path would: the last bias's gradient is the plain sum of the upstream rows, exact in any other mode)."""
    W, layers, lens = 16, 2, (17, 9, 2)
    m = _gravity_module(W, layers)
    data = _padded_batch(lens, W, 7.0)
    up = torch.randn(3, 3, generator=torch.Generator().manual_seed(3))
    (m(data)["pred_normal"] * up.cuda()).sum().backward()
    g_mod = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    # the engine on the oracle's features of each sequence at its own length
    rot, trans = data["head_rot_mat"].cpu(), data["head_trans"].cpu()
    feats = torch.stack([S1.gravity_features(rot[b, :n], trans[b, :n], W)[0] for b, n in enumerate(lens)])
    valid = torch.tensor([n - 1 for n in lens], dtype=torch.int32)
    eng = m.train_engine()
    ts = {n: p.detach() for n, p in m.named_parameters()}
    heads, saves = eng.forward(ts, feats.cuda(), valid.cuda(), 0.0, 0)
    g_eng = eng.backward(ts, saves, up.cuda(), 3, 0.0, 0)
    hidden = [eng.saved(saves, 3, l, "ffn_hidden").cpu() > 0 for l in range(layers)]
    lin = TO.head_linear_names("gravitynet")
    head_hidden = {nm: eng.saved(saves, 3, j, "head_hidden").cpu() > 0 for j, nm in enumerate(lin) if not nm.endswith("_fc")}
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sums = {}
    for tag, kw in (("64", {}), ("em", dict(mm=TO.split_mm)), ("32", dict(dtype=torch.float32))):
        total = None
        for b in range(3):
            masks = dict(relu_masks=[h[b:b + 1] for h in hidden], head_masks={k: v[b:b + 1] for k, v in head_hidden.items()})
            _, g = TO.heads_and_grads(sd, "gravitynet", feats[b:b + 1], valid[b:b + 1], layers, up[b:b + 1], **masks, **kw)
            if tag == "32":  # an fp32 path adds the three runs' gradients in fp32 too
                g = {k: v.float() for k, v in g.items()}
            total = g if total is None else {k: total[k] + g[k] for k in g}
        sums[tag] = {k: v.double() for k, v in total.items()}
    g64 = sums["64"]
    assert sorted(g64) == sorted(g_mod) == sorted(g_eng)
    norm = math.sqrt(sum(float(g.norm()) ** 2 for g in g64.values()))
    ratios, over = {}, []
    for k, ref in g64.items():
        hip = g_mod[k].cpu().double().reshape(ref.shape)
        # the module's own features come from egoego_s1_gravity_features; the oracle's from torch on the CPU: the same formula,
        # possibly other roundings, so the two HIP gradients are compared through the bar and not by their bits
        if float(ref.norm()) <= 1e-9 * norm:
            assert k.endswith("w_k.bias"), k
            assert float(hip.norm()) <= 1e-6 * norm, k
            continue
        e_em, e_32 = TO.rel_err(sums["em"][k], ref), TO.rel_err(sums["32"][k], ref)
        for name, g in (("module", hip), ("engine", g_eng[k].cpu().double().reshape(ref.shape))):
            e_hip = TO.rel_err(g, ref)
            ratios[f"{name} {k}"] = e_hip / (e_em + e_32) if e_em + e_32 > 0 else (0.0 if e_hip == 0 else float("inf"))
            if not e_hip <= 2 * (e_em + e_32):
                over.append((name, k, e_hip, e_em, e_32))
    worst = sorted(((v, k) for k, v in ratios.items()), reverse=True)[:3]
    print("lengths (17, 9, 2): worst e_hip / (e_emul + e_32): " + ", ".join(f"{k} {v:.2f}" for v, k in worst))
    _record("gradients with lengths", ratios=ratios)
    assert not over, over


# ---------------------------------------------------------------------------------------------- the trainer
def _strict(fn):
    """fn under torch.cuda.set_sync_debug_mode("error"): a synchronisation (a device-to-host copy is one) inside it raises."""
    def wrapped(*args, **kwargs):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return wrapped


def _poses():
    lens = (31, 33, 40, 35, 64, 47, 32, 52)
    return {f"{'CMU' if i < 6 else 'SFU'}-{i:02d}": make_seq(n, 500 + i) for i, n in enumerate(lens)}


def _trainer(tmp, model_seed, monkeypatch=None):
    W = 16
    torch.manual_seed(model_seed)
    m = stage1.HeadNormalFormer(_opt(W, 1), torch.device("cuda")).cuda()
    poses = _poses()
    tr_names, val_names = stage1_data.split_by_dataset(list(poses))
    train = stage1_data.GravityBatches(poses, 4, window=W, seed=11, names=tr_names)
    val = stage1_data.GravityBatches(poses, 4, window=W, train=False, for_eval=True, shuffle=False, seed=11, names=val_names)
    assert (len(train), len(val)) == (2, 1)
    return Stage1Trainer(m, train, val, save_dir=str(tmp), save_interval=1), train


def _params(tr):
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


def test_trainer_over_gravity_batches(tmp_path, monkeypatch):
    """8 short sequences (6 train, 2 validation by the split rule), batch 4, 2 epochs.  Every iteration's step and every batch
    build run under the sync debug mode "error" (the epoch's one upload of its order and the epoch means at its end are outside,
    as the validation's read-back is).  A: two epochs.  B: one epoch, then a fresh model, trainer and GravityBatches that load
    train-1.pt and run the second: the same bits as A, which needs the batches' epoch and generator from `data_state`."""
    with pytest.raises(RuntimeError):  # the method itself: a read-back under the mode raises
        _strict(lambda: torch.ones(1, device="cuda").item())()
    monkeypatch.setattr(stage1_data, "gravity_batch", _strict(stage1_data.gravity_batch))
    a, a_train = _trainer(tmp_path / "a", 1)
    a.step = _strict(a.step)
    seen = []
    a_iter = a_train.__class__.__iter__

    def spy(self):
        for batch in a_iter(self):
            seen.append((self.epoch, tuple(batch["seq_name"]), batch["lengths"]))
            yield batch

    monkeypatch.setattr(stage1_data.GravityBatches, "__iter__", spy)
    torch.manual_seed(21)
    assert a.train(1) == 1
    torch.manual_seed(22)
    assert a.train(1) == 2
    assert len(a.history) == 2 and all(math.isfinite(h["loss"]) and h["loss"] > 0 for h in a.history)
    assert len(a.val_history) == 2 and all(math.isfinite(h["loss"]) for h in a.val_history)
    train_seen = [s for s in seen if not s[1][0].startswith("SFU")]
    assert [len(s[1]) for s in train_seen] == [4, 2, 4, 2] and all(sorted(sum((s[1] for s in train_seen[i:i + 2]), ())) ==
                                                                    sorted(n for n in _poses() if n.startswith("CMU")) for i in (0, 2))
    assert all(s[2].tolist() == [17] * len(s[1]) for s in seen)
    ck = torch.load(tmp_path / "a" / "weights" / "train-1.pt", map_location="cpu")
    assert sorted(ck) == ["data_state", "epoch", "loss", "optimizer_state_dict", "transformer_encoder_state_dict"]
    assert ck["data_state"]["epoch"] == 1

    b0, _ = _trainer(tmp_path / "b", 1)
    torch.manual_seed(21)
    assert b0.train(1) == 1
    b, b_train = _trainer(tmp_path / "b", 9)                                # other weights, batches at epoch 0
    assert any(not torch.equal(v, _params(a)[k]) for k, v in _params(b).items())
    b.load(str(tmp_path / "b" / "weights" / "train-1.pt"))
    assert b.epoch == 1 and b_train.epoch == 1
    torch.manual_seed(22)
    assert b.train(1) == 2
    pa, pb = _params(a), _params(b)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    # without the data state the second epoch draws other batches
    c, c_train = _trainer(tmp_path / "b", 9)
    ck = torch.load(tmp_path / "b" / "weights" / "train-1.pt", map_location="cpu")
    c.model.load_state_dict(ck["transformer_encoder_state_dict"])
    c.optimizer.load_state_dict(ck["optimizer_state_dict"])
    c.epoch = 1
    torch.manual_seed(22)
    c.train(1)
    pc = _params(c)
    assert any(not torch.equal(pa[k], pc[k]) for k in pa)
    fresh = stage1.HeadNormalFormer(_opt(16, 1), torch.device("cuda"))
    fresh.load_state_dict(torch.load(tmp_path / "a" / "weights" / "train-2.pt", map_location="cpu")["transformer_encoder_state_dict"])


def test_the_training_tool_on_a_motion_file(tmp_path, capsys):
    """tools/train_stage1.py --kind gravitynet --motion FILE (in this process: the test is about the tool's loop): a motion file in
    the layout of tools/process_amass.py, the validation set from the split rule; the checkpoint loads into a fresh module."""
    import importlib.util
    import pickle
    spec = importlib.util.spec_from_file_location("train_stage1_tool", os.path.join(ROOT, "tools", "train_stage1.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    motion = {name: {"head_qpos": p, "seq_name": name, "trans": p[:, :3]} for name, p in _poses().items()}
    path = tmp_path / "train_amass_smplh_motion.p"
    with open(path, "wb") as f:
        pickle.dump(motion, f)
    out = tmp_path / "run"
    tool.main(["--kind", "gravitynet", "--motion", str(path), "--save_dir", str(out), "--epochs", "2", "--window", "16", "--n_dec_layers", "1",
               "--batch_size", "4", "--save_interval", "2"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["epoch"] for l in lines[:2]] == [1, 2] and math.isfinite(lines[1]["train"]["loss"]) and "val" in lines[0]
    ck = torch.load(out / "weights" / "train-2.pt", map_location="cpu", weights_only=True)
    assert ck["data_state"]["epoch"] == 2
    stage1.HeadNormalFormer(_opt(16, 1), torch.device("cuda")).load_state_dict(ck["transformer_encoder_state_dict"])
