"""HeadNet's training batches on the GPU (egoego_s1_head_batch; egoego_release_amd/stage1_data.py): the reference's recorded items,
the numpy oracle of tests/head_batch_oracle.py at the shapes where a copy kernel goes wrong, ragged for_eval batches, the keyed
draw, ids that do not fit, pre-filled outputs, HeadFormer's loss and gradients on a built batch, Stage1Trainer and the two tools.
(The side-stream check is tests/test_gpu_streams_head_batches.py.)

The bar everywhere is BIT EQUALITY: the kernel only selects and copies, and the padding is exact zeros.  head_vels is compared
with the reference's fp64 rounded once to fp32.
"""
import ctypes as C
import importlib.util
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import head_batch_oracle as O
from egoego_release_amd import _lib, stage1, stage1_data, synthetic
from egoego_release_amd.trainer import Stage1Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "head_batch_golden.npz")
SEED = 2 ** 33 + 5
KEYS = ("head_pose", "head_vels", "of", "lengths", "seq_len", "start_t_idx")
TAILS = dict(zip(O.SLAM_KEYS, ((3,), (4,), (3, 3), (3,), (4,), (3, 3))))


# ---------------------------------------------------------------------------------------------- fixtures
def make_seq(T, D, seed, L=None, name=None):
    """An entry of distinct random numbers (a row copied from the wrong place shows); L: rows of a planted, already aligned track."""
    g = np.random.default_rng(7000 + seed)
    e = {"seq_name": name or f"scene_{seed}-seq_{seed}", "head_qpos": g.normal(size=(T, 7)).astype(np.float32),
         "head_vels": g.normal(size=(T, 6)), "of_feats": g.normal(size=(T - 1, D)).astype(np.float32)}
    if L is not None:
        for k in O.SLAM_KEYS:
            e[k] = g.normal(size=(L,) + TAILS[k]).astype(np.float64 if k == "ori_slam_trans" else np.float32)
    return e


def cut(seq):
    """The entry as the tables hold it: the track's rows past T are cut at packing (no slice reaches them)."""
    T = len(seq["head_qpos"])
    return {k: (v[:T] if k in O.SLAM_KEYS else v) for k, v in seq.items()}


def tables_of(seqs):
    """Every sequence of at least one feature frame, packed and uploaded (for_eval's dropping rule: the short ones stay in)."""
    p = stage1_data.pack_head_sequences(seqs, 1, for_eval=True)
    assert p["names"] == [s["seq_name"] for s in seqs]
    return {k: torch.from_numpy(v).cuda() for k, v in p.items() if isinstance(v, np.ndarray)}


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items() if isinstance(v, torch.Tensor)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(name, seqs, W, ids, starts=None, for_eval=False, tables=None):
    """One launch over the samples (sample b: sequence ids[b], planted start starts[b]); every key of every sample against the
    oracle, bit for bit.  -> the batch on the host."""
    tables = tables_of(seqs) if tables is None else tables
    got = host(stage1_data.head_batch(tables, ids, np.arange(len(ids)), W, SEED, for_eval=for_eval, start=starts))
    slam = "aligned_slam_trans" in seqs[0]
    assert sorted(got) == sorted(KEYS + ((O.SLAM_KEYS + ("pose_lengths",)) if slam else ()))
    assert got["seq_len"].dtype == np.int64 and got["lengths"].dtype == np.int32 and got["start_t_idx"].dtype == np.int32
    for b, sid in enumerate(ids):
        want = O.padded(cut(seqs[sid]), W, for_eval, 0 if starts is None else starts[b])
        for k, w in want.items():
            assert same_bits(got[k][b], w), (name, b, sid, k)
    return got


# ---------------------------------------------------------------------------------------------- 1. the golden
def golden():
    g = np.load(GOLDEN)
    seqs = []
    for n in (str(n) for n in g["kept"]):
        e = {"seq_name": n, **{k: g[f"seq/{n}/{k}"] for k in ("head_qpos", "head_vels", "of_feats") + O.SLAM_KEYS}}
        seqs.append(e)
    items = {m: [{k[len(f"{m}/{j}/"):]: g[k] for k in g.files if k.startswith(f"{m}/{j}/")} for j in range(int(g[f"{m}/count"]))]
             for m in ("train", "eval")}
    return int(g["window"]), seqs, items


def test_the_reference_s_recorded_items():
    """Window 4, D = 12, T = 6, 5, 9 (a track of 7 rows) and 8; the T = 5 sequence's track has 8 rows.  The 8 training items with
    their recorded starts planted in one launch, the 4 for_eval items in one launch padded to the longest: every key is the
    reference's bits (head_vels: its fp64 rounded once), the rest zeros, pose_lengths the rows the reference returned."""
    W, seqs, items = golden()
    names = [s["seq_name"] for s in seqs]
    for mode, recs in items.items():
        ids = [names.index(str(r["seq"])) for r in recs]
        ev = mode == "eval"
        Wm = max(len(s["head_qpos"]) - 1 for s in seqs) if ev else W
        got = check(f"golden {mode}", seqs, Wm, ids, None if ev else [int(r["start"]) for r in recs], for_eval=ev)
        assert len(recs) == (4 if ev else 8)
        for b, r in enumerate(recs):
            n = int(r["seq_len"])
            assert got["seq_len"][b] == n and got["start_t_idx"][b] == int(r["start"])
            assert got["pose_lengths"][b] == len(r["aligned_slam_trans"]) == len(r["ori_slam_rot_mat"])
            for k in ("head_pose", "of") + O.SLAM_KEYS:
                assert same_bits(got[k][b, :len(r[k])], r[k]) and not got[k][b, len(r[k]):].any(), (mode, b, k)
            assert r["head_vels"].dtype == np.float64 and same_bits(got["head_vels"][b, :n], r["head_vels"].astype(np.float32))
            assert not got["head_vels"][b, n:].any()
        if ev:
            assert sorted(got["pose_lengths"].tolist()) == [5, 6, 7, 8] and sorted(got["seq_len"].tolist()) == [4, 5, 7, 8]
    # through HeadBatches: the same tables, the for_eval batch with its host lists
    hb = stage1_data.HeadBatches(seqs, 4, window=W, train=False, for_eval=True, shuffle=False)
    batch = next(iter(hb))
    assert batch["lengths_host"] == [5, 4, 8, 7] and batch["pose_lengths_host"] == [6, 5, 7, 8] and batch["seq_name"] == names
    assert batch["lengths"].tolist() == batch["lengths_host"] and batch["pose_lengths"].tolist() == batch["pose_lengths_host"]
    assert batch["of"].shape == (4, 8, 12) and batch["ori_slam_trans"].dtype == torch.float64


# ---------------------------------------------------------------------------------------------- 2. the oracle sweep
def sweep_case(W, D):
    """F = W (a room of 1), W + 1 and 3 W + 2; tracks of L = T, T + 3 (cut at T), 1 and, for the last sequence, L = room - 1 (its
    last start gives pose_len 0).  -> (sequences, [(sequence, start)]: starts 0 and room - 1, first and last sequence of the
    tables included)"""
    Fs = (W, W + 1, 3 * W + 2, W, 3 * W + 2)
    Ls = (W + 1, W + 5, 1, W + 1, 2 * W + 2)
    seqs = [make_seq(F + 1, D, 10 * W + i, L) for i, (F, L) in enumerate(zip(Fs, Ls))]
    samples = []
    for sid, F in enumerate(Fs):
        samples += [(sid, 0), (sid, F - W)]
    return seqs, samples


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("D", [4, 12, 512])
@pytest.mark.parametrize("W", [1, 2, 60])
def test_oracle_sweep(W, D, B):
    """W + 1 = 2, 3 and 61 are no multiples of the kernel's frame tile of 4.  B = 33: every (sequence, start) pair several times in
    one launch, so one sequence id is used more than once; B = 1: each pair in a launch of its own."""
    seqs, samples = sweep_case(W, D)
    tables = tables_of(seqs)
    bare = [{k: v for k, v in s.items() if k not in O.SLAM_KEYS} for s in seqs]
    bare_tables = tables_of(bare)
    assert "slam32" not in bare_tables
    if B == 1:
        for sid, st in samples:
            got = check(f"W {W} D {D} alone", seqs, W, [sid], [st], tables=tables)
            assert got["seq_len"][0] == W
            check(f"W {W} D {D} alone, no SLAM", bare, W, [sid], [st], tables=bare_tables)
    else:
        pairs = [samples[(3 * b) % len(samples)] for b in range(B)]
        ids, starts = [p[0] for p in pairs], [p[1] for p in pairs]
        got = check(f"W {W} D {D} B {B}", seqs, W, ids, starts, tables=tables)
        assert (got["seq_len"] == W).all() and 0 in got["pose_lengths"] and got["pose_lengths"].max() == W + 1
        nb = check(f"W {W} D {D} B {B}, no SLAM", bare, W, ids, starts, tables=bare_tables)
        assert not any(k in nb for k in O.SLAM_KEYS + ("pose_lengths",))       # no SLAM tables: the keys are absent
        for k in ("head_pose", "head_vels", "of"):
            assert same_bits(nb[k], got[k])


# ---------------------------------------------------------------------------------------------- 3. for_eval, ragged
def test_for_eval_ragged():
    D = 512
    Fs, Ls = (1, 2, 7, 61), (2, 1, 11, 40)
    seqs = [make_seq(F + 1, D, 300 + i, L) for i, (F, L) in enumerate(zip(Fs, Ls))]
    got = check("for_eval ragged", seqs, 61, [3, 0, 2, 1], for_eval=True)
    assert got["lengths"].tolist() == [61, 1, 7, 2] and got["pose_lengths"].tolist() == [40, 2, 8, 1]
    assert not got["start_t_idx"].any()
    for b, (n, pl) in enumerate(zip(got["lengths"], got["pose_lengths"])):
        assert not got["of"][b, n:].any() and not got["head_pose"][b, n + 1:].any() and got["head_pose"][b, n].any()
        assert not got["ori_slam_trans"][b, pl:].any() and not got["aligned_slam_rot_mat"][b, pl:].any()
    check("for_eval at a shorter pad", seqs, 5, [0, 1, 2, 3], for_eval=True)      # n = min(F, W)
    hb = stage1_data.HeadBatches(seqs, 3, window=90, train=False, for_eval=True, shuffle=False)
    a, b = list(hb)
    assert a["of"].shape == (3, 7, D) and b["of"].shape == (1, 61, D) and a["lengths_host"] == [1, 2, 7] and b["pose_lengths_host"] == [40]
    assert same_bits(b["of"][0].cpu().numpy(), seqs[3]["of_feats"])


# ---------------------------------------------------------------------------------------------- 4. the draws
def test_draws_are_the_keyed_philox_draws():
    W, D = 5, 12
    Fs = (W, 40, 1000, 9)
    seqs = [make_seq(F + 1, D, 400 + i, F + 1) for i, F in enumerate(Fs)]
    tables = tables_of(seqs)
    draws = [0, 5, 2 ** 40 + 1, 2 ** 32 - 1, 2 ** 32, 7, 123456789012]
    ids = [1, 2, 2, 1, 3, 0, 2]
    seen = set()
    for seed in (SEED, 3, 2 ** 63 + 11):
        got = host(stage1_data.head_batch(tables, ids, draws, W, seed))
        for b, (sid, d) in enumerate(zip(ids, draws)):
            room = Fs[sid] - W + 1
            want = int(O.draw_start(seed, [d], room)[0])
            assert got["start_t_idx"][b] == want and 0 <= want < room and got["seq_len"][b] == W, (seed, b)
            planted = host(stage1_data.head_batch(tables, [sid], [0], W, 0, start=[want]))
            for k in planted:
                assert same_bits(planted[k][0], got[k][b]), k
            seen.add(want)
        assert got["start_t_idx"][5] == 0                                     # a room of 1
        ev = host(stage1_data.head_batch(tables, ids, draws, W, seed, for_eval=True))
        assert not ev["start_t_idx"].any()
    assert len(seen) > 10
    # a sample is the same bits alone, in another batch, under another order
    base = host(stage1_data.head_batch(tables, ids, draws, W, SEED))
    order = [4, 6, 0, 2, 5, 1, 3]
    perm = host(stage1_data.head_batch(tables, [ids[i] for i in order], [draws[i] for i in order], W, SEED))
    for j, i in enumerate(order):
        alone = host(stage1_data.head_batch(tables, [ids[i]], [draws[i]], W, SEED))
        for k in base:
            assert same_bits(perm[k][j], base[k][i]) and same_bits(alone[k][0], base[k][i]), (k, i)
    other = host(stage1_data.head_batch(tables, ids, draws, W, SEED + 1))
    assert not np.array_equal(other["start_t_idx"], base["start_t_idx"])


# ---------------------------------------------------------------------------------------------- 5. ids that do not fit
def test_ids_that_do_not_fit_give_empty_samples_and_host_ids_raise():
    W, D = 6, 12
    seqs = [make_seq(20, D, 500, 20), make_seq(6, D, 501, 6), make_seq(7, D, 502, 7)]      # F = 19, 5 (< W) and 6
    tables = tables_of(seqs)
    with pytest.raises(ValueError):
        stage1_data.head_batch(tables, [3], [0], W, SEED)
    with pytest.raises(ValueError):
        stage1_data.head_batch(tables, [-1], [0], W, SEED)
    with pytest.raises(ValueError):
        stage1_data.head_batch(dict(tables, offsets=[0, 20, 20, 33]), [0], [0], W, SEED)   # a sequence of no frames
    ids = torch.tensor([0, 5, -1, 1, 2, 0, 0, 2], dtype=torch.int32, device="cuda")          # not read back: the kernel guards
    starts = [13, 0, 0, 0, 0, 14, -1, 1]                                                   # rooms of 14, -, -, 0, 1, 14, 14, 1
    got = host(stage1_data.head_batch(tables, ids, np.arange(8), W, SEED, start=starts))
    assert got["seq_len"].tolist() == [W, 0, 0, 0, W, 0, 0, 0] and got["pose_lengths"].tolist() == [W + 1, 0, 0, 0, W + 1, 0, 0, 0]
    assert not got["start_t_idx"][[1, 2, 3, 5, 6, 7]].any()
    for b in (1, 2, 3, 5, 6, 7):
        for k in ("head_pose", "head_vels", "of") + O.SLAM_KEYS:
            assert not got[k][b].any(), (b, k)
    for b, (sid, st) in ((0, (0, 13)), (4, (2, 0))):
        want = O.padded(seqs[sid], W, False, st)
        assert all(same_bits(got[k][b], w) for k, w in want.items())
    drawn = host(stage1_data.head_batch(tables, ids, np.arange(8), W, SEED))              # the same without planted starts
    assert drawn["seq_len"].tolist() == [W, 0, 0, 0, W, W, W, W]


# ---------------------------------------------------------------------------------------------- 6. every byte is written
def _raw(tables, off_host, sid, starts, W, fill):
    """The C entry point on outputs pre-filled with `fill` (a float, or a byte for memset) -> dict of host arrays."""
    B, dev = len(sid), tables["pose"].device
    D = tables["feats"].shape[1]
    shapes = {"head_pose": ((B, W + 1, 7), torch.float32), "head_vels": ((B, W, 6), torch.float32), "of": ((B, W, D), torch.float32),
              "lengths": ((B,), torch.int32), "start_t_idx": ((B,), torch.int32)}
    for k in O.SLAM_KEYS:
        shapes[k] = ((B, W + 1) + TAILS[k], torch.float64 if k == "ori_slam_trans" else torch.float32)
    shapes["pose_lengths"] = ((B,), torch.int32)
    out = {}
    for k, (shape, dt) in shapes.items():
        t = torch.empty(shape, dtype=dt, device=dev)
        if isinstance(fill, float) and dt.is_floating_point:
            t.fill_(fill)
        else:
            t.view(torch.uint8).fill_(0x7f)
        out[k] = t
    d_sid = torch.tensor(sid, dtype=torch.int32, device=dev)
    d_did = torch.arange(B, dtype=torch.int64, device=dev)
    d_start = torch.tensor(starts, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check_s1_data(_lib.load().egoego_s1_head_batch(
        tables["pose"].data_ptr(), tables["vels"].data_ptr(), tables["feats"].data_ptr(), tables["pose"].shape[0], D,
        tables["offsets"].data_ptr(), len(off_host) - 1, tables["slam32"].data_ptr(), tables["slam_trans64"].data_ptr(),
        tables["slam_offsets"].data_ptr(), tables["slam32"].shape[0], d_sid.data_ptr(), d_did.data_ptr(), B, W, SEED, 0,
        d_start.data_ptr(), *[out[k].data_ptr() for k in shapes], stream))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("W,D", [(2, 12), (60, 512)])
def test_every_byte_is_written_whatever_the_outputs_held(W, D):
    seqs, samples = sweep_case(W, D)
    tables = tables_of(seqs)
    pairs = [samples[(3 * b) % len(samples)] for b in range(33)] + [(1, 5)]                # ... and an empty sample (a room of 2)
    ids, starts = [p[0] for p in pairs], [p[1] for p in pairs]
    want = check("the sweep's batch", seqs, W, ids, starts, tables=tables)
    assert want["seq_len"][-1] == 0
    off = tables["offsets"].cpu().tolist()
    for fill in (float("nan"), 0x7f):
        got = _raw(tables, off, ids, starts, W, fill)
        for k, v in got.items():
            assert same_bits(v.reshape(want[k].shape), want[k]), (fill, k)


# ---------------------------------------------------------------------------------------------- 7. the model
def _opt(window, layers, gw=31, gl=1):
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0, input_of_feats=True,
                     w_rotation=1.0, w_va=1.0, w_dist=1.0, normal_window=gw, normal_n_dec_layers=gl, normal_n_head=4, normal_d_k=256,
                     normal_d_v=256, normal_d_model=256)


def real_seq(T, seed, L=None, name=None):
    """An entry a net can run on: the poses, velocities and features of synthetic.make_stage1_train_batch, a raw SLAM track."""
    b = synthetic.make_stage1_train_batch("headnet", 1, T - 1, seed=seed)
    g = np.random.default_rng(8000 + seed)
    vels = np.concatenate([np.asarray(b["head_vels"][0], np.float64), np.zeros((1, 6))], 0) + g.normal(0, 1e-9, (T, 6))  # (true fp64)
    e = {"seq_name": name or f"scene{seed}-seq{seed}", "head_qpos": np.asarray(b["head_pose"][0], np.float32), "head_vels": vels,
         "of_feats": np.asarray(b["of"][0], np.float32)}
    if L is not None:
        q = g.normal(size=(1, 4)) + np.cumsum(g.normal(0, 0.05, (L, 4)), 0)
        e["slam"] = np.concatenate([np.cumsum(g.normal(0, 0.05, (L, 3)), 0), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)
    return e


def test_headformer_loss_and_gradients_on_a_built_batch():
    """forward + compute_loss + backward (hip_training) on a HeadBatches batch and on the reference-format dict built on the host
    from the same slices (CPU tensors, head_vels fp64): the same loss parts and gradients, bit for bit."""
    W = 16
    seqs = [real_seq(T, 600 + i) for i, T in enumerate((17, 30, 18, 41, 25))]
    torch.manual_seed(0)
    m = stage1.HeadFormer(_opt(W, 1), torch.device("cuda")).cuda()
    m.hip_training = True
    m.eval()  # no dropout: the same bits on every call
    hb = stage1_data.HeadBatches(seqs, 5, window=W, shuffle=True, seed=9)
    batch = next(iter(hb))
    starts = batch["start_t_idx"].tolist()
    by = {s["seq_name"]: s for s in seqs}
    assert len(set(starts)) > 1 and batch["head_vels"].dtype == torch.float32
    items = [O.item(by[n], st, W) for n, st in zip(batch["seq_name"], starts)]
    ref = {k: torch.from_numpy(np.stack([np.asarray(it[k]) for it in items])) for k in ("head_pose", "head_vels", "of")}
    ref["seq_len"] = torch.tensor([it["seq_len"] for it in items])
    assert ref["head_vels"].dtype == torch.float64 and not torch.equal(ref["head_vels"].float().double(), ref["head_vels"])
    res = []
    for data in (batch, ref):
        m.zero_grad(set_to_none=True)
        parts = m.compute_loss(m(data), data)
        parts[0].backward()
        res.append(([p.detach().clone() for p in parts], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (pa, ga), (pb, gb) = res
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and math.isfinite(float(pa[0])) and float(pa[0]) > 0
    assert sorted(ga) == sorted(gb) and len(ga) > 10 and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert any(float(g.abs().max()) > 0 for g in ga.values())


def test_for_eval_batch_through_estimate_head_pose():
    """A for_eval batch of HeadBatches through estimate_head_pose(lengths=, pose_lengths=) against per-sequence calls on
    single-sequence batches built on the host: the same bits below each end, zeros past it (the bar tests/test_gpu_stage1_ragged.py
    holds the ragged call to: a sequence's rows do not depend on its batch)."""
    hw, gw = 16, 31
    seqs = [real_seq(T, 700 + i, L) for i, (T, L) in enumerate(((40, 40), (21, 30), (33, 25)))]
    dev = torch.device("cuda")
    hn = stage1.HeadFormer(_opt(hw, 1, gw, 1), dev)
    hn.load_state_dict(synthetic.make_stage1_weights("headnet", hn.cfg, 216))
    gn = stage1.HeadNormalFormer(_opt(hw, 1, gw, 1), dev, eval_whole_pipeline=True)
    gn.load_state_dict(synthetic.make_stage1_weights("gravitynet", gn.cfg, 331))
    hb = stage1_data.HeadBatches(seqs, 3, window=hw, train=False, for_eval=True, shuffle=False)
    batch = next(iter(hb))
    assert batch["lengths_host"] == [39, 20, 32] and batch["pose_lengths_host"] == [40, 21, 25]
    with torch.no_grad():
        pose, _, _, n = stage1.estimate_head_pose(hn, gn, batch, lengths=batch["lengths_host"], pose_lengths=batch["pose_lengths_host"])
        assert n.tolist() == [40, 21, 25]
        packed = stage1_data.pack_head_sequences(seqs, hw, for_eval=True)
        for b, s in enumerate(seqs):
            T = len(s["head_qpos"])
            so, L = packed["slam_offsets"][b], batch["pose_lengths_host"][b]
            row = packed["slam32"][so:so + L]
            one = {"of": torch.from_numpy(s["of_feats"])[None], "head_pose": torch.from_numpy(s["head_qpos"])[None],
                   "aligned_slam_trans": torch.from_numpy(row[:, :3].copy())[None],
                   "ori_slam_trans": torch.from_numpy(packed["slam_trans64"][so:so + L].copy())[None],
                   "ori_slam_rot_mat": torch.from_numpy(row[:, 20:].copy().reshape(L, 3, 3))[None]}
            alone = stage1.estimate_head_pose(hn, gn, one, lengths=[T - 1], pose_lengths=[L])[0]
            assert torch.equal(alone[0, :L], pose[b, :L]) and not pose[b, L:].any(), b
    assert torch.isfinite(pose).all()


# ---------------------------------------------------------------------------------------------- 8. the trainer and the tools
def _train_seqs():
    return [real_seq(T, 800 + i, T + (i % 2)) for i, T in enumerate((18, 25, 31, 20, 40, 22))]


def _trainer(tmp, model_seed):
    W = 16
    torch.manual_seed(model_seed)
    m = stage1.HeadFormer(_opt(W, 1), torch.device("cuda")).cuda()
    seqs = _train_seqs()
    train = stage1_data.HeadBatches(seqs[:5], 2, window=W, seed=11)
    val = stage1_data.HeadBatches(seqs[4:], 2, window=W, train=False, shuffle=False, seed=11)
    assert (len(train), len(val)) == (3, 1)
    return Stage1Trainer(m, train, val, save_dir=str(tmp), save_interval=1), train


def test_trainer_over_head_batches_resumes_to_the_same_bits(tmp_path):
    """3 epochs straight against 2 epochs, a checkpoint, fresh objects, load and 1 epoch: the same `history`, which needs the
    batches' epoch and shuffle generator from the checkpoint's data_state."""
    a, _ = _trainer(tmp_path / "a", 1)
    for e in range(3):
        torch.manual_seed(20 + e)
        a.train(1)
    assert len(a.history) == 3 and all(math.isfinite(h["loss"]) and h["loss"] > 0 for h in a.history) and len(a.val_history) == 3
    b, _ = _trainer(tmp_path / "b", 1)
    for e in range(2):
        torch.manual_seed(20 + e)
        b.train(1)
    ck = torch.load(tmp_path / "b" / "weights" / "train-2.pt", map_location="cpu")
    assert ck["data_state"]["epoch"] == 2
    c, c_train = _trainer(tmp_path / "b", 9)                                # other weights, batches at epoch 0
    c.load(str(tmp_path / "b" / "weights" / "train-2.pt"))
    assert c.epoch == 2 and c_train.epoch == 2
    torch.manual_seed(22)
    c.train(1)
    assert b.history == a.history[:2] and c.history == a.history[2:]
    pa, pc = a.model.state_dict(), c.model.state_dict()
    assert all(torch.equal(pa[k], pc[k]) for k in pa)
    d, _ = _trainer(tmp_path / "b", 9)                                      # without the data state: other batches
    d.model.load_state_dict(ck["transformer_encoder_state_dict"])
    d.optimizer.load_state_dict(ck["optimizer_state_dict"])
    d.epoch = 2
    torch.manual_seed(22)
    d.train(1)
    assert d.history != a.history[2:]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_on_an_ares_tree(tmp_path, capsys):
    """tools/train_stage1.py --kind headnet --data_root TMP (in this process: the test is about the tool's loop), 2 epochs on a
    temporary ARES tree with a feature cache; the checkpoint loads into a fresh HeadFormer; tools/eval_stage1.py on it (GravityNet
    on seeded weights) prints finite metrics."""
    root, out = str(tmp_path / "data"), tmp_path / "run"
    seqs = _train_seqs() + [real_seq(12, 899, 12)]                          # the last one is shorter than the window: filtered
    O.write_ares_tree(root, seqs, stage1.ARES_SRC_ROOT)
    cache = str(tmp_path / "cache" / "feats")
    common = ["--data_root", root, "--window", "16", "--n_dec_layers", "1", "--feature_cache", cache]
    _tool("train_stage1").main(["--kind", "headnet", "--save_dir", str(out), "--epochs", "2", "--batch_size", "4", "--save_interval", "2"]
                               + common)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["epoch"] for l in lines[:2]] == [1, 2] and math.isfinite(lines[1]["train"]["loss"]) and "val" in lines[0]
    assert os.path.exists(cache + ".train.npz") and os.path.exists(cache + ".test.npz")
    ck = torch.load(out / "weights" / "train-2.pt", map_location="cpu", weights_only=True)
    assert ck["data_state"]["epoch"] == 2
    stage1.HeadFormer(_opt(16, 1), torch.device("cuda")).load_state_dict(ck["transformer_encoder_state_dict"])
    _tool("eval_stage1").main(["--headnet", str(out / "weights" / "train-2.pt"), "--normal_window", "31", "--normal_n_dec_layers", "1",
                               "--batch_size", "4"] + common)
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["sequences"] == 6 and res["dropped"] == {"short": 0, "no_slam": 0}
    assert all(math.isfinite(res[k]) and res[k] >= 0 for k in ("s1_head_dist", "s1_head_dist_rot_only", "s1_head_trans_err_mm"))
