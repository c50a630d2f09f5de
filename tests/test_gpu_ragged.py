"""Ragged stage 2 on the GPU: windows of different lengths in one batch (lengths= / window_ids= of the engine, the model and the
ragged sliding-window harness).

The reference for a ragged window is the oracle run on that window ALONE at its own length — what the reference computes when it
calls the denoiser on a shorter window (M:355-356) — at the project's bar (POSE_TOL = 1e-3, BASELINE north star).  Windows of one
length are handed to the oracle as one batch (it treats the windows of a batch independently), each reference is computed once.
Every attention form of the dispatch takes part, named by the kernels the launch sites record, with lengths at the key-tile edges;
independence, uniform equivalence and the reuse of the captured step are bit-for-bit checks."""
import functools

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

from egoego_release_amd import ModelConfig, make_weights, _lib, harness
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O
from oracle import harness_oracle as HO
from attention_forms import P3, P8, P9, S6, S3, S2, AW, CS, LENGTHS, FORMS, lens as _lens  # noqa: F401

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-3


@functools.lru_cache(maxsize=None)
def _weights(T):
    return make_weights(ModelConfig(max_timesteps=T + 1), 0)


@functools.lru_cache(maxsize=4)
def _model(T, prec):
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(_weights(T), strict=False)
    m.hip_precision = prec
    m = m.cuda()
    eng = m.hip_engine()
    assert m.hip_precision_used == prec and m._slot.plan["flags"] == 0
    return m, eng


def _inputs(T, B, seed):
    g = torch.Generator().manual_seed(seed)
    x, xc, nz = (torch.randn(B, T, 198, generator=g) for _ in range(3))  # (the padded frames hold random values too)
    t = torch.randint(1, 1000, (B,), generator=g)
    return x, xc, nz, t


def _per_window(fn, lens):
    """fn(rows, n) -> [len(rows), n, D] for the windows `rows` cut to their common length n; -> {window: [n, D]}"""
    out = {}
    for n in sorted(set(lens)):
        rows = [b for b, v in enumerate(lens) if v == n]
        res = fn(rows, n)
        out.update({b: res[i] for i, b in enumerate(rows)})
    return out


@functools.lru_cache(maxsize=None)
def _oracle_step(T, B):
    """The oracle's denoiser output and p_sample result of every window alone at its own length (computed once per (T, B))."""
    sd, sched = _weights(T), O.make_schedule(1000)
    x, xc, nz, t = _inputs(T, B, 100 * T + B)
    lens = _lens(T, B)
    den = _per_window(lambda r, n: O.denoise(sd, torch.cat((x[r, :n], xc[r, :n]), -1), t[r]), lens)
    smp = _per_window(lambda r, n: O.p_sample(sd, sched, x[r, :n], t[r], xc[r, :n], nz[r, :n]), lens)
    return lens, den, smp


def _worst(got, want, lens):
    return max(float((got[b, :n].cpu() - want[b]).abs().max()) for b, n in enumerate(lens))


@pytest.mark.parametrize("prec, T, B, qkv, attn", FORMS)
def test_forward_and_p_sample_per_window_against_the_oracle(prec, T, B, qkv, attn):
    """(a) one ragged forward and one ragged p_sample step through every attention form; every window's real frames against the
    oracle on that window alone."""
    m, eng = _model(T, prec)
    lens, den, smp = _oracle_step(T, B)
    x, xc, nz, t = (v.cuda() for v in _inputs(T, B, 100 * T + B))
    out = eng.denoise(x, xc, t, lengths=lens)
    assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)
    assert bool(torch.isfinite(out).all())  # rows past a window's length: unspecified but finite
    e_den = _worst(out, den, lens)
    x1 = eng.p_sample_(x.clone(), xc, t, noise=nz, lengths=torch.tensor(lens, device="cuda", dtype=torch.int32))  # (a CUDA tensor is taken as given)
    assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)
    assert bool(torch.isfinite(x1).all())
    e_smp = _worst(x1, smp, lens)
    print(f"precision {prec} T={T} B={B} {attn}: denoise {e_den:.2e} p_sample {e_smp:.2e}")
    assert e_den < POSE_TOL and e_smp < POSE_TOL, (e_den, e_smp)


def _chain(eng, x, xc, lens, ids, seed=1234, n=8, prefix=None):
    x = x.clone()
    eng.sample_loop_(x, xc, 999, n, noise_mode=_lib.NOISE_PHILOX, seed=seed, prefix=prefix, lengths=lens, window_ids=ids)
    return x


def _garbage(x, lens, seed):
    """x with other random values in the frames past every window's length"""
    g = torch.Generator().manual_seed(seed)
    y = x.clone()
    for b, n in enumerate(lens):
        y[b, n:] = torch.randn(y.shape[1] - n, y.shape[2], generator=g).to(y.device)
    return y


@pytest.mark.parametrize("prec", [P3, P9])
def test_a_windows_rows_depend_on_that_window_only(prec):
    """(b) window b of a ragged batch of 25, bit for bit: the same window in a batch of one (same padded T, length and id), after one
    forward and after 8 Philox steps; and in a batch whose OTHER windows have other lengths and whose padded frames hold other values."""
    T, B = 120, 25
    m, eng = _model(T, prec)
    lens = _lens(T, B)
    ids = [1000 + 7 * b for b in range(B)]
    x, xc, _, t = (v.cuda() for v in _inputs(T, B, 77))
    out = eng.denoise(x, xc, t, lengths=lens)
    end = _chain(eng, x, xc, lens, ids)
    for b, n in enumerate(lens):
        one = eng.denoise(x[b:b + 1].contiguous(), xc[b:b + 1].contiguous(), t[b:b + 1].contiguous(), lengths=[n])
        assert torch.equal(one[0, :n], out[b, :n]), (b, n)
        one = _chain(eng, x[b:b + 1].contiguous(), xc[b:b + 1].contiguous(), [n], [ids[b]])
        assert torch.equal(one[0, :n], end[b, :n]), (b, n)
    # the even windows keep their lengths and ids, the odd ones get other lengths and ids; every padded frame gets other values
    lens2 = [n if b % 2 == 0 else LENGTHS[T][(b + 3) % 9] for b, n in enumerate(lens)]
    ids2 = [i if b % 2 == 0 else i + 5 for b, i in enumerate(ids)]
    assert any(a != c for a, c in zip(lens, lens2))
    x2, xc2 = _garbage(x, lens, 5), _garbage(xc, lens, 6)
    out2 = eng.denoise(x2, xc2, t, lengths=lens2)
    end2 = _chain(eng, x2, xc2, lens2, ids2)
    for b in range(0, B, 2):
        n = lens[b]
        assert torch.equal(out2[b, :n], out[b, :n]) and torch.equal(end2[b, :n], end[b, :n]), (b, n)
    # a moved window keeps its stream through its id: the batch reversed
    rev = list(range(B))[::-1]
    end3 = _chain(eng, x[rev].contiguous(), xc[rev].contiguous(), [lens[b] for b in rev], [ids[b] for b in rev])
    for i, b in enumerate(rev):
        assert torch.equal(end3[i, :lens[b]], end[b, :lens[b]]), b


@pytest.mark.parametrize("prec, B, qkv", [(P9, 2, S6), (P9, 11, S3), (P9, 22, S2), (P8, 11, S3), (P8, 22, S2), (P9, 25, AW)])
def test_padded_frames_and_other_lengths_do_not_reach_a_window_in_any_int8_form(prec, B, qkv):
    """The int8 forms up to 128 tokens scale V per feature column over the window's keys: the V rows of the keys past a window's
    length must stay out of that scale in EVERY form that has such an epilogue (six, three and two projection workgroups, the
    one-kernel layer).  Bit for bit: other values in every padded frame, other lengths and ids for the odd windows; the even
    windows' real frames after one forward and after 8 Philox steps."""
    T = 120
    m, eng = _model(T, prec)
    lens = [LENGTHS[T][(b + 2) % 9] for b in range(B)]  # (window 0, which every B compares, is a short one: 31 frames)
    ids = [50 + 3 * b for b in range(B)]
    x, xc, _, t = (v.cuda() for v in _inputs(T, B, 900 + B))
    out = eng.denoise(x, xc, t, lengths=lens)
    assert eng.last_kernel("qkv") == qkv
    end = _chain(eng, x, xc, lens, ids)
    lens2 = [n if b % 2 == 0 else LENGTHS[T][(b + 5) % 9] for b, n in enumerate(lens)]
    ids2 = [i if b % 2 == 0 else i + 1000 for b, i in enumerate(ids)]
    assert lens2 != lens and any(n < T for n in lens[::2])
    x2, xc2 = _garbage(x, lens, 15) * 3.0, _garbage(xc, lens, 16)
    for b, n in enumerate(lens):  # (the real frames are the same values, the padded ones three times as large as before)
        x2[b, :n] = x[b, :n]
    out2 = eng.denoise(x2, xc2, t, lengths=lens2)
    assert eng.last_kernel("qkv") == qkv
    end2 = _chain(eng, x2, xc2, lens2, ids2)
    for b in range(0, B, 2):
        n = lens[b]
        assert torch.equal(out2[b, :n], out[b, :n]) and torch.equal(end2[b, :n], end[b, :n]), (b, n)


def test_uniform_equivalence_and_graph_reuse():
    """(c) one engine, one workspace, in this order: uniform, ragged with every length = T and ids = arange, ragged with mixed
    lengths, ragged with other mixed lengths, uniform again.  The first, second and last results are the same bits; the two mixed
    results are what every window gives alone (a captured step serves every lengths array)."""
    T, B, prec = 120, 25, P9
    m, eng = _model(T, prec)
    x, xc, _, _ = (v.cuda() for v in _inputs(T, B, 31))
    pfx = torch.randn(B, 10, 198, generator=torch.Generator().manual_seed(9)).cuda()
    full, ids = [T] * B, list(range(B))
    mixed = [_lens(T, B), _lens(T, B, shift=4)]
    assert mixed[0] != mixed[1] and min(min(v) for v in mixed) >= 10
    res = [_chain(eng, x, xc, None, None, prefix=pfx), _chain(eng, x, xc, full, ids, prefix=pfx),
           _chain(eng, x, xc, mixed[0], ids, prefix=pfx), _chain(eng, x, xc, mixed[1], ids, prefix=pfx),
           _chain(eng, x, xc, None, None, prefix=pfx)]
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[4])
    for lens, got in zip(mixed, res[2:4]):
        assert bool(torch.isfinite(got).all())
        for b, n in enumerate(lens):
            one = _chain(eng, x[b:b + 1].contiguous(), xc[b:b + 1].contiguous(), [n], [b], prefix=pfx[b:b + 1].contiguous())
            assert torch.equal(one[0, :n], got[b, :n]), (b, n)
            assert torch.equal(got[b, :10], pfx[b])  # the in-painted prefix lies inside every window
    assert not torch.equal(res[2], res[3])


@pytest.mark.parametrize("prec", [P3, P8, P9])
def test_short_chain_against_the_oracle(prec):
    """(d) 8 steps with injected noise and a 10-frame prefix on windows of mixed lengths; every window against oracle.p_sample on
    that window alone."""
    T, B, n_steps = 40, 5, 8
    m, eng = _model(T, prec)
    sd, sched = _weights(T), O.make_schedule(1000)
    lens = list(LENGTHS[T])
    g = torch.Generator().manual_seed(41)
    x0, xc = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g)
    steps, pfx = torch.randn(n_steps, B, T, 198, generator=g), torch.rand(B, 10, 198, generator=g) * 2 - 1
    x = x0.clone().cuda()
    eng.sample_loop_(x, xc.cuda(), n_steps - 1, n_steps, noise=steps.cuda(), prefix=pfx.cuda(), lengths=lens)
    worst = 0.0
    for b, n in enumerate(lens):
        w = x0[b:b + 1, :n].clone()
        for i in range(n_steps):
            w = O.p_sample(sd, sched, w, torch.full((1,), n_steps - 1 - i, dtype=torch.long), xc[b:b + 1, :n], steps[i, b:b + 1, :n])
            w[:, :10] = pfx[b]
        worst = max(worst, float((x[b, :n].cpu() - w[0]).abs().max()))
    print(f"precision {prec}: {n_steps}-step ragged chain vs oracle {worst:.2e}")
    assert bool(torch.isfinite(x).all()) and worst < POSE_TOL, worst


# ------------------------------------------------------------------------------------------------ (e) the ragged harness
SEQ_FRAMES = (50, 40, 75, 41, 111)  # two windows with a short last one, one full window, three windows, a second window of 11 frames, four windows
HARNESS_SEQ_LEN, HARNESS_STEPS = 40, 6


def _rand_quat(shape, seed):
    q = np.random.default_rng(seed).standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(q[..., :1] < 0, -q, q)


def _skeleton(seed):
    g = np.random.default_rng(seed)
    off = g.uniform(-0.2, 0.2, (22, 3))
    off[0] = 0
    jmin, jmax = g.uniform(-2.0, -1.0, (22, 3)), g.uniform(1.0, 2.0, (22, 3))
    return harness.SkeletonStats(jmin, jmax, off), HO.SkeletonOracle(jmin, jmax, off)


@functools.lru_cache(maxsize=None)
def _harness_setup(prec):
    """The model of tests/test_harness.py::test_sliding_window_hip_vs_oracle (trained-like output head, synthetic skeleton), five
    head trajectories and every draw of every sequence."""
    cfg = ModelConfig(max_timesteps=HARNESS_SEQ_LEN + 1)
    sd = make_weights(cfg, 0)
    rng = np.random.default_rng(11)
    pose = np.concatenate([rng.uniform(-0.5, 0.5, 66), HO.quat_to_mat(_rand_quat((22,), 40))[:, :2, :].reshape(132)])
    sd["denoise_fn.linear_out.bias"] = torch.from_numpy(pose).float()
    sd["denoise_fn.linear_out.weight"] = sd["denoise_fn.linear_out.weight"] * 0.05
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=False)
    m.hip_precision = prec
    m.sampling_rng = "philox"
    m = m.cuda()
    m.num_timesteps = HARNESS_STEPS
    ds, dso = _skeleton(2)
    g = torch.Generator().manual_seed(5)
    poses, noise = [], []
    for s, T in enumerate(SEQ_FRAMES):
        hq = _rand_quat((T,), 12 + s)
        hp = np.cumsum(rng.standard_normal((T, 3)) * 0.01, 0) + np.array([0.0, 0.0, 1.5])
        poses.append(torch.from_numpy(np.concatenate([hp, hq], -1)).float())
        spans = harness.window_spans(T, HARNESS_SEQ_LEN)
        noise.append({"x_all": torch.randn(1, T, 198, generator=g), "cond": [torch.randn(1, n, 198, generator=g) for _, n in spans],
                      "steps": [torch.randn(HARNESS_STEPS, 1, n, 198, generator=g) for _, n in spans]})
    return sd, m, ds, dso, poses, noise


def test_ragged_harness_against_the_oracle_per_sequence():
    sd, m, ds, dso, poses, noise = _harness_setup(P3)
    # the five cases the lengths were picked for
    assert [harness.window_spans(T, 40) for T in SEQ_FRAMES] == [[(0, 40), (30, 20)], [(0, 40)], [(0, 40), (30, 40), (60, 15)],
                                                                 [(0, 40), (30, 11)], [(0, 40), (30, 40), (60, 40), (90, 21)]]
    aa, root, out_len = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [p.cuda() for p in poses], noise=noise)
    assert out_len.tolist() == [harness.output_frames(T, 40) for T in SEQ_FRAMES] == list(SEQ_FRAMES)
    assert aa.shape == (5, max(SEQ_FRAMES), 22, 3) and root.shape == (5, max(SEQ_FRAMES), 3)
    for s, T in enumerate(SEQ_FRAMES):
        assert not aa[s, T:].any() and not root[s, T:].any()
        hp = poses[s][None]
        aa2, root2 = HO.sliding_window(sd, O.make_schedule(1000), dso, 40, HARNESS_STEPS, hp[..., :3].double().numpy(),
                                       hp[..., 3:].double().numpy(), O.head_condition_mask((1, T, 198)), noise[s])
        e_root = np.abs(root[s, :T].cpu().numpy() - root2[0]).max()
        d = Rot.from_rotvec(aa[s, :T].reshape(-1, 3).cpu().numpy().astype(np.float64)) * Rot.from_rotvec(aa2.reshape(-1, 3)).inv()
        ang = np.abs(d.magnitude())
        print(f"sequence {s} ({T} frames): root {e_root:.2e} rotation {ang.max():.2e} rad")
        assert e_root < 2e-4 and ang.max() < 1e-3, (s, e_root, ang.max())


@pytest.mark.parametrize("prec", [P3, P9])
def test_ragged_harness_philox_is_the_one_sequence_harness(prec):
    """In-kernel Philox noise, a fixed precision: the ragged call over all five sequences = five ragged calls of one sequence each
    with the matching sequence_offset, bit for bit; a sequence whose windows are all full length = the one-sequence harness with
    window_offset."""
    sd, m, ds, dso, poses, noise = _harness_setup(prec)
    draws = [{k: v for k, v in d.items() if k != "steps"} for d in noise]  # x_T and the condition noise injected, the steps in-kernel
    off = 300
    aa, root, out_len = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [p.cuda() for p in poses], noise=draws,
                                                                                   sequence_offset=off)
    assert m.hip_precision_used == prec
    for s, T in enumerate(SEQ_FRAMES):
        a1, r1, l1 = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [poses[s].cuda()], noise=[draws[s]],
                                                                                sequence_offset=off + s)
        assert l1.tolist() == [T] and torch.equal(a1[0], aa[s, :T]) and torch.equal(r1[0], root[s, :T]), s
    # full-length windows only: 40 frames; 111 would need a last span of 40 — it has 21, so 130 = 40 + 3 * 30 stands in
    assert harness.window_spans(111, 40)[-1] == (90, 21) and harness.window_spans(130, 40) == [(0, 40), (30, 40), (60, 40), (90, 40)]
    g = torch.Generator().manual_seed(8)
    rng = np.random.default_rng(3)
    hp = np.concatenate([np.cumsum(rng.standard_normal((130, 3)) * 0.01, 0) + np.array([0.0, 0.0, 1.5]), _rand_quat((130,), 99)], -1)
    long_pose = torch.from_numpy(hp).float()
    long_draws = {"x_all": torch.randn(1, 130, 198, generator=g), "cond": [torch.randn(1, 40, 198, generator=g) for _ in range(4)]}
    a2, r2, l2 = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [poses[0].cuda(), long_pose.cuda(), poses[1].cuda()],
                                                                            noise=[draws[0], long_draws, draws[1]], sequence_offset=off)
    assert l2.tolist() == [50, 130, 40]
    for i, (pose, dr) in ((1, (long_pose, long_draws)), (2, (poses[1], draws[1]))):
        a3, r3 = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, pose[None].cuda(), noise=dr, window_offset=off + i)
        n = pose.shape[0]
        assert torch.equal(a3[0], a2[i, :n]) and torch.equal(r3[0], r2[i, :n]), i


# ------------------------------------------------------------------------------------------------ (f) sample(..., lengths=)
def test_sample_with_lengths_on_motion_windows():
    from egoego_release_amd import motion_data as MD
    from test_harness_golden import REST_OFFSETS
    rng = np.random.default_rng(17)
    frames = [40, 55, 31]
    F = sum(frames)
    seqs = (np.cumsum(rng.standard_normal((F, 3)) * 0.01, 0) + np.array([0.0, 0.0, 0.9]), rng.standard_normal((F, 3)) * 0.3,
            rng.standard_normal((F, 63)) * 0.2, frames)
    mw = MD.build_motion_windows(seqs, REST_OFFSETS, window=40, min_frames=12)
    lens = [int(v) for v in mw.seq_len.tolist()]
    assert lens == [40, 20, 40, 35, 15, 31]
    motion = mw.motion()
    mask = harness.prep_head_condition_mask(motion)
    m, _ = _model(40, P9)
    saved = m.num_timesteps
    try:
        m.num_timesteps = 6
        g = torch.Generator().manual_seed(2)
        noise = {"x_T": torch.randn(motion.shape, generator=g), "cond": torch.randn(motion.shape, generator=g),
                 "steps": torch.randn(6, *motion.shape, generator=g)}
        res = m.sample(motion, mask, noise=noise, lengths=mw.seq_len)
        ref = m.p_sample_loop(motion.shape, motion, mask, noise=noise, lengths=lens)
        full = m.sample(motion, mask, noise=noise)
    finally:
        m.num_timesteps = saved
    assert res.shape == motion.shape and bool(torch.isfinite(res).all())
    for b, n in enumerate(lens):
        assert not res[b, n:].any() and res[b, :n].abs().max() > 0, b
        assert torch.equal(res[b, :n], ref[b, :n])
        # a full window is the uniform call's; a short one is not (its padded frames no longer act as keys)
        assert torch.equal(res[b], full[b]) == (n == 40), b
