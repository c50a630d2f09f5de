"""The strided (DDIM) sampler through the sliding-window harnesses, on the GPU: egoego_ddim_loop_ragged (prefix in-painting, row
mask, per-window lengths and Philox ids) from the C ABI up to the two harnesses.

DDIM is not in the reference, so no reference oracle exists for it.  The checker is test_ddim_harness.ddim_ref — the published
update on top of oracle.denoise, pinned there to oracle.ddim_loop — run on every window ALONE at its own length (what the reference
means by a short window, M:355-356), at the bar the existing DDIM-vs-oracle tests hold (POSE_TOL = 1e-3).  Additivity, independence
and the reuse of the captured step are bit-for-bit checks; the tie to the reference's own chain is eta = 1 on the full timestep list.
Common setup: B = 3, one T per key-tile count, lengths [T, 11, T - 7], a 10-frame prefix, six timesteps."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from egoego_release_amd import ModelConfig, make_weights, _lib, harness
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O
from oracle import harness_oracle as HO
from test_ddim_harness import ddim_ref

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-3  # tests/test_gpu_parity.py: the bar of the DDIM-vs-oracle tests
P3, P8, P9 = _lib.PREC_BF16X3, _lib.PREC_I8X3, _lib.PREC_I8X3_FC
PRECS = pytest.mark.parametrize("prec", [P3, P8, P9], ids=["bf16x3", "i8x3", "i8x3fc"])
TS = pytest.mark.parametrize("T", [20, 40, 120, 196])  # 1, 2, 4 and 7 key tiles
B, PFX = 3, 10
STEPS = [900, 700, 500, 300, 100, 0]


def _lens(T):
    return [T, 11, T - 7]


@functools.lru_cache(maxsize=None)
def _weights(T):
    return make_weights(ModelConfig(max_timesteps=T + 1), 0)


@functools.lru_cache(maxsize=None)  # (three windows per engine: every (T, precision) context stays)
def _model(T, prec, graph=True):
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(_weights(T), strict=False)
    m.hip_precision = prec
    m.hip_graph = graph
    m = m.cuda()
    eng = m.hip_engine()
    assert m.hip_precision_used == prec
    return m, eng


@functools.lru_cache(maxsize=None)
def _inputs(T):
    """x_T, x_cond, the injected draws of every step and the prefix, on the host (the padded frames hold random values too)"""
    g = torch.Generator().manual_seed(1000 + T)
    x, xc = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g)
    nz = torch.randn(len(STEPS), B, T, 198, generator=g)
    pre = torch.rand(B, PFX, 198, generator=g) * 2 - 1
    return x, xc, nz, pre


@functools.lru_cache(maxsize=None)
def _reference(T, eta):
    """ddim_ref of every window alone at its own length, with its slice of the draws and its prefix (once per (T, eta))."""
    sd, sched = _weights(T), O.make_schedule(1000)
    x, xc, nz, pre = _inputs(T)
    with torch.no_grad():
        return [ddim_ref(sd, sched, x[b:b + 1, :n], xc[b:b + 1, :n], STEPS, eta, nz[:, b:b + 1, :n], pre[b:b + 1])[0]
                for b, n in enumerate(_lens(T))]


@functools.lru_cache(maxsize=None)
def _reference_masked(T):
    sd, sched = _weights(T), O.make_schedule(1000)
    x, xc, nz, pre = _inputs(T)
    with torch.no_grad():
        return ddim_ref(sd, sched, x, xc, STEPS, 0.5, nz, pre, padding_mask=_mask(T))


def _mask(T):
    pm = torch.ones(B, 1, T + 1).bool()
    pm[0, 0, T - 4:] = False
    pm[1, 0, T // 2 + 1:] = False
    return pm


# ------------------------------------------------------------------------------------------------ 1. additive
@TS
@PRECS
def test_new_arguments_left_out_are_the_uniform_entry_point(T, prec):
    """Every new argument None: the bits of a direct egoego_ddim_loop call.  Every length = T, ids = window_offset + b, no prefix:
    the ragged instantiations give the uniform call's bits."""
    m, eng = _model(T, prec)
    x0, xc = (v.cuda() for v in _inputs(T)[:2])
    seed, off = 77, 40
    for eta, mode in ((0.0, _lib.NOISE_NONE), (0.5, _lib.NOISE_PHILOX)):
        direct = x0.clone()
        ws, n = eng.workspace(B, T)
        arr = (C.c_int32 * len(STEPS))(*STEPS)
        _lib.check(eng.lib.egoego_ddim_loop(eng._ctx, direct.data_ptr(), xc.data_ptr(), arr, len(STEPS), eta, None, mode, seed, off,
                                            B, T, ws, n, eng._stream()))
        a = eng.ddim_loop_(x0.clone(), xc, STEPS, eta=eta, seed=seed, window_offset=off)
        assert torch.equal(a, direct), eta
        b = eng.ddim_loop_(x0.clone(), xc, STEPS, eta=eta, seed=seed, window_offset=off, lengths=[T] * B,
                           window_ids=[off + i for i in range(B)])
        assert torch.equal(b, direct), eta
    assert not torch.equal(a, x0)


# ------------------------------------------------------------------------------------------------ 2. against the restatement
@TS
@PRECS
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_every_window_against_the_restatement_at_its_own_length(T, prec, eta):
    m, eng = _model(T, prec)
    x0, xc, nz, pre = (v.cuda() for v in _inputs(T))
    lens = _lens(T)
    want = _reference(T, eta)
    x = eng.ddim_loop_(x0.clone(), xc, STEPS, eta=eta, noise=nz if eta > 0 else None, prefix=pre, lengths=lens)
    assert bool(torch.isfinite(x).all())  # rows past a window's length: unspecified but finite
    worst = max(float((x[b, :n].cpu() - want[b]).abs().max()) for b, n in enumerate(lens))
    print(f"precision {prec} T={T} eta={eta}: strided ragged chain vs restatement {worst:.2e}")
    assert worst < POSE_TOL, worst
    assert torch.equal(x[:, :PFX], pre)  # re-imposed after the last step too: the prefix's own bits


# ------------------------------------------------------------------------------------------------ 3. independence
@TS
@PRECS
def test_a_windows_rows_do_not_depend_on_its_neighbours(T, prec):
    """Philox at eta = 0.5 with explicit ids: a window's real rows are the same bits alone, at another batch position and among
    other lengths (whose padded frames hold other values)."""
    m, eng = _model(T, prec)
    x0, xc, _, pre = (v.cuda() for v in _inputs(T))
    lens, ids = _lens(T), [500, 77, 3]

    def run(rows, ln, x=x0, cond=xc):
        r = torch.as_tensor(rows, device="cuda")
        return eng.ddim_loop_(x[r].contiguous(), cond[r].contiguous(), STEPS, eta=0.5, noise_mode=_lib.NOISE_PHILOX, seed=21,
                              prefix=pre[r].contiguous(), lengths=ln, window_ids=[ids[b] for b in rows])

    full = run([0, 1, 2], lens)
    rev = run([2, 1, 0], lens[::-1])
    g = torch.Generator().manual_seed(4)
    x2, xc2 = x0.clone(), xc.clone()
    for b, n in enumerate(lens):
        x2[b, n:] = torch.randn(T - n, 198, generator=g).cuda()
        xc2[b, n:] = torch.randn(T - n, 198, generator=g).cuda()
    for b, n in enumerate(lens):
        alone = run([b], [n])
        assert torch.equal(alone[0, :n], full[b, :n]), (b, n)
        assert torch.equal(rev[2 - b, :n], full[b, :n]), (b, n)
        others = [n if i == b else max(PFX, (v * 2) // 3) for i, v in enumerate(lens)]
        among = run([0, 1, 2], others, x2, xc2)
        assert torch.equal(among[b, :n], full[b, :n]), (b, n)
    other_id = eng.ddim_loop_(x0[:1].contiguous(), xc[:1].contiguous(), STEPS, eta=0.5, noise_mode=_lib.NOISE_PHILOX, seed=21,
                              prefix=pre[:1].contiguous(), lengths=[lens[0]], window_ids=[ids[0] + 1])
    assert not torch.equal(other_id[0], full[0])  # the id selects the stream


# ------------------------------------------------------------------------------------------------ 4. tie to the reference's chain
@PRECS
def test_eta1_on_the_full_list_is_the_ancestral_ragged_chain(prec):
    """eta = 1 on 999..0 is algebraically the ancestral chain (sig_t^2 = posterior variance, same mean) and draws the same Philox
    stream at every timestep: with the prefix, the lengths and the ids it lands on sample_loop_ within the 3e-4 that
    test_ddim_eta1_full_chain_is_the_ddpm_chain holds for the uniform call; eta = 0 does not."""
    T = 20
    m, eng = _model(T, prec)
    x0, xc, _, pre = (v.cuda() for v in _inputs(T))
    lens, ids = _lens(T), [9, 4, 300]
    kw = dict(seed=9, window_offset=5, prefix=pre, lengths=lens, window_ids=ids)
    a = eng.sample_loop_(x0.clone(), xc, 999, 1000, noise_mode=_lib.NOISE_PHILOX, **kw)
    every = list(range(999, -1, -1))
    b = eng.ddim_loop_(x0.clone(), xc, every, eta=1.0, **kw)
    c = eng.ddim_loop_(x0.clone(), xc, every, eta=0.0, **kw)
    d1 = max(float((a[i, :n] - b[i, :n]).abs().max()) for i, n in enumerate(lens))
    d0 = max(float((a[i, :n] - c[i, :n]).abs().max()) for i, n in enumerate(lens))
    print(f"precision {prec}: eta=1 full list vs the ancestral ragged chain {d1:.2e}; eta=0 {d0:.2e}")
    assert d1 < 3e-4, d1
    assert d0 > 1e-3, d0


# ------------------------------------------------------------------------------------------------ 5. graph reuse
@TS
@PRECS
def test_one_captured_step_serves_other_arrays_buffers_and_lists(T, prec):
    """Two calls of one shape with different length arrays, prefix buffers and timestep lists: each the bits of the same call on an
    EGOEGO_FLAG_NO_GRAPH engine (the second replays the step the first captured)."""
    m, eng = _model(T, prec)
    m2, eng2 = _model(T, prec, False)
    x0, xc, _, pre = (v.cuda() for v in _inputs(T))
    pre2 = (torch.rand(B, PFX, 198, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    calls = [(_lens(T), pre, STEPS, [3, 4, 5]), ([T - 1, T, PFX], pre2, [999, 650, 333, 120, 7], [60, 2, 11])]
    got = []
    for lens, p, ts, ids in calls:
        kw = dict(eta=0.5, noise_mode=_lib.NOISE_PHILOX, seed=5, prefix=p, lengths=lens, window_ids=ids)
        u = eng.ddim_loop_(x0.clone(), xc, ts, **kw)
        v = eng2.ddim_loop_(x0.clone(), xc, ts, **kw)
        assert torch.equal(u, v), lens
        assert torch.equal(u[:, :PFX], p)
        got.append(u)
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------ 6. row mask
@TS
@PRECS
def test_row_mask_against_the_restatement(T, prec):
    """A [B, T + 1] padding mask reaches every step of the strided loop like it reaches the ancestral one's (M:259, 268)."""
    m, _ = _model(T, prec)
    eng = m.hip_engine(masked=True)
    x0, xc, nz, pre = (v.cuda() for v in _inputs(T))
    pm = _mask(T)
    x = eng.ddim_loop_(x0.clone(), xc, STEPS, eta=0.5, noise=nz, prefix=pre, row_mask=pm.reshape(B, T + 1).cuda())
    want = _reference_masked(T)
    err = float((x.cpu() - want).abs().max())
    free = float((eng.ddim_loop_(x0.clone(), xc, STEPS, eta=0.5, noise=nz, prefix=pre).cpu() - want).abs().max())
    print(f"precision {prec} T={T}: masked strided chain vs restatement {err:.2e} (unmasked: {free:.2e})")
    assert err < POSE_TOL, err
    assert free > POSE_TOL  # the mask matters


# ------------------------------------------------------------------------------------------------ 7. the harnesses
SEQ_LEN, N_STEPS = 120, 6
SEQ_FRAMES, N_SMP = (40, 140, 250), 2


def _rand_quat(shape, seed):
    q = np.random.default_rng(seed).standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(q[..., :1] < 0, -q, q)


def _trajectory(n, seed):
    rng = np.random.default_rng(seed)
    hp = np.cumsum(rng.standard_normal((n, 3)) * 0.01, 0) + np.array([0.0, 0.0, 1.5])
    return torch.from_numpy(np.concatenate([hp, _rand_quat((n,), seed + 100)], -1)).float()


@functools.lru_cache(maxsize=None)
def _harness_setup(prec):
    """The model of tests/test_gpu_ragged.py's harness tests (trained-like output head, synthetic skeleton) at seq_len = 120, with
    the whole 1000-step schedule: the strided sampler walks ddim_timesteps(6) of it."""
    cfg = ModelConfig(max_timesteps=SEQ_LEN + 1)
    sd = make_weights(cfg, 0)
    rng = np.random.default_rng(11)
    pose = np.concatenate([rng.uniform(-0.5, 0.5, 66), HO.quat_to_mat(_rand_quat((22,), 40))[:, :2, :].reshape(132)])
    sd["denoise_fn.linear_out.bias"] = torch.from_numpy(pose).float()
    sd["denoise_fn.linear_out.weight"] = sd["denoise_fn.linear_out.weight"] * 0.05
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=False)
    m.hip_precision = prec
    m.sampling_rng = "philox"
    m.philox_seed = 17
    m = m.cuda()
    g = np.random.default_rng(2)
    off = g.uniform(-0.2, 0.2, (22, 3))
    off[0] = 0
    ds = harness.SkeletonStats(g.uniform(-2.0, -1.0, (22, 3)), g.uniform(1.0, 2.0, (22, 3)), off)
    return m, ds


def _draws(n, frames, seed):
    g = torch.Generator().manual_seed(seed)
    return {"x_all": torch.randn(n, frames, 198, generator=g),
            "cond": [torch.randn(n, w, 198, generator=g) for _, w in harness.window_spans(frames, SEQ_LEN)]}


@PRECS
def test_one_sequence_harness_runs_the_strided_sampler_per_window(prec):
    """A 140-frame trajectory (windows of 120 and 30 frames), six steps, x_T and the condition noise injected.  The first window of
    the result is convert_model_res_to_data of a direct ddim_loop_ call on that window's condition, bit for bit, at eta = 0 and at
    eta = 0.5 (seed philox_seed + window index); sampler="ddpm" is the call without the argument."""
    m, ds = _harness_setup(prec)
    assert harness.window_spans(140, SEQ_LEN) == [(0, 120), (110, 30)]
    pose = _trajectory(140, 5)[None].cuda()
    nz = _draws(1, 140, 8)
    ts = m.ddim_timesteps(N_STEPS)
    assert ts == [999, 799, 599, 400, 200, 0]
    cm = harness.prep_head_condition_mask(torch.zeros(1, SEQ_LEN, 198, device="cuda"))
    for eta in (0.0, 0.5):
        aa, root = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, pose, noise=nz, window_offset=31, sampler="ddim",
                                                                       n_steps=N_STEPS, eta=eta)
        assert aa.shape == (1, 140, 22, 3) and root.shape == (1, 140, 3) and bool(torch.isfinite(aa).all())
        jpos, jquat = pose[:, :SEQ_LEN, :3].contiguous(), pose[:, :SEQ_LEN, 3:].contiguous()
        x_start, recover = harness._window_condition_hip(ds, jpos, jquat)
        x_cond = (x_start * (1.0 - cm) + cm * nz["cond"][0].cuda()).float().contiguous()
        x = nz["x_all"][:, :SEQ_LEN].cuda().contiguous().clone()
        m.hip_engine().ddim_loop_(x, x_cond, ts, eta=eta, seed=m.philox_seed, window_offset=31)
        aa0, root0, _ = harness.convert_model_res_to_data(ds, x, recover, jpos)
        assert torch.equal(aa[:, :SEQ_LEN], aa0) and torch.equal(root[:, :SEQ_LEN], root0), eta
    # the default sampler is untouched: the ancestral chain (a short schedule keeps it quick)
    saved = m.num_timesteps
    try:
        m.num_timesteps = N_STEPS
        a1, r1 = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, pose, noise=nz, window_offset=31)
        a2, r2 = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, pose, noise=nz, window_offset=31, sampler="ddpm")
        a3, r3, _ = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [pose[0]], noise=[nz], sequence_offset=31)
        a4, r4, _ = harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, ds, [pose[0]], noise=[nz], sequence_offset=31,
                                                                                sampler="ddpm", n_steps=3, eta=0.0)
    finally:
        m.num_timesteps = saved
    assert torch.equal(a1, a2) and torch.equal(r1, r2) and torch.equal(a3, a4) and torch.equal(r3, r4)
    assert not torch.equal(a1, aa)


@PRECS
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ragged_harness_with_the_strided_sampler_is_the_one_sequence_harness(prec, eta):
    """Trajectories of 40, 140 and 250 frames x 2 samples through the ragged harness with sampler="ddim" against the one-sequence
    harness per sequence at window_offset = sequence_offset + s * n: the agreement tests/test_gpu_ragged.py asserts between the two
    harnesses for the ancestral chain — the same bits."""
    m, ds = _harness_setup(prec)
    off = 300
    poses = [_trajectory(f, 20 + s) for s, f in enumerate(SEQ_FRAMES)]
    draws = [_draws(N_SMP, f, 30 + s) for s, f in enumerate(SEQ_FRAMES)]
    aa, root, out_len = harness.full_body_gen_cond_head_pose_sliding_window_ragged(
        m, ds, [p.cuda() for p in poses], samples_per_sequence=N_SMP, noise=draws, sequence_offset=off, sampler="ddim", n_steps=N_STEPS, eta=eta)
    assert out_len.tolist() == [f for f in SEQ_FRAMES for _ in range(N_SMP)]
    assert m.hip_precision_used == prec
    single = []
    for s, f in enumerate(SEQ_FRAMES):
        rows = slice(s * N_SMP, (s + 1) * N_SMP)
        assert not aa[rows, f:].any() and not root[rows, f:].any()
        a1, r1 = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, poses[s][None].repeat(N_SMP, 1, 1).cuda(), noise=draws[s],
                                                                     window_offset=off + s * N_SMP, sampler="ddim", n_steps=N_STEPS, eta=eta)
        single.append((a1, r1))
    print(f"precision {prec} eta={eta}: ragged vs one-sequence harness (frames, max |d aa|, max |d root|):",
          [(f, float((a1 - aa[s * N_SMP:(s + 1) * N_SMP, :f]).abs().max()), float((r1 - root[s * N_SMP:(s + 1) * N_SMP, :f]).abs().max()))
           for (s, f), (a1, r1) in zip(enumerate(SEQ_FRAMES), single)])
    for (s, f), (a1, r1) in zip(enumerate(SEQ_FRAMES), single):
        rows = slice(s * N_SMP, (s + 1) * N_SMP)
        assert torch.equal(a1, aa[rows, :f]) and torch.equal(r1, root[rows, :f]), (s, f)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_bad_arguments_are_the_librarys_error_not_a_launch():
    T = 20
    m, eng = _model(T, P3)
    x0, xc, nz, pre = (v.cuda() for v in _inputs(T))
    x = x0.clone()
    with pytest.raises(_lib.EgoEgoHipError, match="eta"):
        eng.ddim_loop_(x, xc, STEPS, eta=1.5, prefix=pre, lengths=_lens(T))
    with pytest.raises(_lib.EgoEgoHipError, match="noise source"):
        eng.ddim_loop_(x, xc, STEPS, eta=0.5, noise_mode=_lib.NOISE_NONE, prefix=pre, lengths=_lens(T))
    with pytest.raises(_lib.EgoEgoHipError, match="prefix_len"):
        eng.ddim_loop_(x, xc, STEPS, prefix=torch.zeros(B, T + 1, 198, device="cuda"))
    with pytest.raises(_lib.EgoEgoHipError, match="strictly descending"):
        eng.ddim_loop_(x, xc, [5, 7], prefix=pre)
    with pytest.raises(ValueError, match="prefix"):  # the host check of the lengths comes before the library
        eng.ddim_loop_(x, xc, STEPS, prefix=pre, lengths=[T, PFX - 1, T])
    torch.cuda.synchronize()
    assert torch.equal(x, x0)  # nothing was launched
