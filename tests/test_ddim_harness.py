"""The strided (DDIM) sampler behind the sliding-window harnesses: everything that needs no GPU.

The ABI entry (egoego_ddim_loop_ragged), the public timestep list, the host-side validation of the new arguments, and `ddim_ref`:
the restatement tests/test_gpu_ddim_harness.py checks the GPU against.  DDIM is not in the reference, so there is no reference
oracle: `ddim_ref` restates the published update (Song et al. 2021, eq. 12 / 16) on top of oracle.denoise with the coefficients in
float64 as include/egoego_hip.h gives them, plus the prefix overwrite after every step (the reference's in-painting of its own
chain, M:395-397) — and is itself pinned to oracle.ddim_loop here."""
import os

import numpy as np
import pytest
import torch

from egoego_release_amd import ModelConfig, make_weights, _lib, harness
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ddim_ref(sd, sched, x, x_cond, ts, eta=0.0, noise=None, prefix=None, padding_mask=None):
    """x [B,T,D] after the strided chain over the descending list `ts`:
        sig = eta sqrt((1 - abar_prev) / (1 - abar_t)) sqrt(1 - abar_t / abar_prev),   abar_prev = 1 after the last entry
        x  <- sqrt(abar_prev) x0 + sqrt(1 - abar_prev - sig^2) eps + sig noise[i],     eps = (x - sqrt(abar_t) x0) / sqrt(1 - abar_t)
    with x0 = clamp(denoiser output) (pred_x0), then x[:, :P] <- prefix after EVERY step, the last included."""
    abar = sched["alphas_cumprod"].double()
    x = x.clone()
    for i, t in enumerate(ts):
        tt = torch.full((x.shape[0],), int(t), dtype=torch.long)
        x0 = O.denoise(sd, torch.cat((x, x_cond), dim=-1), tt, padding_mask=padding_mask).clamp(-1.0, 1.0)
        a_t = abar[t]
        a_prev = abar[ts[i + 1]] if i + 1 < len(ts) else torch.tensor(1.0, dtype=torch.float64)
        sig = torch.tensor(0.0, dtype=torch.float64)
        if eta > 0 and a_prev < 1 and a_t < 1:
            sig = eta * ((1 - a_prev) / (1 - a_t)).sqrt() * (1 - a_t / a_prev).clamp(min=0).sqrt()
        eps = (x - a_t.sqrt().float() * x0) / (1 - a_t).float().clamp(min=1e-20).sqrt()
        x = a_prev.sqrt().float() * x0 + (1 - a_prev - sig * sig).clamp(min=0).sqrt().float() * eps
        if eta > 0:
            x = x + sig.float() * noise[i]
        if prefix is not None:
            x[:, :prefix.shape[1]] = prefix
    return x


def _cpu_model(T=20):
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    return cfg, m


def test_the_ragged_strided_loop_is_exported_and_declared():
    assert "egoego_ddim_loop_ragged" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    assert "int egoego_ddim_loop_ragged(egoego_ctx* ctx" in src
    assert "NOT ragged: egoego_ddim_loop" not in src  # the sentence that said the strided loop takes one T
    assert _lib.ABI_VERSION == 8  # additive: the version stays


@pytest.mark.parametrize("n", [1, 2, 12, 50, 1000])
def test_ddim_timesteps_is_the_list_ddim_sample_walks(n):
    _, m = _cpu_model()
    assert m.num_timesteps == 1000
    ts = m.ddim_timesteps(n)
    assert ts == sorted({int(round(v)) for v in np.linspace(0, m.num_timesteps - 1, n)}, reverse=True)
    assert all(a > b for a, b in zip(ts, ts[1:])) and ts[-1] == 0 and len(ts) == n
    assert all(isinstance(v, int) for v in ts)


def _head_pose(n_seq, n_frames):
    hp = torch.zeros(n_seq, n_frames, 7)
    hp[..., 3] = 1.0
    return hp


def test_an_unknown_sampler_raises_before_anything_runs():
    """The module sits on the CPU, where taking the engine raises EgoEgoHipError: a ValueError shows the check came first."""
    _, m = _cpu_model()
    hp = _head_pose(1, 30)
    data = torch.zeros(1, 30, 198)
    cm = harness.prep_head_condition_mask(data)
    with pytest.raises(ValueError, match="unknown sampler"):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="dpm")
    with pytest.raises(ValueError, match="unknown sampler"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, None, [hp[0]], sampler="dpm")
    with pytest.raises(ValueError, match="unknown sampler"):
        m.sample_sliding_window_w_canonical(None, hp[..., :3], hp[..., 3:], data, cm, sampler="dpm")
    assert m.denoise_fn.training  # (the check runs before the module's mode is touched)
    with pytest.raises(ValueError, match="unknown sampler"):
        m.p_sample_loop_sliding_window_w_canonical(None, data.shape, hp[..., :3], hp[..., 3:], cm, sampler="dpm")
    # the default is the ancestral chain and reaches the engine: on the CPU that is the library's error, not a ValueError
    with pytest.raises(_lib.EgoEgoHipError):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="ddpm")


def test_eta_needs_the_philox_stream_unless_every_step_is_injected():
    _, m = _cpu_model()
    hp = _head_pose(1, 30)
    assert m.sampling_rng == "torch"
    with pytest.raises(ValueError, match="philox"):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="ddim", n_steps=6, eta=0.5)
    with pytest.raises(ValueError, match="philox"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, None, [hp[0]], sampler="ddim", n_steps=6, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="ddim", eta=1.5)
    # eta == 0 draws nothing per step: any sampling_rng passes the check (and then meets the missing GPU)
    with pytest.raises(_lib.EgoEgoHipError):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="ddim", n_steps=6, eta=0.0)
    with pytest.raises(_lib.EgoEgoHipError):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(m, None, [hp[0]], sampler="ddim", n_steps=6, eta=0.0)
    # injected steps stand in for the stream; Philox satisfies it
    steps = {"x_all": torch.zeros(1, 30, 198), "cond": [torch.zeros(1, 30, 198)], "steps": [torch.zeros(6, 1, 30, 198)]}
    assert harness.sampler_timesteps(m, "ddim", 6, 0.5, True) == m.ddim_timesteps(6)
    with pytest.raises(_lib.EgoEgoHipError):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, noise=steps, sampler="ddim", n_steps=6, eta=0.5)
    m.sampling_rng = "philox"
    with pytest.raises(_lib.EgoEgoHipError):
        harness.full_body_gen_cond_head_pose_sliding_window(m, None, hp, sampler="ddim", n_steps=6, eta=0.5)
    assert harness.sampler_timesteps(m, "ddpm", 6, 0.5, False) is None


def test_a_prefix_longer_than_the_shortest_window_raises_on_the_host():
    from egoego_release_amd.engine import check_lengths
    _, m = _cpu_model()
    xs = torch.zeros(3, 20, 198)
    cm = harness.prep_head_condition_mask(xs)
    with pytest.raises(ValueError, match="prefix"):
        m.ddim_sample(xs, cm, n_steps=6, lengths=[20, 9, 13], prefix=torch.zeros(3, 10, 198))
    with pytest.raises(ValueError, match="1..20"):
        m.ddim_sample(xs, cm, n_steps=6, lengths=[20, 21, 13])
    with pytest.raises(_lib.EgoEgoHipError):  # a prefix that fits passes the check (and then meets the missing GPU)
        m.ddim_sample(xs, cm, n_steps=6, lengths=[20, 10, 13], prefix=torch.zeros(3, 10, 198))
    assert check_lengths([20, 10, 13], 3, 20, 10).tolist() == [20, 10, 13]


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_the_restatement_without_prefix_is_the_oracles_ddim_loop(eta):
    B, T = 1, 20
    cfg, _ = _cpu_model(T)
    sd, sched = make_weights(cfg, 0), O.make_schedule(1000)
    ts = [900, 700, 500, 300, 100, 0]
    g = torch.Generator().manual_seed(3)
    x, xc, nz = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g), torch.randn(len(ts), B, T, 198, generator=g)
    with torch.no_grad():
        want = O.ddim_loop(sd, sched, x.clone(), xc, ts, eta=eta, noise=nz)
        got = ddim_ref(sd, sched, x, xc, ts, eta, nz, None)
        pre = torch.rand(B, 10, 198, generator=g) * 2 - 1
        with_prefix = ddim_ref(sd, sched, x, xc, ts, eta, nz, pre)
    assert torch.equal(got, want)
    assert torch.equal(with_prefix[:, :10], pre) and not torch.equal(with_prefix[:, 10:], want[:, 10:])  # the prefix reaches the free frames
