"""Host side of the HIP training step: the oracle of tests/train_oracle.py pinned to the module's own plain path, the emulated
split-bf16 products, the binding, and the opt-in flag off the GPU."""
import inspect
import os
import re

import pytest
import torch

import train_oracle as TO
from egoego_release_amd import ModelConfig, make_weights, _lib, train
from egoego_release_amd.model import CondGaussianDiffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**kw):
    cfg = ModelConfig(**kw)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    sd = make_weights(cfg, 0)
    m.load_state_dict(sd, strict=False)
    return cfg, m, sd


def _draws(B, T, seed=3, D=198):
    g = torch.Generator().manual_seed(seed)
    x_start = torch.randn(B, T, D, generator=g) * 0.5
    noise = torch.randn(B, T, D, generator=g)
    cond_mask = torch.ones(B, T, D)
    cond_mask[..., 45:48] = 0
    cond_mask[..., 156:162] = 0
    return x_start, noise, cond_mask


@pytest.mark.parametrize("loss_type,objective", [("l1", "pred_x0"), ("l2", "pred_noise")])
def test_oracle_matches_the_plain_path(loss_type, objective):
    """Nothing forced, dropout off, same state dict and draws: the fp64 oracle and the module's own fp32 plain path (which oracle/
    pins to the reference's goldens) agree on the loss and on every gradient to fp32 rounding (e_32 is a few 1e-6 per tensor)."""
    cfg = ModelConfig(n_dec_layers=2, max_timesteps=13, objective=objective)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type=loss_type)
    sd = make_weights(cfg, 0)
    m.load_state_dict(sd, strict=False)
    m.eval()
    B, T = 3, 11
    x_start, noise, cond_mask = _draws(B, T)
    t = torch.tensor([0, 500, 999])
    pm = torch.ones(B, 1, T + 1).bool()
    pm[1, 0, 6:] = False
    pm[2, 0, 2:] = False
    torch.manual_seed(11)
    cond_noise = torch.randn_like(x_start)
    torch.manual_seed(11)
    loss = m.p_losses(x_start, cond_mask, t, noise=noise, padding_mask=pm)
    loss.backward()
    tables = (m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, m.p2_loss_weight)
    res, grads = TO.loss_and_grads(m.state_dict(), x_start, noise, cond_noise, cond_mask, t, tables, row_mask=pm[:, 0].float(),
                                   objective=objective, loss_type=loss_type)
    assert abs(float(res["loss"]) - float(loss.detach())) <= 2e-6 * abs(float(loss.detach()))
    named = dict(m.named_parameters())
    assert len(grads) == 16 * 2 + 8
    total = torch.sqrt(sum(g.norm() ** 2 for g in grads.values()))
    for k, g in grads.items():
        ref = named[k].grad.double()
        if "w_k.bias" in k:  # identically zero in exact arithmetic: both are rounding noise
            assert g.norm() <= 1e-12 * total and ref.norm() <= 1e-6 * total, k
            continue
        assert TO.rel_err(ref.reshape(g.shape), g) <= 5e-5, k


def test_forcing_own_decisions_changes_nothing():
    cfg, m, sd = _model(n_dec_layers=1, max_timesteps=9)
    B, T = 2, 7
    x_start, noise, cond_mask = _draws(B, T)
    cond_noise = torch.randn(B, T, 198, generator=torch.Generator().manual_seed(4))
    t = torch.tensor([3, 700])
    tables = (m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, m.p2_loss_weight)
    args = (x_start, noise, cond_noise, cond_mask, t, tables)
    r0, g0 = TO.loss_and_grads(m.state_dict(), *args)
    r1, g1 = TO.loss_and_grads(m.state_dict(), *args, relu_masks=[p > 0 for p in r0["ffn_pre"]], loss_sign=torch.sign(r0["diff"]))
    assert float(r0["loss"]) == pytest.approx(float(r1["loss"]), rel=1e-14)
    for k in g0:
        assert torch.allclose(g0[k], g1[k], rtol=1e-12, atol=1e-18), k
    # a flipped decision does change them
    flipped = [~(p > 0) for p in r0["ffn_pre"]]
    _, g2 = TO.loss_and_grads(m.state_dict(), *args, relu_masks=flipped)
    assert TO.rel_err(g2["denoise_fn.linear_out.weight"], g0["denoise_fn.linear_out.weight"]) > 1e-3


def test_split_product_precision():
    """hi*hi + lo*hi + hi*lo keeps about 16 mantissa bits per operand; one bf16 per operand keeps 8."""
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(64, 512, generator=g).double(), torch.randn(512, 48, generator=g).double()
    exact = a.float().double() @ b.float().double()
    e3 = (TO._split_product(a, b) - exact).norm() / exact.norm()
    e1 = (TO._split(a)[0] @ TO._split(b)[0] - exact).norm() / exact.norm()
    assert 1e-7 < e3 < 2e-5 and e1 > 1e-3
    a.requires_grad_(True)
    TO.split_mm(a, b).sum().backward()
    assert TO.rel_err(a.grad, (torch.ones(64, 48).double() @ b.t())) < 2e-5


def test_flag_defaults_off_and_raises_on_cpu():
    cfg, m, sd = _model(n_dec_layers=1, max_timesteps=9)
    assert m.hip_training is False
    x_start, noise, cond_mask = _draws(2, 7)
    torch.manual_seed(0)
    a = m(x_start, cond_mask)
    m.hip_training = True
    with pytest.raises(_lib.EgoEgoHipError):
        m(x_start, cond_mask)
    with pytest.raises(_lib.EgoEgoHipError):
        m.p_losses(x_start, cond_mask, torch.tensor([1, 2]))
    m.hip_training = False
    torch.manual_seed(0)
    assert torch.equal(m(x_start, cond_mask), a)


def test_param_names_cover_the_denoiser():
    cfg, m, sd = _model()
    names = train.param_names(cfg.n_dec_layers)
    assert sorted(names) == sorted(n for n, _ in m.denoise_fn.named_parameters())
    assert len([n for n in names if not n.endswith("position_vec.weight")]) == 72


def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    declared = set(re.findall(r"\b(egoego_train_\w+)\s*\(", text))
    bound = {n for n in _lib.EXPORTS if n.startswith("egoego_train_")}
    assert declared == bound and len(bound) == 9
    assert callable(_lib.check_train)
    assert re.search(r"#define EGOEGO_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    src = open(os.path.join(ROOT, "egoego_release_amd", "csrc", "train_step.h")).read()
    assert f"CHUNK = {_lib.TRAIN_GRAD_CHUNK};" in src and f"MAX_L = {_lib.TRAIN_MAX_L};" in src
    from egoego_release_amd import build
    assert "train_step.hip" in build.SOURCES
    host = open(os.path.join(ROOT, "egoego_release_amd", "csrc", "train_step.hip")).read()
    assert '#include "host_util.h"' in host
    for banned in ("hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomicAdd"):
        assert banned not in host and banned not in src, banned


def test_train_like_tool_has_the_hip_switch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mtl", os.path.join(ROOT, "tools", "make_trained_like_checkpoint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert inspect.signature(mod.train_like).parameters["hip"].default is False
