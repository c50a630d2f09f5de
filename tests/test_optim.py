"""Host side of the fused parameter update: the fp64 oracle of tests/optim_oracle.py pinned to torch.optim.Adam, the binding, the
state dicts FusedAdam and torch.optim.Adam exchange, the EMA schedule where it changes regime, and the trainer's plain path."""
import copy
import importlib.util
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import optim_oracle as OO
from egoego_release_amd import ModelConfig, make_weights, _lib, optim
from egoego_release_amd.model import CondGaussianDiffusion
from egoego_release_amd.trainer import Stage2Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egoego_release_amd", "csrc")


def _lists(seed=0, sizes=(1, 3, 198, 700)):
    g = torch.Generator().manual_seed(seed)
    p = [torch.randn(n, generator=g) * 0.05 for n in sizes]
    grads = [[torch.randn(n, generator=g) * 10.0 ** (-6 * torch.rand(n, generator=g)) for n in sizes] for _ in range(10)]
    return p, grads


def test_oracle_matches_torch_adam_over_ten_steps():
    """The oracle carries fp64 state from fp32 inputs; torch carries fp32 state.  exp_avg_sq (a sum of positive terms) agrees to a
    few fp32 ulps of its own magnitude after 10 steps.  exp_avg mixes signs and may cancel, so its error is held against the
    largest gradient of the element: two roundings per step, each at most half an ulp of a value no larger than that.  A
    parameter may sit near zero while its updates are of the size of lr: its error is held against |p| + lr, one ulp of that
    per step for the subtraction and the quotient together."""
    p0, grads = _lists()
    params = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.Adam(params, lr=1e-3, foreach=False)
    P, M, V = [x.numpy() for x in p0], [np.zeros(x.numel(), np.float32) for x in p0], [np.zeros(x.numel(), np.float32) for x in p0]
    c = OO.Counters()
    for k in range(10):
        for q, g in zip(params, grads[k]):
            q.grad = g.clone()
        opt.step()
        P, M, V, _, c, info = OO.step(P, [g.numpy() for g in grads[k]], M, V, None, c, lr=1e-3, do_ema=False)
        assert not info["skip"]
    assert c.adam_step == 10 and c.applied == 10
    for i, (q, want, m, v) in enumerate(zip(params, P, M, V)):
        st = opt.state[q]
        assert np.all(np.abs(q.detach().numpy() - want) <= 10 * 2.0 ** -23 * (np.abs(want) + 1e-3))
        gmax = np.max(np.abs(np.stack([grads[k][i].numpy() for k in range(10)])), axis=0).astype(np.float64)
        assert np.all(np.abs(st["exp_avg"].numpy() - m) <= 10 * 2 * 2.0 ** -24 * gmax)
        assert OO.ulp_distance(st["exp_avg_sq"].numpy(), v) <= 16


def test_oracle_skip_rule_and_counters():
    p, grads = _lists(1, (5,))
    z = [np.zeros(5, np.float32)]
    g = grads[0][0].numpy().copy()
    c = OO.Counters()
    g_nan = g.copy()
    g_nan[3] = np.nan
    P, M, V, E, c1, info = OO.step([p[0].numpy()], [g_nan], z, z, [p[0].numpy()], c)
    assert info["skip"] and c1.as_tuple() == (0, 0, 0, 0, 1) and np.array_equal(P[0], p[0].numpy().astype(np.float64))
    g_inf = g.copy()
    g_inf[0] = np.inf
    assert not OO.step([p[0].numpy()], [g_inf], z, z, None, c)[5]["skip"]
    assert OO.step([p[0].numpy()], [g_inf], z, z, None, c, skip_on="nonfinite")[5]["skip"]
    assert OO.step([p[0].numpy()], [g], z, z, None, c, losses=(0.5, float("nan")))[5]["skip"]
    assert OO.step([p[0].numpy()], [g], z, z, None, c, found_inf=1.0)[5]["skip"]
    assert OO.step([p[0].numpy()], [g], z, z, None, c)[4].as_tuple() == (1, 0, 0, 1, 0)


def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(egoego_optim_\w+)\s*\(", code))
    bound = {n for n in _lib.EXPORTS if n.startswith("egoego_optim_")}
    assert declared == bound and len(bound) == 8
    assert not any(n.startswith("egoego_train_") for n in bound)
    assert len({n for n in _lib.EXPORTS if n.startswith("egoego_train_")}) == 9  # the training step's nine stay nine
    assert callable(_lib.check_optim)
    assert re.search(r"#define EGOEGO_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    assert text.index("egoego_optim_ctx egoego_optim_ctx;") > text.index("int egoego_train_saved(")  # new structs behind everything
    src = open(os.path.join(CSRC, "optim_step.h")).read()
    assert f"CHUNK = {_lib.OPTIM_CHUNK};" in src and f"#define EGOEGO_OPTIM_CHUNK {_lib.OPTIM_CHUNK}\n" in text
    assert f"#define EGOEGO_OPTIM_MAX_LOSSES {_lib.OPTIM_MAX_LOSSES}\n" in text
    enums = {k: int(v) for k, v in re.findall(r"\b(EGOEGO_OPTIM_[A-Z0-9_]+)\s*=\s*(\d+)", code)}
    assert enums["EGOEGO_OPTIM_SKIP_NAN"] == _lib.OPTIM_SKIP["nan"] and enums["EGOEGO_OPTIM_SKIP_NONFINITE"] == _lib.OPTIM_SKIP["nonfinite"]
    assert (enums["EGOEGO_OPTIM_EMA_NONE"], enums["EGOEGO_OPTIM_EMA_COPY"], enums["EGOEGO_OPTIM_EMA_LERP"]) == (
        _lib.OPTIM_EMA_NONE, _lib.OPTIM_EMA_COPY, _lib.OPTIM_EMA_LERP)
    from egoego_release_amd import build
    assert "optim_step.hip" in build.SOURCES
    host = open(os.path.join(CSRC, "optim_step.hip")).read()
    assert '#include "host_util.h"' in host
    for banned in ("hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomicAdd", "hipMemcpyHostToDevice", "hipMemcpyDeviceToHost"):
        assert banned not in host and banned not in src, banned
    # the state header: the ctypes mirror has the header's fields in the header's order
    body = code[code.index("typedef struct {", code.index("egoego_optim_ctx egoego_optim_ctx;")):code.index("} egoego_optim_state;")]
    assert re.findall(r"(?:int64_t|int32_t|double|float)\s+(\w+);", body) == [n for n, _ in _lib.OptimState._fields_]


def test_state_dicts_go_both_ways():
    """FusedAdam -> torch.optim.Adam -> FusedAdam: the same keys, and both continue with the same arithmetic (the plain path)."""
    p0, grads = _lists(2, (7, 33))
    a = [torch.nn.Parameter(x.clone()) for x in p0]
    b = [torch.nn.Parameter(x.clone()) for x in p0]
    fa = optim.FusedAdam(a, lr=1e-3, fused=False)
    ta = torch.optim.Adam(b, lr=1e-3, foreach=False)
    for k in range(3):
        for q, g in zip(a, grads[k]):
            q.grad = g.clone()
        fa.step()
    sd = fa.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert isinstance(sd["state"][0]["step"], torch.Tensor) and float(sd["state"][0]["step"]) == 3.0
    assert sorted(sd["param_groups"][0]) == sorted(ta.state_dict()["param_groups"][0])
    for q, r in zip(a, b):
        r.data.copy_(q.data)
    ta.load_state_dict(copy.deepcopy(sd))  # (load_state_dict keeps a tensor that needs no cast: without the copy both would share moments)
    for q, r, g in zip(a, b, grads[3]):
        q.grad, r.grad = g.clone(), g.clone()
    fa.step()
    ta.step()
    for q, r in zip(a, b):
        assert torch.equal(q, r)
    fb = optim.FusedAdam([torch.nn.Parameter(x.detach().clone()) for x in b], lr=5.0, fused=False)
    fb.load_state_dict(ta.state_dict())
    assert fb.param_groups[0]["lr"] == 1e-3 and fb.counters()["adam_step"] == 4
    # a fused optimizer takes the same dict without a GPU: the counter goes to the device with the first step
    fc = optim.FusedAdam([torch.nn.Parameter(x.detach().clone()) for x in b], fused=True)
    fc.load_state_dict(ta.state_dict())
    assert {int(s["step"]) for s in fc.state.values()} == {4}
    with pytest.raises(_lib.EgoEgoHipError):
        for q in fc.param_groups[0]["params"]:
            q.grad = torch.zeros_like(q)
        fc.step()


def test_fused_adam_refuses_what_it_does_not_serve():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        optim.FusedAdam(p, amsgrad=True)
    with pytest.raises(ValueError):
        optim.FusedAdam(p, skip_on="never")
    with pytest.raises(ValueError):
        optim.FusedAdam([{"params": p}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(RuntimeError):
        optim.FusedAdam(p, fused=False).step()  # no gradient yet
    assert optim.FusedAdam(p)._step_supports_amp_scaling is True
    assert list(inspect.signature(optim.FusedAdam.step).parameters)[1:] == ["closure", "ema", "losses"]


def test_apply_kernel_on_the_host_under_sanitizers(tmp_path):
    """csrc/optim_step.h compiled by the host compiler over tests/host_sim's stand-in for the HIP header, and apply_kernel run
    thread after thread by a stand-alone program (tests/host_sim/apply_main.cpp) under AddressSanitizer and UBSan's alignment
    check.  The device takes a 16-byte access off its boundary without a word and computes the same values, so a wrong scalar
    head — (4 - phase) & 1, say — passes every comparison there; here it stops the program, and so does an access over either
    end of a view.  Every 16-byte phase, every single tensor off the others' phase, counts below the head and over two chunks;
    every element visited exactly once under a grid smaller than the chunk count."""
    sim = os.path.join(ROOT, "tests", "host_sim")
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "apply_sim")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=on", "-fsanitize=address,alignment", "-fno-sanitize-recover=all", "-I", sim, "-I", CSRC,
           os.path.join(sim, "apply_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and "24 cases, 0 wrong elements" in run.stdout, run.stdout + run.stderr


# ---------------------------------------------------------------------------------------------------------------- the EMA schedule
def test_ema_schedule_at_its_regime_changes():
    """update_every = 10, update_after_step = 100 (the reference's): the counter values 0, 1, 10; 100 and the first multiple after
    it; and the step at which the decay reaches beta."""
    kw = dict(update_every=10, update_after_step=100)
    assert optim.ema_action(0, False, **kw) == "copy"
    assert optim.ema_action(1, False, **kw) == "none"
    assert optim.ema_action(10, False, **kw) == "copy"
    assert optim.ema_action(100, False, **kw) == "copy"          # step <= update_after_step still copies
    assert optim.ema_action(110, False, **kw) == "copy"          # the first later one copies and sets initted
    assert optim.ema_action(110, True, **kw) == "lerp"
    assert optim.ema_action(115, True, **kw) == "none"
    for f in (optim.ema_decay, OO.decay_at):
        assert f(101, 0.995, 100) == 0.0                          # e = 0
        assert f(102, 0.995, 100) == pytest.approx(1 - 2 ** (-2 / 3))
        assert f(111, 0.995, 100) == pytest.approx(1 - 11 ** (-2 / 3))
        # decay = beta where (1 + e)^(-2/3) <= 0.005: e >= 0.005^-1.5 - 1 = 2827.4...
        assert f(100 + 1 + 2827, 0.995, 100) < 0.995 and f(100 + 1 + 2828, 0.995, 100) == 0.995
        assert f(10 ** 7, 0.995, 100) == 0.995
        assert f(111, 0.995, 100, min_value=0.9) == 0.9


def _tiny(T=11, seed=0):
    cfg = ModelConfig(n_dec_layers=1, max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type="l1")
    m.load_state_dict(make_weights(cfg, seed), strict=False)
    m.train()
    return cfg, m


def _batches(T=11, B=2, n=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [{"motion": torch.randn(B, T, 198, generator=g) * 0.5, "seq_len": torch.tensor([T, T - 3])} for _ in range(n)]


def test_ema_module_plain_path_follows_the_schedule():
    cfg, m = _tiny()
    ema = optim.EMA(m, beta=0.995, update_every=3, update_after_step=4, fused=False)
    keys = set(ema.state_dict())
    assert {"initted", "step"} <= keys and any(k.startswith("ema_model.") for k in keys) and any(k.startswith("online_model.") for k in keys)
    assert not any(p.requires_grad for p in ema.ema_model.parameters())
    w = m.denoise_fn.linear_out.bias
    e = ema.ema_model.denoise_fn.linear_out.bias
    c = OO.Counters()
    E = e.detach().numpy().astype(np.float64)
    for k in range(12):
        with torch.no_grad():
            w.add_(0.01 * (k + 1))
        before = e.detach().clone()
        ema.update()
        act = OO.ema_action(k, c.initted, 3, 4)
        if act == "none":
            assert torch.equal(e, before)
        elif act == "copy":
            assert torch.equal(e, w)
            c.initted = c.initted or k > 4
            E = w.detach().numpy().astype(np.float64)
        else:
            d = OO.decay_at(k + 1, 0.995, 4)
            E = E - (E - w.detach().numpy().astype(np.float64)) * (1 - d)
            np.testing.assert_allclose(e.numpy(), E, rtol=1e-6)
    assert int(ema.step) == 12 and float(ema.initted) == 1.0
    assert [OO.ema_action(k, k > 6, 3, 4) for k in (0, 3, 6, 9)] == ["copy", "copy", "copy", "lerp"]


# ---------------------------------------------------------------------------------------------------------------- the trainer, plain
def _snapshot(tr):
    return ({k: v.clone() for k, v in tr.model.state_dict().items()}, {k: v.clone() for k, v in tr.ema.state_dict().items()},
            {i: {k: v.clone() for k, v in st.items()} for i, st in tr.optimizer.state_dict()["state"].items()}, tr.step)


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_trainer_nan_loss_changes_nothing(tmp_path):
    cfg, m = _tiny()
    tr = Stage2Trainer(m, _batches(), fused=False, results_folder=str(tmp_path), ema_update_every=1)
    torch.manual_seed(0)
    assert tr.train(2) == 2
    before = _snapshot(tr)
    tr.inject_loss = lambda idx, i, loss: loss * float("nan") if i == 1 else loss
    assert tr.train(1) == 2
    after = _snapshot(tr)
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and before[3] == after[3] == 2
    assert all(_same(before[2][i], after[2][i]) for i in before[2])
    assert tr.optimizer.counters()["skipped"] == 1 and int(tr.optimizer.last_skipped) == 1
    tr.inject_loss = None
    assert tr.train(1) == 3


def test_trainer_refuses_a_save_cadence_its_checks_cannot_keep(tmp_path):
    """fused=True reads the step count every host_check iterations and writes one checkpoint per check: milestones closer together
    than the checks would be lost, so the constructor (which launches nothing) raises.  The plain path checks every iteration."""
    cfg, m = _tiny()
    kw = dict(results_folder=str(tmp_path))
    with pytest.raises(ValueError, match="save_and_sample_every.*host_check"):
        Stage2Trainer(m, _batches(), fused=True, host_check=5, save_and_sample_every=3, **kw)
    with pytest.raises(ValueError, match="milestones"):
        Stage2Trainer(m, _batches(), fused=True, host_check=4, save_and_sample_every=3, **kw)
    assert Stage2Trainer(m, _batches(), fused=True, host_check=3, save_and_sample_every=3, **kw).host_check == 3
    assert Stage2Trainer(m, _batches(), fused=True, host_check=1, save_and_sample_every=1, **kw).host_check == 1
    assert Stage2Trainer(m, _batches(), fused=False, host_check=5, save_and_sample_every=3, **kw).host_check == 1
    assert "save_and_sample_every must be at least host_check" in " ".join(Stage2Trainer.__doc__.split())


def test_two_micro_batches_equal_one_step_on_the_summed_gradient(tmp_path):
    cfg, m = _tiny()
    cfg2, m2 = _tiny()
    batches = _batches()
    tr = Stage2Trainer(m, batches, fused=False, results_folder=str(tmp_path), gradient_accumulate_every=2)
    torch.manual_seed(3)
    tr.train(1)
    # by hand: the same draws, the two losses halved and summed, one torch.optim.Adam step
    opt = torch.optim.Adam(m2.parameters(), lr=1e-4, foreach=False)
    torch.manual_seed(3)
    for b in batches[:2]:
        pm = tr.prep_padding_mask(b["motion"], b["seq_len"])
        (m2(b["motion"], tr.prep_head_condition_mask(b["motion"]), padding_mask=pm) / 2).backward()
    opt.step()
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_checkpoint_layout_and_round_trip(tmp_path):
    from egoego_release_amd.harness import load_stage2_checkpoint
    cfg, m = _tiny()
    tr = Stage2Trainer(m, _batches(), fused=False, results_folder=str(tmp_path), ema_update_every=2, save_and_sample_every=3,
                       ema_kwargs=dict(update_after_step=0))
    torch.manual_seed(1)
    tr.train(5)  # the reference's cadence: the save happens in the iteration that STARTS at step 3, after its update
    path = tmp_path / "model-1.pt"
    assert path.exists() and not (tmp_path / "model-2.pt").exists()
    data = torch.load(path, map_location="cpu")
    assert sorted(data) == ["ema", "model", "scaler", "step"] and data["step"] == 3
    assert {"initted", "step"} <= set(data["ema"]) and int(data["ema"]["step"]) == 4
    k = "denoise_fn.linear_out.bias"
    assert not torch.equal(data["ema"]["ema_model." + k], data["model"][k])  # a real EMA entry, not a copy of the online weights
    _, fresh = _tiny(seed=9)
    got, info = load_stage2_checkpoint(str(path), model=fresh, use_ema=True)
    assert torch.equal(got.state_dict()[k], data["ema"]["ema_model." + k]) and info["step"] == 3 and not info["missing"]
    got, _ = load_stage2_checkpoint(str(path), model=fresh, use_ema=False)
    assert torch.equal(got.state_dict()[k], data["model"][k])
    # load(): step, both models and the scaler
    _, other = _tiny(seed=7)
    tr2 = Stage2Trainer(other, _batches(), fused=False, results_folder=str(tmp_path), save_optimizer=True)
    tr2.load(1)
    assert tr2.step == 3 and int(tr2.ema.step) == 4
    assert _same(dict(tr2.model.state_dict()), data["model"]) and _same(dict(tr2.ema.state_dict()), data["ema"])
    assert tr2.scaler.state_dict() == data["scaler"]
    tr2.save(7)
    assert sorted(torch.load(tmp_path / "model-7.pt", map_location="cpu")) == ["ema", "model", "optimizer", "scaler", "step"]


def test_tools_have_their_switches():
    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    mtl = load("make_trained_like_checkpoint")
    sig = inspect.signature(mtl.train_like).parameters
    assert sig["fused"].default is False and sig["hip"].default is False
    ts = load("train_stage2")
    args = ts.parser().parse_args(["--windows", "w.p", "--stats", "s.p"])
    assert args.window == 120 and args.batch_size == 32 and args.learning_rate == 1e-4 and not args.hip_loss and not args.plain_update
    assert callable(load("optim_step_bench").main)
