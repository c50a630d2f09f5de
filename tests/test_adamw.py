"""Host side of the fused clip + AdamW update: the fp64 oracle of tests/adamw_oracle.py pinned to clip_grad_norm_ +
torch.optim.AdamW, FusedAdamW's plain path, the state dicts it exchanges with torch.optim.AdamW, StepLR, the binding, and the
stage-1 trainer's default."""
import copy
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import adamw_oracle as AO
from egoego_release_amd import _lib, optim, stage1, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-3, 1e-2


def _lists(seed=0, sizes=(1, 3, 198, 700), steps=25):
    g = torch.Generator().manual_seed(seed)
    p = [torch.randn(n, generator=g) * 0.05 + 0.1 for n in sizes]  # away from zero: the bar on p counts in units of |p| + lr
    grads = [[torch.randn(n, generator=g) * 10.0 ** (-6 * torch.rand(n, generator=g)) for n in sizes] for _ in range(steps)]
    return p, grads


def _torch_clip_adamw(params, opt, grads, max_norm):
    for q, g in zip(params, grads):
        q.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False, foreach=False)
    opt.step()
    return norm


def test_oracle_matches_torch_clip_and_adamw_over_25_steps():
    """The oracle carries fp64 state from fp32 gradients, torch fp32 state; only torch's own distances are taken here.  Per step
    the clipped gradient has two fp32 roundings (optim_oracle's has none), exp_avg's lerp two more, the decay p * wmul one beside
    the subtraction and the quotient.  So, after 25 steps: exp_avg within 25 * 4 half-ulps of the element's largest gradient;
    p within 25 * 1.5 ulps of |p| + lr.  exp_avg_sq is a sum of positive terms: each step adds at most one ulp of its own (the
    products b2 v and the fused sum) to what it inherits, and a new term g^2 comes with at most 2.5 ulp (g twice rounded, squared;
    w2 g rounded), weighted below 1: under 25 + 2.5 relative units of 2^-24, that is under 55 ulp; 64 allowed.  The norms agree to
    fp32 rounding of a sum of n terms."""
    p0, grads = _lists()
    n = sum(x.numel() for x in p0)
    params = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, foreach=False)
    P, M, V = [x.numpy() for x in p0], [np.zeros(x.numel(), np.float32) for x in p0], [np.zeros(x.numel(), np.float32) for x in p0]
    c = AO.Counters()
    clipped = 0
    for k in range(25):
        norm = _torch_clip_adamw(params, opt, grads[k], 1.0)
        P, M, V, c, info = AO.step(P, [g.numpy() for g in grads[k]], M, V, c, lr=LR, weight_decay=WD, max_norm=1.0)
        assert not info["skip"] and float(norm) == pytest.approx(info["norm"], rel=n * 2.0 ** -24)
        clipped += info["coef"] < 1.0
    assert c.adam_step == 25 and c.applied == 25 and clipped == 25
    for i, (q, want, m, v) in enumerate(zip(params, P, M, V)):
        st = opt.state[q]
        assert np.all(np.abs(q.detach().numpy() - want) <= 25 * 1.5 * 2.0 ** -23 * (np.abs(want) + LR))
        gmax = np.max(np.abs(np.stack([grads[k][i].numpy() for k in range(25)])), axis=0).astype(np.float64)
        assert np.all(np.abs(st["exp_avg"].numpy() - m) <= 25 * 4 * 2.0 ** -24 * gmax)
        d = AO.ulp_distance(st["exp_avg_sq"].numpy(), v)
        print(f"tensor {i}: exp_avg_sq d_torch {d:.2f}")
        assert d <= 64


def test_oracle_coefficient_is_clip_grad_norms():
    """A lone gradient of 1.0 at max_norm = 1.  The oracle's coefficient is 1 / 1.000001 in fp64, which rounds to the fp32 value
    1 - 17 * 2^-24 = 0.99999899.  torch forms it in fp32 throughout: 1 + 1e-6 rounds to 1 + 8 * 2^-23, whose reciprocal is
    1 - 16 * 2^-24 = 0.99999905, one ulp above.  Below max_norm the coefficient is exactly 1; a zero norm gives 1 / 1e-6, clamped
    to 1."""
    q = torch.nn.Parameter(torch.zeros(1))
    q.grad = torch.ones(1)
    torch.nn.utils.clip_grad_norm_([q], 1.0, foreach=False)
    ours = np.float32(AO.clip_coef(1.0, 1.0))
    assert ours == np.float32(1 / 1.000001) == np.float32(1 - 17 * 2.0 ** -24) and q.grad.numpy()[0] == np.float32(1 - 16 * 2.0 ** -24)
    assert abs(float(ours) - float(q.grad)) <= 2.0 ** -24 and float(q.grad) < 1.0
    assert AO.clip_coef(0.03, 1.0) == 1.0 and AO.clip_coef(0.0, 1.0) == 1.0 and AO.clip_coef(27.0, None) == 1.0
    assert AO.clip_coef(27.0, 1.0) == 1.0 / (27.0 + 1e-6)
    # one step on 16 k elements: exp_avg_sq to a few ulps (three roundings of g^2's share; nothing inherited)
    g = torch.Generator().manual_seed(5)
    p0, g0 = torch.randn(16384, generator=g) * 0.05, torch.randn(16384, generator=g)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=LR, weight_decay=WD, foreach=False)
    _torch_clip_adamw([q], opt, [g0], 1.0)
    z = np.zeros(16384, np.float32)
    P, M, V, _, info = AO.step([p0.numpy()], [g0.numpy()], [z], [z], AO.Counters(), lr=LR, weight_decay=WD, max_norm=1.0)
    assert info["coef"] < 0.01 and AO.ulp_distance(opt.state[q]["exp_avg_sq"].numpy(), V[0]) <= 8


def test_l2_form_without_clipping_is_optim_oracles_step():
    import optim_oracle as OO
    p0, grads = _lists(3, (5, 40), 1)
    z = [np.zeros(x.numel(), np.float32) for x in p0]
    a = AO.step([x.numpy() for x in p0], [g.numpy() for g in grads[0]], z, z, AO.Counters(), lr=LR, weight_decay=WD, decoupled=False)
    b = OO.step([x.numpy() for x in p0], [g.numpy() for g in grads[0]], z, z, None, OO.Counters(), lr=LR, weight_decay=WD, do_ema=False)
    for x, y in zip(a[:3], b[:3]):
        assert all(np.array_equal(s, t) for s, t in zip(x, y))
    assert a[3].as_tuple() == b[4].as_tuple()


def test_plain_path_is_clip_grad_norm_and_torch_adamw_bit_for_bit():
    p0, grads = _lists(1, steps=5)
    a = [torch.nn.Parameter(x.clone()) for x in p0]
    b = [torch.nn.Parameter(x.clone()) for x in p0]
    fa = optim.FusedAdamW(a, lr=LR, max_grad_norm=1.0, fused=False)
    tb = torch.optim.AdamW(b, lr=LR, foreach=False)
    assert fa.param_groups[0]["weight_decay"] == tb.param_groups[0]["weight_decay"] == 1e-2
    for k in range(5):
        for q, g in zip(a, grads[k]):
            q.grad = g.clone()
        fa.step()
        norm = _torch_clip_adamw(b, tb, grads[k], 1.0)
        assert torch.equal(fa.last_grad_norm, norm) and int(fa.last_skipped) == 0  # the norm BEFORE clipping
        assert float(fa.last_clip_coef) == pytest.approx(1.0 / (float(norm) + 1e-6), rel=1e-6)
        for q, r in zip(a, b):
            assert torch.equal(q, r) and torch.equal(q.grad, r.grad)  # the plain path clips in place, as torch does
    for q, r in zip(a, b):
        assert torch.equal(fa.state[q]["exp_avg"], tb.state[r]["exp_avg"]) and torch.equal(fa.state[q]["exp_avg_sq"], tb.state[r]["exp_avg_sq"])
    assert fa.counters()["adam_step"] == 5
    # the skip rule of the plain path: a NaN gradient changes nothing, and is not spread by the clip
    before = [q.detach().clone() for q in a]
    for q, g in zip(a, grads[0]):
        q.grad = g.clone()
    a[2].grad[7] = float("nan")
    fa.step()
    assert int(fa.last_skipped) == 1 and all(torch.equal(q, x) for q, x in zip(a, before)) and fa.counters()["skipped"] == 1
    assert torch.equal(a[3].grad, grads[0][3]) and int(torch.isnan(a[2].grad).sum()) == 1


def test_state_dicts_go_both_ways_with_torch_adamw():
    p0, grads = _lists(2, (7, 33), 5)
    a = [torch.nn.Parameter(x.clone()) for x in p0]
    b = [torch.nn.Parameter(x.clone()) for x in p0]
    fa = optim.FusedAdamW(a, lr=LR, max_grad_norm=1.0, fused=False)
    tb = torch.optim.AdamW(b, lr=5.0, foreach=False)
    for k in range(3):
        for q, g in zip(a, grads[k]):
            q.grad = g.clone()
        fa.step()
    sd = fa.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert float(sd["state"][0]["step"]) == 3.0
    assert sorted(sd["param_groups"][0]) == sorted(tb.state_dict()["param_groups"][0])
    for q, r in zip(a, b):
        r.data.copy_(q.data)
    tb.load_state_dict(copy.deepcopy(sd))
    assert tb.param_groups[0]["lr"] == LR
    for q, g in zip(a, grads[3]):
        q.grad = g.clone()
    fa.step()
    _torch_clip_adamw(b, tb, grads[3], 1.0)
    assert all(torch.equal(q, r) for q, r in zip(a, b))
    fb = optim.FusedAdamW([torch.nn.Parameter(x.detach().clone()) for x in b], lr=5.0, max_grad_norm=1.0, fused=False)
    fb.load_state_dict(copy.deepcopy(tb.state_dict()))
    assert fb.param_groups[0]["lr"] == LR and fb.counters()["adam_step"] == 4
    for q, g in zip(fb.param_groups[0]["params"], grads[4]):
        q.grad = g.clone()
    fb.step()
    _torch_clip_adamw(b, tb, grads[4], 1.0)
    assert all(torch.equal(q, r) for q, r in zip(fb.param_groups[0]["params"], b))
    # a fused one takes the same dict without a GPU: the counter goes to the device with the first step, which needs one
    fc = optim.FusedAdamW([torch.nn.Parameter(x.detach().clone()) for x in b], max_grad_norm=1.0)
    fc.load_state_dict(copy.deepcopy(tb.state_dict()))
    assert {int(s["step"]) for s in fc.state.values()} == {5}
    with pytest.raises(_lib.EgoEgoHipError):
        for q in fc.param_groups[0]["params"]:
            q.grad = torch.zeros_like(q)
        fc.step()


def test_step_lr_sets_the_lr_of_the_next_step():
    p0, grads = _lists(4, (9,), 4)
    a, b = [torch.nn.Parameter(p0[0].clone())], [torch.nn.Parameter(p0[0].clone())]
    fa = optim.FusedAdamW(a, lr=LR, max_grad_norm=1.0, fused=False)
    tb = torch.optim.AdamW(b, lr=LR, foreach=False)
    sa = torch.optim.lr_scheduler.StepLR(fa, step_size=2, gamma=0.3)
    sb = torch.optim.lr_scheduler.StepLR(tb, step_size=2, gamma=0.3)
    seen = []
    for k in range(4):
        a[0].grad = grads[k][0].clone()
        seen.append(fa.param_groups[0]["lr"])
        fa.step()
        _torch_clip_adamw(b, tb, grads[k], 1.0)
        sa.step()
        sb.step()
        assert torch.equal(a[0], b[0]), k
    assert seen == pytest.approx([LR, LR, 0.3 * LR, 0.3 * LR]) and fa.param_groups[0]["lr"] == pytest.approx(0.09 * LR)


def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "egoego_optimw_step" in _lib.EXPORTS and re.search(r"\bint egoego_optimw_step\s*\(", code)
    assert hasattr(_lib.load(), "egoego_optimw_step")
    assert re.search(r"#define EGOEGO_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    fields = lambda body: [n for decl in re.findall(r"(?:int64_t|int32_t|double|float|int)\s+([\w\s,]+);", body)  # noqa: E731
                           for n in re.split(r"\s*,\s*", decl.strip())]
    body = code[code.rindex("typedef struct {", 0, code.index("} egoego_optim_hyper_w;")):code.index("} egoego_optim_hyper_w;")]
    assert fields(body) == [n for n, _ in _lib.OptimHyperW._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay", "decoupled",
                                                                        "max_norm", "clip_eps"]
    import ctypes as C
    assert C.sizeof(_lib.OptimHyperW) == 64 and _lib.OptimHyperW.max_norm.offset == 48
    body = code[code.rindex("typedef struct {", 0, code.index("} egoego_optim_state;")):code.index("} egoego_optim_state;")]
    names = [n for n, _ in _lib.OptimState._fields_]
    assert fields(body) == names and names[-2:] == ["ema_action", "clip_coef"]  # appended: no earlier field moved
    assert _lib.OptimState.ema_action.offset == 52 and _lib.OptimState.clip_coef.offset == 56 and C.sizeof(_lib.OptimState) <= 256
    # the old entry point is a call into the new one, and the kernels gained no launch, atomic or read-back
    host = open(os.path.join(ROOT, "egoego_release_amd", "csrc", "optim_step.hip")).read()
    old = host[host.index("int egoego_optim_step(egoego_optim_ctx*"):host.index("int egoego_optim_read_state(")]
    assert "return egoego_optimw_step(" in old and "hipLaunchKernelGGL" not in old
    assert host.count("hipLaunchKernelGGL") == 7  # table, chunks; norm, decide, three forms of apply


def test_constructors_refuse_what_they_do_not_serve():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(skip_on="never"), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0),
                dict(max_grad_norm=float("nan")), dict(max_grad_norm=float("inf")), dict(weight_decay=-0.1), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            optim.FusedAdamW(p, **bad)
    with pytest.raises(ValueError):
        optim.FusedAdam(p, max_grad_norm=0.0)
    with pytest.raises(ValueError, match="FusedAdamW takes one param group"):
        optim.FusedAdamW([{"params": p}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(RuntimeError):
        optim.FusedAdamW(p, fused=False).step()  # no gradient yet
    o = optim.FusedAdamW(p)
    assert o.defaults["weight_decay"] == 1e-2 and o.max_grad_norm is None and o._step_supports_amp_scaling is True
    assert optim.FusedAdam(p).max_grad_norm is None and optim.FusedAdam(p).defaults["weight_decay"] == 0


def _opt(window=8, layers=1):
    return Namespace(window=window, n_dec_layers=layers, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True,
                     w_rotation=1.0, w_va=1.0, w_dist=1.0, dist_scale=10.0)


def test_stage1_trainer_keeps_torch_adamw_by_default():
    m = stage1.HeadFormer(_opt(), torch.device("cpu"))
    tr = trainer.Stage1Trainer(m, [])
    assert type(tr.optimizer) is torch.optim.AdamW and tr.fused_update is False
    tf = trainer.Stage1Trainer(stage1.HeadNormalFormer(_opt(), torch.device("cpu")), [], fused_update=True, max_grad_norm=0.5, lr=3e-4)
    o = tf.optimizer
    assert type(o) is optim.FusedAdamW and o.hip and o.max_grad_norm == 0.5 and o.zero_grads and o.skip_on == "nonfinite"
    assert o.modules == (tf.model,) and o.param_groups[0]["lr"] == 3e-4 and o.param_groups[0]["weight_decay"] == 1e-2
    assert tf.scheduler.optimizer is o and tf.scheduler.step_size == 2000
    # the hook a pointer-writing optimizer calls: the packed copy of the inference engine is declared stale
    m._packed = ("anything",)
    m.invalidate_engine()
    assert m._packed is None
    assert "optim.FusedAdam has neither" not in trainer.Stage1Trainer.__doc__ and "fused_update=True" in trainer.Stage1Trainer.__doc__


def test_the_training_tool_has_its_switch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_stage1_tool", os.path.join(ROOT, "tools", "train_stage1.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse_opt([]).fused_update is False and tool.parse_opt(["--fused_update"]).fused_update is True
