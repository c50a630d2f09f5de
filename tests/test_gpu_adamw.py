"""The fused clip + AdamW update on the GPU (egoego_optimw_step, optim.FusedAdamW, Stage1Trainer(fused_update=True)) against the
fp64 oracle of tests/adamw_oracle.py, on the tensor lists, guards and rig of tests/test_gpu_optim.py.

The bar is that file's: for each of p, exp_avg and exp_avg_sq, d = the largest distance from the oracle in units of the oracle
value's fp32 ulp, d99 the 99th percentile over all elements of the kind; d_torch and d99_torch the same figures for
clip_grad_norm_(foreach=False) + torch.optim.AdamW(foreach=False) on the CPU from the same fp32 inputs; d_hip <= 2 d_torch + 1 and
d99_hip <= 2 d99_torch + 1.

EGOEGO_ADAMW_RECORD=<file>: the measured values are written there as JSON (profiles/adamw_error.json is such a file).
"""
import importlib.util
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import adamw_oracle as AO
import stream_cases as SC
import test_gpu_optim as TG
from egoego_release_amd import _lib, optim, stage1
from egoego_release_amd.synthetic import make_stage1_train_batch
from egoego_release_amd.trainer import Stage1Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = _lib.OPTIM_CHUNK
SPECS, PHASE_SPECS, ZERO = TG.SPECS, TG.PHASE_SPECS, TG.ZERO
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)  # lr, betas, eps, weight_decay (decoupled unless a test says otherwise)
KINDS = ("p", "exp_avg", "exp_avg_sq")
_RECORD = {}
_bits, _same_bits = TG._bits, TG._same_bits


def _record(case, **kw):
    path = os.environ.get("EGOEGO_ADAMW_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _hold(case, got, tor, want):
    d_hip, d_torch, q_hip, q_torch = TG._distances(got, want), TG._distances(tor, want), TG._d99(got, want), TG._d99(tor, want)
    for name, h, t, qh, qt in zip(KINDS, d_hip, d_torch, q_hip, q_torch):
        print(f"{case}: {name}: d_hip {h:.3f}  d_torch {t:.3f}  d99_hip {qh:.3f}  d99_torch {qt:.3f}")
    _record(case, d_hip=dict(zip(KINDS, d_hip)), d_torch=dict(zip(KINDS, d_torch)), d99_hip=dict(zip(KINDS, q_hip)), d99_torch=dict(zip(KINDS, q_torch)))
    for name, h, t, qh, qt in zip(KINDS, d_hip, d_torch, q_hip, q_torch):
        assert h <= 2 * t + 1, (case, name, h, t)
        assert qh <= 2 * qt + 1, (case, name, "d99", qh, qt)


def _torch_step(p, g, m, v, adam_step, hyper=HYPER, max_norm=1.0, decoupled=True):
    """clip_grad_norm_(foreach=False) + torch.optim.AdamW / Adam (foreach=False) on the CPU from fp32 lists -> (p, m, v, norm)."""
    params = [torch.nn.Parameter(x.clone()) for x in p]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(params, lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4], foreach=False)
    for q, gg, mm, vv in zip(params, g, m, v):
        q.grad = gg.clone()
        opt.state[q] = {"step": torch.tensor(float(adam_step)), "exp_avg": mm.clone(), "exp_avg_sq": vv.clone()}
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False, foreach=False)
    opt.step()
    return [q.detach() for q in params], [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params], norm


def _oracle(r, lists=None, hyper=HYPER, max_norm=1.0, decoupled=True, **kw):
    p, g, m, v = (lists if lists is not None else r.ref)[:4]
    return AO.step([x.numpy() for x in p], [x.numpy() for x in g], [x.numpy() for x in m], [x.numpy() for x in v],
                   AO.Counters(adam_step=r.cpu[5]), lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4], max_norm=max_norm,
                   decoupled=decoupled, **kw)


def _out(r):
    return (r.whole[0], r.whole[2], r.whole[3])


def _ulps32(a, b):
    """The distance of two fp32 values of one sign in units in the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.fixture(scope="module")
def rig():
    return TG.Rig(hyper=HYPER)


def _scaled(r, factor):
    """The rig's gradients times a power of two, on both sides -> the CPU lists the device now holds."""
    lists = [list(x) for x in r.ref]
    lists[1] = [x * factor for x in lists[1]]
    for d, s in zip(r.whole[1], lists[1]):
        d.copy_(s)
    return lists


def test_one_clipped_step_against_the_oracle_at_the_kernel_edges(rig):
    """SPECS' counts and offsets; the gradients as the rig draws them: a norm of about 27 at max_norm = 1.  clip_coef within one
    ulp of float32(min(1, 1 / (norm + 1e-6))), total_norm to 1e-12, the bar on p and both moments, the zero tensor's moments
    exactly 0, the gradients' bits kept (zero_grads off: nothing is clipped in place), the guards."""
    rig.restore()
    rig.step(ema=False, decoupled=True, max_norm=1.0)
    P, M, V, c1, info = _oracle(rig)
    st = rig.eng.read_state()
    assert 20.0 < info["norm"] < 35.0 and info["coef"] < 0.05 and not info["skip"]
    assert abs(st["total_norm"] - info["norm"]) <= 1e-12 * info["norm"]
    assert _ulps32(st["clip_coef"], np.float32(min(1.0, 1.0 / (info["norm"] + 1e-6)))) <= 1
    assert float(rig.eng.last_clip_coef) == st["clip_coef"] and float(rig.eng.last_grad_norm) == np.float32(st["total_norm"])
    assert (st["adam_step"], st["applied"], st["skipped"], st["last_skip"]) == (c1.adam_step, 1, 0, 0)
    tor = _torch_step(*rig.cpu[:4], rig.cpu[5])
    assert float(tor[3]) == pytest.approx(info["norm"], rel=1e-5)
    _hold("one_step_clipped", _out(rig), tor[:3], (P, M, V))
    assert not rig.m[ZERO].any() and not rig.v[ZERO].any()
    assert all(torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)) for a, b in zip(rig.g, rig.cpu[1]))
    assert rig.guards_clean()


def test_below_max_norm_the_coefficient_is_one_and_the_bits_are_those_without_clipping(rig):
    """The gradients times 2^-10: a norm of about 0.03 at max_norm = 1.  clip_coef is exactly 1.0 and p, m, v have the bits of the
    same step with max_norm = None (the second product is g * 1)."""
    rig.restore()
    _scaled(rig, 2.0 ** -10)
    rig.step(ema=False, decoupled=True, max_norm=None)
    want = _bits(rig.tensors())
    rig.restore()
    lists = _scaled(rig, 2.0 ** -10)
    rig.step(ema=False, decoupled=True, max_norm=1.0)
    st = rig.eng.read_state()
    assert 0.02 < st["total_norm"] < 0.04 and st["clip_coef"] == 1.0
    assert _same_bits(_bits(rig.tensors()), want)
    P, M, V, _, info = _oracle(rig, lists)
    assert info["coef"] == 1.0
    _hold("one_step_not_clipped", _out(rig), _torch_step(*lists[:4], rig.cpu[5])[:3], (P, M, V))
    rig.restore()


def test_a_lone_gradient_of_one():
    """One one-element tensor, g = 1.0, max_norm = 1: the coefficient is 1 / 1.000001 formed in fp64 and rounded once,
    1 - 17 * 2^-24 = 0.99999899.  torch forms it in fp32 (1 + 1e-6 rounds to 1 + 2^-20) and gets 1 - 16 * 2^-24 = 0.99999905, the
    value the feature's description quotes: one ulp apart (tests/test_adamw.py has both)."""
    p, g, m, v = (torch.full((1,), x, device="cuda") for x in (0.5, 1.0, 0.0, 0.0))
    eng = optim.UpdateEngine([1], "cuda")
    eng.set_tensors([p], [g], [m], [v])
    eng.step(HYPER, decoupled=True, max_norm=1.0)
    st = eng.read_state()
    assert st["total_norm"] == 1.0 and st["clip_coef"] == np.float32(1.0 / 1.000001) == np.float32(1 - 17 * 2.0 ** -24)
    assert _ulps32(st["clip_coef"], np.float32(0.99999905)) == 1
    assert float(m) == np.float32(np.float32(0.1) * st["clip_coef"]) and float(g) == 1.0  # lerp from 0 with weight 1 - beta1


def test_zero_gradients_decay_alone():
    """All gradients zero: the norm is 0, 1 / 1e-6 clamps to 1, the moments of zero tensors stay 0, and with weight_decay = 0.01
    p becomes exactly p * wmul, wmul = float32(1 - lr * 0.01), where p != 0 and stays 0 where p == 0: the decoupled form's
    counterpart of test_one_step_with_weight_decay_moves_the_tensor_without_a_gradient."""
    r = TG.Rig(hyper=HYPER)
    for lst in (r.g, r.m, r.v):
        for t in lst:
            t.zero_()
    before = _bits(r.p)
    r.step(ema=False, decoupled=True, max_norm=1.0)
    st = r.eng.read_state()
    assert st["total_norm"] == 0.0 and st["clip_coef"] == 1.0 and st["last_skip"] == 0 and st["adam_step"] == r.cpu[5] + 1
    wmul = np.float32(1.0 - HYPER[0] * HYPER[4])
    zeros = moved = 0
    for b, a, m, v in zip(before, _bits(r.p), r.m, r.v):
        assert np.array_equal((b.numpy() * wmul).view(np.int32), a.numpy().view(np.int32))
        zeros += int((b == 0).sum())
        moved += int((a != b).sum())
        assert not m.any() and not v.any()
        assert bool((a[b == 0] == 0).all())
    assert zeros >= 5 and moved > 10000 and r.guards_clean()  # (the exact zeros left are those of the tensor no warm-up step moved)


def test_the_old_entry_point_is_the_new_one_without_its_two_switches(rig):
    """egoego_optimw_step with decoupled = 0, max_norm = 0 against egoego_optim_step from identical inputs, EMA on, L2 weight
    decay 0.01: the same bits in p, m, v, ema and the same counters."""
    rig.restore()
    rig.step()
    want, cw, sw = _bits(rig.tensors()), rig.counters(), rig.eng.read_state()
    rig.restore()
    rig.step(decoupled=False, max_norm=0.0)
    st = rig.eng.read_state()
    assert _same_bits(_bits(rig.tensors()), want) and rig.counters() == cw
    assert st == sw and st["clip_coef"] == 1.0 and st["ema_action"] == _lib.OPTIM_EMA_LERP


def _skip_case(rig, zero_grads, plant=None, **kw):
    rig.restore()
    rig.step(ema=False, decoupled=True, max_norm=1.0)  # a clipped step first: clip_coef < 1 in the state
    assert rig.eng.read_state()["clip_coef"] < 0.05
    rig.restore()
    g0 = _bits(rig.g)
    if plant is not None:
        t, i, val = plant
        rig.g[t][i] = val
        g0[t][i] = val
    before, c0 = _bits(rig.tensors()), rig.counters()
    rig.step(ema=False, decoupled=True, max_norm=1.0, zero_grads=zero_grads, **kw)
    after, c1, st = _bits(rig.tensors()), rig.counters(), rig.eng.read_state()
    assert _same_bits(before, after), (plant, kw)
    assert c1 == c0[:4] + (c0[4] + 1,), (plant, kw, c0, c1)
    assert st["last_skip"] == 1 and st["clip_coef"] == 1.0 and int(rig.eng.last_skipped) == 1
    if zero_grads:
        assert not any(bool(g.any()) for g in rig.g)
    else:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(_bits(rig.g), g0))
    assert rig.guards_clean()


@pytest.mark.parametrize("zero_grads", [False, True])
def test_skips(rig, zero_grads):
    """A NaN in the last element of the last tensor, an inf norm under "nonfinite", and found_inf: nothing but `skipped`,
    `last_skip` and clip_coef (back to 1) changes; with zero_grads the gradients are cleared all the same."""
    last = len(SPECS) - 1
    _skip_case(rig, zero_grads, (last, SPECS[last][0] - 1, float("nan")))
    _skip_case(rig, zero_grads, (4, 17, float("inf")), skip_on="nonfinite")
    _skip_case(rig, zero_grads, found_inf=torch.tensor(1.0, device="cuda"))
    rig.restore()


def test_inv_scale_and_clipping_equal_prescaled_gradients(rig):
    rig.restore()
    rig.step(ema=False, decoupled=True, max_norm=1.0)
    want, st = _bits(rig.tensors()), rig.eng.read_state()
    rig.restore()
    for g in rig.g:
        g.mul_(1024.0)
    rig.step(ema=False, decoupled=True, max_norm=1.0, inv_scale=torch.tensor(2.0 ** -10, device="cuda"))
    st2 = rig.eng.read_state()
    assert _same_bits(_bits(rig.tensors()), want) and st2["total_norm"] == st["total_norm"] and st2["clip_coef"] == st["clip_coef"] < 1.0
    rig.restore()


def test_phases_2_and_3_and_mixed_phases():
    """PHASE_SPECS: heads of 2 and 1 elements, tensors shorter than their head, and tensors whose EMA sits at another phase (with
    the EMA in the call: scalars throughout), under clipping and decoupled decay; then the gradients' zeros and the guards."""
    r = TG.Rig(seed=4, specs=PHASE_SPECS, hyper=HYPER)
    r.step(ema=False, decoupled=True, max_norm=1.0)
    P, M, V, _, info = _oracle(r)
    assert info["coef"] < 1.0
    _hold("phases_2_3", _out(r), _torch_step(*r.cpu[:4], r.cpu[5])[:3], (P, M, V))
    assert r.guards_clean()
    r.restore()
    r.step(decoupled=True, max_norm=1.0, zero_grads=True)  # the EMA's phase differs in the last two tensors
    _hold("phases_mixed", _out(r), _torch_step(*r.cpu[:4], r.cpu[5])[:3], (P, M, V))
    assert not any(bool(g.any()) for g in r.g) and r.guards_clean()


def test_twenty_five_free_running_steps_under_step_lr():
    """FusedAdamW(max_grad_norm=1) under StepLR(step_size=10, gamma=0.3), one scheduler step per optimizer step: lr 1e-3, 3e-4,
    9e-5.  The oracle carries fp64 state, the device and torch's CPU run fp32 state; every |p| starts at 0.05 or more (25 steps
    of at most lr each and the decay move none to zero: see test_gpu_optim's 25-step test).  last_grad_norm is the norm before
    clipping."""
    sizes = (5, 198, CH + 3, 2 * CH + 5)
    gen = torch.Generator().manual_seed(12)
    p0 = [torch.randn(n, generator=gen) * 0.05 for n in sizes]
    p0 = [torch.where(x < 0, x - 0.05, x + 0.05) for x in p0]
    dev = [torch.nn.Parameter(x.clone().cuda()) for x in p0]
    cpu = [torch.nn.Parameter(x.clone()) for x in p0]
    fa = optim.FusedAdamW(dev, lr=1e-3, max_grad_norm=1.0)
    ta = torch.optim.AdamW(cpu, lr=1e-3, foreach=False)
    sf = torch.optim.lr_scheduler.StepLR(fa, step_size=10, gamma=0.3)
    st = torch.optim.lr_scheduler.StepLR(ta, step_size=10, gamma=0.3)
    P, M, V = [x.numpy() for x in p0], [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]
    c, lrs = AO.Counters(), []
    for k in range(25):
        g = [torch.randn(n, generator=gen) * 10.0 ** (-6 * torch.rand(n, generator=gen)) for n in sizes]
        for q, r, x in zip(dev, cpu, g):
            q.grad, r.grad = x.clone().cuda(), x.clone()
        lr = fa.param_groups[0]["lr"]
        lrs.append(lr)
        assert lr == ta.param_groups[0]["lr"]
        fa.step()
        torch.nn.utils.clip_grad_norm_(cpu, 1.0, error_if_nonfinite=False, foreach=False)
        ta.step()
        P, M, V, c, info = AO.step(P, [x.numpy() for x in g], M, V, c, lr=lr, weight_decay=1e-2, max_norm=1.0)
        assert info["coef"] < 1.0 and float(fa.last_grad_norm) == np.float32(info["norm"]), k
        sf.step()
        st.step()
    assert lrs[0] == 1e-3 and lrs[10] == pytest.approx(3e-4) and lrs[20] == pytest.approx(9e-5)
    ctr = fa.counters()
    assert (ctr["adam_step"], ctr["applied"], ctr["skipped"]) == (25, 25, 0)
    got = ([q.detach() for q in dev], [fa.state[q]["exp_avg"] for q in dev], [fa.state[q]["exp_avg_sq"] for q in dev])
    tor = ([q.detach() for q in cpu], [ta.state[q]["exp_avg"] for q in cpu], [ta.state[q]["exp_avg_sq"] for q in cpu])
    _hold("free_running_25_step_lr", got, tor, (P, M, V))
    assert float(fa.state_dict()["state"][0]["step"]) == 25.0


def test_the_same_step_twice_gives_the_same_bits(rig):
    rig.restore()
    rig.step(decoupled=True, max_norm=1.0)
    a, sa = _bits(rig.tensors()), rig.eng.read_state()
    rig.restore()
    rig.eng._ws.view(torch.float32).fill_(float("nan"))  # what the workspace held is irrelevant
    rig.step(decoupled=True, max_norm=1.0)
    assert _same_bits(_bits(rig.tensors()), a) and rig.eng.read_state() == sa
    rig.restore()


def test_a_clipped_step_runs_on_the_callers_stream_and_replays_from_a_graph(rig):
    rig.restore()
    torch.cuda.synchronize()
    flat = torch.cat([g.reshape(-1) for g in rig.g]).clone()
    sizes = [n for n, _ in SPECS]

    def call(gflat):
        rig.restore()
        for d, s in zip(rig.g, gflat.split(sizes)):
            d.copy_(s)
        rig.step(zero_grads=True, decoupled=True, max_norm=1.0)
        return rig.tensors() + rig.g + [rig.eng.last_grad_norm, rig.eng.last_clip_coef, rig.ema_step]

    call(flat)
    delay = SC.Delay().calibrate({"optim_step_w": lambda: call(flat)})
    SC.check("optim_step_w", SC.ENQUEUES, call, [flat], torch.cuda.Stream(), delay, decoys=[flat.flip(0).contiguous()])
    # one captured step (a linear chain of three launches) replayed three times = three eager steps
    rig.restore()
    for _ in range(3):
        rig.step(decoupled=True, max_norm=1.0)
    want, cw = _bits(rig.tensors()), rig.counters()
    rig.restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.step(decoupled=True, max_norm=1.0)
    rig.restore()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(_bits(rig.tensors()), want) and rig.counters() == cw
    rig.restore()


def test_bad_arguments_are_refused_before_any_launch(rig):
    rig.restore()
    before = _bits(rig.tensors())
    for kw, word in ((dict(max_norm=float("nan")), "max_norm"), (dict(max_norm=1.0, clip_eps=-1e-6), "clip_eps"),
                     (dict(max_norm=1.0, clip_eps=float("nan")), "clip_eps")):
        with pytest.raises(_lib.EgoEgoHipError, match=word):
            rig.step(ema=False, decoupled=True, **kw)
    h = _lib.OptimHyperW(*HYPER, 2, 1.0, 1e-6)
    import ctypes as C
    ws, wn = rig.eng._workspace()
    rc = rig.eng.lib.egoego_optimw_step(rig.eng._ctx, C.byref(h), None, None, 0, None, None, 0, 0, 1, 0, rig.eng.state.data_ptr(),
                                         rig.eng.state.numel(), ws, wn, rig.eng._stream())
    assert rc != 0 and "decoupled" in rig.eng.lib.egoego_optim_last_error().decode()
    assert _same_bits(_bits(rig.tensors()), before) and rig.eng.read_state()["applied"] == 0


# ---------------------------------------------------------------------------------------------------------------- stage 1
W1, B1 = 8, 2


def _opt():
    return Namespace(window=W1, n_dec_layers=1, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, w_rotation=1.0, w_va=1.0,
                     w_dist=1.0, dist_scale=10.0)


def _module(kind):
    cls = stage1.HeadFormer if kind == "headnet" else stage1.HeadNormalFormer
    return cls(_opt(), torch.device("cuda")).cuda()  # (the constructor's seeded weights: every module starts the same)


def _batch(kind, seed):
    return {k: v.cuda() for k, v in make_stage1_train_batch(kind, B1, W1, seed=seed).items()}


def _trainer(kind, tmp, **kw):
    tr = Stage1Trainer(_module(kind), [], save_dir=str(tmp), save_interval=1, lr=1e-3, **kw)
    tr.model.eval()  # no dropout: the same bits on every run (hip_training stays on: the training encode, with a graph)
    return tr


def _forward(m, batch):
    with torch.no_grad():
        return [t.clone() for t in SC.flat(m(batch))]


@pytest.mark.parametrize("kind", ["headnet", "gravitynet"])
def test_stage1_inference_sees_the_fused_step(kind, tmp_path):
    """The inference engine packs the weights once per (data_ptr, _version); the fused step moves neither.  After one
    Stage1Trainer(fused_update=True).step an eval()-mode no_grad forward equals, bit for bit, that of a fresh module loaded from
    the trained module's state_dict(): the step's invalidate_engine() call.  The update synchronises nothing; for GravityNet on
    a device-resident batch the whole step is held to that (HeadNet's forward uploads a few host integers per call, fused or not)."""
    tr = _trainer(kind, tmp_path, fused_update=True)
    batch = _batch(kind, 1)
    old = _forward(tr.model, batch)  # a packed copy of the OLD weights exists
    w0 = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    tr.optimizer.step = _strict(tr.optimizer.step)
    step = _strict(tr.step) if kind == "gravitynet" else tr.step
    parts = step(batch)
    step(_batch(kind, 2))
    assert len(parts) == len(tr.keys) and math.isfinite(float(parts[0]))
    assert sum(not torch.equal(v, w0[k]) for k, v in tr.model.state_dict().items()) >= 10
    ctr = tr.optimizer.counters()
    assert (ctr["adam_step"], ctr["applied"], ctr["skipped"]) == (2, 2, 0) and 0.0 < ctr["clip_coef"] <= 1.0
    trainable = [p for p in tr.model.parameters() if p.requires_grad]
    assert len(trainable) > 10 and not any(bool(p.grad.any()) for p in trainable)  # zero_grads: cleared, not clipped in place
    fresh = _module(kind)
    fresh.load_state_dict({k: v.detach().clone() for k, v in tr.model.state_dict().items()})
    fresh.eval()
    new, want = _forward(tr.model, batch), _forward(fresh, batch)
    assert len(new) == len(want) > 0 and all(torch.equal(a, b) for a, b in zip(new, want))
    assert any(not torch.equal(a, b) for a, b in zip(new, old))


def _strict(fn):
    """fn under torch.cuda.set_sync_debug_mode("error"): a synchronisation inside it raises (tests/test_gpu_stage1_data.py's)."""
    def wrapped(*args, **kwargs):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return wrapped


def _curve(tr, kind, steps=8):
    return [float(tr.step(_batch(kind, 10 + k))[0]) for k in range(steps)]


@pytest.mark.parametrize("kind", ["headnet", "gravitynet"])
def test_stage1_loss_curves_fused_against_torch(kind, tmp_path):
    """8 steps from the same start in eval() mode with fused_update on and off.  The yardstick is torch against itself: the
    default path with AdamW(foreach=True) against AdamW(foreach=False), the same formula in another order of roundings.  The
    fused curve stays within 4 times that distance of the default path's, and never held below 1e-6 relative."""
    with pytest.raises(RuntimeError):
        _strict(lambda: torch.ones(1, device="cuda").item())()
    runs = {}
    for name, kw, foreach in (("fused", dict(fused_update=True), None), ("torch", {}, True), ("torch_for", {}, False)):
        tr = _trainer(kind, tmp_path / name, **kw)
        if foreach is not None:
            tr.optimizer = torch.optim.AdamW(tr.model.parameters(), lr=1e-3, foreach=foreach)
        runs[name] = _curve(tr, kind)
    rel = lambda a, b: max(abs(x - y) / abs(y) for x, y in zip(a, b))  # noqa: E731
    d_torch, d_fused = rel(runs["torch_for"], runs["torch"]), rel(runs["fused"], runs["torch"])
    print(f"{kind}: loss curves over 8 steps: fused against torch {d_fused:.3e}; torch foreach against for-loop {d_torch:.3e}")
    _record(f"stage1_{kind}_loss_curve", d_fused=d_fused, d_torch=d_torch, first_loss=runs["torch"][0], last_loss=runs["torch"][-1])
    assert all(math.isfinite(x) for x in runs["fused"]) and runs["fused"][0] == runs["torch"][0]
    assert d_fused <= max(4 * d_torch, 1e-6), (d_fused, d_torch)


def test_stage1_checkpoints_resume_under_the_other_path(tmp_path):
    kind = "gravitynet"
    for first, second in ((True, False), (False, True)):
        tmp = tmp_path / str(first)
        a = _trainer(kind, tmp, fused_update=first)
        for k in range(2):
            a.step(_batch(kind, 20 + k))
        a.epoch = 1
        path = a.save(1)
        ck = torch.load(path, map_location="cpu")
        assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "transformer_encoder_state_dict"]
        sd = ck["optimizer_state_dict"]
        assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][0]["step"]) == 2.0
        keys = set(torch.optim.AdamW([torch.zeros(1)]).state_dict()["param_groups"][0]) | {"initial_lr"}  # (StepLR's addition)
        assert set(sd["param_groups"][0]) == keys
        b = _trainer(kind, tmp, fused_update=second)
        b.load(path)
        assert b.epoch == 1 and all(torch.equal(v, ck["transformer_encoder_state_dict"][k].cuda()) for k, v in b.model.state_dict().items())
        held = b.optimizer.param_groups[0]["params"]  # (a frozen parameter has an index and no state)
        assert len(sd["state"]) > 10 and all(torch.equal(b.optimizer.state[held[i]]["exp_avg_sq"].cpu(), st["exp_avg_sq"])
                                             for i, st in sd["state"].items())
        # the resumed step against the same step on the path that wrote the checkpoint: the same formula, other roundings
        la, lb = a.step(_batch(kind, 30)), b.step(_batch(kind, 30))
        assert float(la[0]) == float(lb[0])  # the loss is taken before the update: the same weights, the same bits
        assert float(b.optimizer.state_dict()["state"][0]["step"]) == 3.0
        # p' = p wmul - s q: half an ulp of |p| for each of the product and the difference, and |s q| <= 2 lr (three steps in,
        # |m^| / sqrt(v^) stays below 2) known to about 12 ulp (torch's coefficient comes from an fp32 norm of norms: a few ulp;
        # the clipped gradient, two roundings in exp_avg, three in exp_avg_sq, the quotients and eps): 2^-23 (max |p| + 24 lr)
        for (n, x), (_, y) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
            assert torch.allclose(x, y, rtol=0, atol=2.0 ** -23 * (float(x.abs().max()) + 24 * 1e-3)), n


def test_the_training_tool_with_fused_update(tmp_path, capsys):
    """tools/train_stage1.py --fused_update, in this process (the test is about the tool's loop): 2 epochs on synthetic batches."""
    spec = importlib.util.spec_from_file_location("train_stage1_tool_fused", os.path.join(ROOT, "tools", "train_stage1.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "run"
    tool.main(["--kind", "headnet", "--fused_update", "--save_dir", str(out), "--epochs", "2", "--window", str(W1), "--n_dec_layers", "1",
               "--batch_size", str(B1), "--synthetic_batches", "2", "--save_interval", "2"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["epoch"] for l in lines[:2]] == [1, 2] and math.isfinite(lines[1]["train"]["loss"]) and "val" in lines[0]
    assert json.load(open(out / "opt.json"))["fused_update"] is True
    ck = torch.load(out / "weights" / "train-2.pt", map_location="cpu", weights_only=True)
    assert float(ck["optimizer_state_dict"]["state"][0]["step"]) == 4.0
    stage1.HeadFormer(_opt(), torch.device("cuda")).load_state_dict(ck["transformer_encoder_state_dict"])
