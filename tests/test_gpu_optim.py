"""The fused parameter update on the GPU (csrc/optim_step.*, egoego_release_amd/optim.py) against the fp64 oracle of
tests/optim_oracle.py, on tensor lists unless a test says otherwise.

The bar of every comparison with the oracle: for each of p, exp_avg, exp_avg_sq and ema, d = the largest distance from the oracle
in units of the oracle value's fp32 ulp; d_torch is the same figure for torch.optim.Adam(foreach=False) and the three-line lerp on
the CPU from the same fp32 inputs; d_hip <= 2 d_torch + 1.  Both evaluate the same few-rounding formula; FMA contraction and the
device's fp64 scalars change the order of the roundings, so neither bounds the other element by element.

EGOEGO_OPTIM_RECORD=<file>: the measured d values are written there as JSON (profiles/optim_error.json is such a file).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import optim_oracle as OO
import stream_cases as SC
from egoego_release_amd import ModelConfig, make_weights, _lib, optim

pytestmark = pytest.mark.gpu

CH = _lib.OPTIM_CHUNK
# (elements, element offset of p / g / m / v / ema inside a larger buffer)
SPECS = [(1, (0, 0, 0, 0, 0)), (3, (0, 0, 0, 0, 0)), (198, (1, 0, 0, 0, 0)),  # a view one element in: phases differ, scalars throughout
         (CH - 1, (0, 0, 0, 0, 0)), (CH, (0, 0, 0, 0, 0)), (CH + 1, (1, 1, 1, 1, 1)),  # one phase, off the boundary: head, body, tail
         (2 * CH + 5, (0, 0, 0, 0, 0)), (37, (0, 0, 0, 0, 0))]  # the last one: zero gradient, zero moments
ZERO = len(SPECS) - 1
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.0)
_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_OPTIM_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _inputs(seed=0, warm=3, away=0.0):
    """fp32 CPU lists p, g, m, v, ema: p ~ N(0, 0.05) with some exact zeros, g = N(0, 1) * 10^U(-6, 0), moments from `warm`
    oracle steps on other gradients (rounded to fp32), ema = p moved a little.  away > 0: no zeros, and every |p| >= away."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [n for n, _ in SPECS]

    def grads():
        out = [torch.randn(n, generator=gen) * 10.0 ** (-6 * torch.rand(n, generator=gen)) for n in sizes]
        out[ZERO] = torch.zeros(sizes[ZERO])
        return out

    p = [torch.randn(n, generator=gen) * 0.05 for n in sizes]
    for x in p:
        if away:
            x.copy_(torch.where(x < 0, x - away, x + away))
        else:
            x[::7] = 0.0
    P, M, V = [x.numpy() for x in p], [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]
    c = OO.Counters()
    for _ in range(warm):
        P, M, V, _, c, _ = OO.step(P, [g.numpy() for g in grads()], M, V, None, c, lr=HYPER[0], do_ema=False)
    p = [torch.from_numpy(x.astype(np.float32)) for x in P]
    m = [torch.from_numpy(np.asarray(x, np.float64).astype(np.float32)) for x in M]
    v = [torch.from_numpy(np.asarray(x, np.float64).astype(np.float32)) for x in V]
    ema = [x + 1e-3 * torch.randn(x.shape, generator=gen) for x in p]
    return p, grads(), m, v, ema, c.adam_step


def _views(lists):
    """The five CPU lists on the device, each tensor a view at its SPECS offset into a buffer of its own."""
    out = []
    for which, lst in enumerate(lists):
        dev = []
        for (n, offs), t in zip(SPECS, lst):
            buf = torch.zeros(n + offs[which] + 3, device="cuda")
            view = buf[offs[which]:offs[which] + n]
            view.copy_(t)
            dev.append(view)
        out.append(dev)
    return out


class Rig:
    """One UpdateEngine over SPECS with device lists p, g, m, v, ema and the EMA's two counters."""

    def __init__(self, seed=0, ema_step=120, initted=1.0, away=0.0, **sched):
        self.cpu = _inputs(seed, away=away)
        self.p, self.g, self.m, self.v, self.e = _views(self.cpu[:5])
        self.eng = optim.UpdateEngine([n for n, _ in SPECS], "cuda")
        self.eng.set_tensors(self.p, self.g, self.m, self.v, self.e)
        self.ema_step = torch.tensor([ema_step], device="cuda")
        self.initted = torch.tensor([initted], device="cuda")
        self.sched_kw = dict(beta=0.995, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0, update_every=10, update_after_step=100)
        self.sched_kw.update(sched)
        self.eng.adam_step.fill_(self.cpu[5])
        self.start = self.snapshot()
        torch.cuda.synchronize()

    def sched(self):
        k = self.sched_kw
        return _lib.OptimEma(k["beta"], k["inv_gamma"], k["power"], k["min_value"], k["update_every"], k["update_after_step"],
                             self.ema_step.data_ptr(), self.initted.data_ptr())

    def step(self, ema=True, **kw):
        self.eng.step(HYPER, self.sched() if ema else None, **kw)

    def tensors(self):
        return self.p + self.m + self.v + self.e

    def snapshot(self):
        return [t.clone() for t in self.tensors() + self.g + [self.ema_step, self.initted, self.eng.state[:_lib.OptimState.total_norm.offset]]]

    def restore(self, snap=None):
        snap = self.start if snap is None else snap
        for t, s in zip(self.tensors() + self.g + [self.ema_step, self.initted, self.eng.state[:_lib.OptimState.total_norm.offset]], snap):
            t.copy_(s)

    def counters(self):
        st = self.eng.read_state()
        return (st["adam_step"], int(self.ema_step), int(float(self.initted)), st["applied"], st["skipped"])

    def oracle(self, c, lists=None, **kw):
        p, g, m, v, e = lists if lists is not None else self.cpu[:5]
        k = dict(self.sched_kw)
        return OO.step([x.numpy() for x in p], [x.numpy() for x in g], [x.numpy() for x in m], [x.numpy() for x in v],
                       [x.numpy() for x in e], c, lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3], **k, **kw)


def _bits(ts):
    return [t.detach().cpu().clone() for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _torch_step(p, g, m, v, e, adam_step, decay):
    """torch.optim.Adam(foreach=False) and ema-pytorch's lerp on the CPU from fp32 lists (decay None: the EMA is left alone)."""
    params = [torch.nn.Parameter(x.clone()) for x in p]
    opt = torch.optim.Adam(params, lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3], foreach=False)
    for q, gg, mm, vv in zip(params, g, m, v):
        q.grad = gg.clone()
        opt.state[q] = {"step": torch.tensor(float(adam_step)), "exp_avg": mm.clone(), "exp_avg_sq": vv.clone()}
    opt.step()
    ema = [x.clone() for x in e]
    if decay is not None:
        for x, q in zip(ema, params):
            difference = x - q.data
            difference.mul_(1.0 - decay)
            x.sub_(difference)
    return ([q.detach() for q in params], [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params], ema)


def _distances(got, want):
    """The four d values (p, m, v, ema) of lists-of-lists `got` against the oracle's fp64 lists."""
    return [max(OO.ulp_distance(x.detach().cpu().numpy(), w) for x, w in zip(a, b)) for a, b in zip(got, want)]


def _hold(case, d_hip, d_torch):
    for name, h, t in zip(("p", "exp_avg", "exp_avg_sq", "ema"), d_hip, d_torch):
        print(f"{case}: {name}: d_hip {h:.3f}  d_torch {t:.3f}")
    _record(case, d_hip=dict(zip(("p", "exp_avg", "exp_avg_sq", "ema"), d_hip)), d_torch=dict(zip(("p", "exp_avg", "exp_avg_sq", "ema"), d_torch)))
    for name, h, t in zip(("p", "exp_avg", "exp_avg_sq", "ema"), d_hip, d_torch):
        assert h <= 2 * t + 1, (case, name, h, t)


@pytest.fixture(scope="module")
def rig():
    return Rig()


def test_one_step_against_the_oracle_at_the_kernel_edges(rig):
    """Counts 1, 3, 198 (a view one element in), CHUNK - 1, CHUNK, CHUNK + 1 (all five one element in), 2 CHUNK + 5, and a tensor
    with zero gradient and zero moments: its parameter keeps its bits and its moments stay exactly 0.  The EMA lerps (counter 120)."""
    rig.restore()
    assert not rig.g[ZERO].any() and not rig.m[ZERO].any() and not rig.v[ZERO].any()  # (_inputs: no gradient ever reached it)
    p0 = _bits(rig.p)
    rig.step()
    c0 = OO.Counters(adam_step=rig.cpu[5], ema_step=120, initted=True)
    P, M, V, E, c1, info = rig.oracle(c0)
    assert info["action"] == "lerp" and not info["skip"]
    assert rig.counters() == c1.as_tuple()
    st = rig.eng.read_state()
    assert st["ema_action"] == _lib.OPTIM_EMA_LERP and st["last_skip"] == 0
    assert st["one_minus_decay"] == pytest.approx(1.0 - info["decay"], rel=1.2e-7) and st["step_size"] == pytest.approx(HYPER[0] / (1 - 0.9 ** c1.adam_step), rel=1e-6)
    tor = _torch_step(*rig.cpu[:5], rig.cpu[5], info["decay"])
    _hold("one_step", _distances((rig.p, rig.m, rig.v, rig.e), (P, M, V, E)), _distances(tor, (P, M, V, E)))
    assert _same_bits(_bits([rig.p[ZERO]]), [p0[ZERO]])
    assert not rig.m[ZERO].any() and not rig.v[ZERO].any()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(rig.g, rig.cpu[1]))  # zero_grads off: the gradients stay


def test_twenty_five_free_running_steps():
    """update_every = 3, update_after_step = 4: the copy phase, the first call past it, the steady lerp.  Exact on the way: ema
    has p's bits on a copy step and its own on the steps in between; the counters are the oracle's.  At the end: the bar.

    The oracle carries fp64 state through the run, the device and torch fp32 state.  The bar counts in ulps of the oracle's
    value, so it says nothing about a parameter that passes zero on the way: any fp32 run, torch's included, is then thousands of
    ulps of that value away, by an amount that is chance (with the one-step test's inputs: p 7300 on the device, 3157 for torch,
    both at the same element).  28 steps of at most lr = 1e-3 each move a parameter by at most 0.028, so every |p| starts at 0.05
    or more.  exp_avg mixes signs whatever the inputs; its distances are large and come out equal on both sides."""
    r = Rig(seed=1, ema_step=0, initted=0.0, away=0.05, update_every=3, update_after_step=4)
    gen = torch.Generator().manual_seed(9)
    cur = [[x.clone() for x in lst] for lst in r.cpu[:5]]  # the torch side's fp32 state
    O = [[x.numpy().astype(np.float64) for x in lst] for lst in r.cpu[:5]]  # the oracle's fp64 state
    c, adam_step = OO.Counters(adam_step=r.cpu[5]), r.cpu[5]
    seen = set()
    for k in range(25):
        g = [torch.randn(n, generator=gen) * 10.0 ** (-6 * torch.rand(n, generator=gen)) for n, _ in SPECS]
        for d, s in zip(r.g, g):
            d.copy_(s)
        before = _bits(r.e)
        r.step()
        P, M, V, E, c, info = OO.step(O[0], [x.numpy() for x in g], O[2], O[3], O[4], c, lr=HYPER[0], **r.sched_kw)
        O = [P, None, M, V, E]
        seen.add(info["action"])
        tor = _torch_step(cur[0], g, cur[2], cur[3], cur[4], adam_step, info["decay"])
        if info["action"] == "copy":
            tor = tor[:3] + ([x.clone() for x in tor[0]],)
            assert _same_bits(_bits(r.e), _bits(r.p)), k
        elif info["action"] == "none":
            assert _same_bits(_bits(r.e), before), k
        cur = [tor[0], None, tor[1], tor[2], tor[3]]
        adam_step += 1
        assert r.counters() == c.as_tuple(), k
    assert seen == {"copy", "none", "lerp"} and c.initted and c.ema_step == 25
    _hold("free_running_25", _distances((r.p, r.m, r.v, r.e), (O[0], O[2], O[3], O[4])),
          _distances((cur[0], cur[2], cur[3], cur[4]), (O[0], O[2], O[3], O[4])))


def test_the_norm(rig):
    """Against numpy's fp64 sqrt(sum g^2) within n 2^-53 (relative); the same bits on two runs and with a NaN-filled workspace."""
    rig.restore()
    rig.step()
    st = rig.eng.read_state()
    n = sum(k for k, _ in SPECS)
    want = float(np.sqrt(sum(np.sum(x.numpy().astype(np.float64) ** 2) for x in rig.cpu[1])))
    assert abs(st["total_norm"] - want) <= n * 2.0 ** -53 * want
    assert st["total_norm_f32"] == np.float32(st["total_norm"]) and float(rig.eng.last_grad_norm) == st["total_norm_f32"]
    rig.restore()
    rig.step()
    again = rig.eng.read_state()["total_norm"]
    rig.restore()
    rig.eng._ws.view(torch.float32).fill_(float("nan"))
    rig.step()
    st2 = rig.eng.read_state()
    assert np.float64(again).tobytes() == np.float64(st["total_norm"]).tobytes() == np.float64(st2["total_norm"]).tobytes()
    assert st2["last_skip"] == 0 and st2["applied"] == 1


def _skip_case(rig, zero_grads, plant=None, **kw):
    rig.restore()
    g0 = _bits(rig.g)
    if plant is not None:
        t, i, val = plant
        rig.g[t][i] = val
        g0[t][i] = val
    before, c0 = _bits(rig.tensors()), rig.counters()
    rig.step(zero_grads=zero_grads, **kw)
    after, c1 = _bits(rig.tensors()), rig.counters()
    assert _same_bits(before, after), (plant, kw)
    assert c1 == c0[:4] + (c0[4] + 1,), (plant, kw, c0, c1)
    assert int(rig.eng.last_skipped) == 1
    if zero_grads:
        assert not any(bool(g.any()) for g in rig.g)  # (NaN != 0: a NaN left behind counts)
    else:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(_bits(rig.g), g0))


@pytest.mark.parametrize("zero_grads", [False, True])
def test_skips(rig, zero_grads):
    nan = float("nan")
    last = len(SPECS) - 1
    for plant in ((0, 0, nan), (last, SPECS[last][0] - 1, nan), (6, 2 * CH + 4, nan)):  # first of the first, last of the last, a scalar tail
        _skip_case(rig, zero_grads, plant)
    one, bad = torch.tensor(0.5, device="cuda"), torch.tensor(nan, device="cuda")
    _skip_case(rig, zero_grads, losses=[one, bad])
    _skip_case(rig, zero_grads, found_inf=torch.tensor(1.0, device="cuda"))
    _skip_case(rig, zero_grads, (4, 17, float("inf")), skip_on="nonfinite")
    _skip_case(rig, zero_grads, losses=[one, torch.tensor(float("-inf"), device="cuda")], skip_on="nonfinite")
    # under "nan", the reference's rule, an inf gradient steps; two finite losses and found_inf = 0 step too
    rig.restore()
    rig.g[4][17] = float("inf")
    rig.step(zero_grads=zero_grads)
    assert int(rig.eng.last_skipped) == 0 and rig.eng.read_state()["total_norm"] == float("inf")
    rig.restore()
    c0 = rig.counters()
    rig.step(zero_grads=zero_grads, losses=[one, one], found_inf=torch.tensor(0.0, device="cuda"))
    c1 = rig.counters()
    assert c1[0] == c0[0] + 1 and c1[3] == c0[3] + 1 and c1[4] == c0[4]
    assert bool(any(g.any() for g in rig.g)) is (not zero_grads)


def test_inv_scale_is_exact_for_a_power_of_two(rig):
    rig.restore()
    rig.step()
    want, norm = _bits(rig.tensors()), rig.eng.read_state()["total_norm"]
    rig.restore()
    for g in rig.g:
        g.mul_(1024.0)
    rig.step(inv_scale=torch.tensor(1.0 / 1024.0, device="cuda"))
    assert _same_bits(_bits(rig.tensors()), want) and rig.eng.read_state()["total_norm"] == norm


def _small_fused(seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.05).cuda()) for n in (5, 198, CH + 3)]
    grads = [(torch.randn(p.shape, generator=gen) * 0.1).cuda() for p in params]
    return params, grads


def test_grad_scaler_steps_and_skips_without_a_read_back():
    pa, grads = _small_fused()
    pb, _ = _small_fused()
    oa, ob = optim.FusedAdam(pa, lr=1e-3), optim.FusedAdam(pb, lr=1e-3)
    for p, g in zip(pa, grads):
        p.grad = g.clone()
    oa.step()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    loss = sum((p * g).sum() for p, g in zip(pb, grads))  # d loss / d p = g: the scaled backward leaves 1024 g
    scaler.scale(loss).backward()
    assert torch.equal(pb[1].grad, grads[1] * 1024.0)
    scaler.step(ob)
    scaler.update()
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert float(scaler.get_scale()) == 1024.0 and ob.counters()["applied"] == 1
    assert not hasattr(ob, "grad_scale") and not hasattr(ob, "found_inf")
    # an inf planted: the step is skipped on the device and the scaler halves its scale
    before = _bits(pb)
    ob.zero_grad()
    scaler.scale(sum((p * g).sum() for p, g in zip(pb, grads))).backward()
    pb[2].grad[CH + 1] = float("inf")
    scaler.step(ob)
    scaler.update()
    assert _same_bits(_bits(pb), before)
    c = ob.counters()
    assert (c["adam_step"], c["applied"], c["skipped"]) == (1, 1, 1) and float(scaler.get_scale()) == 512.0


def test_fused_adam_front():
    """The optimizer in front of the engine: a missing gradient raises; the state dict is torch.optim.Adam's and loads into it and
    back; zero_grad() clears in place; zero_grads=True makes it a no-op."""
    pa, grads = _small_fused(3)
    oa = optim.FusedAdam(pa, lr=1e-3, zero_grads=True)
    with pytest.raises(RuntimeError):
        oa.step()
    for p, g in zip(pa, grads):
        p.grad = g.clone()
    ptrs = [p.grad.data_ptr() for p in pa]
    oa.step()
    assert not any(bool(p.grad.any()) for p in pa) and [p.grad.data_ptr() for p in pa] == ptrs
    for p, g in zip(pa, grads):
        p.grad.copy_(g)
    oa.zero_grad()  # a no-op: step() clears
    assert torch.equal(pa[0].grad, grads[0])
    oa.step()
    sd = oa.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0 and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ot = torch.optim.Adam(pt, lr=1e-3, foreach=False)
    ot.load_state_dict(copy.deepcopy(sd))
    ob = optim.FusedAdam([torch.nn.Parameter(p.detach().clone()) for p in pa], lr=1.0)
    ob.load_state_dict(copy.deepcopy(ot.state_dict()))
    for plist in (pa, pt, ob.param_groups[0]["params"]):
        for p, g in zip(plist, grads):
            p.grad = g.clone()
    oa.step()
    ot.step()
    ob.step()
    assert ob.counters()["adam_step"] == 3
    assert all(torch.equal(a, b) for a, b in zip(pa, ob.param_groups[0]["params"]))
    for a, t in zip(pa, pt):  # torch's own arithmetic: the same formula, its own roundings
        assert torch.allclose(a, t, rtol=0, atol=4 * 2.0 ** -24 * (float(a.detach().abs().max()) + 1e-3))
    plain = optim.FusedAdam(pt, fused=False)
    plain.zero_grad()
    assert not any(bool(p.grad.any()) for p in pt)


def test_ema_update_alone_is_the_same_call():
    """EMA.update() by itself (do_adam = 0) against the plain path of the same class, over the copy phase and the first lerps."""
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(31, 67)
            self.frozen = torch.nn.Parameter(torch.ones(5), requires_grad=False)
            self.register_buffer("buf", torch.arange(4.0))

    torch.manual_seed(0)
    net = Net().cuda()
    fused = optim.EMA(net, beta=0.995, update_every=2, update_after_step=3)
    plain = optim.EMA(net, beta=0.995, update_every=2, update_after_step=3, fused=False).cuda()
    assert sorted(fused.state_dict()) == sorted(plain.state_dict()) and "initted" in fused.state_dict() and "ema_model.a.weight" in fused.state_dict()
    online = dict(net.named_parameters())
    for k in range(11):
        with torch.no_grad():
            for p in net.a.parameters():
                p.add_(0.01 * torch.randn_like(p))
        prev = [{n: e.clone() for n, e in side.ema_model.named_parameters()} for side in (fused, plain)]
        fused.update()
        plain.update()
        assert int(fused.step) == int(plain.step) == k + 1 and float(fused.initted) == float(plain.initted)
        action = optim.ema_action(k, k > 4, 2, 3)
        for (n, a), (_, b) in zip(fused.ema_model.named_parameters(), plain.ema_model.named_parameters()):
            if action == "none" or not online[n].requires_grad:
                assert torch.equal(a, prev[0][n]) and torch.equal(b, prev[1][n]), (k, n)
            elif action == "copy":
                assert torch.equal(a, online[n]) and torch.equal(b, online[n]), (k, n)
            # one FMA against three roundings: under two ulps of the tensor's largest value per lerp, carried on times a decay
            # below 1, over the three lerps of this run
            assert torch.allclose(a, b, rtol=0, atol=6 * 2.0 ** -24 * float(b.abs().max())), (k, n)
    assert float(fused.initted) == 1.0


def test_a_step_runs_on_the_callers_stream_and_replays_from_a_graph(rig):
    rig.restore()
    torch.cuda.synchronize()
    flat = torch.cat([g.reshape(-1) for g in rig.g]).clone()
    sizes = [n for n, _ in SPECS]

    def call(gflat):
        rig.restore()
        for d, s in zip(rig.g, gflat.split(sizes)):
            d.copy_(s)
        rig.step(zero_grads=True)
        return rig.tensors() + rig.g + [rig.eng.last_grad_norm, rig.ema_step]

    call(flat)
    delay = SC.Delay().calibrate({"optim_step": lambda: call(flat)})
    SC.check("optim_step", SC.ENQUEUES, call, [flat], torch.cuda.Stream(), delay, decoys=[flat.flip(0).contiguous()])
    # one captured step replayed three times = three eager steps: the counters live on the device and no pointer changes
    rig.restore()
    for _ in range(3):
        rig.step()
    want, cw = _bits(rig.tensors()), rig.counters()
    rig.restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.step()
    rig.restore()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(_bits(rig.tensors()), want) and rig.counters() == cw


# ---------------------------------------------------------------------------------------------------------------- with the model
def _trainer(fused, tmp_path, seed=0):
    from egoego_release_amd.model import CondGaussianDiffusion
    from egoego_release_amd.trainer import Stage2Trainer
    cfg = ModelConfig(n_dec_layers=1, max_timesteps=12)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type="l1")
    sd = make_weights(cfg, seed)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    m.hip_training = True
    m.train()
    gen = torch.Generator().manual_seed(5)
    batches = [{"motion": (torch.randn(2, 11, 198, generator=gen) * 0.5).cuda(), "seq_len": torch.tensor([11, 8])} for _ in range(2)]
    tr = Stage2Trainer(m, batches, fused=fused, results_folder=str(tmp_path), ema_update_every=1)
    tr.optimizer.zero_grads = False  # the test reads the gradients after the step
    return cfg, sd, tr


def _sample_inputs(S=4):
    gen = torch.Generator().manual_seed(99)
    xs = torch.randn(2, 11, 198, generator=gen) * 0.5
    cm = torch.ones(2, 11, 198)
    cm[..., 45:48] = 0
    cm[..., 156:162] = 0
    noise = {"x_T": torch.randn(xs.shape, generator=gen), "cond": torch.randn(xs.shape, generator=gen),
             "steps": torch.randn(S, *xs.shape, generator=gen)}
    return xs.cuda(), cm.cuda(), noise


def test_one_trainer_step_fused_against_plain_and_the_sampler_sees_it(tmp_path):
    from egoego_release_amd.model import CondGaussianDiffusion
    cfg, sd, tf = _trainer(True, tmp_path / "f")
    _, _, tp = _trainer(False, tmp_path / "p")
    S = 4
    xs, cm, noise = _sample_inputs(S)
    for m in (tf.model, tf.ema.ema_model):  # both have sampled before the step: a packed copy of the OLD weights exists
        m.num_timesteps = S
        m.sample(xs, cm, noise=noise)
        m.num_timesteps = cfg.timesteps
    torch.manual_seed(7)
    assert tf.train(1) == 1
    torch.manual_seed(7)
    assert tp.train(1) == 1
    named_f, named_p = dict(tf.model.named_parameters()), dict(tp.model.named_parameters())
    trainable = [n for n, p in named_f.items() if p.requires_grad]
    assert len(trainable) == 16 + 8
    for n in trainable:  # §5j: the gradients of the HIP training step are the same bits from run to run
        assert torch.equal(named_f[n].grad, named_p[n].grad), n
    p0 = [sd[n].reshape(-1) for n in trainable]
    z = [np.zeros(x.numel(), np.float32) for x in p0]
    P, M, V, E, c, info = OO.step([x.numpy() for x in p0], [named_p[n].grad.reshape(-1).cpu().numpy() for n in trainable], z, z,
                                  [x.numpy() for x in p0], OO.Counters(), lr=1e-4, update_every=1)
    assert info["action"] == "copy" and not info["skip"]
    got = lambda named: [[named[n].detach().reshape(-1) for n in trainable]]  # noqa: E731
    d_hip, d_torch = _distances(got(named_f), [P])[0], _distances(got(named_p), [P])[0]
    print(f"model step: p: d_hip {d_hip:.3f}  d_torch {d_torch:.3f}")
    _record("model_step", d_hip={"p": d_hip}, d_torch={"p": d_torch})
    assert d_hip <= 2 * d_torch + 1
    ema_named = dict(tf.ema.ema_model.named_parameters())
    for n in trainable:
        assert torch.equal(ema_named[n], named_f[n]), n  # counter 0: a copy
    assert int(tf.ema.step) == 1 and tf.optimizer.counters()["applied"] == 1
    for m in (tf.model, tf.ema.ema_model):  # the invalidate_engine() hook: sampling reads the stepped weights
        fresh = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type="l1")
        fresh.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=False)
        fresh = fresh.cuda()
        fresh.num_timesteps = m.num_timesteps = S
        assert torch.equal(m.sample(xs, cm, noise=noise), fresh.sample(xs, cm, noise=noise))
