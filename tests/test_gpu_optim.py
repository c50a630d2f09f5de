"""The fused parameter update on the GPU (csrc/optim_step.*, egoego_release_amd/optim.py) against the fp64 oracle of
tests/optim_oracle.py, on tensor lists unless a test says otherwise.

The bar of every comparison with the oracle: for each of p, exp_avg, exp_avg_sq and ema, d = the largest distance from the oracle
in units of the oracle value's fp32 ulp; d_torch is the same figure for torch.optim.Adam(foreach=False) and the three-line lerp on
the CPU from the same fp32 inputs; d_hip <= 2 d_torch + 1.  Both evaluate the same few-rounding formula; FMA contraction and the
device's fp64 scalars change the order of the roundings, so neither bounds the other element by element.  The maximum is set by
a handful of elements that cancel; d99, the 99th percentile of the same distances over all elements of a kind, is held in the same
form beside it: d99_hip <= 2 d99_torch + 1.

Every view sits between GUARD zeros on both sides inside its buffer; after a step the guards of all five buffers are still zero.

EGOEGO_OPTIM_RECORD=<file>: the measured d and d99 values are written there as JSON (profiles/optim_error.json is such a file).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import optim_oracle as OO
import stream_cases as SC
import trainer_cases as TC
from egoego_release_amd import _lib, optim

pytestmark = pytest.mark.gpu

CH = _lib.OPTIM_CHUNK
# (elements, element offset of p / g / m / v / ema inside a larger buffer)
SPECS = [(1, (0, 0, 0, 0, 0)), (3, (0, 0, 0, 0, 0)), (198, (1, 0, 0, 0, 0)),  # a view one element in: phases differ, scalars throughout
         (CH - 1, (0, 0, 0, 0, 0)), (CH, (0, 0, 0, 0, 0)), (CH + 1, (1, 1, 1, 1, 1)),  # one phase, off the boundary: head, body, tail
         (2 * CH + 5, (0, 0, 0, 0, 0)), (37, (0, 0, 0, 0, 0))]  # the last one: zero gradient, zero moments
ZERO = len(SPECS) - 1
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.0)
DECAYED = HYPER[:4] + (0.01,)
GUARD = 4  # zeros on both sides of every view (a multiple of 4: the 16-byte phase of a view is its SPECS offset)
# The 16-byte phases 2 and 3: apply_kernel's scalar head is (4 - phase) & 3 = 2 and 1 elements.  Count 1 at phase 2 is shorter than
# its head, and so is count 1 with any head.  The last two: p, g, m, v at phase 3 and ema at phase 0 — scalars throughout.
PHASE_SPECS = ([(n, (2,) * 5) for n in (1, 2, 3, 6, CH + 2)] + [(n, (3,) * 5) for n in (1, 2, 3, 6, CH + 2)]
               + [(6, (3, 3, 3, 3, 0)), (CH + 2, (3, 3, 3, 3, 0))])
KINDS = ("p", "exp_avg", "exp_avg_sq", "ema")
_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_OPTIM_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


def _inputs(seed=0, warm=3, away=0.0, sizes=None, zero=ZERO):
    """fp32 CPU lists p, g, m, v, ema: p ~ N(0, 0.05) with some exact zeros, g = N(0, 1) * 10^U(-6, 0), moments from `warm`
    oracle steps on other gradients (rounded to fp32), ema = p moved a little.  away > 0: no zeros, and every |p| >= away.
    sizes: the element counts (default: those of SPECS); zero: the tensor that never sees a gradient, or None."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [n for n, _ in SPECS] if sizes is None else list(sizes)

    def grads():
        out = [torch.randn(n, generator=gen) * 10.0 ** (-6 * torch.rand(n, generator=gen)) for n in sizes]
        if zero is not None:
            out[zero] = torch.zeros(sizes[zero])
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


def _views(lists, specs=None):
    """The five CPU lists on the device, each tensor a view at its `specs` offset (SPECS by default) into a buffer of its own, with
    GUARD zeros on both sides -> (the five lists of views, [(buffer, first element of the view, elements)] over all of them)."""
    out, guards = [], []
    for which, lst in enumerate(lists):
        dev = []
        for (n, offs), t in zip(SPECS if specs is None else specs, lst):
            first = GUARD + offs[which]
            buf = torch.zeros(first + n + GUARD, device="cuda")
            view = buf[first:first + n]
            assert ((view.data_ptr() >> 2) & 3) == (offs[which] & 3)  # (the allocator's blocks are 16-byte aligned and more)
            view.copy_(t)
            dev.append(view)
            guards.append((buf, first, n))
        out.append(dev)
    return out, guards


def _flat_views(lists, lead=(0, 0, 0, 0, 1)):
    """The five CPU lists on the device as consecutive views of five flat buffers: the phases of the tensors vary with the counts
    before them, and the `ema` buffer's one leading element sets its phases one off the other four."""
    out, guards = [], []
    for which, lst in enumerate(lists):
        total = sum(t.numel() for t in lst)
        first = GUARD + lead[which]
        buf = torch.zeros(first + total + GUARD, device="cuda")
        buf[first:first + total].copy_(torch.cat(lst))
        dev, at = [], first
        for t in lst:
            dev.append(buf[at:at + t.numel()])
            at += t.numel()
        out.append(dev)
        guards.append((buf, first, total))
    return out, guards


class Rig:
    """One UpdateEngine over SPECS (or `specs`; or `flat`, a list of counts laid out by _flat_views) with device lists p, g, m, v,
    ema and the EMA's two counters.  hyper: (lr, beta1, beta2, eps, weight_decay) of step() and oracle() unless a call overrides it."""

    def __init__(self, seed=0, ema_step=120, initted=1.0, away=0.0, specs=None, flat=None, hyper=HYPER, **sched):
        self.specs, self.hyper = SPECS if specs is None else specs, hyper
        self.sizes = [n for n, _ in self.specs] if flat is None else list(flat)
        self.cpu = _inputs(seed, away=away, sizes=self.sizes, zero=ZERO if specs is None and flat is None else None)
        (self.p, self.g, self.m, self.v, self.e), self.guards = _views(self.cpu[:5], self.specs) if flat is None else _flat_views(self.cpu[:5])
        # what the comparisons read: the lists themselves, or (flat) each buffer's whole range as one tensor and the CPU lists joined
        self.ref, self.whole = self.cpu[:5], (self.p, self.g, self.m, self.v, self.e)
        if flat is not None:
            self.ref = tuple([torch.cat(lst)] for lst in self.cpu[:5])
            self.whole = tuple([buf[first:first + n]] for buf, first, n in self.guards)
        self.eng = optim.UpdateEngine(self.sizes, "cuda")
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

    def step(self, ema=True, hyper=None, **kw):
        self.eng.step(self.hyper if hyper is None else hyper, self.sched() if ema else None, **kw)

    def guards_clean(self):
        """No element outside a view has been written: every buffer is still zero before and behind its view(s)."""
        return not any(bool(buf[:first].any()) or bool(buf[first + n:].any()) for buf, first, n in self.guards)

    def out(self):
        """The device's p, exp_avg, exp_avg_sq and ema as the comparisons read them."""
        return (self.whole[0], self.whole[2], self.whole[3], self.whole[4])

    def tensors(self):
        return [t for lst in self.out() for t in lst]

    def snapshot(self):
        return [t.clone() for t in self.tensors() + self.whole[1] + [self.ema_step, self.initted, self.eng.state[:_lib.OptimState.total_norm.offset]]]

    def restore(self, snap=None):
        snap = self.start if snap is None else snap
        for t, s in zip(self.tensors() + self.whole[1] + [self.ema_step, self.initted, self.eng.state[:_lib.OptimState.total_norm.offset]], snap):
            t.copy_(s)

    def counters(self):
        st = self.eng.read_state()
        return (st["adam_step"], int(self.ema_step), int(float(self.initted)), st["applied"], st["skipped"])

    def oracle(self, c, lists=None, hyper=None, **kw):
        p, g, m, v, e = lists if lists is not None else self.ref
        k, h = dict(self.sched_kw), self.hyper if hyper is None else hyper
        return OO.step([x.numpy() for x in p], [x.numpy() for x in g], [x.numpy() for x in m], [x.numpy() for x in v],
                       [x.numpy() for x in e], c, lr=h[0], betas=h[1:3], eps=h[3], weight_decay=h[4], **k, **kw)

    def set_counters(self, adam_step=None, ema_step=None, initted=None):
        """After restore(): other counter values than the rig started with."""
        if adam_step is not None:
            self.eng.adam_step.fill_(adam_step)
        if ema_step is not None:
            self.ema_step.fill_(ema_step)
        if initted is not None:
            self.initted.fill_(float(initted))

    def check_step(self, case, c0, lists=None, hyper=None, **sched):
        """One step (Adam + EMA, the gradients left in place) from counters c0 under `hyper` and the schedule values `sched`,
        against the oracle: the counters, the EMA action, the bar on all four outputs, the guards -> (oracle info, state header,
        the oracle's P, M, V, E).  lists: the fp32 CPU state the device holds when it differs from self.cpu."""
        saved = dict(self.sched_kw)
        self.sched_kw.update(sched)
        try:
            self.set_counters(c0.adam_step, c0.ema_step, c0.initted)
            self.step(hyper=hyper)
            P, M, V, E, c1, info = self.oracle(c0, lists, hyper)
        finally:
            self.sched_kw = saved
        assert not info["skip"] and self.counters() == c1.as_tuple(), (case, self.counters(), c1.as_tuple())
        st = self.eng.read_state()
        assert st["ema_action"] == {"none": _lib.OPTIM_EMA_NONE, "copy": _lib.OPTIM_EMA_COPY, "lerp": _lib.OPTIM_EMA_LERP}[info["action"]], case
        h = self.hyper if hyper is None else hyper
        cpu = lists if lists is not None else self.ref
        tor = _torch_step(*cpu, c0.adam_step, info["decay"] if info["action"] == "lerp" else info["action"], h)
        _hold(case, self.out(), tor, (P, M, V, E))
        assert self.guards_clean(), case
        return info, st, (P, M, V, E)


def _bits(ts):
    return [t.detach().cpu().clone() for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _torch_step(p, g, m, v, e, adam_step, decay, hyper=HYPER):
    """torch.optim.Adam(foreach=False) and ema-pytorch's lerp on the CPU from fp32 lists (decay None or "none": the EMA is left
    alone; "copy": it takes the stepped parameters)."""
    params = [torch.nn.Parameter(x.clone()) for x in p]
    opt = torch.optim.Adam(params, lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4], foreach=False)
    for q, gg, mm, vv in zip(params, g, m, v):
        q.grad = gg.clone()
        opt.state[q] = {"step": torch.tensor(float(adam_step)), "exp_avg": mm.clone(), "exp_avg_sq": vv.clone()}
    opt.step()
    ema = [x.clone() for x in e]
    if decay == "copy":
        ema = [q.detach().clone() for q in params]
    elif decay is not None and decay != "none":
        for x, q in zip(ema, params):
            difference = x - q.data
            difference.mul_(1.0 - decay)
            x.sub_(difference)
    return ([q.detach() for q in params], [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params], ema)


def _distances(got, want):
    """The four d values (p, m, v, ema) of lists-of-lists `got` against the oracle's fp64 lists."""
    return [max(OO.ulp_distance(x.detach().cpu().numpy(), w) for x, w in zip(a, b)) for a, b in zip(got, want)]


def _d99(got, want):
    """The 99th percentile of the same distances, over all elements of each kind."""
    return [float(np.percentile(np.concatenate([OO.ulp_distances(x.detach().cpu().numpy(), w).reshape(-1) for x, w in zip(a, b)]), 99))
            for a, b in zip(got, want)]


def _hold(case, got, tor, want):
    """The bar: `got` (the device's p, m, v, ema lists) and `tor` (torch's) against the oracle's `want`, maximum and d99."""
    d_hip, d_torch, q_hip, q_torch = _distances(got, want), _distances(tor, want), _d99(got, want), _d99(tor, want)
    for name, h, t, qh, qt in zip(KINDS, d_hip, d_torch, q_hip, q_torch):
        print(f"{case}: {name}: d_hip {h:.3f}  d_torch {t:.3f}  d99_hip {qh:.3f}  d99_torch {qt:.3f}")
    _record(case, d_hip=dict(zip(KINDS, d_hip)), d_torch=dict(zip(KINDS, d_torch)), d99_hip=dict(zip(KINDS, q_hip)), d99_torch=dict(zip(KINDS, q_torch)))
    for name, h, t, qh, qt in zip(KINDS, d_hip, d_torch, q_hip, q_torch):
        assert h <= 2 * t + 1, (case, name, h, t)
        assert qh <= 2 * qt + 1, (case, name, "d99", qh, qt)


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
    _hold("one_step", (rig.p, rig.m, rig.v, rig.e), tor, (P, M, V, E))
    assert _same_bits(_bits([rig.p[ZERO]]), [p0[ZERO]])
    assert not rig.m[ZERO].any() and not rig.v[ZERO].any()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(rig.g, rig.cpu[1]))  # zero_grads off: the gradients stay
    assert rig.guards_clean()


def test_one_step_with_weight_decay_moves_the_tensor_without_a_gradient():
    """The same inputs and sizes at weight_decay = 0.01 (the L2 form: g + wd p enters both moments).  In the tensor with zero
    gradient and zero moments the decay is the whole gradient: where p != 0 the parameter moves and both moments become non-zero;
    where p == 0 exactly, p, exp_avg and exp_avg_sq keep their bits."""
    r = Rig(hyper=DECAYED)
    assert not r.g[ZERO].any() and not r.m[ZERO].any() and not r.v[ZERO].any()
    before = [_bits([x[ZERO]])[0] for x in (r.p, r.m, r.v)]
    c0 = OO.Counters(adam_step=r.cpu[5], ema_step=120, initted=True)
    info, st, _ = r.check_step("one_step_weight_decay", c0)
    assert info["action"] == "lerp" and st["last_skip"] == 0
    after = [_bits([x[ZERO]])[0] for x in (r.p, r.m, r.v)]
    at_zero = before[0] == 0
    assert bool(at_zero.any()) and bool((~at_zero).any())
    for b, a in zip(before, after):
        assert torch.equal(b[at_zero].view(torch.int32), a[at_zero].view(torch.int32))
    assert bool((after[0][~at_zero] != before[0][~at_zero]).all())
    assert bool((after[1][~at_zero] != 0).all()) and bool((after[2][~at_zero] > 0).all())


def _free_run(r, steps, seed, hyper=HYPER):
    """`steps` steps on fresh gradients, the device against the oracle (fp64 state) and torch (fp32 state).  Exact on the way: ema
    has p's bits on a copy step and its own on a step that leaves it alone; the counters are the oracle's.  -> (the actions seen,
    the oracle's counters, the device's lists, torch's lists, the oracle's lists)."""
    gen = torch.Generator().manual_seed(seed)
    cur = [[x.clone() for x in lst] for lst in r.cpu[:5]]  # the torch side's fp32 state
    O = [[x.numpy().astype(np.float64) for x in lst] for lst in r.cpu[:5]]  # the oracle's fp64 state
    c, adam_step = OO.Counters(adam_step=r.cpu[5], ema_step=int(r.ema_step), initted=bool(float(r.initted))), r.cpu[5]
    seen = set()
    for k in range(steps):
        g = [torch.randn(n, generator=gen) * 10.0 ** (-6 * torch.rand(n, generator=gen)) for n in r.sizes]
        for d, s in zip(r.g, g):
            d.copy_(s)
        before = _bits(r.e)
        r.step(hyper=hyper)
        P, M, V, E, c, info = OO.step(O[0], [x.numpy() for x in g], O[2], O[3], O[4], c, lr=hyper[0], betas=hyper[1:3], eps=hyper[3],
                                      weight_decay=hyper[4], **r.sched_kw)
        O = [P, None, M, V, E]
        seen.add(info["action"])
        tor = _torch_step(cur[0], g, cur[2], cur[3], cur[4], adam_step, info["decay"], hyper)
        if info["action"] == "copy":
            tor = tor[:3] + ([x.clone() for x in tor[0]],)
            assert _same_bits(_bits(r.e), _bits(r.p)), k
        elif info["action"] == "none":
            assert _same_bits(_bits(r.e), before), k
        cur = [tor[0], None, tor[1], tor[2], tor[3]]
        adam_step += 1
        assert r.counters() == c.as_tuple(), k
    assert r.guards_clean()
    return seen, c, (r.p, r.m, r.v, r.e), (cur[0], cur[2], cur[3], cur[4]), (O[0], O[2], O[3], O[4])


def test_five_free_running_steps_with_weight_decay():
    """weight_decay = 0.01 carried through fp32 state, parameters held away from zero (see the next test); update_every = 1 and
    update_after_step = 0: an EMA update on every step — a copy, the copy that sets `initted`, then three lerps."""
    r = Rig(seed=2, ema_step=0, initted=0.0, away=0.05, hyper=DECAYED, update_every=1, update_after_step=0)
    seen, c, got, tor, want = _free_run(r, 5, 11, DECAYED)
    assert seen == {"copy", "lerp"} and c.initted and c.ema_step == 5
    _hold("free_running_5_weight_decay", got, tor, want)


def test_twenty_five_free_running_steps():
    """update_every = 3, update_after_step = 4: the copy phase, the first call past it, the steady lerp.  Exact on the way: ema
    has p's bits on a copy step and its own on the steps in between; the counters are the oracle's.  At the end: the bar.

    The oracle carries fp64 state through the run, the device and torch fp32 state.  The bar counts in ulps of the oracle's
    value, so it says nothing about a parameter that passes zero on the way: any fp32 run, torch's included, is then thousands of
    ulps of that value away, by an amount that is chance (with the one-step test's inputs: p 7300 on the device, 3157 for torch,
    both at the same element).  28 steps of at most lr = 1e-3 each move a parameter by at most 0.028, so every |p| starts at 0.05
    or more.  exp_avg mixes signs whatever the inputs; its distances are large and come out equal on both sides."""
    r = Rig(seed=1, ema_step=0, initted=0.0, away=0.05, update_every=3, update_after_step=4)
    seen, c, got, tor, want = _free_run(r, 25, 9)
    assert seen == {"copy", "none", "lerp"} and c.initted and c.ema_step == 25
    _hold("free_running_25", got, tor, want)


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


# ---------------------------------------------------------------------------------------------------------------- phases, many chunks
def test_one_step_at_the_16_byte_phases_2_and_3():
    """PHASE_SPECS: heads of 2 and of 1 elements, tensors shorter than their head, and an EMA tensor alone off the others' phase.
    Adam, the lerp and the gradient's zeros; a vector store over the edge of a view would land in a guard."""
    r = Rig(seed=4, specs=PHASE_SPECS)
    c0 = OO.Counters(adam_step=r.cpu[5], ema_step=120, initted=True)
    info, _, _ = r.check_step("phases_2_3", c0)
    assert info["action"] == "lerp"
    r.restore()
    r.step(zero_grads=True)
    assert not any(bool(g.any()) for g in r.g) and r.guards_clean()


# apply_kernel's grid is at most op::MAX_BLOCKS = 2048 workgroups (csrc/optim_step.h): above that a workgroup strides to further chunks
MAX_BLOCKS = 2048
N_MANY = 2 * MAX_BLOCKS + 37
MANY = [(1, 2, 3, 4, 5, 7)[i % 6] for i in range(N_MANY)]
MANY[0], MANY[16], MANY[N_MANY - 1] = CH + 1, 2 * CH, CH - 1


@pytest.fixture(scope="module")
def many():
    return Rig(seed=6, flat=MANY, away=0.01)  # (_inputs' zeros sit at every tensor's first element: no place for them here)


def test_thousands_of_chunks_from_tiny_tensors(many):
    """N = 2 * 2048 + 37 tensors of 1 .. 7 elements and three of about a chunk or two, consecutive views of five flat buffers (the
    EMA's one element off): more chunks than two grids of apply_kernel, more than 256 * 16 partials in decide_kernel, 259 table
    launches, every phase and mismatches.  Every element against the oracle; the norm; the gradients' zeros."""
    r = many
    n_chunks = sum((n + CH - 1) // CH for n in MANY)
    assert n_chunks > 2 * MAX_BLOCKS and len(MANY) == N_MANY and 30000 < sum(MANY) < 45000
    r.restore()
    c0 = OO.Counters(adam_step=r.cpu[5], ema_step=120, initted=True)
    P, M, V, E, c1, info = r.oracle(c0)
    r.step(zero_grads=True)
    assert info["action"] == "lerp" and r.counters() == c1.as_tuple()
    _hold("many_chunks", r.out(), _torch_step(*r.ref, r.cpu[5], info["decay"]), (P, M, V, E))
    st = r.eng.read_state()
    want = float(np.sqrt(sum(np.sum(x.numpy().astype(np.float64) ** 2) for x in r.cpu[1])))
    assert abs(st["total_norm"] - want) <= sum(MANY) * 2.0 ** -53 * want
    assert not any(bool(g.any()) for g in r.g) and r.guards_clean()


def test_thousands_of_chunks_skip_on_a_nan_in_the_last_one_element_tensor(many):
    r = many
    last_one = max(i for i, n in enumerate(MANY) if n == 1)
    assert last_one > 2 * MAX_BLOCKS
    r.restore()
    r.g[last_one][0] = float("nan")
    before, c0 = _bits(r.tensors()), r.counters()
    r.step(zero_grads=True)
    assert _same_bits(_bits(r.tensors()), before)
    assert r.counters() == c0[:4] + (c0[4] + 1,) and int(r.eng.last_skipped) == 1
    assert not any(bool(g.any()) for g in r.g) and r.guards_clean()


@pytest.mark.parametrize("n", [16, 17, 32, 33])
def test_one_element_tensors_at_the_table_batch_boundaries(n):
    """egoego_optim_set_tensors uploads 16 table entries per launch: one and two full launches, and each with one entry more."""
    r = Rig(seed=n, flat=[1] * n, away=0.01)
    c0 = OO.Counters(adam_step=r.cpu[5], ema_step=120, initted=True)
    info, _, _ = r.check_step(f"table_{n}", c0)
    assert info["action"] == "lerp"


# ---------------------------------------------------------------------------------------------------------------- other regimes
def test_the_schedules_other_regimes(rig):
    """The decay a long run holds (beta), the min_value clamp, the copy at step == update_after_step that leaves `initted` alone,
    the first call past it that sets it, and update_every = 1.  The expected actions and decays are the oracle's."""
    assert OO.decay_at(100001) == 0.995 and OO.decay_at(111, min_value=0.9) == 0.9
    assert OO.ema_action(100, False) == "copy" and OO.ema_action(110, False) == "copy"
    k = rig.cpu[5]
    rig.restore()
    info, st, _ = rig.check_step("ema_at_beta", OO.Counters(k, 100000, True))
    assert info["action"] == "lerp" and info["decay"] == 0.995 and st["one_minus_decay"] == pytest.approx(0.005, rel=1.2e-7)
    rig.restore()
    info, st, _ = rig.check_step("ema_min_value", OO.Counters(k, 110, True), min_value=0.9)
    assert info["action"] == "lerp" and info["decay"] == 0.9 and st["one_minus_decay"] == pytest.approx(0.1, rel=1.2e-7)
    rig.restore()
    info, _, _ = rig.check_step("ema_copy_at_update_after_step", OO.Counters(k, 100, False), update_after_step=100, update_every=10)
    assert info["action"] == "copy" and rig.counters()[1:3] == (101, 0) and _same_bits(_bits(rig.e), _bits(rig.p))
    rig.restore()
    info, _, _ = rig.check_step("ema_first_past", OO.Counters(k, 110, False))
    assert info["action"] == "copy" and rig.counters()[1:3] == (111, 1) and _same_bits(_bits(rig.e), _bits(rig.p))
    for s in (121, 122):  # no multiple of 10: with update_every = 1 both lerp
        rig.restore()
        info, _, _ = rig.check_step(f"ema_every_step_{s}", OO.Counters(k, s, True), update_every=1)
        assert info["action"] == "lerp"
    rig.restore()
    rig.set_counters(ema_step=121)
    before = _bits(rig.e)
    rig.step()  # the rig's own update_every = 10: counter 121 leaves the EMA alone
    assert _same_bits(_bits(rig.e), before) and rig.eng.read_state()["ema_action"] == _lib.OPTIM_EMA_NONE


def test_adams_other_regimes():
    """A late step (beta^k underflows: both bias corrections are exactly 1), betas = (0, 0), and a changed lr between two steps.

    Every |p| starts at 0.05 or more.  The bar counts in ulps of the oracle's value, and a parameter that lands next to zero is
    thousands of such ulps off on any fp32 run, by an amount that is chance (see the 25-step test).  One step moves a parameter by
    at most step_size |m| / (sqrt(v) bc2) <= lr (1 - beta1) / sqrt(1 - beta2) = 3.2e-3 without the bias corrections, and by at
    most lr with betas = (0, 0): none gets near zero from 0.05."""
    rig = Rig(seed=3, away=0.05)
    lr = HYPER[0]
    rig.restore()
    _, st, _ = rig.check_step("adam_step_1e6", OO.Counters(10 ** 6, 120, True))
    assert st["adam_step"] == 10 ** 6 + 1 and st["step_size"] == pytest.approx(lr, rel=1e-6) and st["bc2_sqrt"] == 1.0
    # betas = (0, 0): exp_avg is the gradient itself and exp_avg_sq its square, whatever the moments held
    rig.restore()
    rig.check_step("betas_zero", OO.Counters(rig.cpu[5], 120, True), hyper=(lr, 0.0, 0.0, 1e-8, 0.0))
    assert _same_bits(_bits(rig.m), rig.cpu[1])
    # lr = 1e-3, then lr = 0 from the state the first step left: p keeps its bits, the moments and the counter move on
    rig.restore()
    rig.check_step("lr_first", OO.Counters(rig.cpu[5], 120, True))
    mid = [_bits(x) for x in (rig.p, rig.g, rig.m, rig.v, rig.e)]
    _, st, _ = rig.check_step("lr_zero_second", OO.Counters(rig.cpu[5] + 1, 121, True, applied=1), lists=mid, hyper=(0.0,) + HYPER[1:])
    assert st["step_size"] == 0.0 and st["adam_step"] == rig.cpu[5] + 2
    assert _same_bits(_bits(rig.p), mid[0])
    for now, then in ((rig.m, mid[2]), (rig.v, mid[3])):  # (the last tensor has no gradient and no moments: it stays)
        assert float((torch.cat(_bits(now)[:ZERO]) != torch.cat(then[:ZERO])).float().mean()) > 0.9


def test_a_skipped_replay_between_two_good_ones(rig):
    """One captured step (the linear chain of three launches, gradients left in place): a replay on good gradients, one with a NaN
    written into a gradient element — nothing changes but `skipped` — and one with the element restored.  The bits of two eager
    steps; 2 applied, 1 skipped."""
    rig.restore()
    rig.step()
    rig.step()
    want, cw = _bits(rig.tensors()), rig.counters()
    rig.restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.step()
    rig.restore()
    c0 = rig.counters()
    graph.replay()
    torch.cuda.synchronize()
    mid, c1 = _bits(rig.tensors()), rig.counters()
    assert c1 == (c0[0] + 1, c0[1] + 1, c0[2], c0[3] + 1, c0[4])
    t, i = 5, CH  # the last element of the CHUNK + 1 tensor: a chunk of its own
    good = rig.g[t][i].clone()
    rig.g[t][i] = float("nan")
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(_bits(rig.tensors()), mid)
    assert rig.counters() == c1[:4] + (c1[4] + 1,) and int(rig.eng.last_skipped) == 1  # adam_step and the EMA counter stay
    rig.g[t][i] = good
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(_bits(rig.tensors()), want)
    assert rig.counters() == cw[:4] + (cw[4] + 1,) and (rig.counters()[3] - c0[3], rig.counters()[4] - c0[4]) == (2, 1)
    assert rig.guards_clean()


# ---------------------------------------------------------------------------------------------------------------- with the model
def _trainer(fused, tmp_path, seed=0):
    return TC.make_trainer(fused, tmp_path, seed, keep_grads=True)  # the test reads the gradients after the step


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
