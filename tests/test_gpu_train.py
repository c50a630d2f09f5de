"""The HIP training step (egoego_train_*, egoego_release_amd/train.py) on the GPU: loss and gradients against the fp64 oracle of
tests/train_oracle.py, the run-to-run and batch-composition properties, the dropout masks, and a short training run against the
plain-PyTorch path.

The gradient bar, per parameter tensor p, is computed on the CPU for the same inputs and the same forced ReLU masks and l1 signs:
    e_hip(p) <= 2 * (e_emul(p) + e_32(p)),     e(p) = |g(p) - g64(p)|_2 / |g64(p)|_2
e_emul: every product of the oracle as split-bf16 (forward and backward) with an exact accumulation; e_32: the oracle in fp32.  The
kernels carry both the operand rounding and an fp32 accumulation in another order, hence the sum; the factor 2 allows for another
realisation of the same roundings.  The w_k.bias gradients are identically zero in exact arithmetic (softmax does not see a shift
of all keys of a query) and are judged by |g_hip(p)| <= 1e-6 |g64|_global.

EGOEGO_TRAIN_RECORD=<file>: the measured e_hip / (e_emul + e_32) per tensor and the forward errors of every case are written there
as JSON (profiles/train_grad_error.json is such a file).
"""
import json
import math
import os

import pytest
import torch

import stream_cases as SC
import train_oracle as TO
from egoego_release_amd import ModelConfig, make_weights, _lib, train
from egoego_release_amd.model import CondGaussianDiffusion
from egoego_release_amd.synthetic import make_motion_windows, head_condition_mask

pytestmark = pytest.mark.gpu

D = 198
N_LAYERS = 4
_RECORD = {}


def _record(case, **kw):
    path = os.environ.get("EGOEGO_TRAIN_RECORD")
    if not path:
        return
    _RECORD.setdefault(case, {}).update(kw)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_RECORD, f, indent=1, sort_keys=True)


class Rig:
    """One module on the GPU with its training engine; sd = the CPU state dict it was loaded from."""

    def __init__(self, sd, max_timesteps, objective="pred_x0", loss_type="l1"):
        cfg = ModelConfig(max_timesteps=max_timesteps, objective=objective)
        self.model = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type=loss_type)
        self.model.load_state_dict(sd, strict=False)
        self.model = self.model.cuda()
        self.sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        self.engine = self.model._train_engine()
        self.tables = (self.model.sqrt_alphas_cumprod, self.model.sqrt_one_minus_alphas_cumprod, self.model.p2_loss_weight)
        self.tables_cpu = tuple(v.cpu() for v in self.tables)

    def tensors(self):
        return {n: p.detach() for n, p in self.model.denoise_fn.named_parameters()}

    def step(self, inp, objective="pred_x0", loss_type="l1", p_drop=0.0, seed=0, window_ids=None, saves=None, upstream=1.0, sel=None):
        """forward + backward on the engine -> (loss, out, grads {full name: tensor}, saves).  sel: the windows of `inp` to run."""
        x_start, noise, cond_noise, cond_mask, t, row_mask = [None if v is None else (v if sel is None else v[sel]).cuda() for v in inp]
        B, T, _ = x_start.shape
        ts = self.tensors()
        loss, out, saves = self.engine.forward(ts, x_start, noise, cond_noise, cond_mask, t, row_mask, *self.tables, objective=objective,
                                               loss_type=loss_type, p_drop=p_drop, seed=seed, window_ids=window_ids, saves=saves,
                                               want_out=True)
        up = torch.tensor(float(upstream), device="cuda")
        grads = self.engine.backward(ts, saves, up, B, T, p_drop, seed)
        return loss, out, {"denoise_fn." + k: v for k, v in grads.items()}, saves


_RIGS = {}


def rig(kind="init", objective="pred_x0", loss_type="l1"):
    key = (kind, objective, loss_type)
    if key not in _RIGS:
        if kind == "init":
            cfg = ModelConfig(max_timesteps=197)
            sd = make_weights(cfg, 0)
            _RIGS[key] = Rig(sd, 197, objective, loss_type)
        else:  # 50 Adam steps of the plain path on synthetic motion: weights that are no longer the initialisation
            import importlib.util
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            spec = importlib.util.spec_from_file_location("mtl", os.path.join(root, "tools", "make_trained_like_checkpoint.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            sd, _ = mod.train_like(steps=50, seed=0, device="cuda", T=40, batch=8, pool=64)
            _RIGS[key] = Rig(sd, 41, objective, loss_type)
    return _RIGS[key]


def inputs(B, T, lens, t, seed=0):
    """(x_start, noise, cond_noise, cond_mask, t, row_mask) on the CPU.  lens: valid frames per window (the time token counts as
    valid), or None for no row mask."""
    g = torch.Generator().manual_seed(1000 + seed)
    x_start = make_motion_windows(B, T, seed=seed + 5)
    noise = torch.randn(B, T, D, generator=g)
    cond_noise = torch.randn(B, T, D, generator=g)
    cond_mask = head_condition_mask((B, T, D))
    if t is None:
        t = torch.randint(0, 1000, (B,), generator=g)
    row_mask = None
    if lens is not None:
        row_mask = (torch.arange(T + 1)[None, :] <= torch.tensor(lens)[:, None]).float()
    return x_start, noise, cond_noise, cond_mask, torch.as_tensor(t).long(), row_mask


# name: (B, T, row-mask lengths, t)
CASES = {
    "a": (3, 11, [11, 5, 1], [0, 500, 999]),   # under one 32-row tile
    "b": (3, 40, [40, 20, 33], None),           # crosses a tile; B * L = 123 rows
    "c": (5, 31, None, None),                   # exactly one tile per window
    "d": (2, 120, [120, 30], None),             # the training window
    "e": (1, 196, None, None),                  # the longest window the engine accepts
    # B * L = 513 and 1025: one row past one and two chunks of the weight-gradient sum (TRAIN_GRAD_CHUNK = 512), at the shortest T
    "chunk1": (27, 18, None, None),
    "chunk2": (25, 40, None, None),
}


def check_parity(name, R, case, p_drop=0.0, objective="pred_x0", loss_type="l1"):
    B, T, lens, t = case
    inp = inputs(B, T, lens, t)
    seed = 4242
    loss, out, grads, saves = R.step(inp, objective, loss_type, p_drop, seed)
    eng = R.engine
    masks = None
    if p_drop > 0:
        masks = {(l, s): eng.dropout_mask(p_drop, seed, l, s, B, T).cpu() for l in range(N_LAYERS) for s in ("attn", "fc", "ffn")}
    hidden = [eng.saved(saves, B, T, l, "ffn_hidden").cpu() for l in range(N_LAYERS)]
    loss, out = float(loss.cpu()), out.cpu().double()
    grads = {k: v.cpu().double() for k, v in grads.items()}
    x_start, noise, cond_noise, cond_mask, tt, row_mask = inp
    kw = dict(row_mask=row_mask, objective=objective, loss_type=loss_type, p_drop=p_drop, drop_masks=masks)
    args = (x_start, noise, cond_noise, cond_mask, tt, R.tables_cpu)

    # ---- forward: fp64, nothing forced
    with torch.no_grad():
        r64 = TO.p_losses(TO.leaves(R.sd), *args, **kw)
    d_out = float((out - r64["out"]).abs().max())
    loss64 = float(r64["loss"])
    print(f"{name}: max|model_out - out64| = {d_out:.3e}   loss {loss:.8f} vs {loss64:.8f}")
    assert d_out <= 1e-3
    if loss_type == "l1":
        assert abs(loss - loss64) <= d_out
    else:
        assert abs(loss - loss64) <= 2 * float(r64["diff"].abs().max()) * d_out + d_out ** 2

    # ---- the kinks: every decision that differs from fp64 sits inside the forward error of its tensor; at most 1e-4 of them differ
    relu_masks, n_flip, n_all = [], 0, 0
    for l in range(N_LAYERS):
        pre, h = r64["ffn_pre"][l], hidden[l].double()
        on_hip, on_64 = h > 0, pre > 0
        both = on_hip & on_64
        err = float((h - pre)[both].abs().max())
        flip = on_hip != on_64
        if flip.any():
            assert float(pre[flip].abs().max()) <= err, (l, err)
        n_flip, n_all = n_flip + int(flip.sum()), n_all + flip.numel()
        relu_masks.append(on_hip)
    loss_sign = None
    target = x_start if objective == "pred_x0" else noise
    if loss_type == "l1":
        loss_sign = torch.sign(out.float() - target).double()  # fp32 subtraction, as the kernel does
        flip = loss_sign != torch.sign(r64["diff"])
        if flip.any():
            assert float(r64["diff"][flip].abs().max()) <= d_out
        n_flip, n_all = n_flip + int(flip.sum()), n_all + flip.numel()
    print(f"{name}: {n_flip} of {n_all} decisions differ from fp64")
    assert n_flip <= 1e-4 * n_all

    # ---- gradients with the HIP decisions forced: fp64, emulated split-bf16, fp32
    kw.update(relu_masks=relu_masks, loss_sign=loss_sign)
    _, g64 = TO.loss_and_grads(R.sd, *args, **kw)
    _, gem = TO.loss_and_grads(R.sd, *args, mm=TO.split_mm, **kw)
    _, g32 = TO.loss_and_grads(R.sd, *args, dtype=torch.float32, **kw)
    total = math.sqrt(sum(float(g.norm()) ** 2 for g in g64.values()))
    ratios, over = {}, []
    for k, ref in g64.items():
        g = grads[k].reshape(ref.shape)
        if k.endswith("w_k.bias"):
            ratios[k] = float(g.norm()) / total
            if not float(g.norm()) <= 1e-6 * total:
                over.append((k, ratios[k]))
            continue
        e_hip, e_em, e_32 = TO.rel_err(g, ref), TO.rel_err(gem[k], ref), TO.rel_err(g32[k], ref)
        ratios[k] = e_hip / (e_em + e_32)
        if not e_hip <= 2 * (e_em + e_32):
            over.append((k, e_hip, e_em, e_32))
    worst = sorted(((v, k) for k, v in ratios.items() if not k.endswith("w_k.bias")), reverse=True)[:3]
    print(f"{name}: worst e_hip / (e_emul + e_32): " + ", ".join(f"{k} {v:.2f}" for v, k in worst))
    _record(name, max_out_err=d_out, loss=loss, loss64=loss64, decisions_flipped=n_flip, decisions=n_all, ratios=ratios)
    assert not over, over


@pytest.fixture(scope="module", autouse=True)
def _drop_rigs():
    yield
    _RIGS.clear()


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_parity(name, p_drop):
    check_parity(f"{name} p={p_drop}", rig(), CASES[name], p_drop=p_drop)


@pytest.mark.parametrize("name", ["chunk1", "chunk2"])
def test_parity_past_a_gradient_chunk(name):
    B, T = CASES[name][:2]
    assert B * (T + 1) == (1 if name == "chunk1" else 2) * _lib.TRAIN_GRAD_CHUNK + 1
    check_parity(name, rig(), CASES[name])


@pytest.mark.parametrize("loss_type,objective", [("l2", "pred_x0"), ("l1", "pred_noise")])
def test_parity_other_loss_and_objective(loss_type, objective):
    check_parity(f"b {loss_type} {objective}", rig(), CASES["b"], loss_type=loss_type, objective=objective)


def test_parity_trained_like():
    check_parity("b trained-like", rig("trained"), CASES["b"], p_drop=0.1)


# ------------------------------------------------------------------------------------------------ properties
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def test_bitwise_repeatable_and_workspace_blind():
    """Two runs give the same bits, and so does a run whose workspace and saves held a NaN pattern on entry."""
    R = rig()
    B, T, lens, t = CASES["b"]
    inp = inputs(B, T, lens, t)
    l0, o0, g0, _ = R.step(inp, p_drop=0.1, seed=9)
    l1, o1, g1, _ = R.step(inp, p_drop=0.1, seed=9)
    assert torch.equal(l0, l1) and torch.equal(o0, o1) and _same(g0, g1)
    R.engine._ws.fill_(0xFF)
    saves = R.engine.new_saves(B, T).fill_(0xFF)
    l2, o2, g2, _ = R.step(inp, p_drop=0.1, seed=9, saves=saves)
    assert torch.isfinite(l2) and torch.equal(l0, l2) and torch.equal(o0, o2) and _same(g0, g2)
    l3, _, g3, _ = R.step(inp, p_drop=0.1, seed=10)
    assert not torch.equal(l0, l3)


def test_window_rows_do_not_depend_on_the_batch():
    R = rig()
    B, T, lens, t = CASES["b"]
    inp = inputs(B, T, lens, t)
    ids = [7, 3, 11]
    _, out, _, _ = R.step(inp, p_drop=0.1, seed=5, window_ids=ids)
    for b in range(B):
        _, alone, _, _ = R.step(inp, p_drop=0.1, seed=5, window_ids=ids[b:b + 1], sel=slice(b, b + 1))
        assert torch.equal(alone[0], out[b]), b
    _, pair, _, _ = R.step(inp, p_drop=0.1, seed=5, window_ids=[ids[2], ids[0]], sel=[2, 0])
    assert torch.equal(pair[0], out[2]) and torch.equal(pair[1], out[0])


def test_upstream_gradient_scales_exactly():
    R = rig()
    B, T, lens, t = CASES["a"]
    inp = inputs(B, T, lens, t)
    _, _, g1, _ = R.step(inp, p_drop=0.1, seed=1)
    _, _, g2, _ = R.step(inp, p_drop=0.1, seed=1, upstream=65536.0)
    for k in g1:
        assert torch.equal(g1[k] * 65536.0, g2[k]), k


def _module_inputs(B, T, seed):
    x = make_motion_windows(B, T, seed=seed).cuda()
    return x, head_condition_mask((B, T, D), device="cuda")


def test_two_graphs_outstanding_and_grad_scaling():
    """Two forwards, then two backwards in either order, accumulate what two sequential steps do; loss / 2 halves the gradients."""
    R = rig()
    m = R.model
    m.hip_training = True
    m.train()
    try:
        (x1, mask), (x2, _) = _module_inputs(3, 24, 1), _module_inputs(3, 24, 2)

        def grads():
            g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
            m.zero_grad(set_to_none=True)
            return g

        torch.manual_seed(3)
        la = m(x1, mask); la.backward(); lb = m(x2, mask); lb.backward()
        seq = grads()
        assert len(seq) == 72
        for order in ((0, 1), (1, 0)):
            torch.manual_seed(3)
            ls = [m(x1, mask), m(x2, mask)]
            assert torch.equal(ls[0], la) and torch.equal(ls[1], lb)
            for i in order:
                ls[i].backward()
            assert _same(seq, grads()), order
        assert seq["denoise_fn.motion_transformer.start_conv.weight"].shape == (512, 396, 1)
        torch.manual_seed(3)
        (m(x1, mask) / 2).backward()
        half = grads()
        torch.manual_seed(3)
        m(x1, mask).backward()
        full = grads()
        assert all(torch.equal(half[k] * 2, full[k]) for k in full)
    finally:
        m.hip_training = False
        m.zero_grad(set_to_none=True)


def test_optimizer_step_is_seen_and_eval_mode_has_no_dropout():
    cfg = ModelConfig(max_timesteps=25)
    R = Rig(make_weights(cfg, 1), 25)
    m = R.model
    m.hip_training = True
    x, mask = _module_inputs(4, 24, 3)
    draws = {"x_T": torch.randn(1, 24, D, generator=torch.Generator().manual_seed(1)).cuda(),
             "cond": torch.randn(1, 24, D, generator=torch.Generator().manual_seed(2)).cuda()}
    s0 = m.ddim_sample(x[:1], mask[:1], n_steps=2, noise=draws)  # packs the sampler's copy of the initial weights
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    m.denoise_fn.eval()
    torch.manual_seed(0)
    l0 = m(x, mask)
    l0.backward()
    opt.step()
    torch.manual_seed(0)
    l1 = m(x, mask)
    assert float(l1.detach()) < float(l0.detach())  # one SGD step on the same draws
    fresh = Rig({k: v.detach().cpu() for k, v in m.state_dict().items()}, 25)
    fresh.model.hip_training = True
    fresh.model.denoise_fn.eval()
    torch.manual_seed(0)
    assert torch.equal(fresh.model(x, mask), l1)  # no stale copy of the old weights anywhere
    # eval mode is the p_drop = 0 call: the engine gives the same bits for the same draws
    torch.manual_seed(0)
    t = torch.randint(0, 1000, (4,), device="cuda").long()
    noise, cond_noise = torch.randn_like(x), torch.randn_like(x)
    le, _, _ = fresh.engine.forward(fresh.tensors(), x, noise, cond_noise, mask, t, None, *fresh.tables, p_drop=0.0, seed=123)
    assert torch.equal(le, l1)
    m.denoise_fn.train()
    torch.manual_seed(0)
    assert not torch.equal(m(x, mask), l1)  # dropout on
    # the sampler re-packs by its fingerprint rule: it samples from the stepped weights, like a module loaded from them
    s1 = m.ddim_sample(x[:1], mask[:1], n_steps=2, noise=draws)
    assert not torch.equal(s0, s1)
    assert torch.equal(s1, fresh.model.ddim_sample(x[:1], mask[:1], n_steps=2, noise=draws))


def test_streams():
    R = rig()
    B, T, lens, t = CASES["b"]
    x_start, noise, cond_noise, cond_mask, tt, row_mask = [v.cuda() for v in inputs(B, T, lens, t)]

    def call(xs, nz, cn):
        loss, out, grads, _ = R.step((xs, nz, cn, cond_mask, tt, row_mask), p_drop=0.1, seed=2)
        return [loss, out] + [grads[k] for k in sorted(grads)]

    true = [x_start, noise, cond_noise]
    call(*true)
    delay = SC.Delay().calibrate({"train step": lambda: call(*true)})
    SC.check("egoego_train_forward + egoego_train_backward", SC.ENQUEUES, call, true, torch.cuda.Stream(), delay)


# ------------------------------------------------------------------------------------------------ dropout masks
def test_dropout_masks():
    R = rig()
    eng = R.engine
    B, T, p = 3, 40, 0.1
    L = T + 1
    ids = [5, 900, 2 ** 40 + 1]
    got = {}
    for layer, site, seed in ((0, "attn", 1), (0, "fc", 1), (0, "ffn", 1), (3, "fc", 1), (0, "fc", 2)):
        m = eng.dropout_mask(p, seed, layer, site, B, T, window_ids=ids).cpu()
        assert m.shape == ((B, 4, L, L) if site == "attn" else (B, L, 512))
        n = m[0].numel()
        for b in range(B):
            kept = float(m[b].float().mean())
            assert abs(kept - 0.9) <= 4 * math.sqrt(0.09 / n), (layer, site, seed, b, kept)
            alone = eng.dropout_mask(p, seed, layer, site, 1, T, window_ids=ids[b:b + 1]).cpu()
            assert torch.equal(alone[0], m[b])
        got[(layer, site, seed)] = m
    # any two masks (another layer, site, window or seed) agree like independent draws: 0.9^2 + 0.1^2 = 0.82
    pairs = [(got[(0, "fc", 1)][0], got[(0, "ffn", 1)][0]), (got[(0, "fc", 1)][0], got[(3, "fc", 1)][0]),
             (got[(0, "fc", 1)][0], got[(0, "fc", 2)][0]), (got[(0, "fc", 1)][0], got[(0, "fc", 1)][1]),
             (got[(0, "attn", 1)][0], got[(0, "attn", 1)][2]), (got[(0, "attn", 1)][0].flatten(), got[(0, "fc", 1)][0].flatten()[:4 * L * L])]
    for i, (a, b) in enumerate(pairs):
        agree = float((a == b).float().mean())
        assert abs(agree - 0.82) <= 4 * math.sqrt(0.82 * 0.18 / a.numel()), (i, agree)
    # window b of a call without ids draws the stream of id b
    assert torch.equal(eng.dropout_mask(p, 1, 0, "fc", 2, T).cpu()[1], eng.dropout_mask(p, 1, 0, "fc", 1, T, window_ids=[1]).cpu()[0])
    assert bool(eng.dropout_mask(0.0, 1, 0, "fc", B, T).all())  # p = 0: every value kept, unscaled


# ------------------------------------------------------------------------------------------------ training
def _train(hip, seed, steps=150, B=8, T=24, lr=2e-4):
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(make_weights(cfg, 0), strict=False)
    m = m.cuda()
    m.hip_training = hip
    m.train()
    data = make_motion_windows(64, T, seed=1, device="cuda")
    mask = head_condition_mask((B, T, D), device="cuda")
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(seed)
    losses = []
    for it in range(steps):
        idx = torch.randint(0, 64, (B,), generator=g).cuda()
        loss = m(data[idx], mask)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    first = last = None
    for v in losses[:20]:
        first = v if first is None else 0.9 * first + 0.1 * v
    for v in losses[-50:]:
        last = v if last is None else 0.9 * last + 0.1 * v
    return first, last


def test_training_run_matches_the_plain_path():
    """150 Adam steps: the HIP path ends inside the plain path's spread over three dropout seeds, widened by that spread."""
    plain = [_train(False, s) for s in (1, 2, 3)]
    lo, hi = min(p[1] for p in plain), max(p[1] for p in plain)
    first, last = _train(True, 1)
    print(f"plain path: final smoothed loss in [{lo:.4f}, {hi:.4f}] (first {plain[0][0]:.4f}); HIP path {last:.4f} (first {first:.4f})")
    _record("training", plain_lo=lo, plain_hi=hi, hip=last, hip_first=first)
    assert all(p[1] < p[0] for p in plain) and last < first
    assert lo - (hi - lo) <= last <= hi + (hi - lo)
