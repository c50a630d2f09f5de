"""Attention where softmax is sharp, shifted, or aimed at masked keys (tests/planted_attention.py: layer-0 logits known exactly).

Every attention form of the dispatch (the sixteen rows of attention_forms.FORMS, named by the kernels the launch sites record) runs
the four regimes (M, gamma, over_init) = (6, 0, no), (40, 0, yes), (200, 0, no), (40, -300, yes): a mixed row, a one-hot row on top of
the initialisation's logits, a one-hot row whose runner-up underflows, and a one-hot row 300 below zero (the row maximum must be the
true one).  The bars are the project's existing ones: POSE_TOL at the denoiser output, test_stagewise_against_oracle's at the stops.

What a stop is compared with.  Split-bf16: the exact fp64 restatement and the oracle's taps.  The int8 precisions: the restatement
of their own operand format (planted_attention.attention_i8: exact integers, no kernel) in every regime, because a one-hot row
hands one V row through unaveraged and the format alone moves that row by 3e-4 .. 4e-4 (7.6e-4 in the mixed regime) — the whole of
what the kernels show against the exact result; precision 9, whose bar is relative, also the exact restatement and the oracle's
taps in the one-hot regimes.  tests/test_planted_attention.py holds both to the CPU.  The int8 forms' ragged cases carry their
shift as planted_attention.I8_RAGGED_SHIFTED (why: there).  DESIGN.md 5b-4."""
import functools

import numpy as np
import pytest
import torch

import planted_attention as PA
import stage1_oracle as S1O
from egoego_release_amd import ModelConfig, _lib, stage1
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O
from test_gpu_dispatch import philox_noise
from attention_forms import FORMS, lens as _lens
from test_gpu_ragged import _per_window

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-3   # BASELINE.json north_star, as in test_gpu_parity.py
STAGE_TOL = 3e-4  # test_stagewise_against_oracle's bars (precision 9: 3e-4 of the row maximum and 8e-4 absolute)
P3, P8, P9 = _lib.PREC_BF16X3, _lib.PREC_I8X3, _lib.PREC_I8X3_FC
H = PA.N_HEAD
# one engine per (T, precision, regime), the cases of one engine next to each other
CASES = [(f, r) for r in PA.REGIMES for f in sorted(FORMS, key=lambda f: (f[1], f[0]))]


def _id(f, r):
    return f"p{f[0]}-T{f[1]}-B{f[2]}-{f[4]}-M{r[0]}g{r[1]}{'i' if r[2] else ''}{'s' if r[3:] == (True,) else ''}"


IDS = [_id(f, r) for f, r in CASES]
_MODELS = {}  # (T, precision, regime) -> (module, engine): the KEEP used last (as test_gpu_ragged._model; packing is a fraction of a second)
KEEP = 4


def _drop_models(keep=0):
    while len(_MODELS) > keep:
        m, _ = _MODELS.pop(next(iter(_MODELS)))
        m.invalidate_engine()  # closes the context: its workspace, captured graphs and capture stream go now, not at some collection


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """No packed engine of this file outlives it (the files after it meet the device as they did before this file existed)."""
    yield
    _drop_models()
    torch.cuda.synchronize()


def _model(T, prec, regime):
    key = (T, prec, regime)
    if key in _MODELS:
        _MODELS[key] = _MODELS.pop(key)
        return _MODELS[key]
    _drop_models(keep=KEEP - 1)
    sd, perms = PA.plant(T, *regime)
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=False)
    m.hip_precision = prec
    if prec != P3:
        # exactly the plain form of the precision: an explicit precision otherwise keeps whichever packing measured best on the
        # probe batch, and in the mixed regime that is the prepared one (compensated weight rounding) — not what attention_i8 restates
        m.hip_plan_override = (prec, False, 0)
        m.hip_probe_full_chain = False  # (the verdict is not under test here: stage 1 of the probe is enough to pack the form)
    m = m.cuda()
    eng = m.hip_engine()
    assert m.hip_precision_used == prec and m._slot.plan["flags"] == 0 and not m._slot.plan["prepared"]
    _MODELS[key] = (m, eng)
    return m, eng


@functools.lru_cache(maxsize=None)
def _reference(T, B, regime):
    """The oracle's taps, the fp64 restatement of layer 0 and the int8 restatements (precision 8: "i8", 9: "i8fc") for the inputs of
    a (T, B) case (computed once per regime)."""
    sd, perms = PA.plant(T, *regime)
    x, xc, t = PA.inputs(T, B, 1000 * T + B)
    taps, r64 = PA.block(sd, torch.cat((x, xc), -1), t)
    lt = taps["layer0"]
    keep = {"denoise": taps["denoise"], "attn_out": lt["attn_out"], "attn_ln": lt["attn_ln"],
            "attn_out64": r64["attn_out"].float(), "attn_ln64": r64["attn_ln"].float()}
    for tag, prec in (("i8", P8), ("i8fc", P9)):
        if any(f[:3] == (prec, T, B) for f in FORMS):
            r = PA.attention_i8(sd, PA.TR + "layer_stack.0.self_attn.", taps["embed"], PA.i8_v_scale(T), prec == P9)
            keep["attn_out" + tag], keep["attn_ln" + tag] = r["attn_out"].float(), r["attn_ln"].float()
    return keep


def _stage_err(prec, got, want):
    """-> (max abs, max relative to the row maximum, within test_stagewise_against_oracle's bar)"""
    a, rel = PA.stage_err(got.cpu(), want)
    if prec == P9:
        return a, rel, rel <= 3e-4 and a < 8e-4
    return a, rel, a < STAGE_TOL


@pytest.mark.parametrize("form, regime", CASES, ids=IDS)
def test_every_attention_form_in_every_regime(form, regime):
    """One forward per case: the denoiser output of every window against the oracle; layer 0's attn_out and attn_ln stops against
    the restatements named at the top of this file; and (one-hot regimes) every head's attn_out row i against the GPU's own V row
    pi_h(i) — the V stop runs the split-bf16 projections in every precision, so precision 8 (absolute bar) first takes off what its
    format alone does to that row (its restatement minus the exact one, from the CPU): for precision 8 the check is therefore
    not independent of the restatement comparison above, it names the key addressing."""
    prec, T, B, qkv, attn = form
    m, eng = _model(T, prec, regime)
    perms = PA.plant(T, *regime)[1]
    ref = _reference(T, B, regime)
    x, xc, t = (v.cuda() for v in PA.inputs(T, B, 1000 * T + B))
    assert int(t.min()) == 0 and int(t.max()) == 999
    out = eng.denoise(x, xc, t)
    assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)
    assert bool(torch.isfinite(out).all())
    e_den = float((out.cpu() - ref["denoise"]).abs().amax((1, 2)).max())  # (every window)
    seen = {"denoise": e_den}
    own = {P3: "", P8: "i8", P9: "i8fc"}[prec]
    exact_too = prec == P3 or (prec == P9 and regime[0] >= 40)
    fails = []
    stops = {}
    for st in ("attn_out", "attn_ln"):
        got = stops[st] = eng.debug_stage(x, xc, t, 0, st)
        if st == "attn_out":
            assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)  # the stop taps the same kernels
        assert bool(torch.isfinite(got).all()), st
        for tag, want, asserted in ((st + " vs its int8 restatement", ref.get(st + own), bool(own)),
                                    (st + " vs fp64", ref[st + "64"], exact_too), (st + " vs oracle", ref[st], exact_too)):
            if not own and tag.endswith("restatement"):
                continue
            a, rel, ok = _stage_err(prec, got, want)
            seen[tag] = (a, rel)
            if not ok and asserted:
                fails.append(tag)
    if regime[0] >= 40:
        v = eng.debug_stage(x, xc, t, 0, "v")  # [B, H, L, 256]
        o = stops["attn_out"].cpu()
        if prec == P8:
            o = o - (ref["attn_outi8"] - ref["attn_out64"])
        o = o.view(B, T + 1, H, 256).permute(0, 2, 1, 3)
        for h in range(H):
            a, rel, ok = _stage_err(prec, o[:, h], v[:, h, torch.from_numpy(perms[h]).cuda()].cpu())
            seen[f"head {h} vs own V"] = (a, rel)
            if not ok:
                fails.append(f"attn_out row i is not V row pi(i) in head {h}")
    print(f"precision {prec} T={T} B={B} {attn} regime {regime}:", {k: (f"{v:.1e}" if isinstance(v, float) else tuple(f"{c:.1e}" for c in v))
                                                                  for k, v in seen.items()})
    assert not fails and e_den < POSE_TOL, (fails, seen)


@functools.lru_cache(maxsize=None)
def _ragged_reference(T, B, regime):
    """The oracle's denoiser output and p_sample result of every window alone, cut to its own length."""
    sd, perms = PA.plant(T, *regime)
    sched = O.make_schedule(1000)
    x, xc, t = PA.inputs(T, B, 2000 * T + B)
    nz = torch.randn(B, T, 198, generator=torch.Generator().manual_seed(B))
    lens = _lens(T, B)
    with torch.no_grad():
        den = _per_window(lambda r, n: O.denoise(sd, torch.cat((x[r, :n], xc[r, :n]), -1), t[r]), lens)
        smp = _per_window(lambda r, n: O.p_sample(sd, sched, x[r, :n], t[r], xc[r, :n], nz[r, :n]), lens)
    assert sorted(den) == sorted(smp) == list(range(B))  # no window is left out
    return lens, nz, den, smp


# the same forms and regimes; the int8 forms carry the shift of (40, -300, yes) as planted_attention.I8_RAGGED_SHIFTED
RAGGED = [(f, PA.I8_RAGGED_SHIFTED if f[0] != P3 and r == (40, -300, True) else r) for f, r in CASES]


@pytest.mark.parametrize("form, regime", RAGGED, ids=[_id(f, r) for f, r in RAGGED])
def test_ragged_winner_masked(form, regime):
    """Windows of different lengths (random values in the frames past each length): the rows whose planted winner lies past their
    window's length must not see it — the oracle on the window cut to its length gives such a row the plain average over the keys
    left (pure regimes), and with M = 200 one unmasked key moves the result by O(1).  Every window's real rows, after one forward
    and after one p_sample step."""
    prec, T, B, qkv, attn = form
    m, eng = _model(T, prec, regime)
    perms = PA.plant(T, *regime)[1]
    lens, nz, den, smp = _ragged_reference(T, B, regime)
    masked = sum(int((perms[:, :n + 1] > n).sum()) for n in lens)
    kept = sum(int((perms[:, :n + 1] <= n).sum()) for n in lens if n < T)
    assert masked > 0 and kept > 0
    x, xc, t = (v.cuda() for v in PA.inputs(T, B, 2000 * T + B))
    out = eng.denoise(x, xc, t, lengths=lens)
    assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)
    assert bool(torch.isfinite(out).all())
    e_den = max(float((out[b, :n].cpu() - den[b]).abs().max()) for b, n in enumerate(lens))
    x1 = eng.p_sample_(x.clone(), xc, t, noise=nz.cuda(), lengths=lens)
    assert (eng.last_kernel("qkv"), eng.last_kernel("attn")) == (qkv, attn)
    assert bool(torch.isfinite(x1).all())
    e_smp = max(float((x1[b, :n].cpu() - smp[b]).abs().max()) for b, n in enumerate(lens))
    print(f"precision {prec} T={T} B={B} {attn} regime {regime}: {masked} rows with a masked winner; denoise {e_den:.2e} p_sample {e_smp:.2e}")
    assert e_den < POSE_TOL and e_smp < POSE_TOL, (e_den, e_smp)


CHAIN_SEED, CHAIN_T0, CHAIN_STEPS = 0x51A9E3779B97F4A7, 7, 8  # t = 7 .. 0: where the posterior mean is mostly the denoiser's output


@functools.lru_cache(maxsize=None)
def _chain_reference(B):
    T, regime = 120, (40, 0, True)
    sd, _ = PA.plant(T, *regime)
    sched = O.make_schedule(1000)
    x, xc, _ = PA.inputs(T, B, 31 + B)
    w = x.clone()
    with torch.no_grad():
        for i in range(CHAIN_STEPS):
            tt = CHAIN_T0 - i
            nz = torch.from_numpy(philox_noise(CHAIN_SEED, tt, 0, B, T)).float()
            w = O.p_sample(sd, sched, w, torch.full((B,), tt, dtype=torch.long), xc, nz)
    return x, xc, w


@pytest.mark.parametrize("B", [2, 25])
@pytest.mark.parametrize("prec", [P3, P8, P9])
def test_short_chain_on_sharp_attention(prec, B):
    """8 ancestral steps with in-kernel Philox noise through sample_loop_ (the captured step replays the same kernels) against the
    oracle chain fed the numpy restatement of the same draws."""
    T, regime = 120, (40, 0, True)
    m, eng = _model(T, prec, regime)
    x0, xc, want = _chain_reference(B)
    x = x0.clone().cuda()
    eng.sample_loop_(x, xc.cuda(), CHAIN_T0, CHAIN_STEPS, noise_mode=_lib.NOISE_PHILOX, seed=CHAIN_SEED)
    e = float((x.cpu() - want).abs().amax((1, 2)).max())
    print(f"precision {prec} B={B}: {CHAIN_STEPS}-step Philox chain on regime {regime} vs oracle {e:.2e}")
    assert bool(torch.isfinite(x).all()) and e < POSE_TOL, e


# ------------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("regime", PA.S1_REGIMES, ids=lambda r: f"M{r[0]}g{r[1]}{'i' if r[2] else ''}")
@pytest.mark.parametrize("kind, window", [("headnet", 60), ("headnet", 90), ("headnet", 128), ("gravitynet", 120)])
def test_stage1_sharp_attention(kind, window, regime):
    """s1_attn_kernel on a planted layer 0 (padded tokens are keys there and carry their codes like any other): every layer and the
    heads against tests/stage1_oracle.py at test_random_batches_against_oracle's bar, on batches with short last blocks."""
    n_layers = 2
    cfg, sd, perms = PA.plant_stage1(kind, window, n_layers, *regime)
    eng = stage1.Stage1Engine(cfg, "cuda:0")
    eng.load(sd)
    rng = np.random.default_rng(window * 10 + regime[0] - regime[1])
    feats, valid = [], []
    for T in (1, 19, window - 1, window, window + 1, 2 * window + 13):
        for st, n in stage1.block_spans(T, window):
            f = np.zeros((window, cfg.d_feats), np.float32)
            f[:n] = rng.standard_normal((n, cfg.d_feats))
            feats.append(f)
            valid.append(n)
    assert any(0 < n < window for n in valid) and window in valid
    feats = torch.from_numpy(np.stack(feats))
    valid = torch.tensor(valid, dtype=torch.int32)
    out, layers = eng.encode(feats.cuda(), valid.cuda(), layers=True)
    got, layers = out.cpu(), layers.cpu()
    eng.close()
    ref = S1O.decoder(sd, feats, valid, n_layers)
    worst = [(layers[l] - ref[l]).abs().max().item() for l in range(n_layers)]
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(layers).all())
    if kind == "headnet":
        va, dist = S1O.headnet_heads(sd, ref[-1])
        rh = torch.cat([va, dist], -1)
        mk = (torch.arange(window)[None, :] < valid[:, None].long())
        e_head = max(float((got[..., c][mk] - rh[..., c][mk]).abs().max() / rh[..., c][mk].abs().max()) for c in range(4))
    else:
        rh = S1O.gravity_head(sd, ref[-1][:, 0])
        e_head = float((got - rh).abs().max() / rh.abs().max())
    print(f"{kind} window {window} regime {regime}: layers {[f'{e:.1e}' for e in worst]} heads {e_head:.1e}")
    assert max(worst) < 1e-4 and e_head < 1e-4, (worst, e_head)
