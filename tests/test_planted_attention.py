"""The conditions that make the assertions of tests/test_gpu_sharp_attention.py fair, checked on the CPU: the planted logits are what
planted_attention.plant says they are, they survive the int8 forms' operand format, and the fp32 oracle agrees with the fp64
restatement where the GPU tests compare against either."""
import functools

import numpy as np
import pytest
import torch

import planted_attention as PA
import stage1_oracle as S1O

WINDOWS = (30, 120, 196)
ALL_REGIMES = PA.REGIMES + (PA.I8_RAGGED_SHIFTED,)
CASES = [(T, r) for T in WINDOWS for r in ALL_REGIMES]
POSE_TOL = 1e-3
STAGE_TOL = 3e-4  # test_stagewise_against_oracle: precisions 3 and 8 absolute; precision 9: 3e-4 of the row maximum and 8e-4 absolute


@functools.lru_cache(maxsize=None)
def _block(T, regime, fmt=None):
    sd, perms = PA.plant(T, *regime)
    x, xc, t = PA.inputs(T, 2, 7 * T)
    taps, r64 = PA.block(sd, torch.cat((x, xc), -1), t, fmt)
    return perms, taps, r64


@pytest.mark.parametrize("T, regime", CASES)
def test_every_row_has_its_planted_winner(T, regime):
    M, gamma, over = regime[:3]
    perms, taps, r64 = _block(T, regime)
    ok, margin = PA.margins(r64["logits"], perms)
    lo, hi = float(r64["logits"].min()), float(r64["logits"].max())
    print(f"T={T} M={M} gamma={gamma} over_init={over}: margin {margin:.2f}, logits {lo:.1f} .. {hi:.1f}, |k| max {float(r64['k'].abs().max()):.0f}")
    assert ok
    assert margin >= (25 if over else M - 1e-3), margin  # (the pure regimes: M up to the float32 rounding of the stored weights)
    if not over:  # the logits are M [j = pi(i)] + gamma, nothing else
        L = T + 1
        want = torch.full((PA.N_HEAD, L, L), float(gamma), dtype=torch.float64)
        want[torch.arange(PA.N_HEAD)[:, None], torch.arange(L)[None], torch.from_numpy(perms)] += M
        assert float((r64["logits"] - want).abs().max()) < 1e-3 * max(1.0, abs(gamma) / 30)
    if M >= 30:  # the result is a permutation of V's rows
        v, o = r64["v"], r64["attn_out"].view(2, T + 1, PA.N_HEAD, 256).permute(0, 2, 1, 3)
        for h in range(PA.N_HEAD):
            assert float((o[:, h] - v[:, h, perms[h]]).abs().max()) < 1e-8


@pytest.mark.parametrize("T", WINDOWS)
def test_the_winners_reach_every_key_tile(T):
    L = T + 1
    for regime in ALL_REGIMES:
        _, perms = PA.plant(T, *regime)
        for h, p in enumerate(perms):
            assert sorted(p.tolist()) == list(range(L))
            assert not PA._monotone(p) and not (p == np.arange(L)).all(), (regime, h)
            assert {0, L - 1} <= set(p.tolist())
            assert {int(j) // 32 for j in p} == set(range((L + 31) // 32))
            # a row block of 32 queries does not keep its winners in one key tile (a tile-local mistake cannot hide)
            if L > 64:
                assert all(len({int(j) // 32 for j in p[i:i + 32]}) > 1 for i in range(0, L, 32)), (regime, h)


@pytest.mark.parametrize("T, regime", CASES)
def test_operand_rounding_keeps_the_winners(T, regime):
    """q and k rows rounded to 2^-15 of their row maximum (the int8 forms' fixed point per row, include/egoego_hip.h)."""
    M = regime[0]
    perms, _, exact = _block(T, regime)
    _, _, rounded = _block(T, regime, "qk")
    ok, margin = PA.margins(rounded["logits"], perms)
    moved = float((rounded["attn_out"] - exact["attn_out"]).abs().max())
    print(f"T={T} regime {regime}: margin after rounding {margin:.2f}, attn_out moved by {moved:.1e}")
    if M >= 40:
        assert ok and margin >= 20, margin
    assert moved <= 1e-4, moved


@pytest.mark.parametrize("T, regime", [(T, r) for T in WINDOWS for r in PA.REGIMES])
def test_what_the_int8_operand_format_itself_does(T, regime):
    """attention_i8 (the int8-slice precisions as include/egoego_hip.h and csrc/common.h define them: 16-bit rows in two slices, the
    low x low products dropped — exact integers, no kernel) against the exact restatement.  Rounding q and k alone (above) moves
    nothing, but a one-hot row hands ONE V row through unaveraged, and V carries the format of the layer input, of w_v and of its own
    image.  So the GPU test compares the int8 forms' stops with attention_i8 at the stage bars, in every regime; with the exact
    restatement and the oracle's taps only where the format itself keeps the bar:
    * precision 9 (3e-4 of the row maximum and 8e-4 absolute) keeps it in the one-hot regimes;
    * precision 8 (3e-4 absolute) does not in any regime, precision 9 does not in the mixed one: the format moves the exact
      attn_out by far more than the 1e-4 that admits a case to a comparison."""
    M = regime[0]
    perms, _, exact = _block(T, regime)
    sd, _ = PA.plant(T, *regime)
    x, xc, t = PA.inputs(T, 2, 7 * T)
    e = PA.layer0_input(sd, torch.cat((x, xc), -1), t)
    i8 = PA.attention_i8(sd, PA.TR + "layer_stack.0.self_attn.", e, PA.i8_v_scale(T))
    ok, margin = PA.margins(i8["logits"], perms)
    a8, r8 = PA.format_moves(T, regime, "i8")
    a9, r9 = PA.format_moves(T, regime, "i8fc")
    l9, lr9 = PA.format_moves(T, regime, "i8fc", stage="attn_ln")
    print(f"T={T} regime {regime}: int8 format alone: margin {margin:.1f}; attn_out precision 8 {a8:.1e} / {r8:.1e}, precision 9 {a9:.1e} / {r9:.1e}, "
          f"attn_ln precision 9 {l9:.1e} / {lr9:.1e}")
    if M >= 40:
        assert ok and margin >= 20, margin
        assert r9 <= STAGE_TOL and a9 < 8e-4 and lr9 <= STAGE_TOL and l9 < 8e-4  # precision 9 is compared with the exact result
    else:
        assert a9 > 1e-4, "precision 9's format now keeps the mixed regime: test_gpu_sharp_attention can compare it with the exact result too"
    assert a8 > 1e-4, "precision 8's format now keeps this regime: test_gpu_sharp_attention can compare it with the exact result too"


@pytest.mark.parametrize("T", WINDOWS)
def test_the_ragged_regimes_of_the_int8_forms(T):
    """A row whose winner is masked falls back on the logits left.  With gamma = -300 on w_k.bias those are order-1 differences between
    k rows of magnitude ~500, and the 16-bit rounding of q and k alone moves the exact attn_out by more than the pose bar: the int8
    forms' ragged cases carry their shift as I8_RAGGED_SHIFTED instead, which the format holds like the unshifted regimes."""
    cuts = [n for n in PA.LENGTHS[T] if n < T]
    for regime in PA.REGIMES[:3] + (PA.I8_RAGGED_SHIFTED,):
        worst = max(PA.format_moves(T, regime, "qk", n)[0] for n in cuts)
        print(f"T={T} regime {regime}: q and k rounded, ragged lengths: attn_out moves by up to {worst:.1e}")
        assert worst <= POSE_TOL, (regime, worst)
    worst = max(PA.format_moves(T, PA.REGIMES[3], "qk", n)[0] for n in cuts)
    print(f"T={T} regime {PA.REGIMES[3]}: q and k rounded, ragged lengths: attn_out moves by up to {worst:.1e}")
    assert worst > POSE_TOL
    _, _, r64 = _block(T, PA.I8_RAGGED_SHIFTED)
    assert float(r64["logits"].max()) <= -50.0  # (a row maximum started from 0 leaves rint(p * 8355711) = 0 on every key)


@pytest.mark.parametrize("T, regime", CASES)
def test_the_fp32_oracle_agrees_with_the_fp64_restatement(T, regime):
    perms, taps, r64 = _block(T, regime)
    lt = taps["layer0"]
    e_out = float((lt["attn_out"].double() - r64["attn_out"]).abs().max())
    e_ln = float((lt["attn_ln"].double() - r64["attn_ln"]).abs().max())
    print(f"T={T} regime {regime}: fp32 oracle against fp64: attn_out {e_out:.1e} attn_ln {e_ln:.1e}")
    assert bool(torch.isfinite(taps["denoise"]).all())
    assert e_out <= 1e-5 and e_ln <= 1e-5, (e_out, e_ln)


@pytest.mark.parametrize("T", WINDOWS)
def test_ragged_lengths_mask_some_winners_and_keep_others(T):
    """A window of n frames has the rows and keys 0..n.  At every n < T of LENGTHS[T], in every head, some row's winner lies past
    the window and some row's inside; a row whose winner is masked is, in the pure regimes, the plain average of V over the keys
    left; every window of a ragged batch has one of these lengths."""
    cuts = [n for n in PA.LENGTHS[T] if n < T]
    assert cuts and PA.LENGTHS[T][0] == T
    for B in {b for _, t_, b, _, _ in PA.FORMS if t_ == T}:
        lens = PA._lens(T, B)
        assert len(lens) == B and set(lens) <= set(PA.LENGTHS[T]) and lens[0] == T and any(n < T for n in lens)
    for regime in ALL_REGIMES:
        sd, perms = PA.plant(T, *regime)
        for n in cuts:
            for h, p in enumerate(perms):
                assert (p[:n + 1] > n).any() and (p[:n + 1] <= n).any(), (regime, n, h)
    x, xc, t = PA.inputs(T, 1, 3)
    for regime in ((200, 0, False), (6, 0, False)):
        sd, perms = PA.plant(T, *regime)
        n = cuts[len(cuts) // 2]
        _, r64 = PA.block(sd, torch.cat((x[:, :n], xc[:, :n]), -1), t)
        o = r64["attn_out"].view(1, n + 1, PA.N_HEAD, 256)
        for h, p in enumerate(perms):
            gone = np.flatnonzero(p[:n + 1] > n)
            mean = r64["v"][0, h].mean(0)
            assert float((o[0, gone, h] - mean).abs().max()) < 1e-6, (regime, h)
            kept = np.flatnonzero(p[:n + 1] <= n)
            assert float((o[0, kept, h] - mean).abs().max()) > 1e-2  # (the rows that keep their winner are not the average)


@pytest.mark.parametrize("kind, window", [("headnet", 60), ("headnet", 90), ("headnet", 128), ("gravitynet", 120)])
@pytest.mark.parametrize("regime", PA.S1_REGIMES)
def test_stage1_planting(kind, window, regime):
    """Layer 0 of a planted stage-1 decoder: the winners are the permutations' for a block with padded tokens (they are keys)."""
    M, gamma, over = regime[:3]
    cfg, sd, perms = PA.plant_stage1(kind, window, 2, *regime)
    rng = np.random.default_rng(window)
    valid = max(1, window - 17)
    f = torch.zeros(1, window, cfg.d_feats)
    f[0, :valid] = torch.from_numpy(rng.standard_normal((valid, cfg.d_feats)).astype(np.float32))
    emb = torch.nn.functional.conv1d(f.transpose(1, 2), sd[PA.S1_TR + "start_conv.weight"], sd[PA.S1_TR + "start_conv.bias"]).transpose(1, 2)
    emb = emb + sd[PA.S1_TR + "position_vec.weight"][1:window + 1][None]
    r64 = PA.attention_fp64(sd, PA.S1_TR + "layer_stack.0.self_attn.", emb)
    ok, margin = PA.margins(r64["logits"], perms)
    print(f"{kind} window {window} regime {regime}: margin {margin:.2f}")
    assert ok and margin >= (25 if over else M - 1e-3), margin
    ref = S1O.decoder(sd, f, torch.tensor([valid]), 2)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    for p in perms:
        assert not PA._monotone(p) and {int(j) // 32 for j in p} == set(range((window + 31) // 32))
