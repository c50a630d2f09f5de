"""Ragged stage 2 on the host: the window table of the ragged sliding-window harness against the one-sequence rule, the lengths
validation of the ragged sampling calls (no device is touched), and the new entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

from egoego_release_amd import _lib, engine, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_SYMBOLS = ("egoego_denoise_ragged", "egoego_p_sample_ragged", "egoego_sample_loop_ragged")


@pytest.mark.parametrize("seq_len, frames", [(30, (11, 30, 31, 40, 41, 50, 60, 70, 75)), (120, (140, 120, 121, 230))])
def test_ragged_window_table_matches_window_spans(seq_len, frames):
    table = harness.ragged_window_table(frames, seq_len)
    spans = [harness.window_spans(n, seq_len) for n in frames]
    assert len(table) == max(len(sp) for sp in spans)
    seen = [[] for _ in frames]
    for k, ent in enumerate(table):
        assert ent["sequences"] == [s for s, sp in enumerate(spans) if len(sp) > k]  # every sequence with a k-th window, ascending
        assert len(ent["spans"]) == len(ent["continues"]) == len(ent["sequences"])
        for s, span, cont in zip(ent["sequences"], ent["spans"], ent["continues"]):
            assert span == spans[s][k] and span[0] == k * (seq_len - harness.OVERLAP)
            assert cont == (len(spans[s]) > k + 1)
            if cont:
                assert span[1] == seq_len  # only a sequence's last window is short: what is prefixed from is a full window
            seen[s].append(span)
    for s, n in enumerate(frames):
        assert seen[s] == spans[s]
        assert sum(m for _, m in seen[s]) - harness.OVERLAP * (len(seen[s]) - 1) == harness.output_frames(n, seq_len)
    # the edge the table is built around: 11 frames are one window, a second window of exactly 11 frames exists
    assert harness.window_spans(11, 30) == [(0, 11)] and harness.window_spans(31, 30) == [(0, 30), (20, 11)]


@pytest.mark.parametrize("frames", [(10,), (40, 0), (40, 7, 50), (1,)])
def test_sequences_without_a_window_raise(frames):
    with pytest.raises(ValueError, match="frames"):
        harness.ragged_window_table(frames, 30)


def test_lengths_validation_raises_before_any_device_is_touched(monkeypatch):
    T, B = 120, 4
    # (a ValueError must not come from a device call: the library is not even loaded)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    ok = engine.check_lengths([120, 1, 64, 11], B, T)
    assert ok.dtype == np.int32 and ok.tolist() == [120, 1, 64, 11]
    assert engine.check_lengths(torch.tensor([120, 1, 64, 11]), B, T, prefix_len=1).tolist() == [120, 1, 64, 11]
    for bad, what in (([120, 0, 64, 11], "0..120"), ([120, T + 1, 64, 11], f"11..{T + 1}"), ([120, -3, 64, 11], "-3..120")):
        with pytest.raises(ValueError, match=re.escape(what)):
            engine.check_lengths(bad, B, T)
    for bad in ([120, 64, 11], [[120, 1, 64, 11]], 120, np.zeros((B, 1), dtype=np.int64) + 5):
        with pytest.raises(ValueError, match="expected"):
            engine.check_lengths(bad, B, T)
    with pytest.raises(ValueError, match="prefix of 10 frames"):
        engine.check_lengths([120, 9, 64, 11], B, T, prefix_len=10)
    assert engine.check_lengths([120, 10, 64, 11], B, T, prefix_len=10).min() == 10
    ids = engine.check_window_ids([7, 0, 2 ** 32 - 1, 5], B)
    assert ids.dtype == np.int64 and ids.tolist() == [7, 0, 2 ** 32 - 1, 5]
    for bad in ([1, 2, 3], [-1, 0, 1, 2], [0, 1, 2, 2 ** 32], [0.0, 1.0, 2.0, 3.0], torch.tensor([0.5, 1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            engine.check_window_ids(bad, B)
    with pytest.raises(ValueError, match="integers"):
        engine.check_lengths([120.0, 1.5, 64.0, 11.0], B, T)


def test_model_entry_points_validate_lengths_first():
    """p_sample_loop / sample check host lengths before the draws, the plan and any launch: the module sits on the CPU here, where
    every sampling call would otherwise raise EgoEgoHipError (no CPU path)."""
    from egoego_release_amd import ModelConfig
    from egoego_release_amd.model import CondGaussianDiffusion
    m = CondGaussianDiffusion(**ModelConfig(max_timesteps=41).ctor_kwargs())
    x = torch.zeros(3, 40, 198)
    for bad in ([40, 0, 11], [40, 41, 11], [40, 11]):
        with pytest.raises(ValueError):
            m.sample(x, torch.ones_like(x), lengths=bad)
    with pytest.raises(ValueError, match="prefix"):
        m.p_sample_loop(x.shape, x, torch.ones_like(x), prefix=torch.zeros(3, 10, 198), lengths=[40, 9, 11])
    with pytest.raises(_lib.EgoEgoHipError):  # valid lengths get as far as the missing device
        m.sample(x, torch.ones_like(x), lengths=[40, 1, 11])


def test_ragged_harness_rejects_the_torch_generator_and_short_sequences():
    class Model:  # (both checks come before the model is used for anything else)
        sampling_rng = "torch"
        num_timesteps, seq_len = 6, 40
    with pytest.raises(ValueError, match="philox"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(Model(), None, [torch.zeros(50, 7)])
    # injected x_T / condition noise without 'steps' still means in-kernel Philox steps: the torch generator is refused there too;
    # dicts of which only some carry 'steps' are refused whatever the generator
    draws = [{"x_all": torch.zeros(1, 50, 198), "cond": [torch.zeros(1, 40, 198), torch.zeros(1, 20, 198)]} for _ in range(2)]
    with pytest.raises(ValueError, match="philox"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(Model(), None, [torch.zeros(50, 7)] * 2, noise=draws)
    Model.sampling_rng = "philox"
    mixed = [dict(draws[0], steps=[torch.zeros(6, 1, 40, 198), torch.zeros(6, 1, 20, 198)]), draws[1]]
    with pytest.raises(ValueError, match="every sequence"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(Model(), None, [torch.zeros(50, 7)] * 2, noise=mixed)
    with pytest.raises(ValueError, match="10 frames|more than 10"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(Model(), None, [torch.zeros(50, 7), torch.zeros(10, 7)])
    with pytest.raises(ValueError, match="lengths"):
        harness.full_body_gen_cond_head_pose_sliding_window_ragged(Model(), None, torch.zeros(2, 50, 7))


def test_ragged_symbols_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in RAGGED_SYMBOLS:
        assert re.search(rf"\bint {sym}\s*\(", code), sym
        assert sym in _lib.EXPORTS
    # the ragged forms take the uniform form's arguments plus the device arrays, behind d_row_mask
    def params(name):
        return [p.strip() for p in re.search(rf"\b{name}\s*\((.*?)\);", code, flags=re.S).group(1).replace("\n", " ").split(",")]
    for name, extra in (("egoego_denoise", ["const int32_t* d_lengths"]),
                        ("egoego_p_sample", ["const int32_t* d_lengths", "const int64_t* d_window_ids"]),
                        ("egoego_sample_loop", ["const int32_t* d_lengths", "const int64_t* d_window_ids"])):
        base, rag = params(name), params(name + "_ragged")
        i = base.index("const float* d_row_mask") + 1
        assert rag == base[:i] + extra + base[i:], name
    assert "#define EGOEGO_ABI_VERSION 8" in src and _lib.ABI_VERSION == 8  # purely additive
    lib = _lib.load()
    for sym, n in zip(RAGGED_SYMBOLS, (12, 17, 19)):
        assert len(getattr(lib, sym).argtypes) == n, sym
