"""The two-workgroups-per-CU int8 layer tail runs fc head-major: both feature passes of a wave on the chunk of head h while it sits
in LDS, the attention output's row scales staged in LDS (tail_fused.h DirectGemm::run_heads).  The integer chains and the fold order
per output element are those of the eight-wave tail, whose fc is a single pass over its tiles — so a window must come out with the
SAME bits from a 65-window call (260 token blocks: the smallest grid that takes the two-workgroup form at T <= 127) and from a
64-window call of the same windows (256 blocks: the eight-wave form)."""
import pytest
import torch

from egoego_release_amd import ModelConfig, make_weights, _lib
from egoego_release_amd.engine import HipEngine
from egoego_release_amd.model import CondGaussianDiffusion
from egoego_release_amd.precision import _engine_cfg

pytestmark = pytest.mark.gpu
TWO_WG = "tail_kernel<1,true,true,true,4,true>"
EIGHT_WAVE = "tail_kernel<1,true,true,false,8,true>"
NB, NS = 65, 64


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(T, flags=0):
        if (T, flags) not in made:
            cfg = ModelConfig(max_timesteps=T + 1)
            m = CondGaussianDiffusion(**cfg.ctor_kwargs())
            m.load_state_dict(make_weights(cfg, 0), strict=False)
            made[(T, flags)] = HipEngine(_engine_cfg(m), m.state_dict(), torch.device("cuda"), _lib.PREC_I8X3_FC, flags)
        return made[(T, flags)]

    yield get
    for e in made.values():
        e.close()


def _inputs(T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(NB, T, 198, generator=g).cuda()
    xc = torch.randn(NB, T, 198, generator=g).cuda()
    t = torch.randint(0, 1000, (NB,), generator=g).cuda()
    return x, xc, t


def _chain_pair(eng, x, xc, lengths=None):
    """3 steps of the chain on all 65 windows and on the first 64 -> (big, small), each checked for the tail form it ran."""
    big = x.clone()
    eng.sample_loop_(big, xc, 999, 3, noise_mode=_lib.NOISE_PHILOX, seed=9, lengths=lengths)
    assert eng.last_kernel("fc_ln") == TWO_WG
    small = x[:NS].contiguous().clone()
    eng.sample_loop_(small, xc[:NS].contiguous(), 999, 3, noise_mode=_lib.NOISE_PHILOX, seed=9, lengths=None if lengths is None else lengths[:NS])
    assert eng.last_kernel("fc_ln") == EIGHT_WAVE
    return big, small


@pytest.mark.parametrize("T", [120, 100])  # T = 100: rows 101..127 of every window are padding, the window's last 32-row block is partly valid
def test_chain_of_65_windows_has_the_bits_of_64(engines, T):
    x, xc, _ = _inputs(T, 31 + T)
    big, small = _chain_pair(engines(T), x, xc)
    assert torch.isfinite(big).all()
    assert torch.equal(big[:NS], small)


def test_chain_with_three_slice_fc_weights(engines):
    """EGOEGO_FLAG_FC24: the third-slice contraction runs head-major too."""
    x, xc, _ = _inputs(120, 41)
    big, small = _chain_pair(engines(120, _lib.FLAG_FC24), x, xc)
    assert torch.equal(big[:NS], small)
    plain = x.clone()
    engines(120).sample_loop_(plain, xc, 999, 3, noise_mode=_lib.NOISE_PHILOX, seed=9)
    assert not torch.equal(plain, big)  # the pass really ran


def test_ragged_chain_of_mixed_lengths(engines):
    T = 120
    x, xc, _ = _inputs(T, 51)
    lengths = [T - (7 * i) % 90 for i in range(NB)]  # 31 .. 120 frames, window 0 full
    big, small = _chain_pair(engines(T), x, xc, lengths=lengths)
    for b in range(NS):  # a window's rows past its length come back unspecified
        assert torch.equal(big[b, :lengths[b]], small[b, :lengths[b]]), b


@pytest.mark.parametrize("stage", ["attn_ln", "ffn_hidden"])  # the tail's debug taps: stop = 1 (after LayerNorm-1), 2 (after FFN-1)
def test_debug_taps_of_65_windows_have_the_bits_of_64(engines, stage):
    eng = engines(120)
    x, xc, t = _inputs(120, 61)
    for layer in (0, 3):
        big = eng.debug_stage(x, xc, t, layer, stage)
        assert eng.last_kernel("fc_ln") == TWO_WG
        small = eng.debug_stage(x[:NS].contiguous(), xc[:NS].contiguous(), t[:NS].contiguous(), layer, stage)
        assert eng.last_kernel("fc_ln") == EIGHT_WAVE
        assert torch.equal(big[:NS], small), layer
