"""Every kernel variant of the denoiser's dispatch (run_chunk_np in egoego_hip.hip), checked window by window against the fp32 oracle,
and the in-kernel Philox noise stream checked against a numpy restatement of common.h's philox4x32_10 / philox_normal4.

Which kernels run depends on the precision, the batch and the window length.  The sweep below runs one table of (precision, T, B)
configurations; each names the kernel every launch site must record (egoego_last_kernel_name) and is compared with the oracle at every
debug stop of layers 0 and 3, at the denoiser output and after one p_sample step — for every window, not a sample of them.  The CPU part
holds the table to the source: every name the library can record is either reached by the table or listed in UNREACHABLE with a reason,
and the dispatch constants the table was derived from are the ones in the source."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from egoego_release_amd import ModelConfig, make_weights, _lib
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SRC = os.path.join(ROOT, "egoego_release_amd", "csrc", "egoego_hip.hip")
POSE_TOL = 1e-3  # BASELINE.json north_star, as in test_gpu_parity.py
STAGE_TOL = 3e-4  # test_stagewise_against_oracle's bars (precision 9: 3e-4 of the row maximum and 8e-4 absolute)
P3, P8, P9 = _lib.PREC_BF16X3, _lib.PREC_I8X3, _lib.PREC_I8X3_FC
SLOTS = ("embed", "qkv", "attn", "fc_ln", "ffn1", "ffn2_ln", "out")

# ------------------------------------------------------------------------------------------------ the dispatch table
# The constants of egoego_hip.hip the table below is derived from (test_dispatch_constants_are_the_ones_the_table_assumes).
DISPATCH_CONSTANTS = {"ATTN_SPLIT6_MAX_BLOCKS": 256, "ATTN_SPLIT_MAX_BLOCKS": 256, "ATTN_SPLIT2_MAX_BLOCKS": 192,
                      "ATTN_HALF_MAX_BLOCKS": 192, "TAIL8_MAX_BLOCKS": 256, "TAIL8_BF16_MAX_BLOCKS": 160, "EMBED8_MAX_BLOCKS": 256,
                      "SMALL_GRID": 160, "EGOEGO_CORE4": 0, "EGOEGO_ATTN_WG4": 0, "TAIL8_BF16": 1, "EGOEGO_TAIL128_BF16": 1}
# Derivation (H = 4 heads, one chunk of B windows).  A window has Lr token rows: 128 at T=120 (L = 121, KT = 4); 32 at T=30 (KT = 1);
# at T=150 / 196 (KT = 7) 224 in split-bf16 and 208 in the int8 precisions.  rows = B * Lr rounded up to 256, so an odd B at T=120 runs
# (B + 1) * 128 rows.  Thresholds in B:
#   T=120  direct embed / linear_out: rows / 64 <= 256                      -> B <= 128
#          split-bf16 fused QKV + attention: B * H >= 192                   -> B >= 48
#          int8 attention layer: 6 B H <= 256 (six projection workgroups)   -> B <= 10; 3 B H <= 256 -> B <= 21; 2 B H <= 192 -> B <= 24;
#            attn_layer_i8w beyond (attn_layer_i8h's bound, 2 B H <= 192, is the same as the two-workgroup form's: UNREACHABLE)
#          split-bf16 / precision 8 small-batch tail: rows / 128 <= 128     -> B <= 128; 64-token build: rows / 64 >= 256 -> B >= 127;
#            eight-wave split-bf16 build: rows / 32 <= 160                  -> B <= 40
#          precision 9 resident tail, four-wave build: rows / 32 > 256      -> B >= 65
#          split-bf16, above the small-batch tail: rows / 128 < 200 -> three GEMMs (B <= 198); the fused layer tail beyond, its
#            128-token form from rows / 128 >= 256 (B >= 255); linear_out on CfgC2 while rows / 128 <= 160 (B <= 160)
#          (also straddled: embed_kernel's eight-wave build rows / 32 <= 256 -> B <= 64; out_kernel's two workgroups per token block
#           rows / 32 <= 128 -> B <= 32 — one recorded name each)
#   T=196  split-bf16 (224 rows): direct forms B <= 73; eight-wave tail B <= 22; 64-token tail B = 73; three GEMMs 74..113;
#            fused layer tail 114..145, its 128-token form from 146; CfgC2 up to 91; attn8_kernel from B H >= 256 -> B >= 64
#          int8 (208 rows): direct forms B <= 78; precision 8's 64-token tail B = 78, layer_tail_i8 from 79; CfgC2 79..98;
#            precision 9's resident tail four-wave from rows / 32 > 256 -> B >= 40; qkv_i8q's 128-token blocks from B >= 13 (one name)
#   T=150 the same geometry as T=196 (KT = 7, 208 / 224 rows); T=30 (KT = 1, 32 rows): every B up to 256 is a direct / small-batch form
SWEEP_B = {
    120: (1, 10, 11, 21, 22, 24, 25, 32, 33, 40, 41, 47, 48, 64, 65, 99, 100, 126, 127, 128, 129, 160, 161, 198, 199, 254, 255, 256),
    196: (2, 12, 13, 22, 23, 39, 40, 63, 64, 65, 72, 73, 74, 77, 78, 79, 91, 92, 98, 99, 113, 114, 145, 146, 256),
    150: (2, 256),
    30: (3, 256),
}
E_D, E_A, E_B = "embed_kernel", "gemm_kernel:EpiEmbed<CfgA>", "gemm_kernel:EpiEmbed<CfgB>"
O_D, O_C2, O_C, O_I8 = "out_kernel", "gemm_kernel:EpiOut<CfgC2>", "gemm_kernel:EpiOut<CfgC>", "gemm_i8_kernel:EpiOut"
T8W, T1, T2 = "tail_kernel<1,false,false,false,8>", "tail_kernel<1,false,false>", "tail_kernel<2,false,false>"
T1_8, T2_8 = "tail_kernel<1,true,false>", "tail_kernel<2,true,false>"
R8W, R4W = "tail_kernel<1,true,true,false,8,true>", "tail_kernel<1,true,true,true,4,true>"
N8W, N4W = "tail_kernel<1,true,true,false,8>", "tail_kernel<1,true,true,true>"
LT, LT128, LTI8 = "layer_tail_kernel", "layer_tail_kernel:128", "layer_tail_i8_kernel"
RES_BS, RES_B, FF_A = "gemm_kernel:EpiResLN<CfgBs>", "gemm_kernel:EpiResLN<CfgB>", "gemm_kernel:EpiTiled<CfgA>"
S6, S3, S2, AW, CS = "attn_proj6_i8_kernel", "attn_proj_i8_kernel", "attn_proj2_i8_kernel", "attn_layer_i8w_kernel", "attn_core_s_kernel"
Q8Q, CW = "qkv_i8q_kernel", "attn_core_i8w_kernel"


def _tail(*ranges):
    """The fused layer tails also run FFN-1 and FFN-2 + LayerNorm: the three slots carry one name."""
    return {"fc_ln": list(ranges), "ffn1": list(ranges), "ffn2_ln": list(ranges)}


_I8_LAYER_T120 = {"qkv": [(10, S6), (21, S3), (24, S2), (256, AW)], "attn": [(24, CS), (256, AW)]}
# (precision, T) -> {slot: [(largest B of the range, name), ...] in increasing B}
EXPECT = {
    (P3, 120): {"embed": [(128, E_D), (256, E_A)], "qkv": [(47, "qkv_kernel"), (256, "qkv_attn_kernel")],
                "attn": [(47, "attn_kernel"), (256, "qkv_attn_kernel")],
                "fc_ln": [(40, T8W), (126, T1), (128, T2), (198, RES_BS), (254, LT), (256, LT128)],
                "ffn1": [(40, T8W), (126, T1), (128, T2), (198, FF_A), (254, LT), (256, LT128)],
                "ffn2_ln": [(40, T8W), (126, T1), (128, T2), (198, RES_BS), (254, LT), (256, LT128)],
                "out": [(128, O_D), (160, O_C2), (256, O_C)]},
    (P8, 120): {"embed": [(128, E_D), (256, E_B)], **_I8_LAYER_T120, **_tail((126, T1_8), (128, T2_8), (256, LTI8)),
                "out": [(128, O_D), (160, O_C2), (256, O_C)]},
    (P9, 120): {"embed": [(128, E_D), (256, E_B)], **_I8_LAYER_T120, **_tail((64, R8W), (256, R4W)), "out": [(128, O_D), (256, O_I8)]},
    (P3, 196): {"embed": [(73, E_D), (256, E_A)], "qkv": [(256, "qkv_kernel")], "attn": [(63, "attn_kernel"), (256, "attn8_kernel")],
                "fc_ln": [(22, T8W), (72, T1), (73, T2), (113, RES_BS), (145, LT), (256, LT128)],
                "ffn1": [(22, T8W), (72, T1), (73, T2), (113, FF_A), (145, LT), (256, LT128)],
                "ffn2_ln": [(22, T8W), (72, T1), (73, T2), (113, RES_BS), (145, LT), (256, LT128)],
                "out": [(73, O_D), (91, O_C2), (256, O_C)]},
    (P8, 196): {"embed": [(78, E_D), (256, E_B)], "qkv": [(256, Q8Q)], "attn": [(256, CW)], **_tail((77, T1_8), (78, T2_8), (256, LTI8)),
                "out": [(78, O_D), (98, O_C2), (256, O_C)]},
    (P9, 196): {"embed": [(78, E_D), (256, E_B)], "qkv": [(256, Q8Q)], "attn": [(256, CW)], **_tail((39, R8W), (256, R4W)),
                "out": [(78, O_D), (256, O_I8)]},
    (P3, 30): {"embed": [(256, E_D)], "qkv": [(256, "qkv_kernel")], "attn": [(256, "attn_kernel")], **_tail((160, T8W), (256, T1)),
               "out": [(256, O_D)]},
    (P8, 30): {"embed": [(256, E_D)], "qkv": [(256, "qkv_i8_kernel")], "attn": [(256, "attn_kernel")], **_tail((256, T1_8)),
               "out": [(256, O_D)]},
}
EXPECT[(P9, 30)] = EXPECT[(P8, 30)]  # fc stays split-bf16 below 65 tokens: precision 9 runs precision 8's kernels
for _p in (P3, P8, P9):
    EXPECT[(_p, 150)] = EXPECT[(_p, 196)]  # same geometry: 151 and 197 tokens are both seven key tiles, 208 / 224 rows
# What a debug stop leaves in the tail slots, where that differs from a full pass (aligned geometry: T=120 only):
#   split-bf16 from B = 199: the stopped layer runs the three GEMMs on 128-token tiles (the fused tail skips debug stops);
#   precision 9, a Q/K/V stop: the product path's int8-only rows are off, so the layers before it take the non-resident fc8 tail.
DEBUG_EXPECT = {
    (P3, 120, (3, "out")): {"fc_ln": [(198, None), (256, RES_B)], "ffn1": [(198, None), (256, FF_A)], "ffn2_ln": [(198, None), (256, RES_B)]},
    (P9, 120, (3, "k")): {"fc_ln": [(64, N8W), (256, N4W)]},
}
# Names the library can record that no configuration of the parity precisions (3, 8, 9) reaches in the product build.
UNREACHABLE = {
    "attn_layer_i8h_kernel": "carve() aligns every buffer to 256 B, so att_img is set whenever Lp = 128, and attn_proj2_i8 takes every "
                             "grid attn_layer_i8h would: both bounds are 192 blocks on the same nw * H * 2",
    "attn_core_i8_kernel": "the four-wave int8 attention core: only a variant build with EGOEGO_CORE4=1 dispatches to it",
    "gemm_kernel:EpiResLN<CfgBt>": "precision 1 only: with two operand planes every grid of at most 160 32-token blocks takes the fused "
                                   "small-batch tail",
    "gemm_kernel:EpiTiled<CfgAh>": "precision 1 only (same reason as EpiResLN<CfgBt>)",
}


def _lookup(ranges, B):
    for last, name in ranges:
        if B <= last:
            return name
    raise AssertionError(f"B={B} beyond the table")


def expected_names(prec, T, B):
    return {s: _lookup(EXPECT[(prec, T)][s], B) for s in SLOTS}


def _table_names():
    names = {n for e in EXPECT.values() for r in e.values() for _, n in r}
    names |= {n for e in DEBUG_EXPECT.values() for r in e.values() for _, n in r if n is not None}
    return names


def recorded_names():
    """Every string literal the library assigns to a c->last_kernel[...] slot (ternaries and chained assignments included)."""
    src = open(HIP_SRC).read()
    src = re.sub(r"//[^\n]*", "", src)
    names = set()
    for m in re.finditer(r"c->last_kernel\[[^\]]+\]\s*=([^;]*);", src):
        names |= set(re.findall(r'"([^"]*)"', m.group(1)))
    names.discard("")  # (the reset at context creation)
    return names


# ------------------------------------------------------------------------------------------------ Philox reference
M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Random123's Philox4x32-10, as common.h runs it.  ctr: four uint32 arrays (broadcast), key: two uint32 -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def philox_normal4(seed, c0, c1, c2, c3):
    """common.h philox_normal4: (0, 1] uniforms formed in float32 exactly as the kernel forms them, then Box-Muller in float64
    (v_sin_f32 / v_cos_f32 take their argument in turns: sin(2 pi u)).  -> [..., 4] float64."""
    r = philox4x32_10((c0, c1, c2, c3), (seed & 0xFFFFFFFF, seed >> 32))
    inv = np.float32(2.0 ** -32)
    u0 = np.minimum((r[0].astype(np.float32) + np.float32(1.0)) * inv, np.float32(1.0)).astype(np.float64)
    u2 = np.minimum((r[2].astype(np.float32) + np.float32(1.0)) * inv, np.float32(1.0)).astype(np.float64)
    u1 = (r[1].astype(np.float32) * inv).astype(np.float64)
    u3 = (r[3].astype(np.float32) * inv).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([ra * np.cos(2 * np.pi * u1), ra * np.sin(2 * np.pi * u1), rb * np.cos(2 * np.pi * u3), rb * np.sin(2 * np.pi * u3)], -1)


def philox_noise(seed, t, window_offset, B, T, D=198):
    """The noise EpiOut draws for x[b, frame, f]: philox_normal4(seed; f >> 2, frame, window_offset + b, t[b])[f & 3].  -> [B, T, D]."""
    t = np.broadcast_to(np.asarray(t, dtype=np.int64), (B,))
    g = np.arange((D + 3) // 4, dtype=np.uint64)[None, None, :]
    fr = np.arange(T, dtype=np.uint64)[None, :, None]
    w = ((window_offset + np.arange(B, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint64)[:, None, None]
    z = philox_normal4(seed, g, fr, w, t.astype(np.uint64)[:, None, None])
    return z.reshape(B, T, -1)[..., :D]


# ------------------------------------------------------------------------------------------------ CPU tests
def test_every_recorded_kernel_name_is_swept_or_declared_unreachable():
    rec = recorded_names()
    table = _table_names()
    assert not (table & set(UNREACHABLE)), table & set(UNREACHABLE)
    assert rec == table | set(UNREACHABLE), {"recorded, in neither the table nor UNREACHABLE": sorted(rec - table - set(UNREACHABLE)),
                                            "in the table or UNREACHABLE, never recorded": sorted((table | set(UNREACHABLE)) - rec)}


def test_dispatch_constants_are_the_ones_the_table_assumes():
    src = open(HIP_SRC).read()
    for name, want in DISPATCH_CONSTANTS.items():
        m = re.search(rf"#define {name} (\d+)", src) or re.search(rf"static const int {name} = (\d+);", src)
        assert m is not None, name
        assert int(m.group(1)) == want, (name, m.group(1), want)


def test_table_covers_every_range_of_every_slot():
    """Every range of every slot holds at least one swept B: each name is reached and each threshold is seen from both sides."""
    for (prec, T), slots in EXPECT.items():
        if T == 150:  # (T=196's table: T=150 adds a second window length of that geometry at a small and a large B)
            continue
        for s, ranges in slots.items():
            assert ranges[-1][0] >= max(SWEEP_B[T]), (prec, T, s)
            lo = 1
            for last, name in ranges:
                assert any(lo <= b <= last for b in SWEEP_B[T]), (prec, T, s, name, lo, last)
                lo = last + 1
    for (prec, T, _), slots in DEBUG_EXPECT.items():
        for s, ranges in slots.items():
            lo = 1
            for last, name in ranges:
                assert any(lo <= b <= last for b in SWEEP_B[T]), (prec, T, s, name)
                lo = last + 1


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
], ids=["zero", "ones", "pi"])
def test_philox_reference_known_answers(ctr, key, want):
    """Random123's published Philox4x32-10 known-answer vectors (kat_vectors)."""
    got = philox4x32_10(ctr, key)
    assert tuple(int(v) for v in got) == want


def test_philox_normal_reference_is_standard_normal():
    z = philox_noise((7 << 32) | 3, [999, 500, 1, 0] * 16, 1000, 64, 120).ravel()
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3 and abs((z ** 4).mean() - 3) < 0.05
    # the partial last group (features 196, 197) draws its own counter: not a copy of any other group's first two values
    zz = philox_noise(5, 1, 0, 2, 3)
    for g in range(49):
        assert not np.allclose(zz[..., 196:198], zz[..., 4 * g:4 * g + 2])


# ------------------------------------------------------------------------------------------------ GPU: the sweep
def _model(T, precision):
    cfg = ModelConfig(max_timesteps=T + 1)
    sd = make_weights(cfg, 0)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=False)
    m.hip_precision = precision
    return sd, m.cuda()


def _hm(a, H=4):
    """oracle Q / K / V taps [H * b, L, 256] (head-major) -> [b, H, L, 256]"""
    n, L, d = a.shape
    return a.view(H, n // H, L, d).permute(1, 0, 2, 3)


@pytest.fixture(scope="module", params=[120, 196, 30, 150], ids=lambda T: f"T{T}")
def ref(request):
    """One seeded input set of 256 windows per T and the fp32 oracle over all of them, once: the denoiser output, the taps of layers 0
    and 3 and one p_sample step with injected noise.  Kept on the GPU."""
    T, B, H = request.param, 256, 4
    cfg = ModelConfig(max_timesteps=T + 1)
    sd = make_weights(cfg, 0)
    sched = O.make_schedule(1000)
    g = torch.Generator().manual_seed(4000 + T)
    x, xc = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    nz = torch.randn(B, T, 198, generator=g)
    out, ps = [], []
    taps = {"embed": []}
    for li in (0, 3):
        taps.update({(li, s): [] for s in ("q", "k", "v", "attn_out", "attn_ln", "ffn_hidden", "out")})
    with torch.no_grad():
        for c0 in range(0, B, 32):
            sl = slice(c0, c0 + 32)
            tp = {}
            out.append(O.denoise(sd, torch.cat((x[sl], xc[sl]), -1), t[sl], taps=tp))
            taps["embed"].append(tp["embed"])
            for li in (0, 3):
                lt = tp[f"layer{li}"]
                taps[(li, "q")].append(_hm(lt["q"]) / 16.0)
                taps[(li, "k")].append(_hm(lt["k"]))
                taps[(li, "v")].append(_hm(lt["v"]))
                for s in ("attn_out", "attn_ln", "ffn_hidden", "out"):
                    taps[(li, s)].append(lt[s])
            del tp
            ps.append(O.p_sample(sd, sched, x[sl], t[sl], xc[sl], nz[sl]))
    dev = "cuda"
    r = {"T": T, "x": x.to(dev), "xc": xc.to(dev), "t": t.to(dev), "nz": nz.to(dev),
         "out": torch.cat(out).to(dev), "p_sample": torch.cat(ps).to(dev),
         "taps": {k: torch.cat(v).contiguous().to(dev) for k, v in taps.items()}}
    yield r
    r.clear()
    torch.cuda.empty_cache()


@pytest.fixture(params=[P3, P8, P9], ids=["bf16x3", "i8x3", "i8x3fc"])
def prec(request):
    return request.param


def _engine(T, prec):
    sd, m = _model(T, prec)
    eng = m.hip_engine()
    assert m.hip_precision_used == prec and m._slot.plan["flags"] == 0, (m.hip_precision_used, m._slot.plan)
    return m, eng


def _per_window(got, want):
    """max |got - want| of every window (dim 0) -> [B]"""
    return (got - want).abs().flatten(1).amax(1)


def _worst(errs):
    w = int(torch.argmax(errs))
    return w, float(errs[w])


def _row_relative(prec, T):
    """Where a stop is held to 3e-4 of its row maximum (and 8e-4 absolute) instead of 3e-4 absolute: test_stagewise_against_oracle's
    rule for precision 9, and precision 8 outside 65..128 tokens.  There precision 8 runs the int8 operand images of precision 9's
    attention kernels (qkv_i8q + attn_core_i8w at seven key tiles, qkv_i8 at one), whose error scales with the row maximum: over 256
    windows it reaches 4.0e-4 absolute (0.attn_out, T=196), 3.1e-4 (0.attn_out, T=150) and 3.3e-4 (3.k, T=30) — row-relative well
    inside 3e-4 — while every stop at T=120 stays under 3e-4 absolute."""
    return prec == P9 or (prec == P8 and T != 120)


def _stage_errors(prec, T, got, want):
    """(per-window value the bar applies to, bar, per-window max abs error) — test_stagewise_against_oracle's rule."""
    d = (got - want).abs()
    if _row_relative(prec, T):
        rel = d.amax(-1) / want.abs().amax(-1).clamp_min(1.0)
        return rel.flatten(1).amax(1), STAGE_TOL, d.flatten(1).amax(1)
    e = d.flatten(1).amax(1)
    return e, STAGE_TOL, e


# sub-batch windows against the same windows of the B = 256 run: bit-equal in every configuration (integer contractions, one summation
# order per output element whatever the tiling; measured on MI355X)


@pytest.mark.gpu
def test_dispatch_sweep_every_window_against_oracle(ref, prec):
    T = ref["T"]
    m, eng = _engine(T, prec)
    x, xc, t, nz = ref["x"], ref["xc"], ref["t"], ref["nz"]
    big = {}
    report = []
    for B in sorted(SWEEP_B[T], reverse=True):  # B = 256 first: every sub-batch is compared with it
        cfg_id = f"precision {prec} T={T} B={B}"
        xb, xcb, tb = x[:B].contiguous(), xc[:B].contiguous(), t[:B].contiguous()
        y = eng.denoise(xb, xcb, tb)
        names = {s: eng.last_kernel(s) for s in SLOTS}
        want = expected_names(prec, T, B)
        assert names == want, (cfg_id, {s: (names[s], want[s]) for s in SLOTS if names[s] != want[s]})
        e = _per_window(y, ref["out"][:B])
        w, ev = _worst(e)
        assert ev < POSE_TOL, f"{cfg_id}: denoiser output, window {w}: max |HIP - oracle| = {ev:.3e}"
        worst_stage = ("", -1, 0.0, 0.0)
        stops = [(0, "embed")] + [(li, s) for li in (0, 3) for s in ("q", "k", "v", "attn_out", "attn_ln", "ffn_hidden", "out")]
        for li, st in stops:
            got = eng.debug_stage(xb, xcb, tb, li, st)
            tap = ref["taps"]["embed" if st == "embed" else (li, st)][:B]
            val, bar, absd = _stage_errors(prec, T, got, tap)
            sw, sv = _worst(val)
            name = st if st == "embed" else f"{li}.{st}"
            rel = _row_relative(prec, T)
            assert sv <= bar if rel else sv < bar, f"{cfg_id}: stage {name}, window {sw}: error {sv:.3e} (bar {bar:.0e})"
            aw, av = _worst(absd)
            if rel:
                assert av < 8e-4, f"{cfg_id}: stage {name}, window {aw}: max abs error {av:.3e} (bar 8e-4)"
            if sv > worst_stage[3]:
                worst_stage = (name, sw, av, sv)
            dbg = DEBUG_EXPECT.get((prec, T, (li, st)))
            if dbg is not None:
                for s, ranges in dbg.items():
                    wn = _lookup(ranges, B)
                    if wn is not None:
                        assert eng.last_kernel(s) == wn, (cfg_id, f"after the {name} stop", s, eng.last_kernel(s), wn)
        xs = xb.clone()
        eng.p_sample_(xs, xcb, tb, noise=nz[:B].contiguous())
        pe = _per_window(xs, ref["p_sample"][:B])
        pw, pv = _worst(pe)
        assert pv < POSE_TOL, f"{cfg_id}: p_sample step, window {pw}: max |HIP - oracle| = {pv:.3e}"
        if B == 256:
            big = {"out": y, "p_sample": xs}
            eq = "-"
        else:
            d_out = _per_window(y, big["out"][:B])
            d_ps = _per_window(xs, big["p_sample"][:B])
            bits = torch.equal(y, big["out"][:B]) and torch.equal(xs, big["p_sample"][:B])
            assert bits, f"{cfg_id}: not bit-equal to the same windows of B=256 (denoise {_worst(d_out)}, p_sample {_worst(d_ps)})"
            eq = "bits"
        report.append(f"  B={B:3d} out {ev:.2e} (w{w}) | stage {worst_stage[0]} {worst_stage[3]:.2e} (w{worst_stage[1]}, abs {worst_stage[2]:.2e})"
                      f" | p_sample {pv:.2e} (w{pw}) | vs B=256 {eq} | {names}")
    print(f"\ndispatch sweep precision {prec} T={T}: worst window errors\n" + "\n".join(reversed(report)))


@functools.lru_cache(maxsize=2)
def _masked_ref(T):
    """256 windows, each of a random valid length, and the oracle's masked denoiser output over them (once per T)."""
    B = 256
    sd = make_weights(ModelConfig(max_timesteps=T + 1), 0)
    g = torch.Generator().manual_seed(5000 + T)
    x, xc = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    pm = (torch.arange(T + 1)[None, :] <= lens[:, None])[:, None, :]  # the time token + the first lens[b] frames
    with torch.no_grad():
        want = torch.cat([O.denoise(sd, torch.cat((x[c:c + 32], xc[c:c + 32]), -1), t[c:c + 32], padding_mask=pm[c:c + 32])
                          for c in range(0, B, 32)])
    return x, xc, t, pm, lens, want


@pytest.mark.gpu
@pytest.mark.parametrize("T", [120, 196])
def test_padding_mask_every_window_against_oracle(T, prec):
    """B = 256, each window a random valid length: the mask enters every layer's two LayerNorm epilogues of the product kernels."""
    x, xc, t, pm, lens, want = _masked_ref(T)
    sd, m = _model(T, prec)
    y = m.denoise(x.cuda(), t.cuda(), xc.cuda(), padding_mask=pm.cuda()).cpu()
    assert m.hip_precision_used == prec
    w, ev = _worst(_per_window(y, want))
    print(f"\npadding mask precision {prec} T={T} B=256: worst window {w}: {ev:.3e}")
    assert ev < POSE_TOL, f"precision {prec} T={T} B=256 padding mask, window {w} (length {int(lens[w])}): {ev:.3e}"


# ------------------------------------------------------------------------------------------------ GPU: the Philox stream
PHILOX_SEED = 0x9E3779B97F4A7C15  # high 32 bits non-zero: both key words matter
PHILOX_T = (999, 500, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [120, 196])
@pytest.mark.parametrize("precision", [P3, P9], ids=["bf16x3", "i8x3fc"])
def test_philox_noise_matches_reference(precision, T):
    """(x after a NOISE_PHILOX step - x after a NOISE_NONE step) / sigma_t is the kernel's draw, for every window, frame and feature.
    B = 256 runs linear_out on the ring GEMM / int8 kernel, B = 64 on the direct-operand kernel: both feed EpiOut."""
    sd, m = _model(T, precision)
    eng = m.hip_engine()
    sched = O.make_schedule(1000)
    sig = torch.exp(0.5 * sched["posterior_log_variance_clipped"].double())
    g = torch.Generator().manual_seed(77 + T)
    x0 = torch.randn(256, T, 198, generator=g).cuda()
    xc = torch.randn(256, T, 198, generator=g).cuda()
    worst = 0.0
    for B in (256, 64):
        t = torch.tensor([PHILOX_T[b % 3] for b in range(B)])
        for off in (0, 1000):
            a, b0 = x0[:B].clone(), x0[:B].clone()
            eng.p_sample_(a, xc[:B].contiguous(), t.cuda(), noise_mode=_lib.NOISE_PHILOX, seed=PHILOX_SEED, window_offset=off)
            eng.p_sample_(b0, xc[:B].contiguous(), t.cuda(), noise_mode=_lib.NOISE_NONE)
            z = ((a - b0).double().cpu() / sig[t].view(B, 1, 1)).numpy()
            want = philox_noise(PHILOX_SEED, t.numpy(), off, B, T)
            d = np.abs(z - want)
            wi = np.unravel_index(int(d.argmax()), d.shape)
            assert d.max() < 1e-4, f"precision {precision} T={T} B={B} window_offset={off}: window {wi[0]} frame {wi[1]} feature {wi[2]} " \
                                   f"(t={int(t[wi[0]])}): kernel {z[wi]:.6f}, reference {want[wi]:.6f}"
            worst = max(worst, float(d.max()))
    # the multi-step loop (captured step, timestep and key from the device-resident step state)
    a, b0 = x0[:64].clone(), x0[:64].clone()
    eng.sample_loop_(a, xc[:64].contiguous(), 500, 1, noise_mode=_lib.NOISE_PHILOX, seed=PHILOX_SEED, window_offset=7)
    eng.sample_loop_(b0, xc[:64].contiguous(), 500, 1, noise_mode=_lib.NOISE_NONE)
    z = ((a - b0).double().cpu() / sig[500]).numpy()
    d = np.abs(z - philox_noise(PHILOX_SEED, 500, 7, 64, T))
    assert d.max() < 1e-4, f"sample loop: {d.max():.3e}"
    worst = max(worst, float(d.max()))
    # DDIM, eta = 1: the noisy step draws with the DDIM timestep.  Its draw injected from the reference gives the kernel's own result,
    # and the restatement (oracle.ddim_loop, which computes sig itself) agrees within the pose bar
    ts = [600, 300]
    B = 64
    xa = x0[:B].clone()
    eng.ddim_loop_(xa, xc[:B].contiguous(), ts, eta=1.0, noise_mode=_lib.NOISE_PHILOX, seed=PHILOX_SEED, window_offset=1000)
    ref_z = torch.zeros(2, B, T, 198)
    ref_z[0] = torch.from_numpy(philox_noise(PHILOX_SEED, ts[0], 1000, B, T)).float()
    xb = x0[:B].clone()
    eng.ddim_loop_(xb, xc[:B].contiguous(), ts, eta=1.0, noise=ref_z.cuda(), noise_mode=_lib.NOISE_INJECTED)
    xz = x0[:B].clone()
    eng.ddim_loop_(xz, xc[:B].contiguous(), ts, eta=1.0, noise=torch.zeros_like(ref_z).cuda(), noise_mode=_lib.NOISE_INJECTED)
    dd = (xa - xb).abs().max().item()
    assert (xa - xz).abs().max().item() > 1e-2  # the noise matters to the result
    # (the second, deterministic step runs the denoiser on the two results: in split-bf16 the draws' ~1e-6 differences stay that small;
    # precision 9's int8 rows turn them into up to 2.4e-4 (measured) — a wrong counter moves the noisy step by O(sig))
    bar = 1e-4 if precision == P3 else POSE_TOL
    assert dd < bar, f"DDIM eta=1: Philox against the reference draws injected: {dd:.3e}"
    with torch.no_grad():
        want = O.ddim_loop(sd, sched, x0[:B].cpu(), xc[:B].cpu(), ts, eta=1.0, noise=ref_z)
    assert (xa.cpu() - want).abs().max().item() < POSE_TOL
    print(f"\nPhilox precision {precision} T={T}: max |kernel draw - reference| = {worst:.3e}; DDIM eta=1 {dd:.3e}")
