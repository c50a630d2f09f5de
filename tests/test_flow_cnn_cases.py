"""The flow-CNN parity cases without a GPU: the staged oracle against the monolithic forward it replaced, the emulated
split-bf16 mode against fp64, the preconditions of the trained-like weights, non-finite input through the reference ops, and
the planted defects against the bars of flow_cnn_cases.cell (each must exceed its stage's bar somewhere).

Stages 1-4 and the head are isolated as on the GPU: their input is the previous stage's fp64 output rounded to fp32, which stands
in for the HIP path's own fp32 activations."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_cnn_cases as K
import flow_cnn_oracle as O

ORDINARY = (0, 1, 5, 6)  # the frames that are real flow fields: flow0, flow1, pm40, large


def _legacy_forward(sd, flow, dtype):
    """The oracle's forward as it was before it became a chain of stages, kept here word for word as the fixed point."""
    x = O.prep(flow, dtype)
    x = F.relu(O._bn(sd, "bn1", O._conv(sd, "conv1", x, 2, 3, dtype), dtype))
    x = F.max_pool2d(x, 3, 2, 1)
    stages = [x]
    for li in range(1, 5):
        for b in range(2):
            p = f"layer{li}.{b}."
            s = 2 if li > 1 and b == 0 else 1
            h = F.relu(O._bn(sd, p + "bn1", O._conv(sd, p + "conv1", x, s, 1, dtype), dtype))
            h = O._bn(sd, p + "bn2", O._conv(sd, p + "conv2", h, 1, 1, dtype), dtype)
            idn = x
            if li > 1 and b == 0:
                idn = O._bn(sd, p + "downsample.1", O._conv(sd, p + "downsample.0", x, 2, 0, dtype), dtype)
            x = F.relu(h + idn)
        stages.append(x)
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    feats = F.linear(x, sd[O.PREFIX + "fc.weight"].to(dtype), sd[O.PREFIX + "fc.bias"].to(dtype))
    return feats, stages


@functools.lru_cache(maxsize=None)
def _chain(wname):
    """(features, stages) in fp64 of all 7 frames (shared: not modified)."""
    return O.forward(K.weights(wname), K.frames(), torch.float64)


@functools.lru_cache(maxsize=None)
def _isolated(wname, i):
    """Stage i of all 7 frames on the stand-in input: (r64, emul, f32, acc, the input)."""
    x = torch.from_numpy(K.frames()) if i == 0 else _chain(wname)[1][i - 1].float().double()
    sd = K.weights(wname)
    return tuple(K.run(sd, i, x, m) for m in ("f64", "emul", "f32", "acc")) + (x,)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("wname", ["init", "trained_like1"])
def test_chained_stages_equal_the_monolithic_forward(wname, dtype):
    sd, fl = K.weights(wname), K.frames()[[0, 2, 4]]
    feats, stages = O.forward(sd, fl, dtype)
    ref, ref_stages = _legacy_forward(sd, fl, dtype)
    assert feats.dtype == dtype and torch.equal(feats, ref)
    assert len(stages) == 5
    for a, b in zip(stages, ref_stages):
        assert a.dtype == dtype and torch.equal(a, b)


def test_frames_are_the_seven_of_the_issue():
    fl = K.frames()
    assert fl.shape == (7, 224, 224, 2) and fl.dtype == np.float32 and len(K.FRAME_NAMES) == 7
    assert np.count_nonzero(fl[2]) == 6 and fl[2, 0, 0, 0] == 7 and fl[2, 223, 223, 0] == -9 and fl[2, 1, 222, 1] == 6
    assert (fl[3, ..., 0] == 3.25).all() and (fl[3, ..., 1] == -1.5).all() and not fl[4].any()
    assert abs(fl[5]).max() == 40.0 and (fl[5, 100:110, 100:110] == [40.0, -40.0]).all()
    assert abs(fl[6]).max() > 100.0


@pytest.mark.parametrize("wname", K.WEIGHT_SETS)
def test_emulated_split_bf16_lies_between_fp32_and_1e4(wname):
    """Per isolated stage and frame: e_32 <= e_emul <= 1e-4 (seen: about 9e-6).  The lower bound is not asked of the stem on the
    constant and the all-zero frame: their values are bf16 numbers, the lo plane is empty, and what is left of the emulation's
    error is the weights' split alone (on the all-zero frame: nothing, the stem is the folded shift)."""
    for i in range(6):
        r64, emul, f32, acc, _ = _isolated(wname, i)
        for n in range(7):
            c = K.cell(emul[n], r64[n], emul[n], f32[n])
            assert c["e_emul"] <= 1e-4, (i, n, c)
            if not (i == 0 and n in (3, 4)):
                assert c["e_32"] <= c["e_emul"], (i, n, c)
            # the kernel's own accumulation order is a small step from the emulation, and passes the bars it widens
            a = K.cell(acc[n], r64[n], emul[n], f32[n], acc[n])
            assert K.passes(a) and a["e_hip"] <= 1e-4, (i, n, a)


@pytest.mark.parametrize("seed", [1, 2])
def test_trained_like_meets_its_preconditions(seed):
    """Finite in fp64 and not all zero at every stage of every frame; at least 90 % of the channels live on the frames that are
    flow fields (the impulse, constant and all-zero frames leave much of the stem at its ReLU'd shift, a zero for about half of
    the channels, whatever the weights).  The recipe really reaches the regime it is for: variances under eps, folded scales over
    three decades, negative and zero scales."""
    wname = f"trained_like{seed}"
    sd = K.weights(wname)
    feats, stages = _chain(wname)
    assert torch.isfinite(feats).all()
    for i, s in enumerate(stages):
        assert torch.isfinite(s).all(), i
        C = s.shape[1]
        for n in range(7):
            r = s[n].reshape(C, -1)
            nr = r.pow(2).sum().sqrt()
            assert nr > 0, (i, n)
            live = int((r.pow(2).sum(1).sqrt() >= K.LIVE * nr / C ** 0.5).sum())
            if n in ORDINARY:
                assert live >= 0.9 * C, (i, n, live, C)
    var = sd[O.PREFIX + "bn1.running_var"].double()
    scale = sd[O.PREFIX + "bn1.weight"].double() / torch.sqrt(var + O.EPS)
    assert (var < O.EPS).sum() >= 2 and (scale < 0).sum() >= 8 and (scale == 0).sum() == 2
    nz = scale.abs()[scale != 0]
    assert nz.max() / nz.min() > 1e3
    assert torch.equal(sd[O.PREFIX + "fc.weight"], K.weights("init")[O.PREFIX + "fc.weight"])


@pytest.mark.parametrize("seed", [1, 2])
def test_trained_like_is_the_same_network_up_to_eps(seed):
    """The gains alone move the fp64 features of every frame by the weight of eps and nothing else: not equal, within 0.1 of
    the frame's norm (seen: 0.008 to 0.052).  With the four constant channels per BatchNorm the features of the seven frames
    agree to the loose 0.5 of their joint norm (seen: 0.30 and 0.24); frame by frame that distance is 0.24 to 0.88, largest on
    the constant and all-zero frames, and it is those channels, not eps, that make it."""
    a = _chain("init")[0]
    b = _chain(f"trained_like{seed}")[0]
    g, _ = O.forward(K.trained_like(seed, constant_channels=False), K.frames(), torch.float64)
    assert not torch.equal(a, b) and not torch.equal(a, g)
    for n in range(7):
        assert (a[n] - g[n]).norm() <= 0.1 * a[n].norm(), n
    assert (a - b).norm() <= 0.5 * a.norm()


@pytest.mark.parametrize("wname", ["init", "trained_like1"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_reference_ops_carry_a_non_finite_pixel_into_every_feature(wname, value):
    fl = K.frames()[:3].copy()
    fl[1, 100, 57, 0] = value
    feats, _ = O.forward(K.weights(wname), fl, torch.float64)
    assert not torch.isfinite(feats[1]).any()
    assert torch.isfinite(feats[[0, 2]]).all()


def _defect_cells(wname, defect):
    i = K.defect_stage(defect[1])
    r64, emul, f32, acc, x = _isolated(wname, i)
    got = K.run(K.weights(wname), i, x, "emul", defect)
    return [K.cell(got[n], r64[n], emul[n], f32[n], acc[n]) for n in range(7)]


@pytest.mark.parametrize("defect", K.DEFECTS, ids=lambda d: d[0] + "@" + d[1])
def test_every_planted_defect_exceeds_its_stage_bar(defect):
    """In at least one (weights, frame) cell, whole-stage or per channel (seen: 150 to 4e7 bars); an omitted eps by at least 10
    on the trained-like statistics (seen: 330 to 6e4; on `init` it is over the bar at the stem only and at 0.7 to 0.9 of it in
    layer2 and layer4: the gap this family closes)."""
    worst = {w: max(K.excess(c) for c in _defect_cells(w, defect)) for w in ("init", "trained_like1")}
    print(defect, {w: "%.3g" % v for w, v in worst.items()})
    assert max(worst.values()) > 1.0, worst
    if defect[0] == "no_eps":
        assert worst["trained_like1"] >= 10.0, worst


def test_all_defect_kinds_are_planted_and_the_stem_has_its_own():
    assert {d[0] for d in K.DEFECTS} == set(O.DEFECT_KINDS)
    assert {d[0] for d in K.DEFECTS if d[1] == "conv1"} >= {"transpose_taps", "swap_xy", "replicate_pad", "no_eps"}
    for kind in ("transpose_taps", "swap_xy", "replicate_pad"):  # gross on the stem: more than 1e4 bars
        assert max(K.excess(c) for c in _defect_cells("init", (kind, "conv1"))) > 1e4, kind


@pytest.mark.parametrize("conv", ["conv1", "layer2.0.conv1", "fc"])
def test_a_truncated_weight_lo_plane_is_no_defect(conv):
    """Truncating the weights' lo plane instead of rounding it doubles that one term's error: the stage as a whole stays under
    its bar (0.4 to 0.85).  Single channels do not (up to 7 bars on the stem, and up to 28 on single features of the fc, which
    have one number each): the per-channel bar tells another rounding of the same operands from the emulation, the whole-stage
    bar does not, which is why this variant is not listed as a defect."""
    for w in ("init", "trained_like1"):
        for c in _defect_cells(w, ("trunc_w_lo", conv)):
            assert c["whole"] < 1.0, (w, c)
