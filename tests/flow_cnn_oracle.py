"""CPU restatement of the reference's optical-flow feature extractor (egoego/model/resnet.py FeatureExtractor: torchvision's
resnet18 with fc = Linear(512, 512)) in eval mode, on a state dict, with plain torch.nn.functional ops in fp64 or fp32.

torchvision is not installed here, so no golden can come from the reference's own class: this file restates its forward from
torchvision's resnet18 definition (BasicBlock: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity), downsample = 1x1/2 conv + BN
on block 0 of layer2..4) and the reference's input prep (append a zero third channel, reshape to [-1, 224, 224, 3], permute to
NCHW).  BatchNorm uses the running statistics (training=False), eps 1e-5.

The network is also available stage by stage: stage(sd, 0, flow, mode) is stem + BN + ReLU + max-pool, stage(sd, 1..4, x, mode)
is layer1..4 on an NCHW input, head(sd, x, mode) is the average pool and the fc.  `mode`:
  "f64"   plain fp64 ops,
  "f32"   plain fp32 ops (F.batch_norm in fp32),
  "emul"  what the split-bf16 kernels compute, without their fp32 accumulation: every convolution and the fc as
          conv(x_hi, w_hi) + conv(x_lo, w_hi) + conv(x_hi, w_lo) in fp64, hi = bf16(fp32(v)), lo = bf16(fp32(v) - hi); the
          BatchNorm as the fold scale = w / sqrt(var + 1e-5), shift = b - mean * scale in fp64; then the residual; then ReLU.
  "acc"   "emul" with the kernel's fp32 arithmetic as well.  One MFMA (16 consecutive k, k = (kh * KW + kw) * Cin + c) adds its
          products to the fp32 accumulator as two halves of 8, each half summed exactly and added with one rounding; the three
          MFMAs of a step run hi*hi, lo*hi, hi*lo, step after step in the kernel's K order.  The epilogue is fp32 (one fma for
          scale and shift, then the residual, then ReLU), the average pool a running fp32 sum.  The matrix unit's inner order
          is not documented: the two halves were found by comparison with the kernel's output (the pooled stem is then
          bit-equal in 99 % of its elements, the features from layer4 in 92 %, the stages of four chained convolutions in
          35 to 55 %), so this is a model of the kernel's accumulation error, close to but not its bits.
forward() is the chain of the "f64" or "f32" stages.  `defect` = (kind, convolution name) changes one convolution of the "emul"
stage on purpose (DEFECT_KINDS): what the tests' bars have to catch.
"""
import torch
import torch.nn.functional as F

PREFIX = "cnn.resnet."
EPS = 1e-5
MODES = {"f64": torch.float64, "f32": torch.float32, "emul": torch.float64, "acc": torch.float64}
DEFECT_KINDS = ("drop_act_lo", "drop_w_lo", "transpose_taps", "swap_xy", "replicate_pad", "res_after_relu", "no_eps",
                "downsample_from_1")
# not a defect (the tests show it stays under the bar): the weight-lo plane truncated to bf16 instead of rounded
VARIANT_KINDS = ("trunc_w_lo",)


def prep(flow, dtype=torch.float64):
    """[..., 224, 224, 2] -> [N, 3, 224, 224] as FeatureExtractor.forward builds it."""
    of = torch.as_tensor(flow)
    of = torch.cat((of, torch.zeros(of.shape[:-1] + (1,), dtype=of.dtype)), dim=-1)
    return of.reshape(-1, 224, 224, 3).permute(0, 3, 1, 2).to(dtype)


def _bn(sd, name, x, dtype):
    g = lambda k: sd[PREFIX + name + "." + k].to(dtype)  # noqa: E731
    return F.batch_norm(x, g("running_mean"), g("running_var"), g("weight"), g("bias"), training=False, momentum=0.0, eps=1e-5)


def _conv(sd, name, x, stride, pad, dtype):
    return F.conv2d(x, sd[PREFIX + name + ".weight"].to(dtype), stride=stride, padding=pad)


def split(x, trunc_lo=False):
    """fp64 -> (hi, lo) in fp64: the two bf16 numbers a split-bf16 MFMA reads of the fp32 value (train_oracle._split)."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = x32 - hi
    if trunc_lo:
        lo = (lo.view(torch.int32) & -65536).view(torch.float32)
    else:
        lo = lo.to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


def _emul_conv(sd, conv, bn, x, stride, pad, res=None, relu=True, defect=None):
    """One convolution + folded BatchNorm (+ residual) (+ ReLU) as the kernel's epilogue orders them, in fp64 on split operands."""
    kind = defect[0] if defect is not None and defect[1] == conv else None
    assert kind is None or kind in DEFECT_KINDS + VARIANT_KINDS, kind
    w = sd[PREFIX + conv + ".weight"].to(torch.float64)
    if kind == "transpose_taps":
        w = w.transpose(-1, -2)
    if kind == "swap_xy":
        x = x[:, [1, 0, 2]]
    if kind == "replicate_pad":
        x, pad = F.pad(x, (pad, pad, pad, pad), mode="replicate"), 0
    if kind == "downsample_from_1":
        assert stride == 2
        x = torch.cat((x[:, :, 1:], x[:, :, -1:]), 2)
        x = torch.cat((x[:, :, :, 1:], x[:, :, :, -1:]), 3)
    xh, xl = split(x)
    wh, wl = split(w, trunc_lo=kind == "trunc_w_lo")
    y = F.conv2d(xh, wh, stride=stride, padding=pad)
    if kind != "drop_act_lo":
        y = y + F.conv2d(xl, wh, stride=stride, padding=pad)
    if kind != "drop_w_lo":
        y = y + F.conv2d(xh, wl, stride=stride, padding=pad)
    g = lambda k: sd[PREFIX + bn + "." + k].to(torch.float64)  # noqa: E731
    scale = g("weight") / torch.sqrt(g("running_var") + (0.0 if kind == "no_eps" else EPS))
    shift = g("bias") - g("running_mean") * scale
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    if kind == "res_after_relu":
        assert res is not None and relu
        return F.relu(y) + res
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def _acc_gemm(a, w):
    """a [M, K] x w [Cout, K] (fp64 holding fp32 values, K in the kernel's order) -> fp32 [M, Cout], accumulated as the kernel does."""
    K = a.shape[1]
    Kp = (K + 15) // 16 * 16
    a, w = F.pad(a, (0, Kp - K)), F.pad(w, (0, Kp - K))
    ah, al = split(a)
    wh, wl = (t.T.contiguous() for t in split(w))
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(0, Kp, 16):
        for p, q in ((ah, wh), (al, wh), (ah, wl)):
            for j in (k, k + 8):
                acc = (acc.double() + p[:, j:j + 8] @ q[j:j + 8]).float()
    return acc


def _acc_conv(sd, conv, bn, x, stride, pad, res=None, relu=True):
    """_emul_conv in the kernel's fp32 arithmetic; x and res hold fp32 values, and so does the result."""
    w = sd[PREFIX + conv + ".weight"].to(torch.float64)
    if conv == "conv1":  # the kernel drops the all-zero third channel
        x, w = x[:, :2], w[:, :2]
    N, Cin = x.shape[:2]
    Cout, _, KH, KW = w.shape
    OH = (x.shape[2] + 2 * pad - KH) // stride + 1
    cols = F.unfold(x, (KH, KW), padding=pad, stride=stride)  # [N, Cin * KH * KW, L], c-major
    L = cols.shape[2]
    cols = cols.view(N, Cin, KH * KW, L).permute(0, 3, 2, 1).reshape(N * L, KH * KW * Cin)
    acc = _acc_gemm(cols, w.permute(0, 2, 3, 1).reshape(Cout, -1))
    g = lambda k: sd[PREFIX + bn + "." + k].to(torch.float64)  # noqa: E731
    scale = g("weight") / torch.sqrt(g("running_var") + EPS)
    shift = (g("bias") - g("running_mean") * scale).float().double()
    v = (acc.double() * scale.float().double() + shift).float()
    v = v.view(N, L, Cout).permute(0, 2, 1).reshape(N, Cout, OH, L // OH)
    if res is not None:
        v = v + res.float()
    return (F.relu(v) if relu else v).double()


def stage(sd, i, x, mode="f64", defect=None):
    """Stage i of the network in `mode`.  i = 0: flow [N, 224, 224, 2] -> the pooled stem [N, 64, 56, 56]; i = 1..4: the NCHW
    output of stage i - 1 -> layer i's output.  The result has the mode's dtype."""
    dtype = MODES[mode]
    emul = mode == "emul"
    assert defect is None or emul
    if mode == "acc":
        if i == 0:
            return F.max_pool2d(_acc_conv(sd, "conv1", "bn1", prep(x, dtype), 2, 3), 3, 2, 1)
        x = torch.as_tensor(x).to(dtype)
        for b in range(2):
            p = f"layer{i}.{b}."
            ds = i > 1 and b == 0
            h = _acc_conv(sd, p + "conv1", p + "bn1", x, 2 if ds else 1, 1)
            idn = _acc_conv(sd, p + "downsample.0", p + "downsample.1", x, 2, 0, relu=False) if ds else x
            x = _acc_conv(sd, p + "conv2", p + "bn2", h, 1, 1, res=idn)
        return x
    if i == 0:
        x = prep(x, dtype)
        if emul:
            x = _emul_conv(sd, "conv1", "bn1", x, 2, 3, defect=defect)
        else:
            x = F.relu(_bn(sd, "bn1", _conv(sd, "conv1", x, 2, 3, dtype), dtype))
        return F.max_pool2d(x, 3, 2, 1)
    x = torch.as_tensor(x).to(dtype)
    li = i
    for b in range(2):
        p = f"layer{li}.{b}."
        s = 2 if li > 1 and b == 0 else 1
        ds = li > 1 and b == 0
        if emul:
            h = _emul_conv(sd, p + "conv1", p + "bn1", x, s, 1, defect=defect)
            idn = _emul_conv(sd, p + "downsample.0", p + "downsample.1", x, 2, 0, relu=False, defect=defect) if ds else x
            x = _emul_conv(sd, p + "conv2", p + "bn2", h, 1, 1, res=idn, defect=defect)
        else:
            h = F.relu(_bn(sd, p + "bn1", _conv(sd, p + "conv1", x, s, 1, dtype), dtype))
            h = _bn(sd, p + "bn2", _conv(sd, p + "conv2", h, 1, 1, dtype), dtype)
            idn = x
            if ds:
                idn = _bn(sd, p + "downsample.1", _conv(sd, p + "downsample.0", x, 2, 0, dtype), dtype)
            x = F.relu(h + idn)
    return x


def head(sd, x, mode="f64", defect=None):
    """The NCHW output of stage 4 -> features [N, 512]: global average pool, then the fc."""
    dtype = MODES[mode]
    if mode == "acc":
        px = torch.as_tensor(x).float().flatten(2)  # [N, 512, 49]: pixels summed in order, then / 49
        s = torch.zeros(px.shape[:2], dtype=torch.float32)
        for q in range(px.shape[2]):
            s = s + px[:, :, q]
        s = (s / float(px.shape[2])).double()
        acc = _acc_gemm(s, sd[PREFIX + "fc.weight"].double())
        return (acc.double() + sd[PREFIX + "fc.bias"].double()).float().double()
    x = torch.flatten(F.adaptive_avg_pool2d(torch.as_tensor(x).to(dtype), 1), 1)
    w, b = sd[PREFIX + "fc.weight"].to(dtype), sd[PREFIX + "fc.bias"].to(dtype)
    if mode != "emul":
        return F.linear(x, w, b)
    kind = defect[0] if defect is not None and defect[1] == "fc" else None
    assert kind in (None, "drop_act_lo", "drop_w_lo", "trunc_w_lo"), kind
    xh, xl = split(x)
    wh, wl = split(w, trunc_lo=kind == "trunc_w_lo")
    y = xh @ wh.T
    if kind != "drop_act_lo":
        y = y + xl @ wh.T
    if kind != "drop_w_lo":
        y = y + xh @ wl.T
    return y + b


def forward(sd, flow, dtype=torch.float64):
    """flow [N, 224, 224, 2] -> (features [N, 512], [stem, layer1, layer2, layer3, layer4] activations NCHW) in `dtype`."""
    mode = {torch.float64: "f64", torch.float32: "f32"}[dtype]
    x = flow
    stages = []
    for i in range(5):
        x = stage(sd, i, x, mode)
        stages.append(x)
    return head(sd, x, mode), stages
