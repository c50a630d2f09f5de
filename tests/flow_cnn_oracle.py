"""CPU restatement of the reference's optical-flow feature extractor (egoego/model/resnet.py FeatureExtractor: torchvision's
resnet18 with fc = Linear(512, 512)) in eval mode, on a state dict, with plain torch.nn.functional ops in fp64 or fp32.

torchvision is not installed here, so no golden can come from the reference's own class: this file restates its forward from
torchvision's resnet18 definition (BasicBlock: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity), downsample = 1x1/2 conv + BN
on block 0 of layer2..4) and the reference's input prep (append a zero third channel, reshape to [-1, 224, 224, 3], permute to
NCHW).  BatchNorm uses the running statistics (training=False), eps 1e-5.
"""
import torch
import torch.nn.functional as F

PREFIX = "cnn.resnet."


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


def forward(sd, flow, dtype=torch.float64):
    """flow [N, 224, 224, 2] -> (features [N, 512], [stem, layer1, layer2, layer3, layer4] activations NCHW) in `dtype`."""
    x = prep(flow, dtype)
    x = F.relu(_bn(sd, "bn1", _conv(sd, "conv1", x, 2, 3, dtype), dtype))
    x = F.max_pool2d(x, 3, 2, 1)
    stages = [x]
    for li in range(1, 5):
        for b in range(2):
            p = f"layer{li}.{b}."
            s = 2 if li > 1 and b == 0 else 1
            h = F.relu(_bn(sd, p + "bn1", _conv(sd, p + "conv1", x, s, 1, dtype), dtype))
            h = _bn(sd, p + "bn2", _conv(sd, p + "conv2", h, 1, 1, dtype), dtype)
            idn = x
            if li > 1 and b == 0:
                idn = _bn(sd, p + "downsample.1", _conv(sd, p + "downsample.0", x, 2, 0, dtype), dtype)
            x = F.relu(h + idn)
        stages.append(x)
    x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    feats = F.linear(x, sd[PREFIX + "fc.weight"].to(dtype), sd[PREFIX + "fc.bias"].to(dtype))
    return feats, stages
