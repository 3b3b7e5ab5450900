"""A torch restatement of the reference YOLACT backbone (yolact/model/backbone.py:9-32): torchvision's
resnet18 — restated here from torch's own Conv2d / BatchNorm2d / MaxPool2d under torchvision's
attribute names, because torchvision is not available to these tests — tapped where
create_feature_extractor taps it: the outputs of layer2.1.bn2, layer3.1.bn2 and layer4.1.bn2, each
before the block's residual add and ReLU. Parity with torchvision itself is NOT pinned by any
fixture: the BasicBlock (conv3x3(stride) - bn - relu - conv3x3 - bn, + identity or
downsample = conv1x1(stride) - bn, relu) and the stem (conv 7x7 / 2 / 3, bn, relu, MaxPool2d(3, 2, 1))
are restated from torchvision's resnet.py.

`ResNet18Ref().double()(img)` is the float64 reference. `forward(img, lowp=dtype)` emulates the
native plan's rounding points (as tools/precision_budget.py does): BatchNorm folded in double, the
folded weights rounded to `dtype`, every tensor the plan stores rounded to `dtype`, fp32 accumulation
and fp32 bias / residual sums. `tap` selects what is returned per tapped block: "bn2" (the reference),
or the deliberately wrong "add" (after the residual add) and "relu" (after the ReLU)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicBlock(nn.Module):
    def __init__(self, cin, c, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(c)
        self.downsample = None
        if stride != 1 or cin != c:
            self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), nn.BatchNorm2d(c))


def _fold(conv, bn):
    """(weight, shift) of conv + eval BatchNorm, in double."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return conv.weight.double() * s[:, None, None, None], bn.bias.double() - bn.running_mean.double() * s


class ResNet18Ref(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for L in range(1, 5):
            c = 64 << (L - 1)
            setattr(self, f"layer{L}", nn.Sequential(BasicBlock(cin, c, 2 if L > 1 else 1), BasicBlock(c, c, 1)))
            cin = c
        self.eval()

    def forward(self, x, lowp=None, tap="bn2"):
        if lowp is None:
            q = lambda t: t
            cbn = lambda conv, bn, t: bn(conv(t))
        else:
            q = lambda t: t.to(lowp).float()

            def cbn(conv, bn, t):  # folded conv: rounded weights, fp32 accumulation, fp32 shift
                w, b = _fold(conv, bn)
                return F.conv2d(t, q(w.float()), b.float(), conv.stride, conv.padding)
            x = q(x.float())
        x = q(F.relu(cbn(self.conv1, self.bn1, x)))
        x = self.maxpool(x)
        taps = []
        for L in range(1, 5):
            for b, blk in enumerate(getattr(self, f"layer{L}")):
                h = q(F.relu(cbn(blk.conv1, blk.bn1, x)))
                y = cbn(blk.conv2, blk.bn2, h)
                tapped = L > 1 and b == 1
                if tapped:
                    y = q(y)  # the plan stores bn2's output (the tap), then adds
                res = x if blk.downsample is None else cbn(blk.downsample[0], blk.downsample[1], x)
                s = y + res
                x = q(F.relu(s))
                if tapped:
                    taps.append({"bn2": y, "add": s, "relu": x}[tap])
        return tuple(taps)


def seeded_resnet18_state_dict(seed=0):
    """Weights that keep activations O(1) through the 17 convs: conv N(0, 2 / fan_in), gamma and
    running_var U(0.5, 1.5), beta and running_mean N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in ResNet18Ref().state_dict().items():
        leaf = k.rsplit(".", 1)[1]
        if v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / (v.shape[1] * v.shape[2] * v.shape[3]))
        elif leaf == "num_batches_tracked":
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif leaf in ("weight", "running_var"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    return sd


def resnet18_ref(sd, dtype=torch.float64):
    m = ResNet18Ref()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)
