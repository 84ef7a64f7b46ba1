"""TEST INFRASTRUCTURE -- a plain-torch.nn restatement of torchvision's ResNet (torchvision/models/resnet.py), the yardstick
of the ResNet tests.

The reference's ResNetExtractor only wraps torchvision, which is not installed, so there is no reference fixture to
generate: this file states the architecture again, independently of vision_toolbox/backbones/resnet.py (it imports nothing
from the package), with torchvision's module names, so that its state_dict IS a torchvision state_dict (`fc.*` included).
It runs in float64 on the CPU and is filled by oracle/filler.py like every other yardstick here."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler

# name: (bottleneck?, blocks per layer, groups, width per group)
CONFIGS = {
    "resnet18": (False, [2, 2, 2, 2], 1, 64),
    "resnet34": (False, [3, 4, 6, 3], 1, 64),
    "resnet50": (True, [3, 4, 6, 3], 1, 64),
    "resnet101": (True, [3, 4, 23, 3], 1, 64),
    "wide_resnet50_2": (True, [3, 4, 6, 3], 1, 128),
    "resnext50_32x4d": (True, [3, 4, 6, 3], 32, 4),
}


class RefBlock(nn.Module):
    def __init__(self, bottleneck, cin, planes, stride, groups, base_width):
        super().__init__()
        if bottleneck:
            mid = int(planes * base_width / 64) * groups
            cout = planes * 4
            shapes = [(cin, mid, 1, 1, 0, 1), (mid, mid, 3, stride, 1, groups), (mid, cout, 1, 1, 0, 1)]
        else:
            cout = planes
            shapes = [(cin, planes, 3, stride, 1, 1), (planes, planes, 3, 1, 1, 1)]
        for i, (a, b, k, s, p, g) in enumerate(shapes, 1):
            setattr(self, f"conv{i}", nn.Conv2d(a, b, k, s, p, groups=g, bias=False))
            setattr(self, f"bn{i}", nn.BatchNorm2d(b))
        self.n = len(shapes)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
        self.cout = cout

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        for i in range(1, self.n + 1):
            x = getattr(self, f"bn{i}")(getattr(self, f"conv{i}")(x))
            if i < self.n:
                x = F.relu(x)
        return F.relu(x + skip)


class RefResNet(nn.Module):
    def __init__(self, name: str, num_classes: int = 1000):
        super().__init__()
        bottleneck, depths, groups, base_width = CONFIGS[name]
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for li, (planes, n) in enumerate(zip([64, 128, 256, 512], depths), 1):
            blocks = []
            for bi in range(n):
                blk = RefBlock(bottleneck, cin, planes, 2 if (bi == 0 and li > 1) else 1, groups, base_width)
                blocks.append(blk)
                cin = blk.cout
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        self.fc = nn.Linear(cin, num_classes)

    def maps(self, x):
        """the five nodes the extractor returns: relu, layer1 .. layer4"""
        out = [F.relu(self.bn1(self.conv1(x)))]
        h = F.max_pool2d(out[0], 3, 2, 1)
        for li in range(1, 5):
            h = getattr(self, f"layer{li}")(h)
            out.append(h)
        return out

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.maps(x)[-1], 1), 1))


def make_pair(name: str, prefix: str = "resnet."):
    """(restatement in float64, its filled torchvision-layout state_dict in float32)"""
    ref = RefResNet(name)
    sd = filler.fill_state_dict(ref.state_dict(), prefix)
    for k, v in sd.items():  # (the filler centres 1-D weights at 0: BatchNorm scales are 1 + what it gives)
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    ref.load_state_dict(sd)
    return ref.double(), sd


def param_grads(ref: nn.Module) -> "dict[str, torch.Tensor]":
    return {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
