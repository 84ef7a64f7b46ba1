"""TEST INFRASTRUCTURE -- a plain-torch.nn restatement of torchvision's MobileNetV2 / MobileNetV3 (torchvision/models/
mobilenetv2.py, mobilenetv3.py), the yardstick of the MobileNet tests.

The reference's MobileNetExtractor only wraps torchvision, which is not installed, so there is no reference fixture to
generate: this file states the three architectures again, independently of vision_toolbox/backbones/mobilenet.py (it imports
nothing from the package), with torchvision's module names under `features`, so that its state_dict without `fc.*` IS the
`features.*` part of a torchvision state_dict.  The head is one `fc` (the trainer's Sequential(backbone, AdaptiveAvgPool2d,
Flatten, Linear)), not torchvision's classifier.  It runs in float64 on the CPU and is filled by oracle/filler.py like every
other yardstick here."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler

ACTS = {"R6": nn.ReLU6, "RE": nn.ReLU, "HS": nn.Hardswish}

# torchvision's inverted_residual_setting of mobilenet_v2: t, c, n, s
V2 = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]]
# torchvision's bneck_conf rows: input, kernel, expanded, out, use_se, activation, stride
V3 = {
    "mobilenet_v3_large": [
        (16, 3, 16, 16, 0, "RE", 1), (16, 3, 64, 24, 0, "RE", 2), (24, 3, 72, 24, 0, "RE", 1), (24, 5, 72, 40, 1, "RE", 2),
        (40, 5, 120, 40, 1, "RE", 1), (40, 5, 120, 40, 1, "RE", 1), (40, 3, 240, 80, 0, "HS", 2), (80, 3, 200, 80, 0, "HS", 1),
        (80, 3, 184, 80, 0, "HS", 1), (80, 3, 184, 80, 0, "HS", 1), (80, 3, 480, 112, 1, "HS", 1), (112, 3, 672, 112, 1, "HS", 1),
        (112, 5, 672, 160, 1, "HS", 2), (160, 5, 960, 160, 1, "HS", 1), (160, 5, 960, 160, 1, "HS", 1)],
    "mobilenet_v3_small": [
        (16, 3, 16, 16, 1, "RE", 2), (16, 3, 72, 24, 0, "RE", 2), (24, 3, 88, 24, 0, "RE", 1), (24, 5, 96, 40, 1, "HS", 2),
        (40, 5, 240, 40, 1, "HS", 1), (40, 5, 240, 40, 1, "HS", 1), (40, 5, 120, 48, 1, "HS", 1), (48, 5, 144, 48, 1, "HS", 1),
        (48, 5, 288, 96, 1, "HS", 2), (96, 5, 576, 96, 1, "HS", 1), (96, 5, 576, 96, 1, "HS", 1)],
}
NAMES = ("mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small")
# feature-extractor parameters (torchvision's published totals minus the classifier)
PARAMS = {"mobilenet_v2": 2_223_872, "mobilenet_v3_large": 2_971_952, "mobilenet_v3_small": 927_008}
# the nodes the reference returns, their channels, and their strides
NODES = {"mobilenet_v2": ((2, 4, 7, 14), 18), "mobilenet_v3_large": ((2, 4, 7, 13), 16), "mobilenet_v3_small": ((1, 2, 4, 9), 12)}
CHANNELS = {"mobilenet_v2": (96, 144, 192, 576, 1280), "mobilenet_v3_large": (64, 72, 240, 672, 960),
            "mobilenet_v3_small": (16, 72, 96, 288, 576)}
STRIDES = {"mobilenet_v2": (2, 4, 8, 16, 32), "mobilenet_v3_large": (2, 4, 8, 16, 32), "mobilenet_v3_small": (4, 4, 8, 16, 32)}


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def cna(cin, cout, k=3, stride=1, groups=1, act="R6", **bn):
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, **bn)]
    return nn.Sequential(*layers, *([ACTS[act]()] if act else []))


class RefSE(nn.Module):
    """torchvision.ops.SqueezeExcitation(c, s, scale_activation=Hardsigmoid)"""

    def __init__(self, c, s):
        super().__init__()
        self.fc1 = nn.Conv2d(c, s, 1)
        self.fc2 = nn.Conv2d(s, c, 1)

    def forward(self, x):
        return x * F.hardsigmoid(self.fc2(F.relu(self.fc1(F.adaptive_avg_pool2d(x, 1)))))


class RefBlock(nn.Module):
    """an inverted residual: `seq` registered under torchvision's attribute name (`conv` in v2, `block` in v3)"""

    def __init__(self, attr, seq, shortcut):
        super().__init__()
        self.attr, self.shortcut = attr, shortcut
        self.add_module(attr, seq)

    def both(self, x):
        seq = getattr(self, self.attr)
        first = seq[0](x)
        h = first
        for m in list(seq)[1:]:
            h = m(h)
        return first, (x + h if self.shortcut else h)

    def forward(self, x):
        return self.both(x)[1]


class RefMobileNet(nn.Module):
    def __init__(self, name, num_classes: int = 1000):
        super().__init__()
        self.name = name
        feats = []
        if name == "mobilenet_v2":
            feats.append(cna(3, 32, stride=2))
            cin = 32
            for t, c, n, s in V2:
                for i in range(n):
                    stride, hid = (s if i == 0 else 1), cin * t
                    seq = ([cna(cin, hid, 1)] if t != 1 else []) + [cna(hid, hid, 3, stride, hid), nn.Conv2d(hid, c, 1, bias=False),
                                                                    nn.BatchNorm2d(c)]
                    feats.append(RefBlock("conv", nn.Sequential(*seq), stride == 1 and cin == c))
                    cin = c
            feats.append(cna(cin, 1280, 1))
            last = 1280
        else:
            bn = dict(eps=0.001, momentum=0.01)
            feats.append(cna(3, 16, stride=2, act="HS", **bn))
            for cin, k, exp, c, se, act, s in V3[name]:
                seq = [cna(cin, exp, 1, act=act, **bn)] if exp != cin else []
                seq.append(cna(exp, exp, k, s, exp, act, **bn))
                if se:
                    seq.append(RefSE(exp, make_divisible(exp // 4)))
                seq.append(cna(exp, c, 1, act=None, **bn))
                feats.append(RefBlock("block", nn.Sequential(*seq), s == 1 and cin == c))
            last = 6 * V3[name][-1][3]
            feats.append(cna(V3[name][-1][3], last, 1, act="HS", **bn))
        self.features = nn.Sequential(*feats)
        self.fc = nn.Linear(last, num_classes)

    def maps(self, x):
        """the five nodes the extractor returns: the first child of every strided block, and the last feature layer"""
        stages, _ = NODES[self.name]
        out, h = [], self.features[0](x)
        for i in range(1, len(self.features) - 1):
            first, h = self.features[i].both(h)
            if i in stages:
                out.append(first)
        return out + [self.features[-1](h)]

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.maps(x)[-1], 1), 1))


def make_pair(name, prefix: str = "mobilenet.", num_classes: int = 1000):
    """(restatement in float64, its filled state_dict in float32: torchvision's `features.*` keys and `fc.*`)"""
    ref = RefMobileNet(name, num_classes)
    sd = filler.fill_state_dict(ref.state_dict(), prefix)
    for k, v in sd.items():  # (the filler centres 1-D weights at 0: BatchNorm scales are 1 + what it gives)
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    ref.load_state_dict(sd)
    return ref.double(), sd


def torchvision_layout(sd: dict) -> dict:
    """the restatement's state_dict with a torchvision classifier key in place of fc.* (what load_torchvision_ckpt drops)"""
    return {k.replace("fc.", "classifier.1."): v for k, v in sd.items()}


def param_grads(ref: nn.Module) -> "dict[str, torch.Tensor]":
    return {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
