"""TEST INFRASTRUCTURE -- a plain-torch.nn restatement of torchvision's EfficientNet / EfficientNetV2 (torchvision/models/
efficientnet.py), the yardstick of the EfficientNet tests.

The reference's EfficientNetExtractor only wraps torchvision, which is not installed, so there is no reference fixture to
generate: this file states the architectures again, independently of vision_toolbox/backbones/efficientnet.py (it imports
nothing from the package), with torchvision's module names under `features`, so that its state_dict without `fc.*` IS the
`features.*` part of a torchvision state_dict.  The head is one `fc` (the trainer's Sequential(backbone, AdaptiveAvgPool2d,
Flatten, Linear)), not torchvision's classifier.  Stochastic depth is not drawn here: `maps` / `forward` take the keep factors
as an explicit float[n_sites][B] argument, one row per residual block in order (None: no stochastic depth, what eval mode
computes).  It runs in float64 on the CPU and is filled by oracle/filler.py like every other yardstick here."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler

# (kind, expand ratio, kernel, stride, in, out, layers): torchvision's MBConvConfig / FusedMBConvConfig rows
B0 = [("mb", 1, 3, 1, 32, 16, 1), ("mb", 6, 3, 2, 16, 24, 2), ("mb", 6, 5, 2, 24, 40, 2), ("mb", 6, 3, 2, 40, 80, 3),
      ("mb", 6, 5, 1, 80, 112, 3), ("mb", 6, 5, 2, 112, 192, 4), ("mb", 6, 3, 1, 192, 320, 1)]
V2 = {
    "efficientnet_v2_s": [("fused", 1, 3, 1, 24, 24, 2), ("fused", 4, 3, 2, 24, 48, 4), ("fused", 4, 3, 2, 48, 64, 4),
                          ("mb", 4, 3, 2, 64, 128, 6), ("mb", 6, 3, 1, 128, 160, 9), ("mb", 6, 3, 2, 160, 256, 15)],
    "efficientnet_v2_m": [("fused", 1, 3, 1, 24, 24, 3), ("fused", 4, 3, 2, 24, 48, 5), ("fused", 4, 3, 2, 48, 80, 5),
                          ("mb", 4, 3, 2, 80, 160, 7), ("mb", 6, 3, 1, 160, 176, 14), ("mb", 6, 3, 2, 176, 304, 18),
                          ("mb", 6, 3, 1, 304, 512, 5)],
    "efficientnet_v2_l": [("fused", 1, 3, 1, 32, 32, 4), ("fused", 4, 3, 2, 32, 64, 7), ("fused", 4, 3, 2, 64, 96, 7),
                          ("mb", 4, 3, 2, 96, 192, 10), ("mb", 6, 3, 1, 192, 224, 19), ("mb", 6, 3, 2, 224, 384, 25),
                          ("mb", 6, 3, 1, 384, 640, 7)],
}
# width multiplier, depth multiplier of b0 .. b7
SCALING = {"efficientnet_b0": (1.0, 1.0), "efficientnet_b1": (1.0, 1.1), "efficientnet_b2": (1.1, 1.2), "efficientnet_b3": (1.2, 1.4),
           "efficientnet_b4": (1.4, 1.8), "efficientnet_b5": (1.6, 2.2), "efficientnet_b6": (1.8, 2.6), "efficientnet_b7": (2.0, 3.1)}
SD_PROB = {"efficientnet_b0": 0.2, "efficientnet_b1": 0.2, "efficientnet_b2": 0.3, "efficientnet_b3": 0.3, "efficientnet_b4": 0.4,
           "efficientnet_b5": 0.4, "efficientnet_b6": 0.5, "efficientnet_b7": 0.5, "efficientnet_v2_s": 0.2, "efficientnet_v2_m": 0.3,
           "efficientnet_v2_l": 0.5}
NAMES = tuple(SD_PROB)
# feature-extractor parameters: torchvision's published totals minus the classifier (last width * 1000 + 1000)
PARAMS = {"efficientnet_b0": 4_007_548, "efficientnet_b1": 6_513_184, "efficientnet_b2": 7_700_994, "efficientnet_b3": 10_696_232,
          "efficientnet_b4": 17_548_616, "efficientnet_b5": 28_340_784, "efficientnet_b6": 40_735_704, "efficientnet_b7": 63_786_960,
          "efficientnet_v2_s": 20_177_488, "efficientnet_v2_m": 52_858_356, "efficientnet_v2_l": 117_234_272}
CHANNELS = {"efficientnet_b0": (96, 144, 240, 672, 1280), "efficientnet_b1": (96, 144, 240, 672, 1280),
            "efficientnet_b2": (96, 144, 288, 720, 1408), "efficientnet_b3": (144, 192, 288, 816, 1536),
            "efficientnet_b4": (144, 192, 336, 960, 1792), "efficientnet_b5": (144, 240, 384, 1056, 2048),
            "efficientnet_b6": (192, 240, 432, 1200, 2304), "efficientnet_b7": (192, 288, 480, 1344, 2560),
            "efficientnet_v2_s": (96, 192, 256, 960, 1280), "efficientnet_v2_m": (96, 192, 320, 1056, 1280),
            "efficientnet_v2_l": (128, 256, 384, 1344, 1280)}
STAGES = (2, 3, 4, 6)  # the reference returns features.{i}.0.block.0 of these, and the last feature unit


def strides(name):
    """b*: 2 / 4 / 8 / 16 / 32; v2: the third map is the 1x1 expansion in front of its stride-2 depthwise unit (stride 8)"""
    return (4, 8, 8, 16, 32) if "_v2_" in name else (2, 4, 8, 16, 32)


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def bn_settings(name):
    if "_v2_" in name:
        return dict(eps=1e-3)
    return dict(eps=1e-3, momentum=0.01) if name[-2:] in ("b5", "b6", "b7") else {}


def table(name):
    """(stage rows, width of the last unit)"""
    if name in V2:
        return V2[name], 1280
    wm, dm = SCALING[name]
    rows = [(kd, e, k, s, make_divisible(i * wm), make_divisible(o * wm), int(math.ceil(n * dm))) for kd, e, k, s, i, o, n in B0]
    return rows, 4 * rows[-1][5]


def cna(cin, cout, k=3, stride=1, groups=1, act=True, **bn):
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, **bn)]
    return nn.Sequential(*layers, *([nn.SiLU()] if act else []))


class RefSE(nn.Module):
    """torchvision.ops.SqueezeExcitation(c, s, activation=SiLU)"""

    def __init__(self, c, s):
        super().__init__()
        self.fc1 = nn.Conv2d(c, s, 1)
        self.fc2 = nn.Conv2d(s, c, 1)

    def forward(self, x):
        return x * torch.sigmoid(self.fc2(F.silu(self.fc1(F.adaptive_avg_pool2d(x, 1)))))


class RefBlock(nn.Module):
    """MBConv or FusedMBConv: `block`, the shortcut where stride 1 and in == out, the branch times keep[b] in front of it"""

    def __init__(self, kind, e, k, stride, cin, cout, p, bn):
        super().__init__()
        exp = make_divisible(cin * e)
        if kind == "mb":
            seq = [cna(cin, exp, 1, **bn)] if exp != cin else []
            seq += [cna(exp, exp, k, stride, exp, **bn), RefSE(exp, max(1, cin // 4)), cna(exp, cout, 1, act=False, **bn)]
        elif exp != cin:
            seq = [cna(cin, exp, k, stride, **bn), cna(exp, cout, 1, act=False, **bn)]
        else:
            seq = [cna(cin, cout, k, stride, **bn)]
        self.block = nn.Sequential(*seq)
        self.shortcut, self.p = stride == 1 and cin == cout, p

    def both(self, x, keep=None):
        first = self.block[0](x)
        h = first
        for m in list(self.block)[1:]:
            h = m(h)
        if self.shortcut:
            h = x + (h if keep is None else h * keep.to(h.dtype).view(-1, 1, 1, 1))
        return first, self.out(h)

    def out(self, h):  # (a hook point: the block's stored output)
        return h


class RefEfficientNet(nn.Module):
    def __init__(self, name, num_classes: int = 1000):
        super().__init__()
        self.name = name
        rows, last = table(name)
        bn = bn_settings(name)
        feats = [cna(3, rows[0][4], 3, 2, **bn)]
        total, idx = sum(r[6] for r in rows), 0
        for kind, e, k, s, cin, cout, n in rows:
            stage = []
            for j in range(n):
                stage.append(RefBlock(kind, e, k, s if j == 0 else 1, cin if j == 0 else cout, cout, SD_PROB[name] * idx / total, bn))
                idx += 1
            feats.append(nn.Sequential(*stage))
        feats.append(cna(rows[-1][5], last, 1, **bn))
        self.features = nn.Sequential(*feats)
        self.fc = nn.Linear(last, num_classes)

    def blocks(self):
        return [blk for i in range(1, len(self.features) - 1) for blk in self.features[i]]

    def sites(self):
        """the residual blocks, in order: the rows of a keep table"""
        return [blk for blk in self.blocks() if blk.shortcut]

    def maps(self, x, keep=None):
        """the five nodes the extractor returns; `keep`: float[n_sites][B] (None: no stochastic depth)"""
        rows = {id(blk): keep[r] for r, blk in enumerate(self.sites())} if keep is not None else {}
        out, h = [], self.features[0](x)
        for i in range(1, len(self.features) - 1):
            for j, blk in enumerate(self.features[i]):
                first, h = blk.both(h, rows.get(id(blk)))
                if j == 0 and i in STAGES:
                    out.append(first)
        return out + [self.features[-1](h)]

    def forward(self, x, keep=None):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.maps(x, keep)[-1], 1), 1))


def make_pair(name, prefix: str = "efficientnet.", num_classes: int = 1000):
    """(restatement in float64, its filled state_dict in float32: torchvision's `features.*` keys and `fc.*`)"""
    ref = RefEfficientNet(name, num_classes)
    sd = filler.fill_state_dict(ref.state_dict(), prefix)
    for k, v in sd.items():  # (the filler centres 1-D weights at 0: BatchNorm scales are 1 + what it gives)
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    ref.load_state_dict(sd)
    return ref.double(), sd


def torchvision_layout(sd: dict) -> dict:
    """the restatement's state_dict with a torchvision classifier key in place of fc.* (what load_torchvision_ckpt drops)"""
    return {k.replace("fc.", "classifier.1."): v for k, v in sd.items()}


def keep_table(name, B: int, step: int = 0) -> torch.Tensor:
    """a deterministic keep table float[n_sites][B] for the tests: image (site + step) % B of every site is dropped, and so is
    image (2 * site + 1 + step) % B of every third site; the last image is kept everywhere; kept images get 1 / (1 - p) of
    their block, as training draws them.  At B >= 3 at least three sites drop an image."""
    ref = RefEfficientNet(name, 2)
    sites = ref.sites()
    t = torch.empty(len(sites), B)
    for r, blk in enumerate(sites):
        t[r] = 1.0 / (1.0 - blk.p)
        drop = {(r + step) % B} | ({(2 * r + 1 + step) % B} if r % 3 == 0 else set())
        for b in drop - {B - 1}:
            t[r, b] = 0.0
    return t
