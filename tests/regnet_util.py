"""TEST INFRASTRUCTURE -- a plain-torch.nn restatement of torchvision's RegNet (torchvision/models/regnet.py), the yardstick of
the RegNet tests.

The reference's RegNetExtractor only wraps torchvision, which is not installed, so there is no reference fixture to
generate: this file states the architecture and the width quantisation again, independently of
vision_toolbox/backbones/regnet.py (it imports nothing from the package), with torchvision's module names, so that its
state_dict IS a torchvision state_dict (`fc.*` included).  It runs in float64 on the CPU and is filled by oracle/filler.py
like every other yardstick here."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler

# name: (depth, w_0, w_a, w_m, group width, se_ratio)
CONFIGS = {
    "regnet_y_400mf": (16, 48, 27.89, 2.09, 8, 0.25),
    "regnet_y_800mf": (14, 56, 38.84, 2.4, 16, 0.25),
    "regnet_y_8gf": (17, 192, 76.82, 2.19, 56, 0.25),
    "regnet_x_400mf": (22, 24, 24.48, 2.54, 16, None),
    "regnet_x_800mf": (16, 56, 35.73, 2.28, 16, None),
    "regnet_x_8gf": (23, 80, 49.56, 2.88, 120, None),
}


def block_params(depth, w_0, w_a, w_m, group_width):
    """torchvision's BlockParams.from_init_params + _adjust_widths_groups_compatibilty, in its own words"""
    widths_cont = torch.arange(depth) * w_a + w_0
    block_capacity = torch.round(torch.log(widths_cont / w_0) / math.log(w_m))
    block_widths = (torch.round(torch.divide(w_0 * torch.pow(w_m, block_capacity), 8)) * 8).int().tolist()
    split_helper = zip(block_widths + [0], [0] + block_widths, block_widths + [0], [0] + block_widths)
    splits = [w != wp or r != rp for w, wp, r, rp in split_helper]
    stage_widths = [w for w, t in zip(block_widths, splits[:-1]) if t]
    stage_depths = torch.diff(torch.tensor([d for d, t in enumerate(splits) if t])).int().tolist()
    group_widths = [min(group_width, w) for w in stage_widths]

    def make_divisible(v, divisor):
        new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
        return new_v + divisor if new_v < 0.9 * v else new_v

    return [make_divisible(w, g) for w, g in zip(stage_widths, group_widths)], stage_depths, group_widths


def _cna(cin, cout, k, stride, groups, act):
    layers = [nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]
    return nn.Sequential(*layers, *([nn.ReLU()] if act else []))


class RefSE(nn.Module):
    def __init__(self, c, s):
        super().__init__()
        self.fc1 = nn.Conv2d(c, s, 1)
        self.fc2 = nn.Conv2d(s, c, 1)

    def forward(self, x):
        return x * torch.sigmoid(self.fc2(F.relu(self.fc1(F.adaptive_avg_pool2d(x, 1)))))


class RefTransform(nn.Sequential):
    def __init__(self, cin, cout, stride, gw, se_ratio):
        super().__init__()
        self.a = _cna(cin, cout, 1, 1, 1, True)
        self.b = _cna(cout, cout, 3, stride, cout // gw, True)
        if se_ratio:
            self.se = RefSE(cout, int(round(se_ratio * cin)))
        self.c = _cna(cout, cout, 1, 1, 1, False)


class RefBlock(nn.Module):
    def __init__(self, cin, cout, stride, gw, se_ratio):
        super().__init__()
        self.proj = _cna(cin, cout, 1, stride, 1, False) if (cin != cout or stride != 1) else None
        self.f = RefTransform(cin, cout, stride, gw, se_ratio)

    def forward(self, x):
        return F.relu((x if self.proj is None else self.proj(x)) + self.f(x))


class RefRegNet(nn.Module):
    def __init__(self, name=None, num_classes: int = 1000, stages=None):
        """`name`: a torchvision variant; or `stages` = (widths, depths, group width, se_ratio)"""
        super().__init__()
        if stages is None:
            *init, se_ratio = CONFIGS[name]
            widths, depths, gws = block_params(*init)
        else:
            widths, depths, gw, se_ratio = stages
            gws = [min(gw, w) for w in widths]
        self.widths, self.depths, self.group_widths = widths, depths, gws
        self.stem = _cna(3, 32, 3, 2, 1, True)
        self.trunk_output = nn.Sequential()
        cin = 32
        for i, (w, d, g) in enumerate(zip(widths, depths, gws), 1):
            stage = nn.Sequential()
            for j in range(d):
                stage.add_module(f"block{i}-{j}", RefBlock(cin if j == 0 else w, w, 2 if j == 0 else 1, g, se_ratio))
            self.trunk_output.add_module(f"block{i}", stage)
            cin = w
        self.fc = nn.Linear(cin, num_classes)

    def maps(self, x):
        """the five nodes the extractor returns: stem, trunk_output.block1 .. block4"""
        out = [self.stem(x)]
        for stage in self.trunk_output:
            out.append(stage(out[-1]))
        return out

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.maps(x)[-1], 1), 1))


def make_pair(name=None, prefix: str = "regnet.", stages=None, num_classes: int = 1000):
    """(restatement in float64, its filled torchvision-layout state_dict in float32)"""
    ref = RefRegNet(name, num_classes, stages)
    sd = filler.fill_state_dict(ref.state_dict(), prefix)
    for k, v in sd.items():  # (the filler centres 1-D weights at 0: BatchNorm scales are 1 + what it gives)
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    ref.load_state_dict(sd)
    return ref.double(), sd


def param_grads(ref: nn.Module) -> "dict[str, torch.Tensor]":
    return {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
