"""RegNetX / RegNetY feature extractors on libvt_amd.

The reference's `RegNetExtractor` (vision_toolbox/backbones/torchvision_models.py) wraps a torchvision RegNet in
`create_feature_extractor`.  torchvision is not imported here, so the architecture is written out as our own modules with
torchvision's child names -- `stem.{0,1}`, `trunk_output.block{i}.block{i}-{j}` with `proj.{0,1}`, `f.a.{0,1}`, `f.b.{0,1}`,
`f.se.{fc1,fc2}`, `f.c.{0,1}` under `feat_extractor` -- torchvision's width quantisation (`_block_params`) and its
initialisation, so that state_dict keys and a torchvision checkpoint match (`load_torchvision_ckpt`).  `avgpool` and `fc`
do not exist: `create_feature_extractor` prunes what the five returned nodes do not need.

CPU tensors run the children with plain torch ops (`_eager_maps`).  GPU tensors run a launch list (`_vt_emit_maps`):

* `stem`, `proj`, `f.a` and `f.c` are Conv -> BatchNorm [-> ReLU] units on the kernels the Darknet and ResNet families use;
  the block ends in `relu(proj(x) + f(x))`, the `residual_pre_act` mode of Builder.conv_unit on `f.c`;
* `f.b`, the grouped 3x3 convolution, is Builder.grouped3x3_unit -- ONE launch per pass over all groups (vt_gconv.hip) --
  where a group has 8 .. 64 channels.  The wide-group variants (x_8gf, x_16gf, x_32gf, y_16gf, y_32gf: 112 .. 232 channels
  per group, at most 16 groups) run it as per-group units on the matrix-bound general kernels, or as one plain unit where the
  stage is a single group;
* the Squeeze-Excitation of the Y variants is the global average pool, Builder.se_mlp (its squeeze widths 8, 12, 26, 110 ... are
  no whole 16-byte chunks, which the 1x1 units need) and Builder.se_gate.

`regnet_y_128gf` is not in the table.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Optional, Sequence, Union

import torch
from torch import Tensor, nn

from ..components import HipModule
from .base import BaseBackbone
from .patchconvnet import SqueezeExcitation

__all__ = ["RegNetBlock", "RegNetExtractor", "regnet_block_params"]


def _make_divisible(v: float, divisor: int) -> int:
    """torchvision.models._utils._make_divisible with min_value = divisor"""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def regnet_block_params(depth: int, w_0: int, w_a: float, w_m: float, group_width: int):
    """torchvision's BlockParams.from_init_params (every stage: stride 2, bottleneck multiplier 1.0):
    (stage widths, stage depths, group width per stage)"""
    if w_a < 0 or w_0 <= 0 or w_m <= 1 or w_0 % 8 != 0:
        raise ValueError("Invalid RegNet settings")
    widths_cont = torch.arange(depth) * w_a + w_0
    capacity = torch.round(torch.log(widths_cont / w_0) / math.log(w_m))
    block_widths = (torch.round(torch.divide(w_0 * torch.pow(w_m, capacity), 8)) * 8).int().tolist()
    widths, depths = [], []
    for w in block_widths:  # the stages are the runs of equal width
        if widths and widths[-1] == w:
            depths[-1] += 1
        else:
            widths.append(w)
            depths.append(1)
    gws = [min(group_width, w) for w in widths]
    widths = [_make_divisible(w, g) for w, g in zip(widths, gws)]
    return widths, depths, gws


def _cna(cin: int, cout: int, k: int, stride: int, groups: int, act: bool) -> nn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm2d, [ReLU]"""
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]
    if act:
        layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


class RegNetBlock(HipModule):
    """torchvision's ResBottleneckBlock with bottleneck multiplier 1: relu(proj(x) + f(x)), f = a (1x1) -> b (grouped 3x3 with
    the stride) -> [se] -> c (1x1, no activation)"""

    def __init__(self, width_in: int, width_out: int, stride: int, group_width: int, se_ratio: Optional[float]) -> None:
        super().__init__()
        self.proj = None
        if width_in != width_out or stride != 1:
            self.proj = _cna(width_in, width_out, 1, stride, 1, False)
        f = OrderedDict()
        f["a"] = _cna(width_in, width_out, 1, 1, 1, True)
        f["b"] = _cna(width_out, width_out, 3, stride, width_out // group_width, True)
        if se_ratio:
            f["se"] = SqueezeExcitation(width_out, int(round(se_ratio * width_in)))
        f["c"] = _cna(width_out, width_out, 1, 1, 1, False)
        self.f = nn.Sequential(f)
        self.activation = nn.ReLU(inplace=True)

    def _vt_emit(self, b, x, out=None, name: str = "block"):
        f = self.f
        identity = x if self.proj is None else b.conv_unit(x, self.proj[0], self.proj[1], 0, name=name + ".proj")
        h = b.conv_unit(x, f.a[0], f.a[1], 1, name=name + ".f.a")
        conv = f.b[0]
        if conv.groups > 1 and conv.in_channels // conv.groups in b.GCONV3_WIDTHS:
            h = b.grouped3x3_unit(h, conv, f.b[1], 1, name=name + ".f.b")
        else:  # one group: a plain unit; wide groups: per-group units (Builder._grouped_unit)
            h = b.conv_unit(h, conv, f.b[1], 1, name=name + ".f.b")
        if hasattr(f, "se"):
            pooled = b.global_avgpool(h, name + ".f.se.pool")
            s = b.se_mlp(pooled, f.se.fc1, f.se.fc2, name=name + ".f.se")
            h = b.se_gate(h, s, name=name + ".f.se")
        return b.conv_unit(h, f.c[0], f.c[1], 1, residual=identity, out=out, name=name + ".f.c", residual_pre_act=True)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        identity = x if self.proj is None else self.proj(x)
        return [self.activation(identity + self.f(x))]


class _Trunk(nn.Module):
    """what create_feature_extractor keeps of a torchvision RegNet: `stem` and `trunk_output`"""

    def __init__(self, widths: Sequence[int], depths: Sequence[int], group_widths: Sequence[int], se_ratio: Optional[float],
                 stem_width: int = 32) -> None:
        super().__init__()
        self.stem = _cna(3, stem_width, 3, 2, 1, True)
        stages, cin = OrderedDict(), stem_width
        for i, (w, d, g) in enumerate(zip(widths, depths, group_widths), start=1):
            blocks = OrderedDict()
            for j in range(d):
                blocks[f"block{i}-{j}"] = RegNetBlock(cin if j == 0 else w, w, 2 if j == 0 else 1, g, se_ratio)
            stages[f"block{i}"] = nn.Sequential(blocks)
            cin = w
        self.trunk_output = nn.Sequential(stages)
        # torchvision's initialisation (BatchNorm: weight 1, bias 0, nn.BatchNorm2d's own; the SE biases keep torch's default)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                nn.init.normal_(m.weight, mean=0.0, std=math.sqrt(2.0 / fan_out))


_VARIANTS = {
    # name: (depth, w_0, w_a, w_m, group width, se_ratio)
    "regnet_y_400mf": (16, 48, 27.89, 2.09, 8, 0.25),
    "regnet_y_800mf": (14, 56, 38.84, 2.4, 16, 0.25),
    "regnet_y_1_6gf": (27, 48, 20.71, 2.65, 24, 0.25),
    "regnet_y_3_2gf": (21, 80, 42.63, 2.66, 24, 0.25),
    "regnet_y_8gf": (17, 192, 76.82, 2.19, 56, 0.25),
    "regnet_y_16gf": (18, 200, 106.23, 2.48, 112, 0.25),
    "regnet_y_32gf": (20, 232, 115.89, 2.53, 232, 0.25),
    "regnet_x_400mf": (22, 24, 24.48, 2.54, 16, None),
    "regnet_x_800mf": (16, 56, 35.73, 2.28, 16, None),
    "regnet_x_1_6gf": (18, 80, 34.01, 2.25, 24, None),
    "regnet_x_3_2gf": (25, 88, 26.31, 2.25, 48, None),
    "regnet_x_8gf": (23, 80, 49.56, 2.88, 120, None),
    "regnet_x_16gf": (22, 216, 55.59, 2.1, 128, None),
    "regnet_x_32gf": (23, 320, 69.86, 2.0, 168, None),
}


class RegNetExtractor(BaseBackbone):
    """`RegNetExtractor(name)`: five feature maps -- `stem` at stride 2, then `trunk_output.block1 .. block4`."""

    def __init__(self, name: str, pretrained: bool = False) -> None:
        if name not in _VARIANTS:
            raise ValueError(f"RegNetExtractor: unknown model {name!r} (one of {', '.join(_VARIANTS)})")
        if pretrained:
            raise NotImplementedError("RegNetExtractor(pretrained=True): nothing is downloaded here; load a local torchvision "
                                      "state_dict with load_torchvision_ckpt(path_or_state_dict)")
        super().__init__()
        *init, se_ratio = _VARIANTS[name]
        self._setup(name, *regnet_block_params(*init), se_ratio)

    def _setup(self, name, widths, depths, group_widths, se_ratio) -> None:
        self.model_name = name
        self.widths, self.depths, self.group_widths, self.se_ratio = tuple(widths), tuple(depths), tuple(group_widths), se_ratio
        self.feat_extractor = _Trunk(widths, depths, group_widths, se_ratio)
        self.out_channels_list = (32, *widths)
        self.stride = 2 ** (len(widths) + 1)

    @classmethod
    def _from_stages(cls, widths: Sequence[int], depths: Sequence[int], group_width: int, se_ratio: Optional[float] = None,
                     name: str = "regnet_custom") -> "RegNetExtractor":
        """a model of explicit stages (tests: two-stage models, wide groups at small widths); every width a multiple of
        min(group_width, width)"""
        self = cls.__new__(cls)
        BaseBackbone.__init__(self)
        gws = [min(group_width, w) for w in widths]
        if len(widths) != len(depths) or any(w % g for w, g in zip(widths, gws)):
            raise ValueError("RegNetExtractor._from_stages: one depth per width, widths divisible by the group width")
        self._setup(name, list(widths), list(depths), gws, se_ratio)
        return self

    # -- launch-list emission ----------------------------------------------------------
    def _vt_emit_maps(self, b, x):
        fe = self.feat_extractor
        if x.needs_grad:
            raise NotImplementedError(f"RegNetExtractor({self.model_name}): x.requires_grad -- the extractor forms no gradient "
                                      "of the image (its input is the data; pass images that do not require a gradient)")
        o = b.conv_unit(x, fe.stem[0], fe.stem[1], 1, name="stem")
        maps = [o]
        for i, stage in enumerate(fe.trunk_output, start=1):
            for j, blk in enumerate(stage):
                o = blk._vt_emit(b, o, name=f"trunk_output.block{i}.block{i}-{j}")
            maps.append(o)
        return maps

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        fe = self.feat_extractor
        maps = [fe.stem(x)]
        for stage in fe.trunk_output:
            h = maps[-1]
            for blk in stage:
                h = blk._eager(h)
            maps.append(h)
        return maps

    # -- checkpoints ---------------------------------------------------------------------
    def load_torchvision_ckpt(self, path_or_state_dict: "Union[str, os.PathLike, dict[str, Tensor]]") -> None:
        """Load a LOCAL torchvision RegNet state_dict (a dict, or the path of a file torch.load reads): `fc.*` is dropped
        (the extractor has no classifier) and every other key gets the `feat_extractor.` prefix.  A key the model does not
        have, or one it needs and the dict lacks, raises KeyError."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(os.fspath(sd), map_location="cpu")
        mapped = {"feat_extractor." + k: v for k, v in sd.items() if not k.startswith("fc.")}
        own = self.state_dict()
        extra = sorted(set(mapped) - set(own))
        if extra:
            raise KeyError(f"load_torchvision_ckpt: unexpected keys {extra}")
        missing = sorted(set(own) - set(mapped))
        if missing:
            raise KeyError(f"load_torchvision_ckpt: missing keys {missing}")
        self.load_state_dict(mapped)
