"""ResNet / Wide ResNet / ResNeXt feature extractors on libvt_amd.

The reference's `ResNetExtractor` (vision_toolbox/backbones/torchvision_models.py:22-27) wraps a torchvision ResNet in
`create_feature_extractor`.  torchvision is not imported here, so the architecture is written out as our own modules with
torchvision's child names -- `conv1, bn1, relu, maxpool, layer1..layer4` under `feat_extractor`, blocks with `conv1..bn3`
and `downsample.{0,1}` -- and torchvision's initialisation, so that state_dict keys and a torchvision checkpoint match
(`load_torchvision_ckpt`).  `avgpool` and `fc` do not exist: `create_feature_extractor` prunes what the five returned
nodes do not need.

What differs is execution.  CPU tensors run the children with plain torch ops (`_eager_maps`).  GPU tensors run a launch
list (`_vt_emit_maps`):

* the stem `Conv2d(3, 64, 7, 2, 3)` is a 4x4 stride-1 convolution over the space-to-depth image (Builder.stem7_unit), and
  `bn1 + relu + maxpool` one normalise-with-pool pass;
* every unit is Conv -> BatchNorm -> ReLU on the kernels the Darknet family uses;
* a block ends in `relu(bn(conv(h)) + identity)`: the residual joins BEFORE the activation, which is the
  `residual_pre_act` mode of Builder.conv_unit on the add-then-ReLU BatchNorm passes of vt_resnet.hip.

The ResNeXt names run on CPU tensors only: their grouped 3x3 convolutions have 4 or 8 channels per group, below or at
one 16-byte chunk, and a 32- or 64-way split of every block into per-group launches is no hot path.  GPU tensors refuse
them by name.
"""
from __future__ import annotations

import os
from typing import Optional, Union

import torch
from torch import Tensor, nn

from ..components import HipModule
from .base import BaseBackbone

__all__ = ["BasicBlock", "Bottleneck", "ResNetExtractor"]


def _downsample(inplanes: int, outplanes: int, stride: int) -> Optional[nn.Sequential]:
    if stride == 1 and inplanes == outplanes:
        return None
    return nn.Sequential(nn.Conv2d(inplanes, outplanes, 1, stride, bias=False), nn.BatchNorm2d(outplanes))


class _Block(HipModule):
    """conv-bn-relu units, then relu(bn(conv(h)) + identity); `_units()` lists (conv, bn) in order"""

    expansion = 1

    def _units(self):  # pragma: no cover - abstract
        raise NotImplementedError

    def _vt_emit(self, b, x, out=None, name: str = "block"):
        identity = x
        if self.downsample is not None:
            identity = b.conv_unit(x, self.downsample[0], self.downsample[1], 0, name=name + ".downsample")
        units = self._units()
        h = x
        for k, (conv, bn) in enumerate(units[:-1], start=1):
            h = b.conv_unit(h, conv, bn, 1, name=f"{name}.conv{k}")
        conv, bn = units[-1]
        return b.conv_unit(h, conv, bn, 1, residual=identity, out=out, name=f"{name}.conv{len(units)}", residual_pre_act=True)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        identity = x if self.downsample is None else self.downsample(x)
        units = self._units()
        h = x
        for conv, bn in units[:-1]:
            h = self.relu(bn(conv(h)))
        conv, bn = units[-1]
        return [self.relu(bn(conv(h)) + identity)]


class BasicBlock(_Block):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, groups: int = 1, base_width: int = 64) -> None:
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = _downsample(inplanes, planes * self.expansion, stride)

    def _units(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]


class Bottleneck(_Block):
    """1x1 -> 3x3 -> 1x1 with the stride on the 3x3 convolution (torchvision's "v1.5")"""

    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, groups: int = 1, base_width: int = 64) -> None:
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = _downsample(inplanes, planes * self.expansion, stride)

    def _units(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]


class _Trunk(nn.Module):
    """what create_feature_extractor keeps of a torchvision ResNet: everything up to layer4"""

    def __init__(self, block, layers, groups: int, width_per_group: int) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers), start=1):
            blocks = []
            for k in range(n):
                blocks.append(block(inplanes, planes, 2 if (k == 0 and i > 1) else 1, groups, width_per_group))
                inplanes = planes * block.expansion
            self.add_module(f"layer{i}", nn.Sequential(*blocks))
        # torchvision's initialisation (BatchNorm: weight 1, bias 0, which is nn.BatchNorm2d's own)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def layers(self):
        return [self.layer1, self.layer2, self.layer3, self.layer4]


_VARIANTS = {
    # name: (block, blocks per layer, groups, width per group)
    "resnet18": (BasicBlock, (2, 2, 2, 2), 1, 64),
    "resnet34": (BasicBlock, (3, 4, 6, 3), 1, 64),
    "resnet50": (Bottleneck, (3, 4, 6, 3), 1, 64),
    "resnet101": (Bottleneck, (3, 4, 23, 3), 1, 64),
    "resnet152": (Bottleneck, (3, 8, 36, 3), 1, 64),
    "wide_resnet50_2": (Bottleneck, (3, 4, 6, 3), 1, 128),
    "wide_resnet101_2": (Bottleneck, (3, 4, 23, 3), 1, 128),
    "resnext50_32x4d": (Bottleneck, (3, 4, 6, 3), 32, 4),
    "resnext101_32x8d": (Bottleneck, (3, 4, 23, 3), 32, 8),
    "resnext101_64x4d": (Bottleneck, (3, 4, 23, 3), 64, 4),
}


class ResNetExtractor(BaseBackbone):
    """`ResNetExtractor(name)`: five feature maps -- the output of `relu` at stride 2, then `layer1 .. layer4`."""

    def __init__(self, name: str, pretrained: bool = False) -> None:
        if name not in _VARIANTS:
            raise ValueError(f"ResNetExtractor: unknown model {name!r} (one of {', '.join(_VARIANTS)})")
        if pretrained:
            raise NotImplementedError("ResNetExtractor(pretrained=True): nothing is downloaded here; load a local torchvision "
                                      "state_dict with load_torchvision_ckpt(path_or_state_dict)")
        super().__init__()
        block, layers, groups, width = _VARIANTS[name]
        self.model_name = name
        self.feat_extractor = _Trunk(block, layers, groups, width)
        e = block.expansion
        self.out_channels_list = (64, 64 * e, 128 * e, 256 * e, 512 * e)
        self.stride = 32

    # -- launch-list emission ----------------------------------------------------------
    def _vt_emit_maps(self, b, x):
        fe = self.feat_extractor
        if _VARIANTS[self.model_name][2] != 1:
            raise NotImplementedError(
                f"{self.model_name} on GPU tensors: its grouped 3x3 convolutions have {_VARIANTS[self.model_name][3]} channels per group at "
                "layer1, at or below one 16-byte channel chunk, and every block would split into "
                f"{_VARIANTS[self.model_name][2]} per-group launches; it runs on CPU tensors")
        Hs, Ws = (x.H + 1) // 2, (x.W + 1) // 2
        pooled = b.act(x.B, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, fe.conv1.out_channels, "maxpool")
        maps = [b.stem7_unit(x, fe.conv1, fe.bn1, 1, pool_out=pooled, name="conv1")]
        o = pooled
        for i, layer in enumerate(fe.layers(), start=1):
            for k, blk in enumerate(layer):
                o = blk._vt_emit(b, o, name=f"layer{i}.{k}")
            maps.append(o)
        return maps

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        fe = self.feat_extractor
        maps = [fe.relu(fe.bn1(fe.conv1(x)))]
        h = fe.maxpool(maps[0])
        for layer in fe.layers():
            for blk in layer:
                h = blk._eager(h)
            maps.append(h)
        return maps

    # -- checkpoints ---------------------------------------------------------------------
    def load_torchvision_ckpt(self, path_or_state_dict: "Union[str, os.PathLike, dict[str, Tensor]]") -> None:
        """Load a LOCAL torchvision ResNet state_dict (a dict, or the path of a file torch.load reads): `fc.*` is dropped
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
