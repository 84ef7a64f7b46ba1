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

Stochastic depth (`stochastic_depth=` of the extractor, the "ResNet strikes back" recipes) is timm's ResNet's: block i of n
in network order drops its branch with p_i = stochastic_depth * i / (n - 1), behind the last BatchNorm and in front of the
shortcut -- y = relu(keep[b] * bn(conv(h)) + identity) in training mode, keep[b] = bernoulli(1 - p_i) / (1 - p_i) per image,
downsample blocks included.  The factor rides on the unit that closes the block (Builder.conv_unit(..., residual_pre_act=True,
keep=row): the keep forms of the passes of vt_resnet.hip); the factors of a forward are one float[n_sites][B] table
(Builder.keep_table) drawn outside the launch list, or the values of `set_keep_factors` -- on the eager path too.  Eval mode,
stochastic_depth = 0 and blocks with p_i = 0 emit what they always emitted.  No parameter or buffer is added.

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
    drop_prob = 0.0  # stochastic depth of this block (a plain attribute: no state_dict entry), set by ResNetExtractor

    def _units(self):  # pragma: no cover - abstract
        raise NotImplementedError

    def drops(self) -> bool:
        """does this block multiply its branch by a per-image keep factor in the current mode?"""
        return self.training and self.drop_prob > 0.0

    def _vt_emit(self, b, x, out=None, name: str = "block", keep=None):
        identity = x
        if self.downsample is not None:
            identity = b.conv_unit(x, self.downsample[0], self.downsample[1], 0, name=name + ".downsample")
        units = self._units()
        h = x
        for k, (conv, bn) in enumerate(units[:-1], start=1):
            h = b.conv_unit(h, conv, bn, 1, name=f"{name}.conv{k}")
        conv, bn = units[-1]
        return b.conv_unit(h, conv, bn, 1, residual=identity, out=out, name=f"{name}.conv{len(units)}", residual_pre_act=True,
                           keep=keep)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor, keep: Optional[Tensor] = None) -> "list[Tensor]":
        """`keep`: float[B] factors of the branch (None: no stochastic depth)"""
        identity = x if self.downsample is None else self.downsample(x)
        units = self._units()
        h = x
        for conv, bn in units[:-1]:
            h = self.relu(bn(conv(h)))
        conv, bn = units[-1]
        h = bn(conv(h))
        if keep is not None:
            h = h * keep.to(h.dtype).view(-1, 1, 1, 1)
        return [self.relu(h + identity)]


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

    def __init__(self, name: str, pretrained: bool = False, stochastic_depth: float = 0.0) -> None:
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
        stochastic_depth = float(stochastic_depth)
        if not 0.0 <= stochastic_depth < 1.0:
            raise ValueError(f"stochastic_depth must lie in [0, 1), got {stochastic_depth}")
        self.stochastic_depth = stochastic_depth
        blocks = self.blocks()
        for i, blk in enumerate(blocks):
            blk.drop_prob = stochastic_depth * i / (len(blocks) - 1)
        self._keep_override: Optional[Tensor] = None

    # -- stochastic depth ----------------------------------------------------------------
    def blocks(self) -> "list[_Block]":
        return [blk for layer in self.feat_extractor.layers() for blk in layer]

    def drop_rates(self) -> "tuple[float, ...]":
        """p_i = stochastic_depth * i / (n - 1) of every block of the net, in order"""
        return tuple(blk.drop_prob for blk in self.blocks())

    def _sites(self) -> "list[_Block]":
        """the blocks that take a keep factor in the current mode: those with p_i > 0, in training mode"""
        return [blk for blk in self.blocks() if blk.drops()]

    def _vt_keep_rates(self) -> "tuple[float, ...]":
        """the drop probability of every site of the keep table (empty: this mode has no table); part of the program cache key"""
        return tuple(blk.drop_prob for blk in self._sites())

    @property
    def n_keep_sites(self) -> int:
        """rows of the keep table in training mode: the blocks with p_i > 0"""
        return sum(blk.drop_prob > 0.0 for blk in self.blocks())

    def set_keep_factors(self, t: Optional[Tensor]) -> None:
        """Fix the stochastic-depth keep factors of the following forwards: a float[n_keep_sites][B] tensor, one row per block
        with p_i > 0 in order and one factor per image (0 drops the image's branch, 1 / (1 - p_i) is what a kept one gets in
        training; any value is taken), used by the eager path and the launch-list engine alike instead of drawing.  None:
        draw again.  Eval mode ignores it."""
        if t is not None:
            if t.dim() != 2 or t.shape[0] != self.n_keep_sites:
                raise ValueError(f"keep factors of shape {tuple(t.shape)}: {self.model_name} with stochastic_depth="
                                 f"{self.stochastic_depth} has {self.n_keep_sites} dropping blocks (rows), one column per image")
            t = t.detach().to(torch.float32).clone()
        self._keep_override = t

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
        sites = self._sites()
        rows = dict(zip(map(id, sites), b.keep_table([blk.drop_prob for blk in sites], x.B))) if sites else {}
        o = pooled
        for i, layer in enumerate(fe.layers(), start=1):
            for k, blk in enumerate(layer):
                o = blk._vt_emit(b, o, name=f"layer{i}.{k}", keep=rows.get(id(blk)))
            maps.append(o)
        return maps

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        fe = self.feat_extractor
        maps = [fe.relu(fe.bn1(fe.conv1(x)))]
        h = fe.maxpool(maps[0])
        sites = self._sites()
        keep = {}
        if sites:
            from ..program import draw_keep_factors

            table = draw_keep_factors([blk.drop_prob for blk in sites], x.shape[0], x.device, self._keep_override)
            keep = {id(blk): table[r] for r, blk in enumerate(sites)}
        for layer in fe.layers():
            for blk in layer:
                h = blk._eager_maps(h, keep.get(id(blk)))[-1]
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
