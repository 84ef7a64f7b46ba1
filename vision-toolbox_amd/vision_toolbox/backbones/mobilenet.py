"""MobileNetV2 / MobileNetV3 feature extractors on libvt_amd.

The reference's `MobileNetExtractor` (vision_toolbox/backbones/torchvision_models.py) wraps a torchvision MobileNet in
`create_feature_extractor` and returns the FIRST child of every block with stride > 1 (`_is_cn`) plus the last feature layer.
torchvision is not imported here, so the three architectures are written out as our own modules with torchvision's child
names -- `features.{i}` with `conv.{...}` (v2) or `block.{...}` (v3) under `feat_extractor` -- and its initialisation, so that
state_dict keys and a torchvision checkpoint match (`load_torchvision_ckpt`).  `avgpool` and `classifier` do not exist.

CPU tensors run the children with plain torch ops (`_eager_maps`).  GPU tensors run a launch list (`_vt_emit_maps`):

* the stem, the 1x1 expansions, the 1x1 projections and the last layer are Conv -> BatchNorm [-> act] units on the kernels
  every family uses, with the activation codes 1 (ReLU), 5 (ReLU6) and 6 (Hardswish) of the BatchNorm passes; a block's
  shortcut is the residual behind its activation-free projection;
* the depthwise k x k convolution is Builder.depthwise_unit: the tiled kernels of vt_dwtile.hip (band + halo in LDS, the filter
  gradient as per-band shares and an ordered reducer: no float atomics, so deterministic mode runs the same program);
* the Squeeze-Excitation of v3 is the global average pool, Builder.se_mlp (squeeze widths 8 .. 240) and Builder.hsig_gate, the
  hardsigmoid gate of VoVNet's eSE without a residual.

In `mobilenet_v3_small`, `features.1` has no expansion, so its first child is the depthwise unit: the first two maps are both
at stride 4, as the reference returns them.
"""
from __future__ import annotations

import os
from typing import Union

import torch
from torch import Tensor, nn

from .base import BaseBackbone
from .patchconvnet import SqueezeExcitation
from .regnet import _make_divisible

__all__ = ["MobileNetExtractor", "InvertedResidualV2", "InvertedResidualV3"]

_ACT = {"RE6": (nn.ReLU6, 5), "RE": (nn.ReLU, 1), "HS": (nn.Hardswish, 6)}


def _act_code(m: nn.Module) -> int:
    return {nn.ReLU: 1, nn.ReLU6: 5, nn.Hardswish: 6}[type(m)]


def _cna(cin: int, cout: int, k: int, stride: int, groups: int, act, bn_kw: dict) -> nn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm2d, [activation]"""
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, **bn_kw)]
    if act is not None:
        layers.append(_ACT[act][0](inplace=True))
    return nn.Sequential(*layers)


def _emit_cna(b, x, unit: nn.Sequential, name: str, residual=None, untiled: bool = False):
    """a Conv2dNormActivation on the GPU: the depthwise ones on the tiled kernels, the others as ordinary units.  `untiled`
    (MobileNetExtractor._untiled_depthwise, for tools/bench_mobilenet.py): the depthwise ones as ConvNormAct(groups=C) runs
    them, on the kernels of vt_dwconv.hip"""
    conv, act = unit[0], (_act_code(unit[2]) if len(unit) > 2 else 0)
    if conv.groups > 1 and not untiled:
        return b.depthwise_unit(x, conv, unit[1], act, name=name)
    return b.conv_unit(x, conv, unit[1], act, residual=residual, name=name)


class InvertedResidualV2(nn.Module):
    """torchvision's mobilenetv2.InvertedResidual: `conv` = [expand 1x1 -BN-ReLU6 if t != 1], depthwise 3x3 -BN-ReLU6 (stride),
    Conv2d 1x1, BatchNorm2d; the shortcut where stride 1 and in == out"""

    def __init__(self, inp: int, oup: int, stride: int, expand_ratio: int) -> None:
        super().__init__()
        hidden = int(round(inp * expand_ratio))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(_cna(inp, hidden, 1, 1, 1, "RE6", {}))
        layers += [_cna(hidden, hidden, 3, stride, hidden, "RE6", {}), nn.Conv2d(hidden, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)
        self._is_cn = stride > 1

    def first_and_out(self, x: Tensor) -> "tuple[Tensor, Tensor]":
        first = self.conv[0](x)
        h = first
        for m in list(self.conv)[1:]:
            h = m(h)
        return first, (x + h if self.use_res_connect else h)

    def forward(self, x: Tensor) -> Tensor:
        return self.first_and_out(x)[1]

    def _vt_emit(self, b, x, name: str, untiled: bool = False):
        units = list(self.conv)[:-2]
        h, first = x, None
        for i, u in enumerate(units):
            h = _emit_cna(b, h, u, f"{name}.conv.{i}", untiled=untiled)
            first = h if first is None else first
        n = len(units)
        out = b.conv_unit(h, self.conv[n], self.conv[n + 1], 0, residual=x if self.use_res_connect else None, name=f"{name}.conv.{n}")
        return first, out


class InvertedResidualV3(nn.Module):
    """torchvision's mobilenetv3.InvertedResidual: `block` = [expand 1x1 -BN-act if exp != in], depthwise k x k -BN-act (stride),
    [SqueezeExcitation(exp, make_divisible(exp // 4, 8), hardsigmoid)], project 1x1 -BN; the shortcut where stride 1, in == out"""

    def __init__(self, inp: int, k: int, exp: int, oup: int, use_se: bool, act: str, stride: int, bn_kw: dict) -> None:
        super().__init__()
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if exp != inp:
            layers.append(_cna(inp, exp, 1, 1, 1, act, bn_kw))
        layers.append(_cna(exp, exp, k, stride, exp, act, bn_kw))
        if use_se:
            layers.append(SqueezeExcitation(exp, _make_divisible(exp // 4, 8), scale_activation=nn.Hardsigmoid))
        layers.append(_cna(exp, oup, 1, 1, 1, None, bn_kw))
        self.block = nn.Sequential(*layers)
        self._is_cn = stride > 1

    def first_and_out(self, x: Tensor) -> "tuple[Tensor, Tensor]":
        first = self.block[0](x)
        h = first
        for m in list(self.block)[1:]:
            h = m(h)
        return first, (x + h if self.use_res_connect else h)

    def forward(self, x: Tensor) -> Tensor:
        return self.first_and_out(x)[1]

    def _vt_emit(self, b, x, name: str, untiled: bool = False):
        h, first = x, None
        last = len(self.block) - 1
        for i, m in enumerate(self.block):
            nm = f"{name}.block.{i}"
            if isinstance(m, SqueezeExcitation):
                pooled = b.global_avgpool(h, nm + ".pool")
                h = b.hsig_gate(h, b.se_mlp(pooled, m.fc1, m.fc2, name=nm), name=nm)
            else:
                h = _emit_cna(b, h, m, nm, residual=x if (i == last and self.use_res_connect) else None, untiled=untiled)
            first = h if first is None else first
        return first, h


# (t, c, n, s) of torchvision's mobilenet_v2
_V2 = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
# (in, k, exp, out, SE, act, stride) of torchvision's mobilenet_v3_large / _small
_V3_LARGE = [(16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2), (24, 3, 72, 24, False, "RE", 1),
             (24, 5, 72, 40, True, "RE", 2), (40, 5, 120, 40, True, "RE", 1), (40, 5, 120, 40, True, "RE", 1),
             (40, 3, 240, 80, False, "HS", 2), (80, 3, 200, 80, False, "HS", 1), (80, 3, 184, 80, False, "HS", 1),
             (80, 3, 184, 80, False, "HS", 1), (80, 3, 480, 112, True, "HS", 1), (112, 3, 672, 112, True, "HS", 1),
             (112, 5, 672, 160, True, "HS", 2), (160, 5, 960, 160, True, "HS", 1), (160, 5, 960, 160, True, "HS", 1)]
_V3_SMALL = [(16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
             (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
             (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
             (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1)]
_VARIANTS = {"mobilenet_v2": _V2, "mobilenet_v3_large": _V3_LARGE, "mobilenet_v3_small": _V3_SMALL}


class _Features(nn.Module):
    """what create_feature_extractor keeps of a torchvision MobileNet: `features`"""

    def __init__(self, name: str) -> None:
        super().__init__()
        layers: "list[nn.Module]" = []
        if name == "mobilenet_v2":
            layers.append(_cna(3, 32, 3, 2, 1, "RE6", {}))
            cin = 32
            for t, c, n, s in _V2:
                for i in range(n):
                    layers.append(InvertedResidualV2(cin, c, s if i == 0 else 1, t))
                    cin = c
            layers.append(_cna(cin, 1280, 1, 1, 1, "RE6", {}))
        else:
            bn_kw = dict(eps=0.001, momentum=0.01)
            layers.append(_cna(3, 16, 3, 2, 1, "HS", bn_kw))
            for cfg in _VARIANTS[name]:
                layers.append(InvertedResidualV3(*cfg, bn_kw))
            cin = _VARIANTS[name][-1][3]
            layers.append(_cna(cin, 6 * cin, 1, 1, 1, "HS", bn_kw))
        self.features = nn.Sequential(*layers)
        # torchvision's initialisation
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)


class MobileNetExtractor(BaseBackbone):
    """`MobileNetExtractor(name)`, name one of mobilenet_v2 / mobilenet_v3_large / mobilenet_v3_small: five feature maps -- the
    first child of every block with stride > 1, then the last feature layer."""

    def __init__(self, name: str, pretrained: bool = False) -> None:
        if name not in _VARIANTS:
            raise ValueError(f"MobileNetExtractor: unknown model {name!r} (one of {', '.join(_VARIANTS)})")
        if pretrained:
            raise NotImplementedError("MobileNetExtractor(pretrained=True): nothing is downloaded here; load a local torchvision "
                                      "state_dict with load_torchvision_ckpt(path_or_state_dict)")
        super().__init__()
        self.model_name = name
        self.feat_extractor = _Features(name)
        feats = self.feat_extractor.features
        self.stage_indices = tuple(i for i, m in enumerate(feats) if getattr(m, "_is_cn", False))
        block = "conv" if name == "mobilenet_v2" else "block"
        self.node_names = tuple(f"features.{i}.{block}.0" for i in self.stage_indices) + (f"features.{len(feats) - 1}",)
        firsts = [getattr(feats[i], block)[0][0].out_channels for i in self.stage_indices]
        self.out_channels_list = (*firsts, feats[-1][0].out_channels)
        self.stride = 32
        self._untiled_depthwise = False  # (measurement only: see _emit_cna)

    # -- launch-list emission ----------------------------------------------------------
    def _vt_emit_maps(self, b, x):
        feats = self.feat_extractor.features
        if x.needs_grad:
            raise NotImplementedError(f"MobileNetExtractor({self.model_name}): x.requires_grad -- the extractor forms no gradient "
                                      "of the image (its input is the data; pass images that do not require a gradient)")
        o = _emit_cna(b, x, feats[0], "features.0")
        maps = []
        for i in range(1, len(feats) - 1):
            first, o = feats[i]._vt_emit(b, o, f"features.{i}", self._untiled_depthwise)
            if i in self.stage_indices:
                maps.append(first)
        maps.append(_emit_cna(b, o, feats[-1], f"features.{len(feats) - 1}"))
        return maps

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        feats = self.feat_extractor.features
        h, maps = feats[0](x), []
        for i in range(1, len(feats) - 1):
            first, h = feats[i].first_and_out(h)
            if i in self.stage_indices:
                maps.append(first)
        maps.append(feats[-1](h))
        return maps

    # -- checkpoints ---------------------------------------------------------------------
    def load_torchvision_ckpt(self, path_or_state_dict: "Union[str, os.PathLike, dict[str, Tensor]]") -> None:
        """Load a LOCAL torchvision MobileNet state_dict (a dict, or the path of a file torch.load reads): `classifier.*` is
        dropped (the extractor has no classifier) and every other key gets the `feat_extractor.` prefix.  A key the model does
        not have, or one it needs and the dict lacks, raises KeyError."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(os.fspath(sd), map_location="cpu")
        mapped = {"feat_extractor." + k: v for k, v in sd.items() if not k.startswith("classifier.")}
        own = self.state_dict()
        extra = sorted(set(mapped) - set(own))
        if extra:
            raise KeyError(f"load_torchvision_ckpt: unexpected keys {extra}")
        missing = sorted(set(own) - set(mapped))
        if missing:
            raise KeyError(f"load_torchvision_ckpt: missing keys {missing}")
        self.load_state_dict(mapped)
