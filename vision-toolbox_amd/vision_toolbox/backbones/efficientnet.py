"""EfficientNet (b0 .. b7) and EfficientNetV2 (s / m / l) feature extractors on libvt_amd.

The reference's `EfficientNetExtractor` (vision_toolbox/backbones/torchvision_models.py) wraps a torchvision EfficientNet in
`create_feature_extractor` and returns `features.{i}.0.block.0` for i in (2, 3, 4, 6) -- the FIRST Conv-BN-SiLU of the first
block of those stages, activation included -- plus the last feature unit.  torchvision is not imported here, so the
architectures are written out as our own modules with torchvision's child names -- `features.{s}.{j}.block.{i}` with `fc1` /
`fc2` inside the SqueezeExcitation, under `feat_extractor` -- and its initialisation, so that state_dict keys and a
torchvision checkpoint match (`load_torchvision_ckpt`).  `avgpool` and `classifier` do not exist.

For b0 .. b7 the five maps sit at strides 2 / 4 / 8 / 16 / 32.  For the V2 models the third map is the 1x1 expansion IN FRONT
of its block's stride-2 depthwise unit: it sits at stride 8 like the second map (strides 4 / 8 / 8 / 16 / 32), as the
reference returns it.

CPU tensors run the children with plain torch ops (`_eager_maps`).  GPU tensors run a launch list (`_vt_emit_maps`):

* the stem, the 1x1 expansions and projections, the 3x3 units of a FusedMBConv and the last unit are Conv -> BatchNorm [-> SiLU]
  units on the kernels every family uses (SiLU is activation code 3 of the BatchNorm passes);
* the depthwise k x k convolution is Builder.depthwise_unit (vt_dwtile.hip) with `pool_out`: its normalise pass also writes
  the Squeeze-Excitation's per-image average (vt_bn_act_avgpool_*), so the expanded map -- six times as wide as the block, the
  largest tensor of the net -- is not read once more; in backward the pooled row's gradient joins d(y) in f32 inside the unit's
  BatchNorm backward (the addend of vt_bn_keep_bwd_*), not through a pass that adds it to the stored d(y);
* the Squeeze-Excitation is Builder.se_mlp with SiLU (squeeze widths max(1, block_in // 4)) and Builder.se_gate;
* stochastic depth.  Every torchvision EfficientNet has a non-zero `stochastic_depth_prob`: a residual block computes
  x + keep[b] * f(x) in training mode, keep[b] = bernoulli(1 - p) / (1 - p) per image ("row" mode), with
  p = sd_prob * block_index / total_blocks.  The factor rides on the unit that closes the block: its normalise pass and its
  BatchNorm backward are the keep passes of vt_mbconv.hip (Builder.conv_unit(..., keep=row)).  The factors of a forward are
  a table float[n_sites][B], one row per residual block in order, that lives in the program's arena and is written before each
  forward outside the launch list.  `set_keep_factors(t)` fixes the table -- on the eager path too -- instead of drawing.
  Eval mode, or sd_prob = 0, has no table and emits the ordinary residual passes.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Union

import torch
from torch import Tensor, nn

from ..components import StochasticDepth
from .base import BaseBackbone
from .patchconvnet import SqueezeExcitation
from .regnet import _make_divisible

__all__ = ["EfficientNetExtractor", "MBConv", "FusedMBConv"]

_SILU = 3  # activation code of the BatchNorm passes


def _cna(cin: int, cout: int, k: int, stride: int, groups: int, act: bool, bn_kw: dict) -> nn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm2d, [SiLU]"""
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, **bn_kw)]
    if act:
        layers.append(nn.SiLU(inplace=True))
    return nn.Sequential(*layers)


def _emit_cna(b, x, unit: nn.Sequential, name: str, residual=None, keep=None):
    return b.conv_unit(x, unit[0], unit[1], _SILU if len(unit) > 2 else 0, residual=residual, keep=keep, name=name)


class _Block(nn.Module):
    """what MBConv and FusedMBConv share: `block`, the shortcut where stride 1 and in == out, and StochasticDepth(p, "row") on
    the branch in front of it"""

    block: nn.Sequential

    def __init__(self, inp: int, oup: int, stride: int, sd_prob: float) -> None:
        super().__init__()
        self.use_res_connect = stride == 1 and inp == oup
        self.stochastic_depth = StochasticDepth(sd_prob)

    def drops(self) -> bool:
        """does this block multiply its branch by a per-image keep factor in the current mode?"""
        return self.use_res_connect and self.stochastic_depth.training

    def first_and_out(self, x: Tensor, keep: Optional[Tensor] = None) -> "tuple[Tensor, Tensor]":
        """(output of block.0, output of the block); `keep`: float[B] factors of the branch (None: no stochastic depth)"""
        first = self.block[0](x)
        h = first
        for m in list(self.block)[1:]:
            h = m(h)
        if self.use_res_connect:
            if keep is not None:
                h = h * keep.to(h.dtype).view(-1, 1, 1, 1)
            h = x + h
        return first, h

    def forward(self, x: Tensor) -> Tensor:
        keep = None
        if self.drops() and self.stochastic_depth.p > 0.0:
            survive = torch.full((x.shape[0],), 1.0 - self.stochastic_depth.p, dtype=torch.float32, device=x.device)
            keep = torch.bernoulli(survive) / survive
        return self.first_and_out(x, keep)[1]


class MBConv(_Block):
    """torchvision's efficientnet.MBConv: `block` = [expand 1x1 -BN-SiLU if the expanded width differs from the input width],
    depthwise k x k -BN-SiLU (stride), SqueezeExcitation(expanded, max(1, in // 4), SiLU), project 1x1 -BN"""

    def __init__(self, expand: float, k: int, stride: int, inp: int, oup: int, sd_prob: float, bn_kw: dict) -> None:
        super().__init__(inp, oup, stride, sd_prob)
        exp = _make_divisible(inp * expand, 8)
        layers: "list[nn.Module]" = []
        if exp != inp:
            layers.append(_cna(inp, exp, 1, 1, 1, True, bn_kw))
        layers.append(_cna(exp, exp, k, stride, exp, True, bn_kw))
        layers.append(SqueezeExcitation(exp, max(1, inp // 4), activation=nn.SiLU))
        layers.append(_cna(exp, oup, 1, 1, 1, False, bn_kw))
        self.block = nn.Sequential(*layers)

    def _vt_emit(self, b, x, name: str, keep=None, separate_pool: bool = False):
        h, first = x, None
        last = len(self.block) - 1
        pooled = None
        for i, m in enumerate(self.block):
            nm = f"{name}.block.{i}"
            if isinstance(m, SqueezeExcitation):
                if separate_pool:  # (measurement only: the pool as its own launch, what MobileNetV3 runs)
                    pooled = b.global_avgpool(h, nm + ".pool")
                h = b.se_gate(h, b.se_mlp(pooled, m.fc1, m.fc2, name=nm, act=_SILU), name=nm)
            elif m[0].groups > 1:
                pooled = None if separate_pool else b.act(x.B, 1, 1, m[0].out_channels, nm + ".pooled")
                h = b.depthwise_unit(h, m[0], m[1], _SILU, name=nm, pool_out=pooled)
            else:
                res = x if (i == last and self.use_res_connect) else None
                h = _emit_cna(b, h, m, nm, residual=res, keep=keep if res is not None else None)
            first = h if first is None else first
        return first, h


class FusedMBConv(_Block):
    """torchvision's efficientnet.FusedMBConv (no SE): `block` = 3x3 -BN-SiLU (stride, expanding), project 1x1 -BN; with expand
    ratio 1 the 3x3 -BN-SiLU unit alone"""

    def __init__(self, expand: float, k: int, stride: int, inp: int, oup: int, sd_prob: float, bn_kw: dict) -> None:
        super().__init__(inp, oup, stride, sd_prob)
        exp = _make_divisible(inp * expand, 8)
        if exp != inp:
            layers = [_cna(inp, exp, k, stride, 1, True, bn_kw), _cna(exp, oup, 1, 1, 1, False, bn_kw)]
        else:
            layers = [_cna(inp, oup, k, stride, 1, True, bn_kw)]
        self.block = nn.Sequential(*layers)

    def _vt_emit(self, b, x, name: str, keep=None, separate_pool: bool = False):
        h, first = x, None
        last = len(self.block) - 1
        for i, m in enumerate(self.block):
            res = x if (i == last and self.use_res_connect) else None
            h = _emit_cna(b, h, m, f"{name}.block.{i}", residual=res, keep=keep if res is not None else None)
            first = h if first is None else first
        return first, h


# (fused, expand, k, stride, in, out, layers) per stage
_B0 = [(False, 1, 3, 1, 32, 16, 1), (False, 6, 3, 2, 16, 24, 2), (False, 6, 5, 2, 24, 40, 2), (False, 6, 3, 2, 40, 80, 3),
       (False, 6, 5, 1, 80, 112, 3), (False, 6, 5, 2, 112, 192, 4), (False, 6, 3, 1, 192, 320, 1)]
_V2_S = [(True, 1, 3, 1, 24, 24, 2), (True, 4, 3, 2, 24, 48, 4), (True, 4, 3, 2, 48, 64, 4), (False, 4, 3, 2, 64, 128, 6),
         (False, 6, 3, 1, 128, 160, 9), (False, 6, 3, 2, 160, 256, 15)]
_V2_M = [(True, 1, 3, 1, 24, 24, 3), (True, 4, 3, 2, 24, 48, 5), (True, 4, 3, 2, 48, 80, 5), (False, 4, 3, 2, 80, 160, 7),
         (False, 6, 3, 1, 160, 176, 14), (False, 6, 3, 2, 176, 304, 18), (False, 6, 3, 1, 304, 512, 5)]
_V2_L = [(True, 1, 3, 1, 32, 32, 4), (True, 4, 3, 2, 32, 64, 7), (True, 4, 3, 2, 64, 96, 7), (False, 4, 3, 2, 96, 192, 10),
         (False, 6, 3, 1, 192, 224, 19), (False, 6, 3, 2, 224, 384, 25), (False, 6, 3, 1, 384, 640, 7)]
# name -> (width multiplier, depth multiplier, sd_prob, BatchNorm keywords).  The sd_prob values and the BatchNorm settings of
# b5 .. b7 and the V2 models are written from memory of torchvision's source; keys and counts do not depend on them.
_BN_B5 = dict(eps=0.001, momentum=0.01)
_BN_V2 = dict(eps=0.001)
_B_VARIANTS = {"efficientnet_b0": (1.0, 1.0, 0.2, {}), "efficientnet_b1": (1.0, 1.1, 0.2, {}), "efficientnet_b2": (1.1, 1.2, 0.3, {}),
               "efficientnet_b3": (1.2, 1.4, 0.3, {}), "efficientnet_b4": (1.4, 1.8, 0.4, {}),
               "efficientnet_b5": (1.6, 2.2, 0.4, _BN_B5), "efficientnet_b6": (1.8, 2.6, 0.5, _BN_B5),
               "efficientnet_b7": (2.0, 3.1, 0.5, _BN_B5)}
_V2_VARIANTS = {"efficientnet_v2_s": (_V2_S, 0.2), "efficientnet_v2_m": (_V2_M, 0.3), "efficientnet_v2_l": (_V2_L, 0.5)}
_NAMES = tuple(_B_VARIANTS) + tuple(_V2_VARIANTS)


def _stage_table(name: str):
    """(stages as (fused, expand, k, stride, in, out, layers), last width, sd_prob, BatchNorm keywords)"""
    if name in _V2_VARIANTS:
        table, sd = _V2_VARIANTS[name]
        return list(table), 1280, sd, dict(_BN_V2)
    wm, dm, sd, bn_kw = _B_VARIANTS[name]
    table = [(f, e, k, s, _make_divisible(i * wm, 8), _make_divisible(o * wm, 8), int(math.ceil(n * dm)))
             for f, e, k, s, i, o, n in _B0]
    return table, 4 * table[-1][5], sd, dict(bn_kw)


class _Features(nn.Module):
    """what create_feature_extractor keeps of a torchvision EfficientNet: `features`"""

    def __init__(self, name: str) -> None:
        super().__init__()
        table, last, sd_prob, bn_kw = _stage_table(name)
        layers: "list[nn.Module]" = [_cna(3, table[0][4], 3, 2, 1, True, bn_kw)]
        total = sum(t[6] for t in table)
        idx = 0
        for fused, e, k, s, cin, cout, n in table:
            stage = []
            for j in range(n):
                cls = FusedMBConv if fused else MBConv
                stage.append(cls(e, k, s if j == 0 else 1, cin if j == 0 else cout, cout, sd_prob * idx / total, bn_kw))
                idx += 1
            layers.append(nn.Sequential(*stage))
        layers.append(_cna(table[-1][5], last, 1, 1, 1, True, bn_kw))
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


class EfficientNetExtractor(BaseBackbone):
    """`EfficientNetExtractor(name)`, name one of efficientnet_b0 .. efficientnet_b7, efficientnet_v2_s / _m / _l: five feature
    maps -- `features.{i}.0.block.0` for i in (2, 3, 4, 6), then the last feature unit."""

    stage_indices = (2, 3, 4, 6)

    def __init__(self, name: str, pretrained: bool = False) -> None:
        if name not in _NAMES:
            raise ValueError(f"EfficientNetExtractor: unknown model {name!r} (one of {', '.join(_NAMES)})")
        if pretrained:
            raise NotImplementedError("EfficientNetExtractor(pretrained=True): nothing is downloaded here; load a local "
                                      "torchvision state_dict with load_torchvision_ckpt(path_or_state_dict)")
        super().__init__()
        self.model_name = name
        self.feat_extractor = _Features(name)
        feats = self.feat_extractor.features
        self.node_names = tuple(f"features.{i}.0.block.0" for i in self.stage_indices) + (f"features.{len(feats) - 1}",)
        self.out_channels_list = (*[feats[i][0].block[0][0].out_channels for i in self.stage_indices], feats[-1][0].out_channels)
        self.stride = 32
        self._keep_override: Optional[Tensor] = None
        self._separate_se_pool = False  # (measurement only: see MBConv._vt_emit)

    # -- stochastic depth ----------------------------------------------------------------
    def blocks(self) -> "list[_Block]":
        feats = self.feat_extractor.features
        return [blk for i in range(1, len(feats) - 1) for blk in feats[i]]

    def drop_rates(self) -> "tuple[float, ...]":
        """p = sd_prob * block_index / total_blocks of every block of the net, in order"""
        return tuple(blk.stochastic_depth.p for blk in self.blocks())

    def _sites(self) -> "list[_Block]":
        """the blocks that take a keep factor in the current mode: residual blocks in training mode; none at all where every
        rate is zero"""
        sites = [blk for blk in self.blocks() if blk.drops()]
        return sites if any(blk.stochastic_depth.p > 0.0 for blk in sites) else []

    def _vt_keep_rates(self) -> "tuple[float, ...]":
        """the drop probability of every site of the keep table (empty: this mode has no table); part of the program cache key"""
        return tuple(blk.stochastic_depth.p for blk in self._sites())

    @property
    def n_keep_sites(self) -> int:
        """rows of the keep table in training mode: the residual blocks"""
        return sum(blk.use_res_connect for blk in self.blocks())

    def set_keep_factors(self, t: Optional[Tensor]) -> None:
        """Fix the stochastic-depth keep factors of the following forwards: a float[n_keep_sites][B] tensor, one row per
        residual block in order and one factor per image (0 drops the image's branch, 1 / (1 - p) is what a kept one gets in
        training; any value is taken), used by the eager path and the launch-list engine alike instead of drawing.  None:
        draw again.  Eval mode ignores it."""
        if t is not None:
            if t.dim() != 2 or t.shape[0] != self.n_keep_sites:
                raise ValueError(f"keep factors of shape {tuple(t.shape)}: {self.model_name} has {self.n_keep_sites} residual "
                                 "blocks (rows), one column per image")
            t = t.detach().to(torch.float32).clone()
        self._keep_override = t

    # -- launch-list emission ----------------------------------------------------------
    def _vt_emit_maps(self, b, x):
        feats = self.feat_extractor.features
        if x.needs_grad:
            raise NotImplementedError(f"EfficientNetExtractor({self.model_name}): x.requires_grad -- the extractor forms no "
                                      "gradient of the image (its input is the data; pass images that do not require a gradient)")
        sites = self._sites()
        rows = dict(zip(map(id, sites), b.keep_table([blk.stochastic_depth.p for blk in sites], x.B))) if sites else {}
        o = _emit_cna(b, x, feats[0], "features.0")
        maps = []
        for i in range(1, len(feats) - 1):
            for j, blk in enumerate(feats[i]):
                first, o = blk._vt_emit(b, o, f"features.{i}.{j}", rows.get(id(blk)), self._separate_se_pool)
                if j == 0 and i in self.stage_indices:
                    maps.append(first)
        maps.append(_emit_cna(b, o, feats[-1], f"features.{len(feats) - 1}"))
        return maps

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        feats = self.feat_extractor.features
        sites = self._sites()
        keep = {}
        if sites:
            from ..program import draw_keep_factors

            table = draw_keep_factors([blk.stochastic_depth.p for blk in sites], x.shape[0], x.device, self._keep_override)
            keep = {id(blk): table[r] for r, blk in enumerate(sites)}
        h, maps = feats[0](x), []
        for i in range(1, len(feats) - 1):
            for j, blk in enumerate(feats[i]):
                first, h = blk.first_and_out(h, keep.get(id(blk)))
                if j == 0 and i in self.stage_indices:
                    maps.append(first)
        maps.append(feats[-1](h))
        return maps

    # -- checkpoints ---------------------------------------------------------------------
    def load_torchvision_ckpt(self, path_or_state_dict: "Union[str, os.PathLike, dict[str, Tensor]]") -> None:
        """Load a LOCAL torchvision EfficientNet state_dict (a dict, or the path of a file torch.load reads): `classifier.*` is
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
