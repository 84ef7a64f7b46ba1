"""ConvNeXt (V1; V2 on the CPU path only) on libvt_amd.

Constructor signatures, child names and child indices follow the reference
(vision_toolbox/backbones/convnext.py:15-110), so state_dict keys are the reference's:
`stem.0` (4x4 stride-4 conv) / `stem.2` (LayerNorm); `stages.S.0` = the downsample
(`.0` LayerNorm, `.2` 2x2 stride-2 conv; nn.Identity for stage 0); `stages.S.B.layers.1`
(depthwise 7x7), `.3` (LayerNorm), `.4` / `.7` (the two nn.Linear), `.6` (GlobalResponseNorm,
V2), `.8.gamma` (LayerScale); `norm` (head LayerNorm).

The reference permutes every block to NHWC for LayerNorm / Linear and back for the conv;
the launch lists here are NHWC throughout, so the Permute children never run on the GPU.
A block is six forward launches ("ConvNeXt"):

    vt_dwconv_fwd            depthwise 7x7 WITHOUT its bias
    vt_layernorm_fwd         LayerNorm over C of (z + dwconv.bias): the bias costs no pass
    vt_conv_igemm            Linear(C, 4C) + bias as a 1x1 conv, then
    vt_bn_act_apply          exact GELU (activation code 4; the pre-activation stays for backward)
    vt_conv_igemm            Linear(4C, C) + bias
    vt_scale_residual_fwd    x + gamma * t

`forward(x)` = norm(mean over H, W), shape (B, C), computed inside the program;
`get_feature_maps(x)` = [last stage's map shaped (B, H, W, C)] as the reference returns it.

Refused on the GPU (NotImplementedError; both construct and run on CPU tensors): `v2=True`
(GlobalResponseNorm needs a per-image reduction kernel of its own) and `stochastic_depth > 0`
in training mode.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from ..components import HipModule, LayerScale, Permute, StochasticDepth
from .base import BaseBackbone

__all__ = ["ConvNeXt", "ConvNeXtBlock", "GlobalResponseNorm"]


class GlobalResponseNorm(nn.Module):
    """ConvNeXt-V2: x + gamma * x * (||x||_HW / mean_C ||x||_HW) + beta over an NHWC map (CPU path only)."""

    def __init__(self, dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(dim))
        self.beta = nn.Parameter(torch.zeros(dim))
        self.eps = eps

    def forward(self, x: Tensor) -> Tensor:
        energy = x.square().sum(dim=(1, 2), keepdim=True).sqrt()  # (B, 1, 1, C)
        ratio = energy / (energy.mean(dim=-1, keepdim=True) + self.eps)
        return x * (1.0 + ratio * self.gamma) + self.beta


class ConvNeXtBlock(HipModule):
    def __init__(
        self,
        d_model: int,
        expansion_ratio: float = 4.0,
        bias: bool = True,
        layer_scale_init: Optional[float] = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
        v2: bool = False,
    ) -> None:
        super().__init__()
        if v2:
            layer_scale_init = None
        hidden = int(d_model * expansion_ratio)
        self.layers = nn.Sequential(
            Permute(0, 3, 1, 2),
            nn.Conv2d(d_model, d_model, 7, padding=3, groups=d_model, bias=bias),
            Permute(0, 2, 3, 1),
            nn.LayerNorm(d_model, norm_eps),
            nn.Linear(d_model, hidden, bias=bias),
            nn.GELU(),
            GlobalResponseNorm(hidden) if v2 else nn.Identity(),
            nn.Linear(hidden, d_model, bias=bias),
            LayerScale(d_model, layer_scale_init) if layer_scale_init is not None else nn.Identity(),
            StochasticDepth(stochastic_depth),
        )

    def _vt_refusal(self) -> Optional[str]:
        if isinstance(self.layers[6], GlobalResponseNorm):
            return "ConvNeXt-V2: GlobalResponseNorm has no kernel on the MI355X path yet (it runs on CPU tensors)"
        if self.training and self.layers[9].p > 0.0:
            return "stochastic_depth > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        return None

    def _vt_emit(self, b, x, out=None, name: str = "block"):
        """x: NHWC map -> x + gamma * mlp(LayerNorm(dwconv(x)))"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        L = self.layers
        dw, ln, fc1, fc2, ls = L[1], L[3], L[4], L[7], L[8]
        z = b.depthwise_no_bias(x, dw, name=name + ".layers.1")
        n = b.layer_norm(z, ln, pre_bias=dw.bias, name=name + ".layers.3")
        h = b.linear_unit(n, fc1, act=4, name=name + ".layers.4")
        t = b.linear_unit(h, fc2, name=name + ".layers.7")
        gamma = ls.gamma if isinstance(ls, LayerScale) else None
        return b.scale_residual(t, gamma, x, out=out, name=name + ".layers.8")

    def _vt_emit_maps(self, b, x):
        raise NotImplementedError("a ConvNeXtBlock takes an NHWC map: on the GPU it runs as part of a ConvNeXt program")

    def forward(self, x: Tensor) -> Tensor:  # (B, H, W, C), as in the reference
        if x.is_cuda:
            raise NotImplementedError("a ConvNeXtBlock takes an NHWC map: on the GPU it runs as part of a ConvNeXt program")
        return x + self.layers(x)


class ConvNeXt(BaseBackbone):
    def __init__(
        self,
        d_model: int,
        depths: "tuple[int, ...]",
        expansion_ratio: float = 4.0,
        bias: bool = True,
        layer_scale_init: Optional[float] = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
        v2: bool = False,
    ) -> None:
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, d_model, 4, 4), Permute(0, 2, 3, 1), nn.LayerNorm(d_model, norm_eps))
        n_blocks = sum(depths)
        rates = [stochastic_depth * i / (n_blocks - 1) if n_blocks > 1 else 0.0 for i in range(n_blocks)]
        self.stages = nn.Sequential()
        widths, k = [], 0
        for si, depth in enumerate(depths):
            stage = nn.Sequential()
            if si == 0:
                stage.append(nn.Identity())
            else:
                stage.append(nn.Sequential(
                    nn.LayerNorm(d_model, norm_eps),
                    Permute(0, 3, 1, 2),
                    nn.Conv2d(d_model, 2 * d_model, 2, 2),
                    Permute(0, 2, 3, 1),
                ))
                d_model *= 2
            for _ in range(depth):
                stage.append(ConvNeXtBlock(d_model, expansion_ratio, bias, layer_scale_init, rates[k], norm_eps, v2))
                k += 1
            self.stages.append(stage)
            widths.append(d_model)
        self.norm = nn.LayerNorm(d_model, norm_eps)
        self.out_channels_list = tuple(widths)
        self.stride = 4 * 2 ** (len(depths) - 1)

    # -- launch-list emission: [last map, head] ---------------------------------------------------
    def _vt_emit_maps(self, b, x):
        o = b.conv_unit(x, self.stem[0], None, 0, name="stem.0")
        o = b.layer_norm(o, self.stem[2], name="stem.2")
        for si, stage in enumerate(self.stages):
            for bi, m in enumerate(stage):
                if isinstance(m, ConvNeXtBlock):
                    o = m._vt_emit(b, o, name=f"stages.{si}.{bi}")
                elif not isinstance(m, nn.Identity):
                    o = b.layer_norm(o, m[0], name=f"stages.{si}.0.0")
                    o = b.conv_unit(o, m[2], None, 0, name=f"stages.{si}.0.2")
        pooled = b.global_avgpool(o, name="pool")
        head = b.layer_norm(pooled, self.norm, name="norm")
        return [o, head]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        f = self.stages(self.stem(x))  # (B, H, W, C)
        return [f, self.norm(f.mean(dim=(1, 2)))]

    def _vt_check(self, x: Tensor) -> None:
        if isinstance(x, Tensor) and x.is_cuda:
            for m in self.modules():
                if isinstance(m, ConvNeXtBlock):
                    why = m._vt_refusal()
                    if why is not None:
                        raise NotImplementedError(why)

    def get_feature_maps(self, x: Tensor) -> "list[Tensor]":
        self._vt_check(x)
        f = self._vt_runner()(x, all_maps=True, compute_dtype=self.compute_dtype)[0]
        # the runner hands back a logical-NCHW tensor with channels-last strides: (B, H, W, C) is a free view of it
        return [f.permute(0, 2, 3, 1) if x.is_cuda else f]

    def forward(self, x: Tensor) -> Tensor:
        self._vt_check(x)
        y = self._vt_runner()(x, all_maps=False, compute_dtype=self.compute_dtype)[-1]
        return y.flatten(1) if x.is_cuda else y  # (B, C, 1, 1) -> (B, C)

    _VARIANTS = {
        "A": (40, (2, 2, 6, 2)),
        "F": (48, (2, 2, 6, 2)),
        "P": (64, (2, 2, 6, 2)),
        "N": (80, (2, 2, 8, 2)),
        "T": (96, (3, 3, 9, 3)),
        "S": (96, (3, 3, 27, 3)),
        "B": (128, (3, 3, 27, 3)),
        "L": (192, (3, 3, 27, 3)),
        "XL": (256, (3, 3, 27, 3)),
        "H": (352, (3, 3, 27, 3)),
    }
    _V1_URL = "https://dl.fbaipublicfiles.com/convnext/"
    _V1_CKPTS = {
        "T": "convnext_tiny_22k_224.pth",
        "S": "convnext_small_22k_224.pth",
        "B": "convnext_base_22k_224.pth",
        "L": "convnext_large_22k_224.pth",
        "XL": "convnext_xlarge_22k_224.pth",
    }
    _V2_URL = "https://dl.fbaipublicfiles.com/convnext/convnextv2/pt_only/"
    _V2_CKPTS = {
        "A": "convnextv2_atto_1k_224_fcmae.pt",
        "F": "convnextv2_femto_1k_224_fcmae.pt",
        "P": "convnextv2_pico_1k_224_fcmae.pt",
        "N": "convnextv2_nano_1k_224_fcmae.pt",
        "T": "convnextv2_tiny_1k_224_fcmae.pt",
        "B": "convnextv2_base_1k_224_fcmae.pt",
        "L": "convnextv2_large_1k_224_fcmae.pt",
        "H": "convnextv2_huge_1k_224_fcmae.pt",
    }

    @staticmethod
    def from_config(variant: str, v2: bool = False, pretrained: bool = False) -> "ConvNeXt":
        d_model, depths = ConvNeXt._VARIANTS[variant]
        m = ConvNeXt(d_model, depths, v2=v2)
        if pretrained:
            url = (ConvNeXt._V2_URL + ConvNeXt._V2_CKPTS[variant]) if v2 else (ConvNeXt._V1_URL + ConvNeXt._V1_CKPTS[variant])
            m.load_official_ckpt(torch.hub.load_state_dict_from_url(url)["model"])
        return m

    @torch.no_grad()
    def load_official_ckpt(self, state_dict: "dict[str, Tensor]") -> None:
        """copy a checkpoint in the official ConvNeXt key layout (`downsample_layers.i.j`,
        `stages.i.j.{dwconv,norm,pwconv1,grn,pwconv2,gamma}`, `norm`) into this module.  Every key must be
        consumed; what may remain is the classifier head (`head.weight`, `head.bias`) next to `norm`."""
        left = dict(state_dict)

        def take(dst: Tensor, key: str) -> None:
            dst.copy_(left.pop(key).reshape(dst.shape))

        pairs = [(self.stem[0], "downsample_layers.0.0"), (self.stem[2], "downsample_layers.0.1")]
        for si, stage in enumerate(self.stages):
            if si > 0:
                pairs += [(stage[0][0], f"downsample_layers.{si}.0"), (stage[0][2], f"downsample_layers.{si}.1")]
            for bi, block in enumerate(list(stage)[1:]):
                src, L = f"stages.{si}.{bi}.", block.layers
                pairs += [(L[1], src + "dwconv"), (L[3], src + "norm"), (L[4], src + "pwconv1"), (L[7], src + "pwconv2")]
                if isinstance(L[6], GlobalResponseNorm):
                    take(L[6].gamma, src + "grn.gamma")
                    take(L[6].beta, src + "grn.beta")
                if isinstance(L[8], LayerScale):
                    take(L[8].gamma, src + "gamma")
        has_norm = "norm.weight" in left  # (the self-supervised V2 checkpoints carry no head norm)
        if has_norm:
            pairs.append((self.norm, "norm"))
        for mod, key in pairs:
            take(mod.weight, key + ".weight")
            if mod.bias is not None:
                take(mod.bias, key + ".bias")
        allowed = {"head.weight", "head.bias"} if has_norm else set()
        extra = sorted(set(left) - allowed)
        if extra:
            raise KeyError(f"load_official_ckpt: unexpected keys {extra}")
