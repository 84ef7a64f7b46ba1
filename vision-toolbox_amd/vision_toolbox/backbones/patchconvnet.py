"""PatchConvNet, "Augmenting Convolutional networks with attention-based aggregation" (https://arxiv.org/abs/2112.13692)
on libvt_amd.

Constructor signatures, child names and child indices follow the reference (vision_toolbox/backbones/patchconvnet.py:25-166),
so state_dict keys and shapes are the reference's: `stem.{0,2,4,6}.weight`, `trunk.{1..depth}.layers.{0,1,3,5.fc1,5.fc2,6}`
(bn blocks) or `layers.{0,1,4,6.fc1,6.fc2,8}` (ln blocks), `trunk.i.layer_scale` ((C, 1, 1) for bn, (C,) for ln),
`pool.cls_token` (C,), `pool.attn.in_proj_weight` (3C, C), `pool.attn.in_proj_bias`, `pool.attn.out_proj`, `pool.norm_1|2|3`,
`pool.mlp.0|2`, `pool.layer_scale_1|2` and the BatchNorm buffers.

The reference imports StochasticDepth and SqueezeExcitation from torchvision; this package does not import torchvision.
`SqueezeExcitation` here is a module of our own with torchvision's child names (`avgpool`, `fc1`, `fc2` as 1x1 nn.Conv2d,
`activation`, `scale_activation`), and drop path is the package's `StochasticDepth` (nn.Identity where the rate is 0, as in the
reference).

The launch lists.  The stem is four bias-free 3x3 stride-2 convolutions with GELU behind the first three.  A block is

    vt_channel_stats + BatchNorm finalize / normalise   (bn blocks; vt_layernorm_fwd in ln blocks)
    vt_conv_igemm + GELU                                1x1 (+ bias)
    vt_dw3_gelu_pool_fwd                                depthwise 3x3 + bias + GELU and the SE's average pool, one launch
    vt_conv_igemm x 2                                   the SE's fc1 + ReLU and fc2 on [B, 1, 1, C] rows
    vt_se_gate_fwd                                      a * sigmoid(s)
    vt_conv_igemm                                       1x1 (+ bias)
    vt_scale_residual_fwd                               x + layer_scale * branch

The map is NHWC on the GPU in both variants, so the reference's Permute modules are views there.  `AttentionPooling`:
vt_token_prepend_fwd (the class row in front), vt_layernorm_fwd, the q projection on the class row alone and the k | v
projections of all rows as ONE GEMM into a [B, 1, Lk, 2C] buffer (row slices of `in_proj_weight` / `in_proj_bias`),
vt_pool_attn_fwd (one head as wide as the embedding), out_proj, vt_scale_residual_fwd onto the class row, then the MLP half
and norm_3.  `forward(imgs)` returns (B, C).

Refused on CUDA tensors with NotImplementedError (all of them construct and run on CPU tensors): `drop_path > 0` in training
mode (the reference default is 0.3: pass drop_path=0.0 to train on the GPU), an `embed_dim` whose `embed_dim // 8` -- the
first stem width -- is no whole 16-byte chunk of the compute dtype, and a token map too large for the plane kernels.
"""
from __future__ import annotations

from functools import partial

import torch
from torch import Tensor, nn

from ..components import Permute, StochasticDepth
from .base import BaseBackbone

__all__ = ["SqueezeExcitation", "PatchConvBlockLN", "PatchConvBlockBN", "AttentionPooling", "PatchConvNet"]


class SqueezeExcitation(nn.Module):
    """scale * input with scale = scale_activation(fc2(activation(fc1(avgpool(input))))) (child names of torchvision's)"""

    def __init__(self, input_channels: int, squeeze_channels: int, activation=nn.ReLU, scale_activation=nn.Sigmoid) -> None:
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = activation()
        self.scale_activation = scale_activation()

    def forward(self, input: Tensor) -> Tensor:
        scale = self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(input)))))
        return scale * input


def _drop_path(p: float) -> nn.Module:
    return StochasticDepth(p) if p > 0 else nn.Identity()


def _drop_refusal(*mods: nn.Module) -> "str | None":
    if any(isinstance(m, StochasticDepth) and m.training and m.p > 0.0 for m in mods):
        return ("drop_path > 0 in training mode has no kernel on the MI355X path (pass drop_path=0.0; eval mode and CPU "
                "tensors run)")
    return None


class _PatchConvBlock(nn.Module):
    _IDX: "tuple[int, int, int, int, int]"  # norm, first 1x1 / Linear, depthwise, SE, last 1x1 / Linear

    def forward(self, x: Tensor) -> Tensor:  # the CPU path
        if x.is_cuda:
            raise NotImplementedError(f"a {type(self).__name__} takes a feature map: on the GPU it runs as part of a "
                                      "PatchConvNet program")
        return self._eager(x)

    def _eager(self, x: Tensor) -> Tensor:
        return x + self.drop_path(self.layers(x) * self.layer_scale)

    def _vt_refusal(self) -> "str | None":
        return _drop_refusal(self.drop_path)

    def _vt_emit(self, b, x, name: str = "block"):
        """x: the NHWC map [B, H, W, C]"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        i_norm, i_in, i_dw, i_se, i_out = self._IDX
        L = self.layers
        lname = lambda i: f"{name}.layers.{i}"
        if isinstance(L[i_norm], nn.BatchNorm2d):
            n = b.batch_norm(x, L[i_norm], name=lname(i_norm))
            h = b.conv_unit(n, L[i_in], None, 4, name=lname(i_in))
        else:
            n = b.layer_norm(x, L[i_norm], name=lname(i_norm))
            h = b.linear_unit(n, L[i_in], act=4, name=lname(i_in))
        a, pooled = b.dw3_gelu_pool(h, L[i_dw], name=lname(i_dw))
        se = L[i_se]
        s = b.conv_unit(pooled, se.fc1, None, 1, name=lname(i_se) + ".fc1")
        s = b.conv_unit(s, se.fc2, None, 0, name=lname(i_se) + ".fc2")
        g = b.se_gate(a, s, name=lname(i_se))
        if isinstance(L[i_out], nn.Conv2d):
            t = b.conv_unit(g, L[i_out], None, 0, name=lname(i_out))
        else:
            t = b.linear_unit(g, L[i_out], name=lname(i_out))
        return b.scale_residual(t, self.layer_scale, x, name=name + ".add")


class PatchConvBlockLN(_PatchConvBlock):
    _IDX = (0, 1, 4, 6, 8)

    def __init__(self, embed_dim: int, drop_path: float = 0.3, layer_scale_init: float = 1e-6) -> None:
        super().__init__()
        # LayerNorm version.  Primary format is (N, H, W, C)
        self.layers = nn.Sequential(
            nn.LayerNorm(embed_dim),
            nn.Linear(embed_dim, embed_dim),
            nn.GELU(),
            Permute(0, 3, 1, 2),  # (N, H, W, C) -> (N, C, H, W)
            nn.Conv2d(embed_dim, embed_dim, 3, padding=1, groups=embed_dim),
            nn.GELU(),
            SqueezeExcitation(embed_dim, embed_dim // 4),
            Permute(0, 2, 3, 1),  # (N, C, H, W) -> (N, H, W, C)
            nn.Linear(embed_dim, embed_dim),
        )
        self.layer_scale = nn.Parameter(torch.full((embed_dim,), layer_scale_init))
        self.drop_path = _drop_path(drop_path)


class PatchConvBlockBN(_PatchConvBlock):
    _IDX = (0, 1, 3, 5, 6)

    def __init__(self, embed_dim: int, drop_path: float = 0.3, layer_scale_init: float = 1e-6) -> None:
        super().__init__()
        # BatchNorm version.  Primary format is (N, C, H, W)
        self.layers = nn.Sequential(
            nn.BatchNorm2d(embed_dim),
            nn.Conv2d(embed_dim, embed_dim, 1),
            nn.GELU(),
            nn.Conv2d(embed_dim, embed_dim, 3, padding=1, groups=embed_dim),
            nn.GELU(),
            SqueezeExcitation(embed_dim, embed_dim // 4),
            nn.Conv2d(embed_dim, embed_dim, 1),
        )
        self.layer_scale = nn.Parameter(torch.full((embed_dim, 1, 1), layer_scale_init))
        self.drop_path = _drop_path(drop_path)


class AttentionPooling(nn.Module):
    def __init__(self, embed_dim: int, mlp_ratio: int = 3, drop_path: float = 0.3, layer_scale_init: float = 1e-6) -> None:
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(embed_dim))

        self.norm_1 = nn.LayerNorm(embed_dim)
        self.attn = nn.MultiheadAttention(embed_dim, 1, batch_first=True)
        self.layer_scale_1 = nn.Parameter(torch.full((embed_dim,), layer_scale_init))
        self.drop_path1 = _drop_path(drop_path)

        self.norm_2 = nn.LayerNorm(embed_dim)
        mlp_dim = int(embed_dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(embed_dim, mlp_dim), nn.GELU(), nn.Linear(mlp_dim, embed_dim))
        self.layer_scale_2 = nn.Parameter(torch.full((embed_dim,), layer_scale_init))
        self.drop_path2 = _drop_path(drop_path)

        self.norm_3 = nn.LayerNorm(embed_dim)

    def forward(self, x: Tensor) -> Tensor:  # (N, HW, C) -> (N, C); the CPU path
        if x.is_cuda:
            raise NotImplementedError("an AttentionPooling takes a token map: on the GPU it runs as part of a PatchConvNet "
                                      "program")
        return self._eager(x)

    def _eager(self, x: Tensor) -> Tensor:
        cls_token = self.cls_token.expand(x.shape[0], 1, -1)
        out = torch.cat((cls_token, x), dim=1)

        # attention pooling.  q = cls_token.  k = v = (cls_token, x)
        out = self.norm_1(out)
        out = self.attn(out[:, :1], out, out, need_weights=False)[0]
        cls_token = cls_token + self.drop_path1(out * self.layer_scale_1)

        out = self.mlp(self.norm_2(cls_token))
        cls_token = cls_token + self.drop_path2(out * self.layer_scale_2)
        return self.norm_3(cls_token).squeeze(1)

    def _vt_refusal(self) -> "str | None":
        return _drop_refusal(self.drop_path1, self.drop_path2)

    def _vt_emit(self, b, x, name: str = "pool"):
        """x: the token map [B, 1, HW, C] -> [B, 1, 1, C]"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import ConvSpec, _PSlice

        C, attn = x.C, self.attn
        w, bias = attn.in_proj_weight, attn.in_proj_bias
        if w is None or bias is None or attn.bias_k is not None or tuple(w.shape) != (3 * C, C):
            raise NotImplementedError(f"{name}.attn: a biased nn.MultiheadAttention({C}, 1) with one in_proj_weight")
        cat = b.token_prepend(x, self.cls_token, name=name + ".cat")
        c0 = b.token_select(cat, 0, name=name + ".cls")  # the broadcast class row: the shortcut
        n = b.layer_norm(cat, self.norm_1, name=name + ".norm_1")
        n0 = b.token_select(n, 0, name=name + ".query")
        # row views of the one in_proj parameter: q from the class row alone, k | v from all rows as one GEMM
        q_spec = ConvSpec(1, 1, 0, 1, 1, C, C, _PSlice(w, 0, C * C), _PSlice(bias, 0, C), is_slice=True)
        kv_spec = ConvSpec(1, 1, 0, 1, 1, C, 2 * C, _PSlice(w, C * C, 2 * C * C), _PSlice(bias, C, 2 * C), is_slice=True)
        q = b.conv_unit(n0, q_spec, None, 0, name=name + ".attn.q")
        kv = b.conv_unit(n, kv_spec, None, 0, name=name + ".attn.kv")
        o = b.pool_attention(q, kv.sl(0, C), kv.sl(C, C), name=name + ".attn.attention")
        t = b.linear_unit(o, attn.out_proj, name=name + ".attn.out_proj")
        c = b.scale_residual(t, self.layer_scale_1, c0, name=name + ".add_1")
        m = b.layer_norm(c, self.norm_2, name=name + ".norm_2")
        h = b.linear_unit(m, self.mlp[0], act=4, name=name + ".mlp.0")
        t = b.linear_unit(h, self.mlp[2], name=name + ".mlp.2")
        c = b.scale_residual(t, self.layer_scale_2, c, name=name + ".add_2")
        return b.layer_norm(c, self.norm_3, name=name + ".norm_3")


class PatchConvNet(BaseBackbone):
    def __init__(
        self,
        embed_dim: int,
        depth: int,
        mlp_ratio: int = 3,
        drop_path: float = 0.3,
        layer_scale_init: float = 1e-6,
        norm_type: str = "bn",
    ) -> None:
        assert norm_type in ("bn", "ln")
        super().__init__()
        self.norm_type = norm_type
        self.out_channels_list = (embed_dim,)
        self.stride = 16

        # the stem has no bias and no last activation layer
        conv3x3_s2 = partial(nn.Conv2d, kernel_size=3, stride=2, padding=1, bias=False)
        self.stem = nn.Sequential(
            conv3x3_s2(3, embed_dim // 8),
            nn.GELU(),
            conv3x3_s2(embed_dim // 8, embed_dim // 4),
            nn.GELU(),
            conv3x3_s2(embed_dim // 4, embed_dim // 2),
            nn.GELU(),
            conv3x3_s2(embed_dim // 2, embed_dim),
        )

        blk = PatchConvBlockLN if norm_type == "ln" else PatchConvBlockBN
        self.trunk = nn.Sequential(
            Permute(0, 2, 3, 1) if norm_type == "ln" else nn.Identity(),
            *[blk(embed_dim, drop_path, layer_scale_init) for _ in range(depth)],
            Permute(0, 2, 3, 1) if norm_type == "bn" else nn.Identity(),
        )
        self.pool = AttentionPooling(embed_dim, mlp_ratio, drop_path, layer_scale_init)

        nn.init.trunc_normal_(self.pool.cls_token, std=0.02)
        nn.init.trunc_normal_(self.pool.attn.in_proj_weight, std=0.02)
        nn.init.trunc_normal_(self.pool.attn.out_proj.weight, std=0.02)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    # -- launch-list emission ---------------------------------------------------------------------
    def _blocks(self):
        return [m for m in self.trunk if isinstance(m, _PatchConvBlock)]

    def _vt_refusal(self, dtype: "int | None" = None, hw: "tuple[int, int] | None" = None) -> "str | None":
        for m in (*self._blocks(), self.pool):
            why = m._vt_refusal()
            if why is not None:
                return why
        if dtype is not None:
            from .. import _native as N

            epc = 8 if dtype == N.VT_BF16 else 4
            c8 = self.stem[0].out_channels
            if c8 % epc:
                return (f"embed_dim={self.out_channels_list[0]}: the first stem width embed_dim // 8 = {c8} is no whole 16-byte "
                        f"chunk of the compute dtype ({epc} elements)")
            if hw is not None and self._blocks():
                H, W = hw
                for _ in range(4):
                    H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                if not N.lib().vt_dw3_gelu_pool_supported(H, W, dtype):
                    return (f"a {H}x{W} token map is too large for the plane kernels: the planes of one 16-byte channel slab "
                            "with their halo must fit 160 KiB of LDS")
        return None

    def _vt_emit_maps(self, b, x):
        why = self._vt_refusal(b.dtype, (x.H, x.W))
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import TRef

        o = x
        for i in (0, 2, 4, 6):
            o = b.conv_unit(o, self.stem[i], None, 4 if i < 6 else 0, name=f"stem.{i}")
        for i, blk in enumerate(self.trunk):
            if isinstance(blk, _PatchConvBlock):
                o = blk._vt_emit(b, o, name=f"trunk.{i}")
        # (N, H, W, C) -> (N, HW, C): the same buffer as a token map
        tok = TRef(o.buf, o.B, 1, o.H * o.W, o.C, o.ld, o.coff, o.dtype, o.needs_grad)
        return [self.pool._vt_emit(b, tok, name="pool")]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        out = self.trunk(self.stem(x))
        return [self.pool(out.flatten(1, 2))]

    def _gpu_check(self, x: Tensor) -> None:
        from ..program import resolve_dtype

        why = self._vt_refusal(resolve_dtype(x, self.compute_dtype), tuple(x.shape[2:]) if x.dim() == 4 else None)
        if why is not None:
            raise NotImplementedError(why)

    def get_feature_maps(self, x: Tensor) -> "list[Tensor]":
        if isinstance(x, Tensor) and x.is_cuda:
            self._gpu_check(x)
        y = self._vt_runner()(x, all_maps=True, compute_dtype=self.compute_dtype)[-1]
        return [y.flatten(1) if x.is_cuda else y]  # (B, C, 1, 1) -> (B, C)

    def forward(self, x: Tensor) -> Tensor:
        return self.get_feature_maps(x)[-1]

    @staticmethod
    def from_config(variant: str, depth: int, pretrained: bool = False) -> "PatchConvNet":
        """`variant`: S / B / L = embed_dim 384 / 768 / 1024.  Nothing is fetched: `pretrained=True` raises."""
        embed_dim = dict(S=384, B=768, L=1024)[variant]
        if pretrained:
            raise ValueError("pretrained=True: no checkpoints are published for PatchConvNet and this build downloads nothing")
        return PatchConvNet(embed_dim, depth)
