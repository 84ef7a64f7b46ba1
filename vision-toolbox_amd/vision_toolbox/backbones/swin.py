"""Swin Transformer (https://arxiv.org/abs/2103.14030) on libvt_amd.

Constructor signatures, child names and child indices follow the reference (vision_toolbox/backbones/swin.py:16-263), so
state_dict keys are the reference's: `patch_embed`, `patch_norm`, `stages.s.0` (PatchMerging: `norm`, `reduction`; an Identity
in stage 0), `stages.s.i.mha.0` (LayerNorm), `stages.s.i.mha.1` (`q_proj`, `k_proj`, `v_proj`, `out_proj`,
`relative_pe_table`), `stages.s.i.mha.2.gamma` (LayerScale, where there is one), `stages.s.i.mlp.*` as in a ViTBlock, `norm`.
The buffers `attn_mask` and `relative_pe_index` are non-persistent.

The shift mask at batch > 1.  The reference adds its (windows, 1, L, L) mask to a (1, heads, L, L) bias and hands the
(windows, heads, L, L) result to scaled_dot_product_attention over (B * windows, heads, L, head_dim) operands, which cannot
broadcast it: its shifted blocks raise at batch > 1.  This class TILES the mask over the batch -- identical at batch 1, and the
evident intent at batch > 1 -- on both paths.

The launch lists keep one layout, the NHWC map [B, H, W, C] in un-rolled pixel order.  `window_partition`, both `roll`s and
`window_unpartition` are index arithmetic inside the attention kernel's loads and stores: no map is gathered, rolled or
copied.  Per block, the list of a ViTBlock with the window kernel in place of the global one:

    vt_layernorm_fwd         mha.0
    vt_conv_igemm x 3        q_proj, k_proj, v_proj + bias as 1x1 convs into the slices of the qkv buffer
    vt_win_attn_fwd          softmax(q k^T / sqrt(head_dim) + table[relative index] (+ mask)) v per (window, head)
    vt_conv_igemm            out_proj + bias
    vt_scale_residual_fwd    shortcut + gamma * branch (gamma None: the plain add)
    vt_layernorm_fwd         mlp.0
    vt_conv_igemm            linear1 + bias, then vt_bn_act_apply: exact GELU
    vt_conv_igemm            linear2 + bias
    vt_scale_residual_fwd

in front of them vt_patchify_fwd + one vt_conv_igemm (the patch embedding) and vt_layernorm_fwd (patch_norm); between the
stages PatchMerging = vt_patchify_fwd with p = 2 (its (dy, dx, c) order is the reference's view / transpose / flatten order),
vt_layernorm_fwd over 4 C and the bias-free reduction as a 1x1 conv; behind them vt_layernorm_fwd (norm) and the mean over
the pixels.  `forward(imgs)` returns (B, C); `get_feature_maps(imgs)` the four (B, H_i, W_i, C_i) stage outputs.

Refused on CUDA tensors (all of them construct and run on CPU tensors): a window of more than 64 tokens (window_size 14, the
S3 variants), a `head_dim` other than 32, `bias=False`, `dropout > 0` or `stochastic_depth > 0` in training mode
(NotImplementedError).
"""
from __future__ import annotations

from functools import partial

import torch
from torch import Tensor, nn

from .base import BaseBackbone
from .vit import MHA, ViTBlock

__all__ = ["window_partition", "window_unpartition", "WindowAttention", "SwinBlock", "PatchMerging", "SwinTransformer"]


def window_partition(x: Tensor, window_size: int) -> "tuple[Tensor, int, int]":
    """(B, H, W, C) -> (B * windows, window_size^2, C), windows row-major, tokens row-major inside a window"""
    ws = window_size
    batch, height, width, chans = x.shape
    rows, cols = height // ws, width // ws
    tiles = x.reshape(batch, rows, ws, cols, ws, chans).permute(0, 1, 3, 2, 4, 5)
    return tiles.reshape(batch * rows * cols, ws * ws, chans), rows, cols


def window_unpartition(x: Tensor, window_size: int, nH: int, nW: int) -> Tensor:
    """the inverse of window_partition: (B * nH * nW, window_size^2, C) -> (B, nH window_size, nW window_size, C)"""
    ws = window_size
    tiles = x.reshape(-1, nH, nW, ws, ws, x.shape[-1]).permute(0, 1, 3, 2, 4, 5)
    return tiles.reshape(tiles.shape[0], nH * ws, nW * ws, x.shape[-1])


def _axis_regions(n: int, ws: int, shift: int) -> Tensor:
    """vt_win_region of vt_window_index.h for every rolled coordinate of an axis of n pixels: 0 below n - ws, 1 below
    n - shift, 2 from there (the pixels that the roll wrapped around); shift = 0 is one region"""
    c = torch.arange(n)
    return ((c >= n - ws).long() + (c >= n - shift).long()) if shift > 0 else torch.zeros_like(c)


def shift_mask(H: int, W: int, ws: int, shift: int) -> Tensor:
    """(windows, ws^2, ws^2) f32: -100 where query and key of a window of the rolled H x W map lie in different regions
    (3 r_y + r_x, the rule of vt_win_token_region), 0 elsewhere"""
    region = 3 * _axis_regions(H, ws, shift).view(H, 1) + _axis_regions(W, ws, shift).view(1, W)
    per_token = window_partition(region.view(1, H, W, 1), ws)[0].squeeze(-1)  # (windows, ws^2)
    differ = per_token.unsqueeze(2) != per_token.unsqueeze(1)
    return torch.where(differ, -100.0, 0.0).to(torch.float32)


def relative_index(ws: int) -> Tensor:
    """(ws^2, ws^2) int64: vt_win_rel_index for query token (i_q, j_q) and key token (i_k, j_k) of a window"""
    t = torch.arange(ws * ws)
    i, j = t // ws, t % ws
    di, dj = i.view(-1, 1) - i.view(1, -1), j.view(-1, 1) - j.view(1, -1)
    return (di + ws - 1) * (2 * ws - 1) + (dj + ws - 1)


class WindowAttention(MHA):
    def __init__(
        self,
        input_size: int,
        d_model: int,
        n_heads: int,
        window_size: int = 7,
        shift: bool = False,
        bias: bool = True,
        dropout: float = 0.0,
    ) -> None:
        super().__init__(d_model, n_heads, bias, dropout)
        self.input_size = input_size
        self.window_size = window_size
        self.shift = window_size // 2 if shift else 0
        if self.shift > 0:
            self.register_buffer("attn_mask", shift_mask(input_size, input_size, window_size, self.shift), persistent=False)
        else:
            self.attn_mask = None
        self.relative_pe_table = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, n_heads, (2 * window_size - 1) ** 2), 0, 0.02))
        self.register_buffer("relative_pe_index", relative_index(window_size), persistent=False)

    def forward(self, x: Tensor) -> Tensor:  # (B, H, W, C); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a WindowAttention takes an NHWC map: on the GPU it runs as part of a SwinTransformer program")
        if tuple(x.shape[1:3]) != (self.input_size, self.input_size):
            raise ValueError(f"a {x.shape[1]}x{x.shape[2]} map: the attention was built for {self.input_size}x{self.input_size}")
        s, ws = self.shift, self.window_size
        bias = self.relative_pe_table[:, :, self.relative_pe_index]  # (1, heads, L, L)
        if s > 0:
            # (windows, heads, L, L), tiled over the batch: window b * windows + w of the partition takes mask w
            bias = (bias + self.attn_mask[:, None]).repeat(x.shape[0], 1, 1, 1)
            x = torch.roll(x, (-s, -s), (1, 2))
        tokens, nH, nW = window_partition(x, ws)
        out = window_unpartition(super().forward(tokens, attn_bias=bias), ws, nH, nW)
        return torch.roll(out, (s, s), (1, 2)) if s > 0 else out


class SwinBlock(ViTBlock):
    def __init__(
        self,
        input_size: int,
        d_model: int,
        n_heads: int,
        window_size: int = 7,
        shift: bool = False,
        mlp_ratio: float = 4.0,
        bias: bool = True,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = None,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-5,
    ) -> None:
        attention = partial(WindowAttention, input_size, d_model, n_heads, window_size=window_size, shift=shift, bias=bias,
                            dropout=dropout)
        super().__init__(d_model, n_heads, bias, mlp_ratio, dropout, layer_scale_init, stochastic_depth, norm_eps, attention)

    def forward(self, x: Tensor) -> Tensor:  # (B, H, W, d_model); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a SwinBlock takes an NHWC map: on the GPU it runs as part of a SwinTransformer program")
        x = x + self.mha(x)
        return x + self.mlp(x)

    def _vt_refusal(self) -> "str | None":
        mha = self.mha[1]
        if mha.window_size ** 2 > 64:
            return (f"window_size={mha.window_size}: a window of {mha.window_size ** 2} tokens does not fit the 64-row tile of "
                    "the window attention kernels (window_size <= 8; CPU tensors run)")
        if self.training and (mha.dropout > 0.0 or self.mlp[1].dropout.p > 0.0):
            return "dropout > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        if self.training and (self.mha[3].p > 0.0 or self.mlp[3].p > 0.0):
            return "stochastic_depth > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        d = mha.q_proj.in_features
        if d % mha.n_heads or d // mha.n_heads != 32:
            return (f"n_heads={mha.n_heads} over d_model={d} gives head_dim = {d / mha.n_heads:g}: the window attention kernels "
                    "implement head_dim 32")
        if any(lin.bias is None for lin in (mha.q_proj, mha.k_proj, mha.v_proj, mha.out_proj)):
            return "bias=False: the MI355X path implements the biased projections"
        return None

    def _vt_emit(self, b, x, name: str = "block"):
        """x: NHWC map [B, H, W, C]"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import ConvSpec

        mha, mlp, C = self.mha[1], self.mlp[1], x.C
        if (x.H, x.W) != (mha.input_size, mha.input_size):
            raise ValueError(f"{name}: a {x.H}x{x.W} map, the block was built for {mha.input_size}x{mha.input_size}")
        n = b.layer_norm(x, self.mha[0], name=name + ".mha.0")
        qkv = b.act(x.B, x.H, x.W, 3 * C, name + ".qkv")  # q | k | v: three channel slices of one buffer
        q, k, v = (b.conv_unit(n, ConvSpec.from_linear(lin), None, 0, out=qkv.sl(i * C, C), name=f"{name}.mha.1.{what}")
                   for i, (lin, what) in enumerate(((mha.q_proj, "q_proj"), (mha.k_proj, "k_proj"), (mha.v_proj, "v_proj"))))
        o = b.window_attention(q, k, v, mha.n_heads, mha.relative_pe_table, mha.window_size, mha.shift,
                               name=name + ".mha.1.attention")
        t = b.linear_unit(o, mha.out_proj, name=name + ".mha.1.out_proj")
        x = b.scale_residual(t, getattr(self.mha[2], "gamma", None), x, name=name + ".mha.add")
        n = b.layer_norm(x, self.mlp[0], name=name + ".mlp.0")
        h = b.linear_unit(n, mlp.linear1, act=4, name=name + ".mlp.1.linear1")
        t = b.linear_unit(h, mlp.linear2, name=name + ".mlp.1.linear2")
        return b.scale_residual(t, getattr(self.mlp[2], "gamma", None), x, name=name + ".mlp.add")


class PatchMerging(nn.Module):
    def __init__(self, d_model: int, norm_eps: float = 1e-5) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(d_model * 4, norm_eps)
        self.reduction = nn.Linear(d_model * 4, d_model * 2, False)

    def forward(self, x: Tensor) -> Tensor:  # the CPU path
        if x.is_cuda:
            raise NotImplementedError("a PatchMerging takes an NHWC map: on the GPU it runs as part of a SwinTransformer program")
        batch, height, width, chans = x.shape
        # 2x2 space to depth, channel order (dy, dx, c): the order of vt_patchify_fwd with p = 2
        cells = x.reshape(batch, height // 2, 2, width // 2, 2, chans).permute(0, 1, 3, 2, 4, 5)
        return self.reduction(self.norm(cells.reshape(batch, height // 2, width // 2, 4 * chans)))


class SwinTransformer(BaseBackbone):
    """shifted blocks tile their mask over the batch (the reference's broadcast raises at batch > 1)"""

    def __init__(
        self,
        img_size: int,
        d_model: int,
        n_heads: int,
        depths: "tuple[int, ...]",
        window_sizes: "tuple[int, ...]",
        patch_size: int = 4,
        mlp_ratio: float = 4.0,
        bias: bool = True,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = None,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-5,
    ) -> None:
        assert img_size % patch_size == 0
        assert d_model % n_heads == 0
        super().__init__()
        self.patch_embed = nn.Conv2d(3, d_model, patch_size, patch_size)
        self.patch_norm = nn.LayerNorm(d_model, norm_eps)
        self.dropout = nn.Dropout(dropout)
        self.img_size = int(img_size)

        self.stages = nn.Sequential()
        self.out_channels_list = tuple(d_model << si for si in range(len(depths)))
        self.stride = patch_size << (len(depths) - 1)
        for si, (depth, ws) in enumerate(zip(depths, window_sizes)):
            size, width, heads = (img_size // patch_size) >> si, d_model << si, n_heads << si
            stage = nn.Sequential(PatchMerging(width // 2, norm_eps) if si > 0 else nn.Identity())
            for bi in range(depth):
                # every second block is shifted, unless the map is a single window
                shifted = bi % 2 == 1 and size > ws
                stage.append(SwinBlock(size, width, heads, ws, shifted, mlp_ratio, bias, dropout, layer_scale_init,
                                       stochastic_depth, norm_eps))
            self.stages.append(stage)
        self.norm = nn.LayerNorm(self.out_channels_list[-1], norm_eps)

    # -- launch-list emission: [stage maps ..., head] -----------------------------------------------
    def _vt_refusal(self) -> "str | None":
        if self.training and self.dropout.p > 0.0:
            return "dropout > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        for m in self.modules():
            if isinstance(m, SwinBlock):
                why = m._vt_refusal()
                if why is not None:
                    return why
        return None

    def _vt_emit_maps(self, b, x):
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        if (x.H, x.W) != (self.img_size, self.img_size):
            raise ValueError(f"a {x.H}x{x.W} image: the model was built for {self.img_size}x{self.img_size}")
        o = b.layer_norm(b.patch_embed(x, self.patch_embed, name="patch_embed"), self.patch_norm, name="patch_norm")
        maps = []
        for si, stage in enumerate(self.stages):
            for bi, m in enumerate(stage):
                if isinstance(m, SwinBlock):
                    o = m._vt_emit(b, o, name=f"stages.{si}.{bi}")
                elif isinstance(m, PatchMerging):
                    o = b.patch_merging(o, m.norm, m.reduction, name=f"stages.{si}.0")
            maps.append(o)
        head = b.global_avgpool(b.layer_norm(o, self.norm, name="norm"), name="pool")
        return maps + [head]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        o = self.dropout(self.patch_norm(self.patch_embed(x).movedim(1, -1)))  # NHWC from here on
        maps = []
        for stage in self.stages:
            o = stage(o)
            maps.append(o)
        return maps + [self.norm(o).mean((1, 2))]

    def _vt_check(self, x: Tensor) -> None:
        if isinstance(x, Tensor) and x.is_cuda:
            why = self._vt_refusal()
            if why is not None:
                raise NotImplementedError(why)

    def get_feature_maps(self, x: Tensor) -> "list[Tensor]":
        self._vt_check(x)
        maps = self._vt_runner()(x, all_maps=True, compute_dtype=self.compute_dtype)[:-1]
        # the runner hands back logical-NCHW tensors with channels-last strides: (B, H, W, C) is a free view of each
        return [f.permute(0, 2, 3, 1) for f in maps] if x.is_cuda else maps

    def forward(self, x: Tensor) -> Tensor:
        self._vt_check(x)
        y = self._vt_runner()(x, all_maps=False, compute_dtype=self.compute_dtype)[-1]
        return y.flatten(1) if x.is_cuda else y  # (B, C, 1, 1) -> (B, C)

    def resize_pe(self, img_size: int) -> None:
        raise NotImplementedError()

    # d_model, n_heads, depths, window sizes: T / S / B / L of arXiv 2103.14030 table 7 (22k checkpoints of the Swin authors'
    # release page), S3-* the searched AutoFormerV2 models (window 14 in places: CPU tensors only)
    _W7 = (7, 7, 7, 7)
    _VARIANTS = {
        "T": (96, 3, (2, 2, 6, 2), _W7),
        "S": (96, 3, (2, 2, 18, 2), _W7),
        "B": (128, 4, (2, 2, 18, 2), _W7),
        "L": (192, 6, (2, 2, 18, 2), _W7),
        "S3-T": (96, 3, (2, 2, 6, 2), (7, 7, 14, 7)),
        "S3-S": (96, 3, (2, 2, 18, 2), (14, 14, 14, 14)),
        "S3-B": (96, 3, (2, 2, 30, 2), (7, 7, 14, 7)),
    }
    _SWIN_URL = "https://github.com/SwinTransformer/storage/releases/download/"
    _S3_URL = "https://github.com/silent-chen/AutoFormer-model-zoo/releases/download/v1.0/"
    _CKPTS = {
        "T": "v1.0.8/swin_tiny_patch4_window7_224_22k.pth",
        "S": "v1.0.8/swin_small_patch4_window7_224_22k.pth",
        "B": "v1.0.0/swin_base_patch4_window7_224_22k.pth",
        "L": "v1.0.0/swin_large_patch4_window7_224_22k.pth",
        "S3-T": "supernet-tiny.pth",
        "S3-S": "supernet-small.pth",
        "S3-B": "supernet-base.pth",
    }

    @staticmethod
    def ckpt_url(variant: str) -> str:
        base = SwinTransformer._S3_URL if variant.startswith("S3") else SwinTransformer._SWIN_URL
        return base + SwinTransformer._CKPTS[variant]

    @staticmethod
    def from_config(variant: str, img_size: int, pretrained: bool = False) -> "SwinTransformer":
        # the checkpoints are 224 x 224 models; any other size would need resize_pe, which is not implemented
        m = SwinTransformer(224 if pretrained else img_size, *SwinTransformer._VARIANTS[variant])
        if pretrained:
            m.load_official_ckpt(torch.hub.load_state_dict_from_url(SwinTransformer.ckpt_url(variant))["model"])
            if img_size != 224:
                m.resize_pe(img_size)
        return m

    def _official_keys(self) -> "list[tuple[str, str, str | None]]":
        """(key of this module's state_dict, key of a microsoft/Swin-Transformer checkpoint, transform) for every parameter.
        Transforms: None copies; "q" / "k" / "v" take that third of a fused qkv row block; "T" transposes the
        (2 ws - 1)^2 x heads table; "merge" reorders the four C-wide column groups of a merging tensor from the official
        (dx, dy, c) concatenation -- (0,0) (1,0) (0,1) (1,1) -- to this module's (dy, dx, c)."""
        rows = [("patch_embed", "patch_embed.proj", None), ("patch_norm", "patch_embed.norm", None), ("norm", "norm", None)]
        table = [(f"{d}.{p}", f"{s}.{p}", how) for d, s, how in rows for p in ("weight", "bias")]
        for si, stage in enumerate(self.stages):
            if si > 0:
                dst, src = f"stages.{si}.0.", f"layers.{si - 1}.downsample."
                table += [(dst + k, src + k, "merge") for k in ("norm.weight", "norm.bias", "reduction.weight")]
            for bi in range(1, len(stage)):
                dst, src = f"stages.{si}.{bi}.", f"layers.{si}.blocks.{bi - 1}."
                for p in ("weight", "bias"):
                    table += [(f"{dst}mha.1.{x}_proj.{p}", f"{src}attn.qkv.{p}", x) for x in "qkv"]
                    table += [(f"{dst}mha.0.{p}", f"{src}norm1.{p}", None), (f"{dst}mha.1.out_proj.{p}", f"{src}attn.proj.{p}", None),
                              (f"{dst}mlp.0.{p}", f"{src}norm2.{p}", None), (f"{dst}mlp.1.linear1.{p}", f"{src}mlp.fc1.{p}", None),
                              (f"{dst}mlp.1.linear2.{p}", f"{src}mlp.fc2.{p}", None)]
                table.append((dst + "mha.1.relative_pe_table", src + "attn.relative_position_bias_table", "T"))
        return table

    @torch.no_grad()
    def load_official_ckpt(self, state_dict: "dict[str, Tensor]") -> None:
        """copy a checkpoint in the microsoft/Swin-Transformer key layout into this module (the key table is
        `_official_keys`).  The checkpoint's `attn_mask` and `attn.relative_position_index` buffers must equal this module's
        own; every other key must be consumed, except the classifier head (`head.weight`, `head.bias`).  A missing key is a
        KeyError."""
        transforms = {
            None: lambda t: t,
            "q": lambda t: t[: t.shape[0] // 3],
            "k": lambda t: t[t.shape[0] // 3: 2 * t.shape[0] // 3],
            "v": lambda t: t[2 * t.shape[0] // 3:],
            "T": lambda t: t.T.unsqueeze(0),
            "merge": lambda t: t.unflatten(-1, (2, 2, -1)).transpose(-3, -2).flatten(-3),
        }
        own, used = self.state_dict(), set()
        for dst, src, how in self._official_keys():
            if src not in state_dict:
                raise KeyError(f"load_official_ckpt: {src} is missing")
            own[dst].copy_(transforms[how](state_dict[src]))
            used.add(src)
        for si, stage in enumerate(self.stages):
            for bi in range(1, len(stage)):
                attn, src = stage[bi].mha[1], f"layers.{si}.blocks.{bi - 1}."
                buffers = [(attn.relative_pe_index, src + "attn.relative_position_index")]
                if attn.attn_mask is not None:
                    buffers.append((attn.attn_mask, src + "attn_mask"))
                for mine, key in buffers:
                    if not torch.equal(mine.to(state_dict[key].dtype), state_dict[key]):
                        raise ValueError(f"load_official_ckpt: {key} differs from this module's buffer")
                    used.add(key)
        extra = sorted(set(state_dict) - used - {"head.weight", "head.bias"})
        if extra:
            raise KeyError(f"load_official_ckpt: unexpected keys {extra}")
