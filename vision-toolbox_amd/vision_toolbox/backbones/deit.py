"""DeiT (https://arxiv.org/abs/2012.12877) and DeiT III (https://arxiv.org/abs/2204.07118) on libvt_amd.

Constructor signatures and child names follow the reference (vision_toolbox/backbones/deit.py:14-118): both are a `ViT` with
class-token pooling.  `DeiT` adds the distillation token `dist_token` (1, 1, d), registered after everything ViT registers,
so the state_dict is ViT's keys plus `dist_token` at the end; `DeiT3` is ViT with LayerScale on by default (1e-6) and adds
nothing.

DeiT's forward.  The tokens are [cls | dist | patch_embed + pe] (L = T + 2; neither learned row gets a position), the ViT
blocks follow, and the result is `norm(out[:, :2]).mean(1)`: LayerNorm over the first two rows of every image, then their
mean, (B, d_model).  On the GPU path the two ends are one launch each -- vt_prefix_tokens_fwd in front of the blocks and
vt_prefix_pool_fwd behind them (vt_prefix_tokens.hip) -- in place of ViT's vt_vit_tokens_fwd and vt_token_select_fwd +
vt_layernorm_fwd; the blocks are ViT's, launch for launch.  DeiT3 needs no kernel of its own: its launch list is the one
`ViT(..., layer_scale_init=...)` emits.

Refusals are ViT's, with the same messages (dropout / stochastic depth in training mode, a head_dim other than 32 or 64 --
so the H variants --, `bias=False`, an image whose patch count differs from `pe`), and `resize_pe` is inherited: the prefix
tokens have no position, so nothing else changes.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .vit import ViT

__all__ = ["DeiT", "DeiT3"]


def _from_config(cls, variant: str, img_size: int, pretrained: bool):
    size, patch = variant.split("_")
    d_model, depth, n_heads = ViT._VARIANTS[size]
    if pretrained:
        raise NotImplementedError("pretrained=True: this build downloads nothing; pass the official state_dict to "
                                  "load_official_ckpt")
    return cls(d_model, depth, n_heads, int(patch), img_size)


class DeiT(ViT):
    """`cls_token` and `dist_token` are BROADCAST over the batch on both paths: the reference joins its (1, 1, d) parameters to
    the (N, T, d) patch tokens with torch.cat, which raises at batch > 1; the broadcast is identical at batch 1 and the evident
    intent beyond it (as in `ViT` and `CaiT`)."""

    def __init__(
        self,
        d_model: int,
        depth: int,
        n_heads: int,
        patch_size: int,
        img_size: int,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = None,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__(d_model, depth, n_heads, patch_size, img_size, True, "cls_token", bias, mlp_ratio, dropout,
                         layer_scale_init, stochastic_depth, norm_eps)
        self.dist_token = nn.Parameter(torch.zeros(1, 1, d_model))

    def _vt_emit_tokens(self, b, e):
        return b.prefix_tokens(e, self.pe, [self.cls_token, self.dist_token], name="tokens")

    def _vt_emit_pool(self, b, o):
        return b.prefix_pool(o, self.norm, 2, name="pool")

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        out = self.patch_embed(x).flatten(2).transpose(1, 2) + self.pe  # (B, C, gh, gw) -> (B, tokens, C)
        n = out.shape[0]
        out = torch.cat([self.cls_token.expand(n, -1, -1), self.dist_token.expand(n, -1, -1), out], 1)
        out = self.layers(out)
        return [self.norm(out[:, :2]).mean(1)]

    @staticmethod
    def from_config(variant: str, img_size: int, pretrained: bool = False) -> "DeiT":
        """`variant` is "<size>_<patch>", e.g. "S_16" (the Ti / S / M / B / L / H table of ViT).  Nothing is fetched:
        `pretrained=True` raises; load a downloaded official state_dict with `load_official_ckpt`."""
        return _from_config(DeiT, variant, img_size, pretrained)

    @torch.no_grad()
    def load_official_ckpt(self, state_dict: "dict[str, Tensor]") -> None:
        """copy a state_dict in the layout of the official DeiT repository (`patch_embed.proj`, `pos_embed`, `cls_token`,
        `dist_token`, `blocks.i.{norm1, attn.qkv, attn.proj, gamma_1, norm2, mlp.fc1, mlp.fc2, gamma_2}`, `norm`) into this
        model.  The fused qkv rows are split in thirds.  The last `pe.shape[1]` rows of `pos_embed` go to `pe`; where
        `pos_embed` is longer than that (DeiT: it is not for DeiT III) its row 0 is folded into `cls_token`; with a
        `dist_token` row 1 is folded into it and `head_dist.*` is dropped.  What may remain is the classifier head
        (`head.weight`, `head.bias`); anything else left over, and any array the model needs and the dict lacks, raises
        KeyError."""
        left = dict(state_dict)

        def take(dst: Tensor, key: str) -> None:
            dst.copy_(left.pop(key).reshape(dst.shape))

        def take_wb(m: nn.Module, prefix: str) -> None:
            take(m.weight, prefix + ".weight")
            take(m.bias, prefix + ".bias")

        take_wb(self.patch_embed, "patch_embed.proj")
        pos = left.pop("pos_embed")
        T = self.pe.shape[1]
        self.pe.copy_(pos[:, -T:])
        take(self.cls_token, "cls_token")
        if pos.shape[1] > T:
            self.cls_token.add_(pos[:, 0])
        if hasattr(self, "dist_token"):
            take(self.dist_token, "dist_token")
            self.dist_token.add_(pos[:, 1])
            left.pop("head_dist.weight")
            left.pop("head_dist.bias")
        for i, blk in enumerate(self.layers):
            prefix, mha = f"blocks.{i}.", blk.mha[1]
            take_wb(blk.mha[0], prefix + "norm1")
            for what in ("weight", "bias"):
                thirds = left.pop(f"{prefix}attn.qkv.{what}").chunk(3, 0)
                for proj, part in zip((mha.q_proj, mha.k_proj, mha.v_proj), thirds):
                    getattr(proj, what).copy_(part)
            take_wb(mha.out_proj, prefix + "attn.proj")
            take_wb(blk.mlp[0], prefix + "norm2")
            take_wb(blk.mlp[1].linear1, prefix + "mlp.fc1")
            take_wb(blk.mlp[1].linear2, prefix + "mlp.fc2")
            for seq, key in ((blk.mha, "gamma_1"), (blk.mlp, "gamma_2")):
                if hasattr(seq[2], "gamma"):
                    take(seq[2].gamma, prefix + key)
        take_wb(self.norm, "norm")
        extra = sorted(k for k in left if k not in ("head.weight", "head.bias"))
        if extra:
            raise KeyError(f"load_official_ckpt: unexpected keys {extra}")


class DeiT3(ViT):
    """a `ViT` with class-token pooling and LayerScale (1e-6) by default; the class token is broadcast over the batch as in
    `ViT`.  `cls_token=False` raises ViT's ValueError: class-token pooling needs the token."""

    def __init__(
        self,
        d_model: int,
        depth: int,
        n_heads: int,
        patch_size: int,
        img_size: int,
        cls_token: bool = True,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__(d_model, depth, n_heads, patch_size, img_size, cls_token, "cls_token", bias, mlp_ratio, dropout,
                         layer_scale_init, stochastic_depth, norm_eps)

    @staticmethod
    def from_config(variant: str, img_size: int, pretrained: bool = False) -> "DeiT3":
        """as `DeiT.from_config`"""
        return _from_config(DeiT3, variant, img_size, pretrained)

    load_official_ckpt = DeiT.load_official_ckpt
