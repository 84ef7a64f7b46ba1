"""CaiT, "Going deeper with Image Transformers" (https://arxiv.org/abs/2103.17239) on libvt_amd.

Constructor signatures, child names and child indices follow the reference (vision_toolbox/backbones/cait.py:16-143), so
state_dict keys are the reference's: `patch_embed`, `cls_token`, `pe`, `sa_layers.i.mha.0` (LayerNorm), `sa_layers.i.mha.1`
(`q_proj`, `k_proj`, `v_proj`, `out_proj`, `talking_head_proj.0`, `talking_head_proj.2`), `sa_layers.i.mha.2.gamma`,
`sa_layers.i.mlp.*`, `ca_layers.i.*` (the same without the talking-head maps) and `norm`.

Two stages.  The self-attention stage runs the patch tokens alone through `CaiTSABlock`s whose attention is TALKING-HEADS
attention: the scores of all heads are mixed by a learned n_heads x n_heads map in front of the softmax and by a second one
behind it.  The class-attention stage then lets the class token alone attend over [class token | patch tokens]
(`CaiTCABlock`): one query row per image, the patch tokens are read and never updated.

The class token.  The reference joins its (1, 1, d) parameter to the (N, L, d) patch tokens with torch.cat, which raises at
batch > 1.  As in vit.py this class BROADCASTS the token over the batch on both paths -- identical at batch 1.

The launch lists keep one layout, the token map [B, 1, L, C].  In front: vt_patchify_fwd + one vt_conv_igemm (the patch
embedding) and vt_vit_tokens_fwd (`+ pe`, no class row).  Per SA block the twelve launches of a ViT block with
vt_talk_attn_fwd in place of vt_attn_fwd.  Per CA block:

    vt_token_prepend_fwd     [class row | patch tokens] -> [B, 1, 1 + L, C]
    vt_token_select_fwd      row 0 of it: the class row as the shortcut of the block
    vt_layernorm_fwd         mha.0 on 1 + L rows
    vt_token_select_fwd      row 0 of the normalised map, then vt_conv_igemm: q_proj on B rows
    vt_conv_igemm x 2        k_proj, v_proj into the two channel slices of one [B, 1, 1 + L, 2 C] buffer
    vt_cls_attn_fwd          one query per (image, head) over 1 + L keys
    vt_conv_igemm            out_proj, then vt_scale_residual_fwd onto the class row
    the MLP half of a ViT block on B rows

and vt_layernorm_fwd on B rows behind the last one.  The patch map has `ca_depth` consumers; its gradient accumulates.
`forward(imgs)` returns (B, d_model).

Refused on CUDA tensors (all of them construct and run on CPU tensors): `dropout > 0` or `stochastic_depth > 0` in training
mode, `bias=False`, a `head_dim` other than 48, `n_heads > 16`, `ca_depth = 0` (NotImplementedError); an image whose patch
count differs from `pe` (ValueError).  A `d_model` that is no multiple of a 16-byte chunk needs no refusal of its own: head_dim
48 makes d_model = 48 n_heads a multiple of 8, and anything else is refused by name of its head_dim.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from ..components import HipModule
from .vit import MHA, ViT, ViTBlock

__all__ = ["ClassAttention", "TalkingHeadAttention", "CaiTCABlock", "CaiTSABlock", "CaiT"]


class ClassAttention(MHA):
    """attention pooling: the query is row 0 of x alone"""

    def forward(self, x: Tensor) -> Tensor:  # (B, 1 + L, d_model) -> (B, d_model); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a ClassAttention takes a token map: on the GPU it runs as part of a CaiT program")
        q = self.q_proj(x[:, 0]).unflatten(-1, (self.n_heads, -1)).unsqueeze(2)  # (B, n_heads, 1, head_dim)
        k = self.k_proj(x).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)  # (B, n_heads, 1 + L, head_dim)
        v = self.v_proj(x).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)
        out = F.scaled_dot_product_attention(q, k, v, None, self.dropout if self.training else 0.0)
        return self.out_proj(out.flatten(1))


class TalkingHeadAttention(MHA):
    """the heads' scores are mixed by a 1x1 convolution over the head axis in front of the softmax and behind it; the
    (B, n_heads, L, L) scores are materialised on the CPU path"""

    def __init__(self, d_model: int, n_heads: int, bias: bool = True, dropout: float = 0.0) -> None:
        super().__init__(d_model, n_heads, bias, dropout)
        self.talking_head_proj = nn.Sequential(
            nn.Conv2d(n_heads, n_heads, 1),
            nn.Softmax(-1),
            nn.Conv2d(n_heads, n_heads, 1),
            nn.Dropout(dropout),
        )

    def forward(self, x: Tensor) -> Tensor:  # the CPU path
        if x.is_cuda:
            raise NotImplementedError("a TalkingHeadAttention takes a token map: on the GPU it runs as part of a CaiT program")
        q = self.q_proj(x).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)  # (B, n_heads, L, head_dim)
        k = self.k_proj(x).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)
        v = self.v_proj(x).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)
        attn = q @ (k * self.scale).transpose(-1, -2)
        out = self.talking_head_proj(attn) @ v
        return self.out_proj(out.transpose(-2, -3).flatten(-2))


def _block_refusal(blk: ViTBlock) -> "str | None":
    """what keeps a CaiT block off the MI355X path (None: nothing)"""
    mha = blk.mha[1]
    if blk.training and (mha.dropout > 0.0 or blk.mlp[1].dropout.p > 0.0):
        return "dropout > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
    if blk.training and (blk.mha[3].p > 0.0 or blk.mlp[3].p > 0.0):
        return "stochastic_depth > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
    d = mha.q_proj.in_features
    if d % mha.n_heads or d // mha.n_heads != 48:
        return (f"n_heads={mha.n_heads} over d_model={d} gives head_dim = {d / mha.n_heads:g}: the CaiT attention kernels "
                "implement head_dim 48")
    if mha.n_heads > 16:
        return f"n_heads={mha.n_heads}: the talking-heads kernels hold at most 16 heads"
    if any(lin.bias is None for lin in (mha.q_proj, mha.k_proj, mha.v_proj, mha.out_proj)):
        return "bias=False: the MI355X path implements the biased projections"
    return None


def _emit_mlp_half(blk: ViTBlock, b, x, name: str):
    mlp = blk.mlp[1]
    n = b.layer_norm(x, blk.mlp[0], name=name + ".mlp.0")
    h = b.linear_unit(n, mlp.linear1, act=4, name=name + ".mlp.1.linear1")
    t = b.linear_unit(h, mlp.linear2, name=name + ".mlp.1.linear2")
    return b.scale_residual(t, getattr(blk.mlp[2], "gamma", None), x, name=name + ".mlp.add")


class CaiTCABlock(ViTBlock):
    def __init__(
        self,
        d_model: int,
        n_heads: int,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__(d_model, n_heads, bias, mlp_ratio, dropout, layer_scale_init, stochastic_depth, norm_eps,
                         partial(ClassAttention, d_model, n_heads, bias, dropout))

    def forward(self, x: Tensor, cls_token: Tensor) -> Tensor:  # (B, L, d), (B | 1, 1, d) -> (B, 1, d); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a CaiTCABlock takes a token map: on the GPU it runs as part of a CaiT program")
        cls_token = cls_token.expand(x.shape[0], -1, -1)
        cls_token = cls_token + self.mha(torch.cat((cls_token, x), 1)).unsqueeze(1)
        return cls_token + self.mlp(cls_token)

    def _vt_refusal(self) -> "str | None":
        return _block_refusal(self)

    def _vt_emit(self, b, x, cls, name: str = "block"):
        """x: the patch tokens [B, 1, L, C]; cls: the class row, the parameter or a [B, 1, 1, C] activation"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import ConvSpec

        mha, C = self.mha[1], x.C
        cat = b.token_prepend(x, cls, name=name + ".cat")
        c0 = b.token_select(cat, 0, name=name + ".cls")  # the shortcut
        n = b.layer_norm(cat, self.mha[0], name=name + ".mha.0")
        n0 = b.token_select(n, 0, name=name + ".mha.1.query")
        q = b.linear_unit(n0, mha.q_proj, name=name + ".mha.1.q_proj")
        kv = b.act(x.B, 1, n.W, 2 * C, name + ".kv")  # k | v: two channel slices of one buffer
        k, v = (b.conv_unit(n, ConvSpec.from_linear(lin), None, 0, out=kv.sl(i * C, C), name=f"{name}.mha.1.{what}")
                for i, (lin, what) in enumerate(((mha.k_proj, "k_proj"), (mha.v_proj, "v_proj"))))
        o = b.class_attention(q, k, v, mha.n_heads, name=name + ".mha.1.attention")
        t = b.linear_unit(o, mha.out_proj, name=name + ".mha.1.out_proj")
        c = b.scale_residual(t, getattr(self.mha[2], "gamma", None), c0, name=name + ".mha.add")
        return _emit_mlp_half(self, b, c, name)


class CaiTSABlock(ViTBlock):
    def __init__(
        self,
        d_model: int,
        n_heads: int,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__(d_model, n_heads, bias, mlp_ratio, dropout, layer_scale_init, stochastic_depth, norm_eps,
                         partial(TalkingHeadAttention, d_model, n_heads, bias, dropout))

    def _vt_refusal(self) -> "str | None":
        return _block_refusal(self)

    def _vt_emit(self, b, x, name: str = "block"):
        """x: token map [B, 1, L, C]"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import ConvSpec

        mha, C = self.mha[1], x.C
        n = b.layer_norm(x, self.mha[0], name=name + ".mha.0")
        qkv = b.act(x.B, 1, x.W, 3 * C, name + ".qkv")  # q | k | v: three channel slices of one buffer
        q, k, v = (b.conv_unit(n, ConvSpec.from_linear(lin), None, 0, out=qkv.sl(i * C, C), name=f"{name}.mha.1.{what}")
                   for i, (lin, what) in enumerate(((mha.q_proj, "q_proj"), (mha.k_proj, "k_proj"), (mha.v_proj, "v_proj"))))
        o = b.talking_attention(q, k, v, mha.n_heads, mha.talking_head_proj[0], mha.talking_head_proj[2],
                                name=name + ".mha.1.attention")
        t = b.linear_unit(o, mha.out_proj, name=name + ".mha.1.out_proj")
        x = b.scale_residual(t, getattr(self.mha[2], "gamma", None), x, name=name + ".mha.add")
        return _emit_mlp_half(self, b, x, name)


class CaiT(HipModule):
    """the class token is broadcast over the batch (the reference's torch.cat raises at batch > 1)"""

    def __init__(
        self,
        d_model: int,
        sa_depth: int,
        ca_depth: int,
        n_heads: int,
        patch_size: int,
        img_size: int,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = 1e-6,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        if img_size % patch_size:
            raise ValueError(f"img_size={img_size} is no multiple of patch_size={patch_size}")
        super().__init__()
        self.patch_embed = nn.Conv2d(3, d_model, patch_size, patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d_model))
        self.pe = nn.Parameter(torch.empty(1, (img_size // patch_size) ** 2, d_model))
        nn.init.normal_(self.pe, 0, 0.02)
        args = (d_model, n_heads, bias, mlp_ratio, dropout, layer_scale_init, stochastic_depth, norm_eps)
        self.sa_layers = nn.Sequential()
        for _ in range(sa_depth):
            self.sa_layers.append(CaiTSABlock(*args))
        self.ca_layers = nn.ModuleList()
        for _ in range(ca_depth):
            self.ca_layers.append(CaiTCABlock(*args))
        self.norm = nn.LayerNorm(d_model, norm_eps)
        self.patch_size, self.d_model = int(patch_size), int(d_model)

    def get_last_out_channels(self) -> int:
        return self.d_model

    # -- launch-list emission ---------------------------------------------------------------------
    def _vt_refusal(self) -> "str | None":
        if len(self.ca_layers) == 0:
            return "ca_depth=0: the MI355X path ends in a class-attention block (CPU tensors run)"
        for m in (*self.sa_layers, *self.ca_layers):
            why = m._vt_refusal()
            if why is not None:
                return why
        return None

    _check_patches = ViT._check_patches

    def _vt_emit_maps(self, b, x):
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        self._check_patches(x.H, x.W)
        e = b.patch_embed(x, self.patch_embed, name="patch_embed")
        o = b.vit_tokens(e, self.pe, None, name="tokens")
        for i, blk in enumerate(self.sa_layers):
            o = blk._vt_emit(b, o, name=f"sa_layers.{i}")
        cls = self.cls_token
        for i, blk in enumerate(self.ca_layers):
            cls = blk._vt_emit(b, o, cls, name=f"ca_layers.{i}")
        return [b.layer_norm(cls, self.norm, name="norm")]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        patches = self.patch_embed(x).flatten(2).transpose(1, 2) + self.pe  # (B, C, gh, gw) -> (B, tokens, C)
        patches = self.sa_layers(patches)
        cls_token = self.cls_token.expand(patches.shape[0], -1, -1)
        for blk in self.ca_layers:
            cls_token = blk(patches, cls_token)
        return [self.norm(cls_token.squeeze(1))]

    def forward(self, imgs: Tensor) -> Tensor:
        if isinstance(imgs, Tensor) and imgs.is_cuda:
            why = self._vt_refusal()
            if why is not None:
                raise NotImplementedError(why)
            if imgs.dim() == 4:
                self._check_patches(imgs.shape[2], imgs.shape[3])
        y = self._vt_runner()(imgs, all_maps=False, compute_dtype=self.compute_dtype)[-1]
        return y.flatten(1) if imgs.is_cuda else y  # (B, C, 1, 1) -> (B, C)

    @torch.no_grad()
    def resize_pe(self, size: int, interpolation_mode: str = "bicubic") -> None:
        """interpolate the position embedding to a `size` x `size` image; see ViT.resize_pe"""
        ViT.resize_pe(self, size, interpolation_mode)

    # -- configurations and the official checkpoints ----------------------------------------------
    _WIDTHS = {"xxs": 192, "xs": 288, "s": 384, "m": 768}

    @staticmethod
    def from_config(variant: str, img_size: int, pretrained: bool = False) -> "CaiT":
        """`variant` is "<width>_<sa_depth>", e.g. "xxs_24": d_model 192 / 288 / 384 / 768, two class-attention blocks,
        head_dim 48, 16 x 16 patches.  Nothing is fetched: `pretrained=True` raises; load a downloaded official
        state_dict with `load_official_ckpt`."""
        width, sa_depth = variant.split("_")
        d_model = CaiT._WIDTHS[width]
        if pretrained:
            raise NotImplementedError("pretrained=True: this build downloads nothing; pass the official state_dict to "
                                      "load_official_ckpt")
        return CaiT(d_model, int(sa_depth), 2, d_model // 48, 16, img_size)

    @torch.no_grad()
    def load_official_ckpt(self, state_dict: "dict[str, Tensor]") -> None:
        """copy a state_dict in the layout of the official DeiT repository (`patch_embed.proj`, `cls_token`, `pos_embed`,
        `blocks.i.{norm1, attn.qkv, attn.proj, attn.proj_l, attn.proj_w, gamma_1, norm2, mlp.fc1, mlp.fc2, gamma_2}`,
        `blocks_token_only.i.{norm1, attn.q, attn.k, attn.v, attn.proj, ...}`, `norm`) into this model.  The fused qkv rows
        are split in thirds; `proj_l` / `proj_w` are Linear(n_heads, n_heads) there and 1x1 convolutions here.  What may remain
        is the classifier head (`head.weight`, `head.bias`); anything else left over, and any array the model needs and
        the dict lacks, raises KeyError."""
        left = dict(state_dict)

        def take(dst: Tensor, key: str) -> None:
            dst.copy_(left.pop(key).reshape(dst.shape))

        def take_wb(m: nn.Module, prefix: str) -> None:
            take(m.weight, prefix + ".weight")
            take(m.bias, prefix + ".bias")

        def take_common(blk: ViTBlock, prefix: str) -> None:
            take_wb(blk.mha[0], prefix + "norm1")
            take_wb(blk.mha[1].out_proj, prefix + "attn.proj")
            take_wb(blk.mlp[0], prefix + "norm2")
            take_wb(blk.mlp[1].linear1, prefix + "mlp.fc1")
            take_wb(blk.mlp[1].linear2, prefix + "mlp.fc2")
            for seq, key in ((blk.mha, "gamma_1"), (blk.mlp, "gamma_2")):
                if hasattr(seq[2], "gamma"):
                    take(seq[2].gamma, prefix + key)

        take_wb(self.patch_embed, "patch_embed.proj")
        take(self.cls_token, "cls_token")
        take(self.pe, "pos_embed")
        for i, blk in enumerate(self.sa_layers):
            prefix, mha = f"blocks.{i}.", blk.mha[1]
            take_common(blk, prefix)
            for what in ("weight", "bias"):
                thirds = left.pop(f"{prefix}attn.qkv.{what}").chunk(3, 0)
                for proj, part in zip((mha.q_proj, mha.k_proj, mha.v_proj), thirds):
                    getattr(proj, what).copy_(part)
            take_wb(mha.talking_head_proj[0], prefix + "attn.proj_l")
            take_wb(mha.talking_head_proj[2], prefix + "attn.proj_w")
        for i, blk in enumerate(self.ca_layers):
            prefix, mha = f"blocks_token_only.{i}.", blk.mha[1]
            take_common(blk, prefix)
            take_wb(mha.q_proj, prefix + "attn.q")
            take_wb(mha.k_proj, prefix + "attn.k")
            take_wb(mha.v_proj, prefix + "attn.v")
        take_wb(self.norm, "norm")
        extra = sorted(k for k in left if k not in ("head.weight", "head.bias"))
        if extra:
            raise KeyError(f"load_official_ckpt: unexpected keys {extra}")
