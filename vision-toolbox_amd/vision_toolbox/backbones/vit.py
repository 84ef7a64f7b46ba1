"""Vision Transformer (https://arxiv.org/abs/2010.11929, https://arxiv.org/abs/2106.10270) on libvt_amd.

Constructor signatures, child names and child indices follow the reference (vision_toolbox/backbones/vit.py:18-157), so
state_dict keys are the reference's: `cls_token`, `pe`, `patch_embed`, `layers.i.mha.0` (LayerNorm), `layers.i.mha.1`
(`q_proj`, `k_proj`, `v_proj`, `out_proj`), `layers.i.mha.2.gamma` (LayerScale, where there is one), `layers.i.mlp.0`,
`layers.i.mlp.1.linear1|linear2`, `layers.i.mlp.2.gamma`, `norm`, and `pooler.*` with pool_type="mha".  `MLP` is the one of
mlp_mixer.py (the reference defines it here and the Mixer imports it).

The class token.  The reference joins its (1, 1, d) parameter to the (N, L, d) patch tokens with torch.cat, which raises at
batch > 1; its own tests use batch 1.  This class BROADCASTS the token over the batch -- identical at batch 1, and the evident
intent at batch > 1 -- on both paths.

The launch lists keep one layout, the token map [B, 1, L, C] (tokens along W).  Heads are channel slices, q / k / v are three
channel slices of one [B, 1, L, 3 C] buffer, and nothing is transposed.  Per block:

    vt_layernorm_fwd         mha.0
    vt_conv_igemm x 3        q_proj, k_proj, v_proj + bias as 1x1 convs into the slices of the qkv buffer
    vt_attn_fwd              softmax(q k^T / sqrt(head_dim)) v per (image, head), writes the row log-sum-exp
    vt_conv_igemm            out_proj + bias
    vt_scale_residual_fwd    shortcut + gamma * branch (gamma None: the plain add)
    vt_layernorm_fwd         mlp.0
    vt_conv_igemm            linear1 + bias, then vt_bn_act_apply: exact GELU
    vt_conv_igemm            linear2 + bias
    vt_scale_residual_fwd

in front of them vt_patchify_fwd + one vt_conv_igemm (the patch embedding) and vt_vit_tokens_fwd (`+ pe`, the class token);
behind them pool_type "cls_token": vt_token_select_fwd then vt_layernorm_fwd on B rows; "gap": vt_layernorm_fwd then the mean
over the tokens.  `forward(imgs)` returns (B, d_model).  The token count on the GPU path comes from `pe.shape[1]`, so
`resize_pe` retargets the model to another image size.

Refused on CUDA tensors (all of them construct and run on CPU tensors): `dropout > 0` or `stochastic_depth > 0` in training
mode, `pool_type="mha"` (the single-query cross-attention pooler has no kernel), a `head_dim` other than 32 or 64, a
`d_model` that is no multiple of a 16-byte chunk of the compute dtype (NotImplementedError); an image whose patch count
differs from `pe` (ValueError).
"""
from __future__ import annotations

import os
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

from ..components import _RUNNERS, HipModule, LayerScale, StochasticDepth
from .mlp_mixer import MLP

__all__ = ["MHA", "ViTBlock", "MHAPooling", "ViT"]


class MHA(nn.Module):
    def __init__(self, d_model: int, n_heads: int, bias: bool = True, dropout: float = 0.0) -> None:
        super().__init__()
        self.q_proj = nn.Linear(d_model, d_model, bias)
        self.k_proj = nn.Linear(d_model, d_model, bias)
        self.v_proj = nn.Linear(d_model, d_model, bias)
        self.out_proj = nn.Linear(d_model, d_model, bias)
        self.n_heads = n_heads
        self.dropout = dropout
        self.scale = (d_model // n_heads) ** (-0.5)

    def forward(self, q: Tensor, k: "Tensor | None" = None, v: "Tensor | None" = None, *,
                attn_bias: "Tensor | None" = None) -> Tensor:  # the CPU path
        if q.is_cuda:
            raise NotImplementedError("an MHA takes a token map: on the GPU it runs as part of a ViT program")
        k = q if k is None else k
        v = k if v is None else v
        q = self.q_proj(q).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)  # (B, n_heads, L, head_dim)
        k = self.k_proj(k).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)
        v = self.v_proj(v).unflatten(-1, (self.n_heads, -1)).transpose(-2, -3)
        out = F.scaled_dot_product_attention(q, k, v, attn_bias, self.dropout if self.training else 0.0)
        return self.out_proj(out.transpose(-2, -3).flatten(-2))


class ViTBlock(nn.Module):
    def __init__(
        self,
        d_model: int,
        n_heads: int,
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = None,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
        attention: "type[nn.Module] | None" = None,
    ) -> None:
        if attention is None:
            attention = partial(MHA, d_model, n_heads, bias, dropout)
        super().__init__()
        self.mha = nn.Sequential(
            nn.LayerNorm(d_model, norm_eps),
            attention(),
            LayerScale(d_model, layer_scale_init) if layer_scale_init is not None else nn.Identity(),
            StochasticDepth(stochastic_depth),
        )
        self.mlp = nn.Sequential(
            nn.LayerNorm(d_model, norm_eps),
            MLP(d_model, int(d_model * mlp_ratio), dropout),
            LayerScale(d_model, layer_scale_init) if layer_scale_init is not None else nn.Identity(),
            StochasticDepth(stochastic_depth),
        )

    def forward(self, x: Tensor) -> Tensor:  # (B, L, d_model); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a ViTBlock takes a token map: on the GPU it runs as part of a ViT program")
        x = x + self.mha(x)
        return x + self.mlp(x)

    def _vt_refusal(self) -> "str | None":
        mha = self.mha[1]
        if not isinstance(mha, MHA):
            return f"attention={type(mha).__name__}: the MI355X path implements MHA"
        if self.training and (mha.dropout > 0.0 or self.mlp[1].dropout.p > 0.0):
            return "dropout > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        if self.training and (self.mha[3].p > 0.0 or self.mlp[3].p > 0.0):
            return "stochastic_depth > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        d = mha.q_proj.in_features
        if d % mha.n_heads or d // mha.n_heads not in (32, 64):
            return (f"n_heads={mha.n_heads} over d_model={d} gives head_dim = {d / mha.n_heads:g}: the attention kernels "
                    "implement head_dim 32 and 64")
        if any(lin.bias is None for lin in (mha.q_proj, mha.k_proj, mha.v_proj, mha.out_proj)):
            return "bias=False: the MI355X path implements the biased projections"
        return None

    def _vt_emit(self, b, x, name: str = "block"):
        """x: token map [B, 1, L, C]"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        from ..engine import ConvSpec

        mha, mlp, C = self.mha[1], self.mlp[1], x.C
        n = b.layer_norm(x, self.mha[0], name=name + ".mha.0")
        qkv = b.act(x.B, 1, x.W, 3 * C, name + ".qkv")  # q | k | v: three channel slices of one buffer
        q, k, v = (b.conv_unit(n, ConvSpec.from_linear(lin), None, 0, out=qkv.sl(i * C, C), name=f"{name}.mha.1.{what}")
                   for i, (lin, what) in enumerate(((mha.q_proj, "q_proj"), (mha.k_proj, "k_proj"), (mha.v_proj, "v_proj"))))
        o = b.attention(q, k, v, mha.n_heads, name=name + ".mha.1.attention")
        t = b.linear_unit(o, mha.out_proj, name=name + ".mha.1.out_proj")
        x = b.scale_residual(t, getattr(self.mha[2], "gamma", None), x, name=name + ".mha.add")
        n = b.layer_norm(x, self.mlp[0], name=name + ".mlp.0")
        h = b.linear_unit(n, mlp.linear1, act=4, name=name + ".mlp.1.linear1")
        t = b.linear_unit(h, mlp.linear2, name=name + ".mlp.1.linear2")
        return b.scale_residual(t, getattr(self.mlp[2], "gamma", None), x, name=name + ".mlp.add")


class MHAPooling(nn.Module):
    """a learned probe attends over the tokens (single-query cross-attention), then an MLP with a shortcut; CPU path only"""

    def __init__(self, d_model: int, n_heads: int, bias: bool = True, mlp_ratio: float = 4.0, norm_eps: float = 1e-6) -> None:
        super().__init__()
        self.probe = nn.Parameter(torch.zeros(1, 1, d_model))
        self.mha = MHA(d_model, n_heads, bias)
        self.norm = nn.LayerNorm(d_model, norm_eps)
        self.mlp = MLP(d_model, int(d_model * mlp_ratio))

    def forward(self, x: Tensor) -> Tensor:
        x = self.mha(self.probe.expand(x.shape[0], -1, -1), x).squeeze(1)
        return x + self.mlp(self.norm(x))


def _flax_take(dst: Tensor, weights: dict, key: str, fn=None) -> None:
    v = torch.from_numpy(np.asarray(weights.pop(key)))
    dst.copy_(fn(v) if fn is not None else v)


def _flax_ln(norm: nn.LayerNorm, w: dict, prefix: str) -> None:
    _flax_take(norm.weight, w, f"{prefix}/scale")
    _flax_take(norm.bias, w, f"{prefix}/bias")


def _flax_linear(linear: nn.Linear, w: dict, prefix: str) -> None:
    _flax_take(linear.weight, w, f"{prefix}/kernel", lambda v: v.T)
    _flax_take(linear.bias, w, f"{prefix}/bias")


def _flax_mha(mha: MHA, w: dict, prefix: str) -> None:
    """Flax keeps the projections per head: query / key / value kernels [d][heads][head_dim], out [heads][head_dim][d]"""
    for proj, what in ((mha.q_proj, "query"), (mha.k_proj, "key"), (mha.v_proj, "value")):
        _flax_take(proj.weight, w, f"{prefix}/{what}/kernel", lambda v: v.flatten(1).T)
        _flax_take(proj.bias, w, f"{prefix}/{what}/bias", lambda v: v.flatten())
    _flax_take(mha.out_proj.weight, w, f"{prefix}/out/kernel", lambda v: v.flatten(0, 1).T)
    _flax_take(mha.out_proj.bias, w, f"{prefix}/out/bias", lambda v: v.flatten())


class ViT(HipModule):
    """`cls_token=True` broadcasts the class token over the batch (the reference's torch.cat raises at batch > 1)."""

    def __init__(
        self,
        d_model: int,
        depth: int,
        n_heads: int,
        patch_size: int,
        img_size: int,
        cls_token: bool = True,
        pool_type: str = "cls_token",
        bias: bool = True,
        mlp_ratio: float = 4.0,
        dropout: float = 0.0,
        layer_scale_init: "float | None" = None,
        stochastic_depth: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        if img_size % patch_size:
            raise ValueError(f"img_size={img_size} is no multiple of patch_size={patch_size}")
        if pool_type not in ("cls_token", "gap", "mha"):
            raise ValueError(f"pool_type={pool_type!r}: cls_token, gap or mha")
        if pool_type == "cls_token" and not cls_token:
            raise ValueError("pool_type='cls_token' needs cls_token=True")
        super().__init__()
        self.patch_embed = nn.Conv2d(3, d_model, patch_size, patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d_model)) if cls_token else None
        self.pe = nn.Parameter(torch.empty(1, (img_size // patch_size) ** 2, d_model))
        nn.init.normal_(self.pe, 0, 0.02)
        self.layers = nn.Sequential()
        for _ in range(depth):
            self.layers.append(ViTBlock(d_model, n_heads, bias, mlp_ratio, dropout, layer_scale_init, stochastic_depth, norm_eps))
        self.norm = nn.LayerNorm(d_model, norm_eps)
        self.pool_type = pool_type
        self.pooler = MHAPooling(d_model, n_heads, bias, mlp_ratio, norm_eps) if pool_type == "mha" else None
        self.patch_size, self.d_model = int(patch_size), int(d_model)

    def get_last_out_channels(self) -> int:
        return self.d_model

    # -- launch-list emission ---------------------------------------------------------------------
    def _vt_refusal(self) -> "str | None":
        if self.pool_type == "mha":
            return "pool_type='mha': the single-query cross-attention pooler has no kernel on the MI355X path (CPU tensors run)"
        for m in self.layers:
            why = m._vt_refusal()
            if why is not None:
                return why
        return None

    def _check_patches(self, H: int, W: int) -> None:
        p = self.patch_size
        if H % p or W % p or (H // p) * (W // p) != self.pe.shape[1]:
            raise ValueError(f"a {H}x{W} image is not {self.pe.shape[1]} patches of {p}x{p}, the token count of pe "
                             "(resize_pe retargets the model)")

    def _vt_emit_maps(self, b, x):
        from ..engine import _EPC

        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        self._check_patches(x.H, x.W)
        if self.d_model % _EPC[b.dtype]:
            raise NotImplementedError(f"d_model={self.d_model} must be a multiple of {_EPC[b.dtype]} for dtype {b.dtype}")
        e = b.patch_embed(x, self.patch_embed, name="patch_embed")
        o = self._vt_emit_tokens(b, e)
        for i, blk in enumerate(self.layers):
            o = blk._vt_emit(b, o, name=f"layers.{i}")
        return [self._vt_emit_pool(b, o)]

    # (the two ends of the token map that a subclass with other prefix tokens replaces: DeiT)
    def _vt_emit_tokens(self, b, e):
        return b.vit_tokens(e, self.pe, self.cls_token, name="tokens")

    def _vt_emit_pool(self, b, o):
        if self.pool_type == "cls_token":
            return b.layer_norm(b.token_select(o, 0, name="pool"), self.norm, name="norm")
        return b.global_avgpool(b.layer_norm(o, self.norm, name="norm"), name="pool")

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        out = self.patch_embed(x).flatten(2).transpose(1, 2) + self.pe  # (B, C, gh, gw) -> (B, tokens, C)
        if self.cls_token is not None:
            out = torch.cat([self.cls_token.expand(out.shape[0], -1, -1), out], 1)
        out = self.layers(out)
        if self.pool_type == "cls_token":
            return [self.norm(out[:, 0])]
        if self.pool_type == "gap":
            return [self.norm(out).mean(1)]
        return [self.pooler(self.norm(out))]

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
        """interpolate the position embedding to a `size` x `size` image (host code, as in the reference).  `pe` becomes a NEW
        parameter of another length: the flat parameter store and the compiled programs are dropped, since the store only
        compares the count and the data pointers of what it tracks."""
        old_size = int(self.pe.shape[1] ** 0.5)
        new_size = size // self.patch_size
        pe = self.pe.unflatten(1, (old_size, old_size)).permute(0, 3, 1, 2)
        pe = F.interpolate(pe.float(), (new_size, new_size), mode=interpolation_mode)
        self.pe = nn.Parameter(pe.permute(0, 2, 3, 1).flatten(1, 2).contiguous())
        r = _RUNNERS.get(self)
        if r is not None:
            r.store.pflat = None  # ParamStore.stale() -> True: the next call lays the parameters out again
            r.cache.clear()

    # -- configurations and the official Flax checkpoints -----------------------------------------
    _VARIANTS = {"Ti": (192, 12, 3), "S": (384, 12, 6), "M": (512, 12, 8), "B": (768, 12, 12), "L": (1024, 24, 16),
                 "H": (1280, 32, 16)}
    _CKPT_URL = "https://storage.googleapis.com/"
    _AUGREG = {
        ("Ti", 16): "Ti_16-i21k-300ep-lr_0.001-aug_none-wd_0.03-do_0.0-sd_0.0.npz",
        ("S", 32): "S_32-i21k-300ep-lr_0.001-aug_none-wd_0.1-do_0.0-sd_0.0.npz",
        ("S", 16): "S_16-i21k-300ep-lr_0.001-aug_light1-wd_0.03-do_0.0-sd_0.0.npz",
        ("B", 32): "B_32-i21k-300ep-lr_0.001-aug_light1-wd_0.1-do_0.0-sd_0.0.npz",
        ("B", 16): "B_16-i21k-300ep-lr_0.001-aug_medium1-wd_0.1-do_0.0-sd_0.0.npz",
        ("L", 16): "L_16-i21k-300ep-lr_0.001-aug_strong1-wd_0.1-do_0.0-sd_0.0.npz",
    }
    _SIGLIP = {
        ("B", 16, 224): "webli_en_b16_224_63724782.npz",
        ("B", 16, 256): "webli_en_b16_256_60500360.npz",
        ("B", 16, 384): "webli_en_b16_384_68578854.npz",
        ("B", 16, 512): "webli_en_b16_512_68580893.npz",
        ("L", 16, 256): "webli_en_l16_256_60552751.npz",
        ("L", 16, 384): "webli_en_l16_384_63634585.npz",
    }

    @staticmethod
    def from_config(variant: str, img_size: int, *, weights: "str | None" = None) -> "ViT":
        """`variant` is "<size>_<patch>", e.g. "Ti_16"; `weights`: None, "augreg" (224 px) or "siglip" (no class token, the
        attention pooler), which download the official checkpoint into the torch hub directory once"""
        size, patch = variant.split("_")
        d_model, depth, n_heads = ViT._VARIANTS[size]
        patch = int(patch)
        if weights not in (None, "augreg", "siglip"):
            raise ValueError(f"Unsupported weights={weights}")
        kwargs = dict(cls_token=False, pool_type="mha") if weights == "siglip" else {}
        if weights == "augreg":
            if img_size != 224:
                raise ValueError("weights='augreg' are 224 px checkpoints")
            rel, big_vision, prefix = "vit_models/augreg/" + ViT._AUGREG[(size, patch)], False, ""
        elif weights == "siglip":
            rel, big_vision, prefix = "big_vision/siglip/" + ViT._SIGLIP[(size, patch, img_size)], True, "params/img/"
        m = ViT(d_model, depth, n_heads, patch, img_size, **kwargs)
        if weights is not None:
            path = os.path.join(torch.hub.get_dir(), "checkpoints", rel.replace("/", "_"))
            if not os.path.exists(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
                torch.hub.download_url_to_file(ViT._CKPT_URL + rel, path)
            m.load_flax_ckpt(path, big_vision=big_vision, prefix=prefix)
        return m

    @torch.no_grad()
    def load_flax_ckpt(self, path: str, big_vision: bool = False, prefix: str = "") -> None:
        """read a local Flax `.npz` checkpoint in the vision_transformer layout (`cls`, `Transformer/posembed_input/
        pos_embedding` with the class token's row first -- it is folded into `cls_token` -- , `embedding`,
        `Transformer/encoderblock_i/{LayerNorm_0, MultiHeadDotProductAttention_1, LayerNorm_2, MlpBlock_3}`,
        `Transformer/encoder_norm`) or, with `big_vision`, the big_vision one (`pos_embedding`, `LayerNorm_0,
        MultiHeadDotProductAttention_0, LayerNorm_1, MlpBlock_0`, `MAPHead_0/...` for the pooler).  Only arrays under
        `prefix` are read.  What may remain is the classifier head (`head/...`, `pre_logits/...`); anything else left over,
        and any array the model needs and the file lacks, raises KeyError."""
        if big_vision:
            mha_norm, mha, mlp_norm, mlp = "LayerNorm_0", "MultiHeadDotProductAttention_0", "LayerNorm_1", "MlpBlock_0"
        else:
            mha_norm, mha, mlp_norm, mlp = "LayerNorm_0", "MultiHeadDotProductAttention_1", "LayerNorm_2", "MlpBlock_3"
        with np.load(path) as f:
            left = {k[len(prefix):]: f[k] for k in f.files if k.startswith(prefix)}
        if self.cls_token is not None:
            _flax_take(self.cls_token, left, "cls")
        if big_vision:
            _flax_take(self.pe, left, "pos_embedding")
        else:
            pe = torch.from_numpy(np.asarray(left.pop("Transformer/posembed_input/pos_embedding")))
            if self.cls_token is None:
                raise KeyError("load_flax_ckpt: this layout stores the class token's position in row 0: cls_token=True")
            self.cls_token.add_(pe[:, 0])
            self.pe.copy_(pe[:, 1:])
        _flax_take(self.patch_embed.weight, left, "embedding/kernel", lambda v: v.permute(3, 2, 0, 1))
        _flax_take(self.patch_embed.bias, left, "embedding/bias")
        _flax_ln(self.norm, left, "Transformer/encoder_norm")
        for i, layer in enumerate(self.layers):
            pre = f"Transformer/encoderblock_{i}"
            _flax_ln(layer.mha[0], left, f"{pre}/{mha_norm}")
            _flax_mha(layer.mha[1], left, f"{pre}/{mha}")
            _flax_ln(layer.mlp[0], left, f"{pre}/{mlp_norm}")
            _flax_linear(layer.mlp[1].linear1, left, f"{pre}/{mlp}/Dense_0")
            _flax_linear(layer.mlp[1].linear2, left, f"{pre}/{mlp}/Dense_1")
        if self.pooler is not None:
            _flax_take(self.pooler.probe, left, "MAPHead_0/probe")
            _flax_mha(self.pooler.mha, left, "MAPHead_0/MultiHeadDotProductAttention_0")
            _flax_ln(self.pooler.norm, left, "MAPHead_0/LayerNorm_0")
            _flax_linear(self.pooler.mlp.linear1, left, "MAPHead_0/MlpBlock_0/Dense_0")
            _flax_linear(self.pooler.mlp.linear2, left, "MAPHead_0/MlpBlock_0/Dense_1")
        extra = sorted(k for k in left if not k.startswith(("head/", "pre_logits/")))
        if extra:
            raise KeyError(f"load_flax_ckpt: unexpected keys {extra}")
