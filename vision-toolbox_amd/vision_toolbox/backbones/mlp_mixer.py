"""MLP-Mixer (https://arxiv.org/abs/2105.01601) on libvt_amd.

Constructor signatures and child names follow the reference (vision_toolbox/backbones/mlp_mixer.py:16-64, the `MLP` of
backbones/vit.py:51-57), so state_dict keys are the reference's: `patch_embed` (p x p stride-p conv),
`layers.i.norm1`, `layers.i.token_mixing.linear1|linear2`, `layers.i.norm2`, `layers.i.channel_mixing.linear1|linear2`,
`norm`.  Note `tokens_mlp_dim = int(d_model * mlp_ratio[0])`: a fraction of d_model, not of the token count.

The reference flattens the embedded image to (B, tokens, C) and transposes it twice per block for the token MLP.  The
launch lists here keep ONE layout, the NHWC map [B, gh, gw, C] (tokens = pixels), and never transpose: token mixing is
a GEMM whose reduction index is the pixel index (vt_token_mix.hip).  Per block ("MLP-Mixer"):

    vt_layernorm_fwd         norm1
    vt_token_mix_fwd         token_mixing.linear1 + bias, writes the pre-activation and its exact GELU
    vt_token_mix_fwd         token_mixing.linear2 + bias + the block's shortcut
    vt_layernorm_fwd         norm2
    vt_conv_igemm            channel_mixing.linear1 + bias as a 1x1 conv, then
    vt_bn_act_apply          exact GELU
    vt_conv_igemm            channel_mixing.linear2 + bias
    vt_scale_residual_fwd    the plain add (gamma = None)

in front of them vt_patchify_fwd + one vt_conv_igemm (the patch embedding as a Linear over a patch's 3 p p values),
behind them vt_layernorm_fwd and vt_global_avgpool_fwd: LayerNorm BEFORE the mean, the reverse of ConvNeXt.
`forward(x)` returns (B, d_model).

Refused on CUDA tensors (all of them construct and run on CPU tensors): `dropout > 0` in training mode
(NotImplementedError), an input whose H or W differs from `img_size` (ValueError), a `d_model` that is no multiple of a
16-byte chunk of the compute dtype (NotImplementedError).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor, nn

from ..components import HipModule

__all__ = ["MLP", "MixerBlock", "MLPMixer"]


class MLP(nn.Sequential):
    """Linear -> GELU -> Linear -> Dropout over the last axis; children `linear1`, `act`, `linear2`, `dropout`"""

    def __init__(self, in_dim: int, hidden_dim: int, dropout: float = 0.0) -> None:
        super().__init__()
        self.linear1 = nn.Linear(in_dim, int(hidden_dim))
        self.act = nn.GELU()
        self.linear2 = nn.Linear(int(hidden_dim), in_dim)
        self.dropout = nn.Dropout(dropout)


class MixerBlock(nn.Module):
    def __init__(
        self,
        n_tokens: int,
        d_model: int,
        mlp_ratio: "tuple[float, float]" = (0.5, 4.0),
        dropout: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        super().__init__()
        tokens_mlp_dim, channels_mlp_dim = int(d_model * mlp_ratio[0]), int(d_model * mlp_ratio[1])
        self.norm1 = nn.LayerNorm(d_model, norm_eps)
        self.token_mixing = MLP(n_tokens, tokens_mlp_dim, dropout)
        self.norm2 = nn.LayerNorm(d_model, norm_eps)
        self.channel_mixing = MLP(d_model, channels_mlp_dim, dropout)

    def forward(self, x: Tensor) -> Tensor:  # (B, n_tokens, d_model); the CPU path
        if x.is_cuda:
            raise NotImplementedError("a MixerBlock takes a token map: on the GPU it runs as part of an MLPMixer program")
        x = x + self.token_mixing(self.norm1(x).transpose(-1, -2)).transpose(-1, -2)
        return x + self.channel_mixing(self.norm2(x))

    def _vt_refusal(self) -> "str | None":
        if self.training and (self.token_mixing.dropout.p > 0.0 or self.channel_mixing.dropout.p > 0.0):
            return "dropout > 0 in training mode has no kernel on the MI355X path (eval mode and CPU tensors run)"
        return None

    def _vt_emit(self, b, x, name: str = "block"):
        """x: NHWC map [B, gh, gw, C], tokens = pixels"""
        why = self._vt_refusal()
        if why is not None:
            raise NotImplementedError(why)
        tm, cm = self.token_mixing, self.channel_mixing
        n = b.layer_norm(x, self.norm1, name=name + ".norm1")
        h = b.token_linear(n, tm.linear1, act=4, name=name + ".token_mixing.linear1")
        x = b.token_linear(h, tm.linear2, residual=x, name=name + ".token_mixing.linear2")
        n = b.layer_norm(x, self.norm2, name=name + ".norm2")
        h = b.linear_unit(n, cm.linear1, act=4, name=name + ".channel_mixing.linear1")
        t = b.linear_unit(h, cm.linear2, name=name + ".channel_mixing.linear2")
        return b.scale_residual(t, None, x, name=name + ".add")


def _flax_take(dst: Tensor, weights: dict, key: str, perm=None) -> None:
    """move array `key` of a Flax checkpoint into `dst`, axes permuted by `perm` (Flax kernels are stored input-major)"""
    v = torch.from_numpy(np.asarray(weights.pop(key)))
    dst.copy_(v.permute(*perm) if perm is not None else v)


def _flax_affine(mod: nn.Module, weights: dict, prefix: str, weight_key: str, perm=None) -> None:
    _flax_take(mod.weight, weights, f"{prefix}/{weight_key}", perm)
    _flax_take(mod.bias, weights, f"{prefix}/bias")


class MLPMixer(HipModule):
    def __init__(
        self,
        n_layers: int,
        d_model: int,
        patch_size: int,
        img_size: int,
        mlp_ratio: "tuple[float, float]" = (0.5, 4.0),
        dropout: float = 0.0,
        norm_eps: float = 1e-6,
    ) -> None:
        if img_size % patch_size:
            raise ValueError(f"img_size={img_size} is no multiple of patch_size={patch_size}")
        super().__init__()
        self.patch_embed = nn.Conv2d(3, d_model, patch_size, patch_size)
        n_tokens = (img_size // patch_size) ** 2
        self.layers = nn.Sequential(*[MixerBlock(n_tokens, d_model, mlp_ratio, dropout, norm_eps) for _ in range(n_layers)])
        self.norm = nn.LayerNorm(d_model, norm_eps)
        self.img_size, self.patch_size, self.d_model = int(img_size), int(patch_size), int(d_model)

    def get_last_out_channels(self) -> int:
        return self.d_model

    # -- launch-list emission ---------------------------------------------------------------------
    def _vt_emit_maps(self, b, x):
        from ..engine import _EPC

        if (x.H, x.W) != (self.img_size, self.img_size):
            raise ValueError(f"MLPMixer(img_size={self.img_size}) got a {x.H}x{x.W} image: the token count is part of the weights")
        if self.d_model % _EPC[b.dtype]:
            raise NotImplementedError(f"d_model={self.d_model} must be a multiple of {_EPC[b.dtype]} for dtype {b.dtype}")
        o = b.patch_embed(x, self.patch_embed, name="patch_embed")
        for i, blk in enumerate(self.layers):
            o = blk._vt_emit(b, o, name=f"layers.{i}")
        o = b.layer_norm(o, self.norm, name="norm")
        return [b.global_avgpool(o, name="pool")]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        t = self.patch_embed(x).flatten(2).transpose(1, 2)  # (B, C, gh, gw) -> (B, tokens, C)
        return [self.norm(self.layers(t)).mean(1)]

    def _vt_check(self, x: Tensor) -> None:
        if isinstance(x, Tensor) and x.is_cuda:
            if x.dim() == 4 and tuple(x.shape[2:]) != (self.img_size, self.img_size):
                raise ValueError(f"MLPMixer(img_size={self.img_size}) got a {x.shape[2]}x{x.shape[3]} image: the token count is "
                                 "part of the weights")
            for m in self.layers:
                why = m._vt_refusal()
                if why is not None:
                    raise NotImplementedError(why)

    def forward(self, x: Tensor) -> Tensor:
        self._vt_check(x)
        y = self._vt_runner()(x, all_maps=False, compute_dtype=self.compute_dtype)[-1]
        return y.flatten(1) if x.is_cuda else y  # (B, C, 1, 1) -> (B, C)

    # -- configurations (Table 1 of the paper) and the official Flax checkpoints ------------------
    _VARIANTS = {"S": (8, 512), "B": (12, 768), "L": (24, 1024), "H": (32, 1280)}
    _CKPT_URL = "https://storage.googleapis.com/mixer_models/"
    _CKPTS = {
        ("S", 8): "gsam/Mixer-S_8.npz",
        ("S", 16): "gsam/Mixer-S_16.npz",
        ("S", 32): "gsam/Mixer-S_32.npz",
        ("B", 16): "imagenet21k/Mixer-B_16.npz",
        ("B", 32): "gsam/Mixer-B_32.npz",
        ("L", 16): "imagenet21k/Mixer-L_16.npz",
    }

    @staticmethod
    def from_config(variant: str, patch_size: int, img_size: int, pretrained: bool = False) -> "MLPMixer":
        n_layers, d_model = MLPMixer._VARIANTS[variant]
        m = MLPMixer(n_layers, d_model, patch_size, img_size)
        if pretrained:
            import os

            rel = MLPMixer._CKPTS[(variant, patch_size)]
            path = os.path.join(torch.hub.get_dir(), "checkpoints", rel.replace("/", "_"))
            if not os.path.exists(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
                torch.hub.download_url_to_file(MLPMixer._CKPT_URL + rel, path)
            m.load_jax_weights(path)
        return m

    @torch.no_grad()
    def load_jax_weights(self, path: str) -> None:
        """read a Flax `.npz` checkpoint: `stem/{kernel,bias}` (kernel [p][p][3][d_model]),
        `MixerBlock_i/LayerNorm_{0,1}/{scale,bias}`, `MixerBlock_i/{token,channel}_mixing/Dense_{0,1}/{kernel,bias}` (kernels
        [in][out]), `pre_head_layer_norm/{scale,bias}`.  What may remain is the classifier head (`head/...`)."""
        with np.load(path) as f:
            left = {k: f[k] for k in f.files}
        _flax_affine(self.patch_embed, left, "stem", "kernel", perm=(3, 2, 0, 1))
        _flax_affine(self.norm, left, "pre_head_layer_norm", "scale")
        for i, blk in enumerate(self.layers):
            pre = f"MixerBlock_{i}"
            _flax_affine(blk.norm1, left, f"{pre}/LayerNorm_0", "scale")
            _flax_affine(blk.norm2, left, f"{pre}/LayerNorm_1", "scale")
            for mlp, what in ((blk.token_mixing, "token_mixing"), (blk.channel_mixing, "channel_mixing")):
                _flax_affine(mlp.linear1, left, f"{pre}/{what}/Dense_0", "kernel", perm=(1, 0))
                _flax_affine(mlp.linear2, left, f"{pre}/{what}/Dense_1", "kernel", perm=(1, 0))
        extra = sorted(k for k in left if not k.startswith("head/"))
        if extra:
            raise KeyError(f"load_jax_weights: unexpected keys {extra}")
