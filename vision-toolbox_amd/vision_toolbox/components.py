"""ConvNormAct -- the fused Conv -> BatchNorm -> ReLU unit of the hot path -- and SeparableConv2d, the depthwise + pointwise
pair of such units that BiFPN builds on, and SPPBlock, the cascaded-pooling block of YOLOv5-style necks.

Same constructor signature, child names (`conv`, `norm`, `act`) and therefore the same
state_dict keys as the reference unit (vision_toolbox/components.py:13-46), and the
children are real nn.Conv2d / nn.BatchNorm2d instances so that the reference's
isinstance-based parameter grouping (classifier.py:111-155) keeps working.  What differs
is execution: on the GPU the unit is not three ATen calls but a few launches of
libvt_amd (implicit-GEMM conv on MFMA with the BN statistics in its epilogue, one
normalise+ReLU(+residual) pass), emitted into a static launch list by `_vt_emit`.
CPU tensors run the children with plain torch ops (`_eager_maps`), as in the reference.

Every constructor argument of the reference unit runs on the GPU: the Darknet / VoVNet configuration (bn + relu, groups
= dilation = 1) on the fused kernels; other activations, `groups` (>= one 16-byte channel chunk per group), `dilation`
and norm="none" on the general kernels (engine.Builder.conv_unit / _grouped_unit).  Depthwise units (groups = in_channels = out_channels) run on the streaming kernels of vt_dwconv.hip (round 6); other groups narrower than a 16-byte channel slice raise.
"""
from __future__ import annotations

import math
import weakref
from functools import partial
from typing import Callable, Optional

import torch
from torch import Tensor, nn

__all__ = ["ConvNormAct", "SeparableConv2d", "SPPBlock", "HipModule", "Permute", "StochasticDepth", "LayerScale"]

_RUNNERS: "weakref.WeakKeyDictionary[nn.Module, object]" = weakref.WeakKeyDictionary()


class HipModule(nn.Module):
    """Mixin: a module whose forward is a compiled libvt_amd program.

    Subclasses implement `_vt_emit_maps(builder, x_ref) -> list[TRef]`.
    `compute_dtype` (None / torch.float32 / torch.bfloat16) overrides the dtype rule
    (f32 input -> exact-f32 kernels, bf16 input or bf16 autocast -> bf16 kernels).
    """

    compute_dtype: Optional[torch.dtype] = None

    def _vt_runner(self):
        r = _RUNNERS.get(self)
        if r is None:
            from .program import BackboneRunner

            r = BackboneRunner(self)
            _RUNNERS[self] = r
        return r

    def _vt_emit_maps(self, b, x):  # pragma: no cover - abstract
        raise NotImplementedError

    def _vt_emit(self, b, x, out=None):
        return self._vt_emit_maps(b, x)[-1]

    # Dispatch rule: the SAME module class serves CPU tensors through plain torch ops over
    # its own nn.Conv2d / nn.BatchNorm2d / nn.ReLU children (`_eager*`), and GPU tensors through
    # libvt_amd.  The runner picks by `x.is_cuda`; a GPU tensor never takes the eager path.
    def _eager_maps(self, x: Tensor) -> "list[Tensor]":  # pragma: no cover - abstract
        raise NotImplementedError

    def _eager(self, x: Tensor) -> Tensor:
        return self._eager_maps(x)[-1]

    def forward(self, x: Tensor) -> Tensor:
        return self._vt_runner()(x, all_maps=False, compute_dtype=self.compute_dtype)[-1]


_ACTS = {
    "none": lambda: nn.Identity(),
    "relu": lambda: nn.ReLU(inplace=True),
    "leaky_relu": lambda: nn.LeakyReLU(0.2, inplace=True),
    "swish": lambda: nn.SiLU(inplace=True),
    "silu": lambda: nn.SiLU(inplace=True),
    "gelu": lambda: nn.GELU(),
}
_NORMS = {"none": lambda c: nn.Identity(), "bn": lambda c: nn.BatchNorm2d(c)}


class ConvNormAct(nn.Sequential, HipModule):
    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        kernel_size: int = 3,
        stride: int = 1,
        dilation: int = 1,
        groups: int = 1,
        norm: str = "bn",
        act: str = "relu",
    ):
        if norm not in _NORMS:
            raise KeyError(norm)
        if act not in _ACTS:
            raise KeyError(act)
        super().__init__()
        # "same"-style padding of the reference: ceil((k - s) / 2)  (components.py:31)
        pad = -((stride - kernel_size) // 2)
        assert pad == math.ceil((kernel_size - stride) / 2)
        self.add_module(
            "conv",
            nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, dilation=dilation,
                      groups=groups, bias=(norm == "none")),
        )
        self.add_module("norm", _NORMS[norm](out_channels))
        self.add_module("act", _ACTS[act]())
        self._act_name = act
        if act in ("relu", "leaky_relu"):
            # N(0, sqrt(2 / ((1 + 0.2^2) * fan_out)))  (components.py:45-46)
            nn.init.kaiming_normal_(self.conv.weight, a=0.2, mode="fan_out", nonlinearity=act)

    # -- launch-list emission ----------------------------------------------------------
    def _vt_relu(self) -> int:
        """activation code of the kernels (include/vt_amd.h): 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 SiLU, 4 GELU (exact); the kernels
        also take 5 ReLU6 and 6 Hardswish (the MobileNets), which the reference's ConvNormAct does not have"""
        a = self.act
        if isinstance(a, nn.Identity):
            return 0
        if isinstance(a, nn.ReLU):
            return 1
        if isinstance(a, nn.LeakyReLU) and abs(a.negative_slope - 0.2) < 1e-12:
            return 2
        if isinstance(a, nn.SiLU):
            return 3
        if isinstance(a, nn.GELU) and getattr(a, "approximate", "none") == "none":
            return 4
        raise NotImplementedError(
            f"activation {a!r}: the MI355X path implements ConvNormAct's own choices (components.py:37-44: none, relu, "
            "leaky_relu(0.2), swish / silu, gelu)"
        )

    def _vt_emit(self, b, x, out=None, residual=None, name: str = "cna", pool_out=None, defer_norm: bool = False):
        """`pool_out`: also write MaxPool2d(3, 2, 1) of the unit's output there (VoVNet's `stage.max_pool`, vovnet.py:94):
        fused into the unit's normalise pass where one exists, else a pool launch.  `defer_norm`: the output goes to
        Builder.conv_unit_pair, which may take over the normalise pass (Builder.conv_unit)"""
        norm = self.norm if isinstance(self.norm, nn.BatchNorm2d) else None
        return b.conv_unit(x, self.conv, norm, self._vt_relu(), residual=residual, out=out, name=name, pool_out=pool_out,
                           defer_norm=defer_norm)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        return [self.act(self.norm(self.conv(x)))]

    def forward(self, x: Tensor) -> Tensor:
        return HipModule.forward(self, x)


def _sep_act_code(a: nn.Module, name: str) -> int:
    """activation code of the kernels for what `act_fn()` returned (include/vt_amd.h)"""
    for cls, code in ((nn.Identity, 0), (nn.ReLU6, 5), (nn.ReLU, 1), (nn.SiLU, 3), (nn.Hardswish, 6)):
        if isinstance(a, cls):
            return code
    raise NotImplementedError(f"{name}: activation {a!r} -- the MI355X path of SeparableConv2d implements Identity, ReLU, SiLU, "
                              "ReLU6 and Hardswish")


class _ConvBNAct(nn.Sequential):
    """conv -> norm -> act under the child names of the reference's ConvNormAct (state_dict keys conv.weight, norm.*)"""

    def __init__(self, conv: nn.Conv2d, norm: nn.BatchNorm2d, act: nn.Module):
        super().__init__()
        self.add_module("conv", conv)
        self.add_module("norm", norm)
        self.add_module("act", act)


class SeparableConv2d(nn.Sequential, HipModule):
    """Depthwise k x k Conv-BN-act (`dw`) then pointwise 1x1 Conv-BN-act (`pw`): the block BiFPN builds on.

    The reference's class (components.py:49-72) cannot be constructed -- it hands `padding=` and `act_fn=` to ConvNormAct,
    which takes neither -- so this implements what its ten lines evidently mean: both convolutions without bias, each
    followed by BatchNorm2d and `act_fn()`, torch's default Conv2d initialisation (ConvNormAct re-initialises only for
    relu / leaky_relu).  On the GPU `dw` runs on the tiled depthwise kernels (Builder.depthwise_unit: kernel_size 3 or 5,
    stride 1 or 2, padding (k - 1) / 2, dilation 1; other geometries are refused with its message) and `pw` is a conv_unit."""

    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        kernel_size: int = 3,
        stride: int = 1,
        padding: int = 1,
        dilation: int = 1,
        act_fn: Callable[[], nn.Module] = partial(nn.ReLU6, inplace=True),
    ):
        super().__init__()
        self.add_module("dw", _ConvBNAct(
            nn.Conv2d(in_channels, in_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                      groups=in_channels, bias=False),
            nn.BatchNorm2d(in_channels), act_fn()))
        self.add_module("pw", _ConvBNAct(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                                         act_fn()))

    def _vt_emit(self, b, x, out=None, name: str = "sep"):
        h = b.depthwise_unit(x, self.dw.conv, self.dw.norm, _sep_act_code(self.dw.act, name + ".dw"), name=name + ".dw")
        return b.conv_unit(h, self.pw.conv, self.pw.norm, _sep_act_code(self.pw.act, name + ".pw"), out=out, name=name + ".pw")

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        return [self.pw(self.dw(x))]

    def forward(self, x: Tensor) -> Tensor:
        return HipModule.forward(self, x)


class SPPBlock(HipModule):
    """The SPPF block of YOLOv5-style necks (reference components.py:139-152): one child `pool` -- MaxPool2d or AvgPool2d
    (kernel_size, 1, (kernel_size - 1) // 2) -- applied `repeats` times in a cascade; the output is the concat of the
    `repeats` pooled maps over channels (the input itself is not part of it).  No parameters.

    On the GPU the whole block is one forward launch that writes every stage into its channel slice of the output and one
    backward launch (Builder.spp -> vt_spp_fwd / vt_spp_bwd): odd kernel_size in 3..15, repeats in 1..4 and
    repeats * (kernel_size - 1) / 2 <= 8 -- (5, 3), (3, 4), (7, 2), (9, 2), (13, 1) among them; other geometries raise
    NotImplementedError.  An even kernel_size with repeats > 1 raises on every path: the maps shrink by a pixel per stage
    and the reference's torch.cat refuses them."""

    def __init__(self, kernel_size: int = 5, repeats: int = 3, pool: str = "max"):
        super().__init__()
        self.pool = dict(avg=nn.AvgPool2d, max=nn.MaxPool2d)[pool](kernel_size, 1, (kernel_size - 1) // 2)
        self.repeats = repeats

    def _vt_geometry(self) -> "tuple[int, int, str]":
        k = self.pool.kernel_size
        if not isinstance(k, int):
            if len(set(k)) != 1:
                raise NotImplementedError(f"SPPBlock: kernel_size {k!r} -- the MI355X path pools over square windows")
            k = k[0]
        return int(k), int(self.repeats), "avg" if isinstance(self.pool, nn.AvgPool2d) else "max"

    def _check_concat(self) -> None:
        k = self.pool.kernel_size
        if self.repeats > 1 and any(int(v) % 2 == 0 for v in ((k,) if isinstance(k, int) else k)):
            raise RuntimeError(f"SPPBlock: an even kernel_size ({k}) shrinks the map by a pixel per stage, so the {self.repeats} "
                               "pooled maps cannot be concatenated")

    def _vt_emit(self, b, x, out=None, name: str = "spp"):
        self._check_concat()
        k, repeats, pool = self._vt_geometry()
        if x.logical_c != x.C:  # (an image whose channels were padded: the concat would interleave the padding)
            raise NotImplementedError(f"{name}: SPPBlock over {x.logical_c} channels, which are not whole 16-byte chunks")
        return b.spp(x, k, repeats, pool, out=out, name=name)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        outputs = []
        for _ in range(self.repeats):
            x = self.pool(x)
            outputs.append(x)
        return [torch.cat(outputs, dim=1)]

    def forward(self, x: Tensor) -> Tensor:
        self._check_concat()
        return HipModule.forward(self, x)


# -- small modules of the reference's components.py that ConvNeXt's state_dict layout and CPU path need -----------------
# (on the GPU a ConvNeXt block is a launch list -- backbones/convnext.py -- and these are never called)
class Permute(nn.Module):
    def __init__(self, *dims: int) -> None:
        super().__init__()
        self.dims = tuple(dims)

    def forward(self, x: Tensor) -> Tensor:
        return x.permute(*self.dims)

    def extra_repr(self) -> str:
        return ", ".join(str(d) for d in self.dims)


class StochasticDepth(nn.Module):
    """drops the whole residual branch of a sample with probability p (training only), rescaling the survivors"""

    def __init__(self, p: float) -> None:
        super().__init__()
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be in [0, 1], got {p}")
        self.p = p

    def forward(self, x: Tensor) -> Tensor:
        if not self.training or self.p == 0.0:
            return x
        keep = 1.0 - self.p
        if keep == 0.0:
            return torch.zeros_like(x)
        mask = torch.empty((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device).bernoulli_(keep)
        return x * (mask / keep)

    def extra_repr(self) -> str:
        return f"p={self.p}"


class LayerScale(nn.Module):
    """per-channel scale over the last axis; the parameter is called `gamma`"""

    def __init__(self, dim: int, init: float) -> None:
        super().__init__()
        self.gamma = nn.Parameter(torch.full((dim,), float(init)))

    def forward(self, x: Tensor) -> Tensor:
        return x * self.gamma

    def extra_repr(self) -> str:
        return f"dim={self.gamma.numel()}"
