"""ConvNormAct -- the fused Conv -> BatchNorm -> ReLU unit of the hot path -- and SeparableConv2d, the depthwise + pointwise
pair of such units that BiFPN builds on, SPPBlock, the cascaded-pooling block of YOLOv5-style necks, and DeformableConv2d,
the modulated deformable convolution (defined here and importable by name; it is not listed in `__all__`).

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


class DeformConv2d(nn.Module):
    """The deformable convolution layer under torchvision's names (torchvision.ops.DeformConv2d is not a dependency of this
    package): `weight` (out_channels, in_channels / groups, k, k) with kaiming_uniform_(a=sqrt(5)), `bias` (out_channels,)
    with U(+-1 / sqrt(fan_in)).  forward(x, offset, mask=None) is deform_conv2d in plain torch, gather form: the CPU path of
    DeformableConv2d (the GPU path never calls it: Builder.deform_conv)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, dilation=1, groups: int = 1,
                 bias: bool = True):
        super().__init__()
        if in_channels % groups or out_channels % groups:
            raise ValueError("in_channels and out_channels must be divisible by groups")
        pair = lambda v: (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.kernel_size, self.stride, self.padding, self.dilation = pair(kernel_size), pair(stride), pair(padding), pair(dilation)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.weight.shape[1] * self.weight.shape[2] * self.weight.shape[3]
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x: Tensor, offset: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        return deform_conv2d(x, offset, self.weight, self.bias, self.stride, self.padding, self.dilation, mask)


def deform_conv2d(x: Tensor, offset: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride=(1, 1), padding=(0, 0),
                  dilation=(1, 1), mask: Optional[Tensor] = None) -> Tensor:
    """torchvision's deform_conv2d with one offset group, in plain torch and differentiable by autograd.  Offset channel 2t is
    dy and 2t + 1 is dx of tap t = i * kw + j; the sampling position is (ho * s - p + i * d + dy, wo * s - p + j * d + dx);
    bilinear over floor and floor + 1, a corner outside the map contributes zero; the sample times the mask, then the weighted
    sum over (tap, channel) plus bias.  `floor` has no gradient, so at an exactly integer position d(offset) is the right-hand
    derivative, which is torchvision's choice."""
    B, C_, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    K2, G = kh * kw, C_ // Cg
    Ho, Wo = offset.shape[-2:]
    if offset.shape[1] != 2 * K2:
        raise ValueError(f"offset has {offset.shape[1]} channels, one offset group of a {kh}x{kw} kernel has {2 * K2}")
    dev, dt = x.device, x.dtype
    ti = torch.arange(kh, device=dev).repeat_interleave(kw) * dilation[0]
    tj = torch.arange(kw, device=dev).repeat(kh) * dilation[1]
    by = (torch.arange(Ho, device=dev) * stride[0] - padding[0]).view(1, 1, Ho, 1) + ti.view(1, K2, 1, 1)
    bx = (torch.arange(Wo, device=dev) * stride[1] - padding[1]).view(1, 1, 1, Wo) + tj.view(1, K2, 1, 1)
    off = offset.reshape(B, K2, 2, Ho, Wo)
    py, px = by.to(dt) + off[:, :, 0], bx.to(dt) + off[:, :, 1]
    y0, x0 = py.detach().floor(), px.detach().floor()
    ly, lx = py - y0, px - x0
    flat = x.reshape(B, C_, H * W)

    def corner(yy: Tensor, xx: Tensor, wgt: Tensor) -> Tensor:
        valid = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, 1, K2 * Ho * Wo).expand(B, C_, K2 * Ho * Wo)
        v = torch.gather(flat, 2, idx).view(B, C_, K2, Ho, Wo)
        return v * (wgt * valid.to(dt)).unsqueeze(1)

    col = (corner(y0, x0, (1 - ly) * (1 - lx)) + corner(y0, x0 + 1, (1 - ly) * lx) + corner(y0 + 1, x0, ly * (1 - lx)) +
           corner(y0 + 1, x0 + 1, ly * lx))
    if mask is not None:
        col = col * mask.reshape(B, 1, K2, Ho, Wo)
    y = torch.einsum("bgckhw,gock->bgohw", col.view(B, G, Cg, K2, Ho, Wo), weight.reshape(G, Cout // G, Cg, K2))
    y = y.reshape(B, Cout, Ho, Wo)
    return y if bias is None else y + bias.view(1, Cout, 1, 1)


class DeformableConv2d(HipModule):
    """Modulated deformable convolution (DCNv2; v2=False: DCNv1 without the mask) with the reference's signature and children
    (components.py:77-135): `conv_offset = conv_fn(Cin, 2 k^2, k, stride=, padding=, dilation=)`, `conv_mask =
    Sequential(conv_fn(Cin, k^2, ...), mask_act())` (None with v2=False) and `conv`, a DeformConv2d of our own under
    torchvision's parameter names and initialisation -- state_dict keys conv_offset.{weight,bias}, conv_mask.0.{weight,bias},
    conv.{weight,bias}.

    The reference's default cannot be constructed: it calls `mask_act(inplace=True)` and nn.Sigmoid takes no such argument
    (and torchvision, which its `conv` comes from, is not a dependency here).  This calls `mask_act(inplace=True)` and falls
    back to `mask_act()` on TypeError.  `mask_init_bias` is unused in the reference; it is accepted and unused here too.

    CPU tensors run plain torch in gather form (deform_conv2d above), with every argument the constructor accepts.  CUDA
    tensors run a launch list (Builder.deform_conv -> two conv units, vt_deform_fwd / vt_deform_bwd / vt_deform_wgrad):
    kernel_size 1 or 3, stride 1 or 2, groups = 1, in_channels and out_channels whole 16-byte chunks (8 in bf16, 4 in f32),
    `conv_fn` children that are nn.Conv2d of the matching geometry, mask_act Sigmoid or Identity; everything else raises
    NotImplementedError naming the argument.  d(x) leaves through float atomics, so a deterministic Builder refuses the block."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride: int = 1, padding: int = 0, dilation: int = 1,
                 groups: int = 1, bias: bool = True, conv_fn: Callable[..., nn.Module] = nn.Conv2d,
                 mask_act: Callable[..., nn.Module] = nn.Sigmoid, v2: bool = True, mask_init_bias: float = 0):
        super().__init__()
        num_locations = kernel_size ** 2 if isinstance(kernel_size, int) else kernel_size[0] * kernel_size[1]
        self.conv_offset = conv_fn(in_channels, 2 * num_locations, kernel_size, stride=stride, padding=padding, dilation=dilation)
        self.conv_mask = None
        if v2:
            try:
                act = mask_act(inplace=True)
            except TypeError:
                act = mask_act()
            self.conv_mask = nn.Sequential(
                conv_fn(in_channels, num_locations, kernel_size, stride=stride, padding=padding, dilation=dilation), act)
        self.conv = DeformConv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)

    def _vt_reserve(self) -> "dict[int, int]":
        """elements the slots of the offset / mask convolutions' parameters must hold in the flat store (ParamStore.ensure):
        their 2 k^2 and k^2 output channels run as the next whole 16-byte chunk over zero rows (ConvSpec.from_conv)"""
        out = {}
        for conv in (self.conv_offset, self.conv_mask[0] if self.conv_mask is not None else None):
            if isinstance(conv, nn.Conv2d) and conv.out_channels % 8:
                rows = -(-conv.out_channels // 8) * 8
                out[id(conv.weight)] = rows * conv.weight[0].numel()
                if conv.bias is not None:
                    out[id(conv.bias)] = rows
        return out

    def _vt_check(self, name: str) -> "tuple[int, int]":
        """(kernel_size, mask_act code) of the MI355X path, or NotImplementedError naming the argument it does not cover"""
        c = self.conv
        no = lambda what: NotImplementedError(f"{name}: DeformableConv2d with {what} -- the MI355X path runs kernel_size 1 or 3, "
                                              "stride 1 or 2, groups=1, conv_fn children that are nn.Conv2d and mask_act Sigmoid "
                                              "or Identity (CPU tensors run every geometry)")
        if c.kernel_size[0] != c.kernel_size[1] or c.kernel_size[0] not in (1, 3):
            raise no(f"kernel_size={c.kernel_size}")
        if c.stride[0] != c.stride[1] or c.stride[0] not in (1, 2):
            raise no(f"stride={c.stride}")
        if c.padding[0] != c.padding[1]:
            raise no(f"padding={c.padding}")
        if c.dilation[0] != c.dilation[1]:
            raise no(f"dilation={c.dilation}")
        if c.groups != 1:
            raise no(f"groups={c.groups}")
        code = 0
        convs = [("conv_offset", self.conv_offset, 2)]
        if self.conv_mask is not None:
            convs.append(("conv_mask.0", self.conv_mask[0], 1))
            act = self.conv_mask[1]
            if isinstance(act, nn.Sigmoid):
                code = 1
            elif not isinstance(act, nn.Identity):
                raise no(f"mask_act={type(act).__name__}")
        for cname, m, mult in convs:
            if type(m) is not nn.Conv2d:
                raise no(f"conv_fn={type(m).__name__} ({cname})")
            if (m.kernel_size != c.kernel_size or m.stride != c.stride or m.padding != c.padding or m.dilation != c.dilation or
                    m.groups != 1 or m.in_channels != c.in_channels or m.out_channels != mult * c.kernel_size[0] ** 2 or
                    m.padding_mode != "zeros"):
                raise no(f"conv_fn: {cname} is {m} (not the geometry of conv)")
        return c.kernel_size[0], code

    def _vt_emit(self, b, x, out=None, name: str = "dcn"):
        k, code = self._vt_check(name)
        return b.deform_conv(x, self.conv_offset, self.conv_mask[0] if self.conv_mask is not None else None, self.conv, code,
                             out=out, name=name)

    def _vt_emit_maps(self, b, x):
        return [self._vt_emit(b, x)]

    def _eager_maps(self, x: Tensor) -> "list[Tensor]":
        offset = self.conv_offset(x)
        mask = self.conv_mask(x) if self.conv_mask is not None else None
        return [self.conv(x, offset, mask)]


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
