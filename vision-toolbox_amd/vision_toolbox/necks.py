"""FPN / PAN / BiFPN necks on the backbone kernels.

Same constructors, child names (`lateral_convs`, `output_convs`, `top_down`, `bottom_up`; BiFPN: `laterals`,
`layers.{l}.td_fuses` / `out_fuses` / `last_out_fuse`, each with `.weights` and `.conv`) and
therefore the same state_dict keys as the reference (vision_toolbox/necks.py:45-215); `forward`
takes the list a backbone's `get_feature_maps()` returns (bottom = largest map first) and returns a
list of the same length.  Execution: one compiled launch list per (shapes, dtype, mode) --
biased 1x1 lateral convs and 3x3 ConvNormAct output convs on the implicit-GEMM kernels, and the
`nn.Upsample(nearest, x2 | x0.5)` + `sum` pair as ONE resampling kernel (vt_resample2x_add_fwd);
the whole neck is one autograd.Function, so it composes with the backbone's.

FPN / PAN run `fuse_fn` "sum" / "concat", nearest / bilinear interpolation and `ConvNormAct` blocks on the GPU.  Other
settings construct (state_dict parity) and raise NotImplementedError when run.

BiFPN: biased 1x1 lateral convs, then per layer 2 (levels - 1) fusion nodes.  A node is ONE launch
(Builder.weighted_fuse -> vt_wfuse_fwd: the ReLU of the learned weights, the normalisation by their sum and the nearest
x2 / x0.5 resampling of its 2 or 3 inputs happen inside it, no resampled or scaled map is stored) followed by the node's
block: `SeparableConv2d` (the default; tiled depthwise unit + 1x1 unit) or `ConvNormAct`.  `interpolation_mode="bilinear"`
materialises the resampled map with the resampling kernel first and fuses it at equal size.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _native as N
from . import engine as E
from .components import ConvNormAct, SeparableConv2d
from .program import Program, current_stream_handle, mode_signature, tracing_paused

__all__ = ["FPN", "PAN", "BiFPN"]

_FUSE = ("concat", "sum", "avg", "max")


class _NeckFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner: "_NeckRunner", prog: Program, n_in: int, *tensors):
        st, outs = runner._run_forward(prog, tensors[:n_in])
        ctx.runner, ctx.st, ctx.n_in, ctx.n_params = runner, st, n_in, len(tensors) - n_in
        ctx.in_meta = [(t.dtype, t.requires_grad) for t in tensors[:n_in]]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        dxs, pgrads = ctx.runner._run_backward(ctx.st, gouts, ctx.in_meta)
        ctx.st = None
        return (None, None, None, *dxs, *pgrads[: ctx.n_params])


class _NeckRunner:
    def __init__(self, module: nn.Module):
        self.module = module
        self.store = E.ParamStore(module)
        self.cache: dict = {}

    def program(self, xs: Sequence[Tensor], dtype: int, need_grad: bool) -> Program:
        key = (tuple(tuple(x.shape) for x in xs), dtype, need_grad,
               tuple(bool(x.requires_grad) for x in xs), self.store.version, mode_signature(self.module, self.store))
        prog = self.cache.get(key)
        if prog is None:
            b = E.Builder(self.store, dtype, self.module.training, need_grad)
            b.refresh_mirror()
            refs = [b.input_map(x.shape[0], x.shape[1], x.shape[2], x.shape[3], f"in{i}",
                                requires_grad=bool(x.requires_grad) and need_grad) for i, x in enumerate(xs)]
            outs = self.module._vt_emit_list(b, refs)
            seeds = []
            if need_grad:
                seeds = b.seed_output_grads(outs)
                b.build_backward()
            prog = Program(b, outs, seeds)
            prog.ext_inputs, prog.ext_grads = list(b.ext_inputs), list(b.ext_grads)
            self.cache[key] = prog
        return prog

    def __call__(self, xs: Sequence[Tensor]):
        xs = list(xs)
        if not xs or any((not isinstance(x, Tensor)) or x.dim() != 4 for x in xs):
            raise ValueError("expected a list of 4-D NCHW feature maps")
        if all(not x.is_cuda for x in xs):
            return self.module._eager_list(xs)  # dispatch rule: CPU tensors -> plain torch ops
        if any(not x.is_cuda for x in xs):
            raise RuntimeError("feature maps on different devices")
        N.lib()  # a GPU tensor never falls back to the eager path
        if len({x.dtype for x in xs}) != 1:
            raise ValueError("feature maps of one dtype expected")
        if xs[0].dtype == torch.bfloat16 or (torch.is_autocast_enabled() and
                                              torch.get_autocast_gpu_dtype() == torch.bfloat16):
            dtype = N.VT_BF16
        elif xs[0].dtype == torch.float32:
            dtype = N.VT_F32
        else:
            raise TypeError(f"feature maps must be float32 or bfloat16, got {xs[0].dtype}")
        with tracing_paused():
            self.store.ensure(xs[0].device)
            params = self.store.params
            need_grad = torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or
                                                     any(p.requires_grad for p in params))
            prog = self.program(xs, dtype, need_grad)
        if need_grad:
            outs = _NeckFn.apply(self, prog, len(xs), *xs, *params)
        else:
            _, outs = self._run_forward(prog, xs)
        return list(outs)

    def _run_forward(self, prog: Program, xs):
        dev = xs[0].device
        with torch.cuda.device(dev):
            arena = torch.empty(prog.arena_bytes, dtype=torch.uint8, device=dev)
            for ref, x in zip(prog.ext_inputs, xs):
                E.tref_to_tensor(arena, ref).copy_(x.detach())  # layout / dtype plumbing only
            s = self.store
            bases = prog.bases(arena.data_ptr(), PARAMS=s.pflat.data_ptr(), STATE=s.sflat.data_ptr(),
                               MIRROR=s.mirror.data_ptr(), COUNTERS=s.nflat.data_ptr())
            N.run_ops(prog.fwd_ops, prog.n_fwd, bases, current_stream_handle())
        outs = [E.tref_to_tensor(arena, t) for t in prog.outs]
        return (prog, arena, bases), outs

    def _run_backward(self, st, gouts, in_meta):
        prog, arena, bases = st
        if prog.n_bwd == 0:
            raise RuntimeError("this forward was compiled without a backward list (no-grad call)")
        with torch.cuda.device(arena.device):
            for seed, g in zip(prog.seeds, gouts):
                view = E.tref_to_tensor(arena, seed)
                if g is None:
                    view.zero_()
                else:
                    view.copy_(g)
            N.run_ops(prog.bwd_ops, prog.n_bwd, bases, current_stream_handle())
        dxs = []
        for gref, (dt, rg) in zip(prog.ext_grads, in_meta):
            if not rg or gref is None:
                dxs.append(None)
            else:
                dxs.append(E.tref_to_tensor(arena, gref).to(dt))
        zb = arena[prog.zb_off : prog.zb_off + prog.zb_bytes]
        pgrads = []
        for p in self.store.params:
            off = prog.param_grad_off.get(id(p))
            if off is None or not p.requires_grad:
                pgrads.append(None)
                continue
            g = zb[off : off + p.numel() * 4].view(torch.float32)
            if p.dim() == 4:
                o, i, kh, kw = p.shape
                g = g.view(o, kh, kw, i).permute(0, 3, 1, 2)
            else:
                g = g.view(p.shape)
            pgrads.append(g)
        return dxs, pgrads


class _NeckBase(nn.Module):
    _runner: Optional[_NeckRunner] = None

    def forward(self, x: "list[Tensor]") -> "list[Tensor]":
        r = self.__dict__.get("_runner")
        if r is None:
            r = _NeckRunner(self)
            self.__dict__["_runner"] = r
        return r(x)


# https://arxiv.org/abs/1612.03144
class FPN(_NeckBase):
    def __init__(
        self,
        in_channels_list: "list[int]",
        out_channels: int = 256,
        fuse_fn: str = "sum",
        block: Callable[[int, int], nn.Module] = ConvNormAct,
        interpolation_mode: str = "nearest",
        top_down: bool = True,
    ):
        super().__init__()
        if fuse_fn not in _FUSE:
            raise KeyError(fuse_fn)
        self.fuse_fn = fuse_fn
        self.interpolation_mode = interpolation_mode
        self.out_channels = out_channels
        self.top_down = top_down
        self.lateral_convs = nn.ModuleList(
            [nn.Conv2d(in_c, out_channels, kernel_size=1) if in_c != out_channels else nn.Identity()
             for in_c in in_channels_list]
        )
        self.upsample = nn.Upsample(scale_factor=2.0 if top_down else 0.5, mode=interpolation_mode)
        in_c = out_channels if fuse_fn == "sum" else out_channels * 2
        self.output_convs = nn.ModuleList([block(in_c, out_channels) for _ in range(len(in_channels_list) - 1)])

    def _vt_emit_list(self, b, xs, name: str = "fpn"):
        if self.fuse_fn not in ("sum", "concat") or self.interpolation_mode not in ("nearest", "bilinear"):
            # ('avg' / 'max' cannot run in the reference either: its output convs are built for 2 x out_channels whenever
            #  fuse_fn != 'sum', necks.py:66, while those two fuse functions return out_channels)
            raise NotImplementedError("the MI355X neck implements fuse_fn 'sum' / 'concat' with nearest / bilinear resampling")
        assert len(xs) == len(self.lateral_convs)
        outs = []
        for i, (lat, x) in enumerate(zip(self.lateral_convs, xs)):
            if isinstance(lat, nn.Identity):
                outs.append(x)
            else:
                outs.append(b.conv_unit(x, lat, None, False, name=f"{name}.lateral_convs.{i}"))
        n = len(outs)
        for i, oc in enumerate(self.output_convs):
            if not isinstance(oc, ConvNormAct):
                raise NotImplementedError("neck blocks other than ConvNormAct are outside the hot path")
            # top-down: levels n-2, ..., 0 receive the level above, upsampled (necks.py:70-73); bottom-up: levels 1, ..., n-1
            # the level below, subsampled (necks.py:76-79)
            dst, src = (n - 2 - i, n - 1 - i) if self.top_down else (i + 1, i)
            mode = (0 if self.top_down else 1) + (2 if self.interpolation_mode == "bilinear" else 0)
            if self.fuse_fn == "sum":
                fused = b.resample_add(outs[src], outs[dst], mode, name=f"{name}.fuse.{dst}")
            else:  # torch.cat([x_dst, resample(x_src)], dim=1) (necks.py:14-15): two channel slices of one buffer
                d = outs[dst]
                fused = b.act(d.B, d.H, d.W, 2 * d.C, f"{name}.cat.{dst}")
                b.copy(d, fused.sl(0, d.C))
                b.resample_add(outs[src], None, mode, name=f"{name}.fuse.{dst}", out=fused.sl(d.C, d.C))
            outs[dst] = oc._vt_emit(b, fused, name=f"{name}.output_convs.{i}")
        return outs

    def _eager_list(self, xs):
        """CPU tensors: the same wiring with torch ops over this module's children."""
        if self.fuse_fn not in ("sum", "concat"):
            raise NotImplementedError("fuse_fn 'sum' / 'concat' (the reference's 'avg' / 'max' cannot run there either)")
        assert len(xs) == len(self.lateral_convs)
        outs = [lat(x) for lat, x in zip(self.lateral_convs, xs)]
        n = len(outs)
        for i, oc in enumerate(self.output_convs):
            dst, src = (n - 2 - i, n - 1 - i) if self.top_down else (i + 1, i)
            up = self.upsample(outs[src])
            outs[dst] = oc(outs[dst] + up if self.fuse_fn == "sum" else torch.cat([outs[dst], up], dim=1))
        return outs


# https://arxiv.org/abs/1803.01534
class PAN(_NeckBase):
    def __init__(
        self,
        in_channels_list: "list[int]",
        out_channels: int = 256,
        fuse_fn: str = "sum",
        block: Callable[[int, int], nn.Module] = ConvNormAct,
        interpolation_mode: str = "nearest",
    ):
        super().__init__()
        self.top_down = FPN(in_channels_list, out_channels, fuse_fn=fuse_fn, block=block,
                            interpolation_mode=interpolation_mode)
        self.bottom_up = FPN([out_channels] * len(in_channels_list), out_channels, fuse_fn=fuse_fn, block=block,
                             interpolation_mode=interpolation_mode)

    def _vt_emit_list(self, b, xs, name: str = "pan"):
        return self.bottom_up._vt_emit_list(b, self.top_down._vt_emit_list(b, xs, name + ".top_down"),
                                            name + ".bottom_up")

    def _eager_list(self, xs):
        return self.bottom_up._eager_list(self.top_down._eager_list(xs))


# https://arxiv.org/pdf/1911.09070.pdf
_BIFPN_MODES = ("nearest", "bilinear")


def _bifpn_fuse(b, node: "WeightedFeatureFusion", xs, codes, interpolation_mode: str, name: str):
    """one fusion node on the launch list: the weighted fusion (one launch), then the node's block"""
    if interpolation_mode not in _BIFPN_MODES:
        raise NotImplementedError(f"{name}: interpolation_mode={interpolation_mode!r} -- the MI355X BiFPN implements "
                                  "'nearest' and 'bilinear'")
    if not isinstance(node.conv, (ConvNormAct, SeparableConv2d)):
        raise NotImplementedError(f"{name}.conv: block {type(node.conv).__name__} -- the MI355X BiFPN runs ConvNormAct and "
                                  "SeparableConv2d blocks")
    ins, cs = [], []
    for k, (x, c) in enumerate(zip(xs, codes)):
        if c and interpolation_mode == "bilinear":  # the fusion kernel resamples nearest only: materialise, fuse at equal size
            x, c = b.resample_add(x, None, 2 if c == 1 else 3, name=f"{name}.resample{k}"), 0
        ins.append(x)
        cs.append(c)
    fused = b.weighted_fuse(ins, cs, node.weights, node.eps, name=name)
    return node.conv._vt_emit(b, fused, name=name + ".conv")


class WeightedFeatureFusion(_NeckBase):
    def __init__(
        self,
        num_channels: int,
        num_inputs: int = 2,
        block: Callable[[int, int], nn.Module] = SeparableConv2d,
        eps: float = 1e-4,
    ):
        super().__init__()
        self.weights = nn.Parameter(torch.ones(num_inputs, dtype=torch.float))
        self.conv = block(num_channels, num_channels)
        self.eps = eps

    def forward(self, x: "list[Tensor]") -> Tensor:  # (equal-sized maps, as in the reference: the caller resamples)
        return super().forward(x)[0]

    def _vt_emit_list(self, b, xs, name: str = "fuse"):
        return [_bifpn_fuse(b, self, xs, [0] * len(xs), "nearest", name)]

    def _eager(self, xs) -> Tensor:
        weights = F.relu(self.weights)
        out = 0
        for i in range(weights.shape[0]):
            out = out + xs[i] * weights[i]
        return self.conv(out / (weights.sum() + self.eps))

    def _eager_list(self, xs):
        return [self._eager(xs)]


class BiFPNLayer(_NeckBase):
    def __init__(
        self,
        num_levels: int,
        num_channels: int,
        block: Callable[[int, int], nn.Module] = SeparableConv2d,
        interpolation_mode="nearest",
        eps: float = 1e-4,
    ):
        super().__init__()
        self.num_levels = num_levels
        self.interpolation_mode = interpolation_mode
        self.td_fuses = nn.ModuleList(
            [WeightedFeatureFusion(num_channels, block=block, eps=eps) for _ in range(num_levels - 1)]
        )
        self.out_fuses = nn.ModuleList(
            [WeightedFeatureFusion(num_channels, num_inputs=3, block=block, eps=eps) for _ in range(num_levels - 2)]
        )
        self.last_out_fuse = WeightedFeatureFusion(num_channels, block=block, eps=eps)
        self.upsample = nn.Upsample(scale_factor=2.0, mode=interpolation_mode)
        self.downsample = nn.Upsample(scale_factor=0.5, mode=interpolation_mode)

    def _check(self, xs):
        if self.num_levels < 2 or len(xs) != self.num_levels:
            raise ValueError(f"BiFPNLayer: {len(xs)} feature maps for {self.num_levels} levels (at least 2)")

    def _vt_emit_list(self, b, xs, name: str = "bifpn_layer"):
        self._check(xs)
        n, mode = self.num_levels, self.interpolation_mode
        # top-down: P6td = conv(fuse(P6in, up(P7td))) (necks.py:182-185)
        tds = list(xs)
        for i, node in enumerate(self.td_fuses):
            d = n - 2 - i
            tds[d] = _bifpn_fuse(b, node, [xs[d], tds[d + 1]], [0, 1], mode, f"{name}.td_fuses.{i}")
        # bottom-up: P4out = conv(fuse(P4in, P4td, down(P3td))) (necks.py:187-190); the top level has two inputs (:193)
        outs = list(tds)
        for i, node in enumerate(self.out_fuses):
            outs[i + 1] = _bifpn_fuse(b, node, [xs[i + 1], tds[i + 1], tds[i]], [0, 0, 2], mode, f"{name}.out_fuses.{i}")
        outs[-1] = _bifpn_fuse(b, self.last_out_fuse, [xs[-1], tds[-2]], [0, 2], mode, f"{name}.last_out_fuse")
        return outs

    def _eager_list(self, xs):
        self._check(xs)
        tds = list(xs)
        for i, node in enumerate(self.td_fuses):
            tds[-2 - i] = node._eager([xs[-2 - i], self.upsample(tds[-1 - i])])
        outs = list(tds)
        for i, node in enumerate(self.out_fuses):
            outs[i + 1] = node._eager([xs[i + 1], tds[i + 1], self.downsample(tds[i])])
        outs[-1] = self.last_out_fuse._eager([xs[-1], self.downsample(tds[-2])])
        return outs


# https://github.com/google/automl/blob/master/efficientdet/efficientdet_arch.py
class BiFPN(_NeckBase):
    def __init__(
        self,
        in_channels_list: "list[int]",
        out_channels: int = 64,
        num_layers: int = 1,
        block: Callable[[int, int], nn.Module] = SeparableConv2d,
        interpolation_mode="nearest",
        eps: float = 1e-4,
    ):
        super().__init__()
        self.out_channels = out_channels
        self.laterals = nn.ModuleList([nn.Conv2d(in_c, out_channels, kernel_size=1) for in_c in in_channels_list])
        self.layers = nn.ModuleList(
            [BiFPNLayer(len(in_channels_list), out_channels, block=block, interpolation_mode=interpolation_mode, eps=eps)
             for _ in range(num_layers)]
        )

    def _vt_emit_list(self, b, xs, name: str = "bifpn"):
        if len(xs) != len(self.laterals):
            raise ValueError(f"BiFPN: {len(xs)} feature maps for {len(self.laterals)} lateral convs")
        outs = [b.conv_unit(x, lat, None, False, name=f"{name}.laterals.{i}") for i, (lat, x) in enumerate(zip(self.laterals, xs))]
        for l, layer in enumerate(self.layers):
            outs = layer._vt_emit_list(b, outs, f"{name}.layers.{l}")
        return outs

    def _eager_list(self, xs):
        if len(xs) != len(self.laterals):
            raise ValueError(f"BiFPN: {len(xs)} feature maps for {len(self.laterals)} lateral convs")
        outs = [lat(x) for lat, x in zip(self.laterals, xs)]
        for layer in self.layers:
            outs = layer._eager_list(outs)
        return outs
