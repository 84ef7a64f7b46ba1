"""Static launch-list builder and runner for the backbone hot path.

The reference executes a backbone by walking nn.Sequential in Python and letting
ATen/autograd dispatch conv2d, batch_norm, relu_, cat, add one by one
(vision_toolbox/components.py:26-44, backbones/darknet.py:27-28,51-55,
backbones/vovnet.py:50-63).  Here a backbone is compiled ONCE per
(input shape, dtype, mode) into two flat lists of libvt_amd launches (forward,
backward) over one arena; a step is one call into the native executor
(vt_run_ops) or one hipGraph launch.  Backward is written out explicitly per
unit (no autograd inside), which is what allows concat elision, residual adds
folded into epilogues and gradient accumulation folded into the data-gradient
epilogue.

Only CUDA (HIP) tensors reach this module; CPU tensors are served by the modules' own
torch children (program.py dispatch rule) and never by these launch lists.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field, replace
from typing import Callable, Optional

import torch
from torch import nn

from . import _native as N

ALIGN = 256

# base ids (index into the `bases` array handed to vt_run_ops)
ARENA, PARAMS, GRADS, STATE, MIRROR, INPUT, COUNTERS, LABELS, MOMENTUM, HYPER, ZERO_F, ZERO_B, MOMENT2, OPTWS, EMA = range(15)
NUM_BASES = 15

_TORCH_DTYPE = {N.VT_F32: torch.float32, N.VT_BF16: torch.bfloat16}
_ESIZE = {N.VT_F32: 4, N.VT_BF16: 2}
_EPC = {N.VT_F32: 4, N.VT_BF16: 8}


def _round_up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


@dataclass(eq=False)
class Buf:
    base: int
    offset: int  # bytes from the base
    nbytes: int
    name: str = ""
    # the normalise pass that would write this activation has not been emitted (Builder.conv_unit(defer_norm=True)): the
    # buffer has no place in the arena yet.  TRef.addr() -- the one door every reader goes through -- emits it then.
    deferred: Optional["_DeferredNorm"] = None


@dataclass(eq=False)
class TRef:
    """NHWC activation, possibly a channel slice [coff, coff+C) of a wider buffer."""

    buf: Buf
    B: int
    H: int
    W: int
    C: int
    ld: int  # pixel stride, elements
    coff: int  # channel offset, elements
    dtype: int
    needs_grad: bool = True
    logical_C: Optional[int] = None  # channels before the padding to a 16-byte chunk (input_images); None: C.  Not inherited by sl()
    stem_out: bool = False  # written by the stem unit that recomputes z (conv_unit); not inherited by sl() either

    @property
    def logical_c(self) -> int:
        return self.C if self.logical_C is None else self.logical_C

    @property
    def M(self) -> int:
        return self.B * self.H * self.W

    @property
    def esize(self) -> int:
        return _ESIZE[self.dtype]

    def addr(self):
        if self.buf.deferred is not None:
            self.buf.deferred.materialise()
        return (self.buf.base, self.buf.offset + self.coff * self.esize)

    def sl(self, c0: int, c: int) -> "TRef":
        assert 0 <= c0 and c0 + c <= self.C
        return TRef(self.buf, self.B, self.H, self.W, c, self.ld, self.coff + c0, self.dtype, self.needs_grad)

    def same_geom(self, o: "TRef") -> bool:
        return (self.B, self.H, self.W, self.C) == (o.B, o.H, o.W, o.C)


class _PSlice:
    """Elements [start, start + n) of a parameter or buffer of the flat store: one group's rows of a grouped convolution's
    filter, its share of the bias and of the BatchNorm vectors (conv_unit, `groups > 1`)."""

    def __init__(self, base, start: int, n: int):
        self.base, self.start, self.n = base, int(start), int(n)
        self.requires_grad = bool(getattr(base, "requires_grad", False))

    def numel(self) -> int:
        return self.n


class ParamStore:
    """Flat f32 storage behind every parameter / buffer of a module tree.

    Parameters keep their identity, names and logical shapes (so state_dict keys and
    OIHW shapes are exactly the reference's, base.py:23-25), but their storage becomes
    a slice of one flat tensor; 4-D conv weights are held channels_last, i.e.
    physically [Cout][kh][kw][Cin], which is the filter image the kernels read.

    Non-persistent buffers (register_buffer(..., persistent=False)) of ANY module are left out: they get no slot, are not
    moved to the device and no launch may read them.  Today those are the index / mask tables of the Swin CPU path, which
    the window attention kernels recompute.  A launch that needs a buffer's values needs a persistent buffer.
    """

    def __init__(self, root: nn.Module, order_key=None):
        self.root = root
        self.order_key = order_key  # optional grouping of the flat layout (stable sort key per parameter)
        self.device = None
        self.pflat = self.sflat = self.nflat = self.mirror = None
        self.pad_multiple = 64  # the flat parameter buffer's length is a multiple of this (sharded exchange: 64 * world)
        # id(parameter) -> elements its slot must hold at least (zero beyond the parameter's own): a classifier head whose
        # class count is no multiple of a 16-byte chunk is run as the next wider one over zero rows (trainer.TrainStep)
        self.reserve: dict[int, int] = {}
        self.index: dict[int, tuple[int, int, int]] = {}  # id(tensor owner) -> (base, elem offset, numel)
        self.params: list[nn.Parameter] = []
        self._ptrs: list[tuple[torch.Tensor, int]] = []
        self.version = 0

    # -- layout ---------------------------------------------------------------
    def _collect(self):
        params, fbufs, ibufs, seen = [], [], [], set()
        for p in self.root.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                params.append(p)
        for mod in self.root.modules():
            for name, b in mod._buffers.items():
                if b is None or id(b) in seen:
                    continue
                if name in mod._non_persistent_buffers_set:
                    continue  # derived index / mask tables of the CPU path (Swin): no launch reads them, they stay as they are
                seen.add(id(b))
                (fbufs if b.is_floating_point() else ibufs).append((mod, name, b))
        if self.order_key is not None:
            params.sort(key=self.order_key)  # stable: registration order inside each group
        return params, fbufs, ibufs

    def stale(self, device) -> bool:
        if self.device != device or self.pflat is None:
            return True
        for t, ptr in self._ptrs:
            if t.data_ptr() != ptr or t.dtype not in (torch.float32, torch.int64):
                return True
        params, fbufs, ibufs = self._collect()
        return len(params) + len(fbufs) + len(ibufs) != len(self._ptrs)

    def ensure(self, device) -> None:
        if not self.stale(device):
            return
        params, fbufs, ibufs = self._collect()
        for p in params:
            if not p.is_floating_point():
                raise TypeError("non floating point parameter")
        for mod in self.root.modules():  # (DeformableConv2d: its offset / mask convolutions run over zero rows up to a chunk)
            want = getattr(mod, "_vt_reserve", None)
            if want is not None:
                self.reserve.update(want())
        offs, slots, total = [], [], 0
        for p in params:
            offs.append(total)
            slots.append(_round_up(max(p.numel(), self.reserve.get(id(p), 0)), 64))
            total += slots[-1]
        self.total = total  # elements that belong to parameters (the rest of pflat is padding)
        pflat = torch.zeros(_round_up(max(total, 64), self.pad_multiple), dtype=torch.float32, device=device)
        soffs, stotal = [], 0
        for _, _, b in fbufs:
            soffs.append(stotal)
            stotal += _round_up(b.numel(), 64)
        sflat = torch.zeros(max(stotal, 64), dtype=torch.float32, device=device)
        nflat = torch.zeros(max(len(ibufs), 1) * 2, dtype=torch.int64, device=device)
        self.index.clear()
        self._ptrs = []
        with torch.no_grad():
            for p, off in zip(params, offs):
                n = p.numel()
                seg = pflat[off : off + n]
                if p.dim() == 4:
                    o, i, kh, kw = p.shape
                    view = seg.view(o, kh, kw, i).permute(0, 3, 1, 2)
                else:
                    view = seg.view(p.shape)
                view.copy_(p.data.to(device=device, dtype=torch.float32))
                p.data = view
                self.index[id(p)] = (PARAMS, off, n)
                self._ptrs.append((p, p.data_ptr()))
            for (mod, name, b), off in zip(fbufs, soffs):
                n = b.numel()
                view = sflat[off : off + n].view(b.shape)
                view.copy_(b.to(device=device, dtype=torch.float32))
                mod._buffers[name] = view
                self.index[id(view)] = (STATE, off, n)
                self._ptrs.append((view, view.data_ptr()))
            for k, (mod, name, b) in enumerate(ibufs):
                view = nflat[2 * k : 2 * k + 1].view(b.shape)
                view.copy_(b.to(device=device, dtype=torch.int64))
                mod._buffers[name] = view
                self.index[id(view)] = (COUNTERS, 2 * k, 1)
                self._ptrs.append((view, view.data_ptr()))
        self.params, self.offsets, self.slots = params, offs, slots
        self.pflat, self.sflat, self.nflat = pflat, sflat, nflat
        self.mirror = torch.zeros(pflat.numel(), dtype=torch.bfloat16, device=device)
        self.device = device
        self.version += 1

    def where(self, t) -> tuple[int, int, int]:
        if isinstance(t, _PSlice):
            base, off, _ = self.index[id(t.base)]
            return base, off + t.start, t.n
        return self.index[id(t)]

    def param_signature(self):
        return tuple(p._version for p in self.params)


# -- what Builder.conv_unit is told about a layer -------------------------------------------
@dataclass(frozen=True, eq=False)
class ConvSpec:
    """A conv-like layer as conv_unit sees it: a square nn.Conv2d, one group of a grouped one, or an nn.Linear as a 1x1
    convolution over a [B,1,1,C] map (classifier.py:63).  `weight` / `bias` are parameters, or _PSlice views of them
    (`is_slice`)."""

    k: int
    stride: int
    padding: int
    dilation: int
    groups: int
    in_channels: int
    out_channels: int
    weight: object
    bias: object = None
    is_slice: bool = False
    crop: int = 0  # output rows / columns left out at the far edge (Builder.stem7_unit: a window that is not centred)

    def __post_init__(self):
        if self.dilation * (self.k - 1) > 127:
            raise NotImplementedError(f"dilation {self.dilation}: tap offsets are 8-bit")

    @classmethod
    def from_conv(cls, conv: nn.Conv2d, out_channels: Optional[int] = None) -> "ConvSpec":
        """(out_channels > conv.out_channels: the filter rows and bias entries beyond the parameters' own are zeros their
        slots of the flat store reserve, as with from_linear)"""
        ks, st, dl, pd = conv.kernel_size, conv.stride, conv.dilation, conv.padding
        if ks[0] != ks[1] or st[0] != st[1] or dl[0] != dl[1] or pd[0] != pd[1]:
            raise NotImplementedError("hot path covers square convolutions (kernel, stride, dilation, padding)")
        return cls(ks[0], st[0], pd[0], dl[0], conv.groups, conv.in_channels, out_channels or conv.out_channels, conv.weight,
                   conv.bias)

    @classmethod
    def from_linear(cls, linear: nn.Linear, out_channels: Optional[int] = None) -> "ConvSpec":
        """(out_channels > out_features: the rows beyond the parameter's own are zeros its slot of the flat store reserves)"""
        return cls(1, 1, 0, 1, 1, linear.in_features, out_channels or linear.out_features, linear.weight, linear.bias)

    def group(self, g: int) -> "ConvSpec":
        """group g of a grouped convolution: its rows of the [Cout][kh][kw][Cin / G] filter image, its share of the bias"""
        ci, co = self.in_channels // self.groups, self.out_channels // self.groups
        wn = co * self.k * self.k * ci
        return replace(self, groups=1, in_channels=ci, out_channels=co, weight=_PSlice(self.weight, g * wn, wn),
                       bias=_PSlice(self.bias, g * co, co) if self.bias is not None else None, is_slice=True)

    def without_bias(self) -> "ConvSpec":
        return replace(self, bias=None)

    def out_size(self, H: int, W: int) -> "tuple[int, int]":
        reach = 2 * self.padding - self.dilation * (self.k - 1) - 1
        return (H + reach) // self.stride + 1 - self.crop, (W + reach) // self.stride + 1 - self.crop


@dataclass(frozen=True, eq=False)
class BNSpec:
    """An nn.BatchNorm2d (default variant: affine, running statistics, a momentum), or one group's slice of it."""

    weight: object
    bias: object
    running_mean: object
    running_var: object
    num_batches_tracked: object
    eps: float
    momentum: float
    training: bool

    @classmethod
    def from_bn(cls, bn: nn.BatchNorm2d) -> "BNSpec":
        if bn.momentum is None or not bn.affine or not bn.track_running_stats:
            raise NotImplementedError("BatchNorm2d variants other than the default are outside the hot path")
        return cls(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum,
                   bool(bn.training))

    def group(self, g: int, G: int) -> "BNSpec":
        co = self.weight.numel() // G
        sl = lambda t: _PSlice(t, g * co, co)
        # (the batch counter belongs to the module, not to a group: the first group's finalize advances it)
        return replace(self, weight=sl(self.weight), bias=sl(self.bias), running_mean=sl(self.running_mean),
                       running_var=sl(self.running_var), num_batches_tracked=self.num_batches_tracked if g == 0 else None)


def _addr(t: "Optional[TRef]"):
    return t.addr() if t is not None else None


def _ld(t: "Optional[TRef]") -> int:
    return t.ld if t is not None else 0


# ---------------------------------------------------------------------------------------
# gradient bookkeeping (per forward buffer)
# ---------------------------------------------------------------------------------------
@dataclass
class _GradState:
    gbuf: Optional[Buf] = None
    init: list = field(default_factory=list)  # initialised channel intervals [c0, c1) in buffer coords
    pending: list = field(default_factory=list)  # (c0, c1, TRef addend)
    # the BatchNorm-backward sums of the unit that produced the forward buffer, formed by the launch that wrote the whole
    # gradient (pw_units with a producer operand); Builder.grad_dirty forgets them when anything else writes the gradient
    bn_sums: Optional[Buf] = None

    def covered(self, c0: int, c1: int) -> bool:
        pos = c0
        for a, b in sorted(self.init):
            if a > pos:
                break
            pos = max(pos, b)
        return pos >= c1

    def touches(self, c0: int, c1: int) -> bool:
        return any(a < c1 and c0 < b for a, b in self.init)


class _BNEmitter:
    """The BatchNorm of one unit inside a Builder: parameter addresses resolved once, the coefficient buffer
    (scale | shift | mean | invstd, C floats each) and the launches every BatchNorm unit shares.  `cp`: the four
    coefficient pointers where the caller owns the buffer (pw_units: one buffer over all groups' channels)."""

    def __init__(self, b: "Builder", spec: BNSpec, C_: int, cp=None):
        self.b, self.spec, self.C = b, spec, C_
        if cp is None:
            coef = b.f32(4 * C_, "bncoef")
            cp = [b.bp(coef, i * C_ * 4) for i in range(4)]
        self.cp = cp
        self.params = [b.pref(spec.weight), b.pref(spec.bias), b.pref(spec.running_mean), b.pref(spec.running_var)]
        self.nbt = b.pref(spec.num_batches_tracked) if spec.num_batches_tracked is not None else None

    def grads(self):
        """gradient accumulators of (weight, bias); resolved when a backward op is emitted (they may be allocated then)"""
        return [self.b.pgrad(self.spec.weight), self.b.pgrad(self.spec.bias)]

    def finalize_operands(self, stats: Buf, M: int):
        """(pointers, floats) of the finalize step: batch statistics -> coefficients and running statistics"""
        return ([self.b.bp(stats), *self.params, self.nbt, *self.cp],
                [M * self.b.bn_world, self.spec.eps, self.spec.momentum])

    def finalize(self, stats: Buf, M: int):
        ptrs, flts = self.finalize_operands(stats, M)
        self.b.emit(N.OP_BN_FINALIZE, ptrs, [self.C], flts)

    def eval_coeffs(self, scale_shift_only: bool = False):
        """coefficients from the running statistics"""
        cp = self.cp[:2] + [None, None] if scale_shift_only else self.cp
        self.b.emit(N.OP_BN_EVAL_COEFFS, [*self.params, *cp], [self.C], [self.spec.eps])

    def bwd_buffers(self, y: TRef, dz_name: str):
        """(sums, coefficients, dz) of the unit's backward, in the order every program has allocated them"""
        b = self.b
        sums = b.zeroed_f32(N.stat_floats(self.C), "bwdsums")
        return sums, b.f32(3 * self.C, "bwdcoef"), b.act(y.B, y.H, y.W, self.C, dz_name)

    def bwd_reduce(self, g: TRef, z: TRef, act: int, sums: Buf, M: int, taps=None):
        self.b.emit(N.OP_BN_BWD_REDUCE, [g.addr(), z.addr(), *self.cp, self.b.bp(sums)] + ([taps[0]] if taps else []),
                    [g.ld, z.ld, self.C, int(act), self.b.dtype] + (taps[1] if taps else []), [M])

    def bwd_finalize(self, sums: Buf, bcoef: Buf, M: int):
        b, cp = self.b, self.cp
        b.emit(N.OP_BN_BWD_FINALIZE, [b.bp(sums), cp[0], cp[2], cp[3], *self.grads(), b.bp(bcoef)],
               [self.C, int(self.spec.training)], [M * b.bn_world, 1.0 / b.bn_world])

    def bwd_three_launches(self, g: TRef, z: TRef, act: int, sums: Buf, bcoef: Buf, dz: TRef, taps=None, reduce: bool = True):
        """reduce -> finalize -> apply.  `taps` = (arg-max address, [B, Ho, Wo]): g is the gradient of the unit's fused
        max pool; reduce=False: the sums were formed by the launch that produced g."""
        if reduce:
            self.bwd_reduce(g, z, act, sums, dz.M, taps)
        self.bwd_finalize(sums, bcoef, dz.M)
        self.b._act_bwd(g, z, self.cp[0], self.cp[1], self.b.bp(bcoef), dz, act, taps)


@dataclass(eq=False)
class _ConvUnit:
    """What the forward half of Builder.conv_unit decided about one unit; its backward works from this record."""

    conv: ConvSpec
    relu: int  # activation code
    x: TRef
    y: TRef
    residual: Optional[TRef]
    name: str
    tag: int
    wptr: tuple  # the filter operand ...
    wpack: Optional[Buf]  # ... which is this zero-padded copy for the stem
    ldw: int
    z: Optional[TRef] = None  # stored pre-activation (None: the unit has none, or recomputes it)
    bn: Optional[_BNEmitter] = None
    stem_fused: bool = False  # one-pass stem backward (vt_stem_bwd.hip) ...
    stem_y: bool = False  # ... working from y: z is never stored
    pool_out: Optional[TRef] = None  # max pool fused into the normalise pass ...
    pool_am: Optional[Buf] = None  # ... and its arg-max taps
    wg_key: Optional[tuple] = None  # shape group of held-back filter gradients
    defer: bool = False  # the normalise pass is held back (_DeferredNorm)
    pre_act: bool = False  # the residual joins BEFORE the activation: y = relu(bn(conv) + residual) (vt_resnet.hip)
    stem7: bool = False  # the 7x7 stride-2 stem as a 4x4 convolution over the space-to-depth image (Builder.stem7_unit)
    keep: Optional[tuple] = None  # row of the keep table: y = keep[b] * act(bn(conv)) + residual (vt_mbconv.hip)

    @property
    def padded(self) -> bool:
        return self.wpack is not None


class _DeferredNorm:
    """A training-mode BatchNorm unit whose normalise pass y = act(z * scale + shift) was held back: its only reader may be
    a pointwise launch that applies the pass to z as it loads it (Builder.pw_units, vt_pw_desc::pcoef), and then neither
    the pass nor y exists.  Any OTHER reader -- a unit, a returned feature map, a shortcut, a filter gradient -- asks for
    y's address, and that request (TRef.addr) materialises y here: the buffer gets its place in the arena and the ordinary
    normalise pass is emitted in front of the op being built."""

    def __init__(self, b: "Builder", u: "_ConvUnit", stats: Buf):
        self.b, self.u, self.stats = b, u, stats
        self.finalized = False  # a folding pw_stats launch has finalized the statistics (coefficients, running statistics)

    def materialise(self) -> None:
        b, u = self.b, self.u
        y, z, buf = u.y, u.z, u.y.buf
        if b._cur is not b.fwd:
            raise RuntimeError(f"{u.name}: the deferred output is first read outside the forward list")
        buf.deferred = None
        buf.offset = b.arena_top
        b.arena_top = _round_up(buf.offset + max(buf.nbytes, 1), ALIGN)
        tag, b.tag = b.tag, u.tag
        if self.finalized:
            b._act_apply(z, u.bn.cp[0], u.bn.cp[1], None, y, u.relu)
        else:
            ptrs, flts = u.bn.finalize_operands(self.stats, y.M)
            b.emit(N.OP_BN_FIN_APPLY, ptrs + [z.addr(), None, y.addr()], [y.C, z.ld, 0, y.ld, u.relu, b.dtype], flts + [y.M])
        b.tag = tag


class Builder:
    """Emits the forward / backward launch lists of one model instance."""

    def __init__(self, store: ParamStore, dtype: int, training: bool, need_grad: bool,
                 grad_base: int = ARENA, master_mirror_fresh: bool = False, deterministic: Optional[bool] = None):
        self.store = store
        self.dtype = dtype
        self.training = training
        self.need_grad = need_grad
        self.grad_base = grad_base
        self.fwd: list[N.Op] = []
        self.bwd: list[N.Op] = []
        self._cur = self.fwd
        self.arena_top = 0
        # scratch that must be zero before the forward / backward list runs lives in two
        # contiguous regions (own base ids), so each list needs ONE memset
        self.zf_top = self.zb_top = 0
        self.nodes: list[Callable[[], None]] = []  # backward emitters, forward order
        self.gstate: dict[int, _GradState] = {}
        self.param_grad_off: dict[int, int] = {}  # id(param) -> byte offset in grad base
        self.pgrad_bytes = 0
        self.tag = 0
        self.n_units = 0
        self.debug_refs: dict[str, TRef] = {}
        # the fused trainer sets this: the repacked data-gradient filters depend only on the
        # weights, so their (tiny, launch-bound) pack kernels leave the backward critical path
        # and run on the side stream while the forward list executes
        self.hoist_dgrad_packs = False
        # Schedule and decomposition choices, each the winner of an alternating A/B inside the train step (NOTEBOOK.md):
        #  * a unit's filter gradient is released to the side stream BEFORE its data gradient (after it for every unit:
        #    22.20 vs 21.27 ms) -- except for the unit that reads the stem's output: its data gradient, its filter gradient
        #    and the stem's one-pass backward are the HBM-bound tail of a step, and released after the data gradient the
        #    filter gradient runs beside the stem's backward instead (21.41 -> 21.27 ms);
        #  * stem unit (3 -> 32, s1): BatchNorm-backward reduction and filter gradient in one pass, dz never formed, and
        #    its pre-activation z (B x 224 x 224 x 32, the largest tensor of a step) never stored: the conv runs twice
        #    (statistics only, then with the normalise + ReLU epilogue) and backward works from y (vt_stem_bwd.hip);
        #  * 3x3 stride-2 data gradients whose dz has at most 128 channels (the HBM-bound ones) run as ONE depth-to-space
        #    launch instead of four parity-class launches that each re-read dz (256: 21.90 vs 21.70 ms).
        self.dgrad_d2s_maxc = 128
        # deterministic mode: the last sums still made with f32 atomics take an order-free form -- the filter gradients
        # become two-stage (partial tiles stored into slabs of ONE scratch that every layer reuses, then an ordered
        # reducer), the bias column sums and the one-pass stem kernel's correlations go through fixed point; with
        # the fixed-point BatchNorm statistics every gradient and parameter update is then bit-identical from run to run
        self.deterministic = (os.environ.get("VT_DETERMINISTIC", "0") != "0") if deterministic is None else bool(deterministic)
        self.wgrad_slab_mb = 48 if self.deterministic else 0  # 0 = atomics
        self._wgrad_slab = None
        # 1x1 ConvNormAct units as four streaming passes that recompute z = W x instead of storing z and dz
        # (vt_pointwise.hip); off in deterministic mode (its filter gradient leaves through float atomics)
        self.pointwise = not self.deterministic
        # ... where the unit's input is at least this many MB: smaller tensors stay in the memory-side cache between the
        # passes of the unfused path, which is then as fast (measured at batch 256, CSPDarknet-53: 22.40 ms with the 51 MB
        # tensors of stage 2 included, 22.11 without; 23.32 with the pointwise path off).  VT_PW_MIN_MB (the tests set 0:
        # their toy tensors would otherwise never reach these kernels)
        self.pointwise_min_mb = float(os.environ.get("VT_PW_MIN_MB", "80"))
        # A pointwise launch that is the ONLY reader of a BatchNorm unit's output takes over that unit's normalise pass: it
        # reads the stored pre-activation and applies scale, shift and ReLU as it loads (vt_pw_desc::pcoef), so the pass and
        # its output tensor disappear (CSPDarknetStage.conv -> conv1 | conv2 of stage 0).  Only where the producer's tensor
        # has at least this many MB -- below what the memory-side cache holds the saved pass is a cache hit, as above.
        # VT_PW_FOLD_MIN_MB (tests of the fold set 0); never in deterministic mode (the pointwise path is off there).
        self.pw_fold_min_mb = float(os.environ.get("VT_PW_FOLD_MIN_MB", "80"))
        # ... and, where its backward launch is the only writer of the producer's d(y), the producer's BatchNorm-backward
        # reduction too (vt_pw_desc::psums).  VT_PW_FOLD_BNRED=0: the separate reduction pass.
        self.pw_fold_bnred = os.environ.get("VT_PW_FOLD_BNRED", "1") != "0"
        self._hoisted: list[N.Op] = []
        # Filter gradients of same-shape stride-1 3x3 layers (the DarknetBlock.conv2 units of a stage, darknet.py:23-24;
        # an OSA chain, vovnet.py:41-44) are HELD BACK in backward and released together, as consecutive ops that the
        # executor hands to vt_conv_wgrad_group in launches of <= wgrad_group layers: the CU-owning kernel
        # (vt_wgrad6.hip) then pays its prologue and its f32 atomic flush once per launch (isolated, batch 256:
        # 128 -> 128 @28x28 96 us per layer alone, 64 us in a group of 8; the kernel it replaces: 118 us).  Nothing reads a
        # filter gradient before the optimiser (or the bucket all-reduce, which is cut behind the op that completes the
        # bucket), and the arena keeps every x / dz.  VT_WGRAD_GROUP=1: one layer per launch.
        self.wgrad_group = max(1, min(8, int(os.environ.get("VT_WGRAD_GROUP", "8"))))
        # the 1x1 units' filter gradients held back and grouped too?  Off: 8 layers in one launch of the general kernel are
        # cheaper alone (one atomic flush), but released at the end of a stage they no longer run beside their own units'
        # BatchNorm passes: step 20.31 -> 20.43 ms (NOTEBOOK R5.18).  VT_WGRAD_GROUP_1X1=1 turns it on.
        self.wgrad_group_1x1 = os.environ.get("VT_WGRAD_GROUP_1X1", "0") == "1"
        # ... on the side stream (0) or in line on the main stream (1): the CU-owning kernel shares nothing with the
        # kernels beside it (12 waves x 168 registers, 104 KiB of LDS), so the side stream buys it no overlap
        self.wgrad_inline = os.environ.get("VT_WGRAD_INLINE", "0") != "0"
        # Round 6: a 3x3 stride-1 data gradient that is the ONLY contribution to the gradient of a ConvNormAct unit's
        # output also reduces that unit's BatchNorm backward (vt_conv_dgrad_bnred): the separate reduction pass over
        # d(y) and z disappears (DarknetBlock.conv1 <- conv2, darknet.py:23-28: 23 units of CSPDarknet-53).  The last
        # whole-tensor data-gradient op per gradient buffer is remembered here; any other writer forgets it.
        # VT_FUSE_BNRED=0: the separate passes everywhere.
        # (off by default: the fused epilogue waits for z four times per tile -- 91 us against 66 + 19.5 for the two launches
        #  at 128 channels @28x28, step +0.10 ms; NOTEBOOK R6.4.  VT_FUSE_BNRED=1 turns it on.)
        self.fuse_bnred = os.environ.get("VT_FUSE_BNRED", "0") != "0"
        # BatchNorm backward of a unit as ONE launch (vt_bn_act_bwd_fused: the operands stay in registers between the
        # reduction and the apply pass; the library falls back to the three launches where they do not fit).  Not with
        # SyncBatchNorm (the sums are exchanged between the passes).  OFF by default: alone it equals the three launches
        # (32.5 against 30.8 us at 256 channels @14x14: two grid barriers of ~5 us each eat what the second read costs) and
        # in the step it is 0.3 ms SLOWER -- a launch that owns every CU's register file shares nothing with the
        # filter-gradient stream beside it (NOTEBOOK R6.5).  VT_BN_BWD_FUSED=1 turns it on.
        self.bn_bwd_fused = os.environ.get("VT_BN_BWD_FUSED", "0") != "0"
        self._last_dgrad: dict[int, tuple] = {}  # id(gradient Buf) -> (op, c0, c1)
        # The finalize launches folded into the streaming launches that consume their coefficients (vt_bn_finalize_apply,
        # vt_bn_bwd_finalize_apply): every workgroup of the pass finalizes the channels of its own channel group from the
        # (complete) sums -- nothing is handed over inside the launch -- and the single-workgroup finalize launch between a
        # producer of statistics and its consumer disappears: 114 of the 134 of a CSPDarknet-53 step, 132 with the pointwise
        # passes (pw_units); same-box 20.36 -> 19.79 ms (NOTEBOOK R6.10).  Bit-identical.  Not with SyncBatchNorm (the statistics are exchanged in front of the finalize).
        # VT_BN_FIN_APPLY=0 keeps the separate launches.  (The first form -- the first workgroups finalize and publish, all
        # others poll -- measured 2.3 ms SLOWER, R6.6.)
        self.bn_fin_apply = os.environ.get("VT_BN_FIN_APPLY", "1") != "0"
        # (A third form -- the finalize step as the TAIL of the launch that produces the sums: every workgroup takes a ticket,
        # the last one finalizes, nobody waits -- was bit-identical and NO faster than the launch it replaced, and its unused code
        # at the end of the MFMA kernel cost 0.09 ms per step: removed, NOTEBOOK R6.10.)
        self._wg_expect: dict[tuple, int] = {}   # shape key -> units seen in forward and not yet released
        self._wg_pending: dict[tuple, list] = {}  # shape key -> [(x addr, dz addr, dw addr, desc, ldw)]
        # SyncBatchNorm (configs/base.yaml:22): the trainer all-reduces every layer's statistics
        # between the kernel that accumulates them and the finalize kernel; the finalize kernels
        # are then told the GLOBAL sample count (and scale the affine gradients by 1/world)
        self.bn_world = 1
        self.bn_sync = False  # SyncBatchNorm: the sums are exchanged in front of every finalize step, which stays a launch of its own
        # feature-map inputs of programs that do not start from an image (necks): the runner copies
        # the caller's tensors into these buffers before the forward list and reads their gradients
        # (ext_grads, filled by build_backward) after the backward list
        self.ext_inputs: list[TRef] = []
        self.ext_grads: list[Optional[TRef]] = []
        self.input_grad: Optional[Buf] = None  # NCHW f32 gradient of the images (input_images(requires_grad=True))
        self._deferred_flush: Optional[TRef] = None  # grad_target -> grad_written
        self._tok_slabs: dict[int, Buf] = {}  # _token_slab
        self._attn_scratch: dict[int, Buf] = {}  # attention: the backward's delta, per size
        self._win_scratch: dict[int, Buf] = {}  # window attention: the per-window shares of the table gradient, per size
        self._talk_scratch: dict[int, Buf] = {}  # talking-heads attention: delta and the parameter-gradient shares, per size
        self._dw3_scratch: dict[int, Buf] = {}  # depthwise 3x3 + GELU + pool: the per-image filter-gradient shares, per size
        self._gconv_scratch: dict[int, Buf] = {}  # grouped 3x3: the filter gradient's slabs, per size
        self._dwt_scratch: dict[int, Buf] = {}  # tiled depthwise: the filter-gradient shares of the bands, per size
        self._deform_scratch: dict[int, Buf] = {}  # deformable convolution: the filter gradient's slabs / the d(x) plane, per size
        # stochastic depth ("row" mode): float[n_sites][B] keep factors, one row per residual block in emission order.  The
        # region is written OUTSIDE the launch lists before every forward (BackboneRunner, TrainStep), as `mix` in the HYPER
        # buffer is, so captured graphs stay valid; the arena never reuses it, so the backward reads what the forward read.
        self.keep_buf: Optional[Buf] = None
        self.keep_rates: "tuple[float, ...]" = ()  # drop probability of every site
        self.keep_B = 0

    # -- memory -----------------------------------------------------------------
    def alloc(self, nbytes: int, name: str = "") -> Buf:
        off = self.arena_top
        self.arena_top = _round_up(off + max(nbytes, 1), ALIGN)
        return Buf(ARENA, off, nbytes, name)

    def act(self, B, H, W, C, name="", needs_grad=True) -> TRef:
        buf = self.alloc(B * H * W * C * _ESIZE[self.dtype], name)
        t = TRef(buf, B, H, W, C, C, 0, self.dtype, needs_grad)
        if name:
            self.debug_refs[name] = t  # name -> activation, for tools/debug_*.py
        return t

    def debug_grad_ref(self, name: str) -> Optional[TRef]:
        """the gradient buffer mirroring activation `name` (None if never allocated)."""
        t = self.debug_refs.get(name)
        gs = self.gstate.get(id(t.buf)) if t is not None else None
        if gs is None or gs.gbuf is None:
            return None
        return TRef(gs.gbuf, t.B, t.H, t.W, t.C, t.ld, t.coff, t.dtype)

    def f32(self, n: int, name="") -> Buf:
        return self.alloc(n * 4, name)

    def keep_table(self, rates, B: int) -> list:
        """reserve the keep table of a program -- one float[B] row per residual block with drop probability rates[i] -- and
        return the rows' addresses, the `keep` operand of conv_unit.  Whoever runs the program fills the table before each
        forward: bernoulli(1 - p) / (1 - p) per site and image, or the values the user set."""
        assert self.keep_buf is None, "one keep table per program"
        self.keep_rates, self.keep_B = tuple(float(p) for p in rates), int(B)
        if not all(0.0 <= p < 1.0 for p in self.keep_rates):
            raise ValueError(f"stochastic-depth rates must lie in [0, 1): {self.keep_rates}")
        self.keep_buf = self.alloc(len(self.keep_rates) * B * 4, "keep")
        return [self.bp(self.keep_buf, i * B * 4) for i in range(len(self.keep_rates))]

    def zeroed_f32(self, n: int, name="", bwd: Optional[bool] = None) -> Buf:
        """f32 scratch zeroed once per run of the list being built (stats / reduction sums)."""
        if bwd is None:
            bwd = self._cur is self.bwd
        nbytes = _round_up(n * 4, ALIGN)
        if bwd:
            buf = Buf(ZERO_B, self.zb_top, n * 4, name)
            self.zb_top += nbytes
        else:
            buf = Buf(ZERO_F, self.zf_top, n * 4, name)
            self.zf_top += nbytes
        return buf

    # -- op emission --------------------------------------------------------------
    def emit(self, kind: int, ptrs=(), ints=(), flts=(), desc: Optional[N.ConvDesc] = None, extra_ints=(),
             side: bool = False):
        op = N.Op()
        op.kind = kind | (N.OP_SIDE_STREAM if side else 0)
        op.tag = self.tag
        for k in range(N.VT_OP_MAX_PTR):
            op.ptr[k].base = -1
        for k, p in enumerate(ptrs):
            if p is not None:
                op.ptr[k].base, op.ptr[k].offset = p
        if desc is not None:
            C.memmove(C.addressof(op.i), C.addressof(desc), C.sizeof(desc))
            k0 = C.sizeof(desc) // 4
            for k, v in enumerate(extra_ints):
                op.i[k0 + k] = int(v)
        else:
            for k, v in enumerate(ints):
                op.i[k] = int(v)
        for k, v in enumerate(flts):
            op.f[k] = float(v)
        self._cur.append(op)
        return op

    @staticmethod
    def bp(buf: Buf, byte_off: int = 0):
        return (buf.base, buf.offset + byte_off)

    # -- parameters ---------------------------------------------------------------
    def pref(self, t, mirror: bool = False):
        """address of a parameter or buffer of the flat store (None -> None: an operand the layer does not have)"""
        if t is None:
            return None
        base, off, n = self.store.where(t)
        if mirror:
            assert base == PARAMS
            return (MIRROR, off * 2)
        return (base, off * (8 if base == COUNTERS else 4))

    def pgrad(self, p: nn.Parameter):
        """address of the f32 gradient accumulator of parameter p (None if it needs none)."""
        if p is None or not p.requires_grad:
            return None
        if isinstance(p, _PSlice):
            a = self.pgrad(p.base)
            return (a[0], a[1] + 4 * p.start)
        if self.grad_base == GRADS:
            _, off, _ = self.store.where(p)
            return (GRADS, off * 4)
        key = id(p)
        if key not in self.param_grad_off:
            buf = self.zeroed_f32(max(p.numel(), self.store.reserve.get(key, 0)), "pgrad", bwd=True)
            self.param_grad_off[key] = buf.offset
        return (ZERO_B, self.param_grad_off[key])

    # -- gradient bookkeeping -------------------------------------------------------
    def _gs(self, t: TRef) -> _GradState:
        return self.gstate.setdefault(id(t.buf), _GradState())

    def _gref(self, t: TRef) -> TRef:
        gs = self._gs(t)
        if gs.gbuf is None:
            gs.gbuf = self.alloc(t.buf.nbytes, "d_" + t.buf.name)
        return TRef(gs.gbuf, t.B, t.H, t.W, t.C, t.ld, t.coff, t.dtype)

    def _add_into(self, dst: TRef, src: TRef, accumulate: bool):
        """dst (=|+=) src, elementwise (vt_bn_act_apply with unit scale)."""
        self._last_dgrad.pop(id(dst.buf), None)
        self.emit(N.OP_BN_ACT_APPLY,
                  [src.addr(), None, None, dst.addr() if accumulate else None, dst.addr()],
                  [src.ld, dst.ld, dst.ld, dst.C, 0, self.dtype], [dst.M])

    def grad_dirty(self, t: TRef) -> None:
        """a writer of d(t) is coming: sums formed from its earlier contents (_GradState.bn_sums) no longer describe it"""
        self._gs(t).bn_sums = None

    def _flush_pending(self, t: TRef):
        gs = self._gs(t)
        c0, c1 = t.coff, t.coff + t.C
        keep = []
        for a, b, add in gs.pending:
            if a < c1 and c0 < b:
                if not (c0 <= a and b <= c1):
                    # a contribution wider than the requested slice (a grouped convolution reads channel slices of a
                    # tensor whose gradient arrives full width): the part inside is added now, the rest stays pending
                    lo, hi = max(a, c0), min(b, c1)
                    if a < lo:
                        keep.append((a, lo, add.sl(0, lo - a)))
                    if hi < b:
                        keep.append((hi, b, add.sl(hi - a, b - hi)))
                    add, a, b = add.sl(lo - a, hi - lo), lo, hi
                sub = t.sl(a - c0, b - a)
                g = self._gref(sub)
                acc = gs.covered(a, b)
                if not acc and gs.touches(a, b):
                    raise NotImplementedError("partially initialised gradient slice")
                self.grad_dirty(t)
                self._add_into(g, add, acc)
                if not acc:
                    gs.init.append((a, b))
            else:
                keep.append((a, b, add))
        gs.pending = keep

    def grad_add(self, t: TRef, addend: TRef):
        """register an identity contribution d(t) += addend (materialised lazily)."""
        if t is None or not t.needs_grad:  # (None: an operand the op does not have, a residual as a rule)
            return
        assert t.same_geom(addend)
        self._gs(t).pending.append((t.coff, t.coff + t.C, addend))

    def grad_target(self, t: TRef):
        """for a kernel that writes d(t) and can fold ONE addend into its epilogue.
        returns (destination, residual or None)."""
        gs = self._gs(t)
        c0, c1 = t.coff, t.coff + t.C
        g = self._gref(t)
        self.grad_dirty(t)
        self._last_dgrad.pop(id(g.buf), None)  # (a writer is coming: whatever wrote the buffer last is no longer the only one)
        if gs.covered(c0, c1):
            self._flush_pending(t)
            return g, g
        if gs.touches(c0, c1):
            raise NotImplementedError("partially initialised gradient slice")
        exact = [p for p in gs.pending if p[0] == c0 and p[1] == c1]
        other = [p for p in gs.pending if p[0] < c1 and c0 < p[1] and not (p[0] == c0 and p[1] == c1)]
        if len(exact) == 1 and not other:
            gs.pending.remove(exact[0])
            gs.init.append((c0, c1))
            return g, exact[0][2]
        gs.init.append((c0, c1))
        if exact or other:
            # destination is written first (no residual), the addends are added afterwards
            self._deferred_flush = t
        return g, None

    def grad_written(self, t: TRef):
        """call after emitting the writer returned by grad_target when it had leftovers."""
        d = self._deferred_flush
        if d is not None:
            self._deferred_flush = None
            self._flush_pending(d)

    def grad_accum_target(self, t: TRef):
        """for a kernel that writes d(t) and cannot fold an addend but can ACCUMULATE: returns (destination, acc flag).  A
        foreign addend is materialised in the destination first."""
        gx, res = self.grad_target(t)
        if res is None:
            return gx, 0
        if not (res.buf is gx.buf and res.coff == gx.coff):
            self._add_into(gx, res, False)
        return gx, 1

    def _node(self, y: TRef, bwd: Callable[[TRef], None]):
        """register the backward of the op that wrote y: it runs under the op's tag with the complete d(y), and not at all
        where nothing contributed to d(y)"""
        tag = self.tag

        def run():
            self.tag = tag
            dy = self.grad_read(y)
            if dy is not None:
                bwd(dy)

        self.nodes.append(run)

    def grad_read(self, t: TRef) -> Optional[TRef]:
        """the complete gradient of t, or None if nothing contributed."""
        gs = self._gs(t)
        c0, c1 = t.coff, t.coff + t.C
        over = [p for p in gs.pending if p[0] < c1 and c0 < p[1]]
        if not gs.touches(c0, c1):
            if not over:
                return None
            if len(over) == 1 and over[0][0] <= c0 and c1 <= over[0][1]:
                return over[0][2].sl(c0 - over[0][0], c1 - c0)  # read-only alias of the single contribution
        self._flush_pending(t)
        if not gs.covered(c0, c1):
            # zero-fill the gaps (only dense full-width buffers can be memset)
            if t.ld == t.C and not gs.touches(c0, c1):
                g = self._gref(t)
                self.grad_dirty(t)
                self._last_dgrad.pop(id(g.buf), None)
                self.emit(N.OP_MEMSET, [g.addr()], [0], [t.M * t.C * t.esize])
                gs.init.append((c0, c1))
            else:
                raise NotImplementedError("gradient slice only partially produced")
        return self._gref(t)

    # -- input / output plumbing -------------------------------------------------------
    def refresh_mirror(self):
        """module API: the caller may have changed the f32 masters with any optimiser, so the bf16 mirror is refreshed
        at the head of every forward list"""
        if self.dtype == N.VT_BF16:
            n = self.store.pflat.numel()
            self.emit(N.OP_COPY2D, [(PARAMS, 0), (MIRROR, 0)], [N.VT_F32, N.VT_BF16, n, 0], [n, n, 1])

    MIX_OFF = 32  # byte offset of the MixUp / CutMix parameter block inside the HYPER buffer

    def input_images(self, B, C_, H, W, requires_grad=False, mix: bool = False) -> TRef:
        """NCHW f32 images (base INPUT) -> NHWC dtype with channels padded to 16 bytes; with `mix` the
        conversion applies MixUp / CutMix from the device parameter block (classifier.py:86-87)."""
        epc = _EPC[self.dtype]
        cpad = _round_up(C_, epc)
        x = self.act(B, H, W, cpad, "images", needs_grad=requires_grad)
        self.emit(N.OP_NCHW_TO_NHWC, [(INPUT, 0), x.addr(), (HYPER, self.MIX_OFF) if mix else None],
                  [B, C_, H, W, cpad, self.dtype])
        x.logical_C = C_
        if requires_grad and self.need_grad:
            dx_buf = self.alloc(B * C_ * H * W * 4, "d_images")
            self.input_grad = dx_buf

            def bwd():
                g = self.grad_read(x)
                if g is None:
                    self.emit(N.OP_MEMSET, [self.bp(dx_buf)], [0], [dx_buf.nbytes])
                else:
                    self.emit(N.OP_NHWC_TO_NCHW, [g.addr(), self.bp(dx_buf)], [g.ld, B, C_, H, W, self.dtype])

            self.nodes.append(bwd)
        return x

    # -- the ConvNormAct unit (reference components.py:13-46) --------------------------
    def _conv_desc(self, x: TRef, Cout, Ho, Wo, s, pad, k, ldy, ldw, flags, ldr=0, dil=1) -> N.ConvDesc:
        d = N.ConvDesc()
        d.dtype = self.dtype
        d.B, d.Hi, d.Wi, d.Cin, d.ldx = x.B, x.H, x.W, x.C, x.ld
        d.Ho, d.Wo, d.sh, d.sw, d.h0, d.w0 = Ho, Wo, s, s, -pad, -pad
        d.Cout, d.ldy, d.oH, d.oW = Cout, ldy, Ho, Wo
        d.oHs = d.oWs = 1
        d.oh0 = d.ow0 = 0
        d.ldw, d.ldr, d.flags = ldw, ldr, flags
        d.ntaps = k * k
        for i in range(k * k):
            d.dh[i], d.dw[i] = (i // k) * dil, (i % k) * dil
        return d

    @staticmethod
    def _specs(conv, norm) -> "tuple[ConvSpec, Optional[BNSpec]]":
        """a unit's layers as specs: nn.Conv2d / nn.BatchNorm2d / None / nn.Identity, or specs already"""
        if not isinstance(conv, ConvSpec):
            conv = ConvSpec.from_conv(conv)
        if norm is None or isinstance(norm, (BNSpec, nn.Identity)):
            return conv, norm if isinstance(norm, BNSpec) else None
        if not isinstance(norm, nn.BatchNorm2d):
            raise NotImplementedError(f"norm {type(norm).__name__} is outside the hot path")
        return conv, BNSpec.from_bn(norm)

    def conv_unit(self, x: TRef, conv, norm, relu, residual: Optional[TRef] = None, out: Optional[TRef] = None,
                  name: str = "", pool_out: Optional[TRef] = None, defer_norm: bool = False, residual_pre_act: bool = False,
                  _stem7: Optional[Buf] = None, keep: Optional[tuple] = None) -> TRef:
        """y = [relu]([bn](conv(x))) [+ residual], written to `out` when given.  `conv`: nn.Conv2d or ConvSpec, `norm`:
        nn.BatchNorm2d, BNSpec, nn.Identity or None.  `pool_out`: MaxPool2d(3, 2, 1) of y goes there as well -- from the
        unit's own normalise pass where it has one (vt_bn_act_apply_pool), and then the unit's BatchNorm backward reads the
        pooled gradient through the arg-max taps instead of a materialised d(y).
        `defer_norm`: the caller hands y to conv_unit_pair, which may take over the normalise pass (_DeferredNorm); where
        the unit qualifies, the pass is held back until something asks for y's address.
        `residual_pre_act`: the residual joins BEFORE the activation, y = relu(bn(conv(x)) + residual) -- the last unit of a
        torchvision BasicBlock / Bottleneck.  The general, strided and pointwise-shaped convolutions produce z and its
        statistics as always; the normalise pass and the BatchNorm backward are the add-then-ReLU passes of vt_resnet.hip.
        The paths that cannot honour the mode (the pointwise fold, the fused inference epilogue, a deferred normalise
        pass) are not taken: the unit runs the general kernel plus those passes.
        `keep`: a row of the keep table (keep_table) -- stochastic depth in "row" mode, y = keep[b] * act(bn(conv(x))) +
        residual with one factor per image: the normalise pass and the BatchNorm backward are the keep passes of vt_mbconv.hip
        (any activation code; the residual's gradient stays d(y)).  As with residual_pre_act, the pointwise fold, the fused
        inference epilogue and a deferred normalise pass are not taken.  keep=None emits what it always emitted.
        `keep` with `residual_pre_act`: y = relu(keep[b] * bn(conv(x)) + residual) -- stochastic depth of a ResNet block, the drop
        behind the last BatchNorm and in front of the shortcut -- on the keep forms of the add-then-ReLU passes (vt_resnet.hip):
        the identity's gradient stays the masked d(y), the BatchNorm side sees keep[b] times it.
        Validation and dispatch: grouped -> depthwise -> pointwise -> the general kernels."""
        conv, bn_spec = self._specs(conv, norm)
        relu = int(relu)  # activation code: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 SiLU, 4 GELU, 5 ReLU6, 6 Hardswish (include/vt_amd.h)
        pre_act = bool(residual_pre_act)
        if pre_act and (residual is None or bn_spec is None or relu != 1 or conv.groups != 1 or pool_out is not None):
            raise NotImplementedError(f"{name}: residual_pre_act is relu(bn(conv(x)) + residual): it needs a residual, a "
                                      "BatchNorm, ReLU, groups = 1 and no fused pool")
        # (keep with residual_pre_act: relu(keep[b] * bn(conv(x)) + residual), the keep forms of the add-then-ReLU passes;
        #  the checks of residual_pre_act above are the ones it needs)
        if keep is not None and not pre_act and (residual is None or bn_spec is None or conv.groups != 1 or pool_out is not None):
            raise NotImplementedError(f"{name}: keep is keep[b] * act(bn(conv(x))) + residual: it needs a residual, a BatchNorm, "
                                      "groups = 1, no fused pool and no residual_pre_act")
        if conv.groups != 1:
            return self._grouped_unit(x, conv, bn_spec, relu, residual, out, name, pool_out)
        dt, epc = self.dtype, _EPC[self.dtype]
        k, Cout = conv.k, conv.out_channels
        if k * k > N.VT_MAX_TAPS:
            raise NotImplementedError(f"kernel {k}x{k} exceeds {N.VT_MAX_TAPS} taps")
        if x.logical_c != conv.in_channels:
            raise ValueError(f"conv expects {conv.in_channels} input channels, got {x.logical_c}")
        if Cout % epc:
            raise NotImplementedError(f"out_channels={Cout} must be a multiple of {epc} for dtype {dt}")
        Ho, Wo = conv.out_size(x.H, x.W)
        if Ho <= 0 or Wo <= 0:
            raise ValueError(f"{name}: a {x.H}x{x.W} map is smaller than the dilated {k}x{k} kernel")
        if bn_spec is not None:
            spec = (conv, bn_spec, relu, residual, out, name)
            if not pre_act and keep is None and self._pw_ok(x, [spec]):  # (the pointwise passes add the residual behind the ReLU)
                y_pw = self.pw_units(x, [spec])[0]
                if pool_out is not None:
                    self.maxpool3x3s2(y_pw, out=pool_out, name=name + ".max_pool")
                return y_pw
        assert out is None or (out.B, out.H, out.W, out.C) == (x.B, Ho, Wo, Cout), "out geometry mismatch"
        assert residual is None or (residual.B, residual.H, residual.W, residual.C) == (x.B, Ho, Wo, Cout)

        self.tag += 1
        self.n_units += 1
        wptr, wpack, ldw = self._filter_operand(conv, x) if _stem7 is None else (self.bp(_stem7), _stem7, conv.k ** 2 * x.C)
        has_bn, generic_act = bn_spec is not None, relu >= 2  # (generic: only the unfused BatchNorm passes implement these)
        track, w, s, pad = self.need_grad, conv.weight, conv.stride, conv.padding
        # the unit follows ITS BatchNorm's flag (a frozen bn.eval() inside a training model uses the
        # running statistics and leaves them untouched, like nn.BatchNorm2d)
        unit_training = bn_spec.training if has_bn else self.training
        fused = has_bn and not unit_training and not track and not generic_act and not pre_act and keep is None
        # (a training-mode BatchNorm with activation code < 2, no residual, no pool, no SyncBatchNorm, finalize-in-apply on,
        #  a tensor beyond the memory-side cache; see pw_fold_min_mb)
        defer = (defer_norm and has_bn and unit_training and not fused and not generic_act and residual is None and
                 out is None and pool_out is None and wpack is None and keep is None and not self.bn_sync and self.bn_fin_apply and
                 self.pointwise and not self.deterministic and dt == N.VT_BF16 and
                 x.B * Ho * Wo * Cout * _ESIZE[dt] >= self.pw_fold_min_mb * 1e6)
        if defer:  # y has no place in the arena until something reads it
            y = TRef(Buf(ARENA, -1, x.B * Ho * Wo * Cout * _ESIZE[dt], name + ".y"), x.B, Ho, Wo, Cout, Cout, 0, dt)
        else:
            y = out if out is not None else self.act(x.B, Ho, Wo, Cout, name + ".y")
        u = _ConvUnit(conv, relu, x, y, residual, name, self.tag, wptr, wpack, ldw)
        u.defer, u.pre_act, u.stem7, u.keep = defer, pre_act, _stem7 is not None, keep
        u.stem_fused = stem_fused = (
            track and u.padded and has_bn and not fused and residual is None and not generic_act and keep is None and
            not x.needs_grad and w.requires_grad and dt == N.VT_BF16 and Cout == 32 and k == 3 and s == 1 and
            conv.dilation == 1 and pad == 1 and x.C == 8 and x.ld == 8 and x.W <= 888 and
            x.B * (x.H + 1) * (x.W + 1) < 0x7fff0000)  # (ring in LDS: halo <= 896 rows)
        u.stem_y = stem_y = stem_fused and unit_training and x.W <= 824  # (one more step of halo)
        if has_bn:
            u.bn = _BNEmitter(self, bn_spec, Cout)
        pool_fused = pool_out is not None and has_bn and not fused and not stem_y and not generic_act
        if fused:
            self._fwd_inference_fused(u)
        elif stem_y:
            self._fwd_stem(u)
        elif has_bn:
            self._fwd_bn(u, pool_out if pool_fused else None)
        elif relu:
            self._fwd_act(u)
        else:
            self._fwd_plain(u)
        if pool_out is not None and not pool_fused:
            self.maxpool3x3s2(y, out=pool_out, name=name + ".max_pool")  # (no normalise pass to fuse it into)

        # (round 5: the 1x1 stride-1 units of a stage too -- DarknetBlock.conv1, darknet.py:23 -- through the general
        #  kernel's grouped launch: a launch of one such layer is mostly its atomic flush and its ramp)
        grp3 = k == 3 and s == 1 and conv.dilation == 1 and pad == 1 and x.C > 32 and Cout > 32
        grp1 = k == 1 and s == 1 and pad == 0 and self.wgrad_group_1x1
        if (track and has_bn and not fused and not stem_fused and not u.padded and w.requires_grad and dt == N.VT_BF16 and
                (grp3 or grp1) and self.wgrad_group > 1 and not self.deterministic):
            u.wg_key = (k, x.B, x.H, x.W, x.C, x.ld, Cout, ldw)
            self._wg_expect[u.wg_key] = self._wg_expect.get(u.wg_key, 0) + 1
        if track:
            self.nodes.append(lambda: self._conv_unit_bwd(u))
        return y

    def _filter_operand(self, conv: ConvSpec, x: TRef):
        """(address, padded copy or None, row length) of the filter image the unit's launches read: the f32 master, its bf16
        mirror, or -- the stem, whose 3 input channels are padded to one 16-byte chunk -- a zero-padded copy in the arena"""
        dt, w, Cin_w, rows = self.dtype, conv.weight, conv.in_channels, conv.out_channels * conv.k ** 2
        if x.C == Cin_w:
            return self.pref(w, mirror=dt != N.VT_F32), None, conv.k ** 2 * x.C
        wpack = self.alloc(rows * x.C * _ESIZE[dt], "wpad")
        self.emit(N.OP_MEMSET, [self.bp(wpack)], [0], [wpack.nbytes])
        # (bf16: from the mirror every other filter is read from -- the same rounding of the same master value, and
        #  under the sharded gradient exchange the mirror is what the all-gather refreshes on every rank, whereas the
        #  f32 master of a slice another rank owns goes stale)
        wsrc, wsrc_dt = (self.pref(w, mirror=True), dt) if dt == N.VT_BF16 else (self.pref(w), N.VT_F32)
        self.emit(N.OP_COPY2D, [wsrc, self.bp(wpack)], [wsrc_dt, dt, Cin_w, 0], [Cin_w, x.C, rows])
        return self.bp(wpack), wpack, conv.k ** 2 * x.C

    def _unit_desc(self, u: "_ConvUnit", ldy: int, flags: int, ldr: int = 0) -> N.ConvDesc:
        c = u.conv
        return self._conv_desc(u.x, c.out_channels, u.y.H, u.y.W, c.stride, c.padding, c.k, ldy, u.ldw, flags, ldr, dil=c.dilation)

    def _conv(self, u: "_ConvUnit", dst: Optional[TRef], flags: int = 0, scale=None, shift=None, res: Optional[TRef] = None,
              stats: Optional[Buf] = None):
        """the unit's convolution into dst (None: nothing is stored), with the epilogue its operands ask for"""
        flags |= (N.VT_CONV_AFFINE if shift is not None else 0) | (N.VT_CONV_RESIDUAL if res is not None else 0) | \
            (N.VT_CONV_STATS if stats is not None else 0)
        self.emit(N.OP_CONV_IGEMM, [u.x.addr(), u.wptr, _addr(dst), scale, shift, _addr(res), self.bp(stats) if stats else None],
                  desc=self._unit_desc(u, (dst or u.y).ld, flags, _ld(res)))

    def _fwd_inference_fused(self, u: "_ConvUnit") -> None:
        """eval-mode BatchNorm without gradients: ONE conv launch with the affine (+ ReLU, + residual) epilogue"""
        u.bn.eval_coeffs(scale_shift_only=True)
        self._conv(u, u.y, N.VT_CONV_RELU if u.relu else 0, u.bn.cp[0], u.bn.cp[1], u.residual)

    def _fwd_stem(self, u: "_ConvUnit") -> None:
        """the stem with recomputed z: the conv runs twice (statistics only, then with the normalise + ReLU epilogue)"""
        u.y.stem_out = True  # (the unit that reads it releases its filter gradient late: wgrad_late_stem)
        stats = self.zeroed_f32(N.stat_floats(u.y.C), "stats")
        self._conv(u, None, N.VT_CONV_NOSTORE, stats=stats)
        u.bn.finalize(stats, u.y.M)
        self._conv(u, u.y, N.VT_CONV_RELU if u.relu else 0, u.bn.cp[0], u.bn.cp[1])

    def _fwd_bn(self, u: "_ConvUnit", pool_out: Optional[TRef]) -> None:
        """BatchNorm with stored z: conv (+ batch statistics) -> coefficients -> the normalise pass, which may also
        finalize the statistics for itself (vt_bn_finalize_apply) or write the 3x3 stride-2 max pool of y"""
        y, bn, res, relu = u.y, u.bn, u.residual, u.relu
        u.z = z = self.act(y.B, y.H, y.W, y.C, u.name + ".z")
        fin_fwd = False
        if bn.spec.training:
            stats = self.zeroed_f32(N.stat_floats(y.C), "stats")
            fin_fwd = self.bn_fin_apply and not self.bn_sync and (relu < 2 or u.keep is not None) and pool_out is None
            self._conv(u, z, stats=stats)
            if u.defer:
                y.buf.deferred = _DeferredNorm(self, u, stats)
                return
            if not fin_fwd:
                bn.finalize(stats, y.M)
        else:
            self._conv(u, z)
            bn.eval_coeffs()
        if pool_out is not None:
            assert (pool_out.B, pool_out.H, pool_out.W, pool_out.C) == (y.B, (y.H - 1) // 2 + 1, (y.W - 1) // 2 + 1, y.C)
            u.pool_out, u.pool_am = pool_out, self.alloc(y.B * pool_out.H * pool_out.W * y.C, "argmax")
            self._act_apply(z, bn.cp[0], bn.cp[1], res, y, relu, [pool_out.addr(), self.bp(u.pool_am)],
                            [pool_out.ld, y.B, y.H, y.W])
        elif u.pre_act and u.keep is not None and fin_fwd:
            ptrs, flts = bn.finalize_operands(stats, y.M)
            self.emit(N.OP_BN_ADD_ACT_KEEP_FIN_APPLY, ptrs + [z.addr(), res.addr(), y.addr(), u.keep],
                      [y.C, z.ld, res.ld, y.ld, self.dtype, y.H * y.W], flts + [y.M])
        elif u.pre_act and u.keep is not None:
            self.emit(N.OP_BN_ADD_ACT_KEEP_APPLY, [z.addr(), bn.cp[0], bn.cp[1], res.addr(), y.addr(), u.keep],
                      [z.ld, res.ld, y.ld, y.C, self.dtype, y.H * y.W], [y.M])
        elif u.keep is not None and fin_fwd:
            ptrs, flts = bn.finalize_operands(stats, y.M)
            self.emit(N.OP_BN_KEEP_FIN_APPLY, ptrs + [z.addr(), res.addr(), y.addr(), u.keep],
                      [y.C, z.ld, res.ld, y.ld, y.H * y.W, relu, self.dtype], flts + [y.M])
        elif u.keep is not None:
            self.emit(N.OP_BN_KEEP_APPLY, [z.addr(), bn.cp[0], bn.cp[1], res.addr(), y.addr(), u.keep],
                      [z.ld, res.ld, y.ld, y.H * y.W, y.C, relu, self.dtype], [y.M])
        elif u.pre_act and fin_fwd:
            ptrs, flts = bn.finalize_operands(stats, y.M)
            self.emit(N.OP_BN_ADD_ACT_FIN_APPLY, ptrs + [z.addr(), res.addr(), y.addr()], [y.C, z.ld, res.ld, y.ld, self.dtype],
                      flts + [y.M])
        elif u.pre_act:
            self.emit(N.OP_BN_ADD_ACT_APPLY, [z.addr(), bn.cp[0], bn.cp[1], res.addr(), y.addr()],
                      [z.ld, res.ld, y.ld, y.C, self.dtype], [y.M])
        elif fin_fwd:
            ptrs, flts = bn.finalize_operands(stats, y.M)
            self.emit(N.OP_BN_FIN_APPLY, ptrs + [z.addr(), _addr(res), y.addr()],
                      [y.C, z.ld, _ld(res), y.ld, relu, self.dtype], flts + [y.M])
        else:
            self._act_apply(z, bn.cp[0], bn.cp[1], res, y, relu)

    def _fwd_act(self, u: "_ConvUnit") -> None:
        """conv (+bias) -> activation, no BatchNorm: ConvNormAct(norm="none") (components.py:33-36).  The
        pre-activation is kept (backward needs act'(z)); the activation is the unit-scale form of the normalise pass."""
        u.z = self.act(u.y.B, u.y.H, u.y.W, u.y.C, u.name + ".z")
        self._conv(u, u.z, shift=self.pref(u.conv.bias))
        self._act_apply(u.z, None, None, u.residual, u.y, u.relu)

    def _fwd_plain(self, u: "_ConvUnit") -> None:
        """plain conv (+bias): ESE gate conv (vovnet.py:24), classifier head (classifier.py:63)"""
        self._conv(u, u.y, shift=self.pref(u.conv.bias), res=u.residual)

    def _act_apply(self, z: TRef, scale, shift, residual: Optional[TRef], y: TRef, act: int, pool_ptrs=(), pool_ints=()):
        """y = act(z * scale + shift) [+ residual] (vt_bn_act_apply; scale / shift None: unit scale, no shift)"""
        self.emit(N.OP_BN_ACT_APPLY, [z.addr(), scale, shift, _addr(residual), y.addr(), *pool_ptrs],
                  [z.ld, _ld(residual), y.ld, y.C, int(act), self.dtype, *pool_ints], [y.M])

    def _act_bwd(self, g: TRef, z: TRef, scale, shift, bcoef, dz: TRef, act: int, taps=None):
        """dz = act'(.) * g [- the BatchNorm backward terms of `bcoef`] (vt_bn_act_bwd_apply; no coefficients: the
        activation's backward alone, at the pre-activation z).  `taps` = (arg-max address, [B, Ho, Wo]): g is the gradient
        of the fused max pool."""
        self.emit(N.OP_BN_BWD_APPLY, [g.addr(), z.addr(), scale, shift, bcoef, dz.addr()] + ([taps[0]] if taps else []),
                  [g.ld, z.ld, dz.ld, dz.C, int(act), self.dtype] + (taps[1] if taps else []), [dz.M])

    # .. backward of the unit, from the record its forward left ..........................................................
    def _conv_unit_bwd(self, u: "_ConvUnit") -> None:
        self.tag = u.tag
        x, y, c = u.x, u.y, u.conv
        pool_grad = None  # (fused pool: the gradient of the pooled map, read through the arg-max taps)
        if u.pool_out is not None:
            dp = self.grad_read(u.pool_out)
            if dp is not None:
                if u.residual is None and not u.stem_fused and self.grad_read(y) is None:
                    pool_grad = dp  # the pool is y's only consumer: d(y) is never formed
                else:  # y feeds something else too (a returned feature map, a shortcut): form d(y) as the pool's backward would
                    gy, acc = self.grad_accum_target(y)
                    self.emit(N.OP_MAXPOOL_BWD, [dp.addr(), self.bp(u.pool_am), gy.addr()],
                              [dp.ld, gy.ld, x.B, u.y.H, u.y.W, y.C, acc, self.dtype])
                    self.grad_written(y)
        dy = self.grad_read(y) if pool_grad is None else None
        if dy is None and pool_grad is None:
            return
        if not u.pre_act:  # (pre_act: the identity's gradient is the MASKED d(y), an output of the backward apply pass)
            self.grad_add(u.residual, dy)
        if u.stem_fused:
            return self._stem_bwd(u, dy)
        if u.pre_act:
            dz = self._bn_add_act_bwd(u, dy)
        elif u.keep is not None:
            dz = self._bn_keep_bwd(u, dy)
        else:
            dz = self._bn_bwd(u, dy, pool_grad) if u.bn is not None else self._act_bias_bwd(u, dy)
        # Released BEFORE the unit's data gradient, except behind the stem (see __init__): there the data gradient
        # runs first and the filter gradient beside the stem's one-pass backward.
        late = x.needs_grad and x.stem_out
        if not late:
            self._release_wgrad(u, dz)
        if x.needs_grad:
            self._dgrad(x, dz, u.wptr, u.ldw, c)
        if late:
            self._release_wgrad(u, dz)

    def _stem_bwd(self, u: "_ConvUnit", dy: TRef) -> None:
        # dz = a*g - b*z + d feeds nothing but the filter gradient (the unit's input is the image): the
        # pass that reduces (sum g, sum g*xhat) also correlates g, z and 1 with the tap-shifted x, and a
        # small kernel finishes dW = a*G - b*Z + d*X once (a, b, d) exist (vt_stem_bwd.hip)
        x, cp, Cout, det = u.x, u.bn.cp, u.y.C, int(self.deterministic)
        sums = self.zeroed_f32(N.stat_floats(Cout), "bwdsums")
        gzx = self.zeroed_f32(N.lib().vt_stem_bn_bwd_scratch_bytes(Cout) // 4, "stem_gzx")
        zy = u.y if u.stem_y else u.z
        self.emit(N.OP_STEM_BWD_REDUCE, [x.addr(), dy.addr(), zy.addr(), *cp, self.bp(sums), self.bp(gzx)],
                  [self.dtype, x.B, x.H, x.W, Cout, dy.ld, zy.ld, u.relu, det | (2 if u.stem_y else 0)])
        if u.stem_y:  # sum g * xhat from the correlations (z is linear in the patch): nothing recovered from y
            self.emit(N.OP_STEM_BWD_S2, [self.bp(gzx), u.wptr, cp[2], cp[3], self.bp(sums)], [Cout, det])
        bcoef = self.f32(3 * Cout, "bwdcoef")
        u.bn.bwd_finalize(sums, bcoef, u.y.M)
        self.emit(N.OP_STEM_BWD_COMBINE, [self.bp(gzx), self.bp(bcoef), self.pgrad(u.conv.weight), u.wptr if u.stem_y else None],
                  [Cout, u.conv.in_channels, det])

    def _bn_bwd(self, u: "_ConvUnit", dy: Optional[TRef], pool_grad: Optional[TRef]) -> TRef:
        """dz of a BatchNorm unit from d(y) (or from the gradient of its fused max pool): reduce -> finalize -> apply, the
        last two in one launch by default, or one of the two off-by-default fused forms (see __init__)"""
        bn, z, relu, M, dt = u.bn, u.z, u.relu, u.y.M, self.dtype
        plain = pool_grad is None and dt == N.VT_BF16 and relu < 2
        rec = self._last_dgrad.get(id(dy.buf)) if (self.fuse_bnred and plain and self._cur is self.bwd) else None
        fused_red = rec is not None and rec[1] == dy.coff and rec[2] == dy.coff + dy.C and any(o is rec[0] for o in self.bwd)
        # (the launch that wrote the whole of d(y) also formed this unit's sums, and nothing has written d(y) since)
        pre = self._gs(u.y).bn_sums if (plain and dy.buf is self._gs(u.y).gbuf and (dy.coff, dy.C) == (u.y.coff, u.y.C)) else None
        if pre is not None:
            fused_red = True
        one_launch = self.bn_bwd_fused and not fused_red and plain and not self.bn_sync
        sums, bcoef, dz = bn.bwd_buffers(u.y, u.name + ".dz")
        if pre is not None:
            sums = pre
        if one_launch:
            sync = self.zeroed_f32(4, "bwdsync")
            self.emit(N.OP_BN_BWD_FUSED,
                      [dy.addr(), z.addr(), *bn.cp, self.bp(sums), self.bp(sync), *bn.grads(), self.bp(bcoef), dz.addr()],
                      [dy.ld, z.ld, dz.ld, dz.C, relu, dt, int(bn.spec.training)], [M, M * self.bn_world, 1.0 / self.bn_world])
            return dz
        if fused_red and pre is None:
            # d(y) came out of ONE data-gradient launch and nothing was added to it since: that launch also forms
            # this unit's backward sums (the op is patched in place: ptr dz w dy | z scale shift mean invstd sums)
            fop = rec[0]
            fop.kind = N.OP_CONV_DGRAD_BNRED | (fop.kind & N.OP_SIDE_STREAM)
            for k_, pa in enumerate((z.addr(), *bn.cp, self.bp(sums)), start=3):
                fop.ptr[k_].base, fop.ptr[k_].offset = pa
            k0 = C.sizeof(N.ConvDesc) // 4
            fop.i[k0], fop.i[k0 + 1] = z.ld, relu
            self._last_dgrad.pop(id(dy.buf), None)
        g = dy if pool_grad is None else pool_grad
        taps = None if pool_grad is None else (self.bp(u.pool_am), [u.x.B, u.y.H, u.y.W])
        if self.bn_fin_apply and not self.bn_sync and pool_grad is None and relu < 2:
            if not fused_red:
                bn.bwd_reduce(g, z, relu, sums, M)
            self.emit(N.OP_BN_BWD_FIN_APPLY,
                      [self.bp(sums), *bn.cp, *bn.grads(), self.bp(bcoef), g.addr(), z.addr(), dz.addr()],
                      [dz.C, int(bn.spec.training), g.ld, z.ld, dz.ld, relu, dt], [M * self.bn_world, 1.0 / self.bn_world, M])
        else:
            bn.bwd_three_launches(g, z, relu, sums, bcoef, dz, taps, reduce=not fused_red)
        return dz

    def _bn_add_act_bwd(self, u: "_ConvUnit", dy: TRef) -> TRef:
        """dz and d(residual) of a unit y = relu(bn(conv) + residual): reduce (mask from the stored y) -> finalize -> ONE apply
        pass with two outputs, dz and the identity's gradient g = dy * [y > 0].  The identity usually feeds the block's first
        convolution too: d(residual) is written where it is the first contribution and accumulated where something
        already wrote it (grad_accum_target)."""
        bn, z, y, r, M, dt = u.bn, u.z, u.y, u.residual, u.y.M, self.dtype
        sums, bcoef, dz = bn.bwd_buffers(y, u.name + ".dz")
        if r.needs_grad:
            dr, acc = self.grad_accum_target(r)
        else:  # (nothing reads it: the pass has two outputs)
            dr, acc = self.act(r.B, r.H, r.W, r.C, u.name + ".dr"), 0
        # (u.keep: the keep forms take the plain forms' operands, then the row of the keep table and HW)
        kp, khw = ([u.keep], [y.H * y.W]) if u.keep is not None else ([], [])
        red, fin, app = ((N.OP_BN_ADD_ACT_KEEP_BWD_REDUCE, N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_APPLY)
                         if u.keep is not None else
                         (N.OP_BN_ADD_ACT_BWD_REDUCE, N.OP_BN_ADD_ACT_BWD_FIN_APPLY, N.OP_BN_ADD_ACT_BWD_APPLY))
        self.emit(red, [dy.addr(), y.addr(), z.addr(), bn.cp[2], bn.cp[3], self.bp(sums)] + kp,
                  [dy.ld, y.ld, z.ld, y.C, dt] + khw, [M])
        if self.bn_fin_apply and not self.bn_sync:
            self.emit(fin,
                      [self.bp(sums), bn.cp[0], bn.cp[2], bn.cp[3], *bn.grads(), self.bp(bcoef), dy.addr(), y.addr(), z.addr(),
                       dz.addr(), dr.addr()] + kp,
                      [y.C, int(bn.spec.training), dy.ld, y.ld, z.ld, dz.ld, dr.ld, acc, dt] + khw,
                      [M * self.bn_world, 1.0 / self.bn_world, M])
        else:
            bn.bwd_finalize(sums, bcoef, M)
            self.emit(app, [dy.addr(), y.addr(), z.addr(), self.bp(bcoef), dz.addr(), dr.addr()] + kp,
                      [dy.ld, y.ld, z.ld, dz.ld, dr.ld, acc, y.C, dt] + khw, [M])
        if r.needs_grad:
            self.grad_written(r)
        return dz

    def _bn_keep_bwd(self, u: "_ConvUnit", dy: TRef) -> TRef:
        """dz of a unit y = keep[b] * act(bn(conv)) + residual: reduce -> finalize -> apply with g = keep[b] * dy * act'(.), the
        last two in one launch by default.  d(residual) = d(y) was registered by the caller."""
        bn, z, y, M, dt, act = u.bn, u.z, u.y, u.y.M, self.dtype, u.relu
        HW = y.H * y.W
        sums, bcoef, dz = bn.bwd_buffers(y, u.name + ".dz")
        self.emit(N.OP_BN_KEEP_BWD_REDUCE, [dy.addr(), z.addr(), *bn.cp, self.bp(sums), u.keep],
                  [dy.ld, z.ld, HW, y.C, act, dt], [M])
        if self.bn_fin_apply and not self.bn_sync:
            self.emit(N.OP_BN_KEEP_BWD_FIN_APPLY,
                      [self.bp(sums), *bn.cp, *bn.grads(), self.bp(bcoef), dy.addr(), z.addr(), dz.addr(), u.keep],
                      [y.C, int(bn.spec.training), dy.ld, z.ld, dz.ld, HW, act, dt], [M * self.bn_world, 1.0 / self.bn_world, M])
        else:
            bn.bwd_finalize(sums, bcoef, M)
            self.emit(N.OP_BN_KEEP_BWD_APPLY, [dy.addr(), z.addr(), bn.cp[1], self.bp(bcoef), dz.addr(), u.keep],
                      [dy.ld, z.ld, dz.ld, HW, y.C, act, dt], [M])
        return dz

    def _act_bias_bwd(self, u: "_ConvUnit", dy: TRef) -> TRef:
        """dz of a unit without BatchNorm (dz = dy * act'(z)), and the bias gradient"""
        dz, bias = dy, u.conv.bias
        if u.relu:
            dz = self.act(dy.B, u.y.H, u.y.W, dy.C, u.name + ".dz")
            self._act_bwd(dy, u.z, None, None, None, dz, u.relu)
        if bias is not None and bias.requires_grad:
            if self.deterministic:
                qb = self.zeroed_f32(4 * dz.C, "dbq", bwd=True)
                self.emit(N.OP_COLSUM, [dz.addr(), self.bp(qb)], [dz.ld, dz.C, self.dtype, 1], [u.y.M])
                self.emit(N.OP_FIXED_TO_F32, [self.bp(qb), self.pgrad(bias)], [1], [dz.C])
            else:
                self.emit(N.OP_COLSUM, [dz.addr(), self.pgrad(bias)], [dz.ld, dz.C, self.dtype], [u.y.M])
        return dz

    def _release_wgrad(self, u: "_ConvUnit", dz: TRef) -> None:
        # filter gradient: needs only x and dz and nothing in backward waits for it, so it goes to the
        # side stream, beside the HBM-bound BatchNorm passes of the units that follow in backward order
        x, w = u.x, u.conv.weight
        if not w.requires_grad:
            return
        dfwd = self._unit_desc(u, dz.ld, 0)
        if u.wg_key is not None:
            self._wgrad_hold(u.wg_key, x.addr(), dz.addr(), self.pgrad(w), dfwd, u.ldw)
            return
        self.emit(N.OP_FORK)
        slab, slab_mb = None, 0
        if self.wgrad_slab_mb > 0:  # two-stage (stored slabs + ordered reducer) instead of f32 atomics
            if self._wgrad_slab is None:
                self._wgrad_slab = self.alloc(self.wgrad_slab_mb << 20, "wgrad_slabs")
            slab, slab_mb = self.bp(self._wgrad_slab), self.wgrad_slab_mb
        ws = None
        if u.padded:  # the gradient of the padded filter image, then its first in_channels columns into the parameter's
            rows = u.conv.out_channels * u.conv.k ** 2
            ws = self.bp(self.zeroed_f32(rows * x.C, "dwpad", bwd=True))
        self.emit(N.OP_CONV_WGRAD, [x.addr(), dz.addr(), ws or self.pgrad(w), slab], desc=dfwd,
                  extra_ints=[u.ldw, slab_mb], side=True)
        if u.stem7:  # the transpose of the filter repack: [Cout][4][4][Cs] -> += [Cout][7][7][3]
            self.emit(N.OP_STEM7_UNPACK_WGRAD, [ws, self.pgrad(w)], [x.C, u.conv.out_channels], side=True)
        elif u.padded:
            self.emit(N.OP_COPY2D, [ws, self.pgrad(w)], [N.VT_F32, N.VT_F32, u.conv.in_channels, 1],
                      [x.C, u.conv.in_channels, rows], side=True)

    def stem7_unit(self, x: TRef, conv: nn.Conv2d, norm: nn.BatchNorm2d, relu=1, pool_out: Optional[TRef] = None,
                   name: str = "conv1") -> TRef:
        """The ResNet stem Conv2d(3, C, 7, stride 2, padding 3, bias=False) -> BatchNorm2d -> ReLU [-> MaxPool2d(3, 2, 1) into
        `pool_out`].  49 taps exceed VT_MAX_TAPS; padded to 8 x 8 with a zero first row and column the filter is a 4 x 4
        stride-1 filter over the space-to-depth image (12 channels (py, px, c), zero-padded to whole 16-byte chunks) whose
        taps sit at offsets -2 .. +1 -- a window the descriptor's per-tap offsets express, so forward and filter gradient run
        the existing kernels.  New launches: the image gather, the filter repack and, in backward, its transpose.
        The image gets no gradient."""
        spec, _ = self._specs(conv, norm)
        if ((spec.k, spec.stride, spec.padding, spec.dilation, spec.groups, spec.in_channels) != (7, 2, 3, 1, 1, 3) or
                spec.bias is not None):
            raise NotImplementedError(f"{name}: the stem path is Conv2d(3, C, 7, stride=2, padding=3, bias=False)")
        if x.needs_grad:
            raise NotImplementedError(f"{name}: x.requires_grad -- the 7x7 stem forms no gradient of the image (its input is "
                                      "the data; pass images that do not require a gradient)")
        dt, epc = self.dtype, _EPC[self.dtype]
        if x.logical_c != 3 or x.C != epc:
            raise ValueError(f"{name}: expects the 3-channel image in one 16-byte chunk per pixel, got {x.logical_c} of {x.C}")
        Cs, Cout = int(N.lib().vt_stem7_s2d_channels(dt)), spec.out_channels
        self.tag += 1
        xs = self.act(x.B, (x.H + 1) // 2, (x.W + 1) // 2, Cs, name + ".s2d", needs_grad=False)
        self.emit(N.OP_STEM7_S2D, [x.addr(), xs.addr()], [x.ld, xs.ld, x.B, x.H, x.W, dt])
        w4 = self.alloc(Cout * 16 * Cs * _ESIZE[dt], "w4x4")
        # (bf16: from the mirror, as _filter_operand's padded copy -- the sharded exchange refreshes the mirror on every rank)
        wsrc, wsrc_dt = (self.pref(spec.weight, mirror=True), dt) if dt == N.VT_BF16 else (self.pref(spec.weight), N.VT_F32)
        self.emit(N.OP_STEM7_PACK_FILTER, [wsrc, self.bp(w4)], [wsrc_dt, dt, Cout])
        self.tag -= 1  # (conv_unit advances it: the gather, the repack and the unit share one tag)
        conv4 = ConvSpec(4, 1, 2, 1, 1, Cs, Cout, spec.weight, None, crop=1)
        return self.conv_unit(xs, conv4, norm, relu, name=name, pool_out=pool_out, _stem7=w4)

    def _grouped_unit(self, x: TRef, conv: "ConvSpec", bn: "Optional[BNSpec]", relu, residual, out, name, pool_out) -> TRef:
        """nn.Conv2d(groups=G) inside a ConvNormAct (reference components.py:32): G independent units over channel slices
        of x and y -- the kernels take a pixel stride and a channel offset, the filter rows of a group are contiguous in
        the [Cout][kh][kw][Cin / G] image, and BatchNorm is per channel, so a group's statistics, coefficients and
        parameter gradients are slices too.  Slices are addressed in 16-byte chunks: Cin / G and Cout / G must be
        multiples of 8 (bf16) / 4 (f32); depthwise convolutions are outside the Darknet / VoVNet path."""
        G = conv.groups
        Cin, Cout = conv.in_channels, conv.out_channels
        ci, co = Cin // G, Cout // G
        epc = _EPC[self.dtype]
        if x.logical_c != Cin or x.C != Cin:
            raise ValueError(f"conv expects {Cin} (unpadded) input channels, got {x.logical_c}")
        if ci == 1 and co == 1 and Cin % epc == 0:
            return self._depthwise_unit(x, conv, bn, relu, residual, out, name, pool_out)
        if ci % epc or co % epc:
            raise NotImplementedError(
                f"groups={G} with {ci} -> {co} channels per group: channel slices are addressed in 16-byte chunks "
                f"({epc} elements); narrow groups other than depthwise (groups = in_channels = out_channels) are outside the "
                "hot path")
        Ho, Wo = conv.out_size(x.H, x.W)
        y = out if out is not None else self.act(x.B, Ho, Wo, Cout, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (x.B, Ho, Wo, Cout), "out geometry mismatch"
        for g in range(G):
            self.conv_unit(x.sl(g * ci, ci), conv.group(g), bn.group(g, G) if bn is not None else None, relu,
                           residual=residual.sl(g * co, co) if residual is not None else None,
                           out=y.sl(g * co, co), name=f"{name}.g{g}")
        if pool_out is not None:
            self.maxpool3x3s2(y, out=pool_out, name=name + ".max_pool")
        return y

    def _depthwise_unit(self, x: TRef, conv: "ConvSpec", bn_spec: "Optional[BNSpec]", relu, residual, out, name,
                        pool_out) -> TRef:
        """nn.Conv2d(C, C, k, groups=C) inside a ConvNormAct (reference components.py:26-44 with `groups = in_channels`):
        vt_dwconv_fwd (+ batch statistics) -> the ordinary BatchNorm finalize / normalise passes; backward: the ordinary
        BatchNorm backward -> vt_dwconv_wgrad (side stream) and vt_dwconv_dgrad.  Streaming kernels (round 6): off the
        Darknet / VoVNet path, present so that every `groups` the constructor accepts runs on the GPU."""
        Cc, B = conv.in_channels, x.B
        Ho, Wo = conv.out_size(x.H, x.W)
        M, dt = B * Ho * Wo, self.dtype
        if self.deterministic:
            raise NotImplementedError("depthwise filter gradients use f32 atomics: not available in deterministic mode")
        y = out if out is not None else self.act(B, Ho, Wo, Cc, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (B, Ho, Wo, Cc), "out geometry mismatch"
        self.tag += 1
        self.n_units += 1
        w, bias = conv.weight, conv.bias
        wptr = self.pref(w)  # the f32 master [C][k*k] (the kernels round it for bf16 launches)
        geo = [B, x.H, x.W, Cc, conv.k, conv.stride, conv.padding, conv.dilation, dt]
        z = self.act(B, Ho, Wo, Cc, name + ".z") if (bn_spec is not None or relu) else y
        # (the unit follows ITS BatchNorm's flag, as conv_unit does)
        bn = _BNEmitter(self, bn_spec, Cc) if bn_spec is not None else None
        stats = self.zeroed_f32(N.stat_floats(Cc), "stats") if (bn is not None and bn_spec.training) else None
        self.emit(N.OP_DWCONV_FWD, [x.addr(), wptr, z.addr(), self.bp(stats) if stats is not None else None],
                  [x.ld, z.ld, 0] + geo)
        if bn is not None:
            if stats is not None:
                bn.finalize(stats, M)
            else:
                bn.eval_coeffs()
            self._act_apply(z, bn.cp[0], bn.cp[1], residual, y, relu)
        elif z is not y or bias is not None or residual is not None:
            # (biased conv -> activation: the unit-scale form of the normalise pass, shift = the bias)
            self._act_apply(z, None, self.pref(bias), residual, y, relu)
        if pool_out is not None:
            self.maxpool3x3s2(y, out=pool_out, name=name + ".max_pool")
        if self.need_grad:

            def bwd(dy):
                self.grad_add(residual, dy)
                if bn is not None:
                    sums, bcoef, dz = bn.bwd_buffers(y, name + ".dz")
                    bn.bwd_three_launches(dy, z, relu, sums, bcoef, dz)
                else:
                    dz = dy
                    if relu:  # dz = dy * act'(z + bias): the coefficient-free form reads the pre-activation it is given
                        zb = z
                        if bias is not None:  # act' is taken at z + bias: form it once
                            zb = self.act(B, Ho, Wo, Cc, name + ".zb")
                            self._act_apply(z, None, self.pref(bias), None, zb, 0)
                        dz = self.act(B, Ho, Wo, Cc, name + ".dz")
                        self._act_bwd(dy, zb, None, None, None, dz, relu)
                    if bias is not None and bias.requires_grad:
                        self.emit(N.OP_COLSUM, [dz.addr(), self.pgrad(bias)], [dz.ld, Cc, dt], [M])
                if w.requires_grad:
                    self.emit(N.OP_FORK)
                    self.emit(N.OP_DWCONV_WGRAD, [x.addr(), dz.addr(), self.pgrad(w)], [x.ld, dz.ld, 0] + geo, side=True)
                if x.needs_grad:
                    gx, res = self.grad_target(x)
                    self.emit(N.OP_DWCONV_DGRAD, [dz.addr(), wptr, gx.addr(), _addr(res)], [dz.ld, gx.ld, _ld(res)] + geo)
                    self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- grouped 3x3 units in one launch, and the Squeeze-Excitation MLP (vt_gconv.hip) -------------------------------
    GCONV3_WIDTHS = tuple(range(8, 65, 8))  # channels per group the one-launch kernels take

    def grouped3x3_unit(self, x: TRef, conv, norm, relu=1, out: Optional[TRef] = None, name: str = "gconv") -> TRef:
        """y = [relu](bn(conv(x))) for nn.Conv2d(C, C, 3, stride 1 | 2, padding 1, groups = C / gw, bias=False) with gw in
        GCONV3_WIDTHS -- the `f.b` unit of a RegNet block -- as ONE launch per pass over all groups: vt_gconv3_fwd (+ batch
        statistics) -> the ordinary BatchNorm finalize / normalise passes over all C channels; backward: the ordinary BatchNorm
        backward -> vt_gconv3_wgrad (side stream; slabs + an ordered reducer, so it is the same in deterministic mode) and
        vt_gconv3_dgrad.  ConvNormAct(groups=...) does not come here: it keeps _grouped_unit."""
        conv, bn_spec = self._specs(conv, norm)
        relu, dt, epc = int(relu), self.dtype, _EPC[self.dtype]
        Cc, G = conv.in_channels, conv.groups
        gw = Cc // max(G, 1)
        if ((conv.k, conv.padding, conv.dilation) != (3, 1, 1) or conv.stride not in (1, 2) or conv.out_channels != Cc or
                conv.bias is not None or bn_spec is None or Cc % max(G, 1)):
            raise NotImplementedError(f"{name}: the one-launch grouped unit is Conv2d(C, C, 3, stride 1 or 2, padding 1, groups, "
                                      "bias=False) -> BatchNorm2d")
        if gw not in self.GCONV3_WIDTHS:
            raise NotImplementedError(f"{name}: {gw} channels per group -- vt_gconv3_* take a multiple of 8 from 8 to 64")
        if x.logical_c != Cc or x.C != Cc:
            raise ValueError(f"{name}: conv expects {Cc} (unpadded) input channels, got {x.logical_c}")
        if relu >= 2:
            raise NotImplementedError(f"{name}: activation code {relu} (none or ReLU)")
        B, s = x.B, conv.stride
        Ho, Wo = conv.out_size(x.H, x.W)
        M = B * Ho * Wo
        y = out if out is not None else self.act(B, Ho, Wo, Cc, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (B, Ho, Wo, Cc), "out geometry mismatch"
        self.tag += 1
        self.n_units += 1
        w = conv.weight
        wptr = self.pref(w, mirror=dt != N.VT_F32)
        geo = [B, x.H, x.W, Cc, gw, s, dt]
        u = _ConvUnit(conv, relu, x, y, None, name, self.tag, wptr, None, 9 * gw)
        u.bn = bn = _BNEmitter(self, bn_spec, Cc)
        u.z = z = self.act(B, Ho, Wo, Cc, name + ".z")
        if bn_spec.training:
            stats = self.zeroed_f32(N.stat_floats(Cc), "stats")
            self.emit(N.OP_GCONV3_FWD, [x.addr(), wptr, z.addr(), self.bp(stats)], [x.ld, z.ld] + geo)
            if self.bn_fin_apply and not self.bn_sync:
                ptrs, flts = bn.finalize_operands(stats, M)
                self.emit(N.OP_BN_FIN_APPLY, ptrs + [z.addr(), None, y.addr()], [Cc, z.ld, 0, y.ld, relu, dt], flts + [M])
            else:
                bn.finalize(stats, M)
                self._act_apply(z, bn.cp[0], bn.cp[1], None, y, relu)
        else:
            self.emit(N.OP_GCONV3_FWD, [x.addr(), wptr, z.addr(), None], [x.ld, z.ld] + geo)
            bn.eval_coeffs()
            self._act_apply(z, bn.cp[0], bn.cp[1], None, y, relu)
        if self.need_grad:

            def bwd(dy):
                dz = self._bn_bwd(u, dy, None)
                if w.requires_grad:
                    nbytes = int(N.lib().vt_gconv3_wgrad_scratch_bytes(B, x.H, x.W, Cc, gw, s))
                    # (one scratch per size: every filter gradient of this kind runs on the one side stream, in order)
                    scratch = self._gconv_scratch.get(nbytes)
                    if scratch is None:
                        scratch = self._gconv_scratch[nbytes] = self.alloc(nbytes, "gconv_slabs")
                    self.emit(N.OP_FORK)
                    self.emit(N.OP_GCONV3_WGRAD, [x.addr(), dz.addr(), self.pgrad(w), self.bp(scratch)], [x.ld, dz.ld] + geo,
                              [nbytes], side=True)
                if x.needs_grad:
                    gx, res = self.grad_target(x)
                    self.emit(N.OP_GCONV3_DGRAD, [dz.addr(), wptr, gx.addr(), _addr(res)], [dz.ld, gx.ld, _ld(res)] + geo)
                    self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- tiled depthwise units (vt_dwtile.hip) --------------------------------------------------------------------------
    def depthwise_unit(self, x: TRef, conv, norm, act, out: Optional[TRef] = None, name: str = "dw",
                       pool_out: Optional[TRef] = None) -> TRef:
        """y = act(bn(conv(x))) for nn.Conv2d(C, C, k, stride, (k - 1) / 2, groups=C, bias=False) with k in {3, 5} and stride in
        {1, 2} -- the depthwise unit of a MobileNet block -- on the tiled kernels: vt_dwt_fwd (+ batch statistics) -> the ordinary
        BatchNorm finalize (or eval coefficients) -> the normalise pass with any activation code; backward: the ordinary BatchNorm
        backward -> vt_dwt_bwd (d(x) and the filter-gradient shares of the bands in one launch) -> vt_dwt_wgrad_reduce, both on
        the main stream (the shares scratch is one per size).  No float atomics: it is the same program in deterministic mode.
        ConvNormAct(groups=C) does not come here: it keeps _depthwise_unit.  A geometry the kernels do not take is refused.
        `pool_out`: a [B, 1, 1, C] row that receives the per-image mean of y from the normalise pass itself
        (vt_bn_act_avgpool_*: the Squeeze-Excitation pool of an MBConv block without another read of the expanded map); its
        gradient joins d(y) in f32 INSIDE the unit's BatchNorm backward (the addend of vt_bn_keep_bwd_*: adding it to the stored
        d(y) with the average pool's backward launch would lose it wherever it is below half an ulp of the rounded d(y), and
        costs a pass over the largest tensor of the block)."""
        conv, bn_spec = self._specs(conv, norm)
        act, dt, epc = int(act), self.dtype, _EPC[self.dtype]
        Cc, k, s = conv.in_channels, conv.k, conv.stride
        if conv.groups != Cc or conv.out_channels != Cc or conv.bias is not None or bn_spec is None:
            raise NotImplementedError(f"{name}: the tiled depthwise unit is Conv2d(C, C, k, groups=C, bias=False) -> BatchNorm2d")
        if k not in (3, 5) or s not in (1, 2) or conv.padding != (k - 1) // 2 or conv.dilation != 1:
            raise NotImplementedError(f"{name}: kernel_size={k}, stride={s}, padding={conv.padding}, dilation={conv.dilation} -- "
                                      "vt_dwt_* take kernel_size 3 or 5, stride 1 or 2, padding (k - 1) / 2, dilation 1")
        if Cc % epc:
            raise NotImplementedError(f"{name}: {Cc} channels must be a multiple of {epc} for dtype {dt}")
        if x.logical_c != Cc or x.C != Cc:
            raise ValueError(f"{name}: conv expects {Cc} (unpadded) input channels, got {x.logical_c}")
        if not 0 <= act <= 6:
            raise NotImplementedError(f"{name}: activation code {act}")
        B = x.B
        nbytes = int(N.lib().vt_dwt_shares_bytes(B, x.H, x.W, Cc, k, s, dt))
        if nbytes < 0:
            raise NotImplementedError(f"{name}: {N.last_error()}")
        Ho, Wo = conv.out_size(x.H, x.W)
        M = B * Ho * Wo
        y = out if out is not None else self.act(B, Ho, Wo, Cc, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (B, Ho, Wo, Cc), "out geometry mismatch"
        self.tag += 1
        self.n_units += 1
        w = conv.weight
        wptr = self.pref(w)  # the f32 master [C][k*k] (the kernels round it for bf16 launches)
        geo = [B, x.H, x.W, Cc, k, s, dt]
        bn = _BNEmitter(self, bn_spec, Cc)
        z = self.act(B, Ho, Wo, Cc, name + ".z")
        # (the unit follows ITS BatchNorm's flag, as conv_unit does)
        stats = self.zeroed_f32(N.stat_floats(Cc), "stats") if bn_spec.training else None
        self.emit(N.OP_DWT_FWD, [x.addr(), wptr, z.addr(), self.bp(stats) if stats is not None else None], [x.ld, z.ld] + geo)
        if pool_out is not None:
            if (pool_out.B, pool_out.H, pool_out.W, pool_out.C) != (B, 1, 1, Cc) or pool_out.logical_c != Cc:
                raise ValueError(f"{name}: pool_out is a [B, 1, 1, {Cc}] row per image")
            sb = int(N.lib().vt_bn_act_avgpool_scratch_bytes(B, Ho * Wo, Cc, dt))
            if sb < 0:
                raise NotImplementedError(f"{name}: the fused average pool does not take B={B}, HW={Ho * Wo}, C={Cc}")
            scratch = self.bp(self.zeroed_f32(sb // 4, "poolsums", bwd=False)) if sb else None
            pool_ints = [z.ld, y.ld, pool_out.ld, B, Ho * Wo]
        if pool_out is not None and stats is not None and self.bn_fin_apply and not self.bn_sync:
            ptrs, flts = bn.finalize_operands(stats, M)
            self.emit(N.OP_BN_ACT_AVGPOOL_FIN_APPLY, ptrs + [z.addr(), y.addr(), pool_out.addr(), scratch],
                      [Cc, *pool_ints, act, dt], flts)
        else:
            if stats is not None:
                bn.finalize(stats, M)
            else:
                bn.eval_coeffs()
            if pool_out is not None:
                self.emit(N.OP_BN_ACT_AVGPOOL_APPLY, [z.addr(), bn.cp[0], bn.cp[1], y.addr(), pool_out.addr(), scratch],
                          [*pool_ints, Cc, act, dt])
            else:
                self._act_apply(z, bn.cp[0], bn.cp[1], None, y, act)
        if self.need_grad:

            def bwd(dy):
                sums, bcoef, dz = bn.bwd_buffers(y, name + ".dz")
                dp = self.grad_read(pool_out) if pool_out is not None else None
                if dp is None:
                    bn.bwd_three_launches(dy, z, act, sums, bcoef, dz)
                else:  # g = (d(y) + d(pooled)[b][c] / HW) * act'(.)
                    HW = Ho * Wo
                    self.emit(N.OP_BN_KEEP_BWD_REDUCE, [dy.addr(), z.addr(), *bn.cp, self.bp(sums), None, dp.addr()],
                              [dy.ld, z.ld, HW, Cc, act, dt, dp.ld], [M])
                    if self.bn_fin_apply and not self.bn_sync:
                        self.emit(N.OP_BN_KEEP_BWD_FIN_APPLY,
                                  [self.bp(sums), *bn.cp, *bn.grads(), self.bp(bcoef), dy.addr(), z.addr(), dz.addr(), None, dp.addr()],
                                  [Cc, int(bn_spec.training), dy.ld, z.ld, dz.ld, HW, act, dt, dp.ld],
                                  [M * self.bn_world, 1.0 / self.bn_world, M])
                    else:
                        bn.bwd_finalize(sums, bcoef, M)
                        self.emit(N.OP_BN_KEEP_BWD_APPLY, [dy.addr(), z.addr(), bn.cp[1], self.bp(bcoef), dz.addr(), None, dp.addr()],
                                  [dy.ld, z.ld, dz.ld, HW, Cc, act, dt, dp.ld], [M])
                if not (w.requires_grad or x.needs_grad):
                    return
                # (one scratch per size: the launch that fills it and the one that reads it follow each other on one stream)
                scratch = self._dwt_scratch.get(nbytes)
                if scratch is None:
                    scratch = self._dwt_scratch[nbytes] = self.alloc(nbytes, "dwt_shares")
                if x.needs_grad:
                    gx, res = self.grad_target(x)
                else:  # (the launch always forms d(x))
                    gx, res = self.act(B, x.H, x.W, Cc, name + ".dx", needs_grad=False), None
                self.emit(N.OP_DWT_BWD, [dz.addr(), x.addr(), wptr, gx.addr(), _addr(res), self.bp(scratch)],
                          [dz.ld, x.ld, gx.ld, _ld(res)] + geo, [nbytes])
                if x.needs_grad:
                    self.grad_written(x)
                if w.requires_grad:
                    self.emit(N.OP_DWT_WGRAD_REDUCE, [self.bp(scratch), self.pgrad(w)], geo, [nbytes])

            self._node(y, bwd)
        return y

    def se_mlp(self, pooled: TRef, fc1: nn.Conv2d, fc2: nn.Conv2d, name: str = "se", act: int = 1) -> TRef:
        """The Squeeze-Excitation MLP on a pooled [B, 1, 1, C] row: fc2(relu(fc1(pooled))) with 1x1 biased convolutions of ANY
        squeeze width (RegNetY: round(0.25 * width_in) = 12, 26, 110 ..., no whole 16-byte chunks, which the 1x1 units need) in
        one launch (vt_se_mlp_fwd); the result is the operand `s` of se_gate.  Backward: vt_se_mlp_bwd (d(pooled) and the four
        parameter gradients, one owner per element).  The weights are read from the f32 masters.
        `act`: the squeeze activation, 1 ReLU or 3 SiLU (EfficientNet; `hidden` then also keeps the pre-activations, which
        silu' needs).  The code travels in an op field whose zero value means ReLU: act=1 emits the ops it always emitted."""
        act = int(act)
        if act not in (1, 3):
            raise NotImplementedError(f"{name}: squeeze activation code {act} (1 ReLU, 3 SiLU)")
        Cc, S = fc1.in_channels, fc1.out_channels
        if ((pooled.H, pooled.W, pooled.C) != (1, 1, Cc) or pooled.logical_c != Cc or fc2.in_channels != S or
                fc2.out_channels != Cc or fc1.kernel_size != (1, 1) or fc2.kernel_size != (1, 1) or fc1.bias is None or
                fc2.bias is None or fc1.groups != 1 or fc2.groups != 1):
            raise NotImplementedError(f"{name}: fc1 / fc2 are biased 1x1 convolutions C -> S -> C on a pooled [B, 1, 1, C] row")
        self.tag += 1
        B, dt = pooled.B, self.dtype
        logits = self.act(B, 1, 1, Cc, name + ".logits")
        hidden = self.f32(B * S * (2 if act == 3 else 1), name + ".hidden")
        code = [act] if act != 1 else []
        wts = [self.pref(fc1.weight), self.pref(fc1.bias), self.pref(fc2.weight), self.pref(fc2.bias)]
        self.emit(N.OP_SE_MLP_FWD, [pooled.addr(), *wts, self.bp(hidden), logits.addr()], [pooled.ld, logits.ld, B, Cc, S, dt] + code)
        if self.need_grad:

            def bwd(dl):
                gp = None
                if pooled.needs_grad:
                    gp, res = self.grad_target(pooled)
                    assert res is None and self._deferred_flush is None, "the pooled row has one consumer, the MLP"
                dhid = self.f32(B * S, name + ".dhidden")
                self.emit(N.OP_SE_MLP_BWD,
                          [dl.addr(), pooled.addr(), wts[0], wts[2], self.bp(hidden), self.bp(dhid), _addr(gp),
                           self.pgrad(fc1.weight), self.pgrad(fc1.bias), self.pgrad(fc2.weight), self.pgrad(fc2.bias)],
                          [dl.ld, pooled.ld, _ld(gp), B, Cc, S, dt] + code)

            self._node(logits, bwd)
        return logits

    # -- pointwise (1x1) units without stored pre-activations (vt_pointwise.hip) ------------------------------------
    def _unit_specs(self, specs) -> list:
        """(conv, norm, relu, residual, out, name) per unit, conv and norm as specs"""
        return [(*self._specs(sp[0], sp[1]), *sp[2:]) for sp in specs]

    def _pw_ok(self, x: TRef, specs) -> int:
        """0: the pointwise kernels do not apply to these units (reading the same x); 2: they do, filter gradient
        included; 1: they do, with dz handed to the filter-gradient kernel (vt_pw_supported)."""
        if not self.pointwise or self.dtype != N.VT_BF16 or not (1 <= len(specs) <= 2):
            return 0
        specs = self._unit_specs(specs)
        flags = set()
        for conv, bn, relu, residual, out, _ in specs:
            # (a slice: one group of a grouped convolution; LeakyReLU / SiLU / GELU: the unfused BatchNorm passes only)
            if (conv.is_slice or (conv.k, conv.stride, conv.padding, conv.dilation, conv.groups) != (1, 1, 0, 1, 1) or
                    conv.bias is not None or bn is None or conv.in_channels != x.C or x.logical_c != x.C or int(relu) >= 2):
                return 0
            flags.add((bn.training, bool(relu)))
        if len(flags) != 1 or len({sp[3] is None for sp in specs}) != 1:  # (a residual for every group or for none)
            return 0
        unit_training, _ = next(iter(flags))
        # (inference: the apply pass alone, with the running-statistics coefficients -- it streams x once at ~5.5 TB/s
        #  where the conv launch with the affine + ReLU epilogue stages it through LDS at ~2.7: 160 -> 160 @80x80 x 64
        #  images, 46 vs 91 us)
        if self.need_grad and not x.needs_grad:
            return 0  # (the backward kernel always forms dx)
        if x.M * x.C * 2 < self.pointwise_min_mb * 1e6:
            return 0
        cs = [sp[0].out_channels for sp in specs] + [0]
        mode = int(N.lib().vt_pw_supported(self.dtype, x.C, cs[0], cs[1]))
        if mode == 0 and len(specs) == 1 and not unit_training and not self.need_grad:
            # inference runs the apply pass alone: also on the 80-channel shapes of YOLOv5x's first stage
            mode = 1 if N.lib().vt_pw_apply_supported(self.dtype, x.C, cs[0]) else 0
        return mode

    def pw_units(self, x: TRef, specs) -> "list[TRef]":
        """one or two 1x1 ConvNormAct units reading the same tensor x (components.py:26-44; two: CSPDarknetStage's
        conv1 | conv2, darknet.py:46-47,53) as ONE launch per pass: statistics, normalise, backward reduction, backward
        apply with the data gradient and (small shapes) the filter gradient.  z and dz are never stored."""
        specs = self._unit_specs(specs)
        mode = self._pw_ok(x, specs)
        assert mode in (1, 2)
        self.tag += 1
        self.n_units += len(specs)
        G, Cs = len(specs), [sp[0].out_channels for sp in specs]
        Ntot, K, M = sum(Cs), x.C, x.M
        offs = [0, Cs[0]][:G]
        relu = bool(specs[0][2])
        unit_training = specs[0][1].training
        convs = [sp[0] for sp in specs]
        ys = []
        for (conv, _, _, residual, out, name), c in zip(specs, Cs):
            assert out is None or (out.B, out.H, out.W, out.C) == (x.B, x.H, x.W, c), "out geometry mismatch"
            assert residual is None or (residual.B, residual.H, residual.W, residual.C) == (x.B, x.H, x.W, c)
            ys.append(out if out is not None else self.act(x.B, x.H, x.W, c, name + ".y"))
        coef = self.f32(4 * Ntot, "bncoef4")  # scale | shift | mean | invstd over all groups' channels
        bns = [_BNEmitter(self, sp[1], c, cp=[self.bp(coef, (i * Ntot + o) * 4) for i in range(4)])
               for sp, c, o in zip(specs, Cs, offs)]
        wps = [self.pref(c.weight, mirror=True) for c in convs]
        pad2 = lambda v, fill=None: list(v) + [fill] * (2 - len(v))
        # the producer fold: x is a deferred output that this launch reads whole and whose filter gradient stays in the
        # kernel -- the passes read the producer's pre-activation and normalise it as they load (ptr[20]: its coefficient
        # rows, i[20]: its activation code), and the statistics pass finalizes its BatchNorm (ptr[5..10], f[1..3])
        prod = x.buf.deferred
        if prod is not None and not (mode == 2 and unit_training and not self.bn_sync and x.coff == 0 and
                                     x.ld == x.C == prod.u.y.C and not prod.finalized):
            prod = None
        xs = prod.u.z if prod is not None else x  # the tensor the passes read
        xa = xs.addr()  # (a deferred x that is not folded is materialised here)
        fold_p = lambda ptrs: ptrs + [None] * (20 - len(ptrs)) + [prod.u.bn.cp[0]] if prod is not None else ptrs
        fold_i = lambda ints: ints + [0] * (20 - len(ints)) + [prod.u.relu] if prod is not None else ints
        head_i = [K, G, int(relu)] + pad2(Cs, 0) + [xs.ld] + pad2([K] * G, 0)
        # the finalize step of every group inside the apply passes (vt_pw_fwd_apply_finalize / vt_pw_bwd_apply_finalize)
        pw_fin = self.bn_fin_apply and not self.bn_sync and Ntot <= 128
        fin_p = []
        if unit_training:
            stats = [self.zeroed_f32(N.stat_floats(c), "stats") for c in Cs]
            if prod is not None:
                pbn = prod.u.bn
                self.emit(N.OP_PW_STATS, fold_p([xa, *pad2(wps), *pad2([self.bp(s_) for s_ in stats]), self.bp(prod.stats),
                                                 *pbn.params, pbn.nbt]),
                          fold_i(head_i), [M, M * self.bn_world, pbn.spec.eps, pbn.spec.momentum])
                prod.finalized = True
            else:
                self.emit(N.OP_PW_STATS, [xa, *pad2(wps), *pad2([self.bp(s_) for s_ in stats])], head_i, [M])
            for bn, st in zip(bns, stats):
                if pw_fin:
                    fin_p += [self.bp(st), *bn.params, bn.nbt]
                else:
                    bn.finalize(st, M)
        else:
            for bn in bns:
                bn.eval_coeffs()
        ress = [sp[3] for sp in specs]
        apply_p = [xa, *pad2(wps), self.bp(coef), *pad2([y.addr() for y in ys]), *pad2([_addr(r) for r in ress])]
        apply_i = head_i + pad2([y.ld for y in ys], 0) + pad2([_ld(r) for r in ress], 0)
        if fin_p:
            epsmom = [v for bn in bns for v in (bn.spec.eps, bn.spec.momentum)]
            self.emit(N.OP_PW_APPLY_FIN, fold_p(apply_p + fin_p), fold_i(apply_i), [M, M * self.bn_world] + epsmom)
        else:
            self.emit(N.OP_PW_APPLY, fold_p(apply_p), fold_i(apply_i), [M])
        if self.need_grad:
            tag = self.tag

            def bwd():
                self.tag = tag
                dys = [self.grad_read(y) for y in ys]
                if all(d is None for d in dys):
                    return
                for g in range(G):
                    if dys[g] is None:  # a branch nothing back-propagates into: a zero gradient
                        z_ = self.act(x.B, x.H, x.W, Cs[g], specs[g][5] + ".dy0")
                        self.emit(N.OP_MEMSET, [z_.addr()], [0], [z_.buf.nbytes])
                        dys[g] = z_
                    if ress[g] is not None:
                        self.grad_add(ress[g], dys[g])
                sums = [self.zeroed_f32(N.stat_floats(c), "bwdsums") for c in Cs]
                dy_p, dy_ld = pad2([d.addr() for d in dys]), pad2([d.ld for d in dys], 0)
                self.emit(N.OP_PW_REDUCE, fold_p([xa, *pad2(wps), self.bp(coef), *dy_p, *pad2([self.bp(s_) for s_ in sums])]),
                          fold_i(head_i + dy_ld), [M])
                bcoefs = [self.f32(3 * c, "bwdcoef") for c in Cs]
                bfin_p = []
                for bn, sm, bc in zip(bns, sums, bcoefs):
                    if pw_fin:
                        bfin_p += [self.bp(sm), *bn.grads()]
                    else:
                        bn.bwd_finalize(sm, bc, M)
                gx, res = self.grad_target(x)
                # the only writer of the producer's d(y) (no addend, nothing left to add behind it): its sums too
                psums = None
                if prod is not None and self.pw_fold_bnred and res is None and self._deferred_flush is None:
                    psums = self.zeroed_f32(N.stat_floats(K), "bwdsums")
                fold_b = lambda ptrs: fold_p(ptrs) + [self.bp(psums)] if psums is not None else fold_p(ptrs)
                want_dw = [c.weight.requires_grad for c in convs]
                dws = [self.pgrad(c.weight) if (mode == 2 and w_) else None for c, w_ in zip(convs, want_dw)]
                dzs = [self.act(x.B, x.H, x.W, c, sp[5] + ".dz") if (mode == 1 and w_) else None
                       for c, sp, w_ in zip(Cs, specs, want_dw)]
                self.emit(N.OP_PW_BWD_FIN if bfin_p else N.OP_PW_BWD,
                          fold_b([xa, *pad2(wps), self.bp(coef), *dy_p, *pad2([self.bp(b_) for b_ in bcoefs]), gx.addr(),
                                  _addr(res), *pad2(dws), *pad2([_addr(d) for d in dzs]), *bfin_p]),
                          fold_i(head_i + dy_ld + [gx.ld, _ld(res)] + pad2([K] * G, 0) + pad2([_ld(d) for d in dzs], 0) +
                                 [int(unit_training)]),
                          [M, M * self.bn_world, 1.0 / self.bn_world])
                self.grad_written(x)
                self._gs(x).bn_sums = psums
                if mode == 1 and any(d is not None for d in dzs):
                    # the filter gradient does not fit the kernel's accumulators: dz was written, the usual kernel takes it
                    self.emit(N.OP_FORK)
                    for g, conv in enumerate(convs):
                        if dzs[g] is None:
                            continue
                        dfwd = self._conv_desc(x, Cs[g], x.H, x.W, 1, 0, 1, dzs[g].ld, K, 0)
                        self.emit(N.OP_CONV_WGRAD, [x.addr(), dzs[g].addr(), self.pgrad(conv.weight), None], desc=dfwd,
                                  extra_ints=[K, 0], side=True)

            self.nodes.append(bwd)
        return ys

    def conv_unit_pair(self, x: TRef, a, b):
        """two ConvNormAct units that read the same tensor (CSPDarknetStage.conv1 / conv2): one pointwise launch per
        pass when the kernels cover the joint shape, else two independent units.  a, b = (ConvNormAct, out, name)."""
        specs = [(m.conv, m.norm if isinstance(m.norm, nn.BatchNorm2d) else None, m._vt_relu(), None, out, name)
                 for m, out, name in (a, b)]
        if self._pw_ok(x, specs):  # (0 where either unit has no BatchNorm)
            return self.pw_units(x, specs)
        return [m._vt_emit(self, x, out=out, name=name) for m, out, name in (a, b)]

    def _wgrad_hold(self, key, xa, dza, dwa, desc, ldw):
        """hold a filter gradient back until its shape group is complete (or wgrad_group of them wait), then release the
        group as consecutive side-stream ops behind ONE fork (the executor gathers them: vt_conv_wgrad_group)."""
        pend = self._wg_pending.setdefault(key, [])
        pend.append((xa, dza, dwa, desc, ldw))
        self._wg_expect[key] -= 1
        if len(pend) >= self.wgrad_group or self._wg_expect[key] <= 0:
            self._wgrad_release(key)

    def _wgrad_release(self, key=None):
        for k_ in ([key] if key is not None else list(self._wg_pending)):
            pend = self._wg_pending.pop(k_, [])
            if not pend:
                continue
            side = not self.wgrad_inline
            if side:
                self.emit(N.OP_FORK)
            for xa, dza, dwa, desc, ldw in pend:
                self.emit(N.OP_CONV_WGRAD, [xa, dza, dwa, None], desc=desc, extra_ints=[ldw, 0], side=side)

    def _pack_dgrad(self, wptr, dst, ints):
        """a filter repacked for a data-gradient launch; on the forward list's side stream where the trainer asks for it
        (hoist_dgrad_packs)"""
        keep, hoist = self._cur, self.hoist_dgrad_packs
        self._cur = self._hoisted if hoist else keep
        self.emit(N.OP_PACK_DGRAD, [wptr, dst], ints, side=hoist)
        self._cur = keep

    def _dgrad_launch(self, dz: TRef, wd: Buf, gx: TRef, res: Optional[TRef], grid, cols, step, origin, taps, flags=0):
        """a stride-1 convolution over dz (tap offsets `taps`, `cols` output columns, `grid` output positions) written to the
        pixels origin + step * position of d(x)"""
        d = N.ConvDesc()
        d.dtype = self.dtype
        d.B, d.Hi, d.Wi, d.Cin, d.ldx = dz.B, dz.H, dz.W, dz.C, dz.ld
        d.Ho, d.Wo, d.sh, d.sw, d.h0, d.w0 = grid[0], grid[1], 1, 1, 0, 0
        d.Cout, d.ldy, d.oH, d.oW = cols, gx.ld, gx.H, gx.W
        d.oHs, d.oWs, d.oh0, d.ow0 = step, step, origin[0], origin[1]
        d.ldw, d.ldr = len(taps) * dz.C, _ld(res)
        d.flags = flags | (N.VT_CONV_RESIDUAL if res is not None else 0)
        d.ntaps = len(taps)
        for i, (a, b) in enumerate(taps):
            d.dh[i], d.dw[i] = a, b
        return self.emit(N.OP_CONV_IGEMM, [dz.addr(), self.bp(wd), gx.addr(), None, None, _addr(res), None], desc=d)

    def _dgrad(self, x: TRef, dz: TRef, wptr, ldw, conv: ConvSpec):
        dt, Cout = self.dtype, dz.C
        k, s, pad, dil = conv.k, conv.stride, conv.padding, conv.dilation
        # the s*s parity classes tile d(x) disjointly, so they share one destination and
        # one folded addend: every pixel is produced exactly once
        gx, res = self.grad_target(x)
        if (s == 2 and k == 3 and dil == 1 and pad == 1 and x.H % 2 == 0 and x.W % 2 == 0 and Cout <= self.dgrad_d2s_maxc and
                (4 * x.C) % (4 * _EPC[dt]) == 0 and dt == N.VT_BF16):
            # Every parity class (ph, pw) of d(x) reads dz at offsets {0, 1}^2 of its own grid position, so the four
            # are the column blocks of ONE 2x2-tap convolution over dz with 4*C output columns (zero taps where a
            # class has fewer), written depth-to-space: dz is read once instead of four times.  16/9 of the MFMA work,
            # which these layers (HBM-bound: few channels, large maps) do not notice.
            taps = [(1, 1), (1, 0), (0, 1), (0, 0)]  # the order a parity class lists its own taps in (below)
            wd = self.alloc(4 * x.C * 4 * Cout * _ESIZE[dt], "wd_d2s")
            for ph in range(2):
                for pw in range(2):
                    r0, t0 = (ph + pad) % s, (pw + pad) % s
                    rows, cols = list(range(r0, k, s)), list(range(t0, k, s))
                    eh, ew = (ph + pad - r0) // s, (pw + pad - t0) // s
                    sel = []
                    for (a, b) in taps:  # class tap (u, v) sits at offset (eh - u, ew - v)
                        u, v = eh - a, ew - b
                        sel.append(rows[u] * k + cols[v] if 0 <= u < len(rows) and 0 <= v < len(cols) else -1)
                    self._pack_dgrad(wptr, self.bp(wd, (2 * ph + pw) * x.C * 4 * Cout * _ESIZE[dt]),
                                     [dt, ldw, dt, 4, Cout, k * k, x.C, 0] + sel)
            self._dgrad_launch(dz, wd, gx, res, (x.H // 2, x.W // 2), 4 * x.C, 2, (0, 0), taps, N.VT_CONV_D2S)
            self.grad_written(x)
            return
        # A dilated strided convolution may never read some parity classes of its input (s = 2, dilation 2: the rows
        # 2i - 1 + 2r are all odd): those classes of d(x) are zero, i.e. the folded addend alone.  The whole of d(x) is
        # initialised first then (addend or zeros) and the classes that exist accumulate into it.
        if any(all((ph + pad - r * dil) % s for r in range(k)) for ph in range(s)):
            if res is None:
                zeros = self.act(x.B, x.H, x.W, x.C, "d0")
                self.emit(N.OP_MEMSET, [zeros.addr()], [0], [zeros.M * zeros.C * zeros.esize])
                self._add_into(gx, zeros, False)
            elif not (res.buf is gx.buf and res.coff == gx.coff):
                self._add_into(gx, res, False)
            res = gx
        for ph in range(s):
            for pw in range(s):
                # d(x)[ph + s*c] = sum over the filter rows r with (ph + pad - r*dil) divisible by s of
                # dz[c + (ph + pad - r*dil) / s] * w[r]  (columns alike): a stride-1 convolution over dz per parity class
                rows = [r for r in range(k) if (ph + pad - r * dil) % s == 0]
                cols = [t for t in range(k) if (pw + pad - t * dil) % s == 0]
                Hc = (x.H - ph + s - 1) // s
                Wc = (x.W - pw + s - 1) // s
                if Hc <= 0 or Wc <= 0 or not rows or not cols:  # (no rows / columns: initialised above)
                    continue
                sel = [r * k + t for r in rows for t in cols]
                offs = [((ph + pad - r * dil) // s, (pw + pad - t * dil) // s) for r in rows for t in cols]
                wd = self.alloc(x.C * len(sel) * Cout * _ESIZE[dt], "wd")
                self._pack_dgrad(wptr, self.bp(wd), [dt, ldw, dt, len(sel), Cout, k * k, x.C, 0] + sel)
                op = self._dgrad_launch(dz, wd, gx, res, (Hc, Wc), x.C, s, (ph, pw), offs)
                if s == 1 and res is None and Hc == x.H and Wc == x.W and self._cur is self.bwd:
                    self._last_dgrad[id(gx.buf)] = (op, gx.coff, gx.coff + gx.C)  # this launch alone forms d(x)
        self.grad_written(x)

    def copy(self, x: TRef, dst: TRef) -> TRef:
        """dst = x (places a tensor into a channel slice of a wider buffer)."""
        assert x.same_geom(dst)
        self.tag += 1
        self._add_into(dst, x, False)
        if self.need_grad and x.needs_grad:

            def bwd():
                g = self.grad_read(dst)
                if g is not None:
                    self.grad_add(x, g)

            self.nodes.append(bwd)
        return dst

    # -- pooling -------------------------------------------------------------------------
    def input_map(self, B, C_, H, W, name="in", requires_grad=True) -> TRef:
        """an NHWC feature map supplied by the caller (necks.py:83: the backbone's outputs)."""
        t = self.act(B, H, W, C_, name, needs_grad=requires_grad)
        idx = len(self.ext_inputs)
        self.ext_inputs.append(t)
        self.ext_grads.append(None)
        if requires_grad and self.need_grad:

            def bwd():  # first node appended => last to run: every contribution has been registered
                self.ext_grads[idx] = self.grad_read(t)

            self.nodes.append(bwd)
        return t

    def resample_add(self, src: TRef, other: Optional[TRef], mode: int, name="resample", out: Optional[TRef] = None) -> TRef:
        """nearest x2 (mode 0) / x0.5 (mode 1) or bilinear x2 (mode 2) / x0.5 (mode 3) resampling of `src` plus `other`
        (necks.py:66-81); `out`: write into this tensor (a channel slice of a concat buffer: fuse_fn="concat") instead of
        a fresh one."""
        self.tag += 1
        if mode in (0, 2):
            Hd, Wd = src.H * 2, src.W * 2
        else:
            if src.H % 2 or src.W % 2:
                raise NotImplementedError("x0.5 resampling of an odd-sized map")
            Hd, Wd = src.H // 2, src.W // 2
        if other is not None:
            assert (other.B, other.H, other.W, other.C) == (src.B, Hd, Wd, src.C), "fuse operands differ in shape"
        y = out if out is not None else self.act(src.B, Hd, Wd, src.C, name)
        assert (y.B, y.H, y.W, y.C) == (src.B, Hd, Wd, src.C)
        self.emit(N.OP_RESAMPLE_FWD, [src.addr(), _addr(other), y.addr()],
                  [src.ld, _ld(other), y.ld, src.B, Hd, Wd, src.C, mode, self.dtype])
        if self.need_grad and (src.needs_grad or (other is not None and other.needs_grad)):

            def bwd(dy):
                self.grad_add(other, dy)
                if not src.needs_grad:
                    return
                gx, acc = self.grad_accum_target(src)
                self.emit(N.OP_RESAMPLE_BWD, [dy.addr(), gx.addr()], [dy.ld, gx.ld, src.B, Hd, Wd, src.C, mode, acc, self.dtype])
                self.grad_written(src)

            self._node(y, bwd)
        return y

    def weighted_fuse(self, xs, codes, weights: nn.Parameter, eps: float, name: str = "wfuse") -> TRef:
        """BiFPN's fusion node (necks.py:210-215): out = (sum_i relu(w)_i R_i(x_i)) / (sum_i relu(w)_i + eps) over 2 or 3 maps
        in ONE launch (vt_wfuse_fwd); codes[i] relates xs[i] to the output grid: 0 same size, 1 nearest x2, 2 nearest x0.5.
        `weights` is the raw float[n] parameter, read on the device.  Backward: one launch (vt_wfuse_bwd) writes or
        accumulates every input's gradient -- a map of a BiFPN layer has up to three consumers, so each input gets its own
        accumulate flag -- and the fixed-point sums behind d(weights), which vt_wfuse_finalize adds to the parameter gradient."""
        xs, n = list(xs), len(xs)
        if n not in (2, 3) or len(codes) != n:
            raise NotImplementedError(f"{name}: weighted_fuse takes 2 or 3 inputs with one resample code each, got {n}")
        codes = [int(c) for c in codes]
        if any(c not in (0, 1, 2) for c in codes):
            raise NotImplementedError(f"{name}: resample codes {codes} (0 same size, 1 nearest x2, 2 nearest x0.5)")
        if weights.numel() != n:
            raise ValueError(f"{name}: {n} inputs but {weights.numel()} fusion weights")
        dt, epc = self.dtype, _EPC[self.dtype]
        B, Cc = xs[0].B, xs[0].C
        if Cc % epc:
            raise NotImplementedError(f"{name}: {Cc} channels must be a multiple of {epc} for dtype {dt} (whole 16-byte chunks)")
        for x, c in zip(xs, codes):
            if c == 2 and (x.H % 2 or x.W % 2):
                raise NotImplementedError(f"{name}: x0.5 resampling of an odd-sized map")
        sizes = [(x.H, x.W) if c == 0 else ((2 * x.H, 2 * x.W) if c == 1 else (x.H // 2, x.W // 2)) for x, c in zip(xs, codes)]
        H, W = sizes[0]
        if any(s != (H, W) for s in sizes) or any((x.B, x.C) != (B, Cc) for x in xs):
            raise ValueError(f"{name}: fused maps {[(x.B, x.C, x.H, x.W) for x in xs]} with codes {codes} do not meet on one grid "
                             "(levels must be an exact factor 2 apart)")
        if len({(id(x.buf), x.coff) for x in xs}) != n:
            raise ValueError(f"{name}: the same map is fused twice")
        self.tag += 1
        y = self.act(B, H, W, Cc, name + ".y")
        wp = self.pref(weights)
        x3, c3 = xs + [None] * (3 - n), codes + [0] * (3 - n)
        self.emit(N.OP_WFUSE_FWD, [_addr(x) for x in x3] + [wp, y.addr()],
                  [n, *[_ld(x) for x in x3], *c3, y.ld, B, H, W, Cc, dt], [eps])
        if self.need_grad and (weights.requires_grad or any(x.needs_grad for x in xs)):

            def bwd(dy):
                sums = self.zeroed_f32(N.channel_sums_floats(1, n), "wfsums")
                gxs, accs, flush = [], [], []
                for x in xs:
                    gx, acc = self.grad_accum_target(x) if x.needs_grad else (None, 0)
                    gxs.append(gx)
                    accs.append(acc)
                    # (grad_target keeps ONE deferred flush; this launch has up to three destinations)
                    if self._deferred_flush is not None:
                        flush.append(self._deferred_flush)
                        self._deferred_flush = None
                g3, a3 = gxs + [None] * (3 - n), accs + [0] * (3 - n)
                self.emit(N.OP_WFUSE_BWD, [dy.addr()] + [_addr(x) for x in x3] + [wp] + [_addr(g) for g in g3] + [self.bp(sums)],
                          [n, dy.ld, *[_ld(x) for x in x3], *c3, *[_ld(g) for g in g3], *a3, B, H, W, Cc, dt], [eps])
                for t in flush:
                    self._flush_pending(t)
                if self.pgrad(weights) is not None:
                    self.emit(N.OP_WFUSE_FIN, [self.bp(sums), wp, self.pgrad(weights)], [n], [eps])

            self._node(y, bwd)
        return y

    def maxpool3x3s2(self, x: TRef, out: Optional[TRef] = None, name="maxpool") -> TRef:
        self.tag += 1
        Ho, Wo = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
        y = out if out is not None else self.act(x.B, Ho, Wo, x.C, name)
        assert (y.B, y.H, y.W, y.C) == (x.B, Ho, Wo, x.C)
        am = self.alloc(x.B * Ho * Wo * x.C, "argmax")
        self.emit(N.OP_MAXPOOL_FWD, [x.addr(), y.addr(), self.bp(am)], [x.ld, y.ld, x.B, x.H, x.W, x.C, self.dtype])
        if self.need_grad and x.needs_grad:

            def bwd(dy):
                gx, acc = self.grad_accum_target(x)
                self.emit(N.OP_MAXPOOL_BWD, [dy.addr(), self.bp(am), gx.addr()],
                          [dy.ld, gx.ld, x.B, x.H, x.W, x.C, acc, self.dtype])
                self.grad_written(x)

            self._node(y, bwd)
        return y

    def spp(self, x: TRef, k: int, repeats: int, pool: str, out: Optional[TRef] = None, name: str = "spp") -> TRef:
        """SPPBlock (components.py:139-152): `repeats` cascaded Max/AvgPool2d(k, 1, (k-1)/2) and their concat over channels
        in ONE launch (vt_spp_fwd) that writes every stage into its channel slice of the output.  Backward: one launch
        (vt_spp_bwd) takes the gradient of the whole concatenated map and writes or accumulates d(x).  The winners' taps
        (one byte per element and stage, max only) are allocated only where a gradient is needed."""
        k, repeats = int(k), int(repeats)
        if pool not in ("max", "avg"):
            raise KeyError(pool)
        if not (3 <= k <= 15 and k % 2 == 1 and 1 <= repeats <= 4 and repeats * ((k - 1) // 2) <= 8):
            raise NotImplementedError(
                f"{name}: SPPBlock with kernel_size k={k} and repeats={repeats}: the MI355X path runs odd k in 3..15 (a winner's "
                "tap is one byte) with repeats in 1..4 and repeats*(k-1)/2 <= 8")
        epc = _EPC[self.dtype]
        if x.C % epc:
            raise NotImplementedError(f"{name}: {x.C} channels must be a multiple of {epc} for dtype {self.dtype} (whole 16-byte "
                                      "chunks)")
        self.tag += 1
        code = 0 if pool == "max" else 1
        y = out if out is not None else self.act(x.B, x.H, x.W, repeats * x.C, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (x.B, x.H, x.W, repeats * x.C)
        track = self.need_grad and x.needs_grad
        taps = self.alloc(repeats * x.B * x.H * x.W * x.C, name + ".taps") if track and code == 0 else None
        geom = [x.B, x.H, x.W, x.C, k, repeats, code, self.dtype]
        self.emit(N.OP_SPP_FWD, [x.addr(), y.addr(), self.bp(taps) if taps is not None else None], [x.ld, y.ld, *geom])
        if track:

            def bwd(dy):
                gx, acc = self.grad_accum_target(x)
                self.emit(N.OP_SPP_BWD, [dy.addr(), self.bp(taps) if taps is not None else None, gx.addr()],
                          [dy.ld, gx.ld, acc, *geom])
                self.grad_written(x)

            self._node(y, bwd)
        return y

    def deform_conv(self, x: TRef, conv_offset: nn.Conv2d, conv_mask: Optional[nn.Conv2d], conv, mask_act: int,
                    out: Optional[TRef] = None, name: str = "dcn") -> TRef:
        """DeformableConv2d (components.py:77-135).  `conv_offset` and `conv_mask` are ordinary conv units (no norm, no
        activation) that write the offset map and the raw mask logits in the compute dtype; their 2 k^2 and k^2 output
        channels run as the next whole 16-byte chunk over zero filter rows (ConvSpec.from_conv(out_channels=)), so the maps
        have logical_c < C and the deform kernels read them by leading dimension.  `conv` carries weight (Cout, Cin, k, k),
        bias and the geometry; `mask_act`: 0 identity, 1 sigmoid, applied inside the kernels.  Forward: vt_deform_fwd.
        Backward: vt_deform_wgrad (filter and bias, slabs + ordered reducer), then vt_deform_bwd, which writes d(offset) and
        d(mask logit) into the two units' output gradients (their padding channels are cleared first) and scatters d(x) with
        float atomics into an f32 plane that its flush pass writes or accumulates into d(x); the two units' data gradients
        join d(x) when their own backward runs.  Because of those atomics a deterministic builder refuses the block."""
        dt, epc = self.dtype, _EPC[self.dtype]
        k, s, pad, dil = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        Cin, Cout, K2 = conv.in_channels, conv.out_channels, conv.kernel_size[0] ** 2
        if self.deterministic:
            raise NotImplementedError(f"{name}: DeformableConv2d under a deterministic builder -- d(x) is scattered with float "
                                      "atomics (a fixed-point scatter is not built)")
        if k not in (1, 3) or conv.kernel_size[0] != conv.kernel_size[1]:
            raise NotImplementedError(f"{name}: DeformableConv2d with kernel_size={conv.kernel_size}: the MI355X path runs 1 and 3")
        if s not in (1, 2):
            raise NotImplementedError(f"{name}: DeformableConv2d with stride={s}: the MI355X path runs 1 and 2")
        if conv.groups != 1:
            raise NotImplementedError(f"{name}: DeformableConv2d with groups={conv.groups}: the MI355X path runs groups=1")
        if x.logical_c != Cin:
            raise ValueError(f"{name}: conv expects {Cin} input channels, got {x.logical_c}")
        if Cin % epc or x.C != Cin:
            raise NotImplementedError(f"{name}: DeformableConv2d with in_channels={Cin}: must be a multiple of {epc} for dtype {dt} "
                                      "(whole 16-byte chunks)")
        if Cout % epc:
            raise NotImplementedError(f"{name}: DeformableConv2d with out_channels={Cout}: must be a multiple of {epc} for dtype {dt} "
                                      "(whole 16-byte chunks)")
        padded = lambda c: ConvSpec.from_conv(c, out_channels=_round_up(c.out_channels, epc))
        off = self.conv_unit(x, padded(conv_offset), None, 0, name=name + ".conv_offset")
        off.logical_C = 2 * K2
        msk = None
        if conv_mask is not None:
            msk = self.conv_unit(x, padded(conv_mask), None, 0, name=name + ".conv_mask")
            msk.logical_C = K2
        self.tag += 1
        Ho, Wo = off.H, off.W
        y = out if out is not None else self.act(x.B, Ho, Wo, Cout, name + ".y")
        assert (y.B, y.H, y.W, y.C) == (x.B, Ho, Wo, Cout), "out geometry mismatch"
        w, bias = conv.weight, conv.bias
        wptr = self.pref(w, mirror=dt != N.VT_F32)
        geom = [x.B, x.H, x.W, Cin, Cout, k, s, pad, dil, int(mask_act), dt]
        self.emit(N.OP_DEFORM_FWD, [x.addr(), off.addr(), _addr(msk), wptr, self.pref(bias), y.addr()],
                  [x.ld, off.ld, _ld(msk), y.ld, *geom])
        if self.need_grad:

            def scratch(nbytes: int, what: str) -> Buf:
                # (one scratch per size: the launches that use it run on the main stream, in order)
                buf = self._deform_scratch.get(nbytes)
                if buf is None:
                    buf = self._deform_scratch[nbytes] = self.alloc(nbytes, what)
                return buf

            def bwd(dy):
                if w.requires_grad:
                    nbytes = int(N.lib().vt_deform_wgrad_scratch_bytes(x.B, x.H, x.W, Cin, Cout, k, s, pad, dil))
                    self.emit(N.OP_DEFORM_WGRAD,
                              [dy.addr(), x.addr(), off.addr(), _addr(msk), self.pgrad(w), self.pgrad(bias),
                               self.bp(scratch(nbytes, "deform_slabs"))], [dy.ld, x.ld, off.ld, _ld(msk), *geom], [nbytes])
                elif bias is not None and bias.requires_grad:
                    self.emit(N.OP_COLSUM, [dy.addr(), self.pgrad(bias)], [dy.ld, dy.C, dt], [y.M])
                grads = []
                for t in (off, msk):  # written whole: the logical channels by the kernel, the padding channels stay zero
                    if t is None:
                        grads.append(None)
                        continue
                    g, res = self.grad_target(t)
                    assert res is None, "the offset / mask maps have one consumer"
                    if t.logical_c != t.C:
                        self.emit(N.OP_MEMSET, [g.addr()], [0], [t.M * t.C * t.esize])
                    grads.append(g)
                gx, acc, plane = None, 0, None
                if x.needs_grad:
                    gx, acc = self.grad_accum_target(x)
                    plane = self.bp(scratch(x.M * Cin * 4, "deform_plane"))
                self.emit(N.OP_DEFORM_BWD,
                          [dy.addr(), x.addr(), off.addr(), _addr(msk), wptr, grads[0].addr(), _addr(grads[1]), _addr(gx), plane],
                          [dy.ld, x.ld, off.ld, _ld(msk), grads[0].ld, _ld(grads[1]), _ld(gx), acc, *geom])
                if x.needs_grad:
                    self.grad_written(x)
                for t in (off, msk):
                    if t is not None:
                        self.grad_written(t)

            self._node(y, bwd)
        return y

    def global_avgpool(self, x: TRef, name="avgpool") -> TRef:
        """[B,H,W,C] -> [B,1,1,C]"""
        self.tag += 1
        y = self.act(x.B, 1, 1, x.C, name)
        self.emit(N.OP_AVGPOOL_FWD, [x.addr(), y.addr()], [x.ld, y.ld, x.B, x.H * x.W, x.C, self.dtype])
        if self.need_grad and x.needs_grad:

            def bwd(dy):
                gx, acc = self.grad_accum_target(x)
                self.emit(N.OP_AVGPOOL_BWD, [dy.addr(), gx.addr()], [dy.ld, gx.ld, x.B, x.H * x.W, x.C, acc, self.dtype])
                self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- ConvNeXt pieces (reference backbones/convnext.py:44-58): vt_layernorm.hip ----------------------
    def linear_unit(self, x: TRef, linear: nn.Linear, act: int = 0, name: str = "linear") -> TRef:
        """nn.Linear over the channel axis of an NHWC map = a biased 1x1 convolution (+ activation code `act`)."""
        return self.conv_unit(x, ConvSpec.from_linear(linear), None, act, name=name)

    def depthwise_no_bias(self, x: TRef, conv: nn.Conv2d, name: str = "dwconv") -> TRef:
        """a depthwise nn.Conv2d emitted WITHOUT its bias: the LayerNorm behind it adds the bias while it reads the row
        (layer_norm(pre_bias=conv.bias)) instead of one more read + write pass over the map."""
        if conv.groups != conv.in_channels or conv.in_channels != conv.out_channels:
            raise NotImplementedError("depthwise_no_bias: groups = in_channels = out_channels")
        return self.conv_unit(x, ConvSpec.from_conv(conv).without_bias(), None, 0, name=name)

    def layer_norm(self, x: TRef, ln: nn.LayerNorm, pre_bias: Optional[nn.Parameter] = None, out: Optional[TRef] = None,
                   name: str = "ln") -> TRef:
        """y = LayerNorm_C(x + pre_bias) over the channel axis of every pixel (vt_layernorm_fwd); backward in one launch
        (vt_layernorm_bwd: statistics recomputed from x, d gamma / d beta / d pre_bias through a fixed-point channel-sums
        buffer that vt_channel_sums_to_f32 adds to the gradients)."""
        if tuple(ln.normalized_shape) != (x.C,) or not ln.elementwise_affine or ln.bias is None:
            raise NotImplementedError(f"{name}: LayerNorm({ln.normalized_shape}) over a {x.C}-channel map with weight and bias")
        if x.logical_c != x.C:
            raise NotImplementedError(f"{name}: LayerNorm over a channel-padded map")
        if x.C % _EPC[self.dtype]:
            raise NotImplementedError(f"{name}: {x.C} channels must be a multiple of {_EPC[self.dtype]} for dtype {self.dtype}")
        self.tag += 1
        dt = self.dtype
        y = out if out is not None else self.act(x.B, x.H, x.W, x.C, name + ".y")
        assert y.same_geom(x), "out geometry mismatch"
        pb = self.pref(pre_bias)
        gm = self.pref(ln.weight)
        self.emit(N.OP_LAYERNORM_FWD, [x.addr(), pb, gm, self.pref(ln.bias), y.addr()], [x.ld, y.ld, x.C, dt], [x.M, ln.eps])
        if self.need_grad:

            def bwd(dy):
                sums = self.zeroed_f32(N.channel_sums_floats(3, x.C), "lnsums")
                if x.needs_grad:
                    gx, res = self.grad_target(x)
                else:
                    gx, res = self.act(x.B, x.H, x.W, x.C, name + ".dx"), None
                self.emit(N.OP_LAYERNORM_BWD, [dy.addr(), x.addr(), pb, gm, gx.addr(), _addr(res), self.bp(sums)],
                          [dy.ld, x.ld, gx.ld, _ld(res), x.C, dt], [x.M, ln.eps])
                if x.needs_grad:
                    self.grad_written(x)
                dsts = [self.pgrad(ln.weight), self.pgrad(ln.bias), self.pgrad(pre_bias)]
                if any(d is not None for d in dsts):
                    self.emit(N.OP_CHANNEL_SUMS, [self.bp(sums)] + dsts, [3, x.C])

            self._node(y, bwd)
        return y

    def scale_residual(self, t: TRef, gamma: Optional[nn.Parameter], residual: TRef, out: Optional[TRef] = None,
                       name: str = "scale_residual") -> TRef:
        """y = residual + gamma * t (LayerScale + shortcut; gamma None: the plain add).  Backward: the shortcut's gradient is
        d(y) itself (grad_add), d(t) = d(y) * gamma and d gamma = sum_pixels d(y) * t in one launch (vt_scale_residual_bwd)."""
        assert t.same_geom(residual)
        self.tag += 1
        dt = self.dtype
        y = out if out is not None else self.act(t.B, t.H, t.W, t.C, name + ".y")
        gm = self.pref(gamma)
        self.emit(N.OP_SCALE_RES_FWD, [t.addr(), gm, residual.addr(), y.addr()], [t.ld, residual.ld, y.ld, t.C, dt], [t.M])
        if self.need_grad:

            def bwd(dy):
                self.grad_add(residual, dy)
                if gamma is None:
                    self.grad_add(t, dy)
                    return
                sums = self.zeroed_f32(N.channel_sums_floats(1, t.C), "lssums")
                gt, res = self.grad_target(t)
                assert res is None, "a LayerScale input has one consumer"
                self.emit(N.OP_SCALE_RES_BWD, [dy.addr(), t.addr(), gm, gt.addr(), self.bp(sums)],
                          [dy.ld, t.ld, gt.ld, t.C, dt], [t.M])
                self.grad_written(t)
                if self.pgrad(gamma) is not None:
                    self.emit(N.OP_CHANNEL_SUMS, [self.bp(sums), self.pgrad(gamma)], [1, t.C])

            self._node(y, bwd)
        return y

    # -- MLP-Mixer pieces (reference backbones/mlp_mixer.py:28,34,52,60): vt_token_mix.hip ---------------------
    def patch_embed(self, x: TRef, conv: nn.Conv2d, name: str = "patch_embed") -> TRef:
        """a p x p stride-p nn.Conv2d over the image as a patch gather (vt_patchify_fwd) and ONE Linear over the
        Cin * p * p values of a patch: a 16 x 16 patch is 256 taps, which the convolution descriptor (VT_MAX_TAPS, 8-bit
        tap offsets) does not take.  The gather orders a patch row (py, px, c), the order of the channels_last filter
        image [d_model][p][p][Cin], so the filter is read as it lies (bf16: in the mirror).  Backward scatters into the
        image gradient only where the image requires one."""
        p = conv.kernel_size[0]
        if (tuple(conv.kernel_size) != (p, p) or tuple(conv.stride) != (p, p) or tuple(conv.padding) != (0, 0) or
                tuple(conv.dilation) != (1, 1) or conv.groups != 1):
            raise NotImplementedError(f"{name}: a patch embedding is a p x p convolution with stride p, no padding, groups = 1")
        cin, dt = conv.in_channels, self.dtype
        if x.logical_c != cin:
            raise ValueError(f"{name}: conv expects {cin} input channels, got {x.logical_c}")
        if x.H % p or x.W % p:
            raise ValueError(f"{name}: a {x.H}x{x.W} image is no whole number of {p}x{p} patches")
        rows = cin * p * p
        if rows % _EPC[dt]:
            raise NotImplementedError(f"{name}: {cin} * {p} * {p} = {rows} values per patch must be a multiple of {_EPC[dt]} "
                                      f"for dtype {dt}")
        patches = self._patchify(x, cin, p, name)
        return self.conv_unit(patches, ConvSpec(1, 1, 0, 1, 1, rows, conv.out_channels, conv.weight, conv.bias), None, 0, name=name)

    def _patchify(self, x: TRef, cin: int, p: int, name: str) -> TRef:
        """the p x p patches of the first `cin` channels of x as rows in (py, px, c) order: [B, H, W, C] -> [B, H/p, W/p,
        cin p p] (vt_patchify_fwd); backward scatters them back (vt_patchify_bwd)"""
        self.tag += 1
        B, H, W, dt = x.B, x.H, x.W, self.dtype
        patches = self.act(B, H // p, W // p, cin * p * p, name + ".patches", needs_grad=x.needs_grad)
        self.emit(N.OP_PATCHIFY_FWD, [x.addr(), patches.addr()], [x.ld, patches.ld, B, H, W, cin, p, dt])
        if self.need_grad and x.needs_grad:

            def bwd(dp):
                gx, res = self.grad_target(x)
                self.emit(N.OP_PATCHIFY_BWD, [dp.addr(), gx.addr(), _addr(res)], [dp.ld, gx.ld, _ld(res), B, H, W, cin, x.C, p, dt])
                self.grad_written(x)

            self._node(patches, bwd)
        return patches

    def _token_slab(self, nbytes: int) -> Buf:
        """slab scratch of the token filter gradients: one per size, shared by every layer of that shape (their launches
        follow each other on one stream)"""
        if nbytes not in self._tok_slabs:
            self._tok_slabs[nbytes] = self.alloc(nbytes, "token_wgrad_slabs")
        return self._tok_slabs[nbytes]

    def token_linear(self, x: TRef, linear: nn.Linear, act: int = 0, residual: Optional[TRef] = None,
                     out: Optional[TRef] = None, name: str = "token_linear") -> TRef:
        """nn.Linear over the TOKEN axis of a map: y[b, m, c] = sum_k W[m, k] x[b, k, c] + bias[m], tokens k = the H * W
        pixels of x (vt_token_mix_fwd; the reference transposes the map, applies the Linear and transposes back).  `act`
        (0, or 4 = exact GELU): the launch writes the pre-activation AND its activation; `residual`: y = residual + ...,
        in the residual's geometry.  Without a residual y is [B, M, 1, C].  Backward: the stored pre-activation through
        the activation backward pass, vt_token_mix_wgrad (filter and bias gradient, order-free in every mode) on the
        filter-gradient stream, and the same forward kernel over W^T for the data gradient, which folds one addend."""
        K, M, dt = x.H * x.W, linear.out_features, self.dtype
        if linear.in_features != K:
            raise ValueError(f"{name}: Linear expects {linear.in_features} tokens, the map has {x.H}x{x.W} = {K}")
        if x.logical_c != x.C or x.C % _EPC[dt]:
            raise NotImplementedError(f"{name}: {x.C} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        if act not in (0, 4):
            raise NotImplementedError(f"{name}: activation code {act} (token mixing implements none and exact GELU)")
        if act and residual is not None:
            raise NotImplementedError(f"{name}: an activation and a residual in one launch")
        self.tag += 1
        B, Cc = x.B, x.C
        Hy, Wy = (residual.H, residual.W) if residual is not None else (M, 1)
        if residual is not None and (residual.B, residual.H * residual.W, residual.C) != (B, M, Cc):
            raise ValueError(f"{name}: residual geometry does not match the {M}-token output")
        y = out if out is not None else self.act(B, Hy, Wy, Cc, name + ".y")
        assert (y.B, y.H * y.W, y.C) == (B, M, Cc), "out geometry mismatch"
        w, bias = linear.weight, linear.bias
        # (bf16: from the mirror, like every other GEMM weight -- what the sharded exchange refreshes on every rank)
        wptr = self.pref(w, mirror=True) if dt == N.VT_BF16 else self.pref(w)
        track = self.need_grad
        z = self.act(B, Hy, Wy, Cc, name + ".z") if (act and track) else None
        o1, o2 = (z, y) if act else (y, None)  # (with an activation: the pre-activation, where backward needs it, and y)
        self.emit(N.OP_TOKEN_MIX, [x.addr(), wptr, self.pref(bias), _addr(residual), _addr(o1), _addr(o2)],
                  [x.ld, K, 0, _ld(residual), _ld(o1), _ld(o2), act, B, K, M, Cc, dt])
        if track:

            def bwd(dy):
                self.grad_add(residual, dy)
                dz = dy
                if act:  # dz = dy * act'(z)
                    dz = self.act(B, Hy, Wy, Cc, name + ".dz")
                    self._act_bwd(dy, z, None, None, None, dz, act)
                dw, db = self.pgrad(w), self.pgrad(bias)
                if dw is not None or db is not None:
                    nbytes = int(N.lib().vt_token_mix_wgrad_scratch_bytes(B, K, M, Cc, dt))
                    slab = self._token_slab(nbytes)
                    self.emit(N.OP_FORK)
                    self.emit(N.OP_TOKEN_WGRAD, [dz.addr(), x.addr(), dw, db, self.bp(slab)], [dz.ld, x.ld, B, K, M, Cc, dt],
                              [nbytes], side=True)
                if x.needs_grad:
                    gx, res = self.grad_target(x)
                    self.emit(N.OP_TOKEN_MIX, [dz.addr(), wptr, None, _addr(res), gx.addr(), None],
                              [dz.ld, K, 1, _ld(res), gx.ld, 0, 0, B, M, K, Cc, dt])
                    self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- ViT pieces (reference backbones/vit.py:34-46, 145-151): vt_attention.hip ---------------------------------
    def attention(self, q: TRef, k: TRef, v: TRef, n_heads: int, name: str = "attention") -> TRef:
        """softmax(q k^T / sqrt(head_dim)) v per (image, head) on token maps [B, 1, L, C] (tokens along W), head h = the
        channel slice [h head_dim, (h + 1) head_dim) -- q, k and v may be channel slices of one buffer, nothing is
        transposed (vt_attn_fwd; it also writes the row log-sum-exp the backward needs).  Backward: one vt_attn_bwd
        writes d(q), d(k) and d(v) into the gradient buffers of the three producers; it has no atomics, so it is the
        same launch under `deterministic`."""
        dt = self.dtype
        if not (q.same_geom(k) and q.same_geom(v)) or q.H != 1:
            raise ValueError(f"{name}: q, k and v are [B, 1, L, C] token maps of one geometry")
        if n_heads <= 0 or q.C % n_heads:
            raise ValueError(f"{name}: {q.C} channels do not split into n_heads={n_heads}")
        D = q.C // n_heads
        if D not in (32, 64):
            raise NotImplementedError(f"{name}: head_dim = {q.C} / n_heads={n_heads} = {D}: the attention kernels implement "
                                      "head_dim 32 and 64")
        if any(t.logical_c != t.C for t in (q, k, v)) or q.C % _EPC[dt]:
            raise NotImplementedError(f"{name}: {q.C} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        self.tag += 1
        B, L, scale = q.B, q.W, D ** -0.5
        o = self.act(B, 1, L, q.C, name + ".o")
        lse = self.f32(B * n_heads * L, name + ".lse")
        self.emit(N.OP_ATTN_FWD, [q.addr(), k.addr(), v.addr(), o.addr(), self.bp(lse)],
                  [q.ld, k.ld, v.ld, o.ld, B, n_heads, L, D, dt], [scale])
        if self.need_grad and (q.needs_grad or k.needs_grad or v.needs_grad):

            def bwd(do):
                nbytes = int(N.lib().vt_attn_bwd_scratch_bytes(B, n_heads, L))
                if nbytes not in self._attn_scratch:  # (delta: one per size, the launches follow each other on one stream)
                    self._attn_scratch[nbytes] = self.alloc(nbytes, "attn_delta")
                gs = []
                for t in (q, k, v):
                    g = None
                    if t.needs_grad:
                        g, res = self.grad_target(t)
                        assert res is None and self._deferred_flush is None, "q, k and v have one consumer, the attention"
                    gs.append(g)
                self.emit(N.OP_ATTN_BWD,
                          [q.addr(), k.addr(), v.addr(), o.addr(), do.addr(), self.bp(lse), *[_addr(g) for g in gs],
                           self.bp(self._attn_scratch[nbytes])],
                          [q.ld, k.ld, v.ld, o.ld, do.ld, *[_ld(g) for g in gs], B, n_heads, L, D, dt], [scale, nbytes])

            self._node(o, bwd)
        return o

    # -- Swin pieces (reference backbones/swin.py:32-124): vt_window_attention.hip ---------------------------------
    def window_attention(self, q: TRef, k: TRef, v: TRef, n_heads: int, table: nn.Parameter, ws: int, shift: int,
                         name: str = "window_attention") -> TRef:
        """softmax(q k^T / sqrt(head_dim) + table[relative index] (+ the -100 region mask where shift > 0)) v inside the
        ws x ws windows of [B, H, W, C] maps, cyclically shifted by `shift` (vt_win_attn_fwd).  The partition and both rolls
        are index arithmetic of the kernel: q, k, v and o are maps in un-rolled pixel order, head h a channel slice, and q,
        k, v may be channel slices of one buffer.  `table` is the (1, n_heads, (2 ws - 1)^2) parameter, read as the f32
        master.  Backward: one vt_win_attn_bwd writes d(q), d(k), d(v) into the gradient buffers of the three producers
        and adds the table's gradient, summed in a fixed order through a scratch that every layer of the same size shares:
        no atomics, the same launch under `deterministic`."""
        dt = self.dtype
        if not (q.same_geom(k) and q.same_geom(v)):
            raise ValueError(f"{name}: q, k and v are [B, H, W, C] maps of one geometry")
        if n_heads <= 0 or q.C % n_heads:
            raise ValueError(f"{name}: {q.C} channels do not split into n_heads={n_heads}")
        D = q.C // n_heads
        if D != 32:
            raise NotImplementedError(f"{name}: head_dim = {q.C} / n_heads={n_heads} = {D}: the window attention kernels "
                                      "implement head_dim 32")
        if ws * ws > 64:
            raise NotImplementedError(f"{name}: window_size={ws}: a window of {ws * ws} tokens does not fit the kernels' 64-row "
                                      "tile (window_size <= 8)")
        if q.H % ws or q.W % ws or not 0 <= shift < ws:
            raise ValueError(f"{name}: a {q.H}x{q.W} map, window_size={ws}, shift={shift}")
        if table.numel() != n_heads * (2 * ws - 1) ** 2:
            raise ValueError(f"{name}: the table holds {table.numel()} values, {n_heads} heads x (2 * {ws} - 1)^2 are expected")
        if any(t.logical_c != t.C for t in (q, k, v)) or q.C % _EPC[dt]:
            raise NotImplementedError(f"{name}: {q.C} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        self.tag += 1
        B, H, W, scale = q.B, q.H, q.W, D ** -0.5
        o = self.act(B, H, W, q.C, name + ".o")
        lse = self.f32(B * n_heads * H * W, name + ".lse")
        tb = self.pref(table)
        geom = [B, H, W, n_heads, D, ws, shift, dt]
        self.emit(N.OP_WIN_ATTN_FWD, [q.addr(), k.addr(), v.addr(), o.addr(), self.bp(lse), tb], [q.ld, k.ld, v.ld, o.ld, *geom],
                  [scale])
        if self.need_grad and (q.needs_grad or k.needs_grad or v.needs_grad or self.pgrad(table) is not None):

            def bwd(do):
                nbytes = int(N.lib().vt_win_attn_bwd_scratch_bytes(B, H, W, n_heads, ws))
                if nbytes not in self._win_scratch:  # (one per size: the launches follow each other on one stream)
                    self._win_scratch[nbytes] = self.alloc(nbytes, "win_attn_dtable_shares")
                gs = []
                for t in (q, k, v):
                    g = None
                    if t.needs_grad:
                        g, res = self.grad_target(t)
                        assert res is None and self._deferred_flush is None, "q, k and v have one consumer, the attention"
                    gs.append(g)
                self.emit(N.OP_WIN_ATTN_BWD,
                          [q.addr(), k.addr(), v.addr(), o.addr(), do.addr(), self.bp(lse), tb, *[_addr(g) for g in gs],
                           self.pgrad(table), self.bp(self._win_scratch[nbytes])],
                          [q.ld, k.ld, v.ld, o.ld, do.ld, *[_ld(g) for g in gs], *geom], [scale, nbytes])

            self._node(o, bwd)
        return o

    def patch_merging(self, x: TRef, norm: nn.LayerNorm, reduction: nn.Linear, name: str = "patch_merging") -> TRef:
        """Swin's PatchMerging: the 2 x 2 neighbourhoods of [B, H, W, C] as [B, H/2, W/2, 4 C] rows in (dy, dx, c) order (the
        patch gather with p = 2 -- the order of the reference's view / transpose / flatten), LayerNorm(4 C), then the
        bias-free Linear(4 C, 2 C) as a 1x1 convolution."""
        if x.logical_c != x.C or x.H % 2 or x.W % 2:
            raise ValueError(f"{name}: a {x.H}x{x.W} map of {x.logical_c} channels does not merge 2 x 2")
        if reduction.bias is not None or reduction.in_features != 4 * x.C:
            raise NotImplementedError(f"{name}: the reduction is a bias-free Linear({4 * x.C}, .)")
        g = self._patchify(x, x.C, 2, name)
        n = self.layer_norm(g, norm, name=name + ".norm")
        return self.conv_unit(n, ConvSpec.from_linear(reduction), None, 0, name=name + ".reduction")

    def vit_tokens(self, embed: TRef, pe: nn.Parameter, cls_token: Optional[nn.Parameter], name: str = "tokens") -> TRef:
        """the token map of a ViT: [B, gh, gw, C] patch embeddings + pe, behind the class token where there is one ->
        [B, 1, L, C] (vt_vit_tokens_fwd; the token is broadcast over the batch).  Backward copies the patch rows into
        d(embed) and sums d(pe) / d(cls_token) over the batch in a fixed order (vt_vit_tokens_bwd)."""
        T, Cc, dt = embed.H * embed.W, embed.C, self.dtype
        if embed.logical_c != Cc or pe.numel() != T * Cc:
            raise ValueError(f"{name}: pe holds {pe.numel()} values, the {embed.H}x{embed.W} map of {Cc} channels {T * Cc}")
        if cls_token is not None and cls_token.numel() != Cc:
            raise ValueError(f"{name}: cls_token holds {cls_token.numel()} values for {Cc} channels")
        self.tag += 1
        B, c0 = embed.B, int(cls_token is not None)
        y = self.act(B, 1, T + c0, Cc, name + ".y")
        self.emit(N.OP_VIT_TOKENS_FWD, [embed.addr(), self.pref(pe), self.pref(cls_token), y.addr()], [embed.ld, y.ld, B, T, Cc, dt])
        if self.need_grad:

            def bwd(dy):
                ge = None
                if embed.needs_grad:
                    ge, res = self.grad_target(embed)
                    assert res is None and self._deferred_flush is None, "the patch embedding has one consumer"
                dpe, dcls = self.pgrad(pe), self.pgrad(cls_token)
                if ge is None and dpe is None and dcls is None:
                    return
                self.emit(N.OP_VIT_TOKENS_BWD, [dy.addr(), _addr(ge), dpe, dcls], [dy.ld, _ld(ge), c0, B, T, Cc, dt])

            self._node(y, bwd)
        return y

    def token_select(self, x: TRef, t0: int, name: str = "token_select") -> TRef:
        """token t0 of every image of a [B, 1, L, C] map -> [B, 1, 1, C] (class-token pooling: `out[:, 0]`).  Backward writes
        the row and zeros elsewhere, or adds the row to a gradient that is already there."""
        if x.H != 1 or not 0 <= t0 < x.W:
            raise ValueError(f"{name}: token {t0} of a [B, {x.H}, {x.W}, C] map")
        self.tag += 1
        y = self.act(x.B, 1, 1, x.C, name + ".y")
        self.emit(N.OP_TOKEN_SELECT_FWD, [x.addr(), y.addr()], [x.ld, y.ld, x.B, x.W, t0, x.C, self.dtype])
        if self.need_grad and x.needs_grad:

            def bwd(dy):
                gx, acc = self.grad_accum_target(x)
                self.emit(N.OP_TOKEN_SELECT_BWD, [dy.addr(), gx.addr()], [dy.ld, gx.ld, acc, x.B, x.W, t0, x.C, self.dtype])
                self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- DeiT pieces (reference backbones/deit.py:37-41): vt_prefix_tokens.hip ------------------------------------------
    def prefix_tokens(self, embed: TRef, pe: nn.Parameter, prefix_params, name: str = "tokens") -> TRef:
        """the token map of a DeiT: P learned rows (parameters of C values, read as f32 masters, broadcast over the batch, no
        position) in front of the [B, gh, gw, C] patch embeddings + pe -> [B, 1, P + T, C] (vt_prefix_tokens_fwd).  Backward
        copies the patch rows into d(embed) and sums d(pe) and every d(prefix) over the batch in a fixed order
        (vt_prefix_tokens_bwd), as vit_tokens does for its one row."""
        T, Cc, dt = embed.H * embed.W, embed.C, self.dtype
        prefix_params = list(prefix_params)
        P = len(prefix_params)
        if not 1 <= P <= 4:
            raise ValueError(f"{name}: {P} prefix tokens (1..4)")
        if embed.logical_c != Cc or pe.numel() != T * Cc:
            raise ValueError(f"{name}: pe holds {pe.numel()} values, the {embed.H}x{embed.W} map of {Cc} channels {T * Cc}")
        for k, p in enumerate(prefix_params):
            if p.numel() != Cc:
                raise ValueError(f"{name}: prefix token {k} holds {p.numel()} values for {Cc} channels")
        if Cc % _EPC[dt]:
            raise NotImplementedError(f"{name}: {Cc} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        self.tag += 1
        B = embed.B
        pad = [None] * (4 - P)
        y = self.act(B, 1, P + T, Cc, name + ".y")
        self.emit(N.OP_PREFIX_TOKENS_FWD, [embed.addr(), self.pref(pe), y.addr()] + [self.pref(p) for p in prefix_params] + pad,
                  [embed.ld, y.ld, P, B, T, Cc, dt])
        if self.need_grad:

            def bwd(dy):
                ge = None
                if embed.needs_grad:
                    ge, res = self.grad_target(embed)
                    assert res is None and self._deferred_flush is None, "the patch embedding has one consumer"
                dpe, dpre = self.pgrad(pe), [self.pgrad(p) for p in prefix_params]
                if ge is None and dpe is None and all(d is None for d in dpre):
                    return
                self.emit(N.OP_PREFIX_TOKENS_BWD, [dy.addr(), _addr(ge), dpe] + dpre + pad, [dy.ld, _ld(ge), P, B, T, Cc, dt])

            self._node(y, bwd)
        return y

    def prefix_pool(self, x: TRef, ln: nn.LayerNorm, n_prefix: int, name: str = "pool") -> TRef:
        """the mean of LayerNorm over the first `n_prefix` rows of every image of a [B, 1, L, C] map -> [B, 1, 1, C]
        (`norm(out[:, :P]).mean(1)`, vt_prefix_pool_fwd).  Backward in one launch (vt_prefix_pool_bwd): the LayerNorm backward
        of the prefix rows, zeros in every other row (or an addition to a gradient that is already there), d gamma / d beta
        through a fixed-point channel-sums buffer that vt_channel_sums_to_f32 adds to the gradients."""
        if x.H != 1 or not 1 <= n_prefix <= min(4, x.W):
            raise ValueError(f"{name}: the first {n_prefix} tokens (1..4) of a [B, {x.H}, {x.W}, C] map")
        if tuple(ln.normalized_shape) != (x.C,) or not ln.elementwise_affine or ln.bias is None:
            raise NotImplementedError(f"{name}: LayerNorm({ln.normalized_shape}) over a {x.C}-channel map with weight and bias")
        if x.logical_c != x.C or x.C % _EPC[self.dtype]:
            raise NotImplementedError(f"{name}: {x.C} channels must be a multiple of {_EPC[self.dtype]} for dtype {self.dtype}")
        self.tag += 1
        dt, B, L, Cc = self.dtype, x.B, x.W, x.C
        y = self.act(B, 1, 1, Cc, name + ".y")
        gm = self.pref(ln.weight)
        self.emit(N.OP_PREFIX_POOL_FWD, [x.addr(), gm, self.pref(ln.bias), y.addr()], [x.ld, y.ld, B, L, n_prefix, Cc, dt], [ln.eps])
        if self.need_grad:

            def bwd(dy):
                sums = self.zeroed_f32(N.channel_sums_floats(2, Cc), "poolsums")
                if x.needs_grad:
                    gx, acc = self.grad_accum_target(x)
                else:
                    gx, acc = self.act(B, 1, L, Cc, name + ".dx"), 0
                self.emit(N.OP_PREFIX_POOL_BWD, [dy.addr(), x.addr(), gm, gx.addr(), self.bp(sums)],
                          [dy.ld, x.ld, gx.ld, acc, B, L, n_prefix, Cc, dt], [ln.eps])
                if x.needs_grad:
                    self.grad_written(x)
                dsts = [self.pgrad(ln.weight), self.pgrad(ln.bias)]
                if any(d is not None for d in dsts):
                    self.emit(N.OP_CHANNEL_SUMS, [self.bp(sums)] + dsts, [2, Cc])

            self._node(y, bwd)
        return y

    # -- CaiT pieces (reference backbones/cait.py:16-51, 74-77): vt_talking_attention.hip -----------------------------
    def talking_attention(self, q: TRef, k: TRef, v: TRef, n_heads: int, proj_l: nn.Conv2d, proj_w: nn.Conv2d,
                          name: str = "talking_attention") -> TRef:
        """talking-heads attention on token maps [B, 1, L, C]: the scores of all heads are mixed by `proj_l` (a 1x1
        Conv2d(n_heads, n_heads)) in front of the softmax and by `proj_w` behind it (vt_talk_attn_fwd; it writes the row
        log-sum-exp of the MIXED scores).  The mixing weights and biases are read as f32 masters in both dtypes and their
        gradients go to the f32 gradient buffer.  Backward: one vt_talk_attn_bwd writes d(q), d(k), d(v) and adds the four
        parameter gradients through a scratch that every layer of the same size shares; no atomics, the same launch under
        `deterministic`."""
        dt = self.dtype
        if not (q.same_geom(k) and q.same_geom(v)) or q.H != 1:
            raise ValueError(f"{name}: q, k and v are [B, 1, L, C] token maps of one geometry")
        if n_heads <= 0 or q.C % n_heads:
            raise ValueError(f"{name}: {q.C} channels do not split into n_heads={n_heads}")
        D = q.C // n_heads
        if D != 48:
            raise NotImplementedError(f"{name}: head_dim = {q.C} / n_heads={n_heads} = {D}: the talking-heads kernels "
                                      "implement head_dim 48")
        if n_heads > 16:
            raise NotImplementedError(f"{name}: n_heads={n_heads}: the talking-heads kernels hold at most 16 heads per pair")
        for conv, what in ((proj_l, "proj_l"), (proj_w, "proj_w")):
            if tuple(conv.weight.shape) != (n_heads, n_heads, 1, 1) or conv.bias is None:
                raise ValueError(f"{name}: {what} is a biased 1x1 Conv2d({n_heads}, {n_heads}), its weight is "
                                 f"{tuple(conv.weight.shape)}")
        if any(t.logical_c != t.C for t in (q, k, v)) or q.C % _EPC[dt]:
            raise NotImplementedError(f"{name}: {q.C} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        self.tag += 1
        B, L, scale = q.B, q.W, D ** -0.5
        o = self.act(B, 1, L, q.C, name + ".o")
        lse = self.f32(B * n_heads * L, name + ".lse")
        mix = [proj_l.weight, proj_l.bias, proj_w.weight, proj_w.bias]
        mp = [self.pref(p) for p in mix]
        self.emit(N.OP_TALK_ATTN_FWD, [q.addr(), k.addr(), v.addr(), o.addr(), self.bp(lse), *mp],
                  [q.ld, k.ld, v.ld, o.ld, B, n_heads, L, D, dt], [scale])
        if self.need_grad and (q.needs_grad or k.needs_grad or v.needs_grad or any(self.pgrad(p) is not None for p in mix)):

            def bwd(do):
                nbytes = int(N.lib().vt_talk_attn_bwd_scratch_bytes(B, n_heads, L))
                if nbytes not in self._talk_scratch:  # (one per size: the launches follow each other on one stream)
                    self._talk_scratch[nbytes] = self.alloc(nbytes, "talk_attn_delta_shares")
                gs = []
                for t in (q, k, v):
                    g = None
                    if t.needs_grad:
                        g, res = self.grad_target(t)
                        assert res is None and self._deferred_flush is None, "q, k and v have one consumer, the attention"
                    gs.append(g)
                self.emit(N.OP_TALK_ATTN_BWD,
                          [q.addr(), k.addr(), v.addr(), do.addr(), self.bp(lse), *mp, *[_addr(g) for g in gs],
                           *[self.pgrad(p) for p in mix], self.bp(self._talk_scratch[nbytes])],
                          [q.ld, k.ld, v.ld, do.ld, *[_ld(g) for g in gs], B, n_heads, L, D, dt], [scale, nbytes])

            self._node(o, bwd)
        return o

    def class_attention(self, q: TRef, k: TRef, v: TRef, n_heads: int, name: str = "class_attention") -> TRef:
        """softmax(q k^T / sqrt(head_dim)) v with ONE query row per image: q is [B, 1, 1, C], k and v are [B, 1, Lk, C] maps
        (channel slices of one buffer or not), the result [B, 1, 1, C] (vt_cls_attn_fwd).  Backward: one vt_cls_attn_bwd
        writes d(q) and every row of d(k), d(v); no scratch, no atomics."""
        dt = self.dtype
        if not k.same_geom(v) or k.H != 1 or (q.B, q.H, q.W, q.C) != (k.B, 1, 1, k.C):
            raise ValueError(f"{name}: q is a [B, 1, 1, C] row per image, k and v are [B, 1, Lk, C] token maps of one geometry")
        if n_heads <= 0 or q.C % n_heads:
            raise ValueError(f"{name}: {q.C} channels do not split into n_heads={n_heads}")
        D = q.C // n_heads
        if D not in (32, 48, 64):
            raise NotImplementedError(f"{name}: head_dim = {q.C} / n_heads={n_heads} = {D}: the class-attention kernels "
                                      "implement head_dim 32, 48 and 64")
        if any(t.logical_c != t.C for t in (q, k, v)) or q.C % _EPC[dt]:
            raise NotImplementedError(f"{name}: {q.C} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        self.tag += 1
        B, Lk, scale = k.B, k.W, D ** -0.5
        o = self.act(B, 1, 1, q.C, name + ".o")
        lse = self.f32(B * n_heads, name + ".lse")
        self.emit(N.OP_CLS_ATTN_FWD, [q.addr(), k.addr(), v.addr(), o.addr(), self.bp(lse)],
                  [q.ld, k.ld, v.ld, o.ld, B, n_heads, Lk, D, dt], [scale])
        if self.need_grad and (q.needs_grad or k.needs_grad or v.needs_grad):

            def bwd(do):
                gs = []
                for t in (q, k, v):
                    g = None
                    if t.needs_grad:
                        g, res = self.grad_target(t)
                        assert res is None and self._deferred_flush is None, "q, k and v have one consumer, the attention"
                    gs.append(g)
                self.emit(N.OP_CLS_ATTN_BWD,
                          [q.addr(), k.addr(), v.addr(), o.addr(), do.addr(), self.bp(lse), *[_addr(g) for g in gs]],
                          [q.ld, k.ld, v.ld, o.ld, do.ld, *[_ld(g) for g in gs], B, n_heads, Lk, D, dt], [scale])

            self._node(o, bwd)
        return o

    def token_prepend(self, x: TRef, first, name: str = "token_prepend") -> TRef:
        """[first | x]: one row in front of the tokens of a [B, 1, T, C] map -> [B, 1, 1 + T, C] (vt_token_prepend_fwd).
        `first` is a [B, 1, 1, C] activation or a parameter of C values (read as the f32 master and broadcast over the
        batch).  Backward copies or accumulates the token rows into d(x) and hands row 0 to d(first), summed over the images
        in order for a parameter (vt_token_prepend_bwd)."""
        Cc, dt = x.C, self.dtype
        is_param = not isinstance(first, TRef)
        if x.H != 1 or x.logical_c != Cc:
            raise ValueError(f"{name}: x is a [B, 1, T, C] token map")
        if is_param and first.numel() != Cc:
            raise ValueError(f"{name}: the first token holds {first.numel()} values for {Cc} channels")
        if not is_param and (first.B, first.H, first.W, first.C) != (x.B, 1, 1, Cc):
            raise ValueError(f"{name}: the first token is a [B, 1, 1, {Cc}] row per image")
        self.tag += 1
        B, T = x.B, x.W
        y = self.act(B, 1, T + 1, Cc, name + ".y")
        fa, fp = (None, self.pref(first)) if is_param else (first.addr(), None)
        self.emit(N.OP_TOKEN_PREPEND_FWD, [x.addr(), fa, fp, y.addr()], [x.ld, 0 if is_param else first.ld, y.ld, B, T, Cc, dt])
        if self.need_grad:

            def bwd(dy):
                gx, acc = (None, 0)
                if x.needs_grad:
                    gx, acc = self.grad_accum_target(x)
                gf, gp = None, None
                if is_param:
                    gp = self.pgrad(first)
                elif first.needs_grad:
                    gf, res = self.grad_target(first)
                    assert res is None and self._deferred_flush is None, "the first token has one consumer"
                if gx is None and gf is None and gp is None:
                    return
                self.emit(N.OP_TOKEN_PREPEND_BWD, [dy.addr(), _addr(gx), _addr(gf), gp], [dy.ld, _ld(gx), acc, _ld(gf), B, T, Cc, dt])
                if x.needs_grad:
                    self.grad_written(x)

            self._node(y, bwd)
        return y

    # -- PatchConvNet pieces (reference backbones/patchconvnet.py:25-103): vt_patchconv.hip ------------------------------
    def batch_norm(self, x: TRef, bn: nn.BatchNorm2d, name: str = "bn") -> TRef:
        """a BatchNorm2d that stands IN FRONT of its convolution: there is no conv epilogue to take the batch statistics
        from, so vt_channel_stats forms them from the stored map (the contract of VT_CONV_STATS); the rest are the launches of
        a conv unit with activation code 0 and x as the "pre-activation" -- finalize / normalise (or the two in one), the
        running-statistics update, SyncBatchNorm's exchange in front of the finalize, and the BatchNorm backward."""
        spec = bn if isinstance(bn, BNSpec) else BNSpec.from_bn(bn)
        if x.logical_c != x.C or x.C % _EPC[self.dtype] or spec.weight.numel() != x.C:
            raise NotImplementedError(f"{name}: BatchNorm2d({spec.weight.numel()}) over a {x.logical_c}-channel map")
        self.tag += 1
        em = _BNEmitter(self, spec, x.C)
        y = self.act(x.B, x.H, x.W, x.C, name + ".y")
        if spec.training:
            stats = self.zeroed_f32(N.stat_floats(x.C), "stats")
            self.emit(N.OP_CHANNEL_STATS, [x.addr(), self.bp(stats)], [x.ld, x.C, self.dtype], [x.M])
            if self.bn_fin_apply and not self.bn_sync:
                ptrs, flts = em.finalize_operands(stats, x.M)
                self.emit(N.OP_BN_FIN_APPLY, ptrs + [x.addr(), None, y.addr()], [x.C, x.ld, 0, y.ld, 0, self.dtype], flts + [x.M])
            else:
                em.finalize(stats, x.M)
                self._act_apply(x, em.cp[0], em.cp[1], None, y, 0)
        else:
            em.eval_coeffs()
            self._act_apply(x, em.cp[0], em.cp[1], None, y, 0)
        if self.need_grad:

            def bwd(dy):
                sums, bcoef, dz = em.bwd_buffers(y, name + ".dx")
                if self.bn_fin_apply and not self.bn_sync:
                    em.bwd_reduce(dy, x, 0, sums, x.M)
                    self.emit(N.OP_BN_BWD_FIN_APPLY,
                              [self.bp(sums), *em.cp, *em.grads(), self.bp(bcoef), dy.addr(), x.addr(), dz.addr()],
                              [x.C, int(spec.training), dy.ld, x.ld, dz.ld, 0, self.dtype],
                              [x.M * self.bn_world, 1.0 / self.bn_world, x.M])
                else:
                    em.bwd_three_launches(dy, x, 0, sums, bcoef, dz)
                self.grad_add(x, dz)

            self._node(y, bwd)
        return y

    def dw3_gelu_pool(self, u: TRef, conv: nn.Conv2d, name: str = "dw") -> "tuple[TRef, TRef]":
        """(a, pooled): a = GELU(depthwise 3x3, padding 1, of u + bias) and pooled = mean over the pixels of a, [B, 1, 1, C],
        in ONE launch that owns (image, channel slab) and walks all its pixels (vt_dw3_gelu_pool_fwd).  Backward: one
        launch recomputes z, forms dz from d(a) and d(pooled), writes d(u) and each image's share of the filter / bias
        gradient, which a small second kernel adds in image order (vt_dw3_gelu_pool_bwd): no atomics, the same launch under
        `deterministic`.  The filter and bias are read as f32 masters."""
        dt, Cc = self.dtype, u.C
        if (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation)) != ((3, 3), (1, 1), (1, 1), (1, 1)) \
                or conv.groups != Cc or conv.in_channels != Cc or conv.out_channels != Cc:
            raise NotImplementedError(f"{name}: a depthwise 3x3 convolution with stride 1 and padding 1 over {Cc} channels")
        if u.logical_c != Cc or Cc % _EPC[dt]:
            raise NotImplementedError(f"{name}: {Cc} channels must be a multiple of {_EPC[dt]} for dtype {dt}")
        if not N.lib().vt_dw3_gelu_pool_supported(u.H, u.W, dt):
            raise NotImplementedError(f"{name}: a {u.H}x{u.W} token map is too large for the plane kernels: the planes of one "
                                      "16-byte channel slab with their halo must fit 160 KiB of LDS")
        self.tag += 1
        tag = self.tag
        B, H, W = u.B, u.H, u.W
        a = self.act(B, H, W, Cc, name + ".a")
        pooled = self.act(B, 1, 1, Cc, name + ".pooled")
        wp, bp_ = self.pref(conv.weight), self.pref(conv.bias)
        self.emit(N.OP_DW3_GELU_POOL_FWD, [u.addr(), wp, bp_, a.addr(), pooled.addr()], [u.ld, a.ld, pooled.ld, B, H, W, Cc, dt])
        if self.need_grad:

            def bwd():
                self.tag = tag
                da, dp = self.grad_read(a), self.grad_read(pooled)
                if da is None and dp is None:
                    return
                gu = res = None
                if u.needs_grad:
                    gu, res = self.grad_target(u)
                dw, db = self.pgrad(conv.weight), self.pgrad(conv.bias)
                if gu is None and dw is None and db is None:
                    return
                nbytes = int(N.lib().vt_dw3_gelu_pool_bwd_scratch_bytes(B, Cc))
                if nbytes not in self._dw3_scratch:  # (one per size: the launches follow each other on one stream)
                    self._dw3_scratch[nbytes] = self.alloc(nbytes, "dw3_shares")
                self.emit(N.OP_DW3_GELU_POOL_BWD,
                          [u.addr(), _addr(da), _addr(dp), wp, bp_, _addr(gu), _addr(res), dw, db, self.bp(self._dw3_scratch[nbytes])],
                          [u.ld, _ld(da), _ld(dp), _ld(gu), _ld(res), B, H, W, Cc, dt], [nbytes])
                if gu is not None:
                    self.grad_written(u)

            self.nodes.append(bwd)
        return a, pooled

    def se_gate(self, a: TRef, s: TRef, out: Optional[TRef] = None, name: str = "se") -> TRef:
        """y = a * sigmoid(s): the Squeeze-Excitation scale, s a [B, 1, 1, C] row per image (vt_se_gate_fwd).  Backward: d(a)
        and the f32 d(s), summed over the pixels by the (image, slab) owner (vt_se_gate_bwd)."""
        if (s.B, s.H, s.W, s.C) != (a.B, 1, 1, a.C):
            raise ValueError(f"{name}: s is a [B, 1, 1, {a.C}] row per image")
        self.tag += 1
        dt = self.dtype
        y = out if out is not None else self.act(a.B, a.H, a.W, a.C, name + ".y")
        assert y.same_geom(a), "out geometry mismatch"
        self.emit(N.OP_SE_GATE_FWD, [a.addr(), s.addr(), y.addr()], [a.ld, s.ld, y.ld, a.B, a.H * a.W, a.C, dt])
        if self.need_grad:

            def bwd(dy):
                ga, acc = self.grad_accum_target(a)
                ds32 = self.f32(a.B * a.C, "ds32")
                self.emit(N.OP_SE_GATE_BWD, [dy.addr(), a.addr(), s.addr(), ga.addr(), self.bp(ds32)],
                          [dy.ld, a.ld, s.ld, ga.ld, a.B, a.H * a.W, a.C, acc, dt])
                self.grad_written(a)
                gs_, _ = self.grad_target(s)
                self.emit(N.OP_COPY2D, [self.bp(ds32), gs_.addr()], [N.VT_F32, dt, a.C, 0], [a.C, gs_.ld, a.B])

            self._node(y, bwd)
        return y

    def pool_attention(self, q: TRef, k: TRef, v: TRef, name: str = "pool_attention") -> TRef:
        """softmax(q k^T / sqrt(C)) v with ONE query row per image and ONE head as wide as the embedding: q is [B, 1, 1, C],
        k and v are [B, 1, Lk, C] maps (channel slices of one buffer or not), the result [B, 1, 1, C] (vt_pool_attn_fwd).
        Backward: one vt_pool_attn_bwd writes d(q) and every row of d(k), d(v); no scratch, no atomics."""
        dt = self.dtype
        if not k.same_geom(v) or k.H != 1 or (q.B, q.H, q.W, q.C) != (k.B, 1, 1, k.C):
            raise ValueError(f"{name}: q is a [B, 1, 1, C] row per image, k and v are [B, 1, Lk, C] token maps of one geometry")
        if any(t.logical_c != t.C for t in (q, k, v)) or q.C % _EPC[dt] or q.C // _EPC[dt] > 256:
            raise NotImplementedError(f"{name}: {q.C} channels must be a multiple of {_EPC[dt]} and at most {256 * _EPC[dt]} "
                                      f"for dtype {dt}")
        self.tag += 1
        B, Lk, Cc, scale = k.B, k.W, q.C, q.C ** -0.5
        o = self.act(B, 1, 1, Cc, name + ".o")
        lse = self.f32(B, name + ".lse")
        self.emit(N.OP_POOL_ATTN_FWD, [q.addr(), k.addr(), v.addr(), o.addr(), self.bp(lse)],
                  [q.ld, k.ld, v.ld, o.ld, B, Lk, Cc, dt], [scale])
        if self.need_grad and (q.needs_grad or k.needs_grad or v.needs_grad):

            def bwd(do):
                gs = []
                for t in (q, k, v):
                    g = None
                    if t.needs_grad:
                        g, res = self.grad_target(t)
                        assert res is None and self._deferred_flush is None, "q, k and v have one consumer, the attention"
                    gs.append(g)
                self.emit(N.OP_POOL_ATTN_BWD,
                          [q.addr(), k.addr(), v.addr(), o.addr(), do.addr(), self.bp(lse), *[_addr(g) for g in gs]],
                          [q.ld, k.ld, v.ld, o.ld, do.ld, *[_ld(g) for g in gs], B, Lk, Cc, dt], [scale])

            self._node(o, bwd)
        return o

    # -- ESE gate (reference vovnet.py:20-28) ---------------------------------------------
    def ese(self, x: TRef, linear: nn.Conv2d, residual: Optional[TRef] = None,
            out: Optional[TRef] = None, name="ese") -> TRef:
        pooled = self.global_avgpool(x, name + ".pool")
        s = self.conv_unit(pooled, linear, None, False, name=name + ".linear")
        self.tag += 1
        y = out if out is not None else self.act(x.B, x.H, x.W, x.C, name + ".y")
        self.emit(N.OP_ESE_FWD, [x.addr(), s.addr(), _addr(residual), y.addr()],
                  [x.ld, s.ld, _ld(residual), y.ld, x.B, x.H * x.W, x.C, self.dtype])
        if self.need_grad:

            def bwd(dy):
                self.grad_add(residual, dy)
                gx, acc = self.grad_accum_target(x)
                ds32 = self.f32(x.B * x.C, "ds32")
                self.emit(N.OP_ESE_BWD, [dy.addr(), x.addr(), s.addr(), gx.addr(), self.bp(ds32)],
                          [dy.ld, x.ld, s.ld, gx.ld, x.B, x.H * x.W, x.C, acc, self.dtype])
                self.grad_written(x)
                gs_, _ = self.grad_target(s)
                self.emit(N.OP_COPY2D, [self.bp(ds32), gs_.addr()], [N.VT_F32, self.dtype, x.C, 0], [x.C, gs_.ld, x.B])

            self._node(y, bwd)
        return y

    def hsig_gate(self, a: TRef, s: TRef, out: Optional[TRef] = None, name: str = "se") -> TRef:
        """y = a * hardsigmoid(s): the Squeeze-Excitation scale of MobileNetV3, s a [B, 1, 1, C] row per image -- the gate of
        `ese` without a residual (vt_ese_gate_fwd).  Backward (vt_ese_gate_bwd): d(a), and the f32 d(s) of an (image, column
        group) summed by its one workgroup in fixed point -- order-free, so deterministic mode keeps it."""
        if (s.B, s.H, s.W, s.C) != (a.B, 1, 1, a.C):
            raise ValueError(f"{name}: s is a [B, 1, 1, {a.C}] row per image")
        self.tag += 1
        dt = self.dtype
        y = out if out is not None else self.act(a.B, a.H, a.W, a.C, name + ".y")
        assert y.same_geom(a), "out geometry mismatch"
        self.emit(N.OP_ESE_FWD, [a.addr(), s.addr(), None, y.addr()], [a.ld, s.ld, 0, y.ld, a.B, a.H * a.W, a.C, dt])
        if self.need_grad:

            def bwd(dy):
                ga, acc = self.grad_accum_target(a)
                ds32 = self.f32(a.B * a.C, "ds32")
                self.emit(N.OP_ESE_BWD, [dy.addr(), a.addr(), s.addr(), ga.addr(), self.bp(ds32)],
                          [dy.ld, a.ld, s.ld, ga.ld, a.B, a.H * a.W, a.C, acc, dt])
                self.grad_written(a)
                gs_, _ = self.grad_target(s)
                self.emit(N.OP_COPY2D, [self.bp(ds32), gs_.addr()], [N.VT_F32, dt, a.C, 0], [a.C, gs_.ld, a.B])

            self._node(y, bwd)
        return y

    # -- classifier head + loss (reference classifier.py:58-64, 92) -----------------------
    def xent(self, logits: TRef, label_smoothing: float, grad_scale: float, mix: bool = False,
             num_classes: Optional[int] = None) -> Buf:
        """`num_classes` < logits.C: the head was widened to a whole 16-byte chunk over zero rows; the loss reads the
        first `num_classes` columns and the gradient of the others is zero, so the zero rows stay zero."""
        self.tag += 1
        loss = self.zeroed_f32(64, "loss")
        Bn, Ncls = logits.B, logits.C if num_classes is None else num_classes
        assert 0 < Ncls <= logits.C
        g = None
        if self.need_grad:
            gs = self._gs(logits)
            g = self._gref(logits)
            gs.init.append((logits.coff, logits.coff + logits.C))
            if Ncls < logits.C:
                assert g.coff == 0 and g.ld == g.C, "a widened head is a dense map of its own"
                self.emit(N.OP_MEMSET, [g.addr()], [0], [g.M * g.C * g.esize])
        self.emit(N.OP_XENT, [logits.addr(), (LABELS, 0), self.bp(loss), g.addr() if g else None,
                              (HYPER, self.MIX_OFF) if mix else None],
                  [logits.ld, g.ld if g else 0, Bn, Ncls, self.dtype], [label_smoothing, grad_scale])
        return loss

    def bce(self, logits: TRef, label_smoothing: float, grad_scale: float, mix: bool = False,
            num_classes: Optional[int] = None, target_threshold: Optional[float] = None, sum_classes: bool = False) -> Buf:
        """binary cross-entropy against the smoothed (mixed, thresholded) one-hot target in the place of `xent`
        (vt_sigmoid_bce, include/vt_amd.h): the same operands, plus one double per row of scratch from which the loss is
        added in row order.  `target_threshold=None`: soft targets; `sum_classes`: the loss is summed over the classes and
        averaged over the batch, and the gradient loses its 1 / N.  A widened head as in `xent`."""
        self.tag += 1
        loss = self.zeroed_f32(64, "loss")
        Bn, Ncls = logits.B, logits.C if num_classes is None else num_classes
        assert 0 < Ncls <= logits.C
        g = None
        if self.need_grad:
            gs = self._gs(logits)
            g = self._gref(logits)
            gs.init.append((logits.coff, logits.coff + logits.C))
            if Ncls < logits.C:
                assert g.coff == 0 and g.ld == g.C, "a widened head is a dense map of its own"
                self.emit(N.OP_MEMSET, [g.addr()], [0], [g.M * g.C * g.esize])
        rows = self.f32(2 * Bn, "bce.rows")  # double[B]
        flags = (N.VT_BCE_SUM_CLASSES if sum_classes else 0) | (N.VT_BCE_THRESHOLD if target_threshold is not None else 0)
        self.emit(N.OP_BCE, [logits.addr(), (LABELS, 0), self.bp(loss), g.addr() if g else None,
                             (HYPER, self.MIX_OFF) if mix else None, self.bp(rows)],
                  [logits.ld, g.ld if g else 0, Bn, Ncls, self.dtype, flags],
                  [label_smoothing, grad_scale, 0.0 if target_threshold is None else target_threshold])
        return loss

    def xent_eval(self, logits: TRef, num_classes: Optional[int] = None) -> Buf:
        """validation (classifier.py:97-109): [loss sum without label smoothing, top-1 hits, rows] of the batch, f32[3]."""
        self.tag += 1
        out = self.zeroed_f32(64, "val_sums")
        self.emit(N.OP_XENT_EVAL, [logits.addr(), (LABELS, 0), self.bp(out)],
                  [logits.ld, logits.B, logits.C if num_classes is None else num_classes, self.dtype])
        return out

    # -- finish ---------------------------------------------------------------------------
    def build_backward(self):
        self._cur = self.bwd
        for node in reversed(self.nodes):
            node()
        self._wgrad_release()  # (groups whose units did not all reach backward: a branch without gradient)
        self.emit(N.OP_JOIN)  # all filter gradients done before anything reads the gradient buffers
        self._cur = self.fwd
        if self._hoisted:
            # [FORK, packs on the side stream] ahead of the forward ops; the executor joins the
            # side stream at the end of the list, i.e. before the backward list starts
            # They are enqueued AFTER the first unit of the forward pass: issuing ~80 launches costs the
            # host ~0.5 ms, during which the main stream must already have work (measured: it sat idle
            # for exactly that long at the head of every step when the packs came first).
            body, self.fwd = self.fwd, []
            cut = next((i + 1 for i, op in enumerate(body) if (op.kind & 0xFFFF) in (N.OP_BN_ACT_APPLY, N.OP_BN_FIN_APPLY)), 0)
            self._cur = self.fwd
            self.fwd.extend(body[:cut])
            self.emit(N.OP_FORK)
            self.fwd.extend(self._hoisted)
            self.fwd.extend(body[cut:])
            self._hoisted = []

    def seed_output_grads(self, outs: list[TRef]):
        """reserve gradient buffers of the returned feature maps; they are filled from the
        caller's grad tensors before the backward list runs."""
        seeds = []
        for t in outs:
            g = self._gref(t)
            self._gs(t).init.append((t.coff, t.coff + t.C))
            seeds.append(g)
        return seeds


def ops_array(ops: list) -> "C.Array":
    arr = (N.Op * max(len(ops), 1))()
    for i, op in enumerate(ops):
        C.memmove(C.addressof(arr[i]), C.addressof(op), C.sizeof(N.Op))
    return arr


def tref_to_tensor(arena: torch.Tensor, t: TRef) -> torch.Tensor:
    """view of an arena activation as a logical-NCHW (channels_last strided) torch tensor."""
    # Built with set_() on the arena's storage rather than by slicing/viewing: the result shares
    # (and keeps alive) the arena memory but is NOT an autograd/tracer "view" of another tensor,
    # which is what autograd.Function outputs and torch.jit.trace need.
    td = _TORCH_DTYPE[t.dtype]
    byte_off = arena.storage_offset() + t.buf.offset + t.coff * t.esize
    assert byte_off % t.esize == 0
    out = torch.empty(0, dtype=td, device=arena.device)
    out.set_(arena.untyped_storage(), byte_off // t.esize, (t.B, t.C, t.H, t.W),
             (t.H * t.W * t.ld, 1, t.W * t.ld, t.ld))
    return out
