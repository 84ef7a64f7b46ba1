"""TEST INFRASTRUCTURE -- a plain-torch restatement of the reference's BiFPN (vision_toolbox/necks.py:125-215) with a
switchable block, the yardstick of the BiFPN tests.

The reference's BiFPN runs only with `block=ConvNormAct` (its default SeparableConv2d cannot be constructed), so fixtures of
the unmodified reference pin the wiring, the fusion arithmetic and the state_dict layout through that block
(tools/gen_golden_bifpn.py), this file is tied to those fixtures with the same block ("cna": Conv3x3-BN-ReLU), and the
separable block ("sep": depthwise 3x3 Conv-BN-ReLU6, pointwise 1x1 Conv-BN-ReLU6) is then checked against this file.  It
imports nothing from the package, runs in float32 or float64 on the CPU, can round every stored map to bf16 where the GPU
path stores one (`bf16=True`: the inputs, the lateral outputs, the fused map, z and y of every unit, the filters the
convolutions read, and every gradient on the way back), and records per fusion node what the weight-gradient scale

    S_i = sum |g| (|R_i(x_i)| + |out|) / (sum_j relu(w)_j + eps)

needs (`weight_grad_scales()` after a backward)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler

CASES = {  # name -> (in_channels, out_channels, sizes (bottom first), layers); batch 2.  Must match tools/gen_golden_bifpn.py
    "a": ((16, 24, 40), 16, (16, 8, 4), 1),
    "b": ((16, 24, 40, 64), 24, (32, 16, 8, 4), 2),
    "c": ((8, 16), 8, (8, 4), 1),
}
BATCH = 2
# case b: one weight the ReLU clamps, one exactly at the kink
PINNED = {"b": {"layers.0.out_fuses.0.weights": (1, -0.5), "layers.1.td_fuses.0.weights": (0, 0.0)}}
MIN_WEIGHT_SUM = 0.2


def load_fixture(case: str) -> dict:
    """the reference's arrays of one case, keyed "bifpn_<case>/..." (two files: the eval-mode arrays are kept apart so that
    each file stays under the size limit of a committed file)"""
    from pathlib import Path

    import numpy as np

    out = {}
    for stem in (f"bifpn_{case}", f"bifpn_{case}_eval"):
        with np.load(Path(__file__).parent / "golden" / f"{stem}.npz") as z:
            out.update({k: z[k] for k in z.files})
    return out


def set_fusion_weights(module: nn.Module, prefix: str, case: str = "") -> float:
    """THE rule for the fusion weights, used by the generator and by every test: w = 1 + 0.5 N (keyed by the module's name),
    plus the pinned entries of the case.  (Left as the filler fills them, 0.1 N, about half the weights are negative and
    sum + eps can approach eps = 1e-4, which amplifies everything by 1e4.)  Returns the smallest sum relu(w) of a node."""
    smallest = float("inf")
    with torch.no_grad():
        for name, mod in module.named_modules():
            w = getattr(mod, "weights", None)
            if not isinstance(w, nn.Parameter):
                continue
            w.copy_(1.0 + 0.5 * filler.tensor(prefix + name + ".weights.rule", tuple(w.shape)).to(w.dtype))
            pin = PINNED.get(case, {}).get(name + ".weights")
            if pin is not None:
                w[pin[0]] = pin[1]
            smallest = min(smallest, float(F.relu(w).sum()))
    assert smallest >= MIN_WEIGHT_SUM, smallest
    return smallest


def fill(module: nn.Module, prefix: str, case: str = "") -> None:
    filler.fill_module(module, prefix)
    set_fusion_weights(module, prefix, case)


def inputs(case: str, dtype=torch.float32, device="cpu", tag: str = ""):
    """the case's feature maps.  tag "": the draw the reference fixtures were made with.  Another tag is another draw of the
    same shapes, for runs no fixture is tied to (see kink_distance)"""
    ins, _, sizes, _ = CASES[case]
    return [filler.tensor(f"bifpn_{case}.{tag}x{i}", (BATCH, c, s, s)).to(device=device, dtype=dtype).requires_grad_(True)
            for i, (c, s) in enumerate(zip(ins, sizes))]


def loss(case: str, ys):
    return sum((y.to(torch.float64 if y.dtype == torch.float64 else torch.float32)
                * filler.tensor(f"bifpn_{case}.r{i}", tuple(y.shape)).to(y.device)).sum() for i, y in enumerate(ys))


class _Round(torch.autograd.Function):
    """a bf16 store: the value is rounded going forward, its gradient going backward"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _Use(torch.autograd.Function):
    """one more consumer of a stored map: (this use, the map for later uses).  The GPU path keeps ONE gradient buffer per
    map: backward meets the consumers in reverse order, the first writes it, every other adds to the stored value and
    rounds again.  Going backward, `g_rest` is what the later consumers left in the buffer."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        return x.clone(), x.clone()

    @staticmethod
    def backward(ctx, g_use, g_rest):
        if g_use is None:
            return g_rest
        g = g_use if g_rest is None else g_rest + g_use
        return g.to(torch.bfloat16).to(g.dtype)


class _Map:
    """a stored map and its consumers in forward order (plain tensor semantics unless `chain`)"""

    def __init__(self, t, chain: bool):
        self.t, self.chain = t, chain

    def use(self):
        if not self.chain:
            return self.t
        u, self.t = _Use.apply(self.t)
        return u


class _RoundFwd(torch.autograd.Function):
    """the bf16 mirror of a filter: rounded going forward, the gradient stays f32"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _unit(conv: nn.Conv2d, act: nn.Module) -> nn.Sequential:
    seq = nn.Sequential()
    seq.add_module("conv", conv)
    seq.add_module("norm", nn.BatchNorm2d(conv.out_channels))
    seq.add_module("act", act)
    return seq


def block_cna(cin: int, cout: int) -> nn.Module:
    return _unit(nn.Conv2d(cin, cout, 3, 1, 1, bias=False), nn.ReLU())


def block_sep(cin: int, cout: int) -> nn.Module:
    seq = nn.Sequential()
    seq.add_module("dw", _unit(nn.Conv2d(cin, cin, 3, 1, 1, groups=cin, bias=False), nn.ReLU6()))
    seq.add_module("pw", _unit(nn.Conv2d(cin, cout, 1, bias=False), nn.ReLU6()))
    return seq


BLOCKS = {"cna": block_cna, "sep": block_sep}


class RefFuse(nn.Module):
    def __init__(self, channels: int, n: int, block, eps: float):
        super().__init__()
        self.weights = nn.Parameter(torch.ones(n))
        self.conv = block(channels, channels)
        self.eps = eps


class RefLayer(nn.Module):
    def __init__(self, levels: int, channels: int, block, eps: float):
        super().__init__()
        self.td_fuses = nn.ModuleList([RefFuse(channels, 2, block, eps) for _ in range(levels - 1)])
        self.out_fuses = nn.ModuleList([RefFuse(channels, 3, block, eps) for _ in range(levels - 2)])
        self.last_out_fuse = RefFuse(channels, 2, block, eps)


class RefBiFPN(nn.Module):
    def __init__(self, in_channels, out_channels: int = 64, num_layers: int = 1, block: str = "sep",
                 interpolation_mode: str = "nearest", eps: float = 1e-4, bf16: bool = False):
        super().__init__()
        self.laterals = nn.ModuleList([nn.Conv2d(c, out_channels, 1) for c in in_channels])
        self.layers = nn.ModuleList([RefLayer(len(in_channels), out_channels, BLOCKS[block], eps) for _ in range(num_layers)])
        self.mode, self.bf16 = interpolation_mode, bf16
        self.nodes: list = []  # (weights key, [R_i(x_i)], out, sum relu(w) + eps) per fusion node of the last forward

    # -- the stores of the GPU path -------------------------------------------------------------------------------------
    def _st(self, t):
        return _Round.apply(t) if self.bf16 else t

    def _w(self, w):
        return _RoundFwd.apply(w) if self.bf16 else w

    def _conv_unit(self, u: nn.Sequential, x):
        c = u.conv
        z = self._st(F.conv2d(x, self._w(c.weight), None, c.stride, c.padding, c.dilation, c.groups))
        return self._st(u.act(u.norm(z)))

    def _block(self, blk: nn.Sequential, x):
        if hasattr(blk, "dw"):
            return self._conv_unit(blk.pw, self._conv_unit(blk.dw, x))
        return self._conv_unit(blk, x)

    def _resample(self, x, scale: float):
        t = F.interpolate(x, scale_factor=scale, mode=self.mode)
        return self._st(t) if self.mode != "nearest" else t  # (a bilinear map is materialised, a nearest one never is)

    def _fuse(self, key: str, node: RefFuse, xs) -> _Map:
        w = F.relu(node.weights)
        out = 0
        for i in range(w.shape[0]):
            out = out + xs[i] * w[i]
        den = w.sum() + node.eps
        out = self._st(out / den)
        if out.requires_grad:
            out.retain_grad()
        self.nodes.append((key + ".weights", [x.detach() for x in xs], out, den.detach()))
        return _Map(self._block(node.conv, out), self.bf16)

    def forward(self, xs):
        self.nodes = []
        # (the 1x1 lateral reads the stored input and the bf16 mirror of its filter; its bias stays f32)
        x = [_Map(self._st(F.conv2d(self._st(t), self._w(lat.weight), lat.bias)), self.bf16) for lat, t in zip(self.laterals, xs)]
        for l, layer in enumerate(self.layers):
            p = f"layers.{l}."
            tds = list(x)
            for i, node in enumerate(layer.td_fuses):
                tds[-2 - i] = self._fuse(f"{p}td_fuses.{i}", node, [x[-2 - i].use(), self._resample(tds[-1 - i].use(), 2.0)])
            outs = list(tds)
            for i, node in enumerate(layer.out_fuses):
                outs[i + 1] = self._fuse(f"{p}out_fuses.{i}", node,
                                         [x[i + 1].use(), tds[i + 1].use(), self._resample(tds[i].use(), 0.5)])
            outs[-1] = self._fuse(f"{p}last_out_fuse", layer.last_out_fuse, [x[-1].use(), self._resample(tds[-2].use(), 0.5)])
            x = outs
        return [m.use() for m in x]  # (the caller's seed is the first thing the gradient buffer of an output holds)

    def kink_distance(self, xs) -> float:
        """the smallest distance of a BatchNorm output from a kink of the activation behind it (0 for ReLU, 0 and 6 for
        ReLU6) in a forward of this model.  A value within f32 noise of a kink may fall on the other side in another
        arithmetic; the gradients of the two sides differ by that element's whole contribution, and no f32 bound is
        meaningful there."""
        near, hooks = [], []

        def hook(unit):
            def f(_m, _i, o):
                d = o.abs()
                near.append(float((torch.minimum(d, (o - 6).abs()) if isinstance(unit.act, nn.ReLU6) else d).min()))
            return f

        for u in self.modules():
            if isinstance(u, nn.Sequential) and hasattr(u, "norm") and hasattr(u, "act"):
                hooks.append(u.norm.register_forward_hook(hook(u)))
        with torch.no_grad():
            self(xs)
        for h in hooks:
            h.remove()
        return min(near)

    def weight_grad_scales(self) -> "dict[str, torch.Tensor]":
        """after a backward: S_i of every fusion weight, keyed like the parameter"""
        out = {}
        for key, rx, o, den in self.nodes:
            g = o.grad.abs().double()
            out[key] = torch.stack([(g * (x.abs().double() + o.detach().abs().double())).sum() / den.double() for x in rx])
        return out


def make_ref(case_or_cfg, block: str, prefix: str, case: str = "", dtype=torch.float64, **kw) -> RefBiFPN:
    """the restatement of a case (or of (in_channels, out_channels, layers)), filled by the common rule"""
    if isinstance(case_or_cfg, str):
        ins, outc, _, layers = CASES[case_or_cfg]
    else:
        ins, outc, layers = case_or_cfg
    ref = RefBiFPN(list(ins), outc, layers, block=block, **kw)
    fill(ref, prefix, case)
    return ref.to(dtype)


def run_ref(ref: RefBiFPN, case: str, training: bool, xs=None, prepare=None, tag: str = ""):
    """forward + backward of the case's loss: (ys, dxs, parameter gradients, S_i, state) as detached tensors;
    `prepare(ref)` runs after the mode is set (a frozen bn.eval() inside a training model)"""
    ref.train(training)
    if prepare is not None:
        prepare(ref)
    ref.zero_grad()
    dt = next(ref.parameters()).dtype
    xs = inputs(case, dt, tag=tag) if xs is None else xs
    ys = ref(xs)
    loss(case, ys).backward()
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    state = {k: v.detach().clone() for k, v in ref.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return [y.detach() for y in ys], [x.grad.detach() for x in xs], grads, ref.weight_grad_scales(), state
