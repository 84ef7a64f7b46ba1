"""TEST INFRASTRUCTURE -- the yardstick of the DeformableConv2d tests: a float64 restatement of torchvision's deform_conv2d
(one offset group) in gather form, differentiable by autograd, a second form built on F.grid_sample that the first is checked
against, the shape tables, and the small modules the module tests compile.

There is NO fixture of the reference here: its DeformableConv2d needs torchvision.ops.DeformConv2d, torchvision is not
installed where these tests run, and so the reference class cannot even be imported.  The op is therefore written out under
torchvision's semantics: offset channel 2t is dy and 2t + 1 is dx of tap t = i*k + j; the sampling position is
(ho*s - p + i*d + dy, wo*s - p + j*d + dx); bilinear over floor and floor + 1, a corner outside [0, H-1] x [0, W-1]
contributes zero; the sample times the mask; the ordinary weighted sum over (tap, channel) plus bias.  `floor` carries no
gradient, so at an exactly integer position d(offset) is the right-hand derivative (torchvision's choice)."""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

# (B, H, W, Cin, Cout, k, s, p, d) of the kernel tests, and the dtypes each runs in
KERNEL_SHAPES = [
    ((2, 9, 9, 16, 16, 3, 1, 1, 1), ("f32", "bf16")),   # baseline
    ((2, 7, 10, 64, 32, 3, 2, 1, 1), ("f32", "bf16")),  # stride 2, non-square, two K-steps
    ((1, 5, 5, 8, 8, 3, 1, 2, 2), ("f32", "bf16")),     # dilation, one chunk
    ((1, 17, 17, 32, 72, 3, 1, 1, 1), ("f32", "bf16")), # several pixel tiles with a partial last one, Cout no multiple of 16
    ((2, 6, 6, 24, 16, 1, 1, 0, 1), ("f32", "bf16")),   # k = 1, zero-padded K
    ((1, 9, 9, 12, 20, 3, 1, 1, 1), ("f32",)),          # whole f32 chunks only
]
OFFSET_STD = 1.5  # N(0, 1.5^2): 10 % or more of the samples fall outside the map

# the module tests: DeformableConv2d(16, 24, 3, padding=1) on (2, 16, 12, 12), alone and inside ConvNormAct(8, 16, 1) -> dcn ->
# ConvNormAct(24, 16, 1) on (2, 8, 12, 12)
BLOCK_SHAPE = (2, 16, 12, 12)
BLOCK_ARGS = dict(in_channels=16, out_channels=24, kernel_size=3, padding=1)
CHAIN_SHAPE = (2, 8, 12, 12)
CHAIN_UNITS = ((8, 16, 1), (24, 16, 1))
# seeds of the module tests, chosen on the CPU so that no float64 sampling position lies within 1e-4 of an integer (the nearest
# is 3.6e-4 / 3.6e-4 / 7.8e-4 away; test_deform_gpu.py asserts the condition): "v1" shares the block's offsets
SEEDS = {"v2": 103, "v1": 103, "chain": 10, "strided": 1}
SEED = SEEDS["v2"]


def out_size(H: int, W: int, k: int, s: int, p: int, d: int) -> "tuple[int, int]":
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def positions(offset: torch.Tensor, k: int, s: int, p: int, d: int) -> "tuple[torch.Tensor, torch.Tensor]":
    """(py, px), each [B][k*k][Ho][Wo]: the sampling positions of every (pixel, tap)"""
    B, _, Ho, Wo = offset.shape
    dt = offset.dtype
    t = torch.arange(k * k)
    by = (torch.arange(Ho) * s - p).view(1, 1, Ho, 1) + (t // k * d).view(1, -1, 1, 1)
    bx = (torch.arange(Wo) * s - p).view(1, 1, 1, Wo) + (t % k * d).view(1, -1, 1, 1)
    return by.to(dt) + offset[:, 0::2], bx.to(dt) + offset[:, 1::2]


def columns(x: torch.Tensor, offset: torch.Tensor, mask, k: int, s: int, p: int, d: int) -> torch.Tensor:
    """the column tensor [B][Ho][Wo][k*k][C] in gather form: four indexed corner reads per (pixel, tap)"""
    B, C, H, W = x.shape
    py, px = positions(offset, k, s, p, d)
    y0, x0 = py.detach().floor(), px.detach().floor()
    ly, lx = py - y0, px - x0
    xl = x.permute(0, 2, 3, 1)  # [B][H][W][C]
    bi = torch.arange(B).view(B, 1, 1, 1)
    col = 0
    for dy_, wy in ((0, 1 - ly), (1, ly)):
        for dx_, wx in ((0, 1 - lx), (1, lx)):
            yy, xx = (y0 + dy_).long(), (x0 + dx_).long()
            inside = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            v = xl[bi, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]  # [B][K2][Ho][Wo][C]
            col = col + v * (wy * wx * inside.to(x.dtype)).unsqueeze(-1)
    if mask is not None:
        col = col * mask.unsqueeze(-1)
    return col.permute(0, 2, 3, 1, 4)


def columns_grid_sample(x: torch.Tensor, offset: torch.Tensor, mask, k: int, s: int, p: int, d: int) -> torch.Tensor:
    """the same tensor through F.grid_sample(align_corners=True, padding_mode="zeros"), one call per tap (H, W > 1)"""
    B, C, H, W = x.shape
    py, px = positions(offset, k, s, p, d)
    cols = []
    for t in range(k * k):
        grid = torch.stack((2 * px[:, t] / (W - 1) - 1, 2 * py[:, t] / (H - 1) - 1), dim=-1)
        v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)  # [B][C][Ho][Wo]
        if mask is not None:
            v = v * mask[:, t].unsqueeze(1)
        cols.append(v.permute(0, 2, 3, 1))
    return torch.stack(cols, dim=3)


def deform_conv2d_ref(x, offset, mask, weight, bias, s: int, p: int, d: int, form=columns) -> torch.Tensor:
    """y [B][Cout][Ho][Wo]; `mask` is the FINAL mask (after mask_act) or None; any groups"""
    Cout, Cg, k, _ = weight.shape
    B, C = x.shape[:2]
    G = C // Cg
    col = form(x, offset, mask, k, s, p, d)  # [B][Ho][Wo][K2][C]
    Ho, Wo = col.shape[1:3]
    y = torch.einsum("bhwkgc,gokc->bgohw", col.reshape(B, Ho, Wo, k * k, G, Cg),
                     weight.permute(0, 2, 3, 1).reshape(G, Cout // G, k * k, Cg))
    y = y.reshape(B, Cout, Ho, Wo)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def outside_fraction(offset: torch.Tensor, H: int, W: int, k: int, s: int, p: int, d: int) -> float:
    """share of the samples with no corner inside the map"""
    py, px = positions(offset.double(), k, s, p, d)
    return float(((py <= -1) | (py >= H) | (px <= -1) | (px >= W)).double().mean())


def min_integer_distance(offset: torch.Tensor, k: int, s: int, p: int, d: int) -> float:
    py, px = positions(offset.double(), k, s, p, d)
    return float(torch.minimum((py - py.round()).abs().min(), (px - px.round()).abs().min()))


# ---- the module tests' models -------------------------------------------------------------------------------------------------
class Round(torch.autograd.Function):
    """a bf16 store: the value is rounded going forward, its gradient going backward (tests/test_resnet_gpu.py `_Round`)"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def bf16_mirror(w: torch.Tensor) -> torch.Tensor:
    """a filter as the bf16 launches read it -- the rounded mirror -- with the gradient going to the f32 master unrounded"""
    return w + (w.to(torch.bfloat16).to(w.dtype) - w).detach()


_SAME = lambda t: t


def dcn_ref(m: nn.Module, x: torch.Tensor, st=_SAME, wst=_SAME) -> torch.Tensor:
    """a DeformableConv2d `m` (float64 parameters) restated: its two convolutions with F.conv2d, mask_act, deform_conv2d_ref.
    `st` is applied where the launch list stores a map (offset map, mask logits, output), `wst` to the filters"""
    c = m.conv
    s, p, d = c.stride[0], c.padding[0], c.dilation[0]
    conv = lambda cv: st(F.conv2d(x, wst(cv.weight), cv.bias, s, p, d))
    offset = conv(m.conv_offset)
    mask = m.conv_mask[1](conv(m.conv_mask[0])) if m.conv_mask is not None else None
    return st(deform_conv2d_ref(x, offset, mask, wst(c.weight), c.bias, s, p, d))


def cna_ref(u: nn.Module, x: torch.Tensor, st=_SAME, wst=_SAME) -> torch.Tensor:
    """a training-mode ConvNormAct(norm="bn", act="relu") restated: stored z, batch statistics of the stored z, stored y"""
    cv, bn = u.conv, u.norm
    z = st(F.conv2d(x, wst(cv.weight), None, cv.stride, cv.padding, cv.dilation))
    return st(torch.relu(F.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)))


def model_ref(m: nn.Module, x: torch.Tensor, emulate_bf16: bool = False) -> torch.Tensor:
    """the block alone (a DeformableConv2d) or the chain cv1 -> dcn -> cv2, in the precision of `m` and `x`"""
    st, wst = (Round.apply, bf16_mirror) if emulate_bf16 else (_SAME, _SAME)
    h = st(x)  # (the image is converted to the compute dtype; its gradient comes back through the same store)
    if hasattr(m, "dcn"):
        return cna_ref(m.cv2, dcn_ref(m.dcn, cna_ref(m.cv1, h, st, wst), st, wst), st, wst)
    return dcn_ref(m, h, st, wst)


def offset_map(m: nn.Module, x: torch.Tensor) -> "tuple[torch.Tensor, nn.Module]":
    """(the offset map the model's DeformableConv2d computes for input x, that DeformableConv2d), in the precision of m and x"""
    dcn, h = (m.dcn, cna_ref(m.cv1, x)) if hasattr(m, "dcn") else (m, x)
    c = dcn.conv
    return F.conv2d(h, dcn.conv_offset.weight, dcn.conv_offset.bias, c.stride[0], c.padding[0], c.dilation[0]), dcn


def init_module(m: nn.Module, seed: int = SEED) -> nn.Module:
    """deterministic parameters of useful size: N(0, 0.1^2), the offset convolution's a little larger so that the offsets reach
    beyond a pixel (torch's default initialisation leaves them at a few tenths); BatchNorm weights around 1"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * (0.12 if "conv_offset" in name else 0.1))
            if name.endswith("norm.weight"):
                prm.add_(1.0)
    return m


def module_input(shape, seed: int = SEED) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1000))


def loss_weights(shape, seed: int = SEED) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 2000))


def build_chain(comp, container) -> nn.Module:
    return container(OrderedDict(cv1=comp.ConvNormAct(*CHAIN_UNITS[0]), dcn=comp.DeformableConv2d(16, 24, 3, padding=1),
                                 cv2=comp.ConvNormAct(*CHAIN_UNITS[1])))


def gerr(a: torch.Tensor, b: torch.Tensor) -> float:
    """relative L2 error with the clamped denominator of the module tests (tests/test_convnext_gpu.py `_gerr`)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))
