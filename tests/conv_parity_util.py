"""Inputs, references, bounds and the case tables of the convolution parity tests (test_conv_parity_gpu.py runs the kernels
against them, test_conv_parity_cpu.py checks on the CPU that draws, references and bounds fit together).

Part A -- lattice inputs.  x, w, dz, residuals and pre-existing gradients are small integers, so every product and every
partial sum is an integer far below 2^24 and ANY summation order is exact in f32 (MFMA chunks, K split between two groups,
atomics, slabs).  Every output of magnitude <= 256 is a bf16 value, so the comparison is torch.equal in both dtypes.  With the
affine epilogue scale is 0.5 / 1 / 2 (a power of two never changes a significand), shift and the residual are EVEN integers:
relu(z * scale + shift) + residual is then a multiple of 1/2 below 128, an integer below 256 or an even integer below 512
for |z| <= 244 -- a bf16 value after each of the two stores.  lattice_ok() asserts this for the draw at hand.

Part B -- free-running inputs (oracle/filler.py), every element held to

    |got - ref64| <= r |ref64| + (1 + r) a (K + 1) u S  (+ the counted roundings of the epilogue, below)

u = 2^-24, r = 2^-8 for a bf16 store (0 for f32), K the number of products of an element, S the float64 convolution of |x|
with |w|: (K + 1) u S is the worst case of K products and adds in any order under IEEE rounding; a covers the MFMA's
internal adder (A_MFMA = 2 on the GPU, 1 for the CPU restatement)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from oracle import filler

U = 2.0 ** -24       # unit roundoff of f32
BF16_U = 2.0 ** -8   # unit roundoff of bf16 (8 significand bits, round to nearest even attains it)
A_MFMA = 2.0         # the MFMA's internal adder, uncharacterised: the factor the GPU bound grants it
F32, BF16 = 0, 1     # VT_F32, VT_BF16 (restated so that the CPU file needs no library)
TD = {F32: torch.float32, BF16: torch.bfloat16}
DNAME = {F32: "f32", BF16: "bf16"}

# epilogue flags (include/vt_amd.h)
RELU, STATS, RESIDUAL, AFFINE, D2S = 1, 2, 4, 8, 16
MODES = {"plain": 0, "stats": STATS, "res": RESIDUAL, "affine": AFFINE | RELU, "affine_res": AFFINE | RELU | RESIDUAL,
         "bnred": 0}  # bnred: vt_conv_dgrad_bnred, d(y) only (its sums: test_dgrad_bnred_gpu.py)

# counted f32 roundings of the epilogues, each against the magnitude of the value it rounds
K_AFFINE = 2         # z * scale, then + shift (2 where the compiler contracts them to one fma: counted as two)
K_RES_ADD = 1        # (stored value) + residual in f32, before the second store
K_PRE_GRAD = 1       # filter gradients: the sum is added to the gradient that is already there

# every dispatcher knob the cases set, with the value it is restored to
KNOB_DEFAULTS = {"VT_IGEMM_SPAN": 1, "VT_SPAN6": 1, "VT_PSPAN": 1, "VT_IGEMM_BN80": 1, "VT_IGEMM_W8": 3, "VT_SPAN_S2": 0,
                 "VT_SPAN6_MASK": 1, "VT_SPAN6_KSPLIT": 1, "VT_SPAN6_SPLIT": 1, "VT_STEM_TILES": 4, "VT_STEM6_KERNEL": 1,
                 "VT_WGRAD_S2_MINW": 0, "VT_WGRAD_S2_MINC": 32, "VT_WGRAD_GROUP_1X1": 0}
GENERAL = {"VT_IGEMM_SPAN": 0, "VT_SPAN6": 0, "VT_PSPAN": 0}  # the gather kernel of vt_igemm.hip for every shape


@dataclass(frozen=True)
class Conv:
    """one vt_conv_igemm launch: shape = (B, Cin, Cout, k, s, H, W); `kernel`: substrings last_kernel_name() must hold"""
    name: str
    shape: tuple
    dtype: int
    mode: str
    kernel: tuple
    knobs: dict = field(default_factory=dict, hash=False, compare=False)
    sliced: bool = False   # operands are channel slices of wider buffers, each with its own ld and offset
    flip: bool = False     # the tap order of a stride-1 data gradient
    partb: bool = False    # also run on free-running inputs

    @property
    def id(self):
        return f"{self.name}-{'x'.join(map(str, self.shape))}-{DNAME[self.dtype]}-{self.mode}" + ("-sliced" if self.sliced else "") + ("-flip" if self.flip else "")


@dataclass(frozen=True)
class Wgrad:
    """one filter gradient: entry = wgrad | slabs | group; n layers for group"""
    name: str
    shape: tuple
    dtype: int
    kernel: tuple
    entry: str = "wgrad"
    n: int = 1
    launches: int | None = None
    knobs: dict = field(default_factory=dict, hash=False, compare=False)
    sliced: bool = False
    partb: bool = False

    @property
    def id(self):
        return f"{self.name}-{'x'.join(map(str, self.shape))}-{DNAME[self.dtype]}-{self.entry}" + ("-sliced" if self.sliced else "")


def pad_of(k, s):
    return -((s - k) // 2)


def out_hw(shape):
    B, Cin, Cout, k, s, H, W = shape
    p = pad_of(k, s)
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  Each shape is the smallest that meets the dispatcher condition named beside it.
S6 = {"VT_SPAN6": 2}
S6P = {"VT_SPAN6": 2, "VT_SPAN6_MASK": 0, "VT_SPAN6_KSPLIT": 0}
S6M = {"VT_SPAN6": 2, "VT_SPAN6_MASK": 2, "VT_SPAN6_KSPLIT": 0}
SP2 = {"VT_IGEMM_SPAN": 2, "VT_SPAN6": 0, "VT_PSPAN": 0}
SP3 = {"VT_IGEMM_SPAN": 3, "VT_SPAN6": 0, "VT_PSPAN": 0}
S2D = {"VT_SPAN_S2": 2, "VT_SPAN6": 0, "VT_PSPAN": 0}
PS = {"VT_PSPAN": 2, "VT_SPAN6": 0}
W8 = lambda v, bn80=1: dict(GENERAL, VT_IGEMM_W8=v, VT_IGEMM_BN80=bn80)  # noqa: E731

CONV_CASES = [
    # ---- vt_igemm.hip, the gather kernel (vt_conv_igemm's last resort; GENERAL switches the span kernels off) ----
    # Cout == 160 and W8 bit 0: 256 x 160.  Cin = 40: chunk tail (uk0); M = 126: a map smaller than one tile
    Conv("g160", (2, 40, 160, 3, 1, 9, 7), BF16, "plain", ("igemm_kernel<bf16,256,160,4,2,2,uk0",), W8(3), partb=True),
    Conv("g160", (2, 40, 160, 3, 1, 9, 7), BF16, "affine_res", ("igemm_kernel<bf16,256,160",), W8(3), sliced=True),
    # Cout % 80 == 0, <= 160, W8 bit 0 clear: 256 x 80.  Cout = 80; Cin = 24 (chunk tail); M = 297: two tiles, B odd
    Conv("g80", (3, 24, 80, 3, 1, 11, 9), BF16, "stats", ("igemm_kernel<bf16,256,80,4,1,2,uk0",), W8(2), partb=True),
    # ... and Cout = 160 as two 80-wide tiles; 1x1, Cin = 96: three chunks
    Conv("g80x2", (1, 96, 160, 1, 1, 17, 16), BF16, "affine", ("igemm_kernel<bf16,256,80,4,1,2,uk1",), W8(2), sliced=True),
    # Cout > 64, W8 bits 1 and 2 (bit 2: below 256 tiles too): 256 x 128.  Cout = 136: 8 columns of the second tile;
    # Cin = 160: five chunks; M = 429 ends inside a row of the second image
    Conv("g256x128", (3, 160, 136, 3, 1, 13, 11), BF16, "plain", ("igemm_kernel<bf16,256,128,4,2,2,uk1",), W8(7), partb=True),
    Conv("g256x128", (3, 160, 136, 3, 1, 13, 11), BF16, "res", ("igemm_kernel<bf16,256,128",), W8(7), sliced=True, flip=True),
    # Cout > 64, W8 = 0 (72 % 80 != 0): 128 x 128.  Cout = 72 of 128, Cin = 40, M = 105 (test_kernels_gpu CONV_CASES)
    Conv("g128x128", (3, 40, 72, 3, 1, 7, 5), BF16, "stats", ("igemm_kernel<bf16,128,128,2,2,2,uk0",), W8(0), partb=True),
    # ... the stride-2 gather on it (CONV_CASES; K = 2304: the narrow x)
    Conv("g128x128s2", (2, 256, 128, 3, 2, 14, 14), BF16, "affine_res", ("igemm_kernel<bf16,128,128,2,2,2,uk1",), W8(0),
         sliced=True, partb=True),
    # 32 < Cout <= 64: 128 x 64.  Cout = 40 of 64, Cin = 24, M = 330, B odd
    Conv("g128x64", (5, 24, 40, 3, 1, 11, 6), BF16, "affine_res", ("igemm_kernel<bf16,128,64,2,2,2,uk0",), GENERAL, sliced=True,
         partb=True),
    Conv("g128x64", (5, 24, 40, 3, 1, 11, 6), BF16, "plain", ("igemm_kernel<bf16,128,64,2,2,2,uk0",), GENERAL, flip=True),
    # Cout <= 32: 256 x 32.  The 6x6 stride-2 gather (CONV_CASES), Cin = 8
    Conv("g256x32k6", (2, 8, 16, 6, 2, 12, 12), BF16, "stats", ("igemm_kernel<bf16,256,32,4,1,2,uk0",), GENERAL, partb=True),
    # ... 3x3 stride 2, Wo = 29 (tiles end inside a row), Cout = 24 of 32, four tiles (CONV_CASES)
    Conv("g256x32s2", (1, 16, 24, 3, 2, 60, 58), BF16, "affine", ("igemm_kernel<bf16,256,32,4,1,2,uk0",), GENERAL, sliced=True),
    # Wo = 1
    Conv("gWo1", (3, 16, 32, 3, 1, 5, 1), BF16, "plain", ("igemm_kernel<bf16,256,32",), GENERAL, partb=True),
    # f32, Cout > 32: 128 x 64 (two filter tiles, the second 8 wide); Cout <= 32: 128 x 32, stride 2 and 1x1
    Conv("g128x64", (3, 40, 72, 3, 1, 7, 5), F32, "stats", ("igemm_kernel<f32,128,64,2,2,2",), GENERAL, partb=True),
    Conv("g128x64", (3, 40, 72, 3, 1, 7, 5), F32, "affine_res", ("igemm_kernel<f32,128,64,2,2,2",), GENERAL, sliced=True, partb=True),
    Conv("g128x32s2", (2, 8, 24, 3, 2, 10, 10), F32, "plain", ("igemm_kernel<f32,128,32,4,1,2",), GENERAL, partb=True),
    Conv("g128x32k1", (2, 16, 32, 1, 1, 8, 8), F32, "res", ("igemm_kernel<f32,128,32,4,1,2",), GENERAL, sliced=True),
    Conv("g128x32k6", (2, 8, 16, 6, 2, 12, 12), F32, "affine", ("igemm_kernel<f32,128,32,4,1,2",), GENERAL),
    # ---- vt_igemm_span.hip (stride 1, Ho x Wo = Hi x Wi, Cin % 32 == 0 in bf16 / % 16 in f32) ----
    # VT_IGEMM_SPAN=2, fewer than 384 256-row tiles: 128-row tiles, the three widths
    Conv("s128x32", (4, 32, 32, 3, 1, 33, 17), BF16, "stats", ("span_kernel<bf16,128,32,4,1,2>",), SP2, partb=True),
    Conv("s128x64", (2, 32, 40, 3, 1, 9, 7), BF16, "affine_res", ("span_kernel<bf16,128,64,4,1,2>",), SP2, sliced=True),
    Conv("s128x128", (1, 64, 136, 3, 1, 14, 14), BF16, "plain", ("span_kernel<bf16,128,128,2,2,2>",), SP2, partb=True),
    Conv("s128x128", (1, 64, 136, 3, 1, 14, 14), BF16, "res", ("span_kernel<bf16,128,128,2,2,2>",), SP2, sliced=True, flip=True),
    Conv("s128x64k1", (2, 128, 64, 1, 1, 12, 12), BF16, "affine", ("span_kernel<bf16,128,64,4,1,2>",), SP2),
    # VT_IGEMM_SPAN=3 and Cout > 64: 224 rows whenever both heights need one round of 512 tiles (every test size).
    # Cin = 96: three chunks; M = 675 = 3 x 224 + 3
    Conv("s224", (3, 96, 72, 3, 1, 15, 15), BF16, "stats", ("span_kernel<bf16,224,128,2,2,2>",), SP3, partb=True),
    Conv("s224", (3, 96, 72, 3, 1, 15, 15), BF16, "affine_res", ("span_kernel<bf16,224,128,2,2,2>",), SP3, sliced=True),
    # ... 256 x 128 needs ceil(M / 224) > 512 >= ceil(M / 256): M = 115,200
    Conv("s256x128", (2, 32, 72, 3, 1, 240, 240), BF16, "plain", ("span_kernel<bf16,256,128,2,2,2>",), SP3),
    # ... Cout <= 64: always 256 rows.  Cin = 160: five chunks
    Conv("s256x64", (2, 160, 40, 3, 1, 13, 11), BF16, "affine", ("span_kernel<bf16,256,64,4,1,2>",), SP3, partb=True),
    Conv("s256x32", (5, 32, 24, 3, 1, 12, 10), BF16, "res", ("span_kernel<bf16,256,32,4,1,2>",), SP3, sliced=True, flip=True),
    # f32: 128 rows
    Conv("s128x32", (2, 16, 16, 3, 1, 9, 9), F32, "stats", ("span_kernel<f32,128,32,4,1,2>",), SP2, partb=True),
    Conv("s128x128", (2, 32, 72, 3, 1, 9, 7), F32, "affine_res", ("span_kernel<f32,128,128,2,2,2>",), SP2, sliced=True, partb=True),
    Conv("s128x64", (2, 32, 40, 3, 1, 9, 7), F32, "plain", ("span_kernel<f32,128,64,4,1,2>",), SP2, flip=True),
    # VT_SPAN_S2=2: 3x3 stride 2 on even maps, Cin % 32 == 0, the three widths (test_span_s2_gpu / CONV_CASES shapes)
    Conv("s2d64", (2, 32, 64, 3, 2, 56, 56), BF16, "stats", ("span_kernel<bf16,128,64,4,1,2,s2d>",), S2D, partb=True),
    Conv("s2d128", (2, 64, 128, 3, 2, 64, 72), BF16, "affine_res", ("span_kernel<bf16,128,128,2,2,2,s2d>",), S2D, sliced=True),
    Conv("s2d32", (1, 32, 24, 3, 2, 60, 58), BF16, "plain", ("span_kernel<bf16,128,32,4,1,2,s2d>",), S2D, partb=True),
    # test_span_s2_gpu.CASES, the ones with a comment: 160 columns (two filter-column tiles, the second a quarter full); four
    # chunks (every plane slot is reloaded three times); three chunks; 32-wide tile with tiles ending inside rows and images;
    # Wo = 4; a map smaller than a tile with 16 output channels; Wo = 1; Wo = 112 (the longest spans)
    Conv("s2d160", (1, 64, 160, 3, 2, 30, 34), BF16, "plain", ("span_kernel<bf16,128,128,2,2,2,s2d>",), S2D, sliced=True),
    Conv("s2d4ch", (2, 128, 256, 3, 2, 28, 28), BF16, "stats", ("span_kernel<bf16,128,128,2,2,2,s2d>",), S2D),
    Conv("s2d3ch", (2, 96, 64, 3, 2, 16, 16), BF16, "affine_res", ("span_kernel<bf16,128,64,4,1,2,s2d>",), S2D, sliced=True),
    Conv("s2d32e", (3, 32, 32, 3, 2, 20, 12), BF16, "affine", ("span_kernel<bf16,128,32,4,1,2,s2d>",), S2D),
    Conv("s2dWo4", (5, 32, 64, 3, 2, 8, 8), BF16, "stats", ("span_kernel<bf16,128,64,4,1,2,s2d>",), S2D, sliced=True),
    Conv("s2dsmall", (2, 32, 16, 3, 2, 4, 6), BF16, "affine_res", ("span_kernel<bf16,128,32,4,1,2,s2d>",), S2D),
    Conv("s2dWo1", (7, 32, 64, 3, 2, 2, 2), BF16, "plain", ("span_kernel<bf16,128,64,4,1,2,s2d>",), S2D),
    Conv("s2dWo112", (1, 32, 64, 3, 2, 224, 224), BF16, "stats", ("span_kernel<bf16,128,64,4,1,2,s2d>",), S2D),
    # ---- vt_igemm_pspan.hip (VT_PSPAN=2; Cin % 32 == 0, Cout <= 128, a resident filter of <= 96 KiB) ----
    Conv("p32", (4, 32, 32, 3, 1, 33, 17), BF16, "stats", ("pspan_kernel<bf16,", ",32,8+4 waves,s1,"), PS, partb=True),
    Conv("p64", (3, 64, 40, 3, 1, 15, 15), BF16, "affine_res", ("pspan_kernel<bf16,", ",64,8+4 waves,s1,"), PS, sliced=True, partb=True),
    Conv("p128", (2, 32, 72, 3, 1, 20, 13), BF16, "res", ("pspan_kernel<bf16,128,128,8+4 waves,s1,",), PS, flip=True),
    Conv("p128", (2, 32, 72, 3, 1, 20, 13), BF16, "plain", ("pspan_kernel<bf16,128,128,8+4 waves,s1,",), PS, sliced=True),
    Conv("ps2d64", (2, 32, 64, 3, 2, 56, 56), BF16, "plain", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS, partb=True),
    Conv("ps2d32", (1, 32, 24, 3, 2, 60, 58), BF16, "affine", ("pspan_kernel<bf16,", ",32,8+4 waves,s2d,"), PS, sliced=True),
    # test_pspan_gpu.CASES, the ones with a comment: 1x1 (one step per chunk, four chunks); three chunks; several tiles per
    # workgroup range with a long halo; stride 2 with two chunks (every plane span is reloaded); Wo = 4 (most fragments wrap
    # rows); a map smaller than a tile; Wo = 1; Wo = 112 (the longest plane spans)
    Conv("p1x1", (2, 128, 128, 1, 1, 12, 12), BF16, "stats", ("pspan_kernel<bf16,", ",128,8+4 waves,s1,"), PS),
    Conv("p1x1", (2, 64, 40, 1, 1, 7, 5), BF16, "affine_res", ("pspan_kernel<bf16,", ",64,8+4 waves,s1,"), PS, sliced=True),
    Conv("p3ch", (1, 96, 32, 3, 1, 40, 24), BF16, "plain", ("pspan_kernel<bf16,", ",32,8+4 waves,s1,"), PS, flip=True),
    Conv("phalo", (1, 32, 32, 3, 1, 130, 70), BF16, "affine", ("pspan_kernel<bf16,", ",32,8+4 waves,s1,"), PS, sliced=True),
    Conv("ps2d2ch", (2, 64, 64, 3, 2, 64, 72), BF16, "stats", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS),
    Conv("ps2dWo4", (5, 32, 64, 3, 2, 8, 8), BF16, "affine_res", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS, sliced=True),
    Conv("ps2dsmall", (2, 32, 16, 3, 2, 4, 6), BF16, "plain", ("pspan_kernel<bf16,", ",32,8+4 waves,s2d,"), PS),
    Conv("ps2dWo1", (7, 32, 64, 3, 2, 2, 2), BF16, "stats", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS, sliced=True),
    Conv("ps2dWo112", (1, 32, 64, 3, 2, 224, 224), BF16, "plain", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS),
    # more than 256 tiles (M = 75,264 > 256 x 256): a workgroup walks several tiles and the span ring is carried from one
    # to the next, as in the benchmark (the default dispatch takes this kernel from M = 262,144)
    Conv("pmany", (6, 32, 32, 3, 1, 112, 112), BF16, "stats", ("pspan_kernel<bf16,", ",32,8+4 waves,s1,"), PS, partb=True),
    Conv("pmany", (6, 32, 32, 3, 1, 112, 112), BF16, "affine_res", ("pspan_kernel<bf16,", ",32,8+4 waves,s1,"), PS, sliced=True),
    Conv("ps2dmany", (6, 32, 64, 3, 2, 224, 224), BF16, "plain", ("pspan_kernel<bf16,", ",64,8+4 waves,s2d,"), PS, partb=True),
    Conv("pmany128", (3, 32, 72, 3, 1, 112, 112), BF16, "res", ("pspan_kernel<bf16,128,128,8+4 waves,s1,",), PS, flip=True),
    # 128 columns: nine K-steps x 128 x 64 B = 72 KiB of resident filter, 128-row tiles only
    Conv("ps2d128", (3, 32, 72, 3, 2, 20, 24), BF16, "stats", ("pspan_kernel<bf16,128,128,8+4 waves,s2d,",), PS, partb=True),
    # ---- vt_igemm_span6.hip (VT_SPAN6=2; Cin >= 64, Cin % 32 == 0, M x filter tiles >= 65,536 even when forced) ----
    # padded positions (MASK=0).  96 x 96: 7 piece taps, the widest map whose span fits the LDS
    Conv("s6pad", (8, 64, 128, 3, 1, 96, 96), BF16, "plain", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P, partb=True),
    # Cout = 160 with statistics runs unsplit: 32 columns of the second tile; Cin = 96
    Conv("s6pad160", (16, 96, 160, 3, 1, 64, 80), BF16, "stats", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P, sliced=True),
    # odd sizes, M = 66,600 (no multiple of 32), B even
    Conv("s6padodd", (40, 64, 128, 3, 1, 45, 37), BF16, "affine_res", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P, sliced=True),
    Conv("s6padodd", (40, 64, 128, 3, 1, 45, 37), BF16, "bnred", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P, flip=True, partb=True),
    # pixel rows with per-tap masks (MASK=2)
    Conv("s6mask", (40, 64, 128, 3, 1, 45, 37), BF16, "res", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, flip=True, partb=True),
    Conv("s6mask", (8, 64, 128, 3, 1, 96, 96), BF16, "stats", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, sliced=True),
    Conv("s6mask", (8, 64, 128, 3, 1, 96, 96), BF16, "affine", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M),
    Conv("s6mask", (40, 64, 128, 3, 1, 45, 37), BF16, "bnred", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, sliced=True, flip=True),
    # test_span6_gpu.SHAPES, the ones with a comment: maps wider than 96 (the tile height drops to 6 units at Wp = 113 and to
    # 5 at Wp = 141); three filter tiles (do not divide the 32 workgroups of an XCD: rslots and the g8 split change); odd
    # batch with two filter tiles; the dominant layer's geometry at 3/8 of the batch; VoVNet-39 stage 2 (160 columns with
    # statistics: unsplit, five chunks)
    Conv("s6w112", (6, 64, 128, 3, 1, 112, 112), BF16, "plain", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P),
    Conv("s6w140", (8, 64, 128, 3, 1, 60, 140), BF16, "affine_res", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, sliced=True),
    Conv("s6w140", (8, 64, 128, 3, 1, 60, 140), BF16, "plain", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P, flip=True),
    Conv("s6t3", (12, 64, 384, 3, 1, 41, 52), BF16, "stats", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P),
    Conv("s6t3", (12, 64, 384, 3, 1, 41, 52), BF16, "res", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, sliced=True, flip=True),
    Conv("s6b33", (33, 64, 256, 3, 1, 29, 71), BF16, "plain", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M, sliced=True),
    Conv("s6b33", (33, 64, 256, 3, 1, 29, 71), BF16, "affine", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P),
    Conv("s6dom", (96, 128, 128, 3, 1, 28, 28), BF16, "affine", ("span6_kernel<bf16,2x4+4 waves,FM", "!masked"), S6P),
    Conv("s6vov", (128, 160, 160, 3, 1, 28, 28), BF16, "stats", ("span6_kernel<bf16,2x4+4 waves,FM", ",masked>"), S6M),
    # K split between the two groups: Cin >= 256, Cin % 64 == 0, M x tiles >= 24,576, every workgroup's rows in one tile
    Conv("s6ks", (24, 256, 128, 3, 1, 32, 32), BF16, "plain", ("masked,ksplit>",), S6, partb=True),
    Conv("s6ks", (24, 256, 128, 3, 1, 32, 32), BF16, "stats", ("masked,ksplit>",), S6, sliced=True),
    Conv("s6ks", (24, 256, 128, 3, 1, 32, 32), BF16, "affine_res", ("masked,ksplit>",), S6, sliced=True),
    Conv("s6ks", (24, 256, 128, 3, 1, 32, 32), BF16, "bnred", ("masked,ksplit>",), S6, flip=True, partb=True),
    # test_span6_gpu.KSPLIT_SHAPES: an odd map with rows no multiple of 32 (K = 4608: the sparse lattice); three filter tiles
    Conv("s6ksodd", (192, 512, 256, 3, 1, 9, 11), BF16, "res", ("masked,ksplit>",), S6, sliced=True, flip=True),
    Conv("s6kst3", (200, 256, 384, 3, 1, 8, 8), BF16, "stats", ("masked,ksplit>",), S6),
    # ---- vt_stem.hip / vt_stem6.hip (Cin = ldx = 8: x is never a slice) ----
    Conv("stem4", (2, 8, 32, 3, 1, 20, 13), BF16, "stats", ("stem_t_kernel<4,1>",), {"VT_STEM_TILES": 4}, sliced=True, partb=True),
    Conv("stem4", (3, 8, 24, 3, 1, 17, 17), BF16, "affine", ("stem_t_kernel<4,0>",), {"VT_STEM_TILES": 4}),
    Conv("stem2", (2, 8, 32, 3, 1, 20, 13), BF16, "affine", ("stem_t_kernel<2,0>",), {"VT_STEM_TILES": 2}, sliced=True, partb=True),
    Conv("stem2", (3, 8, 24, 3, 1, 17, 17), BF16, "stats", ("stem_t_kernel<2,1>",), {"VT_STEM_TILES": 2}),
    Conv("stem0", (3, 8, 24, 3, 1, 17, 17), BF16, "plain", ("stem_kernel<32>",), {"VT_STEM_TILES": 0}, sliced=True, partb=True),
    Conv("stem64", (1, 8, 64, 3, 1, 9, 40), BF16, "stats", ("stem_kernel<64>",), {}, partb=True),
    Conv("stem64", (1, 8, 64, 3, 1, 9, 40), BF16, "affine", ("stem_kernel<64>",), {}, sliced=True),
    # the 6x6 stride-2 stem of the YOLOv5 Darknets: Cout = 80, h0 = w0 = -2 (test_yolov5_stem_kernel's smallest shape)
    Conv("stem6", (2, 8, 80, 6, 2, 24, 20), BF16, "affine", ("stem6_kernel<80>",), {}, sliced=True, partb=True),
    Conv("stem6", (1, 8, 80, 6, 2, 8, 130), BF16, "plain", ("stem6_kernel<80>",), {}),
]

WGRAD_CASES = [
    # ---- vt_wgrad.hip, the general kernel: unit (1x1 stride 1) and gather, both dtypes (CONV_CASES shapes) ----
    Wgrad("unit", (2, 16, 32, 1, 1, 8, 8), BF16, ("wgrad_kernel<bf16,2,1,unit>",), partb=True),
    Wgrad("unit", (2, 128, 64, 1, 1, 12, 12), BF16, ("wgrad_kernel<bf16,2,1,unit>",), sliced=True),
    Wgrad("gather_s2", (2, 8, 24, 3, 2, 10, 10), BF16, ("wgrad_kernel<bf16,2,1,gather>",), partb=True),
    Wgrad("gather_k6", (2, 8, 16, 6, 2, 12, 12), BF16, ("wgrad_kernel<bf16,2,1,gather>",), sliced=True),
    Wgrad("gather_s2", (2, 256, 128, 3, 2, 14, 14), BF16, ("wgrad_kernel<bf16,2,1,gather>",)),
    Wgrad("unit", (2, 16, 32, 1, 1, 8, 8), F32, ("wgrad_kernel<f32,2,1,unit>",), sliced=True, partb=True),
    Wgrad("gather", (3, 40, 72, 3, 1, 7, 5), F32, ("wgrad_kernel<f32,2,1,gather>",), partb=True),
    Wgrad("gather_s2", (2, 8, 24, 3, 2, 10, 10), F32, ("wgrad_kernel<f32,2,1,gather>",), sliced=True),
    # ---- vt_wgrad_span.hip: bf16 3x3 stride 1 with Cin <= 32 or Cout <= 32 (wider layers: wgrad6) ----
    Wgrad("ws11", (2, 16, 16, 3, 1, 9, 9), BF16, ("wgrad_span_kernel<1,1,",), partb=True),
    Wgrad("ws21", (2, 24, 72, 3, 1, 11, 6), BF16, ("wgrad_span_kernel<2,1,",), sliced=True, partb=True),
    Wgrad("ws12", (3, 40, 24, 3, 1, 7, 5), BF16, ("wgrad_span_kernel<1,2,",), partb=True),
    # ... both wider than 32 reach it only in the two-stage mode (wgrad6 flushes with atomics): the `wide` form
    Wgrad("wswide", (1, 64, 136, 3, 1, 14, 14), BF16, ("wgrad_span_kernel<2,2,", ",wide>"), entry="slabs", sliced=True, partb=True),
    # ---- the row-parity stride-2 dispatch (VT_WGRAD_S2_MINW=1): two launches, x dense, even maps, Cin <= 127 ----
    Wgrad("s2rows", (2, 32, 64, 3, 2, 56, 56), BF16, ("wgrad_span_kernel<2,2,",), launches=2,
          knobs={"VT_WGRAD_S2_MINW": 1, "VT_WGRAD_S2_MINC": 8}, partb=True),
    Wgrad("s2rows", (1, 16, 24, 3, 2, 60, 58), BF16, ("wgrad_span_kernel<1,1,",), launches=2,
          knobs={"VT_WGRAD_S2_MINW": 1, "VT_WGRAD_S2_MINC": 8}),
    # ---- vt_wgrad6.hip: bf16 3x3 stride 1, Cin > 32 and Cout > 32; alone and three layers in one launch ----
    Wgrad("w6", (3, 40, 72, 3, 1, 7, 5), BF16, ("wgrad6_kernel<PD", ",G1,"), partb=True),
    Wgrad("w6", (2, 160, 160, 3, 1, 7, 7), BF16, ("wgrad6_kernel<PD", ",G1,"), sliced=True),
    Wgrad("w6", (1, 64, 136, 3, 1, 14, 14), BF16, ("wgrad6_kernel<PD", ",G3,"), entry="group", n=3, launches=1, partb=True),
    # ... a map 100 wide: the taps span 204 positions, four 64-position halo chunks, so the ring keeps PD = 2 ahead
    Wgrad("w6pd2", (1, 40, 72, 3, 1, 6, 100), BF16, ("wgrad6_kernel<PD2,G1,",)),
    # ---- vt_conv_wgrad_slabs on the general kernel (M = 1568: two splits), vt_conv_wgrad_group on 1x1 layers ----
    Wgrad("slabs_s2", (2, 32, 64, 3, 2, 56, 56), BF16, ("wgrad_kernel<bf16,2,1,gather>",), entry="slabs", partb=True),
    Wgrad("slabs_f32", (2, 16, 16, 3, 1, 24, 40), F32, ("wgrad_kernel<f32,2,1,gather>",), entry="slabs", sliced=True),
    Wgrad("group1x1", (2, 128, 64, 1, 1, 12, 12), BF16, ("wgrad_kernel<bf16,2,1,unit>",), entry="group", n=2, launches=1,
          knobs={"VT_WGRAD_GROUP_1X1": 1}, partb=True),
]

# Stride-2 3x3 data gradient: B, Cin (channels of x), Cout (channels of dz), H, W of x, ld of dx, folded residual, knobs,
# substrings of the kernel name of the ONE depth-to-space launch, and of each of the four class launches (32 or 16 columns,
# 1 / 2 / 2 / 4 taps)  (test_dgrad_d2s_gpu.CASES, its smaller shapes)
D2S_CASES = [
    # 64 columns, 24 dz channels (a chunk tail): the gather kernel's 128 x 64 tile
    (2, 16, 24, 20, 28, 16, True, {}, ("igemm_kernel<bf16,128,64,2,2,2,uk0",), ("igemm_kernel<bf16,256,32,4,1,2,uk0>",)),
    # d(x) a channel slice; 48 dz channels (% 32 != 0: no span kernel), 128 columns on 6 tiles: 128 x 128
    (3, 32, 48, 36, 52, 64, True, {}, ("igemm_kernel<bf16,128,128,2,2,2,uk0",), ("igemm_kernel<bf16,256,32,4,1,2,uk0>",)),
    # 128 columns, dz channels % 32 == 0: the span kernel (forced: below 384 tiles the 128-wide tile goes to the gather kernel)
    (2, 32, 64, 24, 40, 48, False, {"VT_IGEMM_SPAN": 2, "VT_PSPAN": 0}, ("span_kernel<bf16,128,128,2,2,2>",),
     ("span_kernel<bf16,128,32,4,1,2>",)),
    # ... the persistent span kernel when forced
    (2, 32, 64, 24, 40, 48, True, {"VT_PSPAN": 2}, ("pspan_kernel<bf16,128,128,8+4 waves,s1,",),
     ("pspan_kernel<bf16,", ",32,8+4 waves,s1,")),
]


# ---------------------------------------------------------------------------------------------------------------------
def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


def lattice(tag, shape, amp, even=False):
    """integers of [-amp, amp] (even: multiples of 2 of [-2 amp, 2 amp]) as f32"""
    g = _gen(tag)
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=g).float()
    while (v != 0).float().mean().item() < 0.5:  # (a filter of 8 entries: the next draw of the same stream)
        v = torch.randint(-amp, amp + 1, tuple(shape), generator=g).float()
    return v * 2 if even else v


def scales(tag, C):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=_gen(tag))]


def sparse(tag, shape):
    """-1 / 0 / 1 with weights 3 : 4 : 3 (60 % non-zero): the draw of x and w where K > 2304, so that |z| stays below 244"""
    table = torch.tensor([-1.0] * 3 + [0.0] * 4 + [1.0] * 3)
    return table[torch.randint(0, 10, tuple(shape), generator=_gen(tag))]


def x_amp(K):
    return 2 if K <= 576 else 1  # (|z| stays below 256: the table of the module docstring's source, checked per case)


_CACHE: dict = {}


def cached(fn):
    def wrap(*key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            if len(_CACHE) > 6:  # a few large operand sets alive at a time
                _CACHE.pop(next(iter(_CACHE)))
            _CACHE[k] = fn(*key)
        return _CACHE[k]
    return wrap


def w_ref(w, flip):
    """OIHW filter the reference convolves with: memory tap i sits at offset (t // k, t % k), t = k*k-1-i when flipped"""
    return w.flip(2, 3) if flip else w


@cached
def conv_operands(shape, flip, lat, dtype):
    """x, w (NCHW / OIHW, f32 holding dtype-representable values), z = conv (f32 exact for lattice, else float64), S"""
    B, Cin, Cout, k, s, H, W = shape
    K = Cin * k * k
    if lat:
        x = lattice(f"x{shape}", (B, Cin, H, W), x_amp(K)) if K <= 2304 else sparse(f"x{shape}", (B, Cin, H, W))
        w = lattice(f"w{shape}", (Cout, Cin, k, k), 1) if K <= 2304 else sparse(f"w{shape}", (Cout, Cin, k, k))
        z = F.conv2d(x, w_ref(w, flip), None, s, pad_of(k, s))
        return x, w, z, None
    x = filler.tensor(f"x{shape}", (B, Cin, H, W)).to(TD[dtype]).float()
    w = filler.tensor(f"w{shape}", (Cout, Cin, k, k), scale=(2.0 / K) ** 0.5).to(TD[dtype]).float()
    z = F.conv2d(x.double(), w_ref(w, flip).double(), None, s, pad_of(k, s))
    S = F.conv2d(x.double().abs(), w_ref(w, flip).double().abs(), None, s, pad_of(k, s))
    return x, w, z, S


def epilogue_operands(case, lat):
    """scale, shift (f32 [Cout]) and the residual (NCHW f32) of a case, None where its mode has none"""
    B, Cin, Cout, k, s, H, W = case.shape
    Ho, Wo = out_hw(case.shape)
    flags = MODES[case.mode]
    sc = sh = res = None
    tag = f"{case.shape}{case.mode}"
    if flags & AFFINE:
        sc = scales("sc" + tag, Cout) if lat else (filler.tensor("sc" + tag, (Cout,)) * 0.5 + 1.0)
        sh = lattice("sh" + tag, (Cout,), 2, even=True) if lat else filler.tensor("sh" + tag, (Cout,)) * 0.2
    if flags & RESIDUAL:
        res = lattice("r" + tag, (B, Cout, Ho, Wo), 1, even=True) if lat else \
            filler.tensor("r" + tag, (B, Cout, Ho, Wo)).to(TD[case.dtype]).float()
    return sc, sh, res


def conv_reference(case, lat):
    """(ref, v): the epilogue of `case` on the float64 (lattice: exact f32) convolution -- ref the output, v the value before
    the residual add (the first of the two bf16 stores; v is ref where the mode has no residual)"""
    x, w, z, S = conv_operands(case.shape, case.flip, lat, case.dtype)
    sc, sh, res = epilogue_operands(case, lat)
    flags = MODES[case.mode]
    c = lambda v: v.to(z.dtype)[None, :, None, None]  # noqa: E731
    v = z
    if flags & AFFINE:
        v = v * c(sc) + c(sh)
    if flags & RELU:
        v = torch.relu(v)
    ref = v + res.to(z.dtype) if res is not None else v
    return ref, v


def conv_bound(case, a):
    """Part B bound per element.  e_z = a (K + 1) u S is the accumulator's error.
    affine:   t = fl(fl(z sc) + sh): |sc| e_z + K_AFFINE u (|sc| S + |sh|)   (each rounding acts on a value <= |sc| S + |sh|)
    relu:     1-Lipschitz, no rounding
    store:    r |v| (round to nearest even), the error before it grows by (1 + r)
    residual: bf16 rounds v FIRST (the r |v| above), then adds in f32 (K_RES_ADD u (|v| + |res|)) and stores again (r |ref|)"""
    x, w, z, S = conv_operands(case.shape, case.flip, False, case.dtype)
    ref, v = conv_reference(case, False)
    sc, sh, res = epilogue_operands(case, False)
    B, Cin, Cout, k, s, H, W = case.shape
    K = Cin * k * k
    r = BF16_U if case.dtype == BF16 else 0.0
    c = lambda t: t.double().abs()[None, :, None, None]  # noqa: E731
    e = a * (K + 1) * U * S
    if sc is not None:
        e = c(sc) * e + K_AFFINE * U * (c(sc) * S + c(sh))
    if res is None:
        return r * ref.abs() + (1 + r) * e
    inner = r * v.abs() + (1 + r) * e                       # the first store (bf16) -- f32 keeps v in registers: r = 0
    inner = inner + K_RES_ADD * U * (v.abs() + res.double().abs()) * (1 + r)
    return r * ref.abs() + (1 + r) * inner


def lattice_ok(ref, dtype, *operands):
    """the conditions of Part A for one case: every reference value is a value of the output dtype (f32 outputs: an
    integer multiple of 1/2 below 2^24), and at least half of the entries of each operand are non-zero"""
    if dtype == BF16:
        assert torch.equal(ref.to(torch.bfloat16).double(), ref.double()), "a lattice reference value is no bf16 value"
    assert ref.abs().max().item() < 2 ** 24
    for t in operands:
        if t is not None:
            assert (t != 0).double().mean().item() >= 0.5, "an operand is mostly zeros"


def stored_ok(case, ref, v):
    """bf16 with a residual stores twice: the value before the add has to be representable too"""
    if case.dtype == BF16:
        assert torch.equal(v.to(torch.bfloat16).double(), v.double())
        assert torch.equal(ref.to(torch.bfloat16).double(), ref.double())


# ---- filter gradients --------------------------------------------------------------------------------------------------
@cached
def wgrad_operands(shape, lat, dtype, layer):
    """x, dz (NCHW), g0 (the gradient already there, [Cout][k][k][Cin]), ref (same layout, g0 included), S"""
    B, Cin, Cout, k, s, H, W = shape
    Ho, Wo = out_hw(shape)
    tag = f"{shape}L{layer}"
    if lat:
        x = lattice("gx" + tag, (B, Cin, H, W), 2)
        dz = lattice("gdz" + tag, (B, Cout, Ho, Wo), 1)
        g0 = lattice("g0" + tag, (Cout, k, k, Cin), 3)
    else:
        x = filler.tensor("gx" + tag, (B, Cin, H, W)).to(TD[dtype]).float()
        dz = filler.tensor("gdz" + tag, (B, Cout, Ho, Wo)).to(TD[dtype]).float()
        g0 = filler.tensor("g0" + tag, (Cout, k, k, Cin))
    p = pad_of(k, s)

    def grad(xx, dd):
        # dw[o][c][r][t] = sum x[b][c][s i + r - p][s j + t - p] dz[b][o][i][j]: a convolution of x^T with dz^T, dilated by s
        g = F.conv2d(xx.transpose(0, 1), dd.transpose(0, 1), None, 1, p, dilation=s)  # [Cin][Cout][>=k][>=k]
        return g[:, :, :k, :k].permute(1, 2, 3, 0)
    T = torch.float32 if lat else torch.float64
    gw = grad(x.to(T), dz.to(T))
    ref = gw + g0.to(T)
    S = None if lat else grad(x.double().abs(), dz.double().abs())
    return x, dz, g0, ref, S


def wgrad_bound(shape, dtype, layer, a):
    """K = M products per element, f32 output (r = 0); the splits' partial sums are part of the K adds, the add to the
    gradient that is already there is one more rounding (K_PRE_GRAD) of a value <= S + |g0|"""
    x, dz, g0, ref, S = wgrad_operands(shape, False, dtype, layer)
    Ho, Wo = out_hw(shape)
    M = shape[0] * Ho * Wo
    return a * (M + 1) * U * S + K_PRE_GRAD * U * (S + g0.double().abs())


# ---- stride-2 data gradient ------------------------------------------------------------------------------------------
@cached
def d2s_operands(B, Cin, Cout, H, W, lat, with_res):
    """dz [B][Cout][H/2][W/2], w OIHW (of the forward conv Cin -> Cout), residual [B][Cin][H][W] or None, ref, S"""
    tag = f"d2s{(B, Cin, Cout, H, W)}"
    if lat:
        dz = lattice("dz" + tag, (B, Cout, H // 2, W // 2), 2)
        w = lattice("w" + tag, (Cout, Cin, 3, 3), 1)
        res = lattice("r" + tag, (B, Cin, H, W), 1, even=True) if with_res else None
        T = torch.float32
    else:
        dz = filler.tensor("dz" + tag, (B, Cout, H // 2, W // 2)).bfloat16().float()
        w = (filler.tensor("w" + tag, (Cout, Cin, 3, 3)) * 0.1).bfloat16().float()
        res = filler.tensor("r" + tag, (B, Cin, H, W)).bfloat16().float() if with_res else None
        T = torch.float64
    v = F.conv_transpose2d(dz.to(T), w.to(T), stride=2, padding=1, output_padding=1)
    S = None if lat else F.conv_transpose2d(dz.double().abs(), w.double().abs(), stride=2, padding=1, output_padding=1)
    ref = v + res.to(T) if with_res else v
    return dz, w, res, ref, v, S


def d2s_bound(B, Cin, Cout, H, W, with_res, a):
    """K <= 4 taps x Cout products (a zero tap of the filter image adds exact zeros); the folded residual as in conv_bound"""
    dz, w, res, ref, v, S = d2s_operands(B, Cin, Cout, H, W, False, with_res)
    r = BF16_U
    e = a * (4 * Cout + 1) * U * S
    if res is None:
        return r * ref.abs() + (1 + r) * e
    inner = r * v.abs() + (1 + r) * e + K_RES_ADD * U * (v.abs() + res.double().abs()) * (1 + r)
    return r * ref.abs() + (1 + r) * inner


def worst_ratio(got, ref, S, K, dtype):
    """(|got - ref| - r |ref|) / ((K + 1) u S), the largest over the elements: what the NOTEBOOK records per family"""
    r = BF16_U if dtype == BF16 else 0.0
    return (((got.double() - ref.double()).abs() - r * ref.double().abs()) / ((K + 1) * U * S.double()).clamp_min(1e-300)).max().item()


def within(got, ref, bound):
    d = (got.double() - ref.double()).abs()
    bad = d > bound
    return int(bad.sum()), (d / bound.clamp_min(1e-300)).max().item()


# ---- grouped and depthwise kernels (vt_gconv.hip, vt_dwtile.hip, vt_dwconv.hip): lattice cases only ------------------------
# vt_gconv3_*: (B, H, W, C, gw, stride), the smallest shapes of test_gconv_kernels_gpu.py: a map smaller than any tile; odd
# extents under stride 2; the 56-wide group (masked rows of the last 16-row tile); 13 groups (no multiple of four waves)
GCONV_SHAPES = [(2, 7, 7, 16, 8, 1), (3, 13, 11, 48, 16, 2), (2, 8, 8, 112, 56, 2), (2, 10, 10, 104, 8, 1)]
# vt_dwt_*: (B, H, W, C, k, stride), the smallest shapes of test_dwtile_kernels_gpu.py: two maps smaller than the filter;
# odd, non-square, 3 bf16 chunks under stride 2; 5x5 stride 1
DWT_SHAPES = [(1, 1, 1, 8, 3, 1), (1, 2, 3, 8, 5, 2), (2, 7, 7, 16, 3, 1), (3, 13, 11, 24, 3, 2), (2, 9, 9, 40, 5, 1)]
# vt_dwconv_*: (B, C, H, W, k, s, pad, dil), the smallest cases of test_dwconv_gpu.py: 1x1; stride 2; dilation 2 (pixels no
# output reads); 5x5 on 20 chunks (no power of two)
DWCONV_CASES = [(5, 8, 9, 9, 1, 1, 0, 1), (3, 32, 20, 18, 3, 2, 1, 1), (3, 24, 22, 26, 3, 2, 1, 2), (2, 160, 17, 17, 5, 1, 2, 1)]


def grouped_geometry(kind, shape):
    """-> B, C, H, W, k, s, pad, dil, groups, channels per group"""
    if kind == "gconv":
        B, H, W, C, gw, s = shape
        return B, C, H, W, 3, s, 1, 1, C // gw, gw
    if kind == "dwt":
        B, H, W, C, k, s = shape
        return B, C, H, W, k, s, (k - 1) // 2, 1, C, 1
    B, C, H, W, k, s, pad, dil = shape
    return B, C, H, W, k, s, pad, dil, C, 1


@cached
def grouped_operands(kind, shape):
    """lattice operands and exact results of a grouped / depthwise case, NCHW / OIHW f32: x, w, dz, res, g0 (the filter
    gradient already there, [C][k][k][gw]) -> z, dx, dxr = dx + res, dw (g0 included)"""
    B, C, H, W, k, s, pad, dil, groups, gw = grouped_geometry(kind, shape)
    tag = f"{kind}{shape}"
    x = lattice("x" + tag, (B, C, H, W), 2)
    w = lattice("w" + tag, (C, gw, k, k), 1)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z = F.conv2d(xd, wd, None, s, pad, dil, groups)
    dz = lattice("dz" + tag, tuple(z.shape), 1)
    z.backward(dz.double())
    res = lattice("r" + tag, (B, C, H, W), 1, even=True)
    g0 = lattice("g0" + tag, (C, k, k, gw), 3)
    return dict(x=x, w=w, dz=dz, res=res, g0=g0, z=z.detach().float(), dx=xd.grad.float(), dxr=(xd.grad + res.double()).float(),
                dw=(wd.grad.permute(0, 2, 3, 1) + g0.double()).float())


def grouped_ok(c, dtype):
    for key in ("z", "dx", "dxr"):
        lattice_ok(c[key], dtype)
    lattice_ok(c["dw"], F32, c["x"], c["w"], c["dz"], c["res"], c["g0"])
