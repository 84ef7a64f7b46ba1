"""Float64 references, inputs and elementwise bounds of the neck, loss and input-mixing kernel tests
(test_head_neck_kernels_gpu.py runs the kernels against them, test_head_neck_refs_cpu.py checks on the CPU that references,
inputs and bounds fit together).

Bounds are elementwise: |got - ref64| <= k * u * S (+ 2^-8 * |ref64| for the one round-to-nearest-even store of a bf16
result, see BF16_U), u = 2^-24, S the float64 sum of the absolute values of the terms that enter the element, k the count of f32
roundings of the kernel, read from vt_elementwise.hip and written next to each K_* below.  A relative rounding error e of a
term t contributes at most e * |t| <= e * S, so counting every rounding against S is an upper bound.

All values come from oracle/filler.py and are rounded to the storage dtype before a reference sees them.  Activations are
NHWC: [B, H, W, C] or [rows, C]."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import filler
from oracle import torch_ref as R

U = 2.0 ** -24           # unit roundoff of f32
# Unit roundoff of bf16.  The format has 8 significand bits (7 stored): neighbours in [1, 2) are 2^-7 apart, and round to
# nearest even moves a value by up to half of that, 2^-8 relative -- 1 + 2^-8 + tiny is stored as 1 + 2^-7.  (A term of
# 2^-9 |ref| would be the roundoff of a 9-bit significand: a correct store of -1.2705 as -1.2734 misses it, as
# test_head_neck_refs_cpu.py found with the first input it tried.)
BF16_U = 2.0 ** -8
F32, BF16 = 0, 1         # VT_F32, VT_BF16 (vision_toolbox._native; restated so that the CPU tests need no library)
TD = {F32: torch.float32, BF16: torch.bfloat16}
DNAME = {F32: "f32", BF16: "bf16"}
EPC = {F32: 4, BF16: 8}  # elements per 16-byte chunk
THREADS = 256            # kThreads (vt_rowmap.h)
LDS_FIX_QUANTUM = 2.0 ** -32  # lds_fix_add (vt_elementwise.hip): a row lane's partial sum is rounded to a multiple of it

# chunk counts of the RowMap kernels: 1; 3 (CT = 3, RT = 85, thread 255 idle); 257 (CT = 256, thread 0 takes a 2nd column)
CPRS = (1, 3, 257)
LONG_ROWS = 4224         # > 4096 rows: RowMap::make gives iters = 2 and the `row >= M` break is live (4224 = 33 * 128)

_CACHE: dict = {}


def cached(fn):
    def wrap(*key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            if any(isinstance(v, str) and v == "long" for v in key):  # one 17 MB-per-tensor case alive at a time
                for old in [o for o in _CACHE if "long" in o]:
                    del _CACHE[old]
            _CACHE[k] = fn(*key)
        return _CACHE[k]
    wrap.__name__ = fn.__name__
    return wrap


def vals(key: str, shape, dtype: int, scale: float = 1.0) -> torch.Tensor:
    """O(1) values as the kernel sees them after storage in `dtype` (f32 on the CPU)"""
    return (filler.tensor(key, tuple(shape)) * scale).to(TD[dtype]).float()


def bound(k: float, S: torch.Tensor, ref: torch.Tensor, dtype: int, extra: float = 0.0) -> torch.Tensor:
    b = k * U * S.double() + extra
    return b + BF16_U * ref.double().abs() if dtype == BF16 else b


def half_bound(k: float, S: torch.Tensor, ref: torch.Tensor, dtype: int, extra: float = 0.0) -> torch.Tensor:
    """what the CPU restatement has to stay within: half of the f32 part.  The bf16 store is not an estimate: round to
    nearest even ATTAINS 2^-8 * |value| (a value just above a power of two, half a unit away from both neighbours), so
    that term stays whole -- halving it would ask the restatement to round better than the format does."""
    b = 0.5 * (k * U * S.double() + extra)
    return b + BF16_U * ref.double().abs() if dtype == BF16 else b


def frac(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> float:
    """the worst |got - ref| as a fraction of its bound (<= 1 passes); NaN / inf in `got` give inf"""
    err = (got.double() - ref.double()).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    ok = bnd > 0
    worst = (err[ok] / bnd[ok]).max().item() if bool(ok.any()) else 0.0
    if bool((err[~ok] > 0).any()):
        return float("inf")
    return worst


# ---- RowMap::make (vt_rowmap.h) and pool_ct (vt_elementwise.hip), for the k that depend on the thread mapping ---------------
def rowmap(C: int, dtype: int, M: int, target_blocks: int = 4096):
    cpr = C // EPC[dtype]
    ct = min(cpr, THREADS)
    rt = THREADS // ct
    iters = min(max(-(-M // (rt * target_blocks)), 1), 64)
    return dict(CPR=cpr, CT=ct, RT=rt, iters=iters)


def pool_ct(C: int, dtype: int) -> int:
    cpr, ct = C // EPC[dtype], 1
    while ct < cpr and ct < 64:
        ct <<= 1
    return ct


# ---- 1. resampling ----------------------------------------------------------------------------------------------------
# (B, h, w) of the SMALL map; the big one is (B, 2h, 2w).  x2 modes read the small map, x0.5 modes the big one.
RESAMPLE_SMALL = [(2, 1, 1), (2, 1, 3), (1, 3, 1), (2, 2, 5), (1, 5, 4)]
RESAMPLE_LONG = (1, 33, 32)   # -> 66 x 64 = 4224 rows on the big map, with CPR = 257
RESAMPLE_GEOS = [s + (cpr,) for s in RESAMPLE_SMALL for cpr in CPRS] + [RESAMPLE_LONG + (257,)]   # (B, h, w, CPR)
# f32 roundings:
K_BILINEAR_FWD = 8   # 4 tap products (weights 0.25 / 0.75 / 0.5 are exact, the products round), 2 inner sums, 2 outer
                     # products, 1 outer sum = 9 without contraction, 7 with FMAs, + 1 for `other`; the issue sets 8
K_NEAREST_UP_BWD = 5  # start value + 4 gradients: 4 adds (+ 1 spare)
# A chain of 4 adds reaches 4 u S where the start value dominates and every partial sum sits just above a power of two, so
# no free-running f32 input keeps a faithful restatement within 2.5 u S over the 2 million elements of the long case (it
# reached 2.8 u S).  The bf16 cases have no such trouble: sums of five 8-bit values are exact in f32.  The f32 inputs of
# mode 0's backward get the same property: gradients and start values on a grid of 2^-16 -- 19 significant bits at
# |v| < 8, which five standard-normal terms stay far below -- whose sums of five (< 2^6, 22 bits) are exact in f32.  The
# restatement's error is then 0 by construction, and the kernel, which does the same four adds, is held to k = 5 all the same.
NEAREST_UP_BWD_GRID = 2.0 ** -16
K_BILINEAR_UP_BWD = 18  # at most 4 x 4 destination pixels, one FMA each (the weight products are exact) = 16, + 2 spare
K_BILINEAR_DOWN_BWD = 2  # one FMA with 0.25 (+ 1 spare)


def _interp(x_nhwc: torch.Tensor, mode: int) -> torch.Tensor:
    x = x_nhwc.permute(0, 3, 1, 2)
    sf = 0.5 if mode & 1 else 2
    y = F.interpolate(x, scale_factor=sf, mode="nearest") if mode < 2 else \
        F.interpolate(x, scale_factor=sf, mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1)


def _interp_bwd(g_nhwc: torch.Tensor, src_shape, mode: int) -> torch.Tensor:
    x = torch.zeros(src_shape, dtype=torch.float64, requires_grad=True)
    _interp(x, mode).backward(g_nhwc)
    return x.grad


def resample_shapes(mode: int, geo):
    """geo = (B, h, w, cpr) -> (source [B, Hs, Ws], destination [B, Hd, Wd])"""
    B, h, w = geo[:3]
    small, big = (B, h, w), (B, 2 * h, 2 * w)
    return (big, small) if mode & 1 else (small, big)


@cached
def resample_case(mode: int, geo, dtype: int, tag: str):
    src, dst = resample_shapes(mode, geo)
    C = geo[3] * EPC[dtype]
    key = f"hn.rs{mode}." + "x".join(map(str, geo)) + DNAME[dtype]
    x, o = vals(key + "x", src + (C,), dtype), vals(key + "o", dst + (C,), dtype)
    g, prior = vals(key + "g", dst + (C,), dtype), vals(key + "p", src + (C,), dtype)
    if mode == 0 and dtype == F32:
        g, prior = (torch.round(t / NEAREST_UP_BWD_GRID) * NEAREST_UP_BWD_GRID for t in (g, prior))
    y = _interp(x.double(), mode)
    Sy = _interp(x.double().abs(), mode)
    d = _interp_bwd(g.double(), src + (C,), mode)
    Sd = _interp_bwd(g.double().abs(), src + (C,), mode)
    return dict(x=x, o=o, g=g, prior=prior, y=y, Sy=Sy, yo=y + o.double(), Syo=Sy + o.double().abs(),
                d=(d, d + prior.double()), Sd=(Sd, Sd + prior.double().abs()))


def resample_bwd_k(mode: int) -> int:
    return {0: K_NEAREST_UP_BWD, 2: K_BILINEAR_UP_BWD, 3: K_BILINEAR_DOWN_BWD}[mode]


# ---- 2. softmax cross entropy ------------------------------------------------------------------------------------------
XENT_SHAPES = [(1, 5), (2, 255), (3, 256), (2, 257), (7, 1000), (4, 1)]
XENT_HEADERS = [(0, 0.7), (1, 0.3), (2, 1.0), (1, 0.0)]   # (mode, lam); mode 0 ignores lam
XENT_EPS = (0.0, 0.1)
XENT_LOSS_REL = 1e-5
# Gradient: |got - ref| <= r * (p + q) * |grad_scale|.  f32: the 256-thread sum of exponentials is a chain of at most
# ceil(N / 256) - 1 + 6 (wave butterfly) + 3 (four waves) <= 12 roundings of positive terms (<= 12 u = 7.2e-7 relative on
# the sum, the same on lse's exponent through logf), one logf (~1 ulp of lse <= 1.2e-7 * 30 absolute at worst, in practice
# 2 u * |lse|), the rounding of lse = mx + log(..) and of z - lse at |z - lse| <= 30 (each <= 30 u = 1.8e-6 absolute in
# the exponent, i.e. relative on p), expf (2 u): together under 4e-6 relative on p; (p - q) * grad_scale adds 2 u (p + q).
# bf16: r = 2^-8 is the store alone -- round to nearest even moves a value by up to u / (1 + u) = 2^-8 - 2^-16 of its size,
# |p - q| <= p + q -- and the 2^-16 = 1.5e-5 that is left covers the f32 part.
XENT_R = {F32: 1e-5, BF16: 2.0 ** -8}


def xent_logits(B: int, N: int, dtype: int) -> torch.Tensor:
    """|z| <= 12; row 0 is peaked when N > 1 (label logit +40, the rest -40); the last row has a tie at its maximum"""
    z = (filler.tensor(f"hn.xe{B}x{N}", (B, N)) * 3).clamp(-12, 12)
    y = xent_labels(B, N)
    if N > 1 and B > 1:
        z[0] = -40.0
        z[0, y[0]] = 40.0
    if N > 2:
        z[B - 1, N // 2] = z[B - 1, N - 1] = min(float(z[B - 1].max()) + 0.5, 12.0)
    return z.to(TD[dtype]).float()


def xent_labels(B: int, N: int) -> torch.Tensor:
    y = filler.labels(B, N, seed=4321 + N)
    if B > 1 and N > 1 and bool((y == y[0]).all()):
        y[1] = (y[0] + 1) % N   # a partner label that differs from the own one
    return y


def f32r(v: float) -> float:
    """a host double as the kernel receives it through a float argument"""
    return float(torch.tensor(v, dtype=torch.float32).item())


def xent_target(labels: torch.Tensor, N: int, mode: int, lam: float) -> torch.Tensor:
    """the soft target of oracle mix_batch (pinned to the reference by test_mix.py): the partner direction is its roll"""
    img = torch.zeros(labels.shape[0], 1, 1, 1, dtype=torch.float64)
    return R.mix_batch(img, labels, N, ("none", "mixup", "cutmix")[mode], f32r(lam))[1]


@cached
def xent_case(B: int, N: int, dtype: int, mode: int, lam: float, eps: float):
    z = xent_logits(B, N, dtype)
    y = xent_labels(B, N)
    zd = z.double().requires_grad_(True)
    tgt = xent_target(y, N, mode, lam)
    loss = F.cross_entropy(zd, tgt, label_smoothing=f32r(eps))
    loss.backward()
    p = torch.softmax(z.double(), 1)
    q = tgt * (1.0 - f32r(eps)) + f32r(eps) / N
    return dict(z=z, y=y, loss=loss.item(), dz_unit=zd.grad * B, p=p, q=q)   # dz_unit * grad_scale is the kernel's dlogits


# ---- 3. MixUp / CutMix on the way into NHWC ------------------------------------------------------------------------------
MIX_SHAPES = [(1, 3, 5, 7, 8), (3, 3, 6, 3, 4), (2, 1, 4, 4, 1), (4, 3, 9, 11, 8)]   # (B, C, H, W, Cpad)
# (every shape runs in both dtypes, which gives the bf16 / Cpad 8 -- the 16-byte store of vt_nchw_to_nhwc -- and the
#  f32 / Cpad 4 cases)
MIX_LAMS = (0.3, 1.0, 0.0)
# v = own * lam + partner * (1.f - lam) has four f32 roundings in the code: own * lam, 1 - lam, partner * (1 - lam), the sum.
# The issue's 3 counts the sum as fused into one of the products; the compiled kernel has no FMA there (a subtraction, a
# packed multiply for both products, an add).  With a = lam own, b = (1 - lam) partner the error is at most
# u (|a| + 2 |b| + |a + b|) <= 2 u |a| + 3 u |b|, and 2 u S where 1 - lam is exact (it is for 0.3f, 1 and 0): a faithful
# restatement stays within half of 4 u S by construction; under 3 it reached 1.54 u S on 32 elements.
K_MIXUP = 4


def mix_boxes(H: int, W: int):
    """(x1, y1, x2, y2): the whole image; empty; one pixel in a corner; touching only the right and bottom borders;
    interior and non-square"""
    return [(0, 0, W, H), (1, 0, 1, H), (W - 1, 0, W, 1), (W // 2, H // 2, W, H), (1, 1, max(W - 1, 2), 2)]


def mix_images(shape) -> torch.Tensor:
    B, C, H, W, _ = shape
    return filler.tensor("hn.mix" + "x".join(map(str, shape)), (B, C, H, W))


def mix_ref(x: torch.Tensor, mode: int, lam: float, box, Cpad: int):
    """(float64 NHWC reference padded to Cpad, S)"""
    B, C, H, W = x.shape
    labels = torch.zeros(B, dtype=torch.int64)
    name = ("none", "mixup", "cutmix")[mode]
    img = R.mix_batch(x.double(), labels, 2, name, f32r(lam), box)[0]
    S = R.mix_batch(x.double().abs(), labels, 2, name, f32r(lam), box)[0] if mode == 1 else img.abs()
    pad = lambda t: F.pad(t.permute(0, 2, 3, 1), (0, Cpad - C))
    return pad(img), pad(S)


# ---- 4. eval-mode BatchNorm coefficients ---------------------------------------------------------------------------------
BN_CS = (1, 8, 255, 256, 257, 600)
BN_EPS = 1e-5
K_BN_SCALE = 4   # rv + eps, sqrtf, 1 / x, g * istd (invstd: the first three)
# What the half needs.  invstd: the rounding of x = rv + eps passes through the square root and counts half; y = sqrtf(x) and
# z = 1 / y (both correctly rounded in the compiled kernel) err by u / m_y and u / m_z of their size, m their significands in
# [1, 2), and m_z = 2 / m_y, so the two give u (1 / m_y + m_y / 2) <= 1.5 u: together at most 2 u, half of 4, by construction.
# scale with a free-running gamma adds a whole rounding, 3 u in the worst case, and over 255 and more channels a faithful
# restatement passes 2 u with most draws (1.02 .. 1.18 of the half with seven of eight).  So gamma is drawn as it would be,
# then moved to the nearest power of two (2^-4 .. 2^2, either sign, differing from channel to channel): g * istd is exact and
# scale inherits invstd's 2 u.  The product's own rounding is then not exercised here; the kernel stays held to k = 4.
# shift = b - rm * scale on S = |b| + |rm * scale|: `scale` brings its own 4 roundings into the product, the product rounds,
# the difference rounds: 6 (5 where the compiler contracts the last two into an FMA).  The issue's 4 left out the last two;
# the restatement reached 2.4 u S on C = 600, more than half of 4.
K_BN_SHIFT = 6


def bn_inputs(C: int, tag: str = ""):
    key = f"hn.bn{C}{tag}"
    g, b, rm = (filler.tensor(key + n, (C,)) for n in "gbm")
    g = torch.sign(g) * torch.exp2(torch.round(torch.log2(g.abs())).clamp(-4, 2))   # see K_BN_SCALE
    rv =filler.tensor(key + "v", (C,)).abs() + 0.05
    rv[0] = 0.0
    if C > 1:
        rv[C - 1] = 1e-12
    return g, b, rm, rv


def bn_ref(g, b, rm, rv, eps: float = BN_EPS):
    """float64 (scale, shift, invstd); g / b None: 1 / 0"""
    istd = 1.0 / torch.sqrt(rv.double() + f32r(eps))
    gd = g.double() if g is not None else torch.ones_like(istd)
    bd = b.double() if b is not None else torch.zeros_like(istd)
    scale = gd * istd
    return scale, bd - rm.double() * scale, istd, bd.abs() + (rm.double() * scale).abs()


# ---- 5. pooling, ESE gate, column sums ---------------------------------------------------------------------------------
POOL_SHAPES = [(2, 1, 1), (3, 7, 3), (2, 20, 65), (1, 300, 130)]   # (B, HW, chunks per row)
K_POOL_TAIL = 3   # behind the fixed-point sum: its conversion to f32, 1 / HW, the product


def pool_k(C: int, dtype: int, HW: int) -> int:
    """a row lane adds its ceil(HW / RT) rows in f32 before the fixed-point sum: that many - 1 roundings, + K_POOL_TAIL.
    (The issue's k = 3 is this count where HW <= RT; at HW = 300 with RT = 4 it left out a chain of 74 adds, which
    its own k for the ESE gate's ds, ceil(HW / RT) + 3, has.)"""
    rt = THREADS // pool_ct(C, dtype)
    return -(-HW // rt) - 1 + K_POOL_TAIL


# (the issue sets no k for the next two; like its own counts they carry two roundings to spare, since a chain of n roundings
#  reaches n u S in the worst case and a bound of exactly n leaves a faithful restatement no half to stay within)
K_POOL_BWD = 5    # 1 / HW, g * inv, + start value: 3, + 2 spare
K_ESE = 7         # gate: 1/6 constant, s * (1/6), + 0.5; x * gate; + residual (or + start value in dx): 5, + 2 spare


def pool_quantum(C: int, dtype: int, HW: int) -> float:
    """every one of the RT row lanes rounds its partial sum to the fixed-point grid: half a quantum each"""
    lanes = min(THREADS // pool_ct(C, dtype), HW)
    return lanes * 0.5 * LDS_FIX_QUANTUM


def ese_s(B: int, C: int, dtype: int, key: str) -> torch.Tensor:
    """gate inputs over (-4.5, 4.5), with s exactly +3 and -3 (the ends of the derivative's open interval) planted"""
    s = vals(key, (B, C), dtype, 1.5)
    flat = s.view(-1)
    flat[0] = 3.0
    if flat.numel() > 1:
        flat[1] = -3.0
    if flat.numel() > 3:
        flat[2], flat[3] = 2.984375, -2.984375   # just inside, exact in bf16
    return s


@cached
def pool_case(shape, dtype: int, tag: str):
    B, HW, chunks = shape
    C = chunks * EPC[dtype]
    key = "hn.pool" + "x".join(map(str, shape)) + DNAME[dtype]
    x, r, dy, prior = (vals(key + n, (B, HW, C), dtype) for n in ("x", "r", "dy", "p"))
    s = ese_s(B, C, dtype, key + "s")
    g = vals(key + "g", (B, C), dtype)
    xd, sd = x.double().requires_grad_(True), s.double().requires_grad_(True)
    y = xd * F.hardsigmoid(sd)[:, None, :] + r.double()
    y.backward(dy.double())
    gate_abs = s.double().abs() / 6 + 0.5
    return dict(x=x, r=r, dy=dy, prior=prior, s=s, g=g, C=C,
                mean=x.double().mean(1), Smean=x.double().abs().mean(1),
                y=y.detach(), Sy=x.double().abs() * gate_abs[:, None, :] + r.double().abs(),
                dx=(xd.grad, xd.grad + prior.double()),
                Sdx=(dy.double().abs() * gate_abs[:, None, :], dy.double().abs() * gate_abs[:, None, :] + prior.double().abs()),
                ds=sd.grad, Sds=(dy.double() * x.double()).abs().sum(1) / 6,
                pb=(g.double()[:, None, :].expand(B, HW, C) / HW, g.double()[:, None, :] / HW + prior.double()),
                Spb=(g.double().abs()[:, None, :].expand(B, HW, C) / HW, g.double().abs()[:, None, :] / HW + prior.double().abs()))


def ese_ds_k(C: int, dtype: int, HW: int) -> int:
    rt = THREADS // pool_ct(C, dtype)
    return -(-HW // rt) + 3


COLSUM_MS = (1, 37, 5000)
COLSUM_CPRS = (3, 257)


def colsum_k(C: int, dtype: int, M: int) -> int:
    """a thread adds its `iters` rows in f32 (iters - 1 roundings), then every thread that owns a row of the column adds
    its partial sum to the output with a float atomic: one rounding each, in whatever order -- as many as there are
    (block, row lane) pairs with a row; + 2 spare.  The issue's "rows per thread + 2" is this count with ONE atomic: at
    M = 37 with CPR = 257 -- RT = 1, one row per block -- the 37 atomics are the whole sum, and the restatement reached
    2 u S of the 3 u S that would allow."""
    rm = rowmap(C, dtype, M, 256)
    per_block = rm["RT"] * rm["iters"]
    lanes = (M // per_block) * rm["RT"] + min(rm["RT"], M % per_block)
    return rm["iters"] - 1 + lanes + 2


@cached
def colsum_case(M: int, cpr: int, dtype: int):
    C = cpr * EPC[dtype]
    a = vals(f"hn.cs{M}x{cpr}{DNAME[dtype]}", (M, C), dtype)
    out0 = filler.tensor(f"hn.cs0{M}x{cpr}", (C,))
    return dict(a=a, out0=out0, ref=a.double().sum(0) + out0.double(), S=a.double().abs().sum(0) + out0.double().abs())


COPY_SHAPES = [(1, 1), (6, 10), (3, 70001)]
