"""The input transform restated in float64 (numpy), the erase generator restated in numpy, and seeded uint8 noise images.

The definition (include/vt_amd.h, vt_augment_batch): crop -> separable triangle resize to a virtual (OH, OW) image ->
the (S_h, S_w) window at (oy, ox) -> flip -> 1/255 -> (v - mean) / std -> erase.  Images are NOISE, not smooth: a tap that
is off by one pixel moves an output by a large fraction of the range."""
from __future__ import annotations

import numpy as np
import torch

FIELDS = 16
MASK = np.uint64(0xFFFFFFFF)

# source sizes (H, W) of the ragged batch of the GPU tests; the last one is the large-downscale image
SIZES = [(37, 53), (64, 48), (9, 7), (131, 97), (20, 20), (300, 400)]
# seeds of the statistics test of the random erase (test_augment_cpu checks that the restatement holds the bounds for them)
STAT_SEEDS = (11, 12345, 2026)


def make_images(sizes=SIZES, seed: int = 0) -> "list[torch.Tensor]":
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)) for H, W in sizes]


def row(top, left, h, w, OH, OW, oy=0, ox=0, flip=0, erase=(0, 0, 0, 0), mode=0, seed=0, value_bits=0) -> "list[int]":
    return [top, left, h, w, OH, OW, oy, ox, flip, *erase, mode, seed, value_bits]


def params_tensor(rows) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), FIELDS)


def f32_bits(v: float) -> int:
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


# ---- the filter ------------------------------------------------------------------------------------------------------
def weight_matrix(n: int, out: int, antialias: bool = True) -> np.ndarray:
    """float64 [out, n]: s = n / out, support = max(s, 1) (antialias) or 1, c = s (i + 0.5); taps j in
    [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)), weight max(0, 1 - |(j - c + 0.5) / support|) over the
    sum of the weights."""
    s = n / out
    support = max(s, 1.0) if antialias else 1.0
    Wm = np.zeros((out, n), dtype=np.float64)
    for i in range(out):
        c = s * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)
        j = np.arange(lo, hi, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) / support))
        Wm[i, lo:hi] = w / w.sum()
    return Wm


def _separable(wy: np.ndarray, crop: np.ndarray, wx: np.ndarray) -> np.ndarray:
    """[Y, h] x [h, w, 3] x [X, w] -> [3, Y, X] (rows first, then columns: two matrix products)"""
    rows = np.tensordot(wy, crop, axes=(1, 0))                       # [Y, w, 3]
    return np.tensordot(rows, wx, axes=(1, 1)).transpose(1, 0, 2)    # [Y, 3, X] -> [3, Y, X]


def resample(crop: np.ndarray, OH: int, OW: int, antialias: bool = True) -> np.ndarray:
    """crop float64 [h, w, 3] -> the whole virtual output, float64 [3, OH, OW]"""
    h, w, _ = crop.shape
    return _separable(weight_matrix(h, OH, antialias), crop, weight_matrix(w, OW, antialias))


# ---- the erase generator ---------------------------------------------------------------------------------------------
def mix32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) & MASK
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & MASK
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & MASK
    return x ^ (x >> np.uint64(16))


def erase_normal(seed: int, b: int, Sh: int, Sw: int) -> np.ndarray:
    """float64 [3, Sh, Sw]: k = mix(seed + 0x9e3779b9), then k = mix(k + v) for v = b, c, y, x; h1 = mix(k ^ 0x68bc21eb),
    h2 = mix(k ^ 0x02e5be93); u1 = ((h1 >> 8) + 1) / 2^24, u2 = (h2 >> 8) / 2^24; z = sqrt(-2 ln u1) cos(t) with t the
    float32 product 6.2831855f * u2 (the one f32 rounding the definition fixes)."""
    c = np.arange(3, dtype=np.uint64).reshape(3, 1, 1)
    y = np.arange(Sh, dtype=np.uint64).reshape(1, Sh, 1)
    x = np.arange(Sw, dtype=np.uint64).reshape(1, 1, Sw)
    k = mix32(np.uint64((seed & 0xFFFFFFFF) + 0x9E3779B9))
    k = mix32(k + np.uint64(b & 0xFFFFFFFF))
    k = mix32(k + c)
    k = mix32(k + y)
    k = mix32(k + x)
    h1, h2 = mix32(k ^ np.uint64(0x68BC21EB)), mix32(k ^ np.uint64(0x02E5BE93))
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0**-24
    u2 = (h2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
    t = (np.float32(6.2831855) * u2).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(t)


# ---- the whole transform ---------------------------------------------------------------------------------------------
def reference_image(img: torch.Tensor, prm, b: int, Sh: int, Sw: int, antialias: bool = True, mean_std=None) -> np.ndarray:
    """one image (uint8 [H, W, 3]) and its params row -> float64 [3, Sh, Sw]"""
    top, left, h, w, OH, OW, oy, ox, flip, ei, ej, eh, ew, mode, seed, bits = [int(v) for v in prm]
    crop = img.numpy()[top : top + h, left : left + w].astype(np.float64)
    wy = weight_matrix(h, OH, antialias)[oy : oy + Sh]
    wx = weight_matrix(w, OW, antialias)[ox : ox + Sw]
    v = _separable(wy, crop, wx)
    if flip:
        v = v[:, :, ::-1]
    v = v / 255.0
    if mean_std is not None:
        m = np.asarray(mean_std, dtype=np.float32).astype(np.float64)  # (the kernel is handed f32 values)
        v = (v - m[:3].reshape(3, 1, 1)) / m[3:].reshape(3, 1, 1)
    v = np.ascontiguousarray(v)
    if mode != 0 and eh > 0 and ew > 0:
        if mode == 1:
            v[:, ei : ei + eh, ej : ej + ew] = float(np.array([bits], dtype=np.int32).view(np.float32)[0])
        else:
            v[:, ei : ei + eh, ej : ej + ew] = erase_normal(seed, b, Sh, Sw)[:, ei : ei + eh, ej : ej + ew]
    return v


def reference_batch(images, params: torch.Tensor, Sh: int, Sw: int, antialias: bool = True, mean_std=None) -> torch.Tensor:
    rows = params.tolist()
    return torch.from_numpy(np.stack([reference_image(im, r, b, Sh, Sw, antialias, mean_std)
                                      for b, (im, r) in enumerate(zip(images, rows))]))


def errors(got: torch.Tensor, ref: torch.Tensor) -> "tuple[float, float]":
    """(relative L2 error, largest element error over the largest magnitude of the reference)"""
    g, r = got.double(), ref.double()
    return ((g - r).norm() / r.norm().clamp_min(1e-300)).item(), ((g - r).abs().max() / r.abs().max().clamp_min(1e-300)).item()
