"""Helpers of the TrivialAugmentWide tests: the tiny 8-bit images, every (op, signed magnitude) setting, and the dispatcher
that applies a table row to an image with PIL, the way torchvision's TrivialAugmentWide dispatches onto PIL images.

Only pil_apply imports PIL, and only when it is called: the GPU tests use the images and the settings without it."""
from __future__ import annotations

import numpy as np
import torch

from vision_toolbox import data as D


def make_images() -> "dict[str, torch.Tensor]":
    """uint8 [H, W, 3] levels by name.  noise37x41: odd, non-square (the general rotate path; 1517 pixels, so Equalize's step
    is 5).  noise24: square (PIL's 90-degree shortcuts).  constant: the identity branches of AutoContrast and Equalize.
    twolevel: red holds two levels, green is a ramp, blue is noise in a narrow range.  thin3x7 and line1x5: no interior for
    Sharpness, the affine clamps dominate.  noise176: red and blue in narrow ranges, so histogram bins hold more than 255."""
    rng = np.random.default_rng(2026)

    def noise(H, W, lo=0, hi=256):
        return rng.integers(lo, hi, size=(H, W, 3), dtype=np.uint8)

    two = noise(20, 32, 60, 90)
    two[..., 0] = np.where(rng.integers(0, 2, size=(20, 32)) == 1, 200, 17)
    two[..., 1] = np.arange(20 * 32, dtype=np.int64).reshape(20, 32) * 255 // (20 * 32 - 1)
    const = np.empty((12, 10, 3), dtype=np.uint8)
    const[...] = (7, 130, 255)
    big = noise(176, 176)
    big[..., 0] = rng.integers(30, 110, size=(176, 176), dtype=np.uint8)   # 80 levels: 387 pixels a bin
    big[..., 2] = rng.integers(100, 140, size=(176, 176), dtype=np.uint8)  # 40 levels: 774 pixels a bin
    images = {"noise37x41": noise(37, 41), "noise24": noise(24, 24), "constant": const, "twolevel": two,
              "thin3x7": noise(3, 7), "line1x5": noise(1, 5), "noise176": big}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in images.items()}


def settings() -> "list[tuple[int, float]]":
    """every (op, signed magnitude): 31 bins x both signs for the signed ops, 31 bins for Posterize and Solarize, one entry
    for the ops without a magnitude"""
    out = []
    for op in range(len(D.TA_OPS)):
        mags = D.ta_magnitudes(op)
        if mags is None:
            out.append((op, 0.0))
            continue
        for m in mags:
            out.append((op, m))
            if op in D.TA_SIGNED:
                out.append((op, -m))
    return out


def table(rows_settings, H: int, W: int) -> torch.Tensor:
    """float64 [n, 8]: the table rows of the settings for H x W levels"""
    return torch.tensor([D.ta_row(op, mag, (H, W)) for op, mag in rows_settings], dtype=torch.float64).reshape(-1, 8)


def pil_apply(img: torch.Tensor, op: int, mag: float, row) -> torch.Tensor:
    """uint8 [H, W, 3] -> uint8 [H, W, 3] through PIL.  Shears and translations take the table row's own matrix; Rotate goes
    through Image.rotate with the angle, so the row's matrix restatement is itself compared with PIL."""
    from PIL import Image, ImageEnhance, ImageOps

    pil = Image.fromarray(img.numpy(), "RGB")
    if op == D.TA_IDENTITY:
        res = pil
    elif op in (D.TA_SHEAR_X, D.TA_SHEAR_Y, D.TA_TRANSLATE_X, D.TA_TRANSLATE_Y):
        res = pil.transform(pil.size, Image.AFFINE, [float(v) for v in row[1:7]], Image.BILINEAR)
    elif op == D.TA_ROTATE:
        res = pil.rotate(mag, Image.BILINEAR)
    elif op == D.TA_BRIGHTNESS:
        res = ImageEnhance.Brightness(pil).enhance(1.0 + mag)
    elif op == D.TA_COLOR:
        res = ImageEnhance.Color(pil).enhance(1.0 + mag)
    elif op == D.TA_CONTRAST:
        res = ImageEnhance.Contrast(pil).enhance(1.0 + mag)
    elif op == D.TA_SHARPNESS:
        res = ImageEnhance.Sharpness(pil).enhance(1.0 + mag)
    elif op == D.TA_POSTERIZE:
        res = ImageOps.posterize(pil, int(mag))
    elif op == D.TA_SOLARIZE:
        res = ImageOps.solarize(pil, mag)
    elif op == D.TA_AUTOCONTRAST:
        res = ImageOps.autocontrast(pil)
    elif op == D.TA_EQUALIZE:
        res = ImageOps.equalize(pil)
    else:
        raise ValueError(op)
    return torch.from_numpy(np.array(res.convert("RGB"), dtype=np.uint8))


def pack(named_rows, images) -> "list[tuple[tuple[int, int], torch.Tensor, torch.Tensor]]":
    """[(image name, table row), ...] -> one (size, uint8 [B, H, W, 3], float64 [B, 8]) batch per image size, rows in order"""
    groups = {}
    for name, row in named_rows:
        img = images[name]
        groups.setdefault((int(img.shape[0]), int(img.shape[1])), []).append((img, row))
    return [(size, torch.stack([i for i, _ in g]), torch.tensor([list(r) for _, r in g], dtype=torch.float64).reshape(-1, 8))
            for size, g in groups.items()]
