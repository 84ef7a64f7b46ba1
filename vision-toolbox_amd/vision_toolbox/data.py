"""The input transform of the reference's data pipeline (data.py:43-61) on the device.

The reference builds a batch on the host with PIL: RandomResizedCrop -> RandomHorizontalFlip -> ToTensor ->
RandomErasing for training, Resize(232) -> CenterCrop(224) -> ToTensor for validation.  Here the decoded uint8 HWC
images of a batch are packed into one buffer (RaggedBatch), the random decisions become one small int32 table
(sample_train_params / eval_params) and ONE HIP launch (vt_augment_batch, csrc/vt_augment.hip) turns both into the
float32 [B, 3, S_h, S_w] batch that TrainStep.images holds:

    aug = GPUBatchTransform(176)
    batch = RaggedBatch.from_images(decoded).to("cuda")
    aug(batch, sample_train_params(batch.sizes, 176), out=ts.images)
    ts.step()

The filter is torch's F.interpolate(mode="bilinear", antialias=True, align_corners=False) of the float crop, with no
rounding to 8 bits in between (PIL rounds after each pass and differs by at most one 8-bit level).  MixUp / CutMix stay
in the program's input op (trainer.py).  JPEG decoding is the last part of this file (decode_jpeg_batch: compressed bytes ->
RaggedBatch on the device).  Not here: WebDataset / ImageFolder loaders.

TrivialAugmentWide (the reference's third stage) is the optional table `ta` (sample_trivial_augment): with it the filtered
value is rounded half up to an 8-bit level (vt_augment_batch_u8), one of the 14 ops (TA_OPS) is applied to the levels of
each image exactly as PIL applies it to an 8-bit image, and a second call (vt_trivial_augment, csrc/vt_trivial_augment.hip)
writes float32(level) * (1 / 255), mean / std and the erase:

    aug(batch, sample_train_params(batch.sizes, 176), out=ts.images, ta=sample_trivial_augment(batch.sizes, 176))

Without a table nothing changes: the one launch above, the same bits.

torchvision is not installed where this was written: the sampling rules of RandomResizedCrop, RandomHorizontalFlip,
RandomErasing, Resize and CenterCrop are restated from its documentation and from memory, and the tests check their
properties (boxes inside the image, area and ratio ranges, the fallback, frequencies), not a torchvision random stream.

CUDA tensors run the kernel; there is no fallback on the GPU.  CPU tensors run a plain-torch float32 path of the same
definition (weight matrices and two matmuls per image), which is what the GPU tests compare the module against; the
TrivialAugmentWide stage alone is trivial_augment_levels, integer / float64 torch on a uint8 [B, S_h, S_w, 3] batch, which
the CPU tests compare with PIL level for level.
"""
from __future__ import annotations

import ctypes as C
import math
import sys
from typing import Optional, Sequence, Union

import torch

from . import _native as N

FIELDS = ("top", "left", "h", "w", "OH", "OW", "oy", "ox", "flip", "ei", "ej", "eh", "ew", "erase_mode", "seed", "value")
(P_TOP, P_LEFT, P_H, P_W, P_OH, P_OW, P_OY, P_OX, P_FLIP, P_EI, P_EJ, P_EH, P_EW, P_MODE, P_SEED, P_VALUE) = range(16)
ERASE_NONE, ERASE_CONSTANT, ERASE_RANDOM = 0, 1, 2
_DRAWS = 48  # uniforms per image: 20 + 2 (crop), 1 (flip), 1 + 20 + 2 (erase), 1 (seed), 1 spare


def _pair(v) -> "tuple[int, int]":
    if isinstance(v, int):
        return v, v
    a, b = v
    return int(a), int(b)


def f32_bits(v: float) -> int:
    """the int32 that holds the bits of float32(v) (the `value` field of a params row)"""
    return C.c_int32.from_buffer_copy(C.c_float(v)).value


class RaggedBatch:
    """Decoded images of different sizes in one uint8 buffer: `raw` (all images packed HWC), `table` int64 [B, 3] =
    (byte offset, H, W) and `sizes` = [(H, W), ...] on the host."""

    status = None  # int32 [B] beside a batch that decode_jpeg_batch made (0 = a clean image), otherwise None

    def __init__(self, raw: torch.Tensor, table: torch.Tensor, sizes: "list[tuple[int, int]]"):
        self.raw, self.table, self.sizes = raw, table, list(sizes)

    @classmethod
    def from_images(cls, images: Sequence[torch.Tensor]) -> "RaggedBatch":
        """pack uint8 HWC tensors (any strides) into one buffer, pinned where there is a GPU to copy it to"""
        if len(images) == 0:
            raise ValueError("RaggedBatch.from_images: no images")
        sizes, offsets, total = [], [], 0
        for i, im in enumerate(images):
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
                raise ValueError(f"image {i}: expected a uint8 tensor, got {getattr(im, 'dtype', type(im).__name__)}")
            if im.dim() != 3 or im.shape[2] != 3:
                raise ValueError(f"image {i}: expected HWC with 3 channels, got shape {tuple(im.shape)}")
            H, W = int(im.shape[0]), int(im.shape[1])
            if H < 1 or W < 1:
                raise ValueError(f"image {i}: empty image, shape {tuple(im.shape)}")
            sizes.append((H, W))
            offsets.append(total)
            total += H * W * 3
        pin = torch.cuda.is_available()
        raw = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
        for im, off, (H, W) in zip(images, offsets, sizes):
            raw[off : off + H * W * 3].view(H, W, 3).copy_(im)
        table = torch.tensor([[o, H, W] for o, (H, W) in zip(offsets, sizes)], dtype=torch.int64)
        if pin:
            table = table.pin_memory()
        return cls(raw, table, sizes)

    def __len__(self) -> int:
        return len(self.sizes)

    def to(self, device, non_blocking: bool = True) -> "RaggedBatch":
        """non_blocking applies to copies TO a GPU only (from the pinned buffer, ordered on the current stream); a copy to
        the host is always complete when this returns, since the host reads it without a stream to order it"""
        nb = non_blocking and torch.device(device).type == "cuda"
        out = RaggedBatch(self.raw.to(device, non_blocking=nb), self.table.to(device, non_blocking=nb), self.sizes)
        if self.status is not None:
            out.status = self.status.to(device, non_blocking=nb)
        return out


# ---- the sampling rules --------------------------------------------------------------------------------------------
def _randint(u: float, n: int) -> int:
    """uniform integer in [0, n) from a uniform u in [0, 1)"""
    return min(int(u * n), n - 1)


def _sample_crop(H: int, W: int, scale, ratio, u) -> "tuple[int, int, int, int, bool]":
    """RandomResizedCrop: up to ten draws of (area, log-uniform ratio), the first that fits at a uniform position;
    otherwise the central crop with the ratio clamped into its range.  u: 22 uniforms."""
    area = H * W
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    for k in range(10):
        target = area * (scale[0] + (scale[1] - scale[0]) * u[2 * k])
        aspect = math.exp(lr0 + (lr1 - lr0) * u[2 * k + 1])
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return _randint(u[20], H - h + 1), _randint(u[21], W - w + 1), h, w, False
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    h, w = max(1, min(h, H)), max(1, min(w, W))
    return (H - h) // 2, (W - w) // 2, h, w, True


def _sample_erase(Sh: int, Sw: int, p: float, scale, ratio, u) -> "tuple[int, int, int, int]":
    """RandomErasing: with probability p, up to ten draws of (area, log-uniform ratio); the box must be strictly smaller
    than the output on both sides; a uniform position.  No draw fits: no erase (eh = 0).  u: 23 uniforms."""
    if not u[0] < p:
        return 0, 0, 0, 0
    area = Sh * Sw
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    for k in range(10):
        target = area * (scale[0] + (scale[1] - scale[0]) * u[1 + 2 * k])
        aspect = math.exp(lr0 + (lr1 - lr0) * u[2 + 2 * k])
        h = int(round(math.sqrt(target * aspect)))
        w = int(round(math.sqrt(target / aspect)))
        if 0 < h < Sh and 0 < w < Sw:
            return _randint(u[21], Sh - h + 1), _randint(u[22], Sw - w + 1), h, w
    return 0, 0, 0, 0


def sample_train_params(sizes, crop_size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p: float = 0.5, erase_p: float = 0.1,
                        erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3), erase_value: Union[str, float] = "random",
                        generator: Optional[torch.Generator] = None, return_fallback: bool = False):
    """The training table, int32 [B, 16] (FIELDS), for images of `sizes` = [(H, W), ...]: RandomResizedCrop(crop_size,
    scale, ratio), RandomHorizontalFlip(flip_p), RandomErasing(erase_p, erase_scale, erase_ratio, erase_value).  All draws
    come from ONE torch.rand(B, 48, float64) of the CPU generator, so a generator seed fixes the table.
    return_fallback: also return a bool [B], True where RandomResizedCrop took its central-crop fallback."""
    Sh, Sw = _pair(crop_size)
    if isinstance(erase_value, str):
        if erase_value != "random":
            raise ValueError(f"erase_value={erase_value!r}: 'random' or a number")
        mode, bits = ERASE_RANDOM, 0
    else:
        mode, bits = ERASE_CONSTANT, f32_bits(float(erase_value))
    B = len(sizes)
    U = torch.rand(B, _DRAWS, dtype=torch.float64, generator=generator).tolist()
    rows, fell = [], []
    for (H, W), u in zip(sizes, U):
        top, left, h, w, fb = _sample_crop(int(H), int(W), scale, ratio, u[:22])
        flip = 1 if u[22] < flip_p else 0
        ei, ej, eh, ew = _sample_erase(Sh, Sw, erase_p, erase_scale, erase_ratio, u[23:46])
        seed = int(u[46] * 2147483648.0)
        rows.append([top, left, h, w, Sh, Sw, 0, 0, flip, ei, ej, eh, ew, mode if eh > 0 else ERASE_NONE, seed,
                     bits if eh > 0 else 0])
        fell.append(fb)
    params = torch.tensor(rows, dtype=torch.int32).reshape(B, 16)
    return (params, torch.tensor(fell, dtype=torch.bool)) if return_fallback else params


def eval_params(sizes, resize_size: int = 232, crop_size=224) -> torch.Tensor:
    """The validation table, int32 [B, 16]: Resize(resize_size) of the whole image (shorter side to resize_size, the other
    to int(resize_size * long / short)) and the CenterCrop(crop_size) window of it; no flip, no erase."""
    Sh, Sw = _pair(crop_size)
    rows = []
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        if H <= W:
            OH, OW = resize_size, int(resize_size * W / H)
        else:
            OH, OW = int(resize_size * H / W), resize_size
        if OH < Sh or OW < Sw:
            raise ValueError(f"image {i}: the resized image ({OH}, {OW}) is smaller than the crop ({Sh}, {Sw})")
        oy, ox = int(round((OH - Sh) / 2.0)), int(round((OW - Sw) / 2.0))
        rows.append([0, 0, H, W, OH, OW, oy, ox, 0, 0, 0, 0, 0, ERASE_NONE, 0, 0])
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 16)


def validate_params(params: torch.Tensor, sizes, out_size) -> None:
    """ValueError naming the image and the field for a host table the kernel would have to clamp."""
    Sh, Sw = _pair(out_size)
    if params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != 16 or params.shape[0] != len(sizes):
        raise ValueError(f"params: expected int32 [{len(sizes)}, 16], got {params.dtype} {tuple(params.shape)}")
    for b, ((H, W), row) in enumerate(zip(sizes, params.tolist())):
        top, left, h, w, OH, OW, oy, ox, _, ei, ej, eh, ew, mode = row[:14]

        def bad(field, why):
            raise ValueError(f"params[{b}].{field} = {row[FIELDS.index(field)]}: {why} (image {H} x {W}, output {Sh} x {Sw})")

        if h < 1:
            bad("h", "the crop box needs h >= 1")
        if w < 1:
            bad("w", "the crop box needs w >= 1")
        if top < 0 or top + h > H:
            bad("top", f"rows [top, top + h = {top + h}) leave the image")
        if left < 0 or left + w > W:
            bad("left", f"columns [left, left + w = {left + w}) leave the image")
        if OH < 1:
            bad("OH", "the virtual output needs OH >= 1")
        if OW < 1:
            bad("OW", "the virtual output needs OW >= 1")
        if oy < 0 or oy + Sh > OH:
            bad("oy", f"the window rows [oy, oy + {Sh}) leave the virtual output of {OH} rows")
        if ox < 0 or ox + Sw > OW:
            bad("ox", f"the window columns [ox, ox + {Sw}) leave the virtual output of {OW} columns")
        if mode not in (ERASE_NONE, ERASE_CONSTANT, ERASE_RANDOM):
            bad("erase_mode", "0 (none), 1 (constant) or 2 (random)")
        if mode != ERASE_NONE and eh != 0:
            if eh < 0:
                bad("eh", "the erase box needs eh >= 0")
            if ew < 0:
                bad("ew", "the erase box needs ew >= 0")
            if ei < 0 or ei + eh > Sh:
                bad("ei", f"the erase rows [ei, ei + eh = {ei + eh}) leave the output")
            if ej < 0 or ej + ew > Sw:
                bad("ej", f"the erase columns [ej, ej + ew = {ej + ew}) leave the output")


# ---- TrivialAugmentWide: the table -----------------------------------------------------------------------------------
TA_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
          "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
(TA_IDENTITY, TA_SHEAR_X, TA_SHEAR_Y, TA_TRANSLATE_X, TA_TRANSLATE_Y, TA_ROTATE, TA_BRIGHTNESS, TA_COLOR, TA_CONTRAST,
 TA_SHARPNESS, TA_POSTERIZE, TA_SOLARIZE, TA_AUTOCONTRAST, TA_EQUALIZE) = range(14)
TA_FIELDS = ("op", "m0", "m1", "m2", "m3", "m4", "m5", "arg")
TA_BINS = 31
TA_SIGNED = frozenset(range(TA_SHEAR_X, TA_SHARPNESS + 1))
_TA_AFFINE = frozenset(range(TA_SHEAR_X, TA_ROTATE + 1))
_TA_IDENTITY_ROW = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]


def ta_magnitudes(op: int) -> "Optional[list[float]]":
    """the 31 magnitudes of an op (torchvision's TrivialAugmentWide._augmentation_space with 31 bins, float32 linspace
    values as Python floats), None for the ops that take none"""
    if op in (TA_SHEAR_X, TA_SHEAR_Y) or TA_BRIGHTNESS <= op <= TA_SHARPNESS:
        return torch.linspace(0.0, 0.99, TA_BINS).tolist()
    if op in (TA_TRANSLATE_X, TA_TRANSLATE_Y):
        return torch.linspace(0.0, 32.0, TA_BINS).tolist()
    if op == TA_ROTATE:
        return torch.linspace(0.0, 135.0, TA_BINS).tolist()
    if op == TA_POSTERIZE:
        return [float(v) for v in (8 - (torch.arange(TA_BINS) / ((TA_BINS - 1) / 6)).round().int()).tolist()]
    if op == TA_SOLARIZE:
        return torch.linspace(255.0, 0.0, TA_BINS).tolist()
    return None


def inverse_affine_matrix(center, angle: float, translate, scale: float, shear) -> "list[float]":
    """torchvision's _get_inverse_affine_matrix: output pixel -> input pixel, rotation and shears in degrees"""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle: float, H: int, W: int) -> "list[float]":
    """the matrix of PIL's Image.rotate(angle) about the image centre (W / 2, H / 2), no expansion"""
    t = -math.radians(angle % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def ta_row(op: int, magnitude: float, out_size) -> "list[float]":
    """one row (op, m0..m5, arg) of the table for a SIGNED magnitude (ignored by the ops that take none) on S_h x S_w levels"""
    Sh, Sw = _pair(out_size)
    m, arg = _TA_IDENTITY_ROW[1:7], 0.0
    if op == TA_SHEAR_X:
        m = inverse_affine_matrix((0.0, 0.0), 0.0, (0, 0), 1.0, (math.degrees(math.atan(magnitude)), 0.0))
    elif op == TA_SHEAR_Y:
        m = inverse_affine_matrix((0.0, 0.0), 0.0, (0, 0), 1.0, (0.0, math.degrees(math.atan(magnitude))))
    elif op == TA_TRANSLATE_X:
        m = inverse_affine_matrix((Sw * 0.5, Sh * 0.5), 0.0, (int(magnitude), 0), 1.0, (0.0, 0.0))
    elif op == TA_TRANSLATE_Y:
        m = inverse_affine_matrix((Sw * 0.5, Sh * 0.5), 0.0, (0, int(magnitude)), 1.0, (0.0, 0.0))
    elif op == TA_ROTATE:
        m = rotate_matrix(magnitude, Sh, Sw)
    elif TA_BRIGHTNESS <= op <= TA_SHARPNESS:
        arg = 1.0 + magnitude
    elif op == TA_POSTERIZE:
        arg = float(int(magnitude))
    elif op == TA_SOLARIZE:
        arg = float(magnitude)
    elif op not in (TA_IDENTITY, TA_AUTOCONTRAST, TA_EQUALIZE):
        raise ValueError(f"op {op}: 0 .. {len(TA_OPS) - 1}")
    return [float(op), *[float(v) for v in m], arg]


def sample_trivial_augment(sizes_or_B, out_size, generator: Optional[torch.Generator] = None, return_draws: bool = False):
    """The TrivialAugmentWide table, float64 [B, 8] (TA_FIELDS), for B images of out_size levels: per image one uniform op of
    the 14, one uniform bin of the 31 and, for the signed ops, a fair coin for the sign.  The draws are ONE torch.rand(B, 3,
    float64) of the CPU generator of its own: the stream of sample_train_params does not move.
    return_draws: also return int64 [B, 3] = (op, bin or -1 for an op without magnitudes, 1 where the magnitude was negated)."""
    B = sizes_or_B if isinstance(sizes_or_B, int) else len(sizes_or_B)
    U = torch.rand(B, 3, dtype=torch.float64, generator=generator).tolist()
    rows, draws = [], []
    for u in U:
        op = _randint(u[0], len(TA_OPS))
        mags = ta_magnitudes(op)
        k = _randint(u[1], TA_BINS) if mags is not None else -1
        mag = mags[k] if mags is not None else 0.0
        neg = op in TA_SIGNED and u[2] >= 0.5
        rows.append(ta_row(op, -mag if neg else mag, out_size))
        draws.append([op, k, int(neg)])
    ta = torch.tensor(rows, dtype=torch.float64).reshape(B, 8)
    return (ta, torch.tensor(draws, dtype=torch.int64).reshape(B, 3)) if return_draws else ta


def trivial_augment_identity(B: int) -> torch.Tensor:
    """a table of B Identity rows: the 8-bit stage alone (levels rounded half up, then / 255)"""
    return torch.tensor([_TA_IDENTITY_ROW] * B, dtype=torch.float64).reshape(B, 8)


def validate_ta(ta: torch.Tensor, B: Optional[int] = None) -> None:
    """ValueError naming the image and the field for a host table the kernel would have to clamp or treat as Identity."""
    if ta.dtype != torch.float64 or ta.dim() != 2 or ta.shape[1] != 8 or (B is not None and ta.shape[0] != B):
        raise ValueError(f"ta: expected float64 [{'B' if B is None else B}, 8], got {ta.dtype} {tuple(ta.shape)}")
    for b, row in enumerate(ta.tolist()):

        def bad(field, why):
            raise ValueError(f"ta[{b}].{field} = {row[TA_FIELDS.index(field)]}: {why}")

        op = row[0]
        if not (math.isfinite(op) and op == int(op) and 0 <= op < len(TA_OPS)):
            bad("op", f"an integer in 0 .. {len(TA_OPS) - 1}")
        for k in range(1, 7):
            if not math.isfinite(row[k]):
                bad(TA_FIELDS[k], "the matrix needs finite coefficients")
        op, arg = int(op), row[7]
        if TA_BRIGHTNESS <= op <= TA_SHARPNESS and not (math.isfinite(arg) and arg >= 0.0):
            bad("arg", f"{TA_OPS[op]} needs a finite factor >= 0")
        if op == TA_POSTERIZE and not (math.isfinite(arg) and arg == int(arg) and 1 <= arg <= 8):
            bad("arg", "Posterize keeps 1 .. 8 bits")
        if op == TA_SOLARIZE and math.isnan(arg):
            bad("arg", "Solarize needs a threshold")


# ---- the plain-torch path (CPU tensors) ----------------------------------------------------------------------------
def round_levels(v255: torch.Tensor) -> torch.Tensor:
    """float32 values on the 0 .. 255 scale -> uint8 levels, rounded half up (floor(v + 0.5) in float32) and clamped"""
    return torch.floor(v255.to(torch.float32) + 0.5).clamp_(0.0, 255.0).to(torch.uint8)


def _blend(deg: torch.Tensor, a: torch.Tensor, f: float) -> torch.Tensor:
    """PIL's ImageEnhance blend on 8-bit levels: deg + f (a - deg) in float32 (a product, then a sum), clipped, truncated"""
    d = deg.to(torch.float32)
    t = d + (a.to(torch.float32) - d) * torch.tensor(f, dtype=torch.float32)
    return torch.where(t <= 0.0, torch.zeros_like(t), torch.where(t >= 255.0, torch.full_like(t, 255.0), torch.floor(t))).to(torch.int64)


def _gray(a: torch.Tensor) -> torch.Tensor:
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16


def _smooth(a: torch.Tensor) -> torch.Tensor:
    """PIL's ImageFilter.SMOOTH: (3 x 3 sum + 4 centre) / 13 rounded half up inside, the border rows and columns copied"""
    out = a.clone()
    H, W = a.shape[:2]
    if H >= 3 and W >= 3:
        s = 4 * a[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + a[dy : dy + H - 2, dx : dx + W - 2]
        out[1:-1, 1:-1] = (2 * s + 13) // 26
    return out


def _affine(a: torch.Tensor, m: "list[float]") -> torch.Tensor:
    """PIL's Image.transform(AFFINE, m, BILINEAR) on 8-bit levels, fill 0: float64, products and sums apart"""
    H, W = a.shape[:2]
    xs = (torch.arange(W, dtype=torch.float64) + 0.5)[None, :]
    ys = (torch.arange(H, dtype=torch.float64) + 0.5)[:, None]
    xin = (m[0] * xs + m[1] * ys) + m[2]
    yin = (m[3] * xs + m[4] * ys) + m[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin = torch.where(inside, xin, torch.zeros_like(xin)) - 0.5
    yin = torch.where(inside, yin, torch.zeros_like(yin)) - 0.5
    x0, y0 = torch.floor(xin), torch.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.to(torch.int64), y0.to(torch.int64)
    xa, xb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
    ya, yb = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    p00, p01, p10, p11 = (a[y, x].to(torch.float64) for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    v1 = p00 + (p01 - p00) * dx
    v2 = p10 + (p11 - p10) * dx
    v = (v1 + (v2 - v1) * dy).to(torch.int64)
    return torch.where(inside[..., None], v, torch.zeros_like(v))


def _autocontrast_lut(h: "list[int]") -> "list[int]":
    nz = [i for i, n in enumerate(h) if n]
    if not nz or nz[-1] <= nz[0]:
        return list(range(256))
    scale = 255.0 / (nz[-1] - nz[0])
    offset = -nz[0] * scale
    return [min(max(int(i * scale + offset), 0), 255) for i in range(256)]


def _equalize_lut(h: "list[int]") -> "list[int]":
    nz = [n for n in h if n]
    if len(nz) <= 1:
        return list(range(256))
    step = (sum(nz) - nz[-1]) // 255
    if step == 0:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += h[i]
    return lut


def ta_decode(row: "Sequence[float]") -> "tuple[int, list[float], float]":
    """(op, matrix, arg) of a table row AS THE KERNEL READS IT (vt_amd.h): an op that is not a number in [0, 14) is Identity, a
    fractional one is truncated; Posterize's bit count is truncated and clamped into 1 .. 8 (not a number: 1)"""
    op = int(row[0]) if 0.0 <= row[0] < float(len(TA_OPS)) else TA_IDENTITY
    arg = row[7]
    if op == TA_POSTERIZE:
        arg = float(int(min(arg, 8.0))) if arg >= 1.0 else 1.0
    return op, [float(v) for v in row[1:7]], arg


def _apply_op(a: torch.Tensor, op: int, m: "list[float]", arg: float) -> torch.Tensor:
    """one image of levels, int64 [H, W, 3] -> int64 [H, W, 3]"""
    if op in _TA_AFFINE:
        return _affine(a, m)
    if op == TA_BRIGHTNESS:
        return _blend(torch.zeros_like(a), a, arg)
    if op == TA_COLOR:
        return _blend(_gray(a)[..., None].expand_as(a), a, arg)
    if op == TA_CONTRAST:
        g = _gray(a)
        mean = int(g.sum().item() / g.numel() + 0.5)
        return _blend(torch.full_like(a, mean), a, arg)
    if op == TA_SHARPNESS:
        return _blend(_smooth(a), a, arg)
    if op == TA_POSTERIZE:
        return a & (256 - (1 << (8 - int(arg))))
    if op == TA_SOLARIZE:
        return torch.where(a.to(torch.float64) < arg, a, 255 - a)
    if op in (TA_AUTOCONTRAST, TA_EQUALIZE):
        make = _autocontrast_lut if op == TA_AUTOCONTRAST else _equalize_lut
        out = torch.empty_like(a)
        for c in range(3):
            lut = torch.tensor(make(torch.bincount(a[..., c].reshape(-1), minlength=256).tolist()), dtype=torch.int64)
            out[..., c] = lut[a[..., c]]
        return out
    return a


def trivial_augment_levels(u8: torch.Tensor, ta: torch.Tensor) -> torch.Tensor:
    """The TrivialAugmentWide stage alone on the host: uint8 levels [B, S_h, S_w, 3] and the table float64 [B, 8] -> uint8
    levels [B, S_h, S_w, 3], each image under its own op exactly as PIL computes it on an 8-bit RGB image (integers, float32
    for the blends, float64 for the affine gather and the AutoContrast table).  The table is read as the kernel reads it
    (ta_decode), not validated."""
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError(f"u8: expected uint8 [B, S_h, S_w, 3], got {u8.dtype} {tuple(u8.shape)}")
    if ta.dtype != torch.float64 or tuple(ta.shape) != (u8.shape[0], 8):
        raise ValueError(f"ta: expected float64 [{u8.shape[0]}, 8], got {ta.dtype} {tuple(ta.shape)}")
    out = torch.empty_like(u8)
    for b, row in enumerate(ta.tolist()):
        out[b] = _apply_op(u8[b].to(torch.int64), *ta_decode(row)).to(torch.uint8)
    return out


def _mix32(x: torch.Tensor) -> torch.Tensor:
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m
    return x ^ (x >> 16)


def erase_normal(seed: int, b: int, Sh: int, Sw: int) -> torch.Tensor:
    """the kernel's standard-normal values for image b under `seed`, float32 [3, Sh, Sw] (the generator of vt_amd.h)"""
    m = 0xFFFFFFFF
    c = torch.arange(3, dtype=torch.int64).view(3, 1, 1)
    y = torch.arange(Sh, dtype=torch.int64).view(1, Sh, 1)
    x = torch.arange(Sw, dtype=torch.int64).view(1, 1, Sw)
    k = _mix32(torch.tensor(((seed & m) + 0x9E3779B9) & m, dtype=torch.int64))
    k = _mix32((k + (b & m)) & m)
    k = _mix32((k + c) & m)
    k = _mix32((k + y) & m)
    k = _mix32((k + x) & m)
    h1, h2 = _mix32(k ^ 0x68BC21EB), _mix32(k ^ 0x02E5BE93)
    u1 = ((h1 >> 8) + 1).to(torch.float32) * 2.0**-24
    u2 = (h2 >> 8).to(torch.float32) * 2.0**-24
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(torch.tensor(6.2831855, dtype=torch.float32) * u2)


def _axis_weights(n: int, out: int, first: int, count: int, antialias: bool) -> torch.Tensor:
    """float32 [count, n]: the normalised tap weights of virtual outputs first .. first + count - 1 (float64 inside)"""
    s = n / out
    sup = max(s, 1.0) if antialias else 1.0
    c = s * (torch.arange(first, first + count, dtype=torch.float64) + 0.5)
    lo = torch.clamp((c - sup + 0.5).to(torch.int64), min=0)
    hi = torch.clamp((c + sup + 0.5).to(torch.int64), max=n)
    j = torch.arange(n, dtype=torch.float64)
    wgt = torch.clamp(1.0 - ((j[None, :] - c[:, None] + 0.5) / sup).abs(), min=0.0)
    wgt = wgt * ((j[None, :] >= lo[:, None]) & (j[None, :] < hi[:, None]))
    return (wgt / wgt.sum(1, keepdim=True)).to(torch.float32)


class GPUBatchTransform:
    """crop-resize-flip-scale-erase of a RaggedBatch into float32 [B, 3, S_h, S_w].

    aug(batch, params, out=None): `params` int32 [B, 16] (sample_train_params / eval_params).  A table on the host is
    validated (ValueError naming image and field) and uploaded; a table already on the device is used as it is (the
    kernel clamps what would leave an image).  `out` may be a preallocated batch such as TrainStep.images.

    ta: the TrivialAugmentWide table, float64 [B, 8] (sample_trivial_augment), or None for exactly the path above.  With a
    table the batch takes two calls, vt_augment_batch_u8 into a uint8 [B, S_h, S_w, 3] intermediate and vt_trivial_augment
    from it into `out`; the intermediate and the histogram workspace are kept on the object per device and batch size.  A
    host table is validated (validate_ta), a device table is used as it is (vt_amd.h says what the kernel makes of it)."""

    def __init__(self, crop_size, antialias: bool = True, mean=None, std=None):
        self.Sh, self.Sw = _pair(crop_size)
        if self.Sh < 1 or self.Sw < 1:
            raise ValueError(f"crop_size={crop_size!r}")
        self.antialias = bool(antialias)
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        self.mean_std = None
        if mean is not None:
            ms = torch.tensor(list(mean) + list(std), dtype=torch.float32)
            if ms.numel() != 6 or not bool((ms[3:] != 0).all()):
                raise ValueError("mean and std are three numbers each, std non-zero")
            self.mean_std = ms
        self._ms_dev = {}
        self._ta_buffers = {}

    def _ta_buffers_on(self, device, B: int):
        """(uint8 [B, S_h, S_w, 3] levels, uint32 [B, 4, 256] histograms as int32) of the two-call path"""
        key = (str(device), B)
        if key not in self._ta_buffers:
            self._ta_buffers[key] = (torch.empty((B, self.Sh, self.Sw, 3), dtype=torch.uint8, device=device),
                                     torch.empty((B, 4, 256), dtype=torch.int32, device=device))
        return self._ta_buffers[key]

    def _mean_std_on(self, device):
        if self.mean_std is None:
            return None
        key = str(device)
        if key not in self._ms_dev:
            self._ms_dev[key] = self.mean_std.to(device)
        return self._ms_dev[key]

    def __call__(self, batch: RaggedBatch, params: torch.Tensor, out: Optional[torch.Tensor] = None,
                 ta: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, dev = len(batch), batch.raw.device
        if ta is not None:
            if ta.device.type == "cpu":
                validate_ta(ta, B)
            elif ta.dtype != torch.float64 or tuple(ta.shape) != (B, 8):
                raise ValueError(f"ta: expected float64 [{B}, 8], got {ta.dtype} {tuple(ta.shape)}")
        if batch.table.device != dev:
            raise ValueError(f"batch.raw is on {dev}, batch.table on {batch.table.device}")
        if params.device.type == "cpu":
            validate_params(params, batch.sizes, (self.Sh, self.Sw))
        elif params.dtype != torch.int32 or tuple(params.shape) != (B, 16):
            raise ValueError(f"params: expected int32 [{B}, 16], got {params.dtype} {tuple(params.shape)}")
        shape = (B, 3, self.Sh, self.Sw)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out: expected a contiguous float32 {shape} on {dev}, got {out.dtype} {tuple(out.shape)} on "
                             f"{out.device}")
        if dev.type != "cuda":
            return self._run_torch(batch, params.cpu(), out, None if ta is None else ta.cpu())
        params = params.to(dev, non_blocking=True).contiguous()
        ms = self._mean_std_on(dev)
        with torch.cuda.device(dev):
            stream = int(torch.cuda.current_stream().cuda_stream)
            if ta is not None:
                ta = ta.to(dev, non_blocking=True).contiguous()
                u8, work = self._ta_buffers_on(dev, B)
                N.check(N.lib().vt_augment_batch_u8(C.c_void_p(batch.raw.data_ptr()), C.c_void_p(batch.table.data_ptr()),
                                                    C.c_void_p(params.data_ptr()), C.c_void_p(u8.data_ptr()), B, self.Sh, self.Sw,
                                                    int(self.antialias), 0, C.c_void_p(stream)))
                N.check(N.lib().vt_trivial_augment(C.c_void_p(u8.data_ptr()), C.c_void_p(ta.data_ptr()),
                                                   C.c_void_p(params.data_ptr()), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(work.data_ptr()), B, self.Sh, self.Sw,
                                                   C.c_void_p(ms.data_ptr()) if ms is not None else None, C.c_void_p(stream)))
                return out
            N.check(N.lib().vt_augment_batch(C.c_void_p(batch.raw.data_ptr()), C.c_void_p(batch.table.data_ptr()),
                                             C.c_void_p(params.data_ptr()), C.c_void_p(out.data_ptr()), B, self.Sh, self.Sw,
                                             int(self.antialias), C.c_void_p(ms.data_ptr()) if ms is not None else None,
                                             0, C.c_void_p(stream)))
        return out

    def _levels_torch(self, batch: RaggedBatch, params: torch.Tensor) -> torch.Tensor:
        """the 8-bit stage of the CPU path (what vt_augment_batch_u8 computes): the filtered value on the 0 .. 255 scale,
        rounded half up, uint8 [B, S_h, S_w, 3]; no erase"""
        Sh, Sw = self.Sh, self.Sw
        levels = torch.empty((len(batch), Sh, Sw, 3), dtype=torch.uint8)
        for b, ((H, W), row) in enumerate(zip(batch.sizes, params.tolist())):
            top, left, h, w, OH, OW, oy, ox, flip = row[:9]
            off = int(batch.table[b, 0])
            img = batch.raw[off : off + H * W * 3].view(H, W, 3)
            crop = img[top : top + h, left : left + w].permute(2, 0, 1).to(torch.float32)
            wy = _axis_weights(h, OH, oy, Sh, self.antialias)
            wx = _axis_weights(w, OW, ox, Sw, self.antialias)
            if flip:
                wx = wx.flip(0)
            levels[b] = round_levels(torch.matmul(torch.matmul(wy, crop), wx.t())).permute(1, 2, 0)
        return levels

    def _finish_torch(self, levels: torch.Tensor, params: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """uint8 levels [B, S_h, S_w, 3] -> float32(level) * (1 / 255), mean / std, erase (what vt_trivial_augment does
        after its op)"""
        Sh, Sw = self.Sh, self.Sw
        for b, row in enumerate(params.tolist()):
            ei, ej, eh, ew, mode, seed, bits = row[9:]
            v = levels[b].permute(2, 0, 1).to(torch.float32) * (1.0 / 255.0)
            if self.mean_std is not None:
                v = (v - self.mean_std[:3].view(3, 1, 1)) / self.mean_std[3:].view(3, 1, 1)
            if mode != ERASE_NONE and eh > 0 and ew > 0:
                if mode == ERASE_CONSTANT:
                    v[:, ei : ei + eh, ej : ej + ew] = C.c_float.from_buffer_copy(C.c_int32(bits)).value
                else:
                    v[:, ei : ei + eh, ej : ej + ew] = erase_normal(seed, b, Sh, Sw)[:, ei : ei + eh, ej : ej + ew]
            out[b].copy_(v)
        return out

    def _run_torch(self, batch: RaggedBatch, params: torch.Tensor, out: torch.Tensor,
                   ta: Optional[torch.Tensor] = None) -> torch.Tensor:
        if ta is not None:
            return self._finish_torch(trivial_augment_levels(self._levels_torch(batch, params), ta), params, out)
        Sh, Sw = self.Sh, self.Sw
        for b, ((H, W), row) in enumerate(zip(batch.sizes, params.tolist())):
            top, left, h, w, OH, OW, oy, ox, flip, ei, ej, eh, ew, mode, seed, bits = row
            off = int(batch.table[b, 0])
            img = batch.raw[off : off + H * W * 3].view(H, W, 3)
            crop = img[top : top + h, left : left + w].permute(2, 0, 1).to(torch.float32)
            wy = _axis_weights(h, OH, oy, Sh, self.antialias)
            wx = _axis_weights(w, OW, ox, Sw, self.antialias)
            if flip:
                wx = wx.flip(0)
            v = torch.matmul(torch.matmul(wy, crop), wx.t()) * (1.0 / 255.0)
            if self.mean_std is not None:
                v = (v - self.mean_std[:3].view(3, 1, 1)) / self.mean_std[3:].view(3, 1, 1)
            if mode != ERASE_NONE and eh > 0 and ew > 0:
                if mode == ERASE_CONSTANT:
                    v[:, ei : ei + eh, ej : ej + ew] = C.c_float.from_buffer_copy(C.c_int32(bits)).value
                else:
                    v[:, ei : ei + eh, ej : ej + ew] = erase_normal(seed, b, Sh, Sw)[:, ei : ei + eh, ej : ej + ew]
            out[b].copy_(v)
        return out


# ---- baseline JPEG decoding ---------------------------------------------------------------------------------------------
# The reference's image_loader (classifier.py:22-25) is torchvision.io.decode_jpeg(read_file(path), device=device).  Here:
#
#     batch = decode_jpeg_batch(files, device="cuda")      # list of JPEG byte strings -> RaggedBatch on the device
#     aug(batch, sample_train_params(batch.sizes, 176), out=ts.images); ts.step()
#
# The host reads the markers (jpeg_info), refuses what is out of scope (jpeg_check) and packs the streams and the tables of
# vt_amd.h (JpegBatch); two launches (vt_jpeg_entropy, vt_jpeg_idct_rgb, csrc/vt_jpeg.hip) decode them.  The DEFINITION of the
# result is jpeg_decode_levels below: libjpeg's default decode restated in integer torch (Huffman decode, the accurate integer
# IDCT, "fancy" triangle chroma upsampling, 16-bit fixed-point YCbCr -> RGB), which the CPU tests compare with PIL level for
# level and the GPU tests compare the kernels with.  libjpeg's source was not at hand: it is restated from its documentation
# and from memory, and PIL arbitrates.
JPEG_NATURAL = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                47, 55, 62, 63)  # zigzag position -> natural (row-major) index
JPEG_IMG_FIELDS, JPEG_SEG_FIELDS, JPEG_HUFF_BYTES = 24, 6, 272
(JI_H, JI_W, JI_NC, JI_HMAX, JI_VMAX, JI_MCUS_X, JI_MCUS_Y, JI_Q0, JI_Q1, JI_Q2, JI_DC0, JI_AC0, JI_DC1, JI_AC1, JI_DC2, JI_AC2,
 JI_COEF, JI_OUT, JI_SEG0, JI_NSEG, JI_RESTART) = range(21)
JPEG_OK, JPEG_ERR_CODE, JPEG_ERR_RUN, JPEG_ERR_TRUNCATED, JPEG_ERR_TABLE, JPEG_ERR_TRAILING = range(6)
JPEG_SAMPLINGS = {((1, 1),): "gray", ((1, 1), (1, 1), (1, 1)): "4:4:4", ((2, 1), (1, 1), (1, 1)): "4:2:2",
                  ((2, 2), (1, 1), (1, 1)): "4:2:0"}
_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
              0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)", 0xCD: "arithmetic coding (SOF13)",
              0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


class JpegInfo:
    """What the markers of a JPEG file say (jpeg_info).  width, height, precision, sof (the marker byte, 0xC0 ..), components =
    [(id, h, v, quantisation table id)] (the factors of a single-component frame are given as 1 x 1, which is what they mean), qtabs = {id: (precision 8 | 16, [64 values in NATURAL order])}, huff = {(class 0 DC | 1
    AC, id): (BITS bytes[16], HUFFVAL bytes)}, restart_interval (MCUs, 0: none), scans = number of SOS markers, scan_components
    = [(component index, DC table id, AC table id)] and spectral = (Ss, Se, Ah, Al) of the FIRST scan, scan_offset = its first
    entropy-coded byte, scan_end = the first byte after its entropy-coded data (the FF of the marker that ends it)."""

    __slots__ = ("width", "height", "precision", "sof", "components", "qtabs", "huff", "restart_interval", "scans",
                 "scan_components", "spectral", "scan_offset", "scan_end", "segments")

    @property
    def sampling(self) -> "Optional[str]":
        return JPEG_SAMPLINGS.get(tuple((h, v) for _, h, v, _ in self.components))

    @property
    def mcu_geometry(self) -> "tuple[int, int, int, int]":
        """(h_max, v_max, MCUs per row, MCU rows)"""
        hm, vm = max(c[1] for c in self.components), max(c[2] for c in self.components)
        return hm, vm, -(-self.width // (8 * hm)), -(-self.height // (8 * vm))


def _jpeg_markers(data: bytes, begin: int, limit: int) -> "list[tuple[int, int]]":
    """(index of the first FF of the marker, marker code) of every marker in data[begin:limit]: an FF followed by a byte that is
    neither 00 (a stuffed data byte) nor FF (a fill byte; the run of FFs belongs to the marker that ends it)"""
    a = torch.frombuffer(bytearray(data[begin:limit]), dtype=torch.uint8) if limit > begin else torch.empty(0, dtype=torch.uint8)
    if a.numel() < 2:
        return []
    hit = ((a[:-1] == 0xFF) & (a[1:] != 0) & (a[1:] != 0xFF)).nonzero().flatten().tolist()
    out = []
    for p in hit:
        q = p + begin
        code = data[q + 1]
        while q > begin and data[q - 1] == 0xFF:
            q -= 1
        out.append((q, code))
    return out


def jpeg_info(data: bytes) -> JpegInfo:
    """Read the markers of a JPEG file; nothing is decoded.  ValueError for a file that is not a JPEG or whose header is
    truncated or inconsistent.  What this package can decode is jpeg_check's business, not this function's."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("not a JPEG file: no SOI marker")
    info = JpegInfo()
    info.qtabs, info.huff, info.restart_interval, info.scans = {}, {}, 0, 0
    info.width = info.height = info.precision = info.sof = None
    info.components, info.scan_components, info.segments = [], [], None
    pos = 2

    def need(k, what):
        if pos + k > n:
            raise ValueError(f"truncated header: the file ends inside {what}")

    while True:
        need(2, "a marker")
        if data[pos] != 0xFF:
            raise ValueError(f"byte {pos}: expected a marker, found {data[pos]:#04x}")
        while pos < n and data[pos] == 0xFF:  # fill bytes
            pos += 1
        need(1, "a marker")
        m = data[pos]
        pos += 1
        if m == 0xD9:
            raise ValueError("truncated header: EOI before any scan")
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        need(2, f"the length of segment {m:#04x}")
        L = (data[pos] << 8) | data[pos + 1]
        if L < 2:
            raise ValueError(f"segment {m:#04x} at byte {pos}: length {L}")
        need(L, f"segment {m:#04x}")
        seg = data[pos + 2 : pos + L]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                size = 128 if pq else 64
                if pq > 1 or i + 1 + size > len(seg):
                    raise ValueError(f"DQT at byte {pos}: malformed table")
                vals = [(seg[i + 1 + 2 * k] << 8) | seg[i + 2 + 2 * k] for k in range(64)] if pq else list(seg[i + 1 : i + 65])
                nat = [0] * 64
                for k in range(64):
                    nat[JPEG_NATURAL[k]] = vals[k]
                info.qtabs[tq] = (16 if pq else 8, nat)
                i += 1 + size
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise ValueError(f"DHT at byte {pos}: malformed table")
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = bytes(seg[i + 1 : i + 17])
                cnt = sum(bits)
                if tc > 1 or cnt > 256 or i + 17 + cnt > len(seg):
                    raise ValueError(f"DHT at byte {pos}: malformed table")
                info.huff[(tc, th)] = (bits, bytes(seg[i + 17 : i + 17 + cnt]))
                i += 17 + cnt
        elif m == 0xDD:
            if len(seg) < 2:
                raise ValueError("DRI: malformed segment")
            info.restart_interval = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if info.sof is not None:
                raise ValueError("two frame headers")
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                raise ValueError("SOF: malformed segment")
            info.sof, info.precision = m, seg[0]
            info.height, info.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            info.components = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])]
            if len(info.components) == 1:  # a single component is never sub-sampled: its factors only scale an MCU that is one block
                info.components = [(info.components[0][0], 1, 1, info.components[0][3])]
        elif m == 0xDA:
            if info.sof is None:
                raise ValueError("SOS before the frame header")
            ns = seg[0] if seg else 0
            if len(seg) < 1 + 2 * ns + 3:
                raise ValueError("SOS: malformed segment")
            ids = [c[0] for c in info.components]
            for k in range(ns):
                cid = seg[1 + 2 * k]
                if cid not in ids:
                    raise ValueError(f"SOS: component id {cid} is not in the frame")
                info.scan_components.append((ids.index(cid), seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15))
            info.spectral = (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15)
            info.scans = 1
            info.scan_offset = pos + L
            break
        pos += L
    # the entropy-coded data of the first scan: up to the first marker that is not RSTn; what follows decides `scans`
    marks = _jpeg_markers(data, info.scan_offset, n)
    segs, begin, info.scan_end = [], info.scan_offset, n
    for q, code in marks:
        if 0xD0 <= code <= 0xD7:
            segs.append((begin, q))
            begin = data.index(bytes([code]), q) + 1
            continue
        info.scan_end = q
        for _, c in marks:  # further scans of THIS image: up to its EOI (what follows EOI -- a trailer, a second image -- is not ours)
            if c == 0xD9:
                break
            info.scans += c == 0xDA
        break
    segs.append((begin, info.scan_end))
    info.segments = segs
    return info


def jpeg_check(info: JpegInfo, index: Optional[int] = None) -> None:
    """Raise for a file outside the scope of the decoder, naming the image and the property: NotImplementedError for a kind of
    JPEG that exists but is not built here, ValueError for a file that is inconsistent."""
    who = "image" if index is None else f"image {index}"

    def no(what):
        raise NotImplementedError(f"{who}: {what} is not supported (baseline Huffman JPEG, 8 bit, one interleaved scan, gray / "
                                  f"4:4:4 / 4:2:2 / 4:2:0)")

    if info.sof in _SOF_NAMES:
        no(_SOF_NAMES[info.sof])
    if info.precision != 8:
        no(f"{info.precision}-bit precision")
    if info.width < 1 or info.height < 1:
        raise ValueError(f"{who}: size {info.width} x {info.height}")
    if len(info.components) == 4:
        no("4 components (CMYK / YCCK)")
    if len(info.components) not in (1, 3):
        no(f"{len(info.components)} components")
    if info.sampling is None:
        no("sampling " + ", ".join(f"{h}x{v}" for _, h, v, _ in info.components))
    if info.scans != 1:
        no(f"{info.scans} scans (multiple scans)")
    if [c for c, _, _ in info.scan_components] != list(range(len(info.components))):
        no(f"a non-interleaved scan (components {[c for c, _, _ in info.scan_components]} of {len(info.components)})")
    if info.spectral != (0, 63, 0, 0):
        no(f"spectral selection / successive approximation {info.spectral}")
    for _, _, _, tq in info.components:
        if tq not in info.qtabs:
            raise ValueError(f"{who}: missing quantisation table {tq}")
        if info.qtabs[tq][0] != 8:
            no(f"16-bit quantisation table {tq}")
    for _, td, ta in info.scan_components:
        for key in ((0, td), (1, ta)):
            if key not in info.huff:
                raise ValueError(f"{who}: missing Huffman table {'DC' if key[0] == 0 else 'AC'} {key[1]}")


def jpeg_segment_table(info: JpegInfo) -> "list[tuple[int, int, int, int]]":
    """(first byte, one past the last byte, first MCU, MCU count) of every entropy segment of the scan.  Without DRI: one segment.
    With an interval of Ri MCUs: ceil(MCUs / Ri) segments; if the file has fewer (damaged), the last one found takes all the
    MCUs that are left, and further segments of the file are not used."""
    _, _, mx, my = info.mcu_geometry
    total, Ri = mx * my, info.restart_interval
    if Ri <= 0:
        return [(info.segments[0][0], info.segments[0][1], 0, total)]
    wanted = -(-total // Ri)
    found = info.segments[:wanted]
    out = []
    for k, (b, e) in enumerate(found):
        first = k * Ri
        out.append((b, e, first, total - first if k == len(found) - 1 else Ri))
    return out


def _huff_lut(bits: bytes, huffval: bytes) -> "Optional[list[int]]":
    """16-bit lookahead -> (length << 8) | value, 0 for a pattern that is no code; None for a table that is not a prefix code
    (the rule of vt_jpeg_huff_build)"""
    key = (bits, huffval)
    if key not in _HUFF_LUTS:
        lut, code, k, valid = [0] * 65536, 0, 0, True
        for l in range(1, 17):
            nl = bits[l - 1]
            if code + nl > (1 << l):
                valid = False
                break
            for _ in range(nl):
                v = huffval[k] if k < len(huffval) else 0
                lut[code << (16 - l) : (code + 1) << (16 - l)] = [(l << 8) | v] * (1 << (16 - l))
                code, k = code + 1, k + 1
            code <<= 1
        _HUFF_LUTS[key] = lut if valid and sum(bits) <= 256 else None
    return _HUFF_LUTS[key]


_HUFF_LUTS: dict = {}


def _unstuff(seg: bytes) -> bytes:
    """the data bytes of a segment: FF 00 -> FF; an FF followed by anything else (or by nothing) ends the data"""
    out, i, n = bytearray(), 0, len(seg)
    while True:
        j = seg.find(b"\xff", i)
        if j < 0:
            out += seg[i:]
            break
        if j + 1 < n and seg[j + 1] == 0:
            out += seg[i : j + 1]
            i = j + 2
        else:
            out += seg[i:j]
            break
    return bytes(out)


def jpeg_decode_coefficients(data: bytes, info: Optional[JpegInfo] = None, segments=None, huff=None):
    """The entropy stage on the host, the definition vt_jpeg_entropy is held to: (coef int16 [blocks, 64], status [segments]).
    Blocks are component after component, each a raster of (MCUs per row x h_c) x (MCU rows x v_c) blocks, coefficients in
    natural order, DC prediction resolved.  Statuses as in vt_amd.h; from the block in which an error happens on, a segment's
    blocks are zeros.  `segments` / `huff` replace the file's own segment table / Huffman tables (the tests damage them)."""
    data = bytes(data)
    if info is None:
        info = jpeg_info(data)
        jpeg_check(info)
    hm, vm, mx, my = info.mcu_geometry
    nc = len(info.components)
    segments = jpeg_segment_table(info) if segments is None else segments
    huff = info.huff if huff is None else huff
    nY = mx * hm * my * vm
    coef = torch.zeros((nY + (2 * mx * my if nc == 3 else 0), 64), dtype=torch.int16)
    luts = []
    for _, td, ta in info.scan_components:
        luts.append((_huff_lut(*huff[(0, td)]), _huff_lut(*huff[(1, ta)])))
    table_ok = all(d is not None and a is not None for d, a in luts)
    statuses = []
    for begin, end, m0, mc in segments:
        if not (0 <= begin <= end <= len(data) and 0 <= m0 and 0 <= mc and m0 + mc <= mx * my):
            statuses.append(JPEG_ERR_TABLE)
            continue
        if not table_ok:
            statuses.append(JPEG_ERR_TABLE)
            continue
        buf = _unstuff(data[begin:end])
        real = 8 * len(buf)
        buf += b"\0" * 260  # zero bits past the end, as the kernel's reader supplies them (a block reads < 2048 bits)
        bp, st, pred = 0, JPEG_OK, [0] * nc
        rows = []
        for mcu in range(m0, m0 + mc):
            mcx, mcy = mcu % mx, mcu // mx
            for c in range(nc):
                dcl, acl = luts[c]
                for v in range(vm if c == 0 else 1):
                    for h in range(hm if c == 0 else 1):
                        blk = (mcy * vm + v) * mx * hm + mcx * hm + h if c == 0 else nY + (c - 1) * mx * my + mcy * mx + mcx
                        if st != JPEG_OK:
                            continue
                        vals = [0] * 64
                        while True:  # one block
                            e = dcl[(int.from_bytes(buf[bp >> 3 : (bp >> 3) + 3], "big") >> (8 - (bp & 7))) & 0xFFFF]
                            if e == 0 or (e & 255) > 15:
                                st = JPEG_ERR_CODE
                                break
                            bp += e >> 8
                            s = e & 255
                            if s:
                                x = (int.from_bytes(buf[bp >> 3 : (bp >> 3) + 3], "big") >> (24 - (bp & 7) - s)) & ((1 << s) - 1)
                                bp += s
                                d = x - (1 << s) + 1 if x < (1 << (s - 1)) else x
                                pred[c] = ((pred[c] + d + 32768) & 0xFFFF) - 32768
                            vals[0] = pred[c]
                            k = 1
                            while k < 64:
                                e = acl[(int.from_bytes(buf[bp >> 3 : (bp >> 3) + 3], "big") >> (8 - (bp & 7))) & 0xFFFF]
                                if e == 0:
                                    st = JPEG_ERR_CODE
                                    break
                                bp += e >> 8
                                run, s = (e & 255) >> 4, e & 15
                                if s == 0:
                                    if run != 15:
                                        break
                                    if k + 15 > 63:
                                        st = JPEG_ERR_RUN
                                        break
                                    k += 16
                                    continue
                                k += run
                                if k > 63:
                                    st = JPEG_ERR_RUN
                                    break
                                x = (int.from_bytes(buf[bp >> 3 : (bp >> 3) + 3], "big") >> (24 - (bp & 7) - s)) & ((1 << s) - 1)
                                bp += s
                                vals[JPEG_NATURAL[k]] = x - (1 << s) + 1 if x < (1 << (s - 1)) else x
                                k += 1
                            break
                        if st == JPEG_OK and bp > real:
                            st = JPEG_ERR_TRUNCATED
                        if st == JPEG_OK:
                            rows.append((blk, vals))
        if rows:
            coef[torch.tensor([b for b, _ in rows])] = torch.tensor([v for _, v in rows], dtype=torch.int16)
        if st == JPEG_OK and real - bp >= 8:
            st = JPEG_ERR_TRAILING
        statuses.append(st)
    return coef, statuses


_IDCT_C = (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172)


def _idct_1d(d, shift: int):
    """one pass of libjpeg's accurate integer IDCT (jidctint) on eight int64 tensors"""
    c0298, c0390, c0541, c0765, c0899, c1175, c1501, c1847, c1961, c2053, c2562, c3072 = _IDCT_C
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * c0541
    tmp2, tmp3 = z1 - z3 * c1847, z1 + z2 * c0765
    z2, z3 = d[0], d[4]
    tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c1175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c0298, tmp1 * c2053, tmp2 * c3072, tmp3 * c1501
    z1, z2, z3, z4 = -z1 * c0899, -z2 * c2562, -z3 * c1961 + z5, -z4 * c0390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)

    def descale(v):  # the sum as a signed 32-bit value (nothing wraps for a real image; see jpeg_idct_blocks), then the shift
        return ((((v + r) + 2147483648) & 0xFFFFFFFF) - 2147483648) >> shift

    return [descale(tmp10 + tmp3), descale(tmp11 + tmp2), descale(tmp12 + tmp1), descale(tmp13 + tmp0),
            descale(tmp13 - tmp0), descale(tmp12 - tmp1), descale(tmp11 - tmp2), descale(tmp10 - tmp3)]


def jpeg_idct_blocks(coef: torch.Tensor, q: "Sequence[int]") -> torch.Tensor:
    """int16 [N, 64] coefficients (natural order) and a quantisation table (natural order) -> int64 [N, 8, 8] samples 0 .. 255:
    dequantise, columns (CONST_BITS 13, PASS1_BITS 2), rows (descale by 18), + 128, clamp.  The sums of a pass are exact in
    int64 and are reduced to signed 32 bits before the pass's shift: for the coefficients of a real image nothing changes (libjpeg's
    32-bit arithmetic never overflows on them), and for the garbage of a damaged stream (any int16 times a table entry) the result
    is what the kernel's modulo-2^32 arithmetic gives, bit for bit, instead of an overflow."""
    d = coef.to(torch.int64).view(-1, 8, 8) * torch.tensor(list(q), dtype=torch.int64).view(1, 8, 8)
    ws = torch.stack(_idct_1d([d[:, k, :] for k in range(8)], 11), dim=1)
    out = torch.stack(_idct_1d([ws[:, :, k] for k in range(8)], 18), dim=2)
    return (out + 128).clamp_(0, 255)


def _jpeg_plane(samples: torch.Tensor, bh: int, bw: int) -> torch.Tensor:
    return samples.view(bh, bw, 8, 8).permute(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _near_far(n_out: int, n_in: int) -> "tuple[torch.Tensor, torch.Tensor, torch.Tensor]":
    """for outputs 0 .. n_out - 1 of a 2x triangle filter over n_in samples: near index, far index (clamped: edge
    replication), and whether the output is the odd one of its pair"""
    o = torch.arange(n_out, dtype=torch.int64)
    near = o >> 1
    odd = (o & 1).bool()
    far = (near + torch.where(odd, 1, -1)).clamp_(0, n_in - 1)
    return near, far, odd


def jpeg_pixels(coef: torch.Tensor, info: JpegInfo) -> torch.Tensor:
    """coefficients (jpeg_decode_coefficients' layout) -> uint8 [H, W, 3]: IDCT, fancy upsampling, colour conversion"""
    hm, vm, mx, my = info.mcu_geometry
    H, W, nc = info.height, info.width, len(info.components)
    nY = mx * hm * my * vm
    y = _jpeg_plane(jpeg_idct_blocks(coef[:nY], info.qtabs[info.components[0][3]][1]), my * vm, mx * hm)[:H, :W]
    if nc == 1:
        return y.to(torch.uint8)[..., None].expand(H, W, 3).contiguous()
    ch, cw = -(-H // vm), -(-W // hm)
    cc = []
    for c in (1, 2):
        blocks = coef[nY + (c - 1) * mx * my : nY + c * mx * my]
        p = _jpeg_plane(jpeg_idct_blocks(blocks, info.qtabs[info.components[c][3]][1]), my, mx)[:ch, :cw]
        if hm == 2 and cw <= 2:
            # libjpeg takes the triangle ("fancy") upsamplers only for a component MORE than two samples wide
            # (downsampled_width > 2); a chroma plane of one or two columns is replicated, in both directions
            p = p[(torch.arange(H) // vm)][:, torch.arange(W) // 2]
        elif hm == 2:
            xn, xf, xodd = _near_far(W, cw)
            if vm == 2:  # h2v2: 9-3-3-1, + 8 on the even and + 7 on the odd output column
                yn, yf, _ = _near_far(H, ch)
                a = 3 * p[yn] + p[yf]
                p = (3 * a[:, xn] + a[:, xf] + torch.where(xodd, 7, 8)[None, :]) >> 4
            else:        # h2v1: 3 near + far, + 1 on the even and + 2 on the odd output column
                p = (3 * p[:, xn] + p[:, xf] + torch.where(xodd, 2, 1)[None, :]) >> 2
        cc.append(p - 128)
    cb, cr = cc
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return torch.stack([r, g, b], dim=2).clamp_(0, 255).to(torch.uint8)


def jpeg_decode_levels(data: bytes, return_status: bool = False):
    """The host stage: a baseline JPEG file -> uint8 [H, W, 3], libjpeg's default decode in integer torch (the definition the
    kernels are held to; PIL's Image.open(...).convert("RGB") level for level).  Out-of-scope files raise as jpeg_check says.
    return_status: also the image's status (the largest of its segments' statuses, 0 = clean)."""
    info = jpeg_info(data)
    jpeg_check(info)
    coef, st = jpeg_decode_coefficients(data, info)
    px = jpeg_pixels(coef, info)
    return (px, max(st)) if return_status else px


class JpegBatch:
    """The compressed streams of a batch packed for the device, with the tables of vt_amd.h (all on the host, pinned where there
    is a GPU): data uint8, images int64 [B, 24], segments int64 [S, 6], qtabs uint8 [NQ, 64], hufftabs uint8 [NH, 272]
    (de-duplicated over the batch), and on the host sizes = [(H, W)], infos, blocks (of the coefficient scratch), raw_bytes,
    max_mcus_x, max_mcus_y.  Built by from_bytes, which refuses out-of-scope files by image index before anything is launched."""

    @classmethod
    def from_bytes(cls, files: "Sequence[bytes]", out_offsets: "Optional[Sequence[int]]" = None,
                   indices: "Optional[Sequence[int]]" = None, infos: "Optional[Sequence[JpegInfo]]" = None,
                   alloc=None) -> "JpegBatch":
        """alloc(name, shape, dtype) -> an uninitialised host tensor for `data`, `images`, `segments`, `qtabs`, `hufftabs`
        (GPUJpegDecoder hands out views of the pinned staging buffers it keeps); None: fresh tensors, pinned where there is a GPU"""
        if len(files) == 0:
            raise ValueError("JpegBatch.from_bytes: no files")
        self = cls()
        self.infos, self.sizes = [], []
        qkeys, hkeys, img_rows, seg_rows, starts = {}, {}, [], [], []
        total, blocks, out = 0, 0, 0
        for i, f in enumerate(files):
            idx = i if indices is None else indices[i]
            if infos is not None:
                info = infos[i]
            else:
                try:
                    info = jpeg_info(f)
                except ValueError as e:
                    raise ValueError(f"image {idx}: {e}") from None
                jpeg_check(info, idx)
            hm, vm, mx, my = info.mcu_geometry
            nc = len(info.components)
            row = [0] * JPEG_IMG_FIELDS
            row[JI_H], row[JI_W], row[JI_NC], row[JI_HMAX], row[JI_VMAX], row[JI_MCUS_X], row[JI_MCUS_Y] = (
                info.height, info.width, nc, hm, vm, mx, my)
            for c, (_, _, _, tq) in enumerate(info.components):
                row[JI_Q0 + c] = qkeys.setdefault(bytes(info.qtabs[tq][1]), len(qkeys))
            for c, (_, td, ta) in enumerate(info.scan_components):
                for k, key in enumerate(((0, td), (1, ta))):
                    bits, vals = info.huff[key]
                    row[JI_DC0 + 2 * c + k] = hkeys.setdefault(bits + vals + b"\0" * (256 - len(vals)), len(hkeys))
            row[JI_COEF] = blocks
            row[JI_OUT] = out if out_offsets is None else int(out_offsets[i])
            segs = jpeg_segment_table(info)
            row[JI_SEG0], row[JI_NSEG], row[JI_RESTART] = len(seg_rows), len(segs), info.restart_interval
            for b, e, m0, mc in segs:
                seg_rows.append([i, total + b, total + e, m0, mc, 0])
            img_rows.append(row)
            starts.append(total)
            self.infos.append(info)
            self.sizes.append((info.height, info.width))
            blocks += mx * my * (hm * vm + (2 if nc == 3 else 0))
            out += info.height * info.width * 3
            total += (len(f) + 3) & ~3
        if alloc is None:
            pin = torch.cuda.is_available()

            def alloc(name, shape, dtype):
                return torch.empty(shape, dtype=dtype, pin_memory=pin)

        self.data = alloc("data", (total,), torch.uint8)  # (the up to 3 bytes between two files belong to no segment: never read)
        for f, s in zip(files, starts):
            self.data[s : s + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8)
        for name, rows, dtype in (("images", img_rows, torch.int64), ("segments", seg_rows, torch.int64),
                                  ("qtabs", [list(k) for k in qkeys], torch.uint8), ("hufftabs", [list(k) for k in hkeys], torch.uint8)):
            t = torch.tensor(rows, dtype=dtype)
            setattr(self, name, alloc(name, tuple(t.shape), dtype).copy_(t))
        self.starts, self.blocks, self.raw_bytes = starts, blocks, out
        self.max_mcus_x = max(r[JI_MCUS_X] for r in img_rows)
        self.max_mcus_y = max(r[JI_MCUS_Y] for r in img_rows)
        return self

    def __len__(self) -> int:
        return len(self.sizes)


class GPUJpegDecoder:
    """files -> RaggedBatch.  decoder(files, device="cuda", on_unsupported="raise"): on a CUDA device the two launches of
    csrc/vt_jpeg.hip; on the CPU the host stage (jpeg_decode_levels), image by image.  There is no fallback on the GPU: a file
    the kernels cannot decode raises (by image index and property) before anything is launched, or with
    on_unsupported="host" is decoded by PIL, if PIL is importable, and packed beside the others.  The batch carries `status`,
    int32 [B] on the batch's device: 0 for a clean image, otherwise the largest status of its entropy segments (vt_amd.h).
    band_mcu_rows is passed on to vt_jpeg_idct_rgb (0: its default).

    The object OWNS its buffers and reuses them from call to call, growing them when a batch needs more: the coefficient scratch,
    one per (device, stream) -- two streams never share one, and on a stream the next call's kernels are ordered behind the last
    call's -- and per device the pinned host staging buffers of everything that is uploaded (the packed streams, the four tables,
    the batch's (offset, H, W) table).  The uploads are asynchronous, so before the staging buffers are written again the object
    waits on an event recorded behind the previous call's uploads.  The host side keeps no lock: use one decoder per thread
    (decode_jpeg_batch shares ONE instance, for one thread)."""

    def __init__(self, band_mcu_rows: int = 0):
        self.band_mcu_rows = int(band_mcu_rows)
        self._scratch = {}
        self._staging = {}  # device -> {name: pinned tensor}
        self._uploaded = {}  # device -> event behind the last call's uploads

    def _stage(self, device, name, shape, dtype) -> torch.Tensor:
        """an uninitialised view of the device's pinned staging buffer `name`, grown (by at least half) when too small"""
        numel = 1
        for n in shape:
            numel *= int(n)
        pool = self._staging.setdefault(str(device), {})
        buf = pool.get(name)
        if buf is None or buf.dtype != dtype or buf.numel() < numel:
            grown = max(numel, 0 if buf is None or buf.dtype != dtype else buf.numel() * 3 // 2, 1)
            buf = pool[name] = torch.empty(grown, dtype=dtype, pin_memory=True)
        return buf[:numel].view(shape)

    def _scratch_on(self, device, blocks: int) -> torch.Tensor:
        key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
        need = int(N.lib().vt_jpeg_scratch_bytes(blocks))
        if key not in self._scratch or self._scratch[key].numel() * 2 < need:
            self._scratch[key] = torch.empty(need // 2, dtype=torch.int16, device=device)
        return self._scratch[key]

    @staticmethod
    def _split(files, on_unsupported):
        """(infos or None per file, PIL-decoded uint8 HWC tensor or None per file)"""
        if on_unsupported not in ("raise", "host"):
            raise ValueError(f"on_unsupported={on_unsupported!r}: 'raise' or 'host'")
        if len(files) == 0:
            raise ValueError("decode_jpeg_batch: no files")
        infos, hosted = [], []
        for i, f in enumerate(files):
            try:
                try:
                    info = jpeg_info(f)
                except ValueError as e:
                    raise ValueError(f"image {i}: {e}") from None
                jpeg_check(info, i)
                infos.append(info)
                hosted.append(None)
            except (ValueError, NotImplementedError):
                if on_unsupported == "raise":
                    raise
                refusal = sys.exc_info()[1]
                try:
                    import io

                    import numpy as np
                    from PIL import Image
                except ImportError:
                    raise refusal from None  # no PIL to hand the file to: the refusal itself, which names image and property
                infos.append(None)
                hosted.append(torch.from_numpy(np.array(Image.open(io.BytesIO(bytes(f))).convert("RGB"))))
        return infos, hosted

    def __call__(self, files: "Sequence[bytes]", device="cuda", on_unsupported: str = "raise") -> RaggedBatch:
        dev = torch.device(device)
        infos, hosted = self._split(files, on_unsupported)
        B = len(files)
        if dev.type != "cuda":
            images, status = [], []
            for f, info, h in zip(files, infos, hosted):
                if h is not None:
                    images.append(h)
                    status.append(0)
                else:
                    coef, st = jpeg_decode_coefficients(f, info)
                    images.append(jpeg_pixels(coef, info))
                    status.append(max(st))
            batch = RaggedBatch.from_images(images)
            batch.status = torch.tensor(status, dtype=torch.int32)
            return batch
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        sizes = [(i.height, i.width) if i is not None else (int(h.shape[0]), int(h.shape[1])) for i, h in zip(infos, hosted)]
        offsets, total = [], 0
        for H, W in sizes:
            offsets.append(total)
            total += H * W * 3
        if str(dev) in self._uploaded:  # the staging buffers may still be the source of the last call's uploads
            self._uploaded.pop(str(dev)).synchronize()

        def stage(name, shape, dtype):
            return self._stage(dev, name, shape, dtype)

        table = stage("table", (B, 3), torch.int64).copy_(torch.tensor([[o, H, W] for o, (H, W) in zip(offsets, sizes)], dtype=torch.int64))
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        on_dev = [i for i in range(B) if infos[i] is not None]
        with torch.cuda.device(dev):
            if on_dev:
                jb = JpegBatch.from_bytes([files[i] for i in on_dev], [offsets[i] for i in on_dev], on_dev, [infos[i] for i in on_dev],
                                          alloc=stage)
                seg_status = self.run(jb, raw, dev)
                which = stage("which", (len(on_dev),), torch.int64).copy_(torch.tensor(on_dev, dtype=torch.int64))
                seg_img = which.to(dev, non_blocking=True)[jb.segments[:, 0].to(dev, non_blocking=True)]
                status.scatter_reduce_(0, seg_img, seg_status, "amax", include_self=True)
            for i, h in enumerate(hosted):
                if h is not None:
                    raw[offsets[i] : offsets[i] + h.numel()].copy_(h.reshape(-1))
            batch = RaggedBatch(raw, table.to(dev, non_blocking=True), sizes)
            self._uploaded[str(dev)] = torch.cuda.Event()
            self._uploaded[str(dev)].record()
        batch.status = status
        return batch

    def run(self, jb: JpegBatch, raw: torch.Tensor, dev, coef: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the two launches for a packed batch into `raw` (uint8 on dev, jb's output offsets); returns the per-SEGMENT status,
        int32 [S] on dev.  `coef`: a scratch of the caller's (int16, at least jb.blocks * 64 elements) instead of the object's."""
        stream = int(torch.cuda.current_stream().cuda_stream)
        data, images, segments, qtabs, hufftabs = (t.to(dev, non_blocking=True)
                                                   for t in (jb.data, jb.images, jb.segments, jb.qtabs, jb.hufftabs))
        if coef is None:
            coef = self._scratch_on(dev, jb.blocks)
        seg_status = torch.empty(segments.shape[0], dtype=torch.int32, device=dev)
        lib = N.lib()
        N.check(lib.vt_jpeg_entropy(C.c_void_p(data.data_ptr()), data.numel(), C.c_void_p(images.data_ptr()), len(jb),
                                    C.c_void_p(segments.data_ptr()), segments.shape[0], C.c_void_p(hufftabs.data_ptr()),
                                    hufftabs.shape[0], C.c_void_p(coef.data_ptr()), jb.blocks, C.c_void_p(seg_status.data_ptr()),
                                    C.c_void_p(stream)))
        N.check(lib.vt_jpeg_idct_rgb(C.c_void_p(coef.data_ptr()), jb.blocks, C.c_void_p(images.data_ptr()), len(jb),
                                     C.c_void_p(qtabs.data_ptr()), qtabs.shape[0], C.c_void_p(raw.data_ptr()), raw.numel(),
                                     jb.max_mcus_x, jb.max_mcus_y, self.band_mcu_rows, C.c_void_p(stream)))
        return seg_status


_DEFAULT_JPEG_DECODER = GPUJpegDecoder()


def decode_jpeg_batch(files: "Sequence[bytes]", device="cpu", on_unsupported: str = "raise") -> RaggedBatch:
    """A list of JPEG byte strings -> RaggedBatch on `device` (raw, table, sizes as RaggedBatch.from_images of the decoded
    images gives them, plus status int32 [B]).  GPUJpegDecoder says what runs where; this is a shared instance of it."""
    return _DEFAULT_JPEG_DECODER(files, device, on_unsupported)


def image_loader(path, device="cpu") -> torch.Tensor:
    """the reference's image_loader (classifier.py:22-25): a JPEG file -> uint8 [3, H, W] on `device`"""
    with open(path, "rb") as f:
        data = f.read()
    batch = decode_jpeg_batch([data], device)
    H, W = batch.sizes[0]
    return batch.raw.view(H, W, 3).permute(2, 0, 1).contiguous()
