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
in the program's input op (trainer.py).  Not here: JPEG decoding, WebDataset / ImageFolder loaders.

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
        return RaggedBatch(self.raw.to(device, non_blocking=nb), self.table.to(device, non_blocking=nb), self.sizes)


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
