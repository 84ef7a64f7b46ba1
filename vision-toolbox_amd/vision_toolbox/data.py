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
in the program's input op (trainer.py).  Not here: TrivialAugmentWide, JPEG decoding, WebDataset / ImageFolder loaders.

torchvision is not installed where this was written: the sampling rules of RandomResizedCrop, RandomHorizontalFlip,
RandomErasing, Resize and CenterCrop are restated from its documentation and from memory, and the tests check their
properties (boxes inside the image, area and ratio ranges, the fallback, frequencies), not a torchvision random stream.

CUDA tensors run the kernel; there is no fallback on the GPU.  CPU tensors run a plain-torch float32 path of the same
definition (weight matrices and two matmuls per image), which is what the GPU tests compare the module against.
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


# ---- the plain-torch path (CPU tensors) ----------------------------------------------------------------------------
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
    kernel clamps what would leave an image).  `out` may be a preallocated batch such as TrainStep.images."""

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

    def _mean_std_on(self, device):
        if self.mean_std is None:
            return None
        key = str(device)
        if key not in self._ms_dev:
            self._ms_dev[key] = self.mean_std.to(device)
        return self._ms_dev[key]

    def __call__(self, batch: RaggedBatch, params: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, dev = len(batch), batch.raw.device
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
            return self._run_torch(batch, params.cpu(), out)
        params = params.to(dev, non_blocking=True).contiguous()
        ms = self._mean_std_on(dev)
        with torch.cuda.device(dev):
            stream = int(torch.cuda.current_stream().cuda_stream)
            N.check(N.lib().vt_augment_batch(C.c_void_p(batch.raw.data_ptr()), C.c_void_p(batch.table.data_ptr()),
                                             C.c_void_p(params.data_ptr()), C.c_void_p(out.data_ptr()), B, self.Sh, self.Sw,
                                             int(self.antialias), C.c_void_p(ms.data_ptr()) if ms is not None else None,
                                             0, C.c_void_p(stream)))
        return out

    def _run_torch(self, batch: RaggedBatch, params: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
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
