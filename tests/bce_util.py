"""The yardstick of the binary cross-entropy tests: the definition of include/vt_amd.h (vt_sigmoid_bce) restated with torch
tensors in whatever dtype the caller hands in -- float64 is the reference, float32 the "plain-f32 restatement" whose distance
from float64 tests/test_bce_cpu.py holds below half of every bound the GPU tests use -- plus the inputs (oracle.filler), the
counted bounds both sides share, and the three-step training restatement of tests/test_bce_gpu.py.

Bounds are elementwise in the k u S style of tests/head_neck_util.py: |got - ref64| <= k * u * S (+ 2^-8 |ref64| for the one
round-to-nearest-even store of a bf16 gradient, which is attainable), u = 2^-24, S the float64 sum of the absolute values of
the terms that enter the element, k the count of f32 roundings read from csrc/vt_bce.hip.  A library function documented to
n ulp counts as 2 n u (an ulp is up to 2 u relative); expf and log1pf are taken at 2 ulp = 4 u each.

K_GRAD = 16, against S = (sigmoid(x) + t) * |grad_scale'|, grad_scale' = grad_scale * (sum_classes ? 1 : 1 / N):
  e = expf(-|x|)                          4 u on e (the negation and |x| are exact)
  r = 1 / (1 + e), sg = r or e * r        the sum 1, the division 1, and e's 4 u reach sg at most whole: 6 u on sg
  t = wb [x lam] + wp [..] + off          1 - s, its product with lam, 1 - lam, its product, s / N, two sums: at most 4 u on t
                                          (the reference sees the f32 values of s and lam; a thresholded t is exact)
  sg - t                                  1, on |sg - t| <= sg + t
  grad_scale'                             1 / N and its product with grad_scale on the host: 2; the product in the kernel: 1
  = 6 + 4 + 1 + 3 = 14, counted as 16.
K_LOSS = 18, against S = sum over the batch of (max(x, 0) + |x t| + log1p(exp(-|x|))) / D:
  x * t                                   t's 4 u and the product's 1: 5 u |x t|
  max(x, 0) - x t                         1 (or none, contracted into a fused multiply-add), on at most S
  log1pf(e)                               e's 4 u move log1p(e) by at most 4 u relative (d log1p / log1p <= d e / e), its own 4
  the sum of the three                    1
  the sums over the row and the batch     double: 2^-53 per level, nothing at this scale
  (float)(total / D)                      1, and loss[0] += onto a zeroed cell is exact
  = 5 + 1 + 8 + 1 + 1 = 16, counted as 18."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import filler
from oracle import torch_ref as R

U = 2.0 ** -24
BF16_U = 2.0 ** -8
F32, BF16 = 0, 1   # VT_F32, VT_BF16
TD = {F32: torch.float32, BF16: torch.bfloat16}
DNAME = {F32: "f32", BF16: "bf16"}
K_GRAD, K_LOSS = 16, 18
# a gradient below the smallest normal number (sigmoid(-80) times a small grad_scale') sits on the subnormal grid or is
# flushed: either way off by less than the smallest normal number, whatever its size
TINY = 2.0 ** -126

# (B, N): the partner of the only row is the row itself; a widened head (the GPU test gives it ldl > N in a NaN-filled
# buffer); an ImageNet-sized row; a row that crosses four rounds of the 256 threads;
# one class; and a shape with ORDINARY logits only (PLAIN): a +-3e38 logit puts S of the loss at 1e35 and above, so next to one
# the scalar loss says little about the ordinary elements -- there the loss bound is tight for every setting
SHAPES = [(1, 16), (3, 10), (5, 1000), (4, 1027), (2, 1), (3, 33)]
PLAIN = {(3, 33)}
# the mix block: absent, or (mode, lam); mode 0 ignores lam.  With lam = 0.9 the threshold 0.2 lies BETWEEN the partner's weight
# and the own label's (0.1 or 0.09 + s / N against 0.9 or 0.81 + s / N); with the others both lie above it
HEADERS = [None, (0, 0.7), (1, 0.3), (2, 0.6), (1, 0.9)]
SMOOTHING = (0.0, 0.1)
THRESHOLDS = (None, 0.2)
THR_MARGIN = 1e-3
SPECIALS = (80.0, -80.0, 3e38, -3e38, 0.0)


def f32r(v: float) -> float:
    """a host double as the kernel receives it through a float argument"""
    return float(torch.tensor(v, dtype=torch.float32).item())


def target_values(N: int, lam: float, s: float):
    """every value an element of t can take before the threshold"""
    return (s / N, (1 - s) * lam + s / N, (1 - s) * (1 - lam) + s / N, 1 - s + s / N)


def labels(B: int, N: int) -> torch.Tensor:
    """row 1 repeats row 0's label (equal partners: the two terms add); where there are classes and rows enough, row 2
    differs from row 1 (unequal partners)"""
    y = filler.labels(B, N, seed=977 + N)
    if B > 1:
        y[1] = y[0]
    if B > 2 and N > 1 and y[2] == y[1]:
        y[2] = (y[1] + 1) % N
    return y


def logits(B: int, N: int, dtype: int) -> torch.Tensor:
    """|x| <= 12 beside +-80, +-3e38 and 0, as the kernel sees them after storage in `dtype`; with more than one row and
    class, row 0 carries 3e38 in its label's column (x * t at the top of the range)"""
    z = (filler.tensor(f"bce.x{B}x{N}", (B, N)) * 3).clamp(-12, 12)
    if (B, N) in PLAIN:
        return z.to(TD[dtype]).float()
    flat = z.view(-1)
    if flat.numel() < len(SPECIALS):
        flat[:] = torch.tensor([3e38, -80.0])[: flat.numel()]
    else:
        step = flat.numel() // len(SPECIALS)
        for j, v in enumerate(SPECIALS):
            flat[j * step + (1 if step > 1 else 0)] = v
    if B > 1 and N > 1:
        z[0, labels(B, N)[0]] = 3e38
    return z.to(TD[dtype]).float()


def target(y: torch.Tensor, N: int, header, s: float, thr, dtype=torch.float64) -> torch.Tensor:
    """t of the definition.  In float32 the operations are the kernel's, in its order."""
    mode, lam = header if header is not None else (0, 1.0)
    one = torch.ones((), dtype=dtype)
    lam_t = one * (f32r(lam) if mode != 0 else 1.0)
    s_t = one * f32r(s)
    own = (torch.arange(N)[None, :] == y[:, None]).to(dtype)
    partner = own.roll(1, 0)
    keep, off = one - s_t, s_t / N
    t = (keep * lam_t) * own + (keep * (one - lam_t)) * partner + off
    if thr is not None:
        t = (t > f32r(thr)).to(dtype)
    return t


def bce(x: torch.Tensor, t: torch.Tensor, grad_scale: float, sum_classes: bool):
    """(loss, dlogits, S of the loss, S of the gradient, row sums of the element loss, S of each row sum) in the dtype of x
    and t.  The element loss and the gradient are formed in that dtype, in the kernel's order; the sums are double, as the
    kernel's are."""
    B, N = x.shape
    dt = x.dtype
    e = torch.exp(-x.abs())
    sp = torch.log1p(e)
    l = (x.clamp(min=0) - x * t) + sp
    D = B if sum_classes else B * N
    loss = l.double().sum(1).sum() / D
    r = 1.0 / (1.0 + e)
    sg = torch.where(x >= 0, r, e * r)
    gs = torch.tensor(f32r(grad_scale), dtype=dt)
    if not sum_classes:
        gs = gs * (torch.ones((), dtype=dt) / N)
    grad = (sg - t) * gs
    s_rows = (x.clamp(min=0).double() + (x.double() * t.double()).abs() + sp.double()).sum(1)
    s_loss = s_rows.sum() / D
    s_grad = (sg.double() + t.double()) * abs(float(gs))
    if dt == torch.float32:
        loss = loss.float()
    return loss, grad, s_loss, s_grad, l.double().sum(1), s_rows


_CACHE: dict = {}


def case(B: int, N: int, dtype: int, header, s: float, thr, sum_classes: bool, grad_scale: float):
    """the float64 reference of one launch, computed once and shared"""
    key = (B, N, dtype, header, s, thr, sum_classes, grad_scale)
    if key not in _CACHE:
        x, y = logits(B, N, dtype), labels(B, N)
        t = target(y, N, header, s, thr)
        loss, grad, s_loss, s_grad, rows, s_rows = bce(x.double(), t, grad_scale, sum_classes)
        # (a row term is the kernel's double before the division and the f32 store: K_LOSS covers it with one to spare)
        _CACHE[key] = dict(x=x, y=y, t=t, loss=loss.item(), grad=grad, loss_bound=K_LOSS * U * s_loss.item(),
                           rows=rows, row_bounds=K_LOSS * U * s_rows,
                           grad_bound=K_GRAD * U * s_grad + TINY + (BF16_U * grad.abs() if dtype == BF16 else 0.0),
                           grad_f32_part=K_GRAD * U * s_grad)
    return _CACHE[key]


def combos():
    for header in HEADERS:
        for s in SMOOTHING:
            for thr in THRESHOLDS:
                for sum_classes in (False, True):
                    yield header, s, thr, sum_classes


# ---- three training steps of the fused trainer, restated ---------------------------------------------------------------
STEP_MODEL, STEP_CLASSES, STEP_BATCH, STEP_SIZE = "darknet_yolov5n", 16, 4, 64
STEP_SMOOTHING, STEP_WD = 0.1, 1e-3
STEP_MIX = [("mixup", 0.3, (0, 0, 0, 0)), ("cutmix", 1 - 20 * 12 / (64 * 64), (10, 30, 30, 42)), ("mixup", 0.6, (0, 0, 0, 0))]
# the loss tolerance of the step tests of tests/test_resnet_gpu.py, and the learning rates at which the restatement's own
# float32 run stays within a tenth of it (tests/test_bce_cpu.py checks that; the rule of NOTEBOOK 23.3)
STEP_RTOL = 1e-2
STEP_LR = {"SGD": 1e-2, "Lamb": 1.5e-3}
LAMB_EPS = 1e-6


def step_inputs():
    return filler.images(STEP_BATCH, STEP_SIZE), filler.labels(STEP_BATCH, STEP_CLASSES)


def step_state(dtype=torch.float64, prefix="bce."):
    sd = {}
    for k, shape in R.classifier_spec(STEP_MODEL, STEP_CLASSES).items():
        dt = torch.int64 if k.endswith("num_batches_tracked") else torch.float32
        v = filler.fill_tensor(prefix + k, torch.zeros(shape, dtype=dt))
        sd[k] = v.to(dtype) if v.is_floating_point() else v
    return sd


def soft_loss(logits_: torch.Tensor, mixed_onehot: torch.Tensor, s: float, thr=None, sum_classes=False) -> torch.Tensor:
    """the batch loss of the definition on an explicit mixed one-hot (autograd goes through it)"""
    B, N = logits_.shape
    t = (1 - f32r(s)) * mixed_onehot + f32r(s) / N
    if thr is not None:
        t = (t > f32r(thr)).to(logits_.dtype)
    l = F.binary_cross_entropy_with_logits(logits_, t, reduction="none")
    return l.sum() / (B if sum_classes else B * N)


def ref_steps(optimizer: str, dtype=torch.float64, lr=None, steps: int = 3):
    """losses of `steps` training steps of nn.Sequential(backbone, pool, flatten, linear) under loss="bce" with the mix
    blocks of STEP_MIX: SGD(momentum 0.9) over the three weight-decay groups, or LAMB (tests/lamb_util.py)"""
    key = ("steps", optimizer, dtype, lr, steps)
    if key in _CACHE:
        return _CACHE[key]
    import lamb_util as LU

    lr = STEP_LR[optimizer] if lr is None else lr
    x, y = step_inputs()
    sd = step_state(dtype)
    params = {k: v for k, v in sd.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    for v in params.values():
        v.requires_grad_(True)
    names = list(params)
    wds = [R.weight_decay_group(k, STEP_WD, 0.0, 0.0) for k in names]
    mom, lamb, losses = {}, None, []
    for i in range(steps):
        for v in params.values():
            v.grad = None
        mode, lam, box = STEP_MIX[i % len(STEP_MIX)]
        xb, tb = R.mix_batch(x.to(dtype), y, STEP_CLASSES, mode, f32r(lam), box)
        loss = soft_loss(R.classifier_logits(STEP_MODEL, sd, xb, True), tb, STEP_SMOOTHING)
        loss.backward()
        losses.append(loss.item())
        if optimizer == "SGD":
            R.sgd_step(params, {k: v.grad for k, v in params.items()}, mom, lr, 0.9, lambda k: wds[names.index(k)])
        else:
            if lamb is None:
                lamb = LU.Lamb([params[k].detach() for k in names], wds, lr, eps=LAMB_EPS, M=1.0)
            lamb.step([params[k].grad for k in names])
            with torch.no_grad():
                for k, p in zip(names, lamb.p):
                    params[k].copy_(p)
    _CACHE[key] = losses
    return losses


def margin_ok(N: int, header, s: float, thr) -> bool:
    if thr is None:
        return True
    lam = f32r(header[1]) if header is not None and header[0] != 0 else 1.0
    return all(abs(v - f32r(thr)) > THR_MARGIN for v in target_values(N, lam, f32r(s)))


assert all(math.isfinite(v) for v in SPECIALS)
