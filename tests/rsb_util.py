"""TEST INFRASTRUCTURE -- stochastic depth on the float64 ResNet restatement of tests/resnet_util.py, with the keep factors as an
ARGUMENT (nothing is drawn here), and the float64 statement of one add-then-ReLU unit with keep factors for the kernel tests.

The definition is timm's ResNet: block i of n in network order has p_i = stochastic_depth * i / (n - 1); in training mode
a block with p_i > 0 is y = relu(keep[b] * bn(conv(h)) + identity), keep[b] = 0 or 1 / (1 - p_i) per image -- the drop behind
the last BatchNorm, in front of the shortcut, downsample blocks included.  resnet_util.py is wrapped, not changed: the blocks
of a RefResNet are run from here, with the factor where the table has a row."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import resnet_util

EPS, MOM = 1e-5, 0.1


def rates(name: str, stochastic_depth: float) -> "list[float]":
    n = sum(resnet_util.CONFIGS[name][1])
    return [stochastic_depth * i / (n - 1) for i in range(n)]


def blocks(ref: resnet_util.RefResNet):
    return [blk for li in range(1, 5) for blk in getattr(ref, f"layer{li}")]


def block_forward(blk: resnet_util.RefBlock, x: torch.Tensor, keep=None) -> torch.Tensor:
    skip = x if blk.downsample is None else blk.downsample(x)
    for i in range(1, blk.n + 1):
        x = getattr(blk, f"bn{i}")(getattr(blk, f"conv{i}")(x))
        if i < blk.n:
            x = F.relu(x)
    if keep is not None:
        x = x * keep.to(x.dtype).view(-1, 1, 1, 1)
    return F.relu(x + skip)


def maps(ref: resnet_util.RefResNet, x: torch.Tensor, ps, table=None, store=None):
    """the five maps with the rows of `table` (float[n_sites][B]) on the blocks whose rate in `ps` is positive, in order.
    table=None: no block drops (eval mode).  `store`: applied to every block output and to the stem map (the bf16-store
    emulation of the model tests; None: nothing)."""
    st = store if store is not None else (lambda t: t)
    out = [st(F.relu(ref.bn1(ref.conv1(x))))]
    h = F.max_pool2d(out[0], 3, 2, 1)
    row, k = 0, 0
    for li in range(1, 5):
        for blk in getattr(ref, f"layer{li}"):
            keep = None
            if table is not None and ps[k] > 0:
                keep, row = table[row], row + 1
            h = st(block_forward(blk, h, keep))
            k += 1
        out.append(h)
    assert table is None or row == table.shape[0]
    return out


def logits(ref: resnet_util.RefResNet, x, ps, table=None):
    return ref.fc(torch.flatten(F.adaptive_avg_pool2d(maps(ref, x, ps, table)[-1], 1), 1))


# ---- one unit y = relu(keep[b] * bn(z) + r) over [M = B * HW][C] rows, float64 ------------------------------------------------
def unit_reference(z, r, gamma, beta, dy, rm, rv, keep, HW: int, train: int, y_mask=None):
    """y, (scale, shift, mean, invstd) as f32, and the gradients of z, r, gamma, beta.  `y_mask`: the stored y the kernels
    read their mask from (None: the reference's own)."""
    M, Cc = z.shape
    kf = keep.double().repeat_interleave(HW).view(M, 1)
    zd, rd = z.double().requires_grad_(True), r.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    x4 = zd.t().reshape(1, Cc, -1, 1)
    bn = F.batch_norm(x4, rm.double().clone(), rv.double().clone(), g, b, bool(train), MOM, EPS).reshape(Cc, -1).t()
    pre = kf * bn + rd
    y = torch.relu(pre)
    if y_mask is None:
        y.backward(dy.double())
    else:  # the mask of the stored y, as the kernels take it
        pre.backward(dy.double() * (y_mask.double() > 0))
    if train:
        mean, var = z.double().mean(0), z.double().var(0, unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    coefs = torch.stack([scale, beta.double() - mean * scale, mean, invstd]).float()
    return y.detach(), coefs, zd.grad, rd.grad, g.grad, b.grad


# ---- keep tables with fixed entries ----------------------------------------------------------------------------------------
def table(ps, B: int, shift: int = 0) -> torch.Tensor:
    """float[n_sites][B]: every second site (row + shift even) drops one image, image (row + shift) / 2 mod B -- with 2 B sites
    or more every image is dropped somewhere, none everywhere -- and the kept images carry 1 / (1 - p)"""
    sites = [p for p in ps if p > 0]
    t = torch.zeros(len(sites), B)
    for row, p in enumerate(sites):
        t[row] = 1.0 / (1.0 - p)
        if (row + shift) % 2 == 0:
            t[row, ((row + shift) // 2) % B] = 0.0
    return t


# ---- three training steps of the fused trainer with the recipe's pieces, restated ---------------------------------------
STEP_MODEL, STEP_CLASSES, STEP_BATCH, STEP_SIZE = "resnet18", 16, 4, 64
STEP_SD, STEP_SMOOTHING, STEP_WD = 0.05, 0.1, 1e-3
STEP_RTOL = 1e-2   # the loss tolerance of the step tests of tests/test_resnet_gpu.py
# the learning rates at which the restatement's own float32 run stays within a tenth of it (tests/test_rsb_cpu.py)
STEP_LR = {"SGD": 2e-3, "Lamb": 5e-4}
LAMB_EPS = 1e-6
_STEPS: dict = {}


def step_state():
    """the filled torchvision-layout state_dict of the step tests (BatchNorm scales centred at 1)"""
    from oracle import filler

    ref = resnet_util.RefResNet(STEP_MODEL, STEP_CLASSES)
    sd = filler.fill_state_dict(ref.state_dict(), "rsb.ts.")
    for k, v in sd.items():
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    return sd


def ref_steps(optimizer: str, dtype=torch.float64, lr=None, steps: int = 3):
    """losses of `steps` steps of loss="bce" on the ResNet with stochastic depth, a different keep table per step"""
    key = (optimizer, dtype, lr, steps)
    if key in _STEPS:
        return _STEPS[key]
    import bce_util as BU
    import lamb_util as LU
    from oracle import filler
    from torch import nn

    lr = STEP_LR[optimizer] if lr is None else lr
    x, y = filler.images(STEP_BATCH, STEP_SIZE).to(dtype), filler.labels(STEP_BATCH, STEP_CLASSES)
    ref = resnet_util.RefResNet(STEP_MODEL, STEP_CLASSES)
    ref.load_state_dict(step_state())
    ref = ref.to(dtype).train()
    ps = rates(STEP_MODEL, STEP_SD)
    norm = [p for m in ref.modules() if isinstance(m, nn.BatchNorm2d) for p in m.parameters(recurse=False)]
    bias = [m.bias for m in ref.modules() if isinstance(m, nn.Linear)]
    other = [m.weight for m in ref.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    params = norm + bias + other
    wds = [0.0] * (len(norm) + len(bias)) + [STEP_WD] * len(other)
    opt = lamb = None
    if optimizer == "SGD":
        opt = torch.optim.SGD([{"params": norm + bias, "weight_decay": 0.0}, {"params": other, "weight_decay": STEP_WD}], lr=lr,
                              momentum=0.9)
    losses = []
    onehot = F.one_hot(y, STEP_CLASSES).to(dtype)
    for i in range(steps):
        for p in params:
            p.grad = None
        loss = BU.soft_loss(logits(ref, x, ps, table(ps, STEP_BATCH, i).to(dtype)), onehot, STEP_SMOOTHING)
        loss.backward()
        losses.append(loss.item())
        if opt is not None:
            opt.step()
        else:
            if lamb is None:
                lamb = LU.Lamb([p.detach() for p in params], wds, lr, eps=LAMB_EPS, M=1.0)
            lamb.step([p.grad for p in params])
            with torch.no_grad():
                for p, q in zip(params, lamb.p):
                    p.copy_(q)
    _STEPS[key] = losses
    return losses


# ---- the model-level checks of tests/test_resnet_gpu.py, restated for runs with a keep table -----------------------------------
# (the same bounds and the same bf16-store emulation; kept here so that the stochastic-depth tests import no other test module)
MODEL_B, MODEL_S = 4, 64  # layer4 is 2 x 2: BatchNorm over 16 samples per channel
F32_MAPS, F32_GRAD_TRAIN = 1e-3, (5e-3, 0.1)  # maps; (median of the gradient norms, worst tensor) in training mode


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Round(torch.autograd.Function):
    """a bf16 store: the value is rounded going forward, its gradient going backward"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class Bf16Emulation:
    """float64 arithmetic with the GPU path's bf16 stores, as hooks on the restatement: what a convolution reads and writes
    (the stored y and z), what a downsample branch writes, and the filters (the bf16 mirror).  A block's own output is
    rounded by `maps(..., store=Round.apply)`, which runs the blocks."""

    def __init__(self, ref):
        self.ref, self.handles = ref, []

    def __enter__(self):
        from torch import nn

        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                self.handles.append(m.register_forward_pre_hook(lambda mod, a: (Round.apply(a[0]),)))
                self.handles.append(m.register_forward_hook(lambda mod, a, out: Round.apply(out)))
                m._w64 = m.weight.data.clone()
                m.weight.data = m.weight.data.to(torch.bfloat16).double()
            elif isinstance(m, resnet_util.RefBlock) and m.downsample is not None:
                self.handles.append(m.downsample.register_forward_hook(lambda mod, a, out: Round.apply(out)))
        return self

    def __exit__(self, *exc):
        from torch import nn

        for h in self.handles:
            h.remove()
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = m._w64
                del m._w64


def seeds(shapes):
    from oracle import filler

    return [filler.tensor(f"resnet.dmap{i}", s) for i, s in enumerate(shapes)]


def run_model(m):
    """the five maps and every parameter gradient of an extractor on the GPU, from the seeds above"""
    from oracle import filler
    from vision_toolbox import _native as N

    x = filler.images(MODEL_B, MODEL_S).cuda()
    before = N.launch_count()
    got = m.get_feature_maps(x)
    torch.autograd.backward(got, [g.cuda().to(t.dtype) for g, t in zip(seeds([t.shape for t in got]), got)])
    torch.cuda.synchronize()
    assert N.launch_count() > before, "the HIP path did not run"
    grads = {k[len("feat_extractor."):]: p.grad.float().cpu() for k, p in m.named_parameters()}
    return [t.detach().float().cpu() for t in got], grads


def check_f32(got_maps, grads, ref):
    import numpy as np

    ref_maps, ref_grads = ref["f64"]
    for i, (g, w) in enumerate(zip(got_maps, ref_maps)):
        assert g.shape == w.shape
        e = rel_err(g, w)
        print(f"f32 map{i}: {e:.3e}")
        assert e < F32_MAPS, f"map{i}"
    assert set(grads) == set(ref_grads)
    med_bound, worst_bound = F32_GRAD_TRAIN
    keys = list(ref_grads)
    got = np.array([grads[k].double().norm().item() for k in keys])
    want = np.array([ref_grads[k].norm().item() for k in keys])
    rel = np.abs(got - want) / np.maximum(want, 1e-6 * want.max())
    errs = {k: rel_err(grads[k], ref_grads[k]) for k in keys}
    worst = max(errs, key=errs.get)
    print(f"f32 gradient norms: median {np.median(rel):.3e}, max {rel.max():.3e}; worst tensor {worst} {errs[worst]:.3e}")
    assert np.median(rel) < med_bound and rel.max() < worst_bound
    for k in keys:
        assert errs[k] < worst_bound, k


def check_bf16(got_maps, grads, ref):
    """every quantity within twice the error of the bf16-emulated restatement against float64"""
    ref_maps, ref_grads = ref["f64"]
    emu_maps, emu_grads = ref["bf16"]
    report, bad = [], []
    for i, (g, w, e) in enumerate(zip(got_maps, ref_maps, emu_maps)):
        report.append((f"map{i}", rel_err(g, w), rel_err(e, w)))
    for k in ref_grads:
        report.append((k, rel_err(grads[k], ref_grads[k]), rel_err(emu_grads[k], ref_grads[k])))
    for k, got, floor in report:
        print(f"bf16 {k}: {got:.3e} (emulation {floor:.3e}, bound {2 * floor:.3e})")
        if not got < 2 * floor:
            bad.append((k, got, 2 * floor))
    assert not bad, bad
