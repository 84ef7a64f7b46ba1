"""ResNetExtractor on the GPU against the float64 restatement of torchvision's ResNet (tests/resnet_util.py): all five
feature maps and every parameter gradient, train and eval mode, f32 and bf16; a frozen bn.eval() inside a training model;
wide_resnet50_2; the FPN / PAN necks over the five maps; the fused train step (SGD, AdamW, deterministic mode); refusals.

Bounds.  f32: what tests/test_modules_gpu.py applies to the Darknet / VoVNet models -- maps within 1e-3; gradient norms
with a median within 5e-3 (train: batch statistics over 16 samples per channel in layer4 are ill-conditioned in ANY f32
implementation) / 1e-4 (eval) and a worst parameter within 0.1 / 5e-2, and here EVERY gradient tensor within that worst
bound.  bf16: not fixed in advance.  The restatement runs on the CPU in float64 with bf16 rounding where the GPU path
rounds (`_Bf16Emulation`: image, filters, every stored z and y, and in backward every stored dz and d(y)); its error against
the plain float64 run on the same inputs is the format's own error on this model, and twice that, per quantity, is the
bound -- the factor covers summation-order differences between the CPU and MFMA accumulation.  Measured on an MI355X (emulated
error, hence bound = 2 x; then the GPU path's error; relative L2; NOTEBOOK.md 22.3):
    resnet18 train  maps 4.7e-3 .. 4.5e-2 (GPU 4.7e-3 .. 4.7e-2), gradients 0.107 / 0.286 / 0.363 min / median / max (GPU 0.108 / 0.276 / 0.350)
    resnet18 eval   maps 3.1e-3 .. 8.2e-3 (GPU 3.1e-3 .. 8.1e-3), gradients 0.056 / 0.102 / 0.172 (GPU 0.067 / 0.113 / 0.180)
    resnet50 train  maps 4.7e-3 .. 0.57   (GPU 4.7e-3 .. 0.57),   gradients 0.56 / 1.24 / 1.44 (GPU 0.56 / 1.22 / 1.51)
    resnet50 eval   maps 3.1e-3 .. 1.1e-2 (GPU 3.1e-3 .. 1.1e-2), gradients 0.038 / 0.255 / 0.478 (GPU 0.051 / 0.246 / 0.514)
the worst quantity at 0.62 / 0.68 / 0.54 / 0.70 of its bound.  (bf16 train-mode gradients at this size are noise in any
implementation: those cases show the GPU path is no worse than the format; the f32 cases check the gradients.)"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import resnet_util
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import necks
from vision_toolbox.backbones import ResNetExtractor
from vision_toolbox.trainer import TrainStep

from gpu_util import rel_err

pytestmark = pytest.mark.gpu

B, S = 4, 64  # layer4 is 2 x 2: BatchNorm over 16 samples per channel
F32_MAPS, F32_GRAD = 1e-3, {True: (5e-3, 0.1), False: (1e-4, 5e-2)}  # (median of the norms, worst) by training


class _Round(torch.autograd.Function):
    """a bf16 store: the value is rounded going forward, its gradient going backward"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _Bf16Emulation:
    """float64 arithmetic with the GPU path's bf16 stores, as hooks on the restatement: what a convolution reads (the image,
    a stored y) and writes (the stored z), what a block and its downsample branch write (the stored y that is the next
    identity), and the filters (the bf16 mirror).  _Round rounds the gradient on the way back: the stored dz and d(y)."""

    def __init__(self, ref: nn.Module):
        self.ref = ref
        self.handles = []

    def __enter__(self):
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                self.handles.append(m.register_forward_pre_hook(lambda mod, a: (_Round.apply(a[0]),)))  # the stored y it reads
                self.handles.append(m.register_forward_hook(lambda mod, a, out: _Round.apply(out)))  # the stored z
                m._w64 = m.weight.data.clone()
                m.weight.data = m.weight.data.to(torch.bfloat16).double()  # the mirror
            elif isinstance(m, resnet_util.RefBlock):
                self.handles.append(m.register_forward_hook(lambda mod, a, out: _Round.apply(out)))
                if m.downsample is not None:
                    self.handles.append(m.downsample.register_forward_hook(lambda mod, a, out: _Round.apply(out)))
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = m._w64
                del m._w64


def _seeds(shapes):
    return [filler.tensor(f"resnet.dmap{i}", s) for i, s in enumerate(shapes)]


_REF_CACHE = {}


def _reference(name, training, frozen=()):
    """float64 maps and parameter gradients of the restatement, and the same with bf16 stores; once per (model, mode)"""
    key = (name, training, tuple(frozen))
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    ref, sd = resnet_util.make_pair(name)
    x = filler.images(B, S)
    out = {"sd": sd}
    for emu in (False, True):
        r = copy.deepcopy(ref)
        r.train(training)
        for mod_name in frozen:
            r.get_submodule(mod_name).eval()
        if emu:
            with _Bf16Emulation(r):
                maps = [_Round.apply(m) for m in r.maps(x.double())]
                sum((m * g.double()).sum() for m, g in zip(maps, _seeds([m.shape for m in maps]))).backward()
        else:
            maps = r.maps(x.double())
            sum((m * g.double()).sum() for m, g in zip(maps, _seeds([m.shape for m in maps]))).backward()
        out["bf16" if emu else "f64"] = ([m.detach() for m in maps], {k: p.grad for k, p in r.named_parameters() if not k.startswith("fc.")})
    _REF_CACHE[key] = out
    return out


def _model(name, sd, training, dtype, frozen=()):
    m = ResNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.compute_dtype = dtype
    m = m.cuda()
    m.train(training)
    for mod_name in frozen:
        m.feat_extractor.get_submodule(mod_name).eval()
    return m


def _run(m, need_grad=True):
    x = filler.images(B, S).cuda()
    before = N.launch_count()
    with torch.set_grad_enabled(need_grad):
        maps = m.get_feature_maps(x)
    if need_grad:
        seeds = _seeds([t.shape for t in maps])
        torch.autograd.backward(maps, [g.cuda().to(t.dtype) for g, t in zip(seeds, maps)])
    torch.cuda.synchronize()
    assert N.launch_count() > before, "the HIP path did not run"
    grads = {k[len("feat_extractor."):]: p.grad.float().cpu() for k, p in m.named_parameters()} if need_grad else {}
    return [t.detach().float().cpu() for t in maps], grads


def _check_f32(maps, grads, ref, training):
    ref_maps, ref_grads = ref["f64"]
    for i, (g, w) in enumerate(zip(maps, ref_maps)):
        assert g.shape == w.shape
        e = rel_err(g, w)
        print(f"f32 map{i}: {e:.3e}")
        assert e < F32_MAPS, f"map{i}"
    assert set(grads) == set(ref_grads)
    med_bound, worst_bound = F32_GRAD[training]
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


def _check_bf16(maps, grads, ref):
    """every quantity within twice the error of the bf16-emulated restatement against float64"""
    ref_maps, ref_grads = ref["f64"]
    emu_maps, emu_grads = ref["bf16"]
    report, bad = [], []
    for i, (g, w, e) in enumerate(zip(maps, ref_maps, emu_maps)):
        report.append((f"map{i}", rel_err(g, w), rel_err(e, w)))
    for k in ref_grads:
        report.append((k, rel_err(grads[k], ref_grads[k]), rel_err(emu_grads[k], ref_grads[k])))
    for k, got, floor in report:
        print(f"bf16 {k}: {got:.3e} (emulation {floor:.3e}, bound {2 * floor:.3e})")
        if not got < 2 * floor:
            bad.append((k, got, 2 * floor))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_maps_and_gradients_match_the_restatement(name, training, dtype):
    ref = _reference(name, training)
    maps, grads = _run(_model(name, ref["sd"], training, dtype))
    assert [t.shape[1] for t in maps] == list(ResNetExtractor(name).out_channels_list) and maps[-1].shape[2:] == (2, 2)
    if dtype == torch.float32:
        _check_f32(maps, grads, ref, training)
    else:
        _check_bf16(maps, grads, ref)


def test_frozen_batchnorm_inside_a_training_model():
    """layer3's BatchNorms in eval mode inside a training model: they normalise with their running statistics, leave them
    untouched, and their block ends take the ready-coefficient form of the add-then-ReLU pass"""
    frozen = ["layer3.0.bn1", "layer3.0.bn2", "layer3.0.downsample.1", "layer3.1.bn1", "layer3.1.bn2"]
    ref = _reference("resnet18", True, frozen)
    m = _model("resnet18", ref["sd"], True, torch.float32, frozen)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    maps, grads = _run(m)
    _check_f32(maps, grads, ref, True)
    after = m.state_dict()
    for k in before:
        moved = not torch.equal(before[k], after[k])
        if "running" in k or "num_batches" in k:
            assert moved == (not k.startswith("feat_extractor.layer3.")), k


def test_wide_resnet50_2_forward():
    ref, sd = resnet_util.make_pair("wide_resnet50_2")
    ref.eval()
    x = filler.images(2, S)
    with torch.no_grad():
        want = ref.maps(x.double())
        m = _model("wide_resnet50_2", sd, False, torch.float32)
        got = m.get_feature_maps(x.cuda())
    assert [t.shape[1] for t in got] == [64, 256, 512, 1024, 2048]
    for i, (g, w) in enumerate(zip(got, want)):
        assert rel_err(g.float().cpu(), w) < F32_MAPS, i


@pytest.mark.parametrize("neck", ["FPN", "PAN"])
def test_necks_take_the_five_maps(neck):
    ref = _reference("resnet18", False)
    m = _model("resnet18", ref["sd"], False, torch.float32)
    nk = getattr(necks, neck)(list(m.out_channels_list), 32)
    filler.fill_module(nk, "resnet.neck.")
    nk.eval()
    eager = copy.deepcopy(nk)
    with torch.no_grad():
        maps = m.get_feature_maps(filler.images(2, S).cuda())
        want = eager([t.float().cpu() for t in maps])  # CPU tensors: the eager neck, on the same maps
        got = nk.cuda()(maps)
    assert len(got) == 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and rel_err(g.float().cpu(), w) < F32_MAPS, i


# ---- the fused train step ------------------------------------------------------------------------------------------------
def _groups(model, wd):
    norm = [p for m in model.modules() if isinstance(m, nn.BatchNorm2d) for p in m.parameters(recurse=False)]
    bias = [m.bias for m in model.modules() if isinstance(m, nn.Linear)]
    other = [m.weight for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    return [{"params": norm, "weight_decay": 0.0}, {"params": bias, "weight_decay": 0.0}, {"params": other, "weight_decay": wd}]


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW"])
def test_train_steps_match_float64_losses(optimizer):
    """three steps of TrainStep(ResNetExtractor("resnet18")) -- the reference's nn.Sequential(backbone, AdaptiveAvgPool2d,
    Flatten, Linear) -- in f32 against the float64 restatement under torch.optim: the losses within 1e-2, the bound
    tests/test_trainer_gpu.py sets for a well-conditioned model at this size (small learning rates, as there)"""
    ncls, Bt, St = 16, 8, 96
    lr, wd = (2e-4, 1e-3) if optimizer == "SGD" else (1e-4, 0.05)
    x, y = filler.images(Bt, St), filler.labels(Bt, ncls)
    ts = TrainStep(ResNetExtractor("resnet18"), ncls, Bt, St, torch.float32, lr=lr, momentum=0.9, weight_decay=wd,
                   label_smoothing=0.1, device="cuda", optimizer=optimizer)
    ref = resnet_util.RefResNet("resnet18", ncls)
    sd = filler.fill_state_dict(ref.state_dict(), "resnet.ts.")
    for k, v in sd.items():
        if v.dim() == 1 and k.endswith(".weight"):
            v += 1.0
    ref.load_state_dict(sd)
    ref = ref.double().train()
    ts.model[0].load_torchvision_ckpt(sd)
    with torch.no_grad():
        ts.model[3].weight.copy_(sd["fc.weight"])
        ts.model[3].bias.copy_(sd["fc.bias"])
    ts.weights_changed()
    opt = (torch.optim.SGD(_groups(ref, wd), lr=lr, momentum=0.9) if optimizer == "SGD"
           else torch.optim.AdamW(_groups(ref, wd), lr=lr, weight_decay=wd))
    got, want = [], []
    for _ in range(3):
        ts.step(x.cuda(), y.cuda())
        got.append(ts.loss())
        opt.zero_grad()
        loss = F.cross_entropy(ref(x.double()), y, label_smoothing=0.1)
        loss.backward()
        opt.step()
        want.append(loss.item())
    print(optimizer, got, want)
    np.testing.assert_allclose(got, want, rtol=1e-2)
    assert got[0] == pytest.approx(want[0], rel=1e-4)  # the first loss: forward only


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_steps_are_bit_identical(dtype):
    """two fresh runs of three deterministic steps end in the same bits"""
    x, y = filler.images(4, S).cuda(), filler.labels(4, 10).cuda()
    states = []
    for _ in range(2):
        ts = TrainStep(ResNetExtractor("resnet18"), 10, 4, S, dtype, lr=0.01, device="cuda", deterministic=True)
        filler.fill_module(ts.model, "resnet.det.")
        ts.weights_changed()
        losses = []
        for _ in range(3):
            ts.step(x, y)
            losses.append(ts.loss())
        torch.cuda.synchronize()
        states.append((losses, ts.store.pflat.clone(), ts.gflat.clone(), ts.mflat.clone(), ts.store.sflat.clone()))
        del ts
    # parameters, gradients, momentum and BatchNorm state: what tools/deterministic_check.py compares.  (The loss SCALAR a step
    # reports is summed over the batch with a float atomic in vt_softmax_xent and may differ in its last bit; nothing reads it.)
    for a, b in zip(states[0][1:], states[1][1:]):
        assert torch.equal(a, b)
    assert states[0][0] == pytest.approx(states[1][0], rel=1e-6) and all(l == l for l in states[0][0])


def test_refusals_by_name():
    m = ResNetExtractor("resnet18").cuda()
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m(torch.rand(2, 3, 64, 64, device="cuda", requires_grad=True))
    with pytest.raises(NotImplementedError, match="resnext50_32x4d"):
        ResNetExtractor("resnext50_32x4d").cuda()(torch.rand(2, 3, 64, 64, device="cuda"))
    with pytest.raises(NotImplementedError, match="pretrained"):
        ResNetExtractor("resnet50", pretrained=True)
