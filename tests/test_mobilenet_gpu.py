"""MobileNetExtractor on the GPU against the float64 restatement of torchvision's MobileNets (tests/mobilenet_util.py): all
five feature maps and every parameter gradient, train and eval mode, f32 and bf16, for mobilenet_v2, mobilenet_v3_large and
mobilenet_v3_small; a frozen bn.eval() inside a training model; the FPN / PAN necks over the five maps of v2; the fused train
step (SGD, AdamW, deterministic mode); refusals.

Method and bounds are those of tests/test_regnet_gpu.py (which are those of tests/test_resnet_gpu.py).  f32: maps within
1e-3; gradient norms with a median within 5e-3 (train) / 1e-4 (eval) and a worst parameter within 0.1 / 5e-2, and EVERY
gradient tensor within that worst bound (relative to its own norm, or to 1e-6 of the largest gradient norm where its own is
smaller: the floor the norm check of that file uses; a MobileNet has parameters whose gradient is exactly zero).  bf16: the
restatement runs in float64 with bf16 rounding where the GPU path rounds (`_Bf16Emulation`: the image, the filters, the stored z and y of every unit, the pooled row, hidden values, gate logits and
gated map of a Squeeze-Excitation, the block output, and in backward every stored gradient); its error against the plain
float64 run is the format's own error on this model, and twice that, per quantity, is the bound.  Both errors are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import mobilenet_util as MU
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import necks
from vision_toolbox.backbones import MobileNetExtractor
from vision_toolbox.trainer import TrainStep

from gpu_util import rel_err

pytestmark = pytest.mark.gpu

B, S = 4, 64  # the last map is 2 x 2: BatchNorm over 16 samples per channel
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
    a stored y, the pooled row, the hidden values) and writes (the stored z, the gate logits), what a block and its
    Squeeze-Excitation write (the block output, the gated map), and the filters of the 1x1 and stem convolutions (the bf16
    mirror; the depthwise and Squeeze-Excitation filters are read as f32 masters and rounded by the kernels: the same values).
    _Round rounds the gradient on the way back."""

    def __init__(self, ref: nn.Module):
        self.ref = ref
        self.handles = []

    def __enter__(self):
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                self.handles.append(m.register_forward_pre_hook(lambda mod, a: (_Round.apply(a[0]),)))
                self.handles.append(m.register_forward_hook(lambda mod, a, out: _Round.apply(out)))
                m._w64 = m.weight.data.clone()
                m.weight.data = m.weight.data.to(torch.bfloat16).double()
            elif isinstance(m, (MU.RefBlock, MU.RefSE)):
                self.handles.append(m.register_forward_hook(lambda mod, a, out: _Round.apply(out)))
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = m._w64
                del m._w64


def _seeds(shapes):
    return [filler.tensor(f"mobilenet.dmap{i}", s) for i, s in enumerate(shapes)]


_REF_CACHE = {}


def _reference(name, training, frozen=False):
    """float64 maps and parameter gradients of the restatement, and the same with bf16 stores; once per (model, mode)"""
    key = (name, training, frozen)
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    ref, sd = MU.make_pair(name)
    x = filler.images(B, S)
    out = {"sd": MU.torchvision_layout(sd)}
    for emu in (False, True):
        r = copy.deepcopy(ref)
        r.train(training)
        if frozen:
            _freeze(r.features)
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


def _freeze(features):
    """bn.eval() on the depthwise unit of features.3 and the projection of features.5, inside a training model"""
    blk3, blk5 = features[3], features[5]
    list(getattr(blk3, "conv", None) or blk3.block)[1][1].eval()
    seq5 = getattr(blk5, "conv", None) or blk5.block
    (seq5[-1] if isinstance(seq5[-1], nn.BatchNorm2d) else seq5[-1][1]).eval()


def _model(name, sd, training, dtype):
    m = MobileNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.compute_dtype = dtype
    m = m.cuda()
    m.train(training)
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
    # (per tensor, against the same floor as the norms: the bias of every projection BatchNorm has a gradient of exactly zero
    #  here -- a per-channel constant added to a block's output is removed by the train-mode BatchNorm behind the next 1x1
    #  expansion -- so float64 leaves 1e-16 and f32 1e-8 of noise there, and a ratio of the two says nothing)
    floor = 1e-6 * want.max()
    errs = {k: (grads[k].double() - ref_grads[k]).norm().item() / max(ref_grads[k].norm().item(), floor) for k in keys}
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
    ratios = [got / max(floor, 1e-30) for _, got, floor in report]
    gk = [r for r in report if not r[0].startswith("map")]
    print(f"bf16 maps: emulation {min(r[2] for r in report[:5]):.2e} .. {max(r[2] for r in report[:5]):.2e}, "
          f"GPU {min(r[1] for r in report[:5]):.2e} .. {max(r[1] for r in report[:5]):.2e}; gradients min / median / max: emulation "
          f"{min(r[2] for r in gk):.3f} / {np.median([r[2] for r in gk]):.3f} / {max(r[2] for r in gk):.3f}, GPU "
          f"{min(r[1] for r in gk):.3f} / {np.median([r[1] for r in gk]):.3f} / {max(r[1] for r in gk):.3f}; worst quantity at "
          f"{max(ratios) / 2:.2f} of its bound")
    for k, got, floor in report:
        if not got < 2 * floor:
            bad.append((k, got, 2 * floor))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", MU.NAMES)
def test_maps_and_gradients_match_the_restatement(name, training, dtype):
    ref = _reference(name, training)
    maps, grads = _run(_model(name, ref["sd"], training, dtype))
    assert [t.shape[1] for t in maps] == list(MU.CHANNELS[name]) and [S // t.shape[2] for t in maps] == list(MU.STRIDES[name])
    if dtype == torch.float32:
        _check_f32(maps, grads, ref, training)
    else:
        _check_bf16(maps, grads, ref)


def test_a_frozen_batchnorm_inside_a_training_model():
    """bn.eval() on a depthwise unit and on a projection: running statistics in forward, constants in backward, untouched"""
    name = "mobilenet_v2"
    ref = _reference(name, True, frozen=True)
    m = _model(name, ref["sd"], True, torch.float32)
    _freeze(m.feat_extractor.features)
    frozen = m.feat_extractor.features[3].conv[1][1]
    before = frozen.running_mean.clone()
    maps, grads = _run(m)
    _check_f32(maps, grads, ref, True)
    assert torch.equal(frozen.running_mean, before) and int(frozen.num_batches_tracked) == 0
    assert int(m.feat_extractor.features[3].conv[0][1].num_batches_tracked) == 1


@pytest.mark.parametrize("neck", ["FPN", "PAN"])
def test_necks_take_the_five_maps(neck):
    ref = _reference("mobilenet_v2", False)
    m = _model("mobilenet_v2", ref["sd"], False, torch.float32)
    nk = getattr(necks, neck)(list(m.out_channels_list), 32)
    filler.fill_module(nk, "mobilenet.neck.")
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
    bias = [m.bias for m in model.modules() if isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None]
    other = [m.weight for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    return [{"params": norm, "weight_decay": 0.0}, {"params": bias, "weight_decay": 0.0}, {"params": other, "weight_decay": wd}]


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW"])
def test_train_steps_match_float64_losses(optimizer):
    """three steps of TrainStep(MobileNetExtractor("mobilenet_v3_large")) -- the reference's nn.Sequential(backbone,
    AdaptiveAvgPool2d, Flatten, Linear) -- in f32, batch 8 @96, against the float64 restatement under torch.optim: the losses
    within 1e-2, the first (forward only) within 1e-4.  The learning rates are where the RESTATEMENT ITSELF is
    well-conditioned: run in plain f32 torch on the CPU it stays within 2.4e-6 (SGD, 2e-4: 1.2e-9 / 1.1e-6 / 2.4e-6 per step)
    and 5.5e-6 (AdamW, 1e-4: 1.2e-9 / 5.5e-6 / 3.9e-6) of its own float64 losses over the three steps, far below a tenth of
    the bound (1e-3); the float64 losses there are 2.936 / 2.915 / 2.877 and 2.936 / 2.468 / 2.071."""
    ncls, Bt, St = 16, 8, 96
    lr, wd = (2e-4, 1e-3) if optimizer == "SGD" else (1e-4, 0.05)
    x, y = filler.images(Bt, St), filler.labels(Bt, ncls)
    ts = TrainStep(MobileNetExtractor("mobilenet_v3_large"), ncls, Bt, St, torch.float32, lr=lr, momentum=0.9, weight_decay=wd,
                   label_smoothing=0.1, device="cuda", optimizer=optimizer)
    ref, sd = MU.make_pair("mobilenet_v3_large", prefix="mobilenet.ts.", num_classes=ncls)
    ref = ref.train()
    ts.model[0].load_torchvision_ckpt(MU.torchvision_layout(sd))
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
@pytest.mark.parametrize("name", ["mobilenet_v2", "mobilenet_v3_small"])
def test_deterministic_steps_are_bit_identical(name, dtype):
    """two fresh runs of three deterministic steps end in the same bits: the depthwise filter gradients are shares added in a
    fixed order, and the hardsigmoid gate's d(s) is summed in fixed point by one workgroup per (image, column group)"""
    x, y = filler.images(4, S).cuda(), filler.labels(4, 10).cuda()
    states = []
    for _ in range(2):
        ts = TrainStep(MobileNetExtractor(name), 10, 4, S, dtype, lr=0.01, device="cuda", deterministic=True)
        filler.fill_module(ts.model, "mobilenet.det.")
        ts.weights_changed()
        losses = []
        for _ in range(3):
            ts.step(x, y)
            losses.append(ts.loss())
        torch.cuda.synchronize()
        states.append((losses, ts.store.pflat.clone(), ts.gflat.clone(), ts.mflat.clone(), ts.store.sflat.clone()))
        del ts
    # parameters, gradients, momentum and BatchNorm state.  (The loss SCALAR a step reports is summed over the batch with a
    # float atomic in vt_softmax_xent and may differ in its last bit; nothing reads it.)
    for a, b in zip(states[0][1:], states[1][1:]):
        assert torch.equal(a, b)
    assert states[0][0] == pytest.approx(states[1][0], rel=1e-6) and all(l == l for l in states[0][0])


def test_refusals_by_name():
    m = MobileNetExtractor("mobilenet_v2").cuda()
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m(torch.rand(2, 3, 64, 64, device="cuda", requires_grad=True))
    with pytest.raises(NotImplementedError, match="pretrained"):
        MobileNetExtractor("mobilenet_v3_large", pretrained=True)
    with pytest.raises(ValueError, match="mobilenet_v1"):
        MobileNetExtractor("mobilenet_v1")
