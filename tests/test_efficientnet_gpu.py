"""EfficientNetExtractor on the GPU against the float64 restatement of torchvision's EfficientNets (tests/efficientnet_util.py):
all five feature maps and every parameter gradient of efficientnet_b0 with a SET keep table (stochastic depth in training mode;
eval mode ignores it), f32 and bf16; the same model drawing its own tables; efficientnet_v2_s (both FusedMBConv closings); a
frozen bn.eval() inside a training model; the FPN / PAN necks; the fused train step (SGD, AdamW, a different keep table per
step, deterministic mode, captured graphs); refusals.

The keep table of tests/efficientnet_util.keep_table drops one image at every site and a second one at every third site, keeps
the last image everywhere, and gives kept images 1 / (1 - p).

Method and bounds are those of tests/test_mobilenet_gpu.py.  f32: maps within 1e-3; gradient norms with a median within 5e-3
(train) / 1e-4 (eval) and a worst parameter within 0.1 / 5e-2, and EVERY gradient tensor within that worst bound (relative to
its own norm, or to 1e-6 of the largest gradient norm where its own is smaller).  bf16: the restatement runs in float64 with
bf16 rounding where the GPU path rounds (`_Bf16Emulation`: the image, the filters, the stored z and y of every unit, the pooled
row, hidden values, gate logits and gated map of a Squeeze-Excitation, the block output, and in backward every stored
gradient); its error against the plain float64 run is the format's own error on this model, and twice that, per quantity, is
the bound.  Both errors are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import efficientnet_util as EU
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import necks
from vision_toolbox.backbones import EfficientNetExtractor
from vision_toolbox.trainer import TrainStep

from gpu_util import rel_err

pytestmark = pytest.mark.gpu

S = 64  # the last map is 2 x 2
BATCH = {"efficientnet_b0": 4, "efficientnet_v2_s": 2}
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
    a stored y, the pooled row, the hidden values) and writes (the stored z, the gate logits), what a Squeeze-Excitation reads
    and writes (the stored y, the gated map), the block output, and the filters (the bf16 mirror; the depthwise and
    Squeeze-Excitation filters are read as f32 masters and rounded by the kernels: the same values)."""

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
            elif isinstance(m, EU.RefSE):
                self.handles.append(m.register_forward_pre_hook(lambda mod, a: (_Round.apply(a[0]),)))
                self.handles.append(m.register_forward_hook(lambda mod, a, out: _Round.apply(out)))
            elif isinstance(m, EU.RefBlock):
                m.out = _Round.apply
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        for m in self.ref.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = m._w64
                del m._w64
            elif isinstance(m, EU.RefBlock):
                del m.out


def _seeds(shapes):
    return [filler.tensor(f"efficientnet.dmap{i}", s) for i, s in enumerate(shapes)]


_REF_CACHE = {}


def _reference(name, training, frozen=False):
    """float64 maps and parameter gradients of the restatement, and the same with bf16 stores; once per (model, mode)"""
    key = (name, training, frozen)
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    ref, sd = EU.make_pair(name)
    Bn = BATCH[name]
    x = filler.images(Bn, S)
    keep = EU.keep_table(name, Bn)
    out = {"sd": EU.torchvision_layout(sd), "keep": keep}
    for emu in ((False, True) if name == "efficientnet_b0" and not frozen else (False,)):
        r = copy.deepcopy(ref)
        r.train(training)
        if frozen:
            _freeze(r.features)
        if emu:
            with _Bf16Emulation(r):
                maps = [_Round.apply(m) for m in r.maps(x.double(), keep if training else None)]
                sum((m * g.double()).sum() for m, g in zip(maps, _seeds([m.shape for m in maps]))).backward()
        else:
            maps = r.maps(x.double(), keep if training else None)
            sum((m * g.double()).sum() for m, g in zip(maps, _seeds([m.shape for m in maps]))).backward()
        out["bf16" if emu else "f64"] = ([m.detach() for m in maps], {k: p.grad for k, p in r.named_parameters() if not k.startswith("fc.")})
    _REF_CACHE[key] = out
    return out


def _freeze(features):
    """bn.eval() on the depthwise unit of features.3.1 and on the projection of features.5.1 (a residual block's keep pass),
    inside a training model"""
    features[3][1].block[1][1].eval()
    features[5][1].block[3][1].eval()


def _model(name, sd, training, dtype, keep):
    m = EfficientNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.compute_dtype = dtype
    m = m.cuda()
    m.train(training)
    m.set_keep_factors(keep)
    return m


def _run(m, need_grad=True):
    x = filler.images(BATCH[m.model_name], S).cuda()
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
    # (per tensor, against the same floor as the norms: the bias of a BatchNorm in front of a train-mode BatchNorm has a gradient
    #  of exactly zero, so float64 leaves 1e-16 and f32 1e-8 of noise there, and a ratio of the two says nothing)
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
            print(f"over its bound: {k} {got:.4f} > {2 * floor:.4f}")
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_b0_maps_and_gradients_match_the_restatement(training, dtype):
    """efficientnet_b0, batch 4 @64.  The bf16 bound is twice, per quantity, the error of the restatement run in float64 with
    bf16 stores; computed on the CPU when this test was written (NOTEBOOK 25.4): eval mode, maps 3.9e-3 .. 5.3e-3, gradients
    0.0018 / 0.0078 / 0.021 (min / median / max); training mode, where BatchNorm runs over 4 images of 2 x 2 .. 32 x 32 pixels
    and the last map has 16 samples per channel, maps 9.1e-3 .. 1.9e-1 and gradients 0.12 / 0.46 (min / median; a few tensors
    whose float64 gradient is zero have no relative error).  d(y) of a depthwise unit is stored ONCE on the GPU path -- the
    pool's gradient joins it in f32 inside the unit's BatchNorm backward -- and once in the emulation."""
    name = "efficientnet_b0"
    ref = _reference(name, training)
    keep = ref["keep"]
    assert (keep == 0).any(1).sum() >= 3 and (keep[:, -1] > 0).all()
    maps, grads = _run(_model(name, ref["sd"], training, dtype, keep))
    assert [t.shape[1] for t in maps] == list(EU.CHANNELS[name]) and [S // t.shape[2] for t in maps] == list(EU.strides(name))
    if dtype == torch.float32:
        _check_f32(maps, grads, ref, training)
    else:
        _check_bf16(maps, grads, ref)


def test_b0_draws_its_own_keep_tables():
    """set_keep_factors(None): the runner draws bernoulli(1 - p) / (1 - p) per site and image before every forward and writes
    the table into the program's arena, from where it is read back"""
    name = "efficientnet_b0"
    ref = _reference(name, True)
    m = _model(name, ref["sd"], True, torch.float32, None)
    for blk in m.blocks():  # (rates at which two tables of 9 x 4 factors almost surely differ: 0 .. 0.75)
        blk.stochastic_depth.p *= 4
    rates = torch.tensor(m._vt_keep_rates())
    tables = []
    for _ in range(2):
        maps, grads = _run(m)
        assert all(torch.isfinite(t).all() for t in maps) and all(torch.isfinite(g).all() for g in grads.values())
        t = m._vt_runner().last_keep_table.cpu()
        assert t.shape == (9, 4)
        kept = 1.0 / (1.0 - rates)[:, None].expand(9, 4)
        assert bool(((t == 0) | ((t - kept).abs() < 1e-6)).all())
        tables.append(t)
        m.zero_grad()
    assert not torch.equal(tables[0], tables[1])
    # a set table is what the arena holds, and the same table twice gives the same maps bit for bit
    m.set_keep_factors(ref["keep"])
    a, _ = _run(m, need_grad=False)
    assert torch.equal(m._vt_runner().last_keep_table.cpu(), ref["keep"])
    b, _ = _run(m, need_grad=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_v2_s_maps_and_gradient_norms():
    """efficientnet_v2_s, f32, batch 2 @64, training mode with a keep table: FusedMBConv blocks closed by a 1x1 projection (code
    0) and, at expand ratio 1, by their only 3x3 unit (SiLU, code 3)"""
    name = "efficientnet_v2_s"
    ref = _reference(name, True)
    maps, grads = _run(_model(name, ref["sd"], True, torch.float32, ref["keep"]))
    assert [t.shape[1] for t in maps] == list(EU.CHANNELS[name]) and [S // t.shape[2] for t in maps] == list(EU.strides(name))
    _check_f32(maps, grads, ref, True)


def test_a_frozen_batchnorm_inside_a_training_model():
    """bn.eval() on a depthwise unit (the fused pool pass with ready coefficients) and on a residual block's projection (the
    keep pass with ready coefficients): running statistics in forward, constants in backward, untouched"""
    name = "efficientnet_b0"
    ref = _reference(name, True, frozen=True)
    m = _model(name, ref["sd"], True, torch.float32, ref["keep"])
    _freeze(m.feat_extractor.features)
    frozen = m.feat_extractor.features[5][1].block[3][1]
    before = frozen.running_mean.clone()
    maps, grads = _run(m)
    _check_f32(maps, grads, ref, True)
    assert torch.equal(frozen.running_mean, before) and int(frozen.num_batches_tracked) == 0
    assert int(m.feat_extractor.features[5][1].block[0][1].num_batches_tracked) == 1


@pytest.mark.parametrize("neck", ["FPN", "PAN"])
def test_necks_take_the_five_maps(neck):
    ref = _reference("efficientnet_b0", False)
    m = _model("efficientnet_b0", ref["sd"], False, torch.float32, None)
    nk = getattr(necks, neck)(list(m.out_channels_list), 32)
    filler.fill_module(nk, "efficientnet.neck.")
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
NCLS, BT, ST = 16, 8, 64
LRS = {"SGD": (2e-4, 1e-3), "AdamW": (1e-4, 0.05)}  # (learning rate, weight decay)


def _groups(model, wd):
    norm = [p for m in model.modules() if isinstance(m, nn.BatchNorm2d) for p in m.parameters(recurse=False)]
    bias = [m.bias for m in model.modules() if isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None]
    other = [m.weight for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    return [{"params": norm, "weight_decay": 0.0}, {"params": bias, "weight_decay": 0.0}, {"params": other, "weight_decay": wd}]


def _train_step(sd, optimizer, **kw):
    lr, wd = LRS[optimizer]
    ts = TrainStep(EfficientNetExtractor("efficientnet_b0"), NCLS, BT, ST, torch.float32, lr=lr, momentum=0.9, weight_decay=wd,
                   label_smoothing=0.1, device="cuda", optimizer=optimizer, **kw)
    ts.model[0].load_torchvision_ckpt(EU.torchvision_layout(sd))
    with torch.no_grad():
        ts.model[3].weight.copy_(sd["fc.weight"])
        ts.model[3].bias.copy_(sd["fc.bias"])
    ts.weights_changed()
    return ts


def _three_steps(ts):
    x, y = filler.images(BT, ST).cuda(), filler.labels(BT, NCLS).cuda()
    losses = []
    for step in range(3):
        table = EU.keep_table("efficientnet_b0", BT, step)
        ts.set_keep_factors(table)
        ts.step(x, y)
        losses.append(ts.loss())
        assert torch.equal(ts.keep_factors().cpu(), table)  # the arena holds what was set
    return losses


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW"])
def test_train_steps_match_float64_losses(optimizer):
    """three steps of TrainStep(EfficientNetExtractor("efficientnet_b0")) in f32, batch 8 @64, a different set keep table per
    step, against the float64 restatement under torch.optim with the same tables: the losses within 1e-2, the first (forward
    only) within 1e-4.  The learning rates are where the RESTATEMENT ITSELF is well-conditioned: run in plain f32 torch on the
    CPU it stays within 1e-3 -- a tenth of the bound -- of its own float64 losses over the three steps (NOTEBOOK 25.5)."""
    lr, wd = LRS[optimizer]
    x, y = filler.images(BT, ST), filler.labels(BT, NCLS)
    ref, sd = EU.make_pair("efficientnet_b0", prefix="efficientnet.ts.", num_classes=NCLS)
    ref = ref.train()
    ts = _train_step(sd, optimizer)
    opt = (torch.optim.SGD(_groups(ref, wd), lr=lr, momentum=0.9) if optimizer == "SGD"
           else torch.optim.AdamW(_groups(ref, wd), lr=lr, weight_decay=wd))
    got, want = _three_steps(ts), []
    for step in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(ref(x.double(), EU.keep_table("efficientnet_b0", BT, step)), y, label_smoothing=0.1)
        loss.backward()
        opt.step()
        want.append(loss.item())
    print(optimizer, got, want)
    np.testing.assert_allclose(got, want, rtol=1e-2)
    assert got[0] == pytest.approx(want[0], rel=1e-4)  # the first loss: forward only


def test_captured_graphs_give_the_executor_paths_losses():
    """use_graphs=True: the keep table is written outside the captured lists, so a replayed graph follows the table of each step"""
    _, sd = EU.make_pair("efficientnet_b0", prefix="efficientnet.ts.", num_classes=NCLS)
    eager = _three_steps(_train_step(sd, "SGD"))
    graphs = _three_steps(_train_step(sd, "SGD", use_graphs=True))
    print(eager, graphs)
    assert graphs == pytest.approx(eager, rel=1e-5) and len(set(eager)) == 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_steps_are_bit_identical(dtype):
    """two fresh runs of three deterministic steps with equal seeds end in the same bits -- the tables are drawn from the
    trainer's own generator, the keep passes and the pool pass sum through fixed point -- and another seed draws other tables"""
    x, y = filler.images(4, S).cuda(), filler.labels(4, 10).cuda()
    states, tables = [], []
    for seed in (7, 7, 8):
        ts = TrainStep(EfficientNetExtractor("efficientnet_b0"), 10, 4, S, dtype, lr=0.01, device="cuda", deterministic=True,
                       drop_seed=seed)
        filler.fill_module(ts.model, "efficientnet.det.")
        ts.weights_changed()
        losses, drawn = [], []
        for _ in range(3):
            ts.step(x, y)
            losses.append(ts.loss())
            drawn.append(ts.keep_factors().cpu())
        torch.cuda.synchronize()
        states.append((losses, ts.store.pflat.clone(), ts.gflat.clone(), ts.mflat.clone(), ts.store.sflat.clone()))
        tables.append(torch.stack(drawn))
        del ts
    # parameters, gradients, momentum and BatchNorm state.  (The loss SCALAR a step reports is summed over the batch with a
    # float atomic in vt_softmax_xent and may differ in its last bit; nothing reads it.)
    for a, b in zip(states[0][1:], states[1][1:]):
        assert torch.equal(a, b)
    assert states[0][0] == pytest.approx(states[1][0], rel=1e-6) and all(l == l for l in states[0][0])
    assert torch.equal(tables[0], tables[1]) and not torch.equal(tables[0], tables[2])
    assert len({t.numpy().tobytes() for t in tables[0]}) > 1  # every step draws anew


def test_refusals_by_name():
    m = EfficientNetExtractor("efficientnet_b0").cuda()
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m(torch.rand(2, 3, 64, 64, device="cuda", requires_grad=True))
    with pytest.raises(NotImplementedError, match="pretrained"):
        EfficientNetExtractor("efficientnet_v2_s", pretrained=True)
    with pytest.raises(ValueError, match="efficientnet_b9"):
        EfficientNetExtractor("efficientnet_b9")
