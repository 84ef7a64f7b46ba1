"""ResNetExtractor(stochastic_depth=...) on the GPU against the float64 restatement with keep factors (tests/rsb_util.py): all
five maps and every parameter gradient with a set table (resnet18, resnet50; f32 and bf16; the bounds, the bf16 emulation
and the checks are those of tests/test_resnet_gpu.py, restated in rsb_util), a drawn table read back from the arena, three
Lamb and SGD steps of the recipe -- loss="bce", stochastic_depth=0.05, a different table per step -- against the float64
losses, captured graphs, deterministic steps bit for bit, and eval mode equal to a model built without the argument."""
import copy

import numpy as np
import pytest
import torch

import resnet_util
import rsb_util as RU
from oracle import filler
from vision_toolbox.backbones import ResNetExtractor
from vision_toolbox.trainer import TrainStep

pytestmark = pytest.mark.gpu

B, S, SD = RU.MODEL_B, RU.MODEL_S, 0.2
_REFS = {}


def _reference(name):
    """float64 maps and parameter gradients in training mode with the set table, and the same with bf16 stores"""
    if name in _REFS:
        return _REFS[name]
    ref, sd = resnet_util.make_pair(name)
    x = filler.images(B, S)
    ps = RU.rates(name, SD)
    table = RU.table(ps, B)
    out = {"sd": sd, "table": table}
    with torch.no_grad():   # the last map without the table: what the set table has to move
        out["plain_last"] = RU.maps(copy.deepcopy(ref).train(), x.double(), ps, None)[-1]
    for emu in (False, True):
        r = copy.deepcopy(ref).train()
        if emu:
            with RU.Bf16Emulation(r):
                maps = RU.maps(r, x.double(), ps, table.double(), store=RU.Round.apply)
                sum((m * g.double()).sum() for m, g in zip(maps, RU.seeds([m.shape for m in maps]))).backward()
        else:
            maps = RU.maps(r, x.double(), ps, table.double())
            sum((m * g.double()).sum() for m, g in zip(maps, RU.seeds([m.shape for m in maps]))).backward()
        out["bf16" if emu else "f64"] = ([m.detach() for m in maps],
                                         {k: p.grad for k, p in r.named_parameters() if not k.startswith("fc.")})
    _REFS[name] = out
    return out


def _model(name, sd, dtype, rate=SD):
    m = ResNetExtractor(name, stochastic_depth=rate)
    m.load_torchvision_ckpt(sd)
    m.compute_dtype = dtype
    return m.cuda().train()


def _plain(name, sd, dtype):
    """a model built without the argument, in training mode"""
    m = ResNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.compute_dtype = dtype
    return m.cuda().train()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_maps_and_gradients_match_the_restatement_with_a_set_table(name, dtype):
    ref = _reference(name)
    assert (ref["table"] == 0).any(0).all() and not (ref["table"] == 0).all(1).any()  # every image is dropped somewhere
    m = _model(name, ref["sd"], dtype)
    m.set_keep_factors(ref["table"])
    maps, grads = RU.run_model(m)
    assert len(maps) == 5 and maps[-1].shape[2:] == (2, 2)
    assert torch.equal(m._vt_runner().last_keep_table.cpu(), ref["table"])
    if dtype == torch.float32:
        RU.check_f32(maps, grads, ref)
        # the table matters: without it the last map is far outside the bound
        assert RU.rel_err(maps[-1], ref["plain_last"]) > 10 * RU.F32_MAPS
    else:
        RU.check_bf16(maps, grads, ref)


def test_eval_mode_equals_a_model_built_without_the_argument():
    _, sd = resnet_util.make_pair("resnet18")
    x = filler.images(B, S).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        a, b = _model("resnet18", sd, dtype).eval(), _plain("resnet18", sd, dtype).eval()
        with torch.no_grad():
            for u, v in zip(a.get_feature_maps(x), b.get_feature_maps(x)):
                assert torch.equal(u, v)
        # rate 0 in training mode as well
        c, d = _model("resnet18", sd, dtype, rate=0.0), _plain("resnet18", sd, dtype)
        with torch.no_grad():
            for u, v in zip(c.get_feature_maps(x), d.get_feature_maps(x)):
                assert torch.equal(u, v)


# ---- the fused train step with the recipe's pieces ----------------------------------------------------------------------------
def _step(dtype, optimizer="SGD", lr=None, **kw):
    extra = dict(eps=RU.LAMB_EPS, lamb_max_grad_norm=1.0) if optimizer == "Lamb" else {}
    ts = TrainStep(ResNetExtractor(RU.STEP_MODEL, stochastic_depth=RU.STEP_SD), RU.STEP_CLASSES, RU.STEP_BATCH, RU.STEP_SIZE, dtype,
                   lr=RU.STEP_LR[optimizer] if lr is None else lr, momentum=0.9, weight_decay=RU.STEP_WD,
                   label_smoothing=RU.STEP_SMOOTHING, device="cuda", optimizer=optimizer, loss="bce", **extra, **kw)
    sd = RU.step_state()
    ts.model[0].load_torchvision_ckpt(sd)
    with torch.no_grad():
        ts.model[3].weight.copy_(sd["fc.weight"])
        ts.model[3].bias.copy_(sd["fc.bias"])
    ts.weights_changed()
    return ts


def _batch():
    return filler.images(RU.STEP_BATCH, RU.STEP_SIZE).cuda(), filler.labels(RU.STEP_BATCH, RU.STEP_CLASSES).cuda()


def _tables():
    ps = RU.rates(RU.STEP_MODEL, RU.STEP_SD)
    return [RU.table(ps, RU.STEP_BATCH, i) for i in range(3)]


@pytest.mark.parametrize("optimizer", ["SGD", "Lamb"])
def test_recipe_steps_match_float64_losses(optimizer):
    """three f32 steps of loss="bce" with stochastic depth and a different table per step: the losses within 1e-2 of the
    float64 restatement's (the bound of the step tests of tests/test_resnet_gpu.py), the first within 1e-4, at the learning
    rates tests/test_rsb_cpu.py checks"""
    want = RU.ref_steps(optimizer)
    ts = _step(torch.float32, optimizer)
    hist = ts.prog.kind_histogram
    assert hist["bce"] == 1 and hist["bn_add_act_keep_fin_apply"] == 7 and hist["bn_add_act_keep_bwd_fin_apply"] == 7
    x, y = _batch()
    got = []
    for t in _tables():
        ts.set_keep_factors(t)
        ts.step(x, y)
        got.append(ts.loss())
        assert torch.equal(ts.keep_factors().cpu(), t)
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print(f"recipe steps {optimizer}: {got} against {want}: off by {rel}")
    np.testing.assert_allclose(got, want, rtol=RU.STEP_RTOL)
    assert got[0] == pytest.approx(want[0], rel=1e-4)


def test_drawn_table_is_read_back_from_the_arena():
    ts = _step(torch.bfloat16, drop_seed=5)
    x, y = _batch()
    seen = []
    for _ in range(3):
        ts.step(x, y)
        t = ts.keep_factors().cpu()
        assert t.shape == (7, RU.STEP_BATCH)
        for row, p in zip(t, ts.model[0].drop_rates()[1:]):
            assert all(v == 0.0 or v == pytest.approx(1.0 / (1.0 - p), rel=1e-6) for v in row.tolist())
        seen.append(t)
    assert np.isfinite(ts.loss())
    # the same seed draws the same tables
    ts2 = _step(torch.bfloat16, drop_seed=5)
    ts2.step(x, y)
    assert torch.equal(ts2.keep_factors().cpu(), seen[0])


def test_captured_graphs_follow_the_table():
    x, y = _batch()
    runs = {}
    for graphs in (False, True):
        ts = _step(torch.float32, "Lamb", use_graphs=graphs)
        losses = []
        for t in _tables():
            ts.set_keep_factors(t)
            ts.step(x, y)
            losses.append(ts.loss())
        runs[graphs] = losses
    print(f"recipe under graphs: {runs[True]} against eager {runs[False]}")
    assert runs[True] == pytest.approx(runs[False], rel=1e-4)
    assert runs[True] == pytest.approx(RU.ref_steps("Lamb"), rel=RU.STEP_RTOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_recipe_steps_are_bit_identical(dtype):
    x, y = _batch()
    states = []
    for _ in range(2):
        ts = _step(dtype, "Lamb", deterministic=True, drop_seed=11)
        losses, tables = [], []
        for _ in range(3):
            ts.step(x, y)
            losses.append(ts.loss())
            tables.append(ts.keep_factors())
        torch.cuda.synchronize()
        states.append((losses, tables, ts.store.pflat.clone(), ts.gflat.clone(), ts.mflat.clone(), ts.vflat.clone(),
                       ts.store.sflat.clone()))
        del ts
    assert states[0][0] == states[1][0] and all(np.isfinite(l) for l in states[0][0])
    for a, b in zip(states[0][1], states[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(states[0][2:], states[1][2:]):
        assert torch.equal(a, b)
