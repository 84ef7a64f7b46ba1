"""optimizer="Lamb" and clip_grad_norm through the fused train step.

As tests/test_adamw_gpu.py argues for AdamW, the step's bookkeeping is checked with the gradients as an INPUT to both
sides: the float64 yardstick of tests/lamb_util.py is fed the flat gradient buffer each step left behind, and the update
of every parameter is bounded by min(max(4 x what the float32 restatement loses on it, 1e-5), 1e-3).  The norm the device
formed is held to the counted bound of lamb_util (C_NORM x 2^-24)."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.backbones import ConvNeXt, DeiT3
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import convnext_util as U
import deit_util as DU
import lamb_util as LU

pytestmark = pytest.mark.gpu

WD, NORM_WD, BIAS_WD = 0.05, 0.01, 0.02  # all three groups adapt
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def _param_views(ts, flat):
    """per-parameter 1-D views of a flat buffer laid out like the store (the parameter's own elements, no slot padding)"""
    return [flat[o: o + p.numel()] for p, o in zip(ts.store.params, ts.store.offsets)]


def _wds(ts):
    groups = param_groups(ts.model)
    wd_of = {GROUP_OTHER: WD, GROUP_NORM: NORM_WD, GROUP_BIAS: BIAS_WD}
    return [wd_of[groups[id(p)]] for p in ts.store.params]


def _names(ts):
    names = {id(p): k for k, p in ts.model.named_parameters()}
    return [names[id(p)] for p in ts.store.params]


def _fixture_step(dtype, optimizer, **kw):
    ts = TrainStep(ConvNeXt(24, (1, 2)), 10, 3, 64, dtype, optimizer=optimizer, include_pool=False, weight_decay=WD,
                   norm_weight_decay=NORM_WD, bias_weight_decay=BIAS_WD, label_smoothing=0.1, device="cuda", **kw)
    U.fill(ts.model[0], "adamw.0.")  # the fixture step of tests/test_adamw_gpu.py
    filler.fill_module(ts.model[1], "adamw.1.")
    ts.weights_changed()
    return ts


def _check_updates(tag, names, init, got, ref64, ref32):
    worst, worst_key = 0.0, None
    for k, name in enumerate(names):
        d64 = ref64[k] - init[k].double()
        den = d64.norm()
        assert den > 0, name
        err = ((got[k].double() - init[k].double()) - d64).norm() / den
        floor = ((ref32[k].double() - init[k].double()) - d64).norm() / den
        bound = min(max(4 * floor.item(), 1e-5), 1e-3)
        if err.item() / bound > worst:
            worst, worst_key = err.item() / bound, (name, err.item(), bound)
        assert err.item() < bound, f"{name}: update error {err.item():.3e} >= {bound:.3e} (float32 restatement: {floor.item():.3e})"
    print(f"{tag}: worst update error {worst_key[1]:.3e} ({worst_key[0]}) at {worst:.2f} of its bound {worst_key[2]:.1e}")


def _check_head_rows_and_mirror(ts, dtype):
    if dtype == torch.bfloat16:
        n = ts.store.total
        assert torch.equal(ts.store.mirror[:n], ts.store.pflat[:n].to(torch.bfloat16))
    i = next(j for j, p in enumerate(ts.store.params) if p is ts.model[1].weight)
    o = ts.store.offsets[i]
    assert not ts.store.pflat[o + 480: o + ts.store.slots[i]].any() and not ts.vflat[o + 480: o + ts.store.slots[i]].any()
    assert not ts.mflat[o + 480: o + ts.store.slots[i]].any()


# ---- Lamb applies the yardstick to the step's own gradients ------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step_applies_lamb_to_its_own_gradients(dtype, graphs):
    lr, lr3, M = 1e-3, 2e-3, 1.0
    ts = _fixture_step(dtype, "Lamb", lr=lr, eps=1e-6, use_graphs=graphs, lamb_max_grad_norm=M)
    names, wds = _names(ts), _wds(ts)
    assert len(set(wds)) == 3
    init = [v.detach().cpu().clone() for v in _param_views(ts, ts.store.pflat)]
    kw = dict(lr=lr, eps=1e-6, M=M)
    refs = {torch.float64: LU.Lamb([p.double() for p in init], wds, **kw), torch.float32: LU.Lamb(init, wds, **kw)}
    x, y = filler.images(3, 64).cuda(), filler.labels(3, 10).cuda()
    before = N.launch_count()
    assert ts.opt_steps() == 0
    for step in range(3):
        if step == 2:  # a schedule step: the device learning rate changes, nothing is rebuilt or re-captured
            ts.set_lr(lr3)
            for r in refs.values():
                r.lr = lr3
        ts.step(x, y)
        grads = [g.detach().cpu().clone() for g in _param_views(ts, ts.gflat)]  # left as the backward wrote them
        for dt, r in refs.items():
            info = r.step([g.to(dt) for g in grads])
        assert ts.opt_steps() == step + 1
        n_dev = ts.last_grad_norm()
        rel = abs(n_dev - info["norm"]) / info["norm"]
        print(f"{dtype}/{'hipgraph' if graphs else 'eager'} step {step}: N {n_dev!r} against {info['norm']!r} "
              f"({rel / LU.U24:.2f} u of {LU.C_NORM}), c2 {info['c2']:.4f}")
        assert rel <= LU.C_NORM * LU.U24
    assert N.launch_count() > before and refs[torch.float64].info["c2"] > 1.0  # LAMB's own clip was active
    got = [v.detach().cpu() for v in _param_views(ts, ts.store.pflat)]
    _check_updates(f"Lamb {dtype}/{'hipgraph' if graphs else 'eager'}", names, init, got, refs[torch.float64].p,
                   refs[torch.float32].p)
    _check_head_rows_and_mirror(ts, dtype)


def test_step_applies_clipped_adamw_to_its_own_gradients():
    lr, lr3 = 1e-3, 2e-3
    probe = _fixture_step(torch.float32, "AdamW", lr=lr)
    x, y = filler.images(3, 64).cuda(), filler.labels(3, 10).cuda()
    probe.step(x, y)
    n0 = float(LU.grad_norm([probe.gflat.double().cpu()]))
    C = n0 / 2  # (the first step clips; whether the later ones do is the reference's business as much as the device's)
    ts = _fixture_step(torch.float32, "AdamW", lr=lr, clip_grad_norm=C)
    names = _names(ts)
    init = [v.detach().cpu().clone() for v in _param_views(ts, ts.store.pflat)]
    refs = {}
    for dt in (torch.float64, torch.float32):
        ps = [nn.Parameter(p.to(dt).clone()) for p in init]
        by_wd = {}
        for p, wd in zip(ps, _wds(ts)):
            by_wd.setdefault(wd, []).append(p)
        refs[dt] = (ps, torch.optim.AdamW([{"params": v, "weight_decay": k} for k, v in by_wd.items()], lr=lr))
    clipped = 0
    for step in range(3):
        if step == 2:
            ts.set_lr(lr3)
            for _, opt in refs.values():
                for grp in opt.param_groups:
                    grp["lr"] = lr3
        ts.step(x, y)
        grads = [g.detach().cpu().clone() for g in _param_views(ts, ts.gflat)]
        norm = float(LU.grad_norm([ts.gflat.double().cpu()]))
        c1, _ = LU.clip_factors(norm, float(np.float32(C)), None)
        clipped += c1 < 1.0
        for dt, (ps, opt) in refs.items():
            for p, g in zip(ps, grads):
                p.grad = (c1 * g.double()).to(dt)
            opt.step()
        rel = abs(ts.last_grad_norm() - norm) / norm
        print(f"clipped AdamW step {step}: N {ts.last_grad_norm()!r} against {norm!r} ({rel / LU.U24:.2f} u), c1 {c1:.4f}")
        assert rel <= LU.C_NORM * LU.U24 and ts.opt_steps() == step + 1
    assert clipped >= 1
    got = [v.detach().cpu() for v in _param_views(ts, ts.store.pflat)]
    _check_updates("clipped AdamW f32", names, init, got, [p.data for p in refs[torch.float64][0]],
                   [p.data for p in refs[torch.float32][0]])
    _check_head_rows_and_mirror(ts, torch.float32)


# ---- clipping on a BatchNorm model with SGD --------------------------------------------------------------------------------
def _vovnet_step(**kw):
    ts = TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.float32, lr=0.05, momentum=0.9, weight_decay=WD,
                   norm_weight_decay=NORM_WD, bias_weight_decay=BIAS_WD, deterministic=True, device="cuda", **kw)
    filler.fill_module(ts.model, "lamb.vovnet.")
    ts.weights_changed()
    return ts


def test_sgd_clipping_on_a_batchnorm_model():
    x, y = filler.images(2, 64).cuda(), filler.labels(2, 16).cuda()
    plain = _vovnet_step()
    assert {plain.opt_ops[k].kind for k in range(plain.n_opt)} == {N.OP_SGD}  # the parent's list
    init = plain.store.pflat.detach().cpu().clone()
    plain.step(x, y)
    torch.cuda.synchronize()
    g0 = plain.gflat.detach().cpu().clone()
    n0 = float(LU.grad_norm([g0.double()]))
    assert n0 > 0 and math.isfinite(n0)
    runs = {}
    for tag, C in (("half", n0 / 2), ("double", 2 * n0), ("inf", float("inf"))):
        ts = _vovnet_step(clip_grad_norm=C)
        assert torch.equal(ts.store.pflat.cpu(), init)
        ts.step(x, y)
        torch.cuda.synchronize()
        assert torch.equal(ts.gflat.cpu(), g0)  # deterministic=True: the same gradient, and the optimiser left it alone
        rel = abs(ts.last_grad_norm() - n0) / n0
        print(f"clip {tag}: N {ts.last_grad_norm()!r} against {n0!r} ({rel / LU.U24:.2f} u of {LU.C_NORM})")
        assert rel <= LU.C_NORM * LU.U24
        runs[tag] = ts
    # nothing clips: the unclipped run's weights, bit for bit
    for tag in ("double", "inf"):
        assert torch.equal(runs[tag].store.pflat, plain.store.pflat) and torch.equal(runs[tag].mflat, plain.mflat)
        assert runs[tag]._ctl[N.VT_CTL_FACTOR].item() == 1.0
    # half the norm: float64 SGD on c1 x the gradient (c1 = C / (N + 1e-6), a hair below 1/2)
    ts = runs["half"]
    c1, _ = LU.clip_factors(n0, float(np.float32(n0 / 2)), None)
    assert abs(c1 - 0.5) < 1e-6
    names, wds = _names(ts), _wds(ts)
    upd = {}
    for dt in (torch.float64, torch.float32):
        ps = _param_views(ts, init.to(dt))
        gs = _param_views(ts, g0.to(dt))
        upd[dt] = [p - 0.05 * (float(np.float32(c1)) * g + wd * p) if dt == torch.float32 else p - 0.05 * (c1 * g + wd * p)
                   for p, g, wd in zip(ps, gs, wds)]  # first step: the momentum buffer is the gradient itself
    got = [v.detach().cpu() for v in _param_views(ts, ts.store.pflat)]
    _check_updates("SGD clipped at N0/2", names, _param_views(ts, init), got, upd[torch.float64], upd[torch.float32])
    assert not torch.equal(ts.store.pflat, plain.store.pflat)


def test_set_clip_grad_norm_under_a_replayed_graph():
    x, y = filler.images(2, 64).cuda(), filler.labels(2, 16).cuda()
    ts = _vovnet_step(clip_grad_norm=float("inf"), use_graphs=True)
    ts.step(x, y)
    torch.cuda.synchronize()
    assert ts._ctl[N.VT_CTL_FACTOR].item() == 1.0
    n1 = ts.last_grad_norm()
    graph = ts._graphs["opt"]
    p1, m1 = ts.store.pflat.double().cpu(), ts.mflat.double().cpu()
    C = float(np.float32(n1 / 64))  # far below any norm the second step can have: it clips
    ts.set_clip_grad_norm(C)
    ts.step(x, y)
    torch.cuda.synchronize()
    assert ts._graphs["opt"] is graph  # replayed, not re-captured
    g2 = ts.gflat.double().cpu()
    n2 = float(LU.grad_norm([g2]))
    c1, _ = LU.clip_factors(n2, C, None)
    assert c1 < 0.1 and abs(ts.last_grad_norm() - n2) <= LU.C_NORM * LU.U24 * n2
    assert abs(ts._ctl[N.VT_CTL_FACTOR].item() - c1) <= LU.C_NORM * LU.U24 * c1
    wd = torch.zeros_like(p1)
    for s0, s1, w in ts.segments:
        wd[s0:s1] = w
    # m2 = mu m1 + (c1 g2 + wd p1): the factor's C_NORM u, two fused operations and the product c1 g2
    terms = (0.9 * m1).abs() + (c1 * g2).abs() + (wd * p1).abs()
    want = 0.9 * m1 + c1 * g2 + wd * p1
    err = (ts.mflat.double().cpu() - want).abs()
    bound = (LU.C_NORM + 4) * LU.U24 * terms + 1e-30
    print(f"graph replay after set_clip_grad_norm: c1 {c1:.5f}, momentum at {(err / bound).max().item():.3f} of its bound; "
          f"unclipped it would differ by {(g2 * (1 - c1)).abs().max().item():.3e}")
    assert (err <= bound).all()
    assert ((g2 * (1 - c1)).abs() > 100 * bound).any()  # (an unclipped second step is far outside)


# ---- determinism --------------------------------------------------------------------------------------------------------------
def test_deterministic_lamb_steps_are_bit_identical_and_validate_runs():
    images, labels = filler.images(3, 16).cuda(), filler.labels(3, 10).cuda()
    finals = []
    for _ in range(2):
        ts = TrainStep(DeiT3(*DU.TRAIN_ARGS, **DU.TRAIN_KW), 10, 3, 16, torch.bfloat16, lr=1e-3, weight_decay=WD,
                       norm_weight_decay=NORM_WD, bias_weight_decay=BIAS_WD, optimizer="Lamb", eps=1e-6, include_pool=False,
                       deterministic=True, device="cuda")
        DU.fill(ts.model, "lamb.deit3.")
        ts.weights_changed()
        for _ in range(3):
            ts.step(images, labels)
        torch.cuda.synchronize()
        finals.append([t.clone() for t in (ts.store.pflat, ts.mflat, ts.vflat, ts.store.mirror)])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
    assert ts.opt_steps() == 3 and ts.mflat.any() and ts.vflat.any() and math.isfinite(ts.last_grad_norm())
    val = ts.validate(images, labels)
    print(f"validate after three Lamb steps: {val}")
    assert np.isfinite(val["loss"]) and val["count"] == 3 and 0 <= val["correct"] <= 3
