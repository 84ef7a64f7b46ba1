"""AdamW / Adam on the GPU: the kernel against torch.optim, the fused train step of a ConvNeXt classifier
(`include_pool=False`) against torch.optim.AdamW fed with the step's own gradients, and gradients / losses against the
fixture of tools/gen_golden_convnext_train.py (the unmodified reference, three AdamW steps on CPU).

Why three separate checks instead of one trajectory comparison: Adam divides by sqrt(v), so relative gradient noise on a
small-gradient element becomes a full-size update error.  With noise of 1e-3 of each gradient's rms (the project's f32
gradient bound) added to the float64 reference, the head weight's 3-step update moves by 0.2 while the losses move by
1e-6 (lr 1e-4).  A per-parameter comparison of trajectories would test conditioning.  So: (1) the kernel's arithmetic
against torch on identical inputs, to f32 rounding; (2) the step's bookkeeping -- groups, decoupled decay per group,
bias-correction count, mirror -- with the gradients as an INPUT to both sides, against torch.optim.AdamW in float64,
bounded by what torch's own float32 optimiser loses on the same parameter; (3) the gradients of step 1 and the three
losses against the reference fixture under the project's gradient and forward bounds.

Every test prints its figures before it asserts (worst update error per dtype, every gradient against its bound, the
losses); NOTEBOOK.md section 13 is where they are recorded."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.backbones import ConvNeXt
from vision_toolbox.trainer import HYPER_STEP, TrainStep

import convnext_util as U
from gpu_util import stream, vp

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 2e-4, 3e-2  # the project's forward bounds (tests/test_convnext_gpu.py)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
_NORMS = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.LayerNorm, nn.GroupNorm)


# ---- 1. the kernel against torch.optim ------------------------------------------------------------------------------
def _run_kernel(name, n, p0, grads, mirror_dtype, grad_scale, lr, betas, eps, wd):
    n_pad = (n + 3) // 4 * 4
    p, m, v = (torch.zeros(n_pad, device="cuda") for _ in range(3))
    p[:n] = p0.cuda()
    mirror = torch.zeros(n_pad, device="cuda", dtype=torch.bfloat16) if mirror_dtype is not None else None
    hyper = torch.zeros(16, device="cuda")
    hyper[:4] = lr  # the learning rate and (slot 4, an int32) the step count live in this device buffer
    L = N.lib()
    for g in grads:
        gd = torch.zeros(n_pad, device="cuda")
        gd[:n] = (g / grad_scale).cuda()
        N.check(L.vt_adam_tick(vp(hyper), betas[0], betas[1], stream()))  # once per step, as the optimiser list does
        N.check(L.vt_adamw(vp(p), vp(gd), vp(m), vp(v), vp(mirror), N.VT_BF16, n, betas[0], betas[1], eps, wd, grad_scale,
                           int(name == "AdamW"), vp(hyper), stream()))
    torch.cuda.synchronize()
    return p[:n].cpu(), m[:n].cpu(), v[:n].cpu(), None if mirror is None else mirror[:n].cpu(), hyper.cpu()


@pytest.mark.parametrize("mirror", [torch.bfloat16, None], ids=["mirror_bf16", "no_mirror"])
@pytest.mark.parametrize("name", ["AdamW", "Adam"])
def test_adamw_kernel_matches_torch_optim(name, mirror):
    n, steps = 100_003, 5  # (odd tail: n % 4 == 3)
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 0.05
    p0 = filler.tensor("adamw.p", (n,))
    scales = [1.0, -0.5, 2.0, 0.25, -1.5]  # a different gradient each step, scale and sign varied
    grads = [s * filler.tensor(f"adamw.g{k}", (n,)) for k, s in enumerate(scales)]
    ref = torch.nn.Parameter(p0.double())
    opt = getattr(torch.optim, name)([ref], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    for g in grads:
        ref.grad = g.double()
        opt.step()
    st = opt.state[ref]
    before = N.launch_count()
    p, m, v, mir, hyper = _run_kernel(name, n, p0, grads, mirror, 1.0, lr, betas, eps, wd)
    assert N.launch_count() >= before + 2 * steps
    for tag, got, want in (("p", p, ref.data), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
        d = (got.double() - want).abs()
        print(f"{name}/{'bf16 mirror' if mirror else 'no mirror'}: {tag} worst |diff| {d.max().item():.3e}, "
              f"outside the bound {(d > 1e-6 + 1e-6 * want.abs()).sum().item()} of {n}")
        torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-6)
    assert int(hyper[HYPER_STEP:HYPER_STEP + 1].view(torch.int32)) == steps
    assert hyper[0].item() == np.float32(lr)  # (the kernels only read the learning rate)
    if mirror is not None:
        assert torch.equal(mir, p.to(torch.bfloat16))  # the mirror is the RNE cast of the NEW weights
    # grad_scale: half of the doubled gradients is the plain gradient
    p2, m2, v2, _, _ = _run_kernel(name, n, p0, grads, mirror, 0.5, lr, betas, eps, wd)
    for got, want in ((p2, ref.data), (m2, st["exp_avg"]), (v2, st["exp_avg_sq"])):
        torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-6)


def test_adamw_entry_refuses_bad_arguments():
    p = torch.zeros(64, device="cuda")
    hyper = torch.zeros(16, device="cuda")
    L = N.lib()
    args = lambda a, h: (vp(a), vp(p), vp(p), vp(p), None, N.VT_BF16, 16, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, h, stream())  # noqa: E731
    assert L.vt_adamw(*args(p[1:], vp(hyper))) == N.VT_ERR_INVALID  # not 16-byte aligned
    assert L.vt_adamw(*args(p, None)) == N.VT_ERR_INVALID  # the step count has to come from the device
    assert L.vt_adam_tick(None, 0.9, 0.999, stream()) == N.VT_ERR_INVALID


# ---- helpers for the train-step checks -----------------------------------------------------------------------------------
def _reference_groups(model, wd, norm_wd, bias_wd):
    """the three weight-decay groups of the reference recipe (classifier.py:122-155), restated on a CPU model: parameters
    of normalisation layers / biases of Linear and convolution layers / everything else"""
    norm, bias, other = [], [], []
    for mod in model.modules():
        own = list(mod.parameters(recurse=False))
        leaf = next(mod.children(), None) is None
        if leaf and isinstance(mod, _NORMS):
            norm += own
        elif leaf and isinstance(mod, (nn.Linear, nn.modules.conv._ConvNd)):
            other.append(mod.weight)
            if mod.bias is not None:
                bias.append(mod.bias)
        else:
            other += own
    groups = [{"params": norm, "weight_decay": norm_wd}, {"params": bias, "weight_decay": bias_wd},
              {"params": other, "weight_decay": wd}]
    return [g for g in groups if g["params"]]


def _device_grads(ts):
    """per-parameter views of the flat f32 gradient buffer the backward list wrote (state_dict naming; 4-D filters are
    stored [O][kh][kw][I])"""
    out = {}
    names = {id(p): k for k, p in ts.model.named_parameters()}
    for p, off in zip(ts.store.params, ts.store.offsets):
        g = ts.gflat[off: off + p.numel()]
        g = g.view(p.shape[0], p.shape[2], p.shape[3], p.shape[1]).permute(0, 3, 1, 2) if p.dim() == 4 else g.view(p.shape)
        out[names[id(p)]] = g.detach().cpu().clone()
    return out


def _cpu_model(sd, dtype=torch.float32):
    m = nn.Sequential(ConvNeXt(24, (1, 2)), nn.Linear(48, 10))
    m.load_state_dict({k: v.detach().cpu() for k, v in sd.items()})
    return m.to(dtype)


def _fixture_step(dtype, pre, **kw):
    ts = TrainStep(ConvNeXt(24, (1, 2)), 10, 3, 64, dtype, optimizer="AdamW", include_pool=False, weight_decay=0.05,
                   norm_weight_decay=0.0, bias_weight_decay=0.0, label_smoothing=0.1, device="cuda", **kw)
    U.fill(ts.model[0], pre + "0.")  # filler + the +1.0 rule of the ConvNeXt fixtures on the backbone
    filler.fill_module(ts.model[1], pre + "1.")
    ts.weights_changed()
    return ts


# ---- 2. the step applies torch's AdamW to the gradients it computed ------------------------------------------------------
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step_applies_torch_adamw_to_its_own_gradients(dtype, graphs):
    lr, lr3, wd = 1e-3, 2e-3, 0.05
    ts = _fixture_step(dtype, "adamw.", lr=lr, use_graphs=graphs)
    init = {k: v.detach().cpu().clone() for k, v in ts.model.state_dict().items()}
    cpu = {torch.float64: _cpu_model(init, torch.float64), torch.float32: _cpu_model(init)}
    opts = {dt: torch.optim.AdamW(_reference_groups(m, wd, 0.0, 0.0), lr=lr, weight_decay=wd) for dt, m in cpu.items()}
    x, y = filler.images(3, 64).cuda(), filler.labels(3, 10).cuda()
    before = N.launch_count()
    assert ts.opt_steps() == 0
    for step in range(3):
        if step == 2:  # a schedule step: the device learning rate changes, nothing is rebuilt or re-captured
            ts.set_lr(lr3)
            for opt in opts.values():
                for grp in opt.param_groups:
                    grp["lr"] = lr3
        ts.step(x, y)
        grads = _device_grads(ts)
        for dt, m in cpu.items():
            for k, p in m.named_parameters():
                p.grad = grads[k].to(dt)
            opts[dt].step()
        assert ts.opt_steps() == step + 1  # the device counts, eager and as a replayed graph
    assert N.launch_count() > before
    sd = {k: v.detach().cpu() for k, v in ts.model.state_dict().items()}
    ref64, ref32 = cpu[torch.float64].state_dict(), cpu[torch.float32].state_dict()
    assert set(sd) == set(ref64) and {"1.weight", "1.bias"} <= set(sd)
    worst, worst_key = 0.0, None
    for k in sd:
        d64 = ref64[k] - init[k].double()
        den = d64.norm()
        assert den > 0, k
        err = ((sd[k].double() - init[k].double()) - d64).norm() / den
        floor = ((ref32[k].double() - init[k].double()) - d64).norm() / den
        # 4 x what torch's own float32 AdamW loses on this parameter; never below 1e-5 (floors at rounding level), never
        # above 1e-3 (a large floor must not hide a wrong update: a wrong decay group, a coupled decay or a bias
        # correction off by one step move an update by 1e-2 or more)
        bound = min(max(4 * floor.item(), 1e-5), 1e-3)
        if err.item() / bound > worst:
            worst, worst_key = err.item() / bound, (k, err.item(), bound)
        assert err.item() < bound, f"{k}: update error {err.item():.3e} >= {bound:.3e} (float32 torch: {floor.item():.3e})"
    print(f"{dtype}/{'hipgraph' if graphs else 'eager'}: worst update error {worst_key[1]:.3e} ({worst_key[0]}) at "
          f"{worst:.2f} of its bound {worst_key[2]:.1e}")
    if dtype == torch.bfloat16:
        n = ts.store.total
        assert torch.equal(ts.store.mirror[:n], ts.store.pflat[:n].to(torch.bfloat16))
    # the rows the store reserves behind the 10-class head stay exactly zero
    i = next(j for j, p in enumerate(ts.store.params) if p is ts.model[1].weight)
    o = ts.store.offsets[i]
    assert not ts.store.pflat[o + 480: o + ts.store.slots[i]].any() and not ts.vflat[o + 480: o + ts.store.slots[i]].any()


# ---- 3. gradients and losses against the reference fixture ---------------------------------------------------------------
def _gerr(got, ref):
    return ((got.float().cpu() - ref).norm() / ref.norm().clamp_min(1e-3 * (ref.numel() ** 0.5))).item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gradients_and_losses_match_the_reference_fixture(dtype):
    g = np.load(U.GOLDEN / "convnext_train.npz")
    pre = str(g["recipe"][0])
    lr, wd, norm_wd, bias_wd, smooth, steps = (float(v) for v in g["hyper"])
    assert (wd, norm_wd, bias_wd, smooth, int(steps)) == (0.05, 0.0, 0.0, 0.1, 3)
    ts = _fixture_step(dtype, pre, lr=lr)
    sd = ts.model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    x, y = filler.images(3, 64).cuda(), filler.labels(3, 10).cuda()
    losses, grads = [], None
    for step in range(int(steps)):
        ts.step(x, y)
        losses.append(ts.loss())
        if step == 0:
            grads = _device_grads(ts)
    names = {k[len("grad/"):] for k in g.files if k.startswith("grad/")}
    assert set(grads) == names and {"1.weight", "1.bias"} <= names
    worst = (0.0, None)
    for k in sorted(names):
        ref = U.t(g["grad/" + k]).float()
        e = _gerr(grads[k], ref)
        b = 4 * F32_TOL if dtype == torch.float32 else min(4 * float(g[f"floor/bf16/grad/{k}"]), 0.25)
        worst = max(worst, (e / b, k))
        print(f"{dtype}: grad {k} {e:.3e} (bound {b:.3e})")
        assert e < b, f"grad {k}: {e} >= {b}"
    print(f"{dtype}: worst gradient {worst[1]} at {worst[0]:.2f} of its bound")
    ref_losses = [float(v) for v in g["loss64"]]
    print(f"{dtype}: losses {losses} against {ref_losses}: relative "
          f"{[abs(a - b) / b for a, b in zip(losses, ref_losses)]}")
    assert ref_losses[0] > ref_losses[1] > ref_losses[2]
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-3 if dtype == torch.float32 else 1e-2)


# ---- 4. validate() -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_validate_matches_the_cpu_model_and_leaves_the_state_alone(dtype):
    ts = _fixture_step(dtype, "adamw.", lr=1e-4)
    x, y = filler.images(3, 64), filler.labels(3, 10)
    ts.step(x.cuda(), y.cuda())  # (so that the moments and the step count are not trivially zero)
    torch.cuda.synchronize()
    state = [t.clone() for t in (ts.store.pflat, ts.mflat, ts.vflat, ts.lr_dev, ts.store.mirror)]
    val = ts.validate(x.cuda(), y.cuda())
    m = _cpu_model(ts.model.state_dict(), torch.float64).eval()
    with torch.no_grad():
        logits = m(x.double())
    ref_loss = F.cross_entropy(logits, y).item()  # (no label smoothing, classifier.py:103)
    ref_hits = int((logits.argmax(-1) == y).sum())
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    print(f"{dtype}: validation loss {val['loss']:.6f} against {ref_loss:.6f}, top-1 {val['correct']} against {ref_hits}")
    assert val["count"] == 3 and val["correct"] == ref_hits
    assert abs(val["loss"] - ref_loss) < tol * abs(ref_loss)
    assert tuple(ts.eval_logits().shape) == (3, 10)
    for t, keep in zip((ts.store.pflat, ts.mflat, ts.vflat, ts.lr_dev, ts.store.mirror), state):
        assert torch.equal(t, keep)
    assert ts.opt_steps() == 1 and ts.mflat.any() and ts.vflat.any()


# ---- 5. SGD is unchanged -----------------------------------------------------------------------------------------------
def test_sgd_default_builds_the_same_optimiser_list():
    a = TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cuda")
    b = TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cuda", optimizer="SGD")
    assert a.vflat is None and b.vflat is None and a.n_opt == b.n_opt == len(a.segments)
    raw = [ctypes.string_at(ctypes.addressof(t.opt_ops), t.n_opt * ctypes.sizeof(N.Op)) for t in (a, b)]
    assert raw[0] == raw[1]  # kinds, (base, offset) pointers, scalars
    assert all(a.opt_ops[k].kind == N.OP_SGD for k in range(a.n_opt))
