"""Swin Transformer through the module API and the fused train step on the GPU against the fixtures of
tools/gen_golden_swin.py / tools/gen_golden_swin_train.py (the unmodified reference on CPU; one image at a time wherever a
block is shifted, whose mask this class tiles over the batch): cases a, b, c x {f32, bf16}.

Bounds are those of tests/test_vit_gpu.py, unchanged; parameter gradients are compared at the elements the fixtures store
(swin_util.sample: every parameter, every s-th element of the large ones).  f32: F32_TOL 2e-4 forward, 4 x for dx and parameter gradients, with
the clamp_min(1e-3 sqrt(numel)) denominator.  bf16: forward BF16_TOL 3e-2; dx and parameter gradients min(4 x the stored floor
of the SAME array, 0.25) -- the floor is the reference's own error under bf16 autocast with bf16 module outputs against
float64, in the same clamped metric.  The parameters the fixture lists under `zero_grad_keys` (every `k_proj.bias`: a constant
added to every key shifts each row of scores by a constant, which softmax ignores) are skipped, after asserting that they are
exactly those; tests/test_window_attention_gpu.py covers dK where it is not zero.  Train step: the three losses at the rtol of
tests/test_adamw_gpu.py (1e-3 f32, 1e-2 bf16), the step-1 gradients at the bounds above."""
import numpy as np
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox.backbones import SwinTransformer
from vision_toolbox.trainer import TrainStep

from oracle import filler

import swin_util as U

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 2e-4, 3e-2
DTYPES = [torch.float32, torch.bfloat16]


def _gtol(g, dtype, key):
    if dtype == torch.float32:
        return 4 * F32_TOL
    return min(4 * float(g[f"floor/bf16/{key}"]), 0.25)


def _setup(name, dtype):
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    m = m.cuda()
    m.compute_dtype = dtype
    return g, m, x.cuda().requires_grad_(True), r.cuda()


def _check_grads(g, m, x, dtype, tag, zero, frozen=()):
    worst = 0.0
    if x.grad is not None:
        e, b = U.gerr(x.grad, U.t(g["dx"])), _gtol(g, dtype, "dx")
        print(f"{tag}: dx {e:.3e} (bound {b:.3e})")
        assert e < b, "dx"
    for k, p in m.named_parameters():
        if k.startswith(frozen):
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        if k in zero:
            print(f"{tag}: grad {k} skipped (exactly zero in exact arithmetic): rms {p.grad.float().pow(2).mean().sqrt().item():.3e}")
            continue
        e, b = U.gerr(U.sample(p.grad), U.t(g["grad/" + k])), _gtol(g, dtype, "grad/" + k)
        worst = max(worst, e / b)
        print(f"{tag}: grad {k} {e:.3e} (bound {b:.3e})")
        assert e < b, f"grad {k}: {e} >= {b}"
    print(f"{tag}: worst parameter gradient at {worst:.2f} of its bound")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_forward_backward_match_the_reference(name, dtype):
    g, m, x, r = _setup(name, dtype)
    zero = U.zero_keys(g, m)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    y = m(x)
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2 and y.dtype == dtype
    ey = U.rel(y.detach().float().cpu(), U.t(g["y"]))
    print(f"{name}/{dtype}: y {ey:.3e} (bound {tol:.1e})")
    assert ey < tol
    _check_grads(g, m, x, dtype, f"{name}/{dtype}", zero)


@pytest.mark.parametrize("name", list(U.CASES))
def test_feature_maps_match_the_cpu_eager_path(name):
    g, m, x, _ = _setup(name, torch.float32)
    before = N.launch_count()
    with torch.no_grad():
        maps = m.get_feature_maps(x)
        torch.cuda.synchronize()
        assert N.launch_count() > before
        want = m.cpu().get_feature_maps(x.detach().cpu())
    assert [list(f.shape) for f in maps] == g["map_shapes"].tolist() == [list(f.shape) for f in want]
    for i, (a, b) in enumerate(zip(maps, want)):
        e = U.rel(a.float().cpu(), b)
        print(f"{name}: stage {i} map {tuple(a.shape)} gpu vs own cpu path {e:.3e} (bound {F32_TOL:.1e})")
        assert e < F32_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_no_grad_forward(name, dtype):
    g, m, x, _ = _setup(name, dtype)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert N.launch_count() > before
    e = U.rel(y.float().cpu(), U.t(g["y"]))
    print(f"{name}/{dtype} no-grad: y {e:.3e} (bound {tol:.1e})")
    assert not y.requires_grad and tuple(y.shape) == g["y"].shape and e < tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_frozen_patch_embed(dtype):
    g, m, x, r = _setup("a", dtype)
    m.patch_embed.requires_grad_(False)
    x = x.detach()  # nothing in front of the embedding needs a gradient: no patch scatter, no embedding gradients
    y = m(x)
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    _check_grads(g, m, x, dtype, f"frozen patch_embed/{dtype}", U.zero_keys(g, m), frozen=("patch_embed.",))


def test_refusals_on_a_cuda_tensor():
    x = torch.randn(2, 3, 32, 32, device="cuda")
    args = (32, 32, 1, (2,), (4,))
    for kw, match in (({"dropout": 0.1}, "dropout"), ({"stochastic_depth": 0.1}, "stochastic_depth")):
        m = SwinTransformer(*args, **kw).cuda().train()
        with pytest.raises(NotImplementedError, match=match):
            m(x)
        assert m.eval()(x).shape == (2, 32)  # (unused in eval mode)
        with pytest.raises(NotImplementedError, match=match):
            m.train().get_feature_maps(x)  # (the refusal does not depend on what was compiled before)
    with pytest.raises(ValueError, match="64x64"):
        SwinTransformer(*args).cuda()(torch.randn(2, 3, 64, 64, device="cuda"))
    with pytest.raises(NotImplementedError, match="window_size=14"):
        SwinTransformer(224, 32, 1, (1,), (14,)).cuda()(torch.randn(1, 3, 224, 224, device="cuda"))
    with pytest.raises(NotImplementedError, match="head_dim"):
        SwinTransformer(32, 64, 1, (1,), (4,)).cuda()(x)
    with pytest.raises(NotImplementedError, match="head_dim"):
        SwinTransformer(32, 32, 2, (1,), (4,)).cuda()(x)
    with pytest.raises(NotImplementedError, match="bias=False"):
        SwinTransformer(32, 32, 1, (1,), (4,), bias=False).cuda()(x)


def _train_step(g, dtype, **kw):
    lr, wd, norm_wd, bias_wd, smooth, _ = [float(v) for v in g["hyper"]]
    m = SwinTransformer(*U.TRAIN_ARGS, **U.TRAIN_KW)
    ts = TrainStep(m, 10, 2, 48, dtype, lr=lr, weight_decay=wd, norm_weight_decay=norm_wd, bias_weight_decay=bias_wd,
                   label_smoothing=smooth, optimizer="AdamW", include_pool=False, device="cuda", **kw)
    pre = str(g["recipe"][0])
    with torch.no_grad():
        filler.fill_module(ts.model, pre)
    U.fill_backbone(ts.model[0])
    ts.weights_changed()
    assert list(ts.model.state_dict().keys()) == [str(k) for k in g["keys"]]
    return ts


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_three_adamw_steps_match_the_reference(dtype, deterministic):
    g = np.load(U.GOLDEN / "swin_train.npz")
    ts = _train_step(g, dtype, deterministic=deterministic)
    zero = U.zero_keys(g, ts.model)
    images, labels = filler.images(2, 48).cuda(), filler.labels(2, 10).cuda()
    rtol = 1e-3 if dtype == torch.float32 else 1e-2
    losses = []
    for step in range(3):
        before = N.launch_count()
        ts.step(images, labels)
        losses.append(ts.loss())
        assert N.launch_count() > before
        if step == 0:
            torch.cuda.synchronize()
            worst = 0.0
            for k, p in ts.model.named_parameters():
                if k in zero:
                    continue
                _, off, n = ts.store.where(p)
                got = ts.gflat[off:off + n].view(p.shape if p.dim() != 4 else (p.shape[0], p.shape[2], p.shape[3], p.shape[1]))
                if p.dim() == 4:
                    got = got.permute(0, 3, 1, 2)
                b = 4 * F32_TOL if dtype == torch.float32 else min(4 * float(g[f"floor/bf16/grad/{k}"]), 0.25)
                e = U.gerr(U.sample(got), U.t(g["grad/" + k]).float())
                worst = max(worst, e / b)
                print(f"train/{dtype}: step-1 grad {k} {e:.3e} (bound {b:.3e})")
                assert e < b, k
            print(f"train/{dtype}: worst step-1 gradient at {worst:.2f} of its bound")
    want = [float(v) for v in g["loss64"]]
    for a, b in zip(losses, want):
        print(f"train/{dtype} deterministic={deterministic}: loss {a:.6f} reference {b:.6f} rel {abs(a - b) / b:.2e} (rtol {rtol:.0e})")
    for a, b in zip(losses, want):
        assert abs(a - b) <= rtol * abs(b)


def test_deterministic_steps_are_bit_identical_and_validate_runs():
    g = np.load(U.GOLDEN / "swin_train.npz")
    images, labels = filler.images(2, 48).cuda(), filler.labels(2, 10).cuda()
    finals = []
    for _ in range(2):
        ts = _train_step(g, torch.bfloat16, deterministic=True, mix=True)
        for _ in range(2):
            ts.step(images, labels)
        torch.cuda.synchronize()
        finals.append(ts.store.pflat.clone())
    assert torch.equal(finals[0], finals[1])
    ts.set_mix("none")
    val = ts.validate(images, labels)
    print(f"validate: {val}")
    assert np.isfinite(val["loss"]) and val["count"] == 2 and 0 <= val["correct"] <= 2
