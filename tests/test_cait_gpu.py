"""CaiT through the module API and the fused train step on the GPU against the fixtures of tools/gen_golden_cait.py /
tools/gen_golden_cait_train.py (the unmodified reference on CPU, one image at a time: this class broadcasts the class token
over the batch): cases a, b, c x {f32, bf16}.

Bounds are those of tests/test_vit_gpu.py, unchanged.  f32: F32_TOL 2e-4 forward, 4 x for dx and parameter gradients, with the
clamp_min(1e-3 sqrt(numel)) denominator.  bf16: forward BF16_TOL 3e-2; dx and parameter gradients min(4 x the stored floor of
the SAME array, 0.25).  The parameters the fixture lists under `zero_grad_keys` (every `k_proj.bias` and every pre-softmax
mixing bias `talking_head_proj.0.bias`: exactly zero in exact arithmetic, noise in every rounded run) are skipped, after
asserting that they are exactly those; tests/test_talking_attention_gpu.py covers dK where it is not zero.  Train step: the
three losses at rtol 1e-3 (f32) / 1e-2 (bf16), the step-1 gradients at the bounds above."""
import numpy as np
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox.backbones import CaiT
from vision_toolbox.trainer import TrainStep

from oracle import filler

import cait_util as U

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 2e-4, 3e-2
DTYPES = [torch.float32, torch.bfloat16]


def _gtol(g, dtype, key):
    if dtype == torch.float32:
        return 4 * F32_TOL
    return min(4 * float(g[f"floor/bf16/{key}"]), 0.25)


def _zero(name, g):
    return U.zero_keys(g, U.CASES[name][0][1], U.CASES[name][0][2])


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
        e, b = U.gerr(p.grad, U.t(g["grad/" + k])), _gtol(g, dtype, "grad/" + k)
        worst = max(worst, e / b)
        print(f"{tag}: grad {k} {e:.3e} (bound {b:.3e})")
        assert e < b, f"grad {k}: {e} >= {b}"
    print(f"{tag}: worst parameter gradient at {worst:.2f} of its bound")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_forward_backward_match_the_reference(name, dtype):
    g, m, x, r = _setup(name, dtype)
    zero = _zero(name, g)
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
    g, m, x, r = _setup("c", dtype)  # two class-attention blocks read the patch map
    m.patch_embed.requires_grad_(False)
    x = x.detach()  # nothing in front of the embedding needs a gradient: no patch scatter, no embedding gradients
    y = m(x)
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    _check_grads(g, m, x, dtype, f"frozen patch_embed/{dtype}", _zero("c", g), frozen=("patch_embed.",))


def test_refusals_on_a_cuda_tensor():
    x = torch.randn(2, 3, 16, 16, device="cuda")
    for kw, match in (({"dropout": 0.1}, "dropout"), ({"stochastic_depth": 0.1}, "stochastic_depth")):
        m = CaiT(96, 1, 1, 2, 4, 16, **kw).cuda().train()
        with pytest.raises(NotImplementedError, match=match):
            m(x)
        assert m.eval()(x).shape == (2, 96)  # (unused in eval mode)
        with pytest.raises(NotImplementedError, match=match):
            m.train()(x)  # (the refusal does not depend on what was compiled before)
    m = CaiT(96, 1, 1, 2, 4, 16).cuda().eval()
    with pytest.raises(ValueError, match="patches"):
        m(torch.randn(2, 3, 32, 32, device="cuda"))
    with pytest.raises(NotImplementedError, match="bias=False"):
        CaiT(96, 1, 1, 2, 4, 16, bias=False).cuda()(x)
    with pytest.raises(NotImplementedError, match="head_dim"):
        CaiT(64, 1, 1, 2, 4, 16).cuda()(x)
    with pytest.raises(NotImplementedError, match="n_heads"):
        CaiT(48 * 17, 1, 1, 17, 4, 16).cuda()(x)
    # (a d_model that is no multiple of the 16-byte chunk cannot have head_dim 48: the head_dim refusal names it first)
    with pytest.raises(NotImplementedError, match="head_dim"):
        CaiT(100, 1, 1, 2, 4, 16).cuda()(x)


def test_resize_pe_retargets_the_gpu_path():
    """pe is replaced by a new, longer parameter: the store and the compiled programs must follow"""
    m = CaiT(96, 1, 1, 2, 4, 16)
    U.fill(m, "cait_resize_gpu.")
    m = m.cuda().eval()
    x = filler.tensor("cait_resize_gpu.x", (2, 3, 32, 32))
    with torch.no_grad():
        m(x[:, :, :16, :16].contiguous().cuda())
        m.resize_pe(32)
        y = m(x.cuda())
        with pytest.raises(ValueError, match="patches"):
            m(x[:, :, :16, :16].contiguous().cuda())
        want = m.cpu()(x)
    e = U.rel(y.float().cpu(), want)
    print(f"after resize_pe: gpu vs own cpu path {e:.3e} (bound {F32_TOL:.1e})")
    assert tuple(y.shape) == (2, 96) and e < F32_TOL


def _train_step(g, dtype, **kw):
    lr, wd, norm_wd, bias_wd, smooth, _ = [float(v) for v in g["hyper"]]
    m = CaiT(*U.TRAIN_ARGS, **U.TRAIN_KW)
    ts = TrainStep(m, 10, 3, 16, dtype, lr=lr, weight_decay=wd, norm_weight_decay=norm_wd, bias_weight_decay=bias_wd,
                   label_smoothing=smooth, optimizer="AdamW", include_pool=False, device="cuda", **kw)
    pre = str(g["recipe"][0])
    with torch.no_grad():
        filler.fill_module(ts.model, pre)
        for k, p in ts.model[0].named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)
    ts.weights_changed()
    assert list(ts.model.state_dict().keys()) == [str(k) for k in g["keys"]]
    return ts


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_three_adamw_steps_match_the_reference(dtype, deterministic):
    g = np.load(U.GOLDEN / "cait_train.npz")
    zero = U.zero_keys(g, 1, 1, prefix="0.")
    ts = _train_step(g, dtype, deterministic=deterministic)
    images, labels = filler.images(3, 16).cuda(), filler.labels(3, 10).cuda()
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
                e = U.gerr(got, U.t(g["grad/" + k]).float())
                worst = max(worst, e / b)
                print(f"train/{dtype}: step-1 grad {k} {e:.3e} (bound {b:.3e})")
                assert e < b, k
            print(f"train/{dtype}: worst step-1 gradient at {worst:.2f} of its bound")
    want = [float(v) for v in g["loss64"]]
    for a, b in zip(losses, want):
        print(f"train/{dtype} deterministic={deterministic}: loss {a:.6f} reference {b:.6f} rel {abs(a - b) / b:.2e} (rtol {rtol:.0e})")
    for a, b in zip(losses, want):
        assert abs(a - b) <= rtol * abs(b)


def test_deterministic_steps_are_bit_identical():
    g = np.load(U.GOLDEN / "cait_train.npz")
    images, labels = filler.images(3, 16).cuda(), filler.labels(3, 10).cuda()
    finals = []
    for _ in range(2):
        ts = _train_step(g, torch.bfloat16, deterministic=True)
        for _ in range(2):
            ts.step(images, labels)
        torch.cuda.synchronize()
        finals.append(ts.store.pflat.clone())
    assert torch.equal(finals[0], finals[1])
