"""ConvNeXt through the module API on the GPU against the fixtures of tools/gen_golden_convnext.py (the unmodified reference
on CPU): cases a, b, c x {f32, bf16}, forward + backward with the fixture's projections of both outputs.

Bounds.  f32: the project's module bounds (test_modules_gpu.py: F32_TOL 2e-4 forward, 4x for dx and parameter gradients, with
its clamp_min(1e-3 sqrt(numel)) denominator); the reference's own float32 error against float64 (stored under floor/f32) is
two orders below.  bf16: forward the project's BF16_TOL 3e-2; dx and parameter gradients 4 x the stored floor of the SAME
array -- the error of the reference under torch.autocast("cpu", bfloat16) with every module output rounded to bf16, against
float64 -- and never above the project's 0.25.  The factor 4 is for what the GPU path rounds and that reference does not: the
weight mirror, the stored pre-activations and every stored gradient are bf16 here.  (The module-output rounding is part of
the floor because plain autocast hands back float32 outputs: the gradient of the head norm's bias -- the column sums of the
projection, which never touch the network -- then has a floor of 1e-7, while this path's output tensor is bf16 and receives
the projection rounded to bf16: 1.7e-3 measured, format noise of the seed and no property of the kernels.)"""
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox.backbones import ConvNeXt

import convnext_util as U

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 2e-4, 3e-2
DTYPES = [torch.float32, torch.bfloat16]


def _gerr(got, ref):
    return ((got.float().cpu() - ref).norm() / ref.norm().clamp_min(1e-3 * (ref.numel() ** 0.5))).item()


def _gtol(g, dtype, key):
    if dtype == torch.float32:
        return 4 * F32_TOL
    return min(4 * float(g[f"floor/bf16/{key}"]), 0.25)


def _setup(name, dtype):
    g = U.load(name)
    m = U.build(name)
    pre, x, r, rf = U.inputs(g)
    U.fill(m, pre)
    m = m.cuda()
    m.compute_dtype = dtype
    return g, m, x.cuda().requires_grad_(True), r.cuda(), rf.cuda()


def _fwd_bwd(m, x, r, rf):
    y = m(x)
    f = m.get_feature_maps(x)
    assert isinstance(f, list) and len(f) == 1
    f = f[0]
    ((y.float() * r).sum() + (f.float() * rf).sum()).backward()
    torch.cuda.synchronize()
    return y, f


def _check_grads(g, m, x, dtype, tag, frozen=()):
    worst = 0.0
    e, b = _gerr(x.grad, U.t(g["dx"])), _gtol(g, dtype, "dx")
    print(f"{tag}: dx {e:.3e} (bound {b:.3e})")
    assert e < b, "dx"
    for k, p in m.named_parameters():
        if k.startswith(frozen):
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        e, b = _gerr(p.grad, U.t(g["grad/" + k])), _gtol(g, dtype, "grad/" + k)
        worst = max(worst, e / b)
        print(f"{tag}: grad {k} {e:.3e} (bound {b:.3e})")
        assert e < b, f"grad {k}: {e} >= {b}"
    print(f"{tag}: worst parameter gradient at {worst:.2f} of its bound")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_forward_backward_match_the_reference(name, dtype):
    g, m, x, r, rf = _setup(name, dtype)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    y, f = _fwd_bwd(m, x, r, rf)
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2 and y.dtype == dtype
    assert tuple(f.shape) == g["f"].shape and f.dim() == 4 and f.shape[-1] == y.shape[-1]
    ey, ef = U.rel(y.detach().float().cpu(), U.t(g["y"])), U.rel(f.detach().float().cpu(), U.t(g["f"]))
    print(f"{name}/{dtype}: y {ey:.3e} f {ef:.3e} (bound {tol:.1e})")
    assert ey < tol and ef < tol
    _check_grads(g, m, x, dtype, f"{name}/{dtype}")
    if name == "b":
        # the 4x4 stem reads rows 0..35 and columns 0..27 of the 38x30 image, and the 9x7 map loses a row and a column
        # in the 2x2 downsample: image rows / columns nothing reads have an exactly zero gradient, as in the reference
        ref = U.t(g["dx"])
        assert (ref[:, :, 36:, :] == 0).all() and (ref[:, :, :, 28:] == 0).all()
        dx = x.grad.cpu()
        assert (dx[:, :, 36:, :] == 0).all() and (dx[:, :, :, 28:] == 0).all()
        assert (dx[:, :, :36, :28] != 0).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_no_grad_forward(name, dtype):
    g, m, x, _, _ = _setup(name, dtype)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    with torch.no_grad():
        y, f = m(x), m.get_feature_maps(x)[0]
    torch.cuda.synchronize()
    assert N.launch_count() > before
    assert not y.requires_grad and tuple(f.shape) == g["f"].shape
    assert U.rel(y.float().cpu(), U.t(g["y"])) < tol and U.rel(f.float().cpu(), U.t(g["f"])) < tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_frozen_stem(dtype):
    g, m, x, r, rf = _setup("a", dtype)
    m.stem.requires_grad_(False)
    _fwd_bwd(m, x, r, rf)
    _check_grads(g, m, x, dtype, f"frozen stem/{dtype}", frozen=("stem.",))


def test_refusals_on_a_cuda_tensor():
    x = torch.randn(2, 3, 32, 32, device="cuda")
    with pytest.raises(NotImplementedError, match="GlobalResponseNorm"):
        ConvNeXt(16, (1, 1), v2=True).cuda()(x)
    m = ConvNeXt(16, (1, 1), stochastic_depth=0.1).cuda().train()
    with pytest.raises(NotImplementedError, match="stochastic_depth"):
        m(x)
    with pytest.raises(NotImplementedError, match="stochastic_depth"):
        m.get_feature_maps(x)
    assert m.eval()(x).shape == (2, 32)  # (drop rate unused in eval mode)
    with pytest.raises(NotImplementedError, match="stochastic_depth"):
        m.train()(x)  # (the refusal does not depend on what was compiled before)


def test_case_a_f32_matches_its_own_cpu_eager_path():
    """a wiring check (the parity evidence is the fixture comparison above)"""
    g = U.load("a")
    pre, x, r, rf = U.inputs(g)
    res = {}
    for dev in ("cpu", "cuda"):
        m = U.build("a")
        U.fill(m, pre)
        m = m.to(dev)
        xd = x.detach().clone().to(dev).requires_grad_(True)
        y, f = m(xd), m.get_feature_maps(xd)[0]
        ((y * r.to(dev)).sum() + (f * rf.to(dev)).sum()).backward()
        res[dev] = [y.detach().cpu(), f.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu() for p in m.parameters()]
    for a, b in zip(res["cuda"], res["cpu"]):
        assert _gerr(a, b) < 4 * F32_TOL
