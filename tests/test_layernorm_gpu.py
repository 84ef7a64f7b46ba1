"""vt_layernorm_fwd / vt_layernorm_bwd / vt_scale_residual_fwd / vt_scale_residual_bwd / vt_channel_sums_to_f32
(vt_layernorm.hip) through the C-ABI against torch in float64 on the same (storage-rounded) operands: nn.LayerNorm(C) over
the last axis of an NHWC map and `residual + gamma * t` with their autograd backward (reference backbones/convnext.py:48,
53, 58).

Channel counts from one chunk per row (8) over rows that are not a power of two of chunks (40, 96, 352) to several chunks per
lane (768, 2816); row counts that are a multiple of nothing, two rows (the head), and enough rows that a workgroup visits
more than one (the per-lane channel sums across the row loop); channel-slice operands (pixel stride > C: the NaN-filled
surroundings must stay NaN); pre_bias on and off; the residual aliasing dx.

Bounds: gpu_util.tol (2e-5 f32, 6e-3 bf16) for y and dx, twice that with a residual (two roundings); the channel sums go
through the fixed-point buffer, so they are compared at 1e-6 of their scale sum |terms| (the bound test_dwconv_gpu.py uses
for the statistics), which is f32 rounding of the terms themselves.  Measured on an MI355X: <= 2e-8 of scale wherever hundreds
of rows average the rounding of the terms; with two rows nothing averages and the f32 rounding of a term is a visible fraction
of a channel's scale -- 1.15e-6 with the row mean held in f32 (which is why vt_layernorm_bwd takes the deviations against
the mean in double), 1.5e-7 .. 5.9e-7 since."""
import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, rel_err, stream, tol, vp

pytestmark = pytest.mark.gpu

EPS = 1e-6
# C, M
CASES = [
    (8, 3 * 19 * 23),
    (40, 3 * 19 * 23),
    (96, 3 * 19 * 23),
    (352, 3 * 19 * 23),
    (768, 3 * 19 * 23),
    (768, 2),
    (2816, 3 * 47 * 61),
    (16, 7 * 211 * 199),  # more rows than one sweep of the grid: every workgroup loops
]


def _slice(M, C, td, off, extra, fill=None):
    """[M][C] operand inside a NaN-filled [M][C + extra] buffer (extra = 0: dense)"""
    wide = torch.full((M, C + extra), float("nan"), device="cuda", dtype=td)
    view = wide[:, off:off + C] if extra else wide
    if fill is not None:
        view.copy_(fill)
    return wide, view


def _nan_outside(wide, off, C):
    return bool(torch.isnan(wide[:, :off].float()).all() and torch.isnan(wide[:, off + C:].float()).all())


def _sums(rows, C):
    return torch.zeros(N.VT_STAT_REPLICAS, rows, C, 2, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layernorm_matches_torch_float64(case, dtype):
    C, M = case
    torch.manual_seed(C + M)
    td, lib, t_ = TD[dtype], N.lib(), tol(dtype)
    ex = (16, 32, 48) if C <= 768 else (0, 0, 0)  # pixel strides C + 16 / 32 / 48, operand at element 8 / 16 / 24
    _, x = _slice(M, C, td, 8, ex[0], torch.randn(M, C, device="cuda") * 1.5 + 0.3)
    _, dy = _slice(M, C, td, 16, ex[1], torch.randn(M, C, device="cuda"))
    gamma = (1.0 + 0.5 * torch.randn(C, device="cuda")).contiguous()
    beta = (0.2 * torch.randn(C, device="cuda")).contiguous()
    pb = (0.3 * torch.randn(C, device="cuda")).contiguous()
    res = torch.randn(M, C, device="cuda").to(td)
    for with_pb in (False, True):
        u = (x.double() + (pb.double() if with_pb else 0.0)).requires_grad_(True)
        g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        ref = F.layer_norm(u, (C,), g64, b64, EPS)
        ref.backward(dy.double())
        # ---- forward
        ywide, y = _slice(M, C, td, 24, ex[2])
        N.check(lib.vt_layernorm_fwd(vp(x), x.stride(0), vp(pb) if with_pb else None, vp(gamma), vp(beta), vp(y), y.stride(0),
                                     M, C, EPS, dtype, stream()))
        torch.cuda.synchronize()
        e = rel_err(y, ref.detach())
        print(f"C={C} M={M} pre_bias={with_pb}: y {e:.2e}")
        assert e < t_
        if ex[2]:
            assert _nan_outside(ywide, 24, C)
        # ---- backward: plain, then with the residual aliasing dx
        sums = _sums(3, C)
        dxwide, dx = _slice(M, C, td, 8, ex[0])
        if with_pb:
            dx.copy_(res)
        N.check(lib.vt_layernorm_bwd(vp(dy), dy.stride(0), vp(x), x.stride(0), vp(pb) if with_pb else None, vp(gamma), vp(dx),
                                     dx.stride(0), vp(dx) if with_pb else None, dx.stride(0) if with_pb else 0, vp(sums), M, C,
                                     EPS, dtype, stream()))
        torch.cuda.synchronize()
        want_dx = u.grad + (res.double() if with_pb else 0.0)
        e = rel_err(dx, want_dx)
        print(f"C={C} M={M} pre_bias={with_pb}: dx {e:.2e}")
        assert e < (2 * t_ if with_pb else t_)
        if ex[0]:
            assert _nan_outside(dxwide, 8, C)
        got = N.stats_decode(sums)  # [3][C]
        mean = u.detach().mean(1, keepdim=True)
        xhat = (u.detach() - mean) / (u.detach().var(1, unbiased=False, keepdim=True) + EPS).sqrt()
        terms = [dy.double() * xhat, dy.double(), u.grad]
        for k in range(3 if with_pb else 2):
            want, scale = terms[k].sum(0), terms[k].abs().sum(0).clamp_min(1e-30)
            e = ((got[k] - want).abs() / scale).max().item()
            print(f"C={C} M={M} pre_bias={with_pb}: sums[{k}] {e:.2e} of scale")
            assert e < 1e-6
        if not with_pb:
            assert (got[2] == 0).all()
        assert rel_err(got[0], g64.grad) < 1e-5 and rel_err(got[1], b64.grad) < 1e-5
        # ---- the fold into f32 gradients (accumulating)
        d = [torch.full((C,), 0.5, device="cuda") for _ in range(3)]
        N.check(lib.vt_channel_sums_to_f32(vp(sums), 3, C, vp(d[0]), None, vp(d[2]), stream()))
        torch.cuda.synchronize()
        assert torch.allclose(d[0].double() - 0.5, got[0], rtol=1e-6, atol=1e-6 * float(got[0].abs().max() + 1))
        assert (d[1] == 0.5).all()
        assert torch.allclose(d[2].double() - 0.5, got[2], rtol=1e-6, atol=1e-6 * float(got[2].abs().max() + 1))


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_constant_row_gives_finite_output(dtype):
    C, M, td = 96, 37, TD[dtype]
    x = torch.randn(M, C, device="cuda").to(td)
    x[5] = 0.75  # variance exactly 0
    gamma, beta = torch.full((C,), 1.5, device="cuda"), torch.linspace(-1, 1, C, device="cuda").contiguous()
    y = torch.full((M, C), float("nan"), device="cuda", dtype=td)
    N.check(N.lib().vt_layernorm_fwd(vp(x), C, None, vp(gamma), vp(beta), vp(y), C, M, C, EPS, dtype, stream()))
    dx = torch.full((M, C), float("nan"), device="cuda", dtype=td)
    sums = _sums(3, C)
    dy = torch.randn(M, C, device="cuda").to(td)
    N.check(N.lib().vt_layernorm_bwd(vp(dy), C, vp(x), C, None, vp(gamma), vp(dx), C, None, 0, vp(sums), M, C, EPS, dtype, stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
    assert rel_err(y[5], beta.to(td)) < tol(dtype)  # xhat = 0: the row is beta
    assert torch.isfinite(N.stats_decode(sums)).all()


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_scale_residual_matches_torch_float64(case, dtype):
    C, M = case
    torch.manual_seed(C + M + 1)
    td, lib, t_ = TD[dtype], N.lib(), tol(dtype)
    ex = (16, 32, 48) if C <= 768 else (0, 0, 0)
    _, t = _slice(M, C, td, 8, ex[0], torch.randn(M, C, device="cuda"))
    _, res = _slice(M, C, td, 16, ex[1], torch.randn(M, C, device="cuda"))
    gamma = (1.0 + 0.5 * torch.randn(C, device="cuda")).contiguous()
    for with_gamma in (True, False):
        ywide, y = _slice(M, C, td, 24, ex[2])
        N.check(lib.vt_scale_residual_fwd(vp(t), t.stride(0), vp(gamma) if with_gamma else None, vp(res), res.stride(0), vp(y),
                                          y.stride(0), M, C, dtype, stream()))
        torch.cuda.synchronize()
        want = res.double() + t.double() * (gamma.double() if with_gamma else 1.0)
        e = rel_err(y, want)
        print(f"C={C} M={M} gamma={with_gamma}: y {e:.2e}")
        assert e < t_
        if ex[2]:
            assert _nan_outside(ywide, 24, C)
    _, dy = _slice(M, C, td, 16, ex[1], torch.randn(M, C, device="cuda"))
    dtwide, dt = _slice(M, C, td, 24, ex[2])
    sums = _sums(1, C)
    N.check(lib.vt_scale_residual_bwd(vp(dy), dy.stride(0), vp(t), t.stride(0), vp(gamma), vp(dt), dt.stride(0), vp(sums), M, C,
                                      dtype, stream()))
    torch.cuda.synchronize()
    e = rel_err(dt, dy.double() * gamma.double())
    print(f"C={C} M={M}: dt {e:.2e}")
    assert e < t_
    if ex[2]:
        assert _nan_outside(dtwide, 24, C)
    terms = dy.double() * t.double()
    got = N.stats_decode(sums)[0]
    e = ((got - terms.sum(0)).abs() / terms.abs().sum(0).clamp_min(1e-30)).max().item()
    print(f"C={C} M={M}: sums {e:.2e} of scale")
    assert e < 1e-6
    dg = torch.zeros(C, device="cuda")
    N.check(lib.vt_channel_sums_to_f32(vp(sums), 1, C, vp(dg), None, None, stream()))
    torch.cuda.synchronize()
    assert torch.allclose(dg.double(), got, rtol=1e-6, atol=1e-6 * float(got.abs().max() + 1))


def test_arguments_are_checked():
    lib = N.lib()
    x = torch.zeros(4, 16, device="cuda", dtype=torch.bfloat16)
    y = torch.zeros(4, 16, device="cuda", dtype=torch.bfloat16)
    g = torch.ones(16, device="cuda")
    s = _sums(3, 16)
    assert lib.vt_layernorm_fwd(vp(x), 16, None, vp(g), vp(g), vp(y), 16, 4, 12, EPS, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED  # C % 8
    assert lib.vt_layernorm_fwd(vp(x), 16, None, vp(g), vp(g), vp(y), 16, 4, 6, EPS, N.VT_F32, stream()) == N.VT_ERR_UNSUPPORTED  # C % 4
    assert lib.vt_layernorm_fwd(vp(x), 16, None, vp(g), vp(g), vp(y), 16, 4, 4096, EPS, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_layernorm_fwd(vp(x), 8, None, vp(g), vp(g), vp(y), 16, 4, 16, EPS, N.VT_BF16, stream()) == N.VT_ERR_INVALID  # ld < C
    assert lib.vt_layernorm_fwd(vp(x), 16, None, vp(g), vp(g), None, 16, 4, 16, EPS, N.VT_BF16, stream()) == N.VT_ERR_INVALID
    assert "vt_layernorm_fwd" in N.last_error()
    assert lib.vt_layernorm_bwd(vp(x), 16, vp(x), 16, None, vp(g), vp(y), 16, None, 0, None, 4, 16, EPS, N.VT_BF16, stream()) == N.VT_ERR_INVALID
    assert "vt_layernorm_bwd" in N.last_error()
    assert lib.vt_scale_residual_fwd(vp(x), 16, vp(g), None, 16, vp(y), 16, 4, 16, N.VT_BF16, stream()) == N.VT_ERR_INVALID
    assert "vt_scale_residual_fwd" in N.last_error()
    assert lib.vt_scale_residual_bwd(vp(x), 16, vp(x), 16, None, vp(y), 16, vp(s), 4, 16, N.VT_BF16, stream()) == N.VT_ERR_INVALID
    assert "vt_scale_residual_bwd" in N.last_error()
    assert lib.vt_channel_sums_to_f32(vp(s), 4, 16, vp(g), None, None, stream()) == N.VT_ERR_INVALID
    N.check(lib.vt_layernorm_fwd(vp(x), 16, None, vp(g), vp(g), vp(y), 16, 4, 16, EPS, N.VT_BF16, stream()))
    torch.cuda.synchronize()
