"""vt_token_mix_fwd / vt_token_mix_wgrad / vt_patchify_fwd / vt_patchify_bwd (vt_token_mix.hip) through the C-ABI against
torch in float64 on the same (storage-rounded) operands, and a builder-level token MLP whose output is projected directly.

Shapes (K tokens in, M tokens out, C channels): Mixer-S/16 (196, 256, 512), B/32 (49, 384, 768), the fixtures' (25, 16, 32)
and (36, 24, 24), and (25, 16, 32) again as a channel slice of a wider buffer (row stride > C: the NaN-filled surroundings
must stay NaN).  W as stored and transposed (the data gradient's view of the same weight), with and without the fused GELU
output, with and without a residual, and the residual aliasing the output.

Bounds.  f32 outputs: the kernel tests' rtol 1e-4 with an atol of 1e-4 of the largest magnitude.  bf16 outputs:
norm-relative 2^-8 -- storing to bf16 rounds each element by at most 2^-9 relative, the fused GELU output is the activation
of the STORED pre-activation (a second rounding of the same size), and the f32 accumulation over K <= 784 adds under 1e-4.
The filter and bias gradients are f32 outputs: they take the f32 bound in both dtypes, against float64 of the same (bf16)
operands; their operands are shifted off zero so that the sums do not cancel.  Two runs of the filter gradient are
bit-identical (it has no atomic path).  The patch gather and scatter are copies: exact.

The linear2-style bias gradient (the one whose gradient vanishes inside a whole Mixer, see tools/gen_golden_mlp_mixer.py) is
checked here twice where it is not zero: as `dbias` of every filter-gradient case, and in the builder-level token MLP, whose
output feeds the loss with no LayerNorm behind it, against autograd in float64."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from vision_toolbox import _native as N
from vision_toolbox.components import HipModule

from gpu_util import TD, rel_err, stream, vp

pytestmark = pytest.mark.gpu

# K, M, C, B, extra row stride
SHAPES = [(196, 256, 512, 3, 0), (49, 384, 768, 2, 0), (25, 16, 32, 5, 0), (36, 24, 24, 4, 0), (25, 16, 32, 3, 40)]
IDS = ["196x256x512", "49x384x768", "25x16x32", "36x24x24", "25x16x32-ld"]
BF16_REL = 2.0 ** -8


def _map(B, T, C, td, extra, fill):
    """[B][T][C] operand inside a NaN-filled [B][T][C + extra] buffer (extra = 0: dense)"""
    wide = torch.full((B, T, C + extra), float("nan"), device="cuda", dtype=td)
    view = wide[:, :, 8:8 + C] if extra else wide
    if fill is not None:
        view.copy_(fill)
    return wide, view


def _nan_outside(wide, C, extra):
    return not extra or bool(torch.isnan(wide[:, :, :8].float()).all() and torch.isnan(wide[:, :, 8 + C:].float()).all())


def _check(tag, got, want, dtype, f32_out=False):
    got, want = got.double().cpu(), want.double().cpu()
    if dtype == N.VT_F32 or f32_out:
        atol = 1e-4 * want.abs().max().item()
        worst = ((got - want).abs() / (atol + 1e-4 * want.abs())).max().item()
        print(f"{tag}: worst |err| / (atol + rtol |ref|) = {worst:.3e} (bound 1), atol {atol:.3e}")
        assert worst < 1.0, tag
    else:
        e = rel_err(got, want)
        print(f"{tag}: norm-relative {e:.3e} (bound {BF16_REL:.3e})")
        assert e < BF16_REL, tag


def _fwd(lib, x, w, transw, bias, res, z, a, act, B, K, M, C, dtype):
    N.check(lib.vt_token_mix_fwd(vp(x), x.stride(1), vp(w), w.stride(0), int(transw), vp(bias), vp(res),
                                 res.stride(1) if res is not None else 0, vp(z), z.stride(1) if z is not None else 0, vp(a),
                                 a.stride(1) if a is not None else 0, act, B, K, M, C, dtype, stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_token_mix_forward_matches_torch_float64(shape, dtype):
    K, M, C, B, extra = shape
    torch.manual_seed(K * M + C)
    td, lib = TD[dtype], N.lib()
    _, x = _map(B, K, C, td, extra, torch.randn(B, K, C, device="cuda"))
    w = (torch.randn(M, K, device="cuda") / K ** 0.5).to(td).contiguous()
    bias = (0.5 * torch.randn(M, device="cuda")).contiguous()
    _, res = _map(B, M, C, td, extra, torch.randn(B, M, C, device="cuda"))
    z64 = torch.einsum("mk,bkc->bmc", w.double(), x.double()) + bias.double()[None, :, None]
    # plain: z alone
    zw, z = _map(B, M, C, td, extra, None)
    _fwd(lib, x, w, False, bias, None, z, None, 0, B, K, M, C, dtype)
    _check(f"{K}x{M}x{C} z", z, z64, dtype)
    assert _nan_outside(zw, C, extra)
    # fused GELU: the pre-activation and its activation from one launch; then the activation alone
    zw, z = _map(B, M, C, td, extra, None)
    aw, a = _map(B, M, C, td, extra, None)
    _fwd(lib, x, w, False, bias, None, z, a, 4, B, K, M, C, dtype)
    _check(f"{K}x{M}x{C} z (with gelu)", z, z64, dtype)
    _check(f"{K}x{M}x{C} gelu(z)", a, F.gelu(z64), dtype)
    assert _nan_outside(zw, C, extra) and _nan_outside(aw, C, extra)
    a2w, a2 = _map(B, M, C, td, extra, None)
    _fwd(lib, x, w, False, bias, None, None, a2, 4, B, K, M, C, dtype)
    assert torch.equal(a2.float(), a.float())
    # residual, then the residual aliasing the output, without a bias
    yw, y = _map(B, M, C, td, extra, None)
    _fwd(lib, x, w, False, bias, res, y, None, 0, B, K, M, C, dtype)
    _check(f"{K}x{M}x{C} residual + z", y, z64 + res.double(), dtype)
    assert _nan_outside(yw, C, extra)
    yw, y = _map(B, M, C, td, extra, res)
    _fwd(lib, x, w, False, None, y, y, None, 0, B, K, M, C, dtype)
    _check(f"{K}x{M}x{C} y += W x", y, z64 - bias.double()[None, :, None] + res.double(), dtype)
    assert _nan_outside(yw, C, extra)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_token_mix_transposed_weight_is_the_data_gradient(shape, dtype):
    """dx[b, k, c] = sum_m W[m, k] dz[b, m, c] (+ an accumulated gradient): the same kernel, W read transposed"""
    K, M, C, B, extra = shape
    torch.manual_seed(K + M * C)
    td, lib = TD[dtype], N.lib()
    w = (torch.randn(M, K, device="cuda") / M ** 0.5).to(td).contiguous()
    _, dz = _map(B, M, C, td, extra, torch.randn(B, M, C, device="cuda"))
    _, acc = _map(B, K, C, td, extra, torch.randn(B, K, C, device="cuda"))
    want = torch.einsum("mk,bmc->bkc", w.double(), dz.double())
    dxw, dx = _map(B, K, C, td, extra, None)
    _fwd(lib, dz, w, True, None, None, dx, None, 0, B, M, K, C, dtype)
    _check(f"{K}x{M}x{C} dx", dx, want, dtype)
    assert _nan_outside(dxw, C, extra)
    dxw, dx = _map(B, K, C, td, extra, acc)
    _fwd(lib, dz, w, True, None, dx, dx, None, 0, B, M, K, C, dtype)
    _check(f"{K}x{M}x{C} dx accumulated", dx, want + acc.double(), dtype)
    assert _nan_outside(dxw, C, extra)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_token_mix_wgrad_matches_torch_float64_and_is_bit_identical(shape, dtype):
    K, M, C, B, extra = shape
    torch.manual_seed(K * C + M)
    td, lib = TD[dtype], N.lib()
    # shifted off zero: sums of B * C products that do not cancel
    _, x = _map(B, K, C, td, extra, torch.randn(B, K, C, device="cuda") + 0.75)
    _, dz = _map(B, M, C, td, extra, torch.randn(B, M, C, device="cuda") + 0.5)
    want_w = torch.einsum("bmc,bkc->mk", dz.double(), x.double())
    want_b = dz.double().sum((0, 2))
    nbytes = int(lib.vt_token_mix_wgrad_scratch_bytes(B, K, M, C, dtype))
    assert nbytes >= (M * K + M) * 4
    runs = []
    for scratch_bytes in (nbytes, nbytes, (M * K + M) * 4):  # twice the usual split, then one slab: a single long split
        scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
        dw = torch.full((M, K), 0.25, device="cuda")  # the kernel ACCUMULATES into the gradient
        db = torch.full((M,), -0.5, device="cuda")
        N.check(lib.vt_token_mix_wgrad(vp(dz), dz.stride(1), vp(x), x.stride(1), vp(dw), vp(db), vp(scratch), scratch_bytes, B, K,
                                       M, C, dtype, stream()))
        torch.cuda.synchronize()
        runs.append((dw.clone(), db.clone()))
    _check(f"{K}x{M}x{C} dW", runs[0][0] - 0.25, want_w, dtype, f32_out=True)
    _check(f"{K}x{M}x{C} dbias", runs[0][1] + 0.5, want_b, dtype, f32_out=True)
    _check(f"{K}x{M}x{C} dW (one split)", runs[2][0] - 0.25, want_w, dtype, f32_out=True)
    _check(f"{K}x{M}x{C} dbias (one split)", runs[2][1] + 0.5, want_b, dtype, f32_out=True)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    # either output alone
    scratch = torch.zeros(nbytes // 4, device="cuda")
    db = torch.zeros(M, device="cuda")
    N.check(lib.vt_token_mix_wgrad(vp(dz), dz.stride(1), vp(x), x.stride(1), None, vp(db), vp(scratch), nbytes, B, K, M, C, dtype,
                                   stream()))
    torch.cuda.synchronize()
    assert torch.equal(db, runs[0][1] + 0.5)


def test_token_mix_rejects_what_it_does_not_cover():
    lib = N.lib()
    x = torch.zeros(1, 8, 12, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(8, 8, device="cuda", dtype=torch.bfloat16)
    z = torch.zeros(1, 8, 12, device="cuda", dtype=torch.bfloat16)
    rc = lib.vt_token_mix_fwd(vp(x), 12, vp(w), 8, 0, None, None, 0, vp(z), 12, None, 0, 0, 1, 8, 8, 12, N.VT_BF16, stream())
    assert rc == N.VT_ERR_INVALID and "multiple of 8" in N.last_error()  # C = 12 off the bf16 chunk
    x = torch.zeros(1, 8, 16, device="cuda", dtype=torch.bfloat16)
    z = torch.zeros(1, 8, 16, device="cuda", dtype=torch.bfloat16)
    rc = lib.vt_token_mix_fwd(vp(x), 16, vp(w), 8, 0, None, None, 0, vp(z), 16, None, 0, 1, 1, 8, 8, 16, N.VT_BF16, stream())
    assert rc == N.VT_ERR_UNSUPPORTED  # activation code 1


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", [(3, 20, 20, 4), (2, 32, 48, 16), (2, 56, 56, 8)], ids=["20x20p4", "32x48p16", "56x56p8"])
def test_patchify_is_an_exact_copy(geom, dtype):
    B, H, W, p = geom
    torch.manual_seed(H + p)
    td, lib = TD[dtype], N.lib()
    cpad = 8 if dtype == N.VT_BF16 else 4
    img = torch.randn(B, H, W, cpad, device="cuda").to(td)
    rows = 3 * p * p
    out = torch.full((B, H // p, W // p, rows), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_patchify_fwd(vp(img), cpad, vp(out), rows, B, H, W, 3, p, dtype, stream()))
    torch.cuda.synchronize()
    # [b][gy][py][gx][px][c] -> [b][gy][gx][py][px][c]: the row order of the channels_last filter [d][p][p][3]
    want = img[..., :3].reshape(B, H // p, p, W // p, p, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, H // p, W // p, rows)
    assert torch.equal(out, want)
    # as a Linear over these rows the embedding equals the convolution
    conv = nn.Conv2d(3, 16, p, p).cuda().double()
    ref = conv(img[..., :3].double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    wrow = conv.weight.permute(0, 2, 3, 1).reshape(16, rows)
    assert rel_err(out.double() @ wrow.T + conv.bias, ref) < 1e-12
    # backward: the scatter, pad channels zero; then added onto a residual that aliases the destination
    dout = torch.randn(B, H // p, W // p, rows, device="cuda").to(td)
    dimg = torch.full((B, H, W, cpad), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_patchify_bwd(vp(dout), rows, vp(dimg), cpad, None, 0, B, H, W, 3, cpad, p, dtype, stream()))
    torch.cuda.synchronize()
    back = dout.reshape(B, H // p, W // p, p, p, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, 3)
    assert torch.equal(dimg[..., :3], back) and not dimg[..., 3:].any()
    acc = torch.randn(B, H, W, cpad, device="cuda").to(td)
    dimg = acc.clone()
    N.check(lib.vt_patchify_bwd(vp(dout), rows, vp(dimg), cpad, vp(dimg), cpad, B, H, W, 3, cpad, p, dtype, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dimg[..., :3], (back.float() + acc[..., :3].float()).to(td)) and torch.equal(dimg[..., 3:], acc[..., 3:])


class _TokenMLP(HipModule):
    """patch embedding -> token MLP with the shortcut, its output returned as the map: NO LayerNorm behind linear2, so the
    gradient of linear2.bias is the plain sum of the output gradient"""

    def __init__(self, d_model, p, size, hidden):
        super().__init__()
        self.embed = nn.Conv2d(3, d_model, p, p)
        n = (size // p) ** 2
        self.linear1, self.linear2 = nn.Linear(n, hidden), nn.Linear(hidden, n)

    def _vt_emit_maps(self, b, x):
        o = b.patch_embed(x, self.embed, name="embed")
        h = b.token_linear(o, self.linear1, act=4, name="linear1")
        return [b.token_linear(h, self.linear2, residual=o, name="linear2")]

    def _eager_maps(self, x):
        o = self.embed(x)  # (B, C, gh, gw)
        t = o.flatten(2)  # (B, C, tokens)
        return [o + self.linear2(F.gelu(self.linear1(t))).reshape(o.shape)]


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def _cpu_run(m, x, r, mode):
    m = m.double() if mode == "f64" else m.float()
    x = (x.double() if mode == "f64" else x.float()).clone().requires_grad_(True)
    m.zero_grad()
    hooks = [mod.register_forward_hook(_to_bf16) for mod in m.modules()] if mode == "bf16" else []
    with torch.autocast("cpu", torch.bfloat16, enabled=mode == "bf16"):
        y = m(x)
    (y.to(r.dtype) * r).sum().backward() if mode != "f64" else (y * r.double()).sum().backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach().double(), "dx": x.grad.detach().double()}
    out.update({k: p.grad.detach().double().clone() for k, p in m.named_parameters()})
    return out


def _gerr(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-3 * (ref.numel() ** 0.5))).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_builder_token_mlp_against_autograd_float64(dtype):
    """bounds of the module tests: f32 2e-4 forward, 4 x for gradients; bf16 3e-2 forward, gradients 4 x the error of the same
    torch module under bf16 autocast with bf16 module outputs (measured here against float64), never above 0.25"""
    torch.manual_seed(11)
    m = _TokenMLP(32, 4, 20, 16)  # 25 tokens -> 16
    for p in m.parameters():
        nn.init.normal_(p, std=0.3)
    x, r = torch.randn(3, 3, 20, 20), torch.randn(3, 32, 5, 5)
    ref = _cpu_run(m, x, r, "f64")
    floor = _cpu_run(m, x, r, "bf16")
    m.zero_grad(set_to_none=True)  # (the CPU runs left their gradients behind: the GPU run must not accumulate onto them)
    m = m.float().cuda()
    m.compute_dtype = dtype
    xd = x.cuda().requires_grad_(True)
    before = N.launch_count()
    y = m(xd)
    (y.float() * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert N.launch_count() > before and y.dtype == dtype and tuple(y.shape) == (3, 32, 5, 5)
    ftol = 2e-4 if dtype == torch.float32 else 3e-2
    e = rel_err(y.detach().float().cpu(), ref["y"])
    print(f"token MLP/{dtype}: y {e:.3e} (bound {ftol:.1e})")
    assert e < ftol
    got = {"dx": xd.grad}
    got.update({k: p.grad for k, p in m.named_parameters()})
    assert ref["linear2.bias"].pow(2).mean().sqrt() > 1.0  # this bias gradient is far from zero here (rms ~ sqrt(B * C))
    for k, g in got.items():
        b = 8e-4 if dtype == torch.float32 else min(4 * _gerr(floor[k], ref[k]), 0.25)
        e = _gerr(g, ref[k])
        print(f"token MLP/{dtype}: {k} {e:.3e} (bound {b:.3e})")
        assert e < b, k
