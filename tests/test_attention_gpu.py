"""vt_attn_fwd / vt_attn_bwd and the ViT token kernels (vt_attention.hip) through the C-ABI against torch in float64 on the
same (storage-rounded) operands: F.scaled_dot_product_attention and autograd for O, dQ, dK, dV, logsumexp of the scaled
scores for lse.

Shapes (B, heads, L, head_dim): ViT-Ti/16 at 224 px (2, 3, 197, 64); L below one 64-row tile (2, 2, 17, 32); exactly one tile
(1, 2, 64, 64); one key past a tile (1, 2, 65, 64); two tiles plus 2 (2, 2, 130, 32); 384 px, many tiles and a tail
(1, 1, 577, 64).  One of them runs again with Q | K | V, O and dQ | dK | dV as channel slices of NaN-filled wider buffers,
8 channels in: the surroundings must still be NaN afterwards and every result finite (a kernel that reads a row or a channel
outside its operand, or forms 0 * NaN from a padded V row, shows here).

Bounds.  f32 outputs, and lse in both dtypes: the `_check` rule of tests/test_token_mix_gpu.py, rtol 1e-4 with an atol of
1e-4 of the largest magnitude.  bf16 outputs: norm-relative 2^-7.  An output passes three or four independent bf16 roundings
of rms 2^-9 / sqrt(3) each (P, or dS and the O inside delta, then the store): 2.0e-3 to 2.3e-3; a CPU emulation of exactly
these rounding points on these shapes measured O at 2.1e-3 to 2.2e-3 and dQ / dK / dV at 2.3e-3 to 2.6e-3.  2^-7 = 7.8e-3 is
three times that, while a wrong mask, a missed key tile or a missing scale is off by 1e-1 or more.  The same emulation is
computed here in torch from the same operands and printed next to the kernel's error.

Large scores: Q multiplied by 32, scores reach +-130, where exp without the row maximum overflows f32.  O and dV must be
finite and inside the bound; dQ and dK are printed, not asserted (their emulated floor on near-one-hot rows is itself 5e-3
to 8e-3)."""
import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, rel_err, stream, vp

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 197, 64), (2, 2, 17, 32), (1, 2, 64, 64), (1, 2, 65, 64), (2, 2, 130, 32), (1, 1, 577, 64)]
IDS = ["2x3x197x64", "2x2x17x32", "1x2x64x64", "1x2x65x64", "2x2x130x32", "1x1x577x64"]
BF16_REL = 2.0 ** -7
DT = [N.VT_F32, N.VT_BF16]
DT_IDS = ["f32", "bf16"]


def _check(tag, got, want, dtype, f32_out=False, emu=None):
    got, want = got.double().cpu(), want.double().cpu()
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    if dtype == N.VT_F32 or f32_out:
        atol = 1e-4 * want.abs().max().item()
        worst = ((got - want).abs() / (atol + 1e-4 * want.abs())).max().item()
        print(f"{tag}: worst |err| / (atol + rtol |ref|) = {worst:.3e} (bound 1), atol {atol:.3e}")
        assert worst < 1.0, tag
    else:
        e = rel_err(got, want)
        note = f", emulated rounding points {rel_err(emu.cpu(), want):.3e}" if emu is not None else ""
        print(f"{tag}: norm-relative {e:.3e} (bound {BF16_REL:.3e}{note})")
        assert e < BF16_REL, tag


def _heads(t, H):  # [B, L, H * D] -> [B, H, L, D]
    B, L, C = t.shape
    return t.reshape(B, L, H, C // H).transpose(1, 2)


def _rows(t):  # back
    B, H, L, D = t.shape
    return t.transpose(1, 2).reshape(B, L, H * D)


def _emulate(q, k, v, do, scale):
    """float64 with the bf16 path's rounding points: P and dS as MFMA operands, the stored O inside delta, the stores"""
    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    S = scale * q @ k.transpose(-1, -2)
    m = S.amax(-1, keepdim=True)
    p = torch.exp(S - m)
    l = p.sum(-1, keepdim=True)
    O = r(r(p) @ v / l)
    P = p / l
    dS = P * (do @ v.transpose(-1, -2) - (do * O).sum(-1, keepdim=True))
    return O, r(scale * r(dS) @ k), r(scale * r(dS).transpose(-1, -2) @ q), r(r(P).transpose(-1, -2) @ do)


_CASES = {}


def _case(shape, dtype, qmul=1.0):
    """operands (storage-rounded, dense, on the device) and the float64 reference, computed once per case"""
    key = (shape, dtype, qmul)
    if key not in _CASES:
        B, H, L, D = shape
        td = TD[dtype]
        gen = torch.Generator(device="cuda").manual_seed(1000 * L + 10 * H + D)
        rnd = lambda: torch.randn(B, L, H * D, device="cuda", generator=gen)  # noqa: E731
        q, k, v, do = (qmul * rnd()).to(td), rnd().to(td), rnd().to(td), rnd().to(td)
        scale = D ** -0.5
        q64, k64, v64 = (_heads(t.double(), H).detach().requires_grad_(True) for t in (q, k, v))
        do64 = _heads(do.double(), H)
        o64 = F.scaled_dot_product_attention(q64, k64, v64)
        dq64, dk64, dv64 = torch.autograd.grad(o64, (q64, k64, v64), do64)
        lse64 = torch.logsumexp(scale * q64.detach() @ k64.detach().transpose(-1, -2), -1)
        emu = None
        if dtype == N.VT_BF16:
            emu = [_rows(t) for t in _emulate(q64.detach(), k64.detach(), v64.detach(), do64, scale)]
        _CASES[key] = dict(q=q, k=k, v=v, do=do, scale=scale, o=_rows(o64.detach()), lse=lse64.detach(), dq=_rows(dq64),
                           dk=_rows(dk64), dv=_rows(dv64), emu=emu)
    return _CASES[key]


def _wide3(B, L, C, td, fills=None):
    """three [B][L][C] channel slices of one NaN-filled [B][L][8 + 3 C + 8] buffer"""
    wide = torch.full((B, L, 3 * C + 16), float("nan"), device="cuda", dtype=td)
    views = [wide[:, :, 8 + i * C:8 + (i + 1) * C] for i in range(3)]
    if fills is not None:
        for dst, src in zip(views, fills):
            dst.copy_(src)
    return wide, views


def _wide1(B, L, C, td, fill=None):
    wide = torch.full((B, L, C + 16), float("nan"), device="cuda", dtype=td)
    view = wide[:, :, 8:8 + C]
    if fill is not None:
        view.copy_(fill)
    return wide, view


def _nan_around(wide, width):
    return bool(torch.isnan(wide[:, :, :8].float()).all() and torch.isnan(wide[:, :, 8 + width:].float()).all())


def _fwd(lib, q, k, v, o, lse, scale, shape, dtype):
    B, H, L, D = shape
    N.check(lib.vt_attn_fwd(vp(q), q.stride(1), vp(k), k.stride(1), vp(v), v.stride(1), vp(o), o.stride(1), vp(lse), scale, B, H,
                            L, D, dtype, stream()))
    torch.cuda.synchronize()


def _bwd(lib, q, k, v, o, do, lse, dq, dk, dv, scale, shape, dtype):
    B, H, L, D = shape
    nbytes = int(lib.vt_attn_bwd_scratch_bytes(B, H, L))
    assert nbytes >= B * H * L * 4
    scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
    ld = lambda t: t.stride(1) if t is not None else 0  # noqa: E731
    N.check(lib.vt_attn_bwd(vp(q), ld(q), vp(k), ld(k), vp(v), ld(v), vp(o), ld(o), vp(do), ld(do), vp(lse), vp(dq), ld(dq), vp(dk),
                            ld(dk), vp(dv), ld(dv), vp(scratch), nbytes, scale, B, H, L, D, dtype, stream()))
    torch.cuda.synchronize()


def _run_dense(shape, dtype, c):
    B, H, L, D = shape
    td, lib = TD[dtype], N.lib()
    o = torch.full((B, L, H * D), float("nan"), device="cuda", dtype=td)
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    _fwd(lib, c["q"], c["k"], c["v"], o, lse, c["scale"], shape, dtype)
    dq, dk, dv = (torch.full((B, L, H * D), float("nan"), device="cuda", dtype=td) for _ in range(3))
    _bwd(lib, c["q"], c["k"], c["v"], o, c["do"], lse, dq, dk, dv, c["scale"], shape, dtype)
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attention_matches_sdpa_and_autograd_in_float64(shape, dtype):
    c = _case(shape, dtype)
    o, lse, dq, dk, dv = _run_dense(shape, dtype, c)
    emu = c["emu"] or [None] * 4
    tag = "x".join(map(str, shape))
    _check(f"{tag} O", o, c["o"], dtype, emu=emu[0])
    _check(f"{tag} lse", lse, c["lse"], dtype, f32_out=True)
    _check(f"{tag} dQ", dq, c["dq"], dtype, emu=emu[1])
    _check(f"{tag} dK", dk, c["dk"], dtype, emu=emu[2])
    _check(f"{tag} dV", dv, c["dv"], dtype, emu=emu[3])


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_attention_on_channel_slices_of_nan_filled_buffers(dtype):
    shape = (2, 2, 130, 32)
    B, H, L, D = shape
    C = H * D
    c = _case(shape, dtype)
    td, lib = TD[dtype], N.lib()
    qkv_w, (q, k, v) = _wide3(B, L, C, td, (c["q"], c["k"], c["v"]))
    o_w, o = _wide1(B, L, C, td)
    do_w, do = _wide1(B, L, C, td, c["do"])
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    _fwd(lib, q, k, v, o, lse, c["scale"], shape, dtype)
    g_w, (dq, dk, dv) = _wide3(B, L, C, td)
    _bwd(lib, q, k, v, o, do, lse, dq, dk, dv, c["scale"], shape, dtype)
    assert _nan_around(qkv_w, 3 * C) and _nan_around(o_w, C) and _nan_around(g_w, 3 * C) and _nan_around(do_w, C)
    emu = c["emu"] or [None] * 4
    _check("slices O", o, c["o"], dtype, emu=emu[0])
    _check("slices lse", lse, c["lse"], dtype, f32_out=True)
    _check("slices dQ", dq, c["dq"], dtype, emu=emu[1])
    _check("slices dK", dk, c["dk"], dtype, emu=emu[2])
    _check("slices dV", dv, c["dv"], dtype, emu=emu[3])
    # the dense run of the same operands gives the same bits: strides change addresses, not arithmetic
    o2, lse2, dq2, dk2, dv2 = _run_dense(shape, dtype, c)
    for a, b in ((o, o2), (lse, lse2), (dq, dq2), (dk, dk2), (dv, dv2)):
        assert torch.equal(a.float(), b.float())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 2, 130, 32), (1, 2, 65, 64)], ids=["2x2x130x32", "1x2x65x64"])
def test_attention_with_large_scores_stays_finite_and_in_bound(shape, dtype):
    c = _case(shape, dtype, qmul=32.0)
    s = c["scale"] * _heads(c["q"].double(), shape[1]) @ _heads(c["k"].double(), shape[1]).transpose(-1, -2)
    top = s.abs().max().item()
    print(f"largest |score| {top:.1f}")
    assert top > 89.0  # exp overflows f32 above 88.7: a kernel that does not subtract the row maximum cannot pass
    o, lse, dq, dk, dv = _run_dense(shape, dtype, c)
    emu = c["emu"] or [None] * 4
    tag = "x".join(map(str, shape)) + " Q*32"
    _check(f"{tag} O", o, c["o"], dtype, emu=emu[0])
    _check(f"{tag} lse", lse, c["lse"], dtype, f32_out=True)
    _check(f"{tag} dV", dv, c["dv"], dtype, emu=emu[3])
    for name, got, want, e in (("dQ", dq, c["dq"], emu[1]), ("dK", dk, c["dk"], emu[2])):
        assert bool(torch.isfinite(got.float()).all())
        note = f", emulated {rel_err(e, want):.3e}" if e is not None else ""
        print(f"{tag} {name}: norm-relative {rel_err(got, want):.3e} (recorded, not asserted{note})")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_attention_backward_is_bit_identical_and_each_gradient_works_alone(dtype):
    shape = (2, 3, 197, 64)
    B, H, L, D = shape
    c = _case(shape, dtype)
    td, lib = TD[dtype], N.lib()
    o, lse, dq, dk, dv = _run_dense(shape, dtype, c)
    o2, lse2, dq2, dk2, dv2 = _run_dense(shape, dtype, c)
    for a, b in ((o, o2), (lse, lse2), (dq, dq2), (dk, dk2), (dv, dv2)):
        assert torch.equal(a.float(), b.float())
    for i, want in enumerate((dq, dk, dv)):
        outs = [None, None, None]
        outs[i] = torch.full((B, L, H * D), float("nan"), device="cuda", dtype=td)
        _bwd(lib, c["q"], c["k"], c["v"], o, c["do"], lse, outs[0], outs[1], outs[2], c["scale"], shape, dtype)
        assert torch.equal(outs[i].float(), want.float())


def test_attention_rejects_what_it_does_not_implement():
    lib = N.lib()
    B, H, L = 1, 2, 16
    lse = torch.zeros(B, H, L, device="cuda")
    t = torch.zeros(B, L, H * 80, device="cuda", dtype=torch.bfloat16)
    rc = lib.vt_attn_fwd(vp(t), 160, vp(t), 160, vp(t), 160, vp(t), 160, vp(lse), 0.1, B, H, L, 80, N.VT_BF16, stream())
    assert rc == N.VT_ERR_UNSUPPORTED and "head_dim" in N.last_error()  # ViT-H
    scratch = torch.zeros(B * H * L, device="cuda")
    rc = lib.vt_attn_bwd(vp(t), 160, vp(t), 160, vp(t), 160, vp(t), 160, vp(t), 160, vp(lse), vp(t), 160, None, 0, None, 0,
                         vp(scratch), scratch.numel() * 4, 0.1, B, H, L, 80, N.VT_BF16, stream())
    assert rc == N.VT_ERR_UNSUPPORTED and "head_dim" in N.last_error()
    t = torch.zeros(B, L, 68, device="cuda", dtype=torch.bfloat16)  # a row stride of 68: no multiple of the 8-element chunk
    rc = lib.vt_attn_fwd(vp(t), 68, vp(t), 68, vp(t), 68, vp(t), 68, vp(lse), 0.1, B, H, L, 32, N.VT_BF16, stream())
    assert rc == N.VT_ERR_INVALID and "row stride 68" in N.last_error()
    t = torch.zeros(B, L, 64, device="cuda", dtype=torch.bfloat16)
    rc = lib.vt_attn_bwd(vp(t), 64, vp(t), 64, vp(t), 64, vp(t), 64, vp(t), 64, vp(lse), None, 0, None, 0, None, 0, vp(scratch),
                         scratch.numel() * 4, 0.1, B, H, L, 32, N.VT_BF16, stream())
    assert rc == N.VT_ERR_INVALID and "no output" in N.last_error()
    rc = lib.vt_attn_bwd(vp(t), 64, vp(t), 64, vp(t), 64, vp(t), 64, vp(t), 64, vp(lse), vp(t), 64, None, 0, None, 0, vp(scratch), 16,
                         0.1, B, H, L, 32, N.VT_BF16, stream())
    assert rc == N.VT_ERR_INVALID and "scratch" in N.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("with_cls", [True, False], ids=["cls", "nocls"])
def test_vit_tokens_forward_and_backward_match_torch(with_cls, dtype):
    B, T, C = 3, 9, 40
    td, lib = TD[dtype], N.lib()
    c0 = 1 if with_cls else 0
    torch.manual_seed(7 + c0)
    ew, embed = _wide1(B, T, C, td, torch.randn(B, T, C, device="cuda"))
    pe = torch.randn(T, C, device="cuda")
    cls = torch.randn(C, device="cuda") if with_cls else None
    ow, out = _wide1(B, T + c0, C, td)
    N.check(lib.vt_vit_tokens_fwd(vp(embed), embed.stride(1), vp(pe), vp(cls), vp(out), out.stride(1), B, T, C, dtype, stream()))
    torch.cuda.synchronize()
    want = embed.float() + pe  # one f32 add, then the store's rounding: exact against the same arithmetic
    assert torch.equal(out[:, c0:].float(), want.to(td).float())
    if with_cls:
        assert torch.equal(out[:, 0].float(), cls.to(td).float().expand(B, C))
    assert _nan_around(ow, C)

    gw, dout = _wide1(B, T + c0, C, td, torch.randn(B, T + c0, C, device="cuda") + 0.5)
    runs = []
    for _ in range(2):
        dw, dembed = _wide1(B, T, C, td)
        dpe = torch.full((T, C), 0.25, device="cuda")  # accumulates onto what is there
        dcls = torch.full((C,), -0.5, device="cuda") if with_cls else None
        N.check(lib.vt_vit_tokens_bwd(vp(dout), dout.stride(1), vp(dembed), dembed.stride(1), vp(dpe), vp(dcls), c0, B, T, C, dtype,
                                      stream()))
        torch.cuda.synchronize()
        assert torch.equal(dembed.float(), dout[:, c0:].float()) and _nan_around(dw, C)  # the copy is exact
        runs.append((dpe, dcls))
    _check("d pe", runs[0][0], 0.25 + dout[:, c0:].double().sum(0), dtype, f32_out=True)
    assert torch.equal(runs[0][0], runs[1][0])
    if with_cls:
        _check("d cls", runs[0][1], -0.5 + dout[:, 0].double().sum(0), dtype, f32_out=True)
        assert torch.equal(runs[0][1], runs[1][1])
    # frozen embedding and position embedding: only the class token's gradient
    if with_cls:
        dcls = torch.zeros(C, device="cuda")
        N.check(lib.vt_vit_tokens_bwd(vp(dout), dout.stride(1), None, 0, None, vp(dcls), 1, B, T, C, dtype, stream()))
        torch.cuda.synchronize()
        _check("d cls alone", dcls, dout[:, 0].double().sum(0), dtype, f32_out=True)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_token_select_forward_and_backward_match_torch(dtype):
    B, T, C, t0 = 3, 7, 24, 2
    td, lib = TD[dtype], N.lib()
    torch.manual_seed(11)
    xw, x = _wide1(B, T, C, td, torch.randn(B, T, C, device="cuda"))
    out = torch.full((B, C), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_token_select_fwd(vp(x), x.stride(1), vp(out), C, B, T, t0, C, dtype, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.float(), x[:, t0].float())
    dout = torch.randn(B, C, device="cuda").to(td)
    dw, dx = _wide1(B, T, C, td)
    N.check(lib.vt_token_select_bwd(vp(dout), C, vp(dx), dx.stride(1), 0, B, T, t0, C, dtype, stream()))
    torch.cuda.synchronize()
    want = torch.zeros(B, T, C, device="cuda")
    want[:, t0] = dout.float()
    assert torch.equal(dx.float(), want) and _nan_around(dw, C)
    base = torch.randn(B, T, C, device="cuda").to(td)
    dw, dx = _wide1(B, T, C, td, base)
    N.check(lib.vt_token_select_bwd(vp(dout), C, vp(dx), dx.stride(1), 1, B, T, t0, C, dtype, stream()))
    torch.cuda.synchronize()
    want = base.float().clone()
    want[:, t0] = (base[:, t0].float() + dout.float()).to(td).float()
    assert torch.equal(dx.float(), want) and _nan_around(dw, C)
