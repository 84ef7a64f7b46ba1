"""vt_win_attn_fwd / vt_win_attn_bwd (vt_window_attention.hip) through the C-ABI against torch in float64 on the same
(storage-rounded) operands.  The float64 side is the package's own window_partition / window_unpartition and
relative_pe_index, the package's shift_mask (its own attn_mask on square maps, asserted equal), torch.roll,
F.scaled_dot_product_attention with the additive bias and autograd for O, dQ, dK, dV and d table, logsumexp of the biased
scores for lse.  It is computed once per case on the CPU and shared by the tests.

Shapes (B, H, W, heads, ws, shift), head_dim 32: the real Swin window (2, 14, 14, 3, 7, 3); (1, 21, 21, 1, 7, 3), which has an
interior window with nothing masked; unshifted (2, 14, 14, 2, 7, 0); a single window (1, 7, 7, 2, 7, 0); 16-token windows
(2, 12, 12, 2, 4, 2); 9-token windows (1, 6, 6, 1, 3, 1); a full 64-token tile (1, 16, 16, 1, 8, 4); non-square (1, 8, 12, 1, 4,
2).  The table has a standard deviation of 1.0.

Bounds.  f32 outputs, and lse in both dtypes: the `_check` rule of tests/test_attention_gpu.py, rtol 1e-4 with an atol of 1e-4
of the largest magnitude.  bf16 outputs, d table included (it is summed in f32 from an f32 dS, but dS inherits the bf16
rounding of the stored O inside delta): norm-relative 2^-7 = 7.8e-3, that file's bound, on condition that the float64
emulation of the kernel's rounding points stays under a third of it (2.6e-3); where it does not, that output's bound on that
shape is three times its emulated error.  `_emulate` restates the rounding points -- exp(S - max) rounded as the operand of
P V, P rounded as the operand of dV, the stored O inside delta, dS rounded as the operand of dK and dQ, the stores -- on the
same operands; its error is printed next to the kernel's.  Measured on the CPU over the listed shapes, in their order:

    O       1.91 1.90 1.92 1.96 1.86 1.82 1.86 1.85 e-3   under a third everywhere: bound 2^-7
    dV      2.35 2.42 2.28 2.20 2.37 2.09 2.41 2.23 e-3   under a third everywhere: bound 2^-7
    dQ      2.67 2.65 2.61 2.40 2.88 3.52 2.82 2.81 e-3   above a third on all but 1x7x7x2x7x0: bound 3 x emulated, 7.83e-3 to 1.055e-2
    dK      2.63 2.55 2.56 2.30 2.77 3.57 2.70 2.91 e-3   above a third on five shapes: bound 3 x emulated there, up to 1.070e-2
    dtable  0.93 1.40 0.74 1.33 1.45 2.72 1.65 2.54 e-3   above a third on 1x6x6x1x3x1 only: bound 8.18e-3 there

(the fewer keys a row has, the less the rounding of dS averages out: 9-token windows are the worst).  A wrong mask, a wrong
bias index or a missing scale is off by 1e-1 or more.  The bounds are stated in _WIDER; test_emulated_rounding_points prints the
table and asserts that each stated bound is what this rule gives.

Large scores: Q times 32 and the table times 30 on the shifted 7x7 shape; |score + bias| passes 89, where exp without the row
maximum overflows f32.  O, lse and dV stay inside the bound; dQ and dK are finite and printed."""
import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N
from vision_toolbox.backbones import WindowAttention, window_partition, window_unpartition
from vision_toolbox.backbones.swin import shift_mask

from gpu_util import TD, rel_err, stream, vp

pytestmark = pytest.mark.gpu

SHAPES = [(2, 14, 14, 3, 7, 3), (1, 21, 21, 1, 7, 3), (2, 14, 14, 2, 7, 0), (1, 7, 7, 2, 7, 0), (2, 12, 12, 2, 4, 2),
          (1, 6, 6, 1, 3, 1), (1, 16, 16, 1, 8, 4), (1, 8, 12, 1, 4, 2)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
D = 32
BF16_REL = 2.0 ** -7
DT = [N.VT_F32, N.VT_BF16]
DT_IDS = ["f32", "bf16"]
NAMES = ("O", "dQ", "dK", "dV", "dtable")
# the bf16 bounds that are not 2^-7: three times the emulated error of the module docstring's table, rounded up to three digits
_WIDER = {
    "dQ": {"2x14x14x3x7x3": 8.02e-3, "1x21x21x1x7x3": 7.95e-3, "2x14x14x2x7x0": 7.83e-3, "2x12x12x2x4x2": 8.65e-3,
           "1x6x6x1x3x1": 1.055e-2, "1x16x16x1x8x4": 8.48e-3, "1x8x12x1x4x2": 8.45e-3},
    "dK": {"2x14x14x3x7x3": 7.90e-3, "2x12x12x2x4x2": 8.31e-3, "1x6x6x1x3x1": 1.070e-2, "1x16x16x1x8x4": 8.11e-3,
           "1x8x12x1x4x2": 8.75e-3},
    "dtable": {"1x6x6x1x3x1": 8.18e-3},
}


def _bound(name, shape):
    return _WIDER.get(name, {}).get("x".join(map(str, shape)), BF16_REL)


def _check(tag, got, want, dtype, f32_out=False, emu=None, bound=None):
    got, want = got.double().cpu(), want.double().cpu()
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    if dtype == N.VT_F32 or f32_out:
        atol = 1e-4 * want.abs().max().item()
        worst = ((got - want).abs() / (atol + 1e-4 * want.abs())).max().item()
        print(f"{tag}: worst |err| / (atol + rtol |ref|) = {worst:.3e} (bound 1), atol {atol:.3e}")
        assert worst < 1.0, tag
    else:
        e, floor = rel_err(got, want), rel_err(emu.cpu(), want)
        print(f"{tag}: norm-relative {e:.3e} (bound {bound:.3e}, emulated rounding points {floor:.3e})")
        assert e < bound, tag


def _mask(H, W, ws, shift):
    """(windows, L, L): the package's region rule on an H x W map (the module's attn_mask on square maps)"""
    if shift == 0:
        return torch.zeros((H // ws) * (W // ws), ws * ws, ws * ws, dtype=torch.float64)
    mask = shift_mask(H, W, ws, shift)
    if H == W:
        assert torch.equal(mask, WindowAttention(H, D, 1, ws, True).attn_mask)
    return mask.double()


def _windows(t, heads, ws, shift):  # [B, H, W, heads * X] -> [B * windows, heads, L, X]
    w, _, _ = window_partition(t.roll((-shift, -shift), (1, 2)), ws)
    return w.unflatten(-1, (heads, -1)).transpose(1, 2)


def _map(t, B, H, W, ws, shift):  # [B * windows, heads, L, X] -> [B, H, W, heads * X]
    return window_unpartition(t.transpose(1, 2).flatten(2), ws, H // ws, W // ws).roll((shift, shift), (1, 2))


def _emulate(qw, kw, vw, gw, bias, index, scale, n):
    """float64 with the bf16 path's rounding points, in window space: exp(S - max) and P as MFMA operands, the stored O
    inside delta, dS as the operand of dK and dQ (d table takes it unrounded), the stores"""
    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    S = scale * qw @ kw.transpose(-1, -2) + bias
    m = S.amax(-1, keepdim=True)
    p = torch.exp(S - m)
    l = p.sum(-1, keepdim=True)
    O = r(r(p) @ vw / l)
    P = p / l
    dS = P * (gw @ vw.transpose(-1, -2) - (gw * O).sum(-1, keepdim=True))
    dtab = torch.zeros(dS.shape[1], n, dtype=torch.float64).index_add_(1, index.flatten(), dS.sum(0).flatten(1))
    return O, r(scale * r(dS) @ kw), r(scale * r(dS).transpose(-1, -2) @ qw), r(r(P).transpose(-1, -2) @ gw), dtab


_CASES = {}


def _case(shape, dtype, qmul=1.0, tmul=1.0):
    """operands (storage-rounded, dense, on the CPU), the float64 reference and the emulation, computed once per case"""
    key = (shape, dtype, qmul, tmul)
    if key not in _CASES:
        B, H, W, heads, ws, shift = shape
        td, C, n, scale = TD[dtype], heads * D, (2 * ws - 1) ** 2, D ** -0.5
        gen = torch.Generator().manual_seed(100000 * H + 1000 * W + 100 * heads + 10 * ws + shift)
        rnd = lambda: torch.randn(B, H, W, C, generator=gen)  # noqa: E731
        q, k, v, do = (qmul * rnd()).to(td), rnd().to(td), rnd().to(td), rnd().to(td)
        table = tmul * torch.randn(heads, n, generator=gen)
        index = WindowAttention(ws, D, 1, ws).relative_pe_index
        mask = _mask(H, W, ws, shift)
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
        t64 = table.double().requires_grad_(True)
        bias = (t64[:, index].unsqueeze(0) + mask.unsqueeze(1)).repeat(B, 1, 1, 1)  # (B * windows, heads, L, L)
        qw, kw, vw = (_windows(t, heads, ws, shift) for t in (q64, k64, v64))
        o64 = _map(F.scaled_dot_product_attention(qw, kw, vw, bias), B, H, W, ws, shift)
        dq, dk, dv, dt = torch.autograd.grad(o64, (q64, k64, v64, t64), do.double())
        with torch.no_grad():
            S = scale * qw @ kw.transpose(-1, -2) + bias
            lse = _map(torch.logsumexp(S, -1).unsqueeze(-1), B, H, W, ws, shift).permute(0, 3, 1, 2).flatten(2)  # [B, heads, H W]
            emu = None
            if dtype == N.VT_BF16:
                e = _emulate(qw, kw, vw, _windows(do.double(), heads, ws, shift), bias, index, scale, n)
                emu = [_map(t, B, H, W, ws, shift) for t in e[:4]] + [e[4]]
        _CASES[key] = dict(q=q, k=k, v=v, do=do, table=table, scale=scale, top=S.abs()[S > -50].max().item(),
                           want=[o64.detach(), dq, dk, dv, dt], lse=lse, emu=emu)
    return _CASES[key]


def test_emulated_rounding_points():
    """the table of the module docstring: pure torch on the CPU, over every listed shape.  O and dV stay under a third of
    2^-7 everywhere; every bound stated in _WIDER is three times the emulated error of its output on its shape, and every
    other output stays under a third of 2^-7"""
    for shape, tag in zip(SHAPES, IDS):
        c = _case(shape, N.VT_BF16)
        errs = {name: rel_err(e, w) for name, e, w in zip(NAMES, c["emu"], c["want"])}
        print(f"{tag}: emulated " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (a third of 2^-7: {BF16_REL / 3:.3e})")
        assert errs["O"] < BF16_REL / 3 and errs["dV"] < BF16_REL / 3, tag
        for name, e in errs.items():
            # a stated bound is 2^-7 exactly where the emulation is under a third of it, else 3 x emulated, rounded up
            if e < BF16_REL / 3:
                assert _bound(name, shape) == BF16_REL, (tag, name)
            else:
                assert 3 * e <= _bound(name, shape) < 3 * e * 1.005, (tag, name, e)
    c = _case(SHAPES[0], N.VT_BF16, qmul=32.0, tmul=30.0)  # the large-score case asserts O and dV at 2^-7
    assert all(rel_err(c["emu"][i], c["want"][i]) < BF16_REL / 3 for i in (0, 3))


def _fwd(lib, q, k, v, o, lse, table, scale, shape, dtype):
    B, H, W, heads, ws, shift = shape
    N.check(lib.vt_win_attn_fwd(vp(q), q.stride(2), vp(k), k.stride(2), vp(v), v.stride(2), vp(o), o.stride(2), vp(lse), vp(table),
                                scale, B, H, W, heads, D, ws, shift, dtype, stream()))
    torch.cuda.synchronize()


def _bwd(lib, q, k, v, o, do, lse, table, dq, dk, dv, dtable, scale, shape, dtype):
    B, H, W, heads, ws, shift = shape
    nbytes = int(lib.vt_win_attn_bwd_scratch_bytes(B, H, W, heads, ws))
    assert nbytes == B * (H // ws) * (W // ws) * heads * (2 * ws - 1) ** 2 * 4
    if dtable is None:
        scratch, nbytes = None, 0  # no table gradient: the scratch is not looked at
    else:
        scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
    ld = lambda t: t.stride(2) if t is not None else 0  # noqa: E731
    N.check(lib.vt_win_attn_bwd(vp(q), ld(q), vp(k), ld(k), vp(v), ld(v), vp(o), ld(o), vp(do), ld(do), vp(lse), vp(table), vp(dq),
                                ld(dq), vp(dk), ld(dk), vp(dv), ld(dv), vp(dtable), vp(scratch), nbytes, scale, B, H, W, heads, D, ws,
                                shift, dtype, stream()))
    torch.cuda.synchronize()


def _dev(c):
    return {k: c[k].cuda() for k in ("q", "k", "v", "do", "table")}


def _run_dense(shape, dtype, c, d=None):
    B, H, W, heads, ws, shift = shape
    td, lib, d = TD[dtype], N.lib(), d or _dev(c)
    nan = lambda: torch.full((B, H, W, heads * D), float("nan"), device="cuda", dtype=td)  # noqa: E731
    o, lse = nan(), torch.full((B, heads, H * W), float("nan"), device="cuda")
    _fwd(lib, d["q"], d["k"], d["v"], o, lse, d["table"], c["scale"], shape, dtype)
    dq, dk, dv = nan(), nan(), nan()
    dtable = torch.zeros_like(d["table"])
    _bwd(lib, d["q"], d["k"], d["v"], o, d["do"], lse, d["table"], dq, dk, dv, dtable, c["scale"], shape, dtype)
    return o, lse, dq, dk, dv, dtable


def _check_all(tag, shape, c, dtype, o, lse, dq, dk, dv, dtable, names=NAMES):
    emu = c["emu"] or [None] * 5
    _check(f"{tag} lse", lse, c["lse"], dtype, f32_out=True)
    for name, got, want, e in zip(NAMES, (o, dq, dk, dv, dtable), c["want"], emu):
        if name in names:
            _check(f"{tag} {name}", got, want, dtype, emu=e, bound=_bound(name, shape))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_window_attention_matches_sdpa_and_autograd_in_float64(shape, dtype):
    c = _case(shape, dtype)
    _check_all("x".join(map(str, shape)), shape, c, dtype, *_run_dense(shape, dtype, c))


def _wide(B, H, W, C, parts, td, fills=None):
    """`parts` [B][H][W][C] channel slices of one NaN-filled [B][H][W][8 + parts C + 8] buffer"""
    wide = torch.full((B, H, W, parts * C + 16), float("nan"), device="cuda", dtype=td)
    views = [wide[..., 8 + i * C:8 + (i + 1) * C] for i in range(parts)]
    for dst, src in zip(views, fills or ()):
        dst.copy_(src)
    return wide, views


def _nan_around(wide, width):
    return bool(torch.isnan(wide[..., :8].float()).all() and torch.isnan(wide[..., 8 + width:].float()).all())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_window_attention_on_channel_slices_of_nan_filled_buffers(dtype):
    shape = (2, 12, 12, 2, 4, 2)
    B, H, W, heads, ws, shift = shape
    C = heads * D
    c = _case(shape, dtype)
    d = _dev(c)
    td, lib = TD[dtype], N.lib()
    qkv_w, (q, k, v) = _wide(B, H, W, C, 3, td, (d["q"], d["k"], d["v"]))
    o_w, (o,) = _wide(B, H, W, C, 1, td)
    do_w, (do,) = _wide(B, H, W, C, 1, td, (d["do"],))
    lse = torch.full((B, heads, H * W), float("nan"), device="cuda")
    _fwd(lib, q, k, v, o, lse, d["table"], c["scale"], shape, dtype)
    g_w, (dq, dk, dv) = _wide(B, H, W, C, 3, td)
    dtable = torch.zeros_like(d["table"])
    _bwd(lib, q, k, v, o, do, lse, d["table"], dq, dk, dv, dtable, c["scale"], shape, dtype)
    assert _nan_around(qkv_w, 3 * C) and _nan_around(o_w, C) and _nan_around(g_w, 3 * C) and _nan_around(do_w, C)
    _check_all("slices", shape, c, dtype, o, lse, dq, dk, dv, dtable)
    # the dense run of the same operands gives the same bits: strides change addresses, not arithmetic
    for a, b in zip((o, lse, dq, dk, dv, dtable), _run_dense(shape, dtype, c, d)):
        assert torch.equal(a.float(), b.float())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_window_attention_is_bit_identical_and_each_gradient_works_alone(dtype):
    shape = (2, 14, 14, 3, 7, 3)
    B, H, W, heads, ws, shift = shape
    c = _case(shape, dtype)
    d = _dev(c)
    td, lib = TD[dtype], N.lib()
    first = _run_dense(shape, dtype, c, d)
    for a, b in zip(first, _run_dense(shape, dtype, c, d)):
        assert torch.equal(a.float(), b.float())
    o, lse, dq, dk, dv, dtable = first
    for i, want in enumerate((dq, dk, dv, dtable)):
        outs = [None] * 4
        outs[i] = torch.zeros_like(d["table"]) if i == 3 else torch.full((B, H, W, heads * D), float("nan"), device="cuda", dtype=td)
        _bwd(lib, d["q"], d["k"], d["v"], o, d["do"], lse, d["table"], *outs, c["scale"], shape, dtype)
        assert torch.equal(outs[i].float(), want.float()), i
    # d table adds onto what is there
    base = torch.randn_like(d["table"])
    acc = base.clone()
    _bwd(lib, d["q"], d["k"], d["v"], o, d["do"], lse, d["table"], None, None, None, acc, c["scale"], shape, dtype)
    assert torch.equal(acc, base + dtable)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_window_attention_with_large_scores_stays_finite_and_in_bound(dtype):
    shape = (2, 14, 14, 3, 7, 3)
    c = _case(shape, dtype, qmul=32.0, tmul=30.0)
    print(f"largest |score + bias| off the mask {c['top']:.1f}")
    assert c["top"] > 89.0  # exp overflows f32 above 88.7: a kernel that does not subtract the row maximum cannot pass
    o, lse, dq, dk, dv, dtable = _run_dense(shape, dtype, c)
    _check_all("Q*32 table*30", (), c, dtype, o, lse, dq, dk, dv, dtable, names=("O", "dV"))  # (): O and dV at 2^-7
    emu = c["emu"] or [None] * 5
    for name, got, i in (("dQ", dq, 1), ("dK", dk, 2), ("dtable", dtable, 4)):
        assert bool(torch.isfinite(got.float()).all())
        note = f", emulated {rel_err(emu[i], c['want'][i]):.3e}" if emu[i] is not None else ""
        print(f"Q*32 table*30 {name}: norm-relative {rel_err(got.double().cpu(), c['want'][i]):.3e} (recorded, not asserted{note})")


def test_window_attention_rejects_what_it_does_not_implement():
    lib = N.lib()
    lse = torch.zeros(1, 2, 28 * 28, device="cuda")
    table = torch.zeros(2, 27 * 27, device="cuda")
    scratch = torch.zeros(1 << 16, device="cuda")
    t = torch.zeros(1, 28, 28, 160, device="cuda", dtype=torch.bfloat16)

    def fwd(t, ld, H, W, heads, hd, ws, shift):
        return lib.vt_win_attn_fwd(vp(t), ld, vp(t), ld, vp(t), ld, vp(t), ld, vp(lse), vp(table), 0.1, 1, H, W, heads, hd, ws, shift,
                                   N.VT_BF16, stream())

    def bwd(t, ld, H, W, heads, hd, ws, shift, nbytes, outs=True, dtable=None):
        g = vp(t) if outs else None
        return lib.vt_win_attn_bwd(vp(t), ld, vp(t), ld, vp(t), ld, vp(t), ld, vp(t), ld, vp(lse), vp(table), g, ld, None, 0, None, 0,
                                   vp(dtable), vp(scratch), nbytes, 0.1, 1, H, W, heads, hd, ws, shift, N.VT_BF16, stream())

    big = scratch.numel() * 4
    for rc in (fwd(t, 160, 28, 28, 2, 32, 14, 0), bwd(t, 160, 28, 28, 2, 32, 14, 0, big)):  # the S3 window
        assert rc == N.VT_ERR_UNSUPPORTED and "ws=14" in N.last_error()
    for rc in (fwd(t, 160, 28, 28, 2, 80, 7, 3), bwd(t, 160, 28, 28, 2, 80, 7, 3, big)):
        assert rc == N.VT_ERR_UNSUPPORTED and "head_dim 80" in N.last_error()
    for rc in (fwd(t, 160, 26, 28, 2, 32, 7, 3), bwd(t, 160, 26, 28, 2, 32, 7, 3, big)):
        assert rc == N.VT_ERR_INVALID and "H=26" in N.last_error() and "ws=7" in N.last_error()
    for rc in (fwd(t, 160, 28, 28, 2, 32, 7, 7), bwd(t, 160, 28, 28, 2, 32, 7, 7, big)):
        assert rc == N.VT_ERR_INVALID and "shift=7" in N.last_error()
    t68 = torch.zeros(1, 14, 14, 68, device="cuda", dtype=torch.bfloat16)  # a pixel stride of 68: no multiple of the 8-element chunk
    for rc in (fwd(t68, 68, 14, 14, 2, 32, 7, 3), bwd(t68, 68, 14, 14, 2, 32, 7, 3, big)):
        assert rc == N.VT_ERR_INVALID and "stride 68" in N.last_error()
    t64 = torch.zeros(1, 14, 14, 64, device="cuda", dtype=torch.bfloat16)
    assert bwd(t64, 64, 14, 14, 2, 32, 7, 3, big, outs=False) == N.VT_ERR_INVALID and "no output" in N.last_error()
    need = int(lib.vt_win_attn_bwd_scratch_bytes(1, 14, 14, 2, 7))
    assert need == 4 * 2 * 169 * 4
    dtable = torch.zeros(2, 169, device="cuda")  # the scratch is checked only where it is written: with a table gradient
    assert bwd(t64, 64, 14, 14, 2, 32, 7, 3, need - 4, dtable=dtable) == N.VT_ERR_INVALID and "scratch" in N.last_error()
    assert str(need) in N.last_error()
    torch.cuda.synchronize()
