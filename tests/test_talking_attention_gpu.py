"""vt_talk_attn_fwd / vt_talk_attn_bwd, vt_cls_attn_fwd / vt_cls_attn_bwd and vt_token_prepend_* (vt_talking_attention.hip)
through the C-ABI against torch in float64 on the same (storage-rounded) operands: autograd of

    A_h = s q_h k_h^T,  M_g = sum_h Wl[g,h] A_h + bl[g],  P = softmax_j M,  R_g = sum_h Ww[g,h] P_h + bw[g],  O_g = R_g v_g

for O, dQ, dK, dV, dWl, dWw, dbw, logsumexp of M for lse; F.scaled_dot_product_attention with one query row for the class
attention.  `dbl` is exactly zero in exact arithmetic (every row of dM sums to zero): it must be finite and is printed.

Talking-heads shapes (B, H, L, 48): (2, 4, 196) xxs at 224 px; (2, 2, 17); (1, 3, 64) odd H; (1, 2, 65); (1, 16, 130) the
largest H; (1, 6, 576) 384 px.  Class-attention shapes (B, H, Lk, D): (2, 4, 197, 48); (3, 2, 5, 48) fewer keys than a wave;
(1, 3, 64, 48); (1, 3, 65, 48); (1, 16, 577, 48); (2, 2, 130, 32); (1, 1, 65, 64).  One shape of each runs again on channel
slices of NaN-filled wider buffers: the surroundings stay NaN and the results are bit-equal to the dense run.

Bounds.  f32 outputs, and lse in both dtypes: the `_check` rule of tests/test_attention_gpu.py, rtol 1e-4 with an atol of 1e-4
of the largest magnitude.  bf16 outputs: the rule of tests/test_window_attention_gpu.py -- norm-relative 2^-7 = 7.8e-3 where the
float64 emulation of the kernels' bf16 rounding points stays under a third of it (2.6e-3), else three times the emulated
error.  The bf16 talking-heads FORWARD runs on the matrix unit: R is rounded to bf16 as the operand of R V, then O is stored
(two rounding points; P stays f32).  Every other kernel computes in f32 from the stored operands, so its only bf16 rounding
point is the STORE of dQ, dK, dV (and of the class attention's O).  The parameter gradients and lse are f32 outputs with no bf16
rounding point: they are held to the elementwise f32 rule in both dtypes.  `_emulate` restates exactly these points in float64.
Measured on the CPU over the listed shapes, in their order (e-3):

    talking heads   O   2.33 2.24 2.28 2.34 2.42 2.19     class attention   O   1.71 1.51 1.58 1.65 1.62 1.70 1.56
                    dQ  1.65 1.71 1.64 1.65 1.67 1.66                       dQ  1.72 1.75 1.75 1.69 1.65 1.59 1.76
                    dK  1.68 1.64 1.63 1.68 1.64 1.67                       dK  1.64 1.79 1.74 1.61 1.64 1.72 1.57
                    dV  1.62 1.71 1.71 1.72 1.67 1.61                       dV  1.67 1.56 1.61 1.55 1.65 1.65 1.61

under a third of 2^-7 (2.60) everywhere: every bf16 bound is 2^-7.  test_emulated_rounding_points prints the table and asserts that.

Large scores: Q times 32, |M| passes 89, where exp without the row maximum overflows f32.  O, lse and dV in bound; dQ / dK
finite and printed."""
import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, rel_err, stream, vp

pytestmark = pytest.mark.gpu

TALK_SHAPES = [(2, 4, 196, 48), (2, 2, 17, 48), (1, 3, 64, 48), (1, 2, 65, 48), (1, 16, 130, 48), (1, 6, 576, 48)]
CLS_SHAPES = [(2, 4, 197, 48), (3, 2, 5, 48), (1, 3, 64, 48), (1, 3, 65, 48), (1, 16, 577, 48), (2, 2, 130, 32), (1, 1, 65, 64)]
BF16_REL = 2.0 ** -7
DT = [N.VT_F32, N.VT_BF16]
DT_IDS = ["f32", "bf16"]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]  # noqa: E731


def _bound(name, shape):
    """the bf16 bound of an output on a shape: 2^-7 everywhere (the emulated error is under a third of it, module docstring)"""
    return BF16_REL


def _check(tag, got, want, dtype, f32_out=False, emu=None, bound=BF16_REL):
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
        print(f"{tag}: norm-relative {e:.3e} (bound {bound:.3e}{note})")
        assert e < bound, tag


def _heads(t, H):  # [B, L, H * D] -> [B, H, L, D]
    B, L, C = t.shape
    return t.reshape(B, L, H, C // H).transpose(1, 2)


def _rows(t):  # back
    B, H, L, D = t.shape
    return t.transpose(1, 2).reshape(B, L, H * D)


def _emulate(outs):
    """float64 with the bf16 dtype's rounding points: the stores"""
    return [t.to(torch.bfloat16).double() for t in outs]


_CASES = {}


def _talk_case(shape, dtype, qmul=1.0):
    """operands (storage-rounded, dense, on the CPU), the float64 reference and the emulation, computed once per case"""
    key = ("talk", shape, dtype, qmul)
    if key not in _CASES:
        B, H, L, D = shape
        td = TD[dtype]
        gen = torch.Generator().manual_seed(1000 * L + 10 * H + D)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        q, k, v, do = ((qmul * rnd(B, L, H * D)).to(td), rnd(B, L, H * D).to(td), rnd(B, L, H * D).to(td), rnd(B, L, H * D).to(td))
        wl, ww = rnd(H, H) / H ** 0.5 + 0.3 * torch.eye(H), rnd(H, H) / H ** 0.5 + 0.3 * torch.eye(H)
        bl, bw = 0.5 * rnd(H), 0.1 * rnd(H)
        scale = D ** -0.5
        leaves = [t.double().detach().requires_grad_(True) for t in (q, k, v, wl, bl, ww, bw)]
        q64, k64, v64, wl64, bl64, ww64, bw64 = leaves
        A = scale * _heads(q64, H) @ _heads(k64, H).transpose(-1, -2)
        M = torch.einsum("gh,bhij->bgij", wl64, A) + bl64[None, :, None, None]
        P = torch.softmax(M, -1)
        R = torch.einsum("gh,bhij->bgij", ww64, P) + bw64[None, :, None, None]
        o64 = _rows(R @ _heads(v64, H))
        dq, dk, dv, dwl, dbl, dww, dbw = torch.autograd.grad(o64, leaves, do.double())
        want = dict(O=o64.detach(), dQ=dq, dK=dk, dV=dv, dWl=dwl, dWw=dww, dbw=dbw, dbl=dbl)
        emu = {}
        if dtype == N.VT_BF16:
            emu = dict(zip(("dQ", "dK", "dV"), _emulate([want[n] for n in ("dQ", "dK", "dV")])))
            # the forward runs on the matrix unit: R is rounded to bf16 as the operand of R V, then the store
            emu["O"] = _emulate([_rows(R.detach().to(torch.bfloat16).double() @ _heads(v64.detach(), H))])[0]
        _CASES[key] = dict(q=q, k=k, v=v, do=do, wl=wl, bl=bl, ww=ww, bw=bw, scale=scale, want=want, emu=emu,
                           lse=torch.logsumexp(M.detach(), -1), top=M.detach().abs().max().item(),
                           m_std=(M.detach() - M.detach().mean(-1, keepdim=True)).std().item())
    return _CASES[key]


def _cls_case(shape, dtype, qmul=1.0):
    key = ("cls", shape, dtype, qmul)
    if key not in _CASES:
        B, H, Lk, D = shape
        td = TD[dtype]
        gen = torch.Generator().manual_seed(7000 * Lk + 10 * H + D)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        q, do = (qmul * rnd(B, H * D)).to(td), rnd(B, H * D).to(td)
        k, v = rnd(B, Lk, H * D).to(td), rnd(B, Lk, H * D).to(td)
        scale = D ** -0.5
        q64, k64, v64 = (t.double().detach().requires_grad_(True) for t in (q, k, v))
        qh = q64.reshape(B, H, 1, D)
        o64 = F.scaled_dot_product_attention(qh, _heads(k64, H), _heads(v64, H)).reshape(B, H * D)
        dq, dk, dv = torch.autograd.grad(o64, (q64, k64, v64), do.double())
        S = scale * qh.detach() @ _heads(k64.detach(), H).transpose(-1, -2)  # [B, H, 1, Lk]
        want = dict(O=o64.detach(), dQ=dq, dK=dk, dV=dv)
        emu = dict(zip(want, _emulate(list(want.values())))) if dtype == N.VT_BF16 else {}
        _CASES[key] = dict(q=q, k=k, v=v, do=do, scale=scale, want=want, emu=emu, lse=torch.logsumexp(S, -1).reshape(B, H),
                           top=S.abs().max().item())
    return _CASES[key]


def test_emulated_rounding_points():
    """the table of the module docstring: pure torch on the CPU, over every listed shape.  Every emulated error stays under a
    third of 2^-7, so the rule gives 2^-7 for every bf16 output, which is what `_bound` states"""
    for kind, shapes, case in (("talk", TALK_SHAPES, _talk_case), ("cls", CLS_SHAPES, _cls_case)):
        for shape in shapes:
            c = case(shape, N.VT_BF16)
            errs = {n: rel_err(e, c["want"][n]) for n, e in c["emu"].items()}
            print(f"{kind} {'x'.join(map(str, shape))}: emulated " + " ".join(f"{n} {e:.3e}" for n, e in errs.items())
                  + f" (a third of 2^-7: {BF16_REL / 3:.3e})")
            for n, e in errs.items():
                assert e < BF16_REL / 3 and _bound(n, shape) == BF16_REL, (kind, shape, n, e)
    for c in (_talk_case((1, 2, 65, 48), N.VT_BF16, qmul=32.0), _cls_case((2, 4, 197, 48), N.VT_BF16, qmul=32.0)):
        assert all(rel_err(c["emu"][n], c["want"][n]) < BF16_REL / 3 for n in ("O", "dV"))


def _dev(c, *names):
    return [c[n].cuda() for n in names]


def _ld(t):
    return t.stride(-2) if t is not None else 0


def _talk_fwd(lib, q, k, v, o, lse, mix, scale, shape, dtype):
    B, H, L, D = shape
    N.check(lib.vt_talk_attn_fwd(vp(q), _ld(q), vp(k), _ld(k), vp(v), _ld(v), vp(o), _ld(o), vp(lse), *[vp(m) for m in mix], scale, B,
                                 H, L, D, dtype, stream()))
    torch.cuda.synchronize()


def _talk_bwd(lib, q, k, v, do, lse, mix, dq, dk, dv, pg, scale, shape, dtype):
    B, H, L, D = shape
    nbytes = int(lib.vt_talk_attn_bwd_scratch_bytes(B, H, L))
    assert nbytes == 4 * (B * H * L + B * ((L + 15) // 16) * (2 * H * H + 2 * H))  # the formula of include/vt_amd.h
    scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
    N.check(lib.vt_talk_attn_bwd(vp(q), _ld(q), vp(k), _ld(k), vp(v), _ld(v), vp(do), _ld(do), vp(lse), *[vp(m) for m in mix],
                                 vp(dq), _ld(dq), vp(dk), _ld(dk), vp(dv), _ld(dv), *[vp(g) for g in pg], vp(scratch), nbytes, scale,
                                 B, H, L, D, dtype, stream()))
    torch.cuda.synchronize()


def _talk_run(shape, dtype, c, ops=None, start=0.0):
    """forward and backward on dense buffers (or on `ops` = (q, k, v, do, o, dq, dk, dv) views); the parameter gradients
    start at `start`"""
    B, H, L, D = shape
    td, lib = TD[dtype], N.lib()
    nan = lambda: torch.full((B, L, H * D), float("nan"), device="cuda", dtype=td)  # noqa: E731
    if ops is None:
        ops = (*_dev(c, "q", "k", "v", "do"), nan(), nan(), nan(), nan())
    q, k, v, do, o, dq, dk, dv = ops
    mix = _dev(c, "wl", "bl", "ww", "bw")
    lse = torch.full((B, H, L), float("nan"), device="cuda")
    _talk_fwd(lib, q, k, v, o, lse, mix, c["scale"], shape, dtype)
    pg = [torch.full_like(m, start) for m in mix]  # dwl dbl dww dbw
    _talk_bwd(lib, q, k, v, do, lse, mix, dq, dk, dv, pg, c["scale"], shape, dtype)
    return dict(O=o, lse=lse, dQ=dq, dK=dk, dV=dv, dWl=pg[0], dbl=pg[1], dWw=pg[2], dbw=pg[3])


def _talk_check(tag, shape, dtype, c, got, names=("O", "dQ", "dK", "dV", "dWl", "dWw", "dbw"), start=0.0):
    _check(f"{tag} lse", got["lse"], c["lse"], dtype, f32_out=True)
    for n in names:
        param = n in ("dWl", "dWw", "dbw")  # f32 sums of f32 terms in both dtypes: the f32 rule, like lse
        want = c["want"][n] + (start if param else 0.0)
        _check(f"{tag} {n}", got[n], want, dtype, f32_out=param, emu=c["emu"].get(n), bound=_bound(n, shape))
    assert bool(torch.isfinite(got["dbl"]).all())
    print(f"{tag} dbl: largest |value - start| {(got['dbl'] - start).abs().max().item():.3e} (exactly zero in exact arithmetic; "
          f"float64 autograd {c['want']['dbl'].abs().max().item():.1e}; recorded, not compared)")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", TALK_SHAPES, ids=_ids(TALK_SHAPES))
def test_talking_attention_matches_autograd_in_float64(shape, dtype):
    c = _talk_case(shape, dtype)
    print(f"mixed score std {c['m_std']:.2f}")
    _talk_check("x".join(map(str, shape)), shape, dtype, c, _talk_run(shape, dtype, c))


def _wide(n, B, L, C, td, fills=None):
    """n [B][L][C] channel slices of one NaN-filled [B][L][8 + n C + 8] buffer"""
    wide = torch.full((B, L, n * C + 16), float("nan"), device="cuda", dtype=td)
    views = [wide[:, :, 8 + i * C:8 + (i + 1) * C] for i in range(n)]
    for dst, src in zip(views, fills or ()):
        dst.copy_(src)
    return wide, views


def _nan_around(wide, width):
    return bool(torch.isnan(wide[..., :8].float()).all() and torch.isnan(wide[..., 8 + width:].float()).all())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_talking_attention_on_channel_slices_of_nan_filled_buffers(dtype):
    shape = (1, 3, 64, 48)
    B, H, L, D = shape
    C, td = H * D, TD[dtype]
    c = _talk_case(shape, dtype)
    qkv_w, (q, k, v) = _wide(3, B, L, C, td, _dev(c, "q", "k", "v"))
    o_w, (o,) = _wide(1, B, L, C, td)
    do_w, (do,) = _wide(1, B, L, C, td, _dev(c, "do"))
    g_w, (dq, dk, dv) = _wide(3, B, L, C, td)
    got = _talk_run(shape, dtype, c, ops=(q, k, v, do, o, dq, dk, dv))
    assert _nan_around(qkv_w, 3 * C) and _nan_around(o_w, C) and _nan_around(g_w, 3 * C) and _nan_around(do_w, C)
    _talk_check("slices", shape, dtype, c, got)
    dense = _talk_run(shape, dtype, c)  # strides change addresses, not arithmetic
    for n in got:
        assert torch.equal(got[n].float(), dense[n].float()), n


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_talking_attention_with_large_scores_stays_finite_and_in_bound(dtype):
    shape = (1, 2, 65, 48)
    c = _talk_case(shape, dtype, qmul=32.0)
    print(f"largest |M| {c['top']:.1f}")
    assert c["top"] > 89.0  # exp overflows f32 above 88.7: a kernel that does not subtract the row maximum cannot pass
    got = _talk_run(shape, dtype, c)
    _talk_check("Q*32", shape, dtype, c, got, names=("O", "dV"))
    for n in ("dQ", "dK"):
        assert bool(torch.isfinite(got[n].float()).all())
        print(f"Q*32 {n}: norm-relative {rel_err(got[n].cpu(), c['want'][n]):.3e} (recorded, not asserted)")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_talking_attention_is_bit_identical_each_gradient_works_alone_and_parameters_accumulate(dtype):
    shape = (2, 4, 196, 48)
    B, H, L, D = shape
    c = _talk_case(shape, dtype)
    td, lib = TD[dtype], N.lib()
    a, b = _talk_run(shape, dtype, c), _talk_run(shape, dtype, c)
    for n in a:
        assert torch.equal(a[n].float(), b[n].float()), n
    q, k, v, do = _dev(c, "q", "k", "v", "do")
    mix = _dev(c, "wl", "bl", "ww", "bw")
    for i, n in enumerate(("dQ", "dK", "dV")):
        outs = [None, None, None]
        outs[i] = torch.full((B, L, H * D), float("nan"), device="cuda", dtype=td)
        _talk_bwd(lib, q, k, v, do, a["lse"], mix, *outs, [None] * 4, c["scale"], shape, dtype)
        assert torch.equal(outs[i].float(), a[n].float()), n
    for i, n in enumerate(("dWl", "dbl", "dWw", "dbw")):
        pg = [None] * 4
        pg[i] = torch.zeros_like(mix[i])
        _talk_bwd(lib, q, k, v, do, a["lse"], mix, None, None, None, pg, c["scale"], shape, dtype)
        assert torch.equal(pg[i], a[n]), n
    # onto a non-zero start: += in f32
    got = _talk_run(shape, dtype, c, start=0.75)
    _talk_check("start 0.75", shape, dtype, c, got, names=("dWl", "dWw", "dbw"), start=0.75)


def _cls_run(shape, dtype, c, ops=None):
    B, H, Lk, D = shape
    td, lib = TD[dtype], N.lib()
    if ops is None:
        nan = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=td)  # noqa: E731
        ops = (*_dev(c, "q", "k", "v", "do"), nan(B, H * D), nan(B, H * D), nan(B, Lk, H * D), nan(B, Lk, H * D))
    q, k, v, do, o, dq, dk, dv = ops
    lse = torch.full((B, H), float("nan"), device="cuda")
    sq = lambda t: t.stride(0)  # noqa: E731  ([B][C] rows)
    N.check(lib.vt_cls_attn_fwd(vp(q), sq(q), vp(k), _ld(k), vp(v), _ld(v), vp(o), sq(o), vp(lse), c["scale"], B, H, Lk, D, dtype,
                                stream()))
    torch.cuda.synchronize()
    _cls_bwd(lib, q, k, v, o, do, lse, dq, dk, dv, c["scale"], shape, dtype)
    return dict(O=o, lse=lse, dQ=dq, dK=dk, dV=dv)


def _cls_bwd(lib, q, k, v, o, do, lse, dq, dk, dv, scale, shape, dtype):
    B, H, Lk, D = shape
    sq = lambda t: t.stride(0) if t is not None else 0  # noqa: E731
    N.check(lib.vt_cls_attn_bwd(vp(q), sq(q), vp(k), _ld(k), vp(v), _ld(v), vp(o), sq(o), vp(do), sq(do), vp(lse), vp(dq), sq(dq),
                                vp(dk), _ld(dk), vp(dv), _ld(dv), scale, B, H, Lk, D, dtype, stream()))
    torch.cuda.synchronize()


def _cls_check(tag, shape, dtype, c, got, names=("O", "dQ", "dK", "dV")):
    _check(f"{tag} lse", got["lse"], c["lse"], dtype, f32_out=True)
    for n in names:
        _check(f"{tag} {n}", got[n], c["want"][n], dtype, emu=c["emu"].get(n), bound=_bound(n, shape))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", CLS_SHAPES, ids=_ids(CLS_SHAPES))
def test_class_attention_matches_sdpa_and_autograd_in_float64(shape, dtype):
    c = _cls_case(shape, dtype)
    _cls_check("x".join(map(str, shape)), shape, dtype, c, _cls_run(shape, dtype, c))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_class_attention_on_channel_slices_of_nan_filled_buffers(dtype):
    shape = (2, 4, 197, 48)
    B, H, Lk, D = shape
    C, td = H * D, TD[dtype]
    c = _cls_case(shape, dtype)
    kv_w, (k, v) = _wide(2, B, Lk, C, td, _dev(c, "k", "v"))
    g_w, (dk, dv) = _wide(2, B, Lk, C, td)
    row_w = torch.full((B, 4 * C + 16), float("nan"), device="cuda", dtype=td)  # q | do | o | dq
    q, do, o, dq = (row_w[:, 8 + i * C:8 + (i + 1) * C] for i in range(4))
    q.copy_(c["q"])
    do.copy_(c["do"])
    got = _cls_run(shape, dtype, c, ops=(q, k, v, do, o, dq, dk, dv))
    assert _nan_around(kv_w, 2 * C) and _nan_around(g_w, 2 * C) and _nan_around(row_w, 4 * C)
    _cls_check("slices", shape, dtype, c, got)
    dense = _cls_run(shape, dtype, c)
    for n in got:
        assert torch.equal(got[n].float(), dense[n].float()), n


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_class_attention_large_scores_bit_identical_and_each_gradient_alone(dtype):
    shape = (2, 4, 197, 48)
    B, H, Lk, D = shape
    c = _cls_case(shape, dtype, qmul=32.0)
    print(f"largest |score| {c['top']:.1f}")
    assert c["top"] > 89.0
    a, b = _cls_run(shape, dtype, c), _cls_run(shape, dtype, c)
    _cls_check("Q*32", shape, dtype, c, a, names=("O", "dV"))
    for n in ("dQ", "dK"):
        assert bool(torch.isfinite(a[n].float()).all())
        print(f"Q*32 {n}: norm-relative {rel_err(a[n].cpu(), c['want'][n]):.3e} (recorded, not asserted)")
    for n in a:
        assert torch.equal(a[n].float(), b[n].float()), n
    td, lib = TD[dtype], N.lib()
    q, k, v, do = _dev(c, "q", "k", "v", "do")
    for i, n in enumerate(("dQ", "dK", "dV")):
        outs = [None, None, None]
        outs[i] = torch.full_like(a[n], float("nan"))
        _cls_bwd(lib, q, k, v, a["O"], do, a["lse"], *outs, c["scale"], shape, dtype)
        assert torch.equal(outs[i].float(), a[n].float()), n


def test_talking_and_class_attention_reject_what_they_do_not_implement():
    lib = N.lib()
    B, H, L = 1, 2, 16
    bf = N.VT_BF16
    lse = torch.zeros(B, 17, L, device="cuda")
    w = torch.zeros(17, 17, device="cuda")
    scratch = torch.zeros(int(lib.vt_talk_attn_bwd_scratch_bytes(B, 17, L)) // 4, device="cuda")
    sb = scratch.numel() * 4
    t = torch.zeros(B, L, 17 * 64, device="cuda", dtype=torch.bfloat16)

    def fwd(t, ld, heads, D):
        return lib.vt_talk_attn_fwd(vp(t), ld, vp(t), ld, vp(t), ld, vp(t), ld, vp(lse), vp(w), None, vp(w), None, 0.1, B, heads, L,
                                    D, bf, stream())

    def bwd(t, ld, heads, D, dq, dwl, nbytes):
        return lib.vt_talk_attn_bwd(vp(t), ld, vp(t), ld, vp(t), ld, vp(t), ld, vp(lse), vp(w), None, vp(w), None, vp(dq), ld, None,
                                    0, None, 0, vp(dwl), None, None, None, vp(scratch), nbytes, 0.1, B, heads, L, D, bf, stream())

    assert fwd(t, 128, H, 64) == N.VT_ERR_UNSUPPORTED and "head_dim" in N.last_error()
    assert bwd(t, 128, H, 64, t, None, sb) == N.VT_ERR_UNSUPPORTED and "head_dim" in N.last_error()
    assert fwd(t, 17 * 48, 17, 48) == N.VT_ERR_UNSUPPORTED and "heads" in N.last_error()
    assert bwd(t, 17 * 48, 17, 48, t, None, sb) == N.VT_ERR_UNSUPPORTED and "heads" in N.last_error()
    t52 = torch.zeros(B, L, 104, device="cuda", dtype=torch.bfloat16)
    assert fwd(t52, 52, 1, 48) == N.VT_ERR_INVALID and "row stride 52" in N.last_error()
    t = torch.zeros(B, L, 96, device="cuda", dtype=torch.bfloat16)
    assert bwd(t, 96, H, 48, None, None, sb) == N.VT_ERR_INVALID and "no output" in N.last_error()
    assert bwd(t, 96, H, 48, t, None, 16) == N.VT_ERR_INVALID and "scratch" in N.last_error()
    assert bwd(t, 96, H, 48, None, w, 16) == N.VT_ERR_INVALID and "scratch" in N.last_error()
    # class attention: head_dim 80, a row stride of 52, no output
    row = torch.zeros(B, 160, device="cuda", dtype=torch.bfloat16)
    t = torch.zeros(B, L, 160, device="cuda", dtype=torch.bfloat16)
    rc = lib.vt_cls_attn_fwd(vp(row), 160, vp(t), 160, vp(t), 160, vp(row), 160, vp(lse), 0.1, B, H, L, 80, bf, stream())
    assert rc == N.VT_ERR_UNSUPPORTED and "head_dim" in N.last_error()
    rc = lib.vt_cls_attn_fwd(vp(row), 52, vp(t52), 52, vp(t52), 52, vp(row), 52, vp(lse), 0.1, B, 1, L, 48, bf, stream())
    assert rc == N.VT_ERR_INVALID and "row stride 52" in N.last_error()
    rc = lib.vt_cls_attn_bwd(vp(row), 96, vp(t), 96, vp(t), 96, vp(row), 96, vp(row), 96, vp(lse), None, 0, None, 0, None, 0, 0.1, B,
                             H, L, 48, bf, stream())
    assert rc == N.VT_ERR_INVALID and "no output" in N.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("param", [True, False], ids=["first_param", "first_rows"])
def test_token_prepend_forward_and_backward_match_torch(param, dtype):
    B, T, C = 3, 9, 40
    td, lib = TD[dtype], N.lib()
    torch.manual_seed(13 + int(param))
    xw, (x,) = _wide(1, B, T, C, td, [torch.randn(B, T, C, device="cuda")])
    first = None if param else torch.randn(B, C, device="cuda").to(td)
    fparam = torch.randn(C, device="cuda") if param else None
    ow, (out,) = _wide(1, B, T + 1, C, td)
    N.check(lib.vt_token_prepend_fwd(vp(x), x.stride(1), vp(first), C, vp(fparam), vp(out), out.stride(1), B, T, C, dtype, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:].float(), x.float()) and _nan_around(ow, C)
    row0 = fparam.to(td).float().expand(B, C) if param else first.float()
    assert torch.equal(out[:, 0].float(), row0)

    gw, (dout,) = _wide(1, B, T + 1, C, td, [torch.randn(B, T + 1, C, device="cuda") + 0.5])
    for accumulate in (0, 1):
        base = torch.randn(B, T, C, device="cuda").to(td)
        dw, (dx,) = _wide(1, B, T, C, td, [base] if accumulate else None)
        dfirst = None if param else torch.full((B, C), float("nan"), device="cuda", dtype=td)
        dparam = torch.full((C,), 0.25, device="cuda") if param else None
        N.check(lib.vt_token_prepend_bwd(vp(dout), dout.stride(1), vp(dx), dx.stride(1), accumulate, vp(dfirst), C, vp(dparam), B, T,
                                         C, dtype, stream()))
        torch.cuda.synchronize()
        want = (base.float() + dout[:, 1:].float()).to(td).float() if accumulate else dout[:, 1:].float()
        assert torch.equal(dx.float(), want) and _nan_around(dw, C)
        if param:
            s = torch.full((C,), 0.25, device="cuda")
            acc = torch.zeros(C, device="cuda")
            for b in range(B):  # the images in order, in f32
                acc = acc + dout[b, 0].float()
            assert torch.equal(dparam, s + acc)
        else:
            assert torch.equal(dfirst.float(), dout[:, 0].float())
    # the first token's gradient alone (frozen patch tokens)
    if param:
        dparam = torch.zeros(C, device="cuda")
        N.check(lib.vt_token_prepend_bwd(vp(dout), dout.stride(1), None, 0, 0, None, 0, vp(dparam), B, T, C, dtype, stream()))
        torch.cuda.synchronize()
        _check("d first_param alone", dparam, dout[:, 0].double().sum(0), dtype, f32_out=True)
    rc = lib.vt_token_prepend_fwd(vp(x), x.stride(1), None, 0, None, vp(out), out.stride(1), B, T, C, dtype, stream())
    assert rc == N.VT_ERR_INVALID and "exactly one" in N.last_error()
    rc = lib.vt_token_prepend_bwd(vp(dout), dout.stride(1), None, 0, 0, None, 0, None, B, T, C, dtype, stream())
    assert rc == N.VT_ERR_INVALID and "no output" in N.last_error()
