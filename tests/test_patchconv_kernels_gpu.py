"""vt_dw3_gelu_pool_fwd / _bwd, vt_se_gate_fwd / _bwd, vt_channel_stats and vt_pool_attn_fwd / _bwd (vt_patchconv.hip)
through the C-ABI against torch in float64 on the operands as the kernels read them: the activations as stored, the
depthwise filter as the launch rounds it (bf16 launches round the f32 master as the conv kernels' mirror does; with the
unrounded master as the reference, the f32 filter and bias gradients of a bf16 launch could not be held to the f32 rule, as
GELU' is taken at a z made from the rounded filter).

Shapes.  dw column (B, H, W, C): (2,14,14,64), (1,3,5,8), (3,1,1,8), (2,7,9,72), (1,24,24,16); one more on channel slices of
NaN-filled wider buffers with the residual aliasing du: the surroundings stay NaN, the results are bit-equal to the dense
run.  SE gate (B, HW, C): (2,196,64), (1,15,8), (3,1,72).  Channel statistics (M, C): (1,8), (27,72), (392,64), against
float64 sums and against what vt_conv_igemm gives for an identity filter.  Pool attention (B, Lk, C): (2,197,384), (1,2,8),
(3,10,72), (2,65,1024); one with k | v as slices of a [.., 2C] buffer; one with the scores scaled by 32.

Bounds, the rules of tests/test_talking_attention_gpu.py.  f32 outputs and every f32 parameter gradient (dw, dbias, the gate's
ds, lse) in both dtypes: `_check`, rtol 1e-4 with an atol of 1e-4 of the largest magnitude.  Fixed-point statistics: 1e-6 of
their scale sum |terms| (tests/test_layernorm_gpu.py).  bf16 outputs: norm-relative 2^-7 where a float64 emulation of the
kernel's bf16 rounding points stays under a third of it, else three times the emulated error.  The rounding points: the
stores (a, pooled, du -- with a residual the sum is stored first, then the add -- y, da, o, dq, dk, dv), the stored a inside
pooled (the mean is taken over the stored values) and the stored o inside delta = dout . o.  test_emulated_rounding_points
prints every emulated error and asserts the bound the rule gives.  Two runs of every backward are bit-identical."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, conv_desc, rel_err, stream, vp

pytestmark = pytest.mark.gpu

DW_SHAPES = [(2, 14, 14, 64), (1, 3, 5, 8), (3, 1, 1, 8), (2, 7, 9, 72), (1, 24, 24, 16)]
SE_SHAPES = [(2, 196, 64), (1, 15, 8), (3, 1, 72)]
STAT_SHAPES = [(1, 8), (27, 72), (392, 64)]
POOL_SHAPES = [(2, 197, 384), (1, 2, 8), (3, 10, 72), (2, 65, 1024)]
BF16_REL = 2.0 ** -7
DT = [N.VT_F32, N.VT_BF16]
DT_IDS = ["f32", "bf16"]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]  # noqa: E731
_CASES = {}


def _bf(t):
    return t.to(torch.bfloat16).double()


def _bound(emu_err):
    """2^-7 where the emulated rounding points stay under a third of it, else three times the emulated error"""
    return BF16_REL if emu_err < BF16_REL / 3 else 3 * emu_err


def _check(tag, got, want, dtype, f32_out=False, emu=None):
    got, want = got.double().cpu(), want.double().cpu()
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    if dtype == N.VT_F32 or f32_out:
        atol = 1e-4 * want.abs().max().item()
        worst = ((got - want).abs() / (atol + 1e-4 * want.abs())).max().item()
        print(f"{tag}: worst |err| / (atol + rtol |ref|) = {worst:.3e} (bound 1), atol {atol:.3e}")
        assert worst < 1.0, tag
    else:
        e, ee = rel_err(got, want), rel_err(emu, want)
        print(f"{tag}: norm-relative {e:.3e} (bound {_bound(ee):.3e}, emulated rounding points {ee:.3e})")
        assert e < _bound(ee), tag


# ---- depthwise 3x3 + GELU + pool ----------------------------------------------------------------------------------------
def _dw_case(shape, dtype, with_res=False):
    key = ("dw", shape, dtype, with_res)
    if key not in _CASES:
        B, H, W, Cc = shape
        td = TD[dtype]
        gen = torch.Generator().manual_seed(100 * H + 10 * W + Cc)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        u, da, res = rnd(B, H, W, Cc).to(td), rnd(B, H, W, Cc).to(td), rnd(B, H, W, Cc).to(td)
        dp = rnd(B, Cc).to(td)
        w, bias = 0.4 * rnd(Cc, 9), 0.2 * rnd(Cc)
        wr = w.to(td).float()  # the filter as the launch reads it
        u64 = u.double().permute(0, 3, 1, 2).detach().requires_grad_(True)
        w64, b64 = wr.double().requires_grad_(True), bias.double().requires_grad_(True)
        a64 = F.gelu(F.conv2d(u64, w64.view(Cc, 1, 3, 3), b64, padding=1, groups=Cc))
        p64 = a64.mean((2, 3))
        loss = (a64 * da.double().permute(0, 3, 1, 2)).sum() + (p64 * dp.double()).sum()
        du, dw, db = torch.autograd.grad(loss, (u64, w64, b64))
        a_ = a64.detach().permute(0, 2, 3, 1)
        du_ = du.permute(0, 2, 3, 1) + (res.double() if with_res else 0.0)
        want = dict(a=a_, pooled=p64.detach(), du=du_, dw=dw, dbias=db)
        emu = {}
        if dtype == N.VT_BF16:
            emu["a"] = _bf(a_)
            emu["pooled"] = _bf(emu["a"].mean((1, 2)))
            emu["du"] = _bf(_bf(du.permute(0, 2, 3, 1)) + res.double()) if with_res else _bf(du_)
        _CASES[key] = dict(u=u, da=da, dp=dp, res=res, w=w, bias=bias, want=want, emu=emu)
    return _CASES[key]


def _wide(t, ld, coff):
    wide = torch.full((*t.shape[:-1], ld), float("nan"), device="cuda", dtype=t.dtype)
    wide[..., coff:coff + t.shape[-1]] = t
    return wide, wide[..., coff:coff + t.shape[-1]]


def _dw_run(shape, dtype, c, with_res=False, sliced=False, start=0.5):
    B, H, W, Cc = shape
    td, lib = TD[dtype], N.lib()
    u, da, dp = c["u"].cuda(), c["da"].cuda(), c["dp"].cuda()
    w, bias = c["w"].cuda(), c["bias"].cuda()
    a = torch.full((B, H, W, Cc), float("nan"), device="cuda", dtype=td)
    du = torch.full((B, H, W, Cc), float("nan"), device="cuda", dtype=td)
    res = c["res"].cuda() if with_res else None
    wides = []
    if sliced:
        (uw, u), (daw, da), (aw, a) = _wide(u, Cc + 16, 8), _wide(da, Cc + 8, 0), _wide(a, Cc + 24, 16)
        duw, du = _wide(c["res"].cuda(), Cc + 8, 8)  # the residual aliases du
        res, wides = du, [(uw, 8), (daw, 0), (aw, 16), (duw, 8)]
    pooled = torch.full((B, Cc), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_dw3_gelu_pool_fwd(vp(u), u.stride(2), vp(w), vp(bias), vp(a), a.stride(2), vp(pooled), Cc, B, H, W, Cc, dtype,
                                     stream()))
    nbytes = int(lib.vt_dw3_gelu_pool_bwd_scratch_bytes(B, Cc))
    assert nbytes == B * Cc * 10 * 4
    scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
    dw, db = torch.full((Cc, 9), start, device="cuda"), torch.full((Cc,), start, device="cuda")
    N.check(lib.vt_dw3_gelu_pool_bwd(vp(u), u.stride(2), vp(da), da.stride(2), vp(dp), Cc, vp(w), vp(bias), vp(du), du.stride(2),
                                     vp(res), res.stride(2) if res is not None else 0, vp(dw), vp(db), vp(scratch), nbytes, B, H, W,
                                     Cc, dtype, stream()))
    torch.cuda.synchronize()
    for wide, coff in wides:  # the surroundings of every slice stay NaN
        mask = torch.ones(wide.shape[-1], dtype=torch.bool, device="cuda")
        mask[coff:coff + Cc] = False
        assert bool(torch.isnan(wide[..., mask]).all())
    return dict(a=a, pooled=pooled, du=du, dw=dw, dbias=db)


def _dw_check(tag, dtype, c, got, start=0.5):
    for n in ("a", "pooled", "du"):
        _check(f"{tag} {n}", got[n], c["want"][n], dtype, emu=c["emu"].get(n))
    _check(f"{tag} dw", got["dw"], c["want"]["dw"] + start, dtype, f32_out=True)
    _check(f"{tag} dbias", got["dbias"], c["want"]["dbias"] + start, dtype, f32_out=True)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", DW_SHAPES, ids=_ids(DW_SHAPES))
def test_dw3_gelu_pool_matches_autograd_in_float64(shape, dtype):
    before = N.launch_count()
    c = _dw_case(shape, dtype)
    got = _dw_run(shape, dtype, c)
    _dw_check("x".join(map(str, shape)), dtype, c, got)
    again = _dw_run(shape, dtype, c)
    assert all(torch.equal(got[n], again[n]) for n in got), "two runs differ"
    assert N.launch_count() >= before + 6


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_dw3_gelu_pool_on_channel_slices_with_the_residual_aliasing_du(dtype):
    shape = (2, 7, 9, 72)
    c = _dw_case(shape, dtype, with_res=True)
    dense = _dw_run(shape, dtype, c, with_res=True)
    _dw_check("dense + residual", dtype, c, dense)
    sl = _dw_run(shape, dtype, c, with_res=True, sliced=True)
    assert all(torch.equal(dense[n], sl[n]) for n in dense)


# ---- the sigmoid gate -----------------------------------------------------------------------------------------------
def _se_case(shape, dtype):
    key = ("se", shape, dtype)
    if key not in _CASES:
        B, HW, Cc = shape
        td = TD[dtype]
        gen = torch.Generator().manual_seed(10 * HW + Cc)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        a, dy, s = rnd(B, HW, Cc).to(td), rnd(B, HW, Cc).to(td), (1.5 * rnd(B, Cc)).to(td)
        a64, s64 = a.double().requires_grad_(True), s.double().requires_grad_(True)
        y = a64 * torch.sigmoid(s64)[:, None, :]
        da, ds = torch.autograd.grad(y, (a64, s64), dy.double())
        want = dict(y=y.detach(), da=da, ds=ds)
        emu = {n: _bf(want[n]) for n in ("y", "da")} if dtype == N.VT_BF16 else {}
        _CASES[key] = dict(a=a, dy=dy, s=s, want=want, emu=emu)
    return _CASES[key]


def _se_run(shape, dtype, c):
    B, HW, Cc = shape
    td, lib = TD[dtype], N.lib()
    a, dy, s = c["a"].cuda(), c["dy"].cuda(), c["s"].cuda()
    y, da = torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))
    ds = torch.full((B, Cc), float("nan"), device="cuda")
    N.check(lib.vt_se_gate_fwd(vp(a), Cc, vp(s), Cc, vp(y), Cc, B, HW, Cc, dtype, stream()))
    N.check(lib.vt_se_gate_bwd(vp(dy), Cc, vp(a), Cc, vp(s), Cc, vp(da), Cc, vp(ds), B, HW, Cc, 0, dtype, stream()))
    torch.cuda.synchronize()
    return dict(y=y, da=da, ds=ds)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", SE_SHAPES, ids=_ids(SE_SHAPES))
def test_se_gate_matches_autograd_in_float64(shape, dtype):
    before = N.launch_count()
    c = _se_case(shape, dtype)
    got = _se_run(shape, dtype, c)
    tag = "x".join(map(str, shape))
    for n in ("y", "da"):
        _check(f"{tag} {n}", got[n], c["want"][n], dtype, emu=c["emu"].get(n))
    _check(f"{tag} ds", got["ds"], c["want"]["ds"], dtype, f32_out=True)
    again = _se_run(shape, dtype, c)
    assert all(torch.equal(got[n], again[n]) for n in got), "two runs differ"
    # accumulate: da += on top of what is there
    B, HW, Cc = shape
    da2 = got["da"].clone()
    ds = torch.empty((B, Cc), device="cuda")
    dy, a, s = c["dy"].cuda(), c["a"].cuda(), c["s"].cuda()
    N.check(N.lib().vt_se_gate_bwd(vp(dy), Cc, vp(a), Cc, vp(s), Cc, vp(da2), Cc, vp(ds), B, HW, Cc, 1, dtype, stream()))
    torch.cuda.synchronize()
    _check(f"{tag} da (accumulated)", da2, 2 * c["want"]["da"], dtype,
           emu=_bf(2 * _bf(c["want"]["da"])) if dtype == N.VT_BF16 else None)
    assert N.launch_count() >= before + 5


# ---- channel statistics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", STAT_SHAPES, ids=_ids(STAT_SHAPES))
def test_channel_stats_match_float64_and_an_identity_convolution(shape, dtype):
    before = N.launch_count()
    M, Cc = shape
    td, lib = TD[dtype], N.lib()
    gen = torch.Generator().manual_seed(10 * M + Cc)
    x = (torch.randn(M, Cc, generator=gen) * 2 + 0.5).to(td)
    wide, xs = _wide(x.cuda(), Cc + 8, 8)
    st = N.stats_buffer(Cc)
    N.check(lib.vt_channel_stats(vp(xs), xs.stride(0), M, Cc, dtype, vp(st), stream()))
    st2 = N.stats_buffer(Cc)
    N.check(lib.vt_channel_stats(vp(xs), xs.stride(0), M, Cc, dtype, vp(st2), stream()))
    # what the convolution's epilogue gives for an identity filter: z = x, stored, then summed
    xm = x.cuda().reshape(M, 1, 1, Cc).contiguous()
    eye = torch.eye(Cc).reshape(Cc, 1, 1, Cc).contiguous().to("cuda", td)
    z = torch.empty_like(xm)
    stc = N.stats_buffer(Cc)
    d = conv_desc(dtype, xm, Cc, Cc, 1, 1, 0, Cc, flags=N.VT_CONV_STATS)
    N.check(lib.vt_conv_igemm(C.byref(d), vp(xm), vp(eye), vp(z), None, None, None, vp(stc), stream()))
    torch.cuda.synchronize()
    got, conv = N.stats_decode(st).cpu(), N.stats_decode(stc).cpu()
    assert torch.equal(got, N.stats_decode(st2).cpu()), "two runs differ"
    assert torch.equal(z, xm)
    x64 = x.double()
    for k, terms in enumerate((x64, x64 * x64)):
        want, scale = terms.sum(0), terms.abs().sum(0).clamp_min(1e-30)
        e = ((got[k] - want).abs() / scale).max().item()
        ec = ((got[k] - conv[k]).abs() / scale).max().item()
        print(f"M={M} C={Cc}: sums[{k}] {e:.2e} of scale against float64, {ec:.2e} against the identity convolution")
        assert e < 1e-6 and ec < 2e-6
    assert N.launch_count() >= before + 3


# ---- attention pooling ------------------------------------------------------------------------------------------------
def _pool_case(shape, dtype, qmul=1.0):
    key = ("pool", shape, dtype, qmul)
    if key not in _CASES:
        B, Lk, Cc = shape
        td = TD[dtype]
        gen = torch.Generator().manual_seed(1000 * Lk + Cc)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        q, do = (qmul * rnd(B, Cc)).to(td), rnd(B, Cc).to(td)
        k, v = rnd(B, Lk, Cc).to(td), rnd(B, Lk, Cc).to(td)
        scale = Cc ** -0.5
        q64, k64, v64 = (t.double().detach().requires_grad_(True) for t in (q, k, v))
        S = scale * torch.einsum("bc,bjc->bj", q64, k64)
        P = torch.softmax(S, -1)
        o64 = torch.einsum("bj,bjc->bc", P, v64)
        dq, dk, dv = torch.autograd.grad(o64, (q64, k64, v64), do.double())
        want = dict(O=o64.detach(), dQ=dq, dK=dk, dV=dv)
        emu = {}
        if dtype == N.VT_BF16:  # the stores, and the STORED o inside delta = dout . o
            P_, g = P.detach(), do.double()
            delta = (g * _bf(o64.detach())).sum(-1, keepdim=True)
            dS = P_ * (torch.einsum("bc,bjc->bj", g, v64.detach()) - delta)
            emu = dict(O=_bf(o64.detach()), dQ=_bf(scale * torch.einsum("bj,bjc->bc", dS, k64.detach())),
                       dK=_bf(scale * dS[..., None] * q64.detach()[:, None, :]), dV=_bf(P_[..., None] * g[:, None, :]))
        _CASES[key] = dict(q=q, k=k, v=v, do=do, scale=scale, want=want, emu=emu, lse=torch.logsumexp(S.detach(), -1),
                           top=S.detach().abs().max().item())
    return _CASES[key]


def _pool_run(shape, dtype, c, kv_sliced=False):
    B, Lk, Cc = shape
    td, lib = TD[dtype], N.lib()
    q, k, v, do = (c[n].cuda() for n in ("q", "k", "v", "do"))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=td)  # noqa: E731
    o, dq, dk, dv = nan(B, Cc), nan(B, Cc), nan(B, Lk, Cc), nan(B, Lk, Cc)
    if kv_sliced:  # k | v and dk | dv as the two halves of [.., 2C] buffers
        kv, dkv = torch.cat((k, v), -1), nan(B, Lk, 2 * Cc)
        k, v, dk, dv = kv[..., :Cc], kv[..., Cc:], dkv[..., :Cc], dkv[..., Cc:]
    lse = torch.full((B,), float("nan"), device="cuda")
    N.check(lib.vt_pool_attn_fwd(vp(q), Cc, vp(k), k.stride(1), vp(v), v.stride(1), vp(o), Cc, vp(lse), c["scale"], B, Lk, Cc, dtype,
                                 stream()))
    N.check(lib.vt_pool_attn_bwd(vp(q), Cc, vp(k), k.stride(1), vp(v), v.stride(1), vp(o), Cc, vp(do), Cc, vp(lse), vp(dq), Cc,
                                 vp(dk), dk.stride(1), vp(dv), dv.stride(1), c["scale"], B, Lk, Cc, dtype, stream()))
    torch.cuda.synchronize()
    return dict(O=o, lse=lse, dQ=dq, dK=dk, dV=dv)


def _pool_check(tag, dtype, c, got, names=("O", "dQ", "dK", "dV")):
    _check(f"{tag} lse", got["lse"], c["lse"], dtype, f32_out=True)
    for n in names:
        _check(f"{tag} {n}", got[n], c["want"][n], dtype, emu=c["emu"].get(n))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_ids(POOL_SHAPES))
def test_pool_attention_matches_autograd_in_float64(shape, dtype):
    before = N.launch_count()
    c = _pool_case(shape, dtype)
    got = _pool_run(shape, dtype, c)
    _pool_check("x".join(map(str, shape)), dtype, c, got)
    again = _pool_run(shape, dtype, c)
    assert all(torch.equal(got[n], again[n]) for n in got), "two runs differ"
    assert N.launch_count() >= before + 4


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_pool_attention_with_k_and_v_as_slices_of_one_buffer(dtype):
    shape = (3, 10, 72)
    c = _pool_case(shape, dtype)
    dense, sl = _pool_run(shape, dtype, c), _pool_run(shape, dtype, c, kv_sliced=True)
    _pool_check("sliced", dtype, c, sl)
    assert all(torch.equal(dense[n], sl[n]) for n in dense)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_pool_attention_with_large_scores_stays_finite(dtype):
    shape = (2, 577, 64)
    c = _pool_case(shape, dtype, qmul=32.0)
    assert c["top"] > 89.0  # exp without the row maximum would overflow f32
    got = _pool_run(shape, dtype, c)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _pool_check("scores x 32", dtype, c, got, names=("O", "dV"))
    print(f"largest |score| {c['top']:.1f}; dQ / dK finite, largest {got['dQ'].abs().max().item():.3e} / "
          f"{got['dK'].abs().max().item():.3e}")


# ---- the rule's inputs, and the refusals ----------------------------------------------------------------------------------
def test_emulated_rounding_points():
    """pure torch on the CPU over every listed shape: prints each emulated error and asserts the bound the rule gives is
    2^-7 or three times the emulated error, and that the emulation is not vacuous"""
    n = 0
    for kind, shapes, case in (("dw", DW_SHAPES, _dw_case), ("se", SE_SHAPES, _se_case), ("pool", POOL_SHAPES, _pool_case)):
        for shape in shapes:
            c = case(shape, N.VT_BF16)
            errs = {k: rel_err(e, c["want"][k]) for k, e in c["emu"].items()}
            print(f"{kind} {'x'.join(map(str, shape))}: emulated " + " ".join(f"{k} {e:.3e}" for k, e in errs.items())
                  + f" (a third of 2^-7: {BF16_REL / 3:.3e})")
            for k, e in errs.items():
                assert 0.0 < e < 2.0 ** -8 and _bound(e) in (BF16_REL, 3 * e), (kind, shape, k, e)
                n += 1
    assert n == 3 * len(DW_SHAPES) + 2 * len(SE_SHAPES) + 4 * len(POOL_SHAPES)
    assert N.launch_count() >= 0 and N.lib().vt_dw3_gelu_pool_supported(14, 14, N.VT_BF16) == 1


def test_oversize_maps_and_bad_channel_counts_are_unsupported():
    before = N.launch_count()
    lib = N.lib()
    for hw in (14, 24, 32):
        assert lib.vt_dw3_gelu_pool_supported(hw, hw, N.VT_BF16) == 1 and lib.vt_dw3_gelu_pool_supported(hw, hw, N.VT_F32) == 1
    assert lib.vt_dw3_gelu_pool_supported(96, 96, N.VT_BF16) == 0
    x = torch.zeros(1, 96, 96, 8, device="cuda", dtype=torch.bfloat16)
    w, b = torch.zeros(8, 9, device="cuda"), torch.zeros(8, device="cuda")
    p = torch.zeros(1, 8, device="cuda", dtype=torch.bfloat16)
    s = torch.zeros(80, device="cuda")
    assert lib.vt_dw3_gelu_pool_fwd(vp(x), 8, vp(w), vp(b), vp(x), 8, vp(p), 8, 1, 400, 400, 8, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert "LDS" in N.last_error() and "163840" in N.last_error()
    assert lib.vt_dw3_gelu_pool_bwd(vp(x), 8, vp(x), 8, vp(p), 8, vp(w), vp(b), vp(x), 8, None, 0, vp(w), vp(b), vp(s), 320, 1, 96, 96, 8,
                                    N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert "LDS" in N.last_error()
    # C = 12 is no whole 16-byte chunk of bf16
    y = torch.zeros(1, 4, 4, 16, device="cuda", dtype=torch.bfloat16)
    assert lib.vt_dw3_gelu_pool_fwd(vp(y), 16, vp(w), vp(b), vp(y), 16, vp(p), 16, 1, 4, 4, 12, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_se_gate_fwd(vp(y), 16, vp(p), 16, vp(y), 16, 1, 16, 12, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_channel_stats(vp(y), 16, 16, 12, N.VT_BF16, vp(N.stats_buffer(16)), stream()) == N.VT_ERR_UNSUPPORTED
    lse = torch.zeros(1, device="cuda")
    assert lib.vt_pool_attn_fwd(vp(y), 16, vp(y), 16, vp(y), 16, vp(y), 16, vp(lse), 1.0, 1, 4, 12, N.VT_BF16,
                                stream()) == N.VT_ERR_UNSUPPORTED
    assert "head_dim" in N.last_error()
    torch.cuda.synchronize()
    assert N.launch_count() == before  # nothing was launched
