"""vt_prefix_tokens_fwd / vt_prefix_tokens_bwd / vt_prefix_pool_fwd / vt_prefix_pool_bwd (vt_prefix_tokens.hip) through the
C-ABI against torch in float64 on the same (storage-rounded) operands: cat([prefix rows, embed + pe], 1) and
LayerNorm(x[:, :P]).mean(1) with their autograd backward (reference backbones/deit.py:37-41), general in P.

Shapes: one chunk per row, rows that are no power of two of chunks (200), several chunks per lane (1280), a channel-slice
operand (row stride C + 24: the NaN-filled surroundings must stay NaN), P = 1, 2 and 4, more images than a workgroup's four
waves (5), and a DeiT-Ti map (198 x 192: several row slabs in the pool backward, several workgroups in the token kernels).

Bounds: gpu_util.tol (2e-5 f32, 6e-3 bf16) for every activation output, twice that where accumulate = 1 adds a second
rounding; the copied rows of d(embed) and the zero rows of d(x) are exact.  The channel sums go through the fixed-point buffer
and are compared at 1e-6 of their scale sum |terms|, the f32 parameter gradients at rtol 1e-6 (atol 1e-6 of their largest
value + 1), as in tests/test_layernorm_gpu.py: f32 rounding of a handful of terms."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, rel_err, stream, tol, vp

pytestmark = pytest.mark.gpu

EPS = 1e-6
DTYPES = [N.VT_F32, N.VT_BF16]
OFF, EXTRA = 8, 24  # a padded operand starts at element 8 of rows of C + 24
# (B, T or L, P, C or None = one chunk, padded)
TOKEN_CASES = [(1, 1, 1, None, False), (3, 16, 2, 64, True), (2, 5, 4, 200, False), (5, 7, 2, 1280, False), (2, 196, 2, 192, False)]
POOL_CASES = [(1, 2, 1, None, False), (3, 18, 2, 64, True), (2, 9, 4, 200, False), (5, 9, 2, 1280, False), (2, 198, 2, 192, False)]


def _ids(c):
    return "x".join("chunk" if v is None else str(int(v)) for v in c)


def _chunk(dtype):
    return 8 if dtype == N.VT_BF16 else 4


def _rows(B, R, C, td, padded, fill=None):
    """[B][R][C] operand, dense or inside a NaN-filled [B][R][C + EXTRA] buffer; returns (buffer, operand)"""
    wide = torch.full((B, R, C + (EXTRA if padded else 0)), float("nan"), device="cuda", dtype=td)
    view = wide[..., OFF:OFF + C] if padded else wide
    if fill is not None:
        view.copy_(fill)
    return wide, view


def _nan_outside(wide, C):
    return bool(torch.isnan(wide[..., :OFF].float()).all() and torch.isnan(wide[..., OFF + C:].float()).all())


def _ptrs(tensors):
    arr = (ctypes.c_void_p * 4)()
    for k, t_ in enumerate(tensors):
        arr[k] = t_.data_ptr() if t_ is not None else None
    return arr


def _sums(C):
    return torch.zeros(N.VT_STAT_REPLICAS, 2, C, 2, dtype=torch.int64, device="cuda")


def _close_f32(got, start, want):
    """an f32 gradient that started at `start` against the float64 sum `want`"""
    return torch.allclose(got.double() - start.double(), want, rtol=1e-6, atol=1e-6 * float(want.abs().max() + 1))


# ---- tokens ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", TOKEN_CASES, ids=_ids)
def test_prefix_tokens_forward_matches_torch_float64(case, dtype):
    B, T, P, C, padded = case
    C = C or _chunk(dtype)
    torch.manual_seed(B + T + P + C)
    td, lib = TD[dtype], N.lib()
    _, embed = _rows(B, T, C, td, padded, torch.randn(B, T, C, device="cuda"))
    pe = torch.randn(T, C, device="cuda")
    prefix = [torch.randn(C, device="cuda") for _ in range(P)]
    outs = []
    for _ in range(2):
        owide, out = _rows(B, P + T, C, td, padded)
        N.check(lib.vt_prefix_tokens_fwd(vp(embed), embed.stride(1), vp(pe), _ptrs(prefix), P, vp(out), out.stride(1), B, T, C,
                                         dtype, stream()))
        torch.cuda.synchronize()
        outs.append(owide.clone())
    want = torch.cat([torch.stack(prefix).double().expand(B, P, C), embed.double() + pe.double()], 1)
    e = rel_err(out, want)
    print(f"tokens fwd {case} {td}: out {e:.2e} (bound {tol(dtype):.0e})")
    assert e < tol(dtype)
    # a prefix row is the master rounded once; the batch sees one value
    assert torch.equal(out[:, :P], torch.stack(prefix).to(td).expand(B, P, C))
    if padded:
        assert _nan_outside(owide, C)
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), "two runs differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", TOKEN_CASES, ids=_ids)
def test_prefix_tokens_backward_matches_torch_float64(case, dtype):
    B, T, P, C, padded = case
    C = C or _chunk(dtype)
    torch.manual_seed(B + T + P + C + 1)
    td, lib = TD[dtype], N.lib()
    _, dout = _rows(B, P + T, C, td, padded, torch.randn(B, P + T, C, device="cuda"))
    dpe0 = torch.randn(T, C, device="cuda")  # non-zero starts: the kernel adds
    dpre0 = [torch.randn(C, device="cuda") for _ in range(P)]
    want_pe = dout[:, P:].double().sum(0)
    want_pre = dout[:, :P].double().sum(0)
    variants = ["all", "all", "no dembed", "no dpe", "no dprefix"] + (["no dprefix[0]"] if P > 1 else [])
    first = None
    for what in variants:
        ewide, dembed = _rows(B, T, C, td, padded)
        dpe = dpe0.clone()
        dpre = [v.clone() for v in dpre0]
        use_e, use_pe = what != "no dembed", what != "no dpe"
        live = [what != "no dprefix" and not (what == "no dprefix[0]" and p == 0) for p in range(P)]
        N.check(lib.vt_prefix_tokens_bwd(vp(dout), dout.stride(1), vp(dembed) if use_e else None, dembed.stride(1) if use_e else 0,
                                         vp(dpe) if use_pe else None,
                                         _ptrs([v if ok else None for v, ok in zip(dpre, live)]) if what != "no dprefix" else None,
                                         P, B, T, C, dtype, stream()))
        torch.cuda.synchronize()
        if use_e:
            assert torch.equal(dembed, dout[:, P:]), what  # (a copy: exact)
            if padded:
                assert _nan_outside(ewide, C)
        else:
            assert torch.isnan(ewide.float()).all(), what
        if use_pe:
            assert _close_f32(dpe, dpe0, want_pe), what
        else:
            assert torch.equal(dpe, dpe0), what
        for p in range(P):
            if live[p]:
                assert _close_f32(dpre[p], dpre0[p], want_pre[p]), (what, p)
            else:
                assert torch.equal(dpre[p], dpre0[p]), (what, p)
        if what == "all":
            state = [dembed.clone(), dpe.clone()] + [v.clone() for v in dpre]
            if first is None:
                first = state
            else:
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, state)), "two runs differ"
    e = ((dpe0.double() + want_pe - first[1].double()).abs().max() / want_pe.abs().max().clamp_min(1e-30)).item()
    print(f"tokens bwd {case} {td}: d pe worst |error| {e:.2e} of the largest sum")


# ---- pool --------------------------------------------------------------------------------------------------------------------
def _pool_operands(case, dtype, seed):
    B, L, P, C, padded = case
    C = C or _chunk(dtype)
    torch.manual_seed(B + L + P + C + seed)
    td = TD[dtype]
    _, x = _rows(B, L, C, td, padded, torch.randn(B, L, C, device="cuda") * 1.5 + 0.3)
    dy = torch.randn(B, C, device="cuda").to(td)
    gamma = (1.0 + 0.5 * torch.randn(C, device="cuda")).contiguous()
    beta = (0.2 * torch.randn(C, device="cuda")).contiguous()
    return B, L, P, C, padded, td, x, dy, gamma, beta


def _pool_reference(x, dy, gamma, beta, P, C):
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(x64[:, :P], (C,), g64, b64, EPS).mean(1)
    y.backward(dy.double())
    return y.detach(), x64.grad, g64.grad, b64.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids)
def test_prefix_pool_forward_matches_torch_float64(case, dtype):
    B, L, P, C, padded, td, x, dy, gamma, beta = _pool_operands(case, dtype, 0)
    lib = N.lib()
    want = _pool_reference(x, dy, gamma, beta, P, C)[0]
    outs = []
    for _ in range(2):
        ywide = torch.full((B, C + (EXTRA if padded else 0)), float("nan"), device="cuda", dtype=td)
        y = ywide[:, OFF:OFF + C] if padded else ywide
        N.check(lib.vt_prefix_pool_fwd(vp(x), x.stride(1), vp(gamma), vp(beta), vp(y), y.stride(0), B, L, P, C, EPS, dtype, stream()))
        torch.cuda.synchronize()
        outs.append(ywide.clone())
    e = rel_err(y, want)
    print(f"pool fwd {case} {td}: y {e:.2e} (bound {tol(dtype):.0e})")
    assert e < tol(dtype)
    if padded:
        assert bool(torch.isnan(ywide[:, :OFF].float()).all() and torch.isnan(ywide[:, OFF + C:].float()).all())
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), "two runs differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids)
def test_prefix_pool_backward_matches_torch_float64(case, dtype):
    B, L, P, C, padded, td, x, dy, gamma, beta = _pool_operands(case, dtype, 1)
    lib, t_ = N.lib(), tol(dtype)
    _, want_dx, want_dg, want_db = _pool_reference(x, dy, gamma, beta, P, C)

    def run(accumulate, start):
        dwide, dx = _rows(B, L, C, td, padded, start)
        sums = _sums(C)
        N.check(lib.vt_prefix_pool_bwd(vp(dy), dy.stride(0), vp(x), x.stride(1), vp(gamma), vp(dx), dx.stride(1), accumulate,
                                       vp(sums), B, L, P, C, EPS, dtype, stream()))
        torch.cuda.synchronize()
        return dwide, dx, sums

    # ---- accumulate = 0 over a NaN-filled gradient: the prefix rows, and exact zeros everywhere else
    dwide, dx, sums = run(0, None)
    e = rel_err(dx[:, :P], want_dx[:, :P])
    print(f"pool bwd {case} {td}: dx {e:.2e} (bound {t_:.0e})")
    assert e < t_
    assert bool((dx[:, P:] == 0).all()), "rows >= P are written zero"
    if padded:
        assert _nan_outside(dwide, C)
    # ---- the channel sums, at 1e-6 of their scale
    got = N.stats_decode(sums)  # [2][C]
    x64 = x.double()[:, :P]
    xhat = (x64 - x64.mean(-1, keepdim=True)) / (x64.var(-1, unbiased=False, keepdim=True) + EPS).sqrt()
    terms = [(dy.double() / P)[:, None, :] * xhat, dy.double()[:, None, :]]
    for k in range(2):
        want, scale = terms[k].sum((0, 1)), terms[k].abs().sum((0, 1)).clamp_min(1e-30)
        es = ((got[k] - want).abs() / scale).max().item()
        print(f"pool bwd {case} {td}: sums[{k}] {es:.2e} of scale (bound 1e-06)")
        assert es < 1e-6
    assert rel_err(got[0], want_dg) < 1e-5 and rel_err(got[1], want_db) < 1e-5
    # ---- the fold into f32 gradients (accumulating)
    d = [torch.full((C,), 0.5, device="cuda") for _ in range(2)]
    N.check(lib.vt_channel_sums_to_f32(vp(sums), 2, C, vp(d[0]), vp(d[1]), None, stream()))
    torch.cuda.synchronize()
    for k in range(2):
        assert _close_f32(d[k], torch.full_like(d[k], 0.5), got[k]), k
    # ---- two runs are bit-identical, the sums included
    dwide2, _, sums2 = run(0, None)
    assert torch.equal(dwide.view(torch.uint8), dwide2.view(torch.uint8)) and torch.equal(sums, sums2), "two runs differ"
    # ---- accumulate = 1 over a random gradient: rows >= P bit-unchanged, rows < P added (a second rounding)
    start = torch.randn(B, L, C, device="cuda").to(td)
    awide, adx, asums = run(1, start)
    assert torch.equal(adx[:, P:].contiguous().view(torch.uint8), start[:, P:].contiguous().view(torch.uint8))
    e = rel_err(adx[:, :P], want_dx[:, :P] + start[:, :P].double())
    print(f"pool bwd {case} {td}: accumulated dx {e:.2e} (bound {2 * t_:.0e})")
    assert e < 2 * t_
    assert torch.equal(asums, sums)
    if padded:
        assert _nan_outside(awide, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_constant_prefix_row_gives_finite_output(dtype):
    B, L, P, C, td = 3, 5, 2, 96, TD[dtype]
    x = torch.randn(B, L, C, device="cuda").to(td)
    x[1, 0] = 0.75  # variance exactly 0
    x[2, 1] = -2.0
    gamma, beta = torch.full((C,), 1.5, device="cuda"), torch.linspace(-1, 1, C, device="cuda").contiguous()
    y = torch.full((B, C), float("nan"), device="cuda", dtype=td)
    N.check(N.lib().vt_prefix_pool_fwd(vp(x), C, vp(gamma), vp(beta), vp(y), C, B, L, P, C, EPS, dtype, stream()))
    dx = torch.full((B, L, C), float("nan"), device="cuda", dtype=td)
    dy = torch.randn(B, C, device="cuda").to(td)
    sums = _sums(C)
    N.check(N.lib().vt_prefix_pool_bwd(vp(dy), C, vp(x), C, vp(gamma), vp(dx), C, 0, vp(sums), B, L, P, C, EPS, dtype, stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all() and torch.isfinite(N.stats_decode(sums)).all()
    # xhat = 0 in the constant row: it contributes beta, so y = (LayerNorm(other row) + beta) / 2
    other = F.layer_norm(x[1, 1].double(), (C,), gamma.double(), beta.double(), EPS)
    assert rel_err(y[1], (other + beta.double()) / 2) < tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_one_prefix_row_agrees_with_token_select_and_layernorm(dtype):
    B, L, C, td, lib = 5, 9, 200, TD[dtype], N.lib()
    torch.manual_seed(7)
    x = (torch.randn(B, L, C, device="cuda") * 1.5 + 0.3).to(td)
    gamma = (1.0 + 0.5 * torch.randn(C, device="cuda")).contiguous()
    beta = (0.2 * torch.randn(C, device="cuda")).contiguous()
    y = torch.empty(B, C, device="cuda", dtype=td)
    N.check(lib.vt_prefix_pool_fwd(vp(x), C, vp(gamma), vp(beta), vp(y), C, B, L, 1, C, EPS, dtype, stream()))
    sel, y2 = torch.empty(B, C, device="cuda", dtype=td), torch.empty(B, C, device="cuda", dtype=td)
    N.check(lib.vt_token_select_fwd(vp(x), C, vp(sel), C, B, L, 0, C, dtype, stream()))
    N.check(lib.vt_layernorm_fwd(vp(sel), C, None, vp(gamma), vp(beta), vp(y2), C, B, C, EPS, dtype, stream()))
    torch.cuda.synchronize()
    e = rel_err(y, y2)
    print(f"P = 1 against token_select + layernorm {td}: {e:.2e} (bound {2 * tol(dtype):.0e})")
    assert e < 2 * tol(dtype)


def test_arguments_are_checked():
    lib, U, I = N.lib(), N.VT_ERR_UNSUPPORTED, N.VT_ERR_INVALID
    bf, st = N.VT_BF16, stream()
    x = torch.zeros(2, 6, 16, device="cuda", dtype=torch.bfloat16)  # embed [2][4][16] / out, dout, x [2][6][16]
    y = torch.zeros(2, 6, 16, device="cuda", dtype=torch.bfloat16)
    dy2 = torch.zeros(2, 16, device="cuda", dtype=torch.bfloat16)
    g = torch.ones(64, device="cuda")  # pe / dpe [4][16]; gamma, beta
    s = _sums(16)
    pp = _ptrs([torch.ones(16, device="cuda"), torch.ones(16, device="cuda")])

    def fwd(C=16, lde=16, ldo=16, P=2, embed=x, pe=g, prefix=pp, out=y, dtype=bf):
        return lib.vt_prefix_tokens_fwd(vp(embed), lde, vp(pe), prefix, P, vp(out), ldo, 2, 4, C, dtype, st)

    assert fwd(C=12) == U and fwd(C=6, dtype=N.VT_F32) == U  # C is no whole chunk
    assert fwd(lde=8) == I and fwd(ldo=8) == I and fwd(ldo=20) == I  # ld < C, ld no multiple of a chunk
    assert fwd(P=0) == I and fwd(P=5) == I
    assert fwd(embed=None) == I and fwd(pe=None) == I and fwd(out=None) == I and fwd(prefix=None) == I
    assert fwd(prefix=_ptrs([g, None])) == I and "vt_prefix_tokens_fwd" in N.last_error()

    def bwd(C=16, lddo=16, lde=16, P=2, dout=x, dembed=y, dpe=g, dprefix=pp, dtype=bf):
        return lib.vt_prefix_tokens_bwd(vp(dout), lddo, vp(dembed), lde, vp(dpe), dprefix, P, 2, 4, C, dtype, st)

    assert bwd(C=12) == U and bwd(C=6, dtype=N.VT_F32) == U
    assert bwd(lddo=8) == I and bwd(lde=8) == I
    assert bwd(P=0) == I and bwd(P=5) == I
    assert bwd(dout=None) == I
    assert bwd(dembed=None, dpe=None, dprefix=None) == I and bwd(dembed=None, dpe=None, dprefix=_ptrs([None, None])) == I
    assert "vt_prefix_tokens_bwd" in N.last_error()

    def pool(C=16, ldx=16, ldy=16, L=6, P=2, x_=x, gamma=g, beta=g, y_=y, dtype=bf):
        return lib.vt_prefix_pool_fwd(vp(x_), ldx, vp(gamma), vp(beta), vp(y_), ldy, 2, L, P, C, EPS, dtype, st)

    assert pool(C=12) == U and pool(C=6, dtype=N.VT_F32) == U and pool(C=4096) == U
    assert pool(ldx=8) == I and pool(ldy=8) == I
    assert pool(P=0) == I and pool(P=5) == I and pool(L=1, P=2) == I  # P > L
    assert pool(x_=None) == I and pool(gamma=None) == I and pool(beta=None) == I and pool(y_=None) == I
    assert "vt_prefix_pool_fwd" in N.last_error()

    def pool_bwd(C=16, lddy=16, ldx=16, lddx=16, L=6, P=2, dy=dy2, x_=x, gamma=g, dx=y, sums=s, dtype=bf):
        return lib.vt_prefix_pool_bwd(vp(dy), lddy, vp(x_), ldx, vp(gamma), vp(dx), lddx, 0, vp(sums), 2, L, P, C, EPS, dtype, st)

    assert pool_bwd(C=12) == U and pool_bwd(C=6, dtype=N.VT_F32) == U and pool_bwd(C=4096) == U
    assert pool_bwd(lddy=8) == I and pool_bwd(ldx=8) == I and pool_bwd(lddx=8) == I
    assert pool_bwd(P=0) == I and pool_bwd(P=5) == I and pool_bwd(L=1, P=2) == I
    assert pool_bwd(dy=None) == I and pool_bwd(x_=None) == I and pool_bwd(gamma=None) == I and pool_bwd(dx=None) == I
    assert pool_bwd(sums=None) == I and "vt_prefix_pool_bwd" in N.last_error()
    # and the well-formed calls run
    x.normal_()
    assert fwd() == N.VT_OK and bwd() == N.VT_OK and pool() == N.VT_OK and pool_bwd() == N.VT_OK
    torch.cuda.synchronize()
