"""vt_dwtile.hip against float64 torch and against vt_dwconv_fwd: the tiled depthwise convolution of the MobileNet units
(forward with batch statistics; one backward launch for the data gradient and the filter-gradient shares; the share reducer),
and the activation codes 5 (ReLU6) / 6 (Hardswish) of the BatchNorm passes.

Every convolution case is launched twice and must be bit-identical (no float atomics), and runs once dense and once as a
channel slice of a NaN-filled buffer 16 channels wider whose surroundings must stay NaN.  z must be torch.equal to
vt_dwconv_fwd's output on the same operands (same taps, same order, f32 FMA from 0).  Bounds: relative L2 within
gpu_util.tol(dtype) -- 2e-5 for the exact-f32 instantiation, which pins the index maps, 6e-3 for bf16 -- for z, the
statistics, dx and dw, against float64 torch on storage-rounded operands.  The shares scratch is pre-filled with NaN (the
launch must write all the reducer reads) and dw starts non-zero (the reducer adds).  The reference of a (shape, dtype) is
computed once and shared."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import filler
from vision_toolbox import _native as N

from gpu_util import DNAME, DTYPES, TD, nhwc, rel_err, rounded, stream, to_nchw, tol, vp

pytestmark = pytest.mark.gpu

# (B, H, W, C, k, stride): two maps smaller than the filter; odd, non-square, 3 bf16 chunks under stride 2; an even extent,
# where the far padding is partly unread; 5x5 stride 1; two with several row bands; 17 bf16 chunks (several slabs, a partial
# last one) with 5 images of shares
SHAPES = [(1, 1, 1, 8, 3, 1), (1, 2, 3, 8, 5, 2), (2, 7, 7, 16, 3, 1), (3, 13, 11, 24, 3, 2), (2, 14, 14, 72, 5, 2),
          (2, 9, 9, 40, 5, 1), (1, 40, 24, 16, 3, 2), (2, 33, 17, 8, 5, 1), (5, 6, 6, 136, 3, 1)]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
DT_IDS = [DNAME[d] for d in DTYPES]
_CASES: dict = {}


def _out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _case(shape, dtype):
    key = (shape, dtype)
    if key not in _CASES:
        B, H, W, Cc, k, s = shape
        tag = "dwt" + "x".join(map(str, shape))
        x = rounded(filler.tensor(tag + "x", (B, Cc, H, W)), dtype)
        w = rounded(filler.tensor(tag + "w", (Cc, 1, k, k)) * (2.0 / (k * k)) ** 0.5, dtype)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        z = F.conv2d(xd, wd, None, s, (k - 1) // 2, 1, Cc)
        dz = rounded(filler.tensor(tag + "dz", tuple(z.shape)), dtype)
        z.backward(dz.double())
        zs = rounded(z.detach().float(), dtype).double()  # the statistics are those of the STORED z
        _CASES[key] = dict(x=x, w=w.reshape(Cc, k * k).contiguous(), dz=dz, z=z.detach(), dx=xd.grad,
                           dw=wd.grad.reshape(Cc, k * k), dw0=filler.tensor(tag + "dw0", (Cc, k * k)) * 0.25,
                           stats=torch.stack([zs.sum((0, 2, 3)), (zs * zs).sum((0, 2, 3))]))
    return _CASES[key]


def _tile(H, W, Cc, k, s, dtype):
    r, c = C.c_int32(), C.c_int32()
    N.check(N.lib().vt_dwt_tile(H, W, Cc, k, s, dtype, C.byref(r), C.byref(c)))
    return r.value, c.value


def _dev(t, dtype, sliced):
    """NCHW cpu tensor -> device NHWC (dense, or channels [8, 8 + C) of a NaN-filled buffer 16 channels wider)"""
    return nhwc(t, dtype, t.shape[1] + 16, 8) if sliced else nhwc(t, dtype)


def _out(B, H, W, Cc, dtype, sliced):
    wide = torch.full((B, H, W, Cc + 16 if sliced else Cc), float("nan"), device="cuda", dtype=TD[dtype])
    return wide, (wide[..., 8:8 + Cc] if sliced else wide)


def _surroundings_nan(wide, Cc, sliced):
    return (not sliced) or bool(torch.isnan(wide[..., :8]).all() and torch.isnan(wide[..., 8 + Cc:]).all())


def test_the_shapes_cross_band_and_slab_boundaries():
    """through vt_dwt_tile: at least two shapes span >= 3 row bands, one spans >= 2 channel slabs, one has a last band
    shorter than the rest (per dtype: the tile depends on the bytes per channel)"""
    for dtype in DTYPES:
        bands, slabs, short = 0, 0, 0
        for (B, H, W, Cc, k, s) in SHAPES:
            R, SCc = _tile(H, W, Cc, k, s, dtype)
            Ho = _out_hw(H, W, s)[0]
            assert 1 <= R <= Ho and SCc >= 1
            nb = -(-Ho // R)
            bands += nb >= 3
            slabs += -(-Cc // SCc) >= 2
            short += nb >= 2 and Ho % R != 0
        assert bands >= 2 and slabs >= 1 and short >= 1, (DNAME[dtype], bands, slabs, short)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_depthwise_forward_statistics_dgrad_wgrad(shape, dtype, sliced):
    before = N.launch_count()
    B, H, W, Cc, k, s = shape
    Ho, Wo = _out_hw(H, W, s)
    c, lib, bound = _case(shape, dtype), N.lib(), tol(dtype)
    x, dz, w = _dev(c["x"], dtype, sliced), _dev(c["dz"], dtype, sliced), c["w"].cuda()
    assert tuple(c["z"].shape) == (B, Cc, Ho, Wo)
    geo = (B, H, W, Cc, k, s, dtype)
    ld = Cc + 16 if sliced else Cc  # (the pixel stride; torch reports any stride for an extent of 1)
    nbytes = lib.vt_dwt_shares_bytes(*geo)
    assert nbytes > 0 and nbytes % (k * k * Cc * 4) == 0

    runs = []
    for _ in range(2):
        zw, z = _out(B, Ho, Wo, Cc, dtype, sliced)
        st = N.stats_buffer(Cc)
        N.check(lib.vt_dwt_fwd(vp(x), ld, vp(w), vp(z), ld, vp(st), *geo, stream()))
        dxw, dx = _out(B, H, W, Cc, dtype, sliced)
        shares = torch.full((nbytes // 4,), float("nan"), device="cuda")
        N.check(lib.vt_dwt_bwd(vp(dz), ld, vp(x), ld, vp(w), vp(dx), ld, None, 0, vp(shares), nbytes, *geo, stream()))
        dw = c["dw0"].cuda()
        N.check(lib.vt_dwt_wgrad_reduce(vp(shares), nbytes, vp(dw), *geo, stream()))
        torch.cuda.synchronize()
        assert _surroundings_nan(zw, Cc, sliced) and _surroundings_nan(dxw, Cc, sliced), "wrote outside its channel slice"
        assert not torch.isnan(shares).any(), "a share the reducer reads was not written"
        runs.append((z.clone(), N.stats_decode(st).cpu(), dx.clone(), dw.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    z, st, dx, dw = runs[0]

    # the same taps in the same order: bit-identical to the untiled kernel, with and without the statistics
    z_old = torch.empty(B, Ho, Wo, Cc, device="cuda", dtype=TD[dtype])
    N.check(lib.vt_dwconv_fwd(vp(x), ld, vp(w), vp(z_old), Cc, None, B, H, W, Cc, k, s, (k - 1) // 2, 1, dtype, stream()))
    z_nostat = torch.empty_like(z_old)
    N.check(lib.vt_dwt_fwd(vp(x), ld, vp(w), vp(z_nostat), Cc, None, *geo, stream()))
    torch.cuda.synchronize()
    assert torch.equal(z.contiguous(), z_old) and torch.equal(z_nostat, z_old), "z differs from vt_dwconv_fwd's"

    errs = dict(z=rel_err(to_nchw(z), c["z"]), sum=rel_err(st[0], c["stats"][0]), sumsq=rel_err(st[1], c["stats"][1]),
                dx=rel_err(to_nchw(dx), c["dx"]), dw=rel_err(dw.cpu(), c["dw"] + c["dw0"].double()))
    print(shape, DNAME[dtype], "slice" if sliced else "dense", {k_: f"{v:.2e}" for k_, v in errs.items()})
    for k_, v in errs.items():
        assert v < bound, (k_, v, bound)
    assert N.launch_count() >= before + 8


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[7]], ids=_ids([SHAPES[3], SHAPES[7]]))
def test_backward_adds_a_residual_that_aliases_dx(shape, dtype):
    B, H, W, Cc, k, s = shape
    c, lib = _case(shape, dtype), N.lib()
    r = rounded(filler.tensor("dwt.res" + "x".join(map(str, shape)), (B, Cc, H, W)), dtype)
    dz, x, w, dx = nhwc(c["dz"], dtype), nhwc(c["x"], dtype), c["w"].cuda(), nhwc(r, dtype)
    nbytes = lib.vt_dwt_shares_bytes(B, H, W, Cc, k, s, dtype)
    shares = torch.full((nbytes // 4,), float("nan"), device="cuda")
    N.check(lib.vt_dwt_bwd(vp(dz), Cc, vp(x), Cc, vp(w), vp(dx), Cc, vp(dx), Cc, vp(shares), nbytes, B, H, W, Cc, k, s, dtype, stream()))
    torch.cuda.synchronize()
    # (the sum is rounded to the storage type before the residual is added, as vt_dwconv_dgrad does: one more rounding)
    assert rel_err(to_nchw(dx), c["dx"] + r.double()) < tol(dtype)


def test_geometries_outside_the_range_are_refused_with_the_argument_named():
    lib = N.lib()
    t = torch.zeros(1, 8, 8, 16, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(16, 49, device="cuda")
    sh = torch.zeros(1 << 16, device="cuda")
    for (Cc, k, s, word) in ((16, 7, 1, "k=7"), (16, 3, 3, "s=3"), (12, 3, 1, "C=12")):
        calls = (lambda: lib.vt_dwt_fwd(vp(t), 16, vp(w), vp(t), 16, None, 1, 8, 8, Cc, k, s, N.VT_BF16, stream()),
                 lambda: lib.vt_dwt_bwd(vp(t), 16, vp(t), 16, vp(w), vp(t), 16, None, 0, vp(sh), 4 << 16, 1, 8, 8, Cc, k, s, N.VT_BF16,
                                        stream()),
                 lambda: lib.vt_dwt_wgrad_reduce(vp(sh), 4 << 16, vp(w), 1, 8, 8, Cc, k, s, N.VT_BF16, stream()),
                 lambda: lib.vt_dwt_tile(8, 8, Cc, k, s, N.VT_BF16, None, None))
        for call in calls:
            rc = call()
            assert rc == N.VT_ERR_UNSUPPORTED
            with pytest.raises(RuntimeError, match=word):
                N.check(rc)
        assert lib.vt_dwt_shares_bytes(1, 8, 8, Cc, k, s, N.VT_BF16) < 0
    need = lib.vt_dwt_shares_bytes(1, 8, 8, 16, 3, 1, N.VT_BF16)
    for rc in (lib.vt_dwt_bwd(vp(t), 16, vp(t), 16, vp(w), vp(t), 16, None, 0, vp(sh), need - 4, 1, 8, 8, 16, 3, 1, N.VT_BF16, stream()),
               lib.vt_dwt_wgrad_reduce(vp(sh), need - 4, vp(w), 1, 8, 8, 16, 3, 1, N.VT_BF16, stream())):
        assert rc == N.VT_ERR_INVALID
        with pytest.raises(RuntimeError, match="shares_bytes"):
            N.check(rc)


# ---- activation codes 5 (ReLU6) and 6 (Hardswish) of the BatchNorm passes --------------------------------------------------
ACTS = {5: F.relu6, 6: F.hardswish}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("code", [5, 6], ids=["relu6", "hardswish"])
def test_relu6_and_hardswish_in_the_batchnorm_passes(code, dtype):
    """vt_bn_act_apply, vt_bn_act_bwd_reduce and vt_bn_act_bwd_apply with u = z*scale + shift against F.relu6 / F.hardswish
    and their autograd in float64.  scale ~ 4 and shift ~ 1.5 put u ~ N(1.5, 16): every linear piece of both functions
    (u < -3, -3..3, 3..6, > 6) holds at least 5 % of the reference input, so no branch goes unchecked."""
    M, Cc = 37 * 29, 40
    lib, td, bound = N.lib(), TD[dtype], tol(dtype)
    tag = f"dwt.act{code}"
    z = rounded(filler.tensor(tag + "z", (M, Cc)), dtype)
    dy = rounded(filler.tensor(tag + "dy", (M, Cc)), dtype)
    scale = 4.0 + 0.2 * filler.tensor(tag + "sc", (Cc,))
    shift = 1.5 + 0.2 * filler.tensor(tag + "sh", (Cc,))
    mean, invstd = 0.1 * filler.tensor(tag + "m", (Cc,)), 1.0 + 0.1 * filler.tensor(tag + "i", (Cc,)).abs()
    coef = filler.tensor(tag + "coef", (3, Cc)) * 0.5

    u = (z.double() * scale.double() + shift.double()).requires_grad_(True)
    regions = [(u < -3), (u >= -3) & (u <= 3), (u > 3) & (u < 6), (u >= 6)]
    for r in regions:
        assert r.double().mean().item() >= 0.05, [q.double().mean().item() for q in regions]
    y_ref = ACTS[code](u)
    y_ref.backward(dy.double())
    g = u.grad  # dy * act'(u)
    xhat = (z.double() - mean.double()) * invstd.double()
    sums_ref = torch.stack([g.sum(0), (g * xhat).sum(0)])
    dz_ref = coef[0].double() * g - coef[1].double() * z.double() + coef[2].double()

    zd, dyd = z.to("cuda", td), dy.to("cuda", td)
    sc, sf, mn, iv, cf = scale.cuda(), shift.cuda(), mean.cuda(), invstd.cuda(), coef.cuda().contiguous()
    y = torch.full((M, Cc), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_bn_act_apply(vp(zd), Cc, vp(sc), vp(sf), None, 0, vp(y), Cc, M, Cc, code, dtype, stream()))
    sums = N.stats_buffer(Cc)
    N.check(lib.vt_bn_act_bwd_reduce(vp(dyd), Cc, vp(zd), Cc, vp(sc), vp(sf), vp(mn), vp(iv), M, Cc, code, dtype, vp(sums), stream()))
    dz = torch.full((M, Cc), float("nan"), device="cuda", dtype=td)
    N.check(lib.vt_bn_act_bwd_apply(vp(dyd), Cc, vp(zd), Cc, vp(sc), vp(sf), vp(cf), vp(dz), Cc, M, Cc, code, dtype, stream()))
    torch.cuda.synchronize()
    errs = dict(y=rel_err(y.float().cpu(), y_ref.detach()), sum_g=rel_err(N.stats_decode(sums).cpu()[0], sums_ref[0]),
                sum_gx=rel_err(N.stats_decode(sums).cpu()[1], sums_ref[1]), dz=rel_err(dz.float().cpu(), dz_ref))
    print(code, DNAME[dtype], {k_: f"{v:.2e}" for k_, v in errs.items()})
    for k_, v in errs.items():
        assert v < bound, (k_, v, bound)
