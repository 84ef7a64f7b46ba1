"""vt_resnet.hip against float64 torch: the BatchNorm passes whose residual joins BEFORE the ReLU (the last unit of a
torchvision BasicBlock / Bottleneck, y = relu(bn(z) + r)) and the 7x7 stride-2 stem as a 4x4 convolution over the
space-to-depth image.

Inputs are built so that about half of z*scale + shift + r is negative, and two channels have a sign that the residual
ALONE decides (channel 0: bn(z) > 0 everywhere and r far below it; channel 1 the other way round): a kernel that masks
on z*scale + shift, as the Darknet passes do, fails on them.  Every variant (dense rows, a channel slice of a wider NaN-filled
buffer, r aliasing y, dr written / accumulated, ready coefficients / finalize inside the launch, train 1 / 0) is launched
twice and must be bit-identical; the reference of a (shape, dtype) is computed once and shared by its variants."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import filler
from vision_toolbox import _native as N

from gpu_util import DNAME, DTYPES, TD, krsc, nhwc, rel_err, rounded, short_grids, stream, to_nchw, tol, vp

pytestmark = pytest.mark.gpu

# (98, 64): one channel group, rows no multiple of the row lanes; (392, 256): two channel groups; (50, 2048): sixteen
# groups, the reduction's channel split, more chunks per row than threads (f32); (1031, 72): a ragged row count and a
# channel count with no divisor in [32, 128] but itself
SHAPES = [(98, 64), (392, 256), (50, 2048), (1031, 72)]
# on a grid of two row blocks per channel group: 7 (bf16) / 14 (f32) trips of the row loop in one group of 72 channels, 25 in
# two finalize groups of 128 and 13 in the reduction's four groups of 64 -- never a multiple of the rows in flight, the last
# trip partial, 194 live rows in the last block, idle row lanes at 72 channels
SHORT_GRIDS = [(390, 72), (390, 256)]
SHAPES += SHORT_GRIDS
EPS, MOM = 1e-5, 0.1


@pytest.fixture(autouse=True)
def _grid_of_the_case(request):
    """the SHORT_GRIDS cases run with two row blocks per channel group (gpu_util.short_grids)"""
    params = getattr(request.node, "callspec", None)
    with short_grids(params is not None and params.params.get("shape") in SHORT_GRIDS):
        yield


def _inputs(M, Cc, dtype):
    key = f"resnet{M}x{Cc}"
    z = rounded(filler.tensor(key + "z", (M, Cc)) * 1.5 + 0.3, dtype)
    r = filler.tensor(key + "r", (M, Cc))
    gamma = filler.tensor(key + "g", (Cc,)) * 0.2 + 1.0
    beta = filler.tensor(key + "b", (Cc,)) * 0.2
    # the two channels whose sign the residual alone decides
    beta[0], beta[1] = 4.0, -4.0
    r[:, 0] = -20.0 - r[:, 0].abs()
    r[:, 1] = 20.0 + r[:, 1].abs()
    r = rounded(r, dtype)
    dy = rounded(filler.tensor(key + "dy", (M, Cc)), dtype)
    dr0 = rounded(filler.tensor(key + "dr0", (M, Cc)), dtype)  # what an accumulating launch finds in d(r)
    rm, rv = filler.tensor(key + "rm", (Cc,)) * 0.1, filler.tensor(key + "rv", (Cc,)).abs() + 0.5
    return z, r, gamma, beta, dy, dr0, rm, rv


def _reference(z, r, gamma, beta, dy, rm, rv, train):
    """float64: y, running statistics, (scale, shift, mean, invstd), and the gradients of z, r, gamma, beta"""
    zd, rd = z.double().requires_grad_(True), r.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_, rv_ = rm.double().clone(), rv.double().clone()
    x4 = zd.t().reshape(1, zd.shape[1], -1, 1)  # [1, C, M, 1]
    bn = F.batch_norm(x4, rm_, rv_, g, b, bool(train), MOM, EPS)
    y = torch.relu(bn.reshape(zd.shape[1], -1).t() + rd)
    y.backward(dy.double())
    if train:
        mean, var = z.double().mean(0), z.double().var(0, unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    coefs = torch.stack([scale, beta.double() - mean * scale, mean, invstd]).float()
    return y.detach(), rm_, rv_, coefs, zd.grad, rd.grad, g.grad, b.grad


def _stats(z):
    """a statistics buffer holding sum z, sum z^2 per channel, spread over the replicas"""
    st = N.stats_buffer(z.shape[1])
    zz = z.float().double()
    for rep, idx in enumerate(torch.chunk(torch.arange(z.shape[0], device="cuda"), N.VT_STAT_REPLICAS)):
        if idx.numel():
            N.stats_encode(st, 0, zz[idx].sum(0), rep)
            N.stats_encode(st, 1, (zz[idx] ** 2).sum(0), rep)
    return st


def _place(t, dtype, sliced):
    """device copy of the [M, C] cpu tensor t: dense, or a channel slice of a wider buffer filled with NaN"""
    v = t.to("cuda", TD[dtype])
    if not sliced:
        return v, v, t.shape[1]
    pad = 16
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device="cuda", dtype=TD[dtype])
    wide[:, pad : pad + t.shape[1]] = v
    return wide, wide[:, pad : pad + t.shape[1]], wide.shape[1]


def _surroundings_are_nan(wide, Cc):
    return bool(torch.isnan(wide[:, :16]).all() and torch.isnan(wide[:, 16 + Cc :]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_add_then_relu_forward(shape, dtype):
    M, Cc = shape
    z, r, gamma, beta, dy, dr0, rm, rv = _inputs(M, Cc, dtype)
    lib = N.lib()
    refs = {train: _reference(z, r, gamma, beta, dy, rm, rv, train) for train in (1, 0)}
    gd, bd = gamma.cuda(), beta.cuda()
    # the residual alone decides channels 0 and 1, and about half of everything is negative
    y_ref = refs[1][0]
    assert (y_ref[:, 0] == 0).all() and (y_ref[:, 1] > 0).all()
    assert 0.35 < (y_ref[:, 2:] == 0).double().mean().item() < 0.65
    for layout in ("dense", "slice", "alias"):
        for fin in (False, True):
            y_want, rm_ref, rv_ref, coefs, *_ = refs[1 if fin else 0]  # (ready coefficients: the eval-mode ones)
            runs = []
            for _ in range(2):
                zw, zv, ldz = _place(z, dtype, layout == "slice")
                rw, rvw, ldr = _place(r, dtype, layout == "slice")
                if layout == "alias":
                    yw, yv, ldy = rw, rvw, ldr  # r aliases y
                else:
                    yw, yv, ldy = _place(torch.full((M, Cc), float("nan")), dtype, layout == "slice")
                if fin:
                    st = _stats(zv)
                    rmd, rvd = rm.cuda(), rv.cuda()
                    nbt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
                    coef = torch.zeros(4, Cc, device="cuda")
                    N.check(lib.vt_bn_add_act_finalize_apply(vp(st), Cc, float(M), vp(gd), vp(bd), EPS, MOM, vp(rmd),
                                                             vp(rvd), vp(nbt), vp(coef[0]), vp(coef[1]), vp(coef[2]), vp(coef[3]),
                                                             vp(zv), ldz, vp(rvw), ldr, vp(yv), ldy, M, dtype, stream()))
                    extra = (coef, rmd, rvd, nbt)
                else:
                    cd = coefs.cuda()
                    N.check(lib.vt_bn_add_act_apply(vp(zv), ldz, vp(cd[0]), vp(cd[1]), vp(rvw), ldr, vp(yv), ldy, M, Cc, dtype, stream()))
                    extra = ()
                torch.cuda.synchronize()
                runs.append((yw, *extra))
            what = f"{layout} fin={fin}"
            for a, b in zip(*runs):  # two runs: bit-identical (NaN surroundings included)
                assert torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float())), what
                assert torch.equal(torch.isnan(a.float()), torch.isnan(b.float())), what
            y = yw[:, 16 : 16 + Cc] if layout == "slice" else yw
            err = rel_err(y.float().cpu(), y_want)
            print(f"{shape} {DNAME[dtype]} {what}: y rel err {err:.3e}")
            assert err < tol(dtype), what
            if layout == "slice":
                assert _surroundings_are_nan(yw, Cc) and _surroundings_are_nan(zw, Cc) and _surroundings_are_nan(rw, Cc), what
            if fin:
                coef, rmd, rvd, nbt = runs[0][1:]
                assert rel_err(coef.cpu(), coefs) < 2e-5, what
                np.testing.assert_allclose(rmd.cpu(), rm_ref, rtol=1e-5, atol=1e-6)
                np.testing.assert_allclose(rvd.cpu(), rv_ref, rtol=1e-4, atol=1e-6)
                assert nbt.item() == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_add_then_relu_backward(shape, dtype):
    M, Cc = shape
    z, r, gamma, beta, dy, dr0, rm, rv = _inputs(M, Cc, dtype)
    lib = N.lib()
    for train in (1, 0):
        y_ref, _, _, coefs, dz_ref, dr_ref, dg_ref, db_ref = _reference(z, r, gamma, beta, dy, rm, rv, train)
        cd = coefs.cuda()
        # the stored y the mask is read from: what the forward kernel wrote
        yd = torch.empty(M, Cc, device="cuda", dtype=TD[dtype])
        zd0, rd0 = z.to("cuda", TD[dtype]), r.to("cuda", TD[dtype])
        N.check(lib.vt_bn_add_act_apply(vp(zd0), Cc, vp(cd[0]), vp(cd[1]), vp(rd0), Cc, vp(yd), Cc, M, Cc, dtype, stream()))
        y_cpu = yd.float().cpu()
        for sliced in (False, True):
            # the reduction, twice: bit-identical sums; checked through d(gamma), d(beta) as the BatchNorm chain test does
            gw, gv, ldg = _place(dy, dtype, sliced)
            yw, yv, ldy = _place(y_cpu, dtype, sliced)
            zw, zv, ldz = _place(z, dtype, sliced)
            sums = [N.stats_buffer(Cc), N.stats_buffer(Cc)]
            for s_ in sums:
                N.check(lib.vt_bn_add_act_bwd_reduce(vp(gv), ldg, vp(yv), ldy, vp(zv), ldz, vp(cd[2]), vp(cd[3]), M, Cc, dtype, vp(s_),
                                                     stream()))
            torch.cuda.synchronize()
            assert torch.equal(N.stats_decode(sums[0]), N.stats_decode(sums[1]))
            got = N.stats_decode(sums[0]).cpu()
            g64 = dy.double() * (y_cpu.double() > 0)
            xhat = (z.double() - coefs[2].double()) * coefs[3].double()
            np.testing.assert_allclose(got[0], g64.sum(0), rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(got[1], (g64 * xhat).sum(0), rtol=1e-4, atol=1e-4)
            for accumulate in (0, 1):
                for fin in (False, True):
                    what = f"train={train} sliced={sliced} accumulate={accumulate} fin={fin}"
                    runs = []
                    for _ in range(2):
                        dzw, dzv, lddz = _place(torch.full((M, Cc), float("nan")), dtype, sliced)
                        drw, drv, lddr = _place(dr0 if accumulate else torch.full((M, Cc), float("nan")), dtype, sliced)
                        dg, db = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
                        bc = torch.zeros(3, Cc, device="cuda")
                        if fin:
                            N.check(lib.vt_bn_add_act_bwd_finalize_apply(
                                vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[2]), vp(cd[3]), train, vp(dg), vp(db), vp(bc), vp(gv), ldg,
                                vp(yv), ldy, vp(zv), ldz, vp(dzv), lddz, vp(drv), lddr, accumulate, M, dtype, stream()))
                        else:
                            N.check(lib.vt_bn_bwd_finalize(vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[2]), vp(cd[3]), train, vp(dg),
                                                           vp(db), vp(bc), stream()))
                            N.check(lib.vt_bn_add_act_bwd_apply(vp(gv), ldg, vp(yv), ldy, vp(zv), ldz, vp(bc), vp(dzv), lddz, vp(drv), lddr,
                                                                accumulate, M, Cc, dtype, stream()))
                        torch.cuda.synchronize()
                        runs.append((dzw, drw, dg, db, bc))
                    for a, b in zip(*runs):
                        assert torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float())), what
                        assert torch.equal(torch.isnan(a.float()), torch.isnan(b.float())), what
                    dzw, drw, dg, db, bc = runs[0]
                    dz_got = (dzw[:, 16 : 16 + Cc] if sliced else dzw).float().cpu()
                    dr_got = (drw[:, 16 : 16 + Cc] if sliced else drw).float().cpu()
                    dr_want = dr_ref + (dr0.double() if accumulate else 0.0)
                    e_dz, e_dr = rel_err(dz_got, dz_ref), rel_err(dr_got, dr_want)
                    print(f"{shape} {DNAME[dtype]} {what}: dz rel err {e_dz:.3e}, dr rel err {e_dr:.3e}")
                    assert e_dz < tol(dtype) and e_dr < tol(dtype), what
                    np.testing.assert_allclose((dg - 1).cpu(), dg_ref, rtol=1e-4, atol=1e-4)
                    np.testing.assert_allclose((db - 1).cpu(), db_ref, rtol=1e-4, atol=1e-4)
                    if sliced:
                        assert _surroundings_are_nan(dzw, Cc) and _surroundings_are_nan(drw, Cc), what
            if sliced:
                assert _surroundings_are_nan(gw, Cc) and _surroundings_are_nan(yw, Cc) and _surroundings_are_nan(zw, Cc)


def test_bad_arguments_return_an_error_code():
    lib = N.lib()
    M, Cc, dt = 10, 16, N.VT_BF16
    t = lambda: torch.zeros(M, Cc, device="cuda", dtype=torch.bfloat16)
    z, r, y, dy, dz, dr = t(), t(), t(), t(), t(), t()
    f = torch.zeros(4, Cc, device="cuda")
    sums = N.stats_buffer(Cc)
    s = stream()
    odd = C.c_void_p(z.data_ptr() + 2)  # misaligned
    bad = [
        lib.vt_bn_add_act_apply(None, Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, M, Cc, dt, s),
        lib.vt_bn_add_act_apply(vp(z), Cc, vp(f[0]), vp(f[1]), None, Cc, vp(y), Cc, M, Cc, dt, s),
        lib.vt_bn_add_act_apply(odd, Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, M, Cc, dt, s),
        lib.vt_bn_add_act_apply(vp(z), Cc, None, vp(f[1]), vp(r), Cc, vp(y), Cc, M, Cc, dt, s),
        lib.vt_bn_add_act_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, 0, Cc, dt, s),
        lib.vt_bn_add_act_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, M, 12, dt, s),  # C no multiple of 8
        lib.vt_bn_add_act_apply(vp(z), 8, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, M, Cc, dt, s),  # ld < C
        lib.vt_bn_add_act_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, M, Cc, 7, s),  # dtype
        lib.vt_bn_add_act_finalize_apply(None, Cc, float(M), None, None, EPS, MOM, None, None, None, vp(f[0]), vp(f[1]), vp(f[2]),
                                         vp(f[3]), vp(z), Cc, vp(r), Cc, vp(y), Cc, M, dt, s),
        lib.vt_bn_add_act_finalize_apply(vp(sums), Cc, 0.0, None, None, EPS, MOM, None, None, None, vp(f[0]), vp(f[1]), vp(f[2]),
                                         vp(f[3]), vp(z), Cc, vp(r), Cc, vp(y), Cc, M, dt, s),
        lib.vt_bn_add_act_finalize_apply(vp(sums), Cc, float(M), None, None, EPS, MOM, vp(f[0]), None, None, vp(f[0]), vp(f[1]),
                                         vp(f[2]), vp(f[3]), vp(z), Cc, vp(r), Cc, vp(y), Cc, M, dt, s),  # running_mean without var
        lib.vt_bn_add_act_bwd_reduce(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f[2]), vp(f[3]), M, Cc, dt, None, s),
        lib.vt_bn_add_act_bwd_reduce(vp(dy), Cc, None, Cc, vp(z), Cc, vp(f[2]), vp(f[3]), M, Cc, dt, vp(sums), s),
        lib.vt_bn_add_act_bwd_apply(vp(dy), Cc, vp(y), Cc, vp(z), Cc, None, vp(dz), Cc, vp(dr), Cc, 0, M, Cc, dt, s),
        lib.vt_bn_add_act_bwd_apply(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f), vp(dz), Cc, vp(dz), Cc, 0, M, Cc, dt, s),  # dz is dr
        lib.vt_bn_add_act_bwd_apply(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f), vp(dz), Cc, None, Cc, 0, M, Cc, dt, s),
        lib.vt_bn_add_act_bwd_finalize_apply(vp(sums), Cc, float(M), 1.0, vp(f[0]), vp(f[2]), vp(f[3]), 1, None, None, None, vp(dy), Cc,
                                             vp(y), Cc, vp(z), Cc, vp(dz), Cc, vp(dr), Cc, 0, M, dt, s),  # no coefficient buffer
        lib.vt_stem7_s2d(None, 8, vp(z), 16, 1, 4, 4, dt, s),
        lib.vt_stem7_s2d(vp(z), 8, vp(y), 8, 1, 2, 2, dt, s),  # ldo below the 16 channels
        lib.vt_stem7_s2d(vp(z), 8, vp(y), 16, 1, 0, 2, dt, s),
        lib.vt_stem7_pack_filter(None, N.VT_F32, vp(y), dt, 4, s),
        lib.vt_stem7_pack_filter(vp(z), N.VT_BF16, vp(f), N.VT_F32, 4, s),  # bf16 -> f32 is no path
        lib.vt_stem7_unpack_wgrad(None, 16, vp(f), 4, s),
        lib.vt_stem7_unpack_wgrad(vp(f), 8, vp(f), 4, s),  # fewer than the 12 real channels
    ]
    torch.cuda.synchronize()
    for k, rc in enumerate(bad):
        assert rc != 0, k
    assert N.last_error()


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 33, 31)], ids=str)
def test_stem_7x7_stride_2_forward_and_filter_gradient(shape, dtype):
    """Conv2d(3, 64, 7, 2, 3) through the space-to-depth image gather, the filter repack, vt_conv_igemm / vt_conv_wgrad with
    the 4x4 descriptor and the repack's transpose, against F.conv2d and its autograd in float64.  A random image: the
    borders (and the zero row / column an odd size adds) count."""
    B, _, H, W = shape
    Cout, epc = 64, 8 if dtype == N.VT_BF16 else 4
    lib = N.lib()
    x = rounded(filler.tensor(f"stem7x{shape}", shape), dtype)
    w = rounded(filler.tensor("stem7w", (Cout, 3, 7, 7)) * 0.1, dtype)
    wd = w.double().requires_grad_(True)
    y_ref = F.conv2d(x.double(), wd, None, 2, 3)
    Ho, Wo = y_ref.shape[2:]
    dz = rounded(filler.tensor(f"stem7dz{shape}", y_ref.shape), dtype)
    y_ref.backward(dz.double())

    xd = torch.zeros(B, H, W, epc, device="cuda", dtype=TD[dtype])  # the image as input_images lays it out
    xd[..., :3] = x.permute(0, 2, 3, 1).to("cuda", TD[dtype])
    Cs = lib.vt_stem7_s2d_channels(dtype)
    assert Cs == (16 if dtype == N.VT_BF16 else 12) and (Ho, Wo) == ((H + 1) // 2, (W + 1) // 2)
    xs = torch.full((B, Ho, Wo, Cs), float("nan"), device="cuda", dtype=TD[dtype])
    N.check(lib.vt_stem7_s2d(vp(xd), epc, vp(xs), Cs, B, H, W, dtype, stream()))
    # the gather itself, against a host restatement
    want = torch.zeros(B, 2 * Ho, 2 * Wo, 3)
    want[:, :H, :W] = x.permute(0, 2, 3, 1)
    want = want.reshape(B, Ho, 2, Wo, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, 12)
    assert torch.equal(xs[..., :12].float().cpu(), want) and (xs[..., 12:] == 0).all()

    w7 = krsc(w, dtype)  # [Cout][7][7][3]
    w4 = torch.full((Cout, 16, Cs), float("nan"), device="cuda", dtype=TD[dtype])
    N.check(lib.vt_stem7_pack_filter(vp(w7), dtype, vp(w4), dtype, Cout, stream()))
    if dtype == N.VT_BF16:  # from the f32 master too: the same values
        w4b, w7f = torch.empty_like(w4), w7.float().contiguous()
        N.check(lib.vt_stem7_pack_filter(vp(w7f), N.VT_F32, vp(w4b), dtype, Cout, stream()))
        assert torch.equal(w4, w4b)

    d = N.ConvDesc()
    d.dtype = dtype
    d.B, d.Hi, d.Wi, d.Cin, d.ldx = B, Ho, Wo, Cs, Cs
    d.Ho, d.Wo, d.sh, d.sw, d.h0, d.w0 = Ho, Wo, 1, 1, -2, -2
    d.Cout, d.ldy, d.oH, d.oW = Cout, Cout, Ho, Wo
    d.oHs = d.oWs = 1
    d.ldw, d.ntaps = 16 * Cs, 16
    for t in range(16):
        d.dh[t], d.dw[t] = t // 4, t % 4
    y = torch.empty(B, Ho, Wo, Cout, device="cuda", dtype=TD[dtype])
    N.check(lib.vt_conv_igemm(C.byref(d), vp(xs), vp(w4), vp(y), None, None, None, None, stream()))
    e_y = rel_err(to_nchw(y), y_ref.detach())

    dzd = nhwc(dz, dtype)
    dws = torch.zeros(Cout, 16, Cs, device="cuda")
    N.check(lib.vt_conv_wgrad(C.byref(d), vp(xs), vp(dzd), vp(dws), 16 * Cs, stream()))
    dw = torch.ones(Cout, 7, 7, 3, device="cuda")  # (the transpose accumulates)
    N.check(lib.vt_stem7_unpack_wgrad(vp(dws), Cs, vp(dw), Cout, stream()))
    torch.cuda.synchronize()
    e_w = rel_err((dw - 1).permute(0, 3, 1, 2).cpu(), wd.grad)
    print(f"{shape} {DNAME[dtype]}: y rel err {e_y:.3e}, dw rel err {e_w:.3e} ({N.last_kernel_name()})")
    assert e_y < tol(dtype) and e_w < tol(dtype)
