"""The keep forms of the add-then-ReLU BatchNorm passes (vt_resnet.hip: y = relu(keep[b] * bn(z) + r), stochastic depth of a
ResNet block) against the float64 statement of tests/rsb_util.py, modelled on tests/test_resnet_kernels_gpu.py: the bounds are
gpu_util.tol(dtype), the backward mask is read from the y the forward kernel stored, two channels have a sign the residual
alone decides, every launch runs twice and must be bit-identical, and a keep row of all ones must give the bits of the entry
points without `keep`.

A dropped image (keep[b] == 0): its z rows are NaN in the forward and in the reduction, which must not read them -- y is
relu(r) bit for bit; the identity's gradient is dy * [y > 0] bit for bit.  Its dz is 0 with the coefficients of a frozen
BatchNorm; under batch statistics it is -coef1 * z + coef2 (the image moved the mean and the variance the others were
normalised with), which is what the float64 autograd reference gives and what the test holds the kernel to there."""
import numpy as np
import pytest
import torch

from oracle import filler
from vision_toolbox import _native as N

import rsb_util as RU
from gpu_util import DNAME, DTYPES, TD, rel_err, rounded, short_grids, stream, tol, vp

pytestmark = pytest.mark.gpu

NAN = float("nan")
# (B, HW, C, ld): one row per image; a slice of a 40-wide NaN buffer where a workgroup's band of rows crosses images; a 7x7
# map with a channel count that is no power of two; 45 rows per image
CASES = [(2, 1, 8, None), (7, 3, 24, 40), (3, 49, 136, None), (5, 45, 72, None)]
KEEPS = {"ones": (1.0,), "zeros": (0.0,), "drop_first": (0.0, 1.25), "scaled": (0.5, 2.0)}
# on a grid of two row blocks per channel group: several trips of every thread's row loop, the last one partial (7 / 14 at 72
# channels, 25 with two finalize groups and 13 with the reduction's four groups at 256), 194 live rows in the last block, and
# the image boundary at row 130 inside the first block's band -- with a dropped, a kept and a rescaled image
SHORT_GRIDS = [(3, 130, 72, None), (3, 130, 256, None)]
CASES += SHORT_GRIDS
SHORT_GRID_KEEPS = {"ones": (1.0,), "mixed": (0.0, 1.0, 1.25)}
EPS, MOM = RU.EPS, RU.MOM


@pytest.fixture(autouse=True)
def _grid_of_the_case(request):
    """the SHORT_GRIDS cases run with two row blocks per channel group (gpu_util.short_grids)"""
    params = getattr(request.node, "callspec", None)
    with short_grids(params is not None and params.params.get("case") in SHORT_GRIDS):
        yield


def _keep(name, B):
    pat = {**KEEPS, **SHORT_GRID_KEEPS}[name]
    return torch.tensor([pat[b % len(pat)] for b in range(B)], dtype=torch.float32)


def _inputs(B, HW, Cc, dtype):
    M = B * HW
    key = f"rsb{B}x{HW}x{Cc}"
    # Two rows under batch statistics are the degenerate BatchNorm: xhat is +-d / sqrt(d^2 + eps) and dz is the gradient times
    # eps / (d^2 + eps) -- with a spread of 1.5 a 1e-5 remainder of cancelling terms, which no f32 pass (the one without keep
    # included, whose bits the row of ones must equal) holds to 2e-5 of ITS norm.  A spread of 0.01 keeps d^2 near eps, and the
    # two-row case well conditioned, at the same bound.
    z = rounded(filler.tensor(key + "z", (M, Cc)) * (1.5 if M >= 8 else 0.01) + 0.3, dtype)
    r = filler.tensor(key + "r", (M, Cc))
    gamma = filler.tensor(key + "g", (Cc,)) * 0.2 + 1.0
    beta = filler.tensor(key + "b", (Cc,)) * 0.2
    beta[0], beta[1] = 4.0, -4.0          # the two channels whose sign the residual alone decides
    r[:, 0] = -40.0 - r[:, 0].abs()
    r[:, 1] = 40.0 + r[:, 1].abs()
    r = rounded(r, dtype)
    dy = rounded(filler.tensor(key + "dy", (M, Cc)), dtype)
    dr0 = rounded(filler.tensor(key + "dr0", (M, Cc)), dtype)
    rm, rv = filler.tensor(key + "rm", (Cc,)) * 0.1, filler.tensor(key + "rv", (Cc,)).abs() + 0.5
    return z, r, gamma, beta, dy, dr0, rm, rv


def _place(t, dtype, ld):
    v = t.to("cuda", TD[dtype])
    if ld is None:
        return v, v, t.shape[1]
    wide = torch.full((t.shape[0], ld), NAN, device="cuda", dtype=TD[dtype])
    wide[:, 8 : 8 + t.shape[1]] = v
    return wide, wide[:, 8 : 8 + t.shape[1]], ld


def _outside_nan(wide, Cc, ld):
    return ld is None or bool(torch.isnan(wide[:, :8]).all() and torch.isnan(wide[:, 8 + Cc :]).all())


def _stats(z):
    st = N.stats_buffer(z.shape[1])
    zz = z.float().double()
    for rep, idx in enumerate(torch.chunk(torch.arange(z.shape[0], device="cuda"), N.VT_STAT_REPLICAS)):
        if idx.numel():
            N.stats_encode(st, 0, zz[idx].sum(0), rep)
            N.stats_encode(st, 1, (zz[idx] ** 2).sum(0), rep)
    return st


def _same(a, b):
    a, b = a.float(), b.float()
    return torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _rows(keep, HW, value):
    """row mask [M] of the images whose factor is `value`"""
    return (keep == value).repeat_interleave(HW)


def _forward(lib, fin, z_dev, ldz, r_dev, ldr, y_dev, ldy, coefs, gamma, beta, rm, rv, stats_of, keep_dev, HW, M, Cc, dtype):
    """one forward launch, with `keep_dev` or (None) through the entry point without it; returns the coefficient buffer"""
    if fin:
        st = _stats(stats_of)
        rmd, rvd = rm.cuda(), rv.cuda()
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        coef = torch.zeros(4, Cc, device="cuda")
        head = (vp(st), Cc, float(M), vp(gamma), vp(beta), EPS, MOM, vp(rmd), vp(rvd), vp(nbt), vp(coef[0]), vp(coef[1]), vp(coef[2]),
                vp(coef[3]), vp(z_dev), ldz, vp(r_dev), ldr, vp(y_dev), ldy)
        if keep_dev is None:
            N.check(lib.vt_bn_add_act_finalize_apply(*head, M, dtype, stream()))
        else:
            N.check(lib.vt_bn_add_act_keep_finalize_apply(*head, vp(keep_dev), HW, M, dtype, stream()))
        return coef
    cd = coefs.cuda()
    head = (vp(z_dev), ldz, vp(cd[0]), vp(cd[1]), vp(r_dev), ldr, vp(y_dev), ldy)
    if keep_dev is None:
        N.check(lib.vt_bn_add_act_apply(*head, M, Cc, dtype, stream()))
    else:
        N.check(lib.vt_bn_add_act_keep_apply(*head, vp(keep_dev), HW, M, Cc, dtype, stream()))
    return cd


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_keep_forward(case, dtype):
    B, HW, Cc, ld = case
    M = B * HW
    z, r, gamma, beta, dy, dr0, rm, rv = _inputs(B, HW, Cc, dtype)
    lib = N.lib()
    gd, bd = gamma.cuda(), beta.cuda()
    for kname in (SHORT_GRID_KEEPS if case in SHORT_GRIDS else KEEPS):
        keep = _keep(kname, B)
        kd = keep.cuda()
        dropped = _rows(keep, HW, 0.0)
        z_nan = z.clone()
        z_nan[dropped] = NAN   # a dropped image's rows of z are not read
        for fin in (False, True):  # ready coefficients (a frozen BatchNorm's) | the finalize step inside the launch
            y_want, coefs, *_ = RU.unit_reference(z, r, gamma, beta, dy, rm, rv, keep, HW, 1 if fin else 0)
            if kname == "scaled":
                assert (y_want[:, 0] == 0).all() and (y_want[:, 1] > 0).all()   # the residual alone decides
                if M * Cc >= 256:   # (a fraction of a dozen elements says nothing)
                    assert 0.25 < (y_want[:, 2:] == 0).double().mean().item() < 0.75
            runs = []
            for _ in range(2):
                zw, zv, ldz = _place(z_nan, dtype, ld)
                rw, rvw, ldr = _place(r, dtype, ld)
                yw, yv, ldy = _place(torch.full((M, Cc), NAN), dtype, ld)
                coef = _forward(lib, fin, zv, ldz, rvw, ldr, yv, ldy, coefs, gd, bd, rm, rv, z.to("cuda", TD[dtype]), kd, HW, M, Cc, dtype)
                torch.cuda.synchronize()
                runs.append((yw, coef))
            what = f"{kname} fin={fin}"
            for a, b in zip(*runs):
                assert _same(a, b), what
            y = (yw[:, 8 : 8 + Cc] if ld else yw).float().cpu()
            assert bool(torch.isfinite(y).all()), what
            assert torch.equal(y[dropped], torch.relu(r[dropped])), what
            err = rel_err(y, y_want)
            print(f"{case} {DNAME[dtype]} {what}: y rel err {err:.3e}")
            assert err < tol(dtype), what
            assert _outside_nan(yw, Cc, ld) and _outside_nan(zw, Cc, ld) and _outside_nan(rw, Cc, ld), what
            if fin:
                assert rel_err(runs[0][1].cpu(), coefs) < 2e-5, what
            if kname == "ones":   # the bits of the pass without keep
                pw, pv, ldp = _place(torch.full((M, Cc), NAN), dtype, ld)
                _forward(lib, fin, zv, ldz, rvw, ldr, pv, ldp, coefs, gd, bd, rm, rv, z.to("cuda", TD[dtype]), None, HW, M, Cc, dtype)
                torch.cuda.synchronize()
                assert _same(pw, yw), what


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_keep_backward(case, dtype):
    B, HW, Cc, ld = case
    M = B * HW
    z, r, gamma, beta, dy, dr0, rm, rv = _inputs(B, HW, Cc, dtype)
    lib = N.lib()
    for kname in (SHORT_GRID_KEEPS if case in SHORT_GRIDS else KEEPS):
        keep = _keep(kname, B)
        kd = keep.cuda()
        dropped = _rows(keep, HW, 0.0)
        z_nan = z.clone()
        z_nan[dropped] = NAN
        for train in (1, 0):
            _, coefs, *_ = RU.unit_reference(z, r, gamma, beta, dy, rm, rv, keep, HW, train)
            cd = coefs.cuda()
            # the stored y the mask is read from: what the forward keep kernel wrote
            yd = torch.empty(M, Cc, device="cuda", dtype=TD[dtype])
            zd0, rd0 = z.to("cuda", TD[dtype]), r.to("cuda", TD[dtype])
            N.check(lib.vt_bn_add_act_keep_apply(vp(zd0), Cc, vp(cd[0]), vp(cd[1]), vp(rd0), Cc, vp(yd), Cc, vp(kd), HW, M, Cc, dtype,
                                                 stream()))
            y_cpu = yd.float().cpu()
            _, _, dz_ref, dr_ref, dg_ref, db_ref = RU.unit_reference(z, r, gamma, beta, dy, rm, rv, keep, HW, train, y_mask=y_cpu)
            g64 = dy.double() * (y_cpu.double() > 0)
            assert torch.equal(dr_ref, g64)
            gw, gv, ldg = _place(dy, dtype, ld)
            yw, yv, ldy = _place(y_cpu, dtype, ld)
            zw, zv, ldz = _place(z, dtype, ld)
            _, znv, _ = _place(z_nan, dtype, ld)   # the reduction does not read a dropped image's rows
            sums = [N.stats_buffer(Cc), N.stats_buffer(Cc)]
            for s_ in sums:
                N.check(lib.vt_bn_add_act_keep_bwd_reduce(vp(gv), ldg, vp(yv), ldy, vp(znv), ldz, vp(cd[2]), vp(cd[3]), vp(kd), HW, M, Cc,
                                                          dtype, vp(s_), stream()))
            torch.cuda.synchronize()
            assert torch.equal(N.stats_decode(sums[0]), N.stats_decode(sums[1]))
            got = N.stats_decode(sums[0]).cpu()
            u64 = g64 * keep.double().repeat_interleave(HW).view(M, 1)
            xhat = (z.double() - coefs[2].double()) * coefs[3].double()
            np.testing.assert_allclose(got[0], u64.sum(0), rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(got[1], (u64 * xhat).sum(0), rtol=1e-4, atol=1e-4)
            if kname == "ones":
                plain = N.stats_buffer(Cc)
                N.check(lib.vt_bn_add_act_bwd_reduce(vp(gv), ldg, vp(yv), ldy, vp(zv), ldz, vp(cd[2]), vp(cd[3]), M, Cc, dtype, vp(plain),
                                                     stream()))
                torch.cuda.synchronize()
                assert torch.equal(plain, sums[0])
            for accumulate in (0, 1):
                for fin in (False, True):
                    what = f"{kname} train={train} accumulate={accumulate} fin={fin}"
                    runs = []
                    for use_keep in (True, True, False):   # twice with keep; once without, compared for the row of ones
                        if not use_keep and kname != "ones":
                            continue
                        dzw, dzv, lddz = _place(torch.full((M, Cc), NAN), dtype, ld)
                        drw, drv, lddr = _place(dr0 if accumulate else torch.full((M, Cc), NAN), dtype, ld)
                        dg, db = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
                        bc = torch.zeros(3, Cc, device="cuda")
                        tail = (vp(kd), HW) if use_keep else ()
                        if fin:
                            fn = lib.vt_bn_add_act_keep_bwd_finalize_apply if use_keep else lib.vt_bn_add_act_bwd_finalize_apply
                            N.check(fn(vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[2]), vp(cd[3]), train, vp(dg), vp(db), vp(bc),
                                       vp(gv), ldg, vp(yv), ldy, vp(zv), ldz, vp(dzv), lddz, vp(drv), lddr, accumulate, *tail, M, dtype,
                                       stream()))
                        else:
                            N.check(lib.vt_bn_bwd_finalize(vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[2]), vp(cd[3]), train, vp(dg),
                                                           vp(db), vp(bc), stream()))
                            fn = lib.vt_bn_add_act_keep_bwd_apply if use_keep else lib.vt_bn_add_act_bwd_apply
                            N.check(fn(vp(gv), ldg, vp(yv), ldy, vp(zv), ldz, vp(bc), vp(dzv), lddz, vp(drv), lddr, accumulate, *tail, M,
                                       Cc, dtype, stream()))
                        torch.cuda.synchronize()
                        runs.append((dzw, drw, dg, db, bc))
                    for other in runs[1:]:   # the second run, and for the row of ones the entry point without keep
                        for a, b in zip(runs[0], other):
                            assert _same(a, b), what
                    dzw, drw, dg, db, bc = runs[0]
                    dz_got = (dzw[:, 8 : 8 + Cc] if ld else dzw).float().cpu()
                    dr_got = (drw[:, 8 : 8 + Cc] if ld else drw).float().cpu()
                    assert bool(torch.isfinite(dz_got).all() and torch.isfinite(dr_got).all()), what
                    dr_want = dr_ref + (dr0.double() if accumulate else 0.0)
                    e_dz, e_dr = rel_err(dz_got, dz_ref), rel_err(dr_got, dr_want)
                    print(f"{case} {DNAME[dtype]} {what}: dz rel err {e_dz:.3e}, dr rel err {e_dr:.3e}")
                    assert e_dz < tol(dtype) and e_dr < tol(dtype), what
                    if not accumulate:   # the identity receives g itself, whatever the factor: bit for bit
                        assert torch.equal(dr_got.double(), g64), what
                    if not train:        # a frozen BatchNorm: a dropped image's dz is zero
                        assert not dz_got[dropped].any(), what
                    elif kname == "zeros":
                        assert not dz_got.any(), what
                    np.testing.assert_allclose((dg - 1).cpu(), dg_ref, rtol=1e-4, atol=1e-4)
                    np.testing.assert_allclose((db - 1).cpu(), db_ref, rtol=1e-4, atol=1e-4)
                    assert _outside_nan(dzw, Cc, ld) and _outside_nan(drw, Cc, ld), what
            assert _outside_nan(gw, Cc, ld) and _outside_nan(yw, Cc, ld) and _outside_nan(zw, Cc, ld)


def test_bad_arguments_return_an_error_code():
    lib = N.lib()
    B, HW, Cc, dt = 2, 5, 16, N.VT_BF16
    M = B * HW
    t = lambda: torch.zeros(M, Cc, device="cuda", dtype=torch.bfloat16)  # noqa: E731
    z, r, y, dy, dz, dr = t(), t(), t(), t(), t(), t()
    f = torch.zeros(4, Cc, device="cuda")
    k = torch.ones(B, device="cuda")
    sums = N.stats_buffer(Cc)
    s = stream()
    bad = [
        lib.vt_bn_add_act_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, None, HW, M, Cc, dt, s),      # no keep
        lib.vt_bn_add_act_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(k), 0, M, Cc, dt, s),      # HW = 0
        lib.vt_bn_add_act_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(k), 3, M, Cc, dt, s),      # HW does not divide M
        lib.vt_bn_add_act_keep_apply(None, Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(k), HW, M, Cc, dt, s),
        lib.vt_bn_add_act_keep_bwd_reduce(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f[2]), vp(f[3]), None, HW, M, Cc, dt, vp(sums), s),
        lib.vt_bn_add_act_keep_bwd_reduce(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f[2]), vp(f[3]), vp(k), 4, M, Cc, dt, vp(sums), s),
        lib.vt_bn_add_act_keep_bwd_apply(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f), vp(dz), Cc, vp(dz), Cc, 0, vp(k), HW, M, Cc, dt, s),
        lib.vt_bn_add_act_keep_bwd_apply(vp(dy), Cc, vp(y), Cc, vp(z), Cc, vp(f), vp(dz), Cc, vp(dr), Cc, 0, None, HW, M, Cc, dt, s),
        lib.vt_bn_add_act_keep_bwd_finalize_apply(vp(sums), Cc, float(M), 1.0, vp(f[0]), vp(f[2]), vp(f[3]), 1, None, None, None, vp(dy),
                                                  Cc, vp(y), Cc, vp(z), Cc, vp(dz), Cc, vp(dr), Cc, 0, vp(k), HW, M, dt, s),
        lib.vt_bn_add_act_keep_finalize_apply(None, Cc, float(M), None, None, EPS, MOM, None, None, None, vp(f[0]), vp(f[1]), vp(f[2]),
                                              vp(f[3]), vp(z), Cc, vp(r), Cc, vp(y), Cc, vp(k), HW, M, dt, s),
    ]
    torch.cuda.synchronize()
    for i, rc in enumerate(bad):
        assert rc != 0, i
    assert N.last_error()
