"""The convolution kernels (vt_igemm.hip, vt_igemm_span.hip, vt_igemm_span6.hip, vt_igemm_pspan.hip, vt_stem.hip,
vt_stem6.hip, vt_wgrad.hip, vt_wgrad_span.hip, vt_wgrad6.hip: the Conv2d of components.py:26-35 forward, its data gradients
and its filter gradient) through the C ABI, against exact and elementwise references (conv_parity_util.py).

Part A: lattice inputs, torch.equal against the integer reference -- one dropped tap, one pixel read across an image
boundary, one filter-column tail changes a value and fails.  Part B: free-running inputs, every element within the rounding
bound of a float64 reference -- a truncating store, a narrow accumulator, a scale applied after the store fail.

Every launch writes into a NaN-filled buffer (nothing outside the channel slice may change), asserts the kernel family and
tile it was forced onto in last_kernel_name(), and restores the knobs it set."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from vision_toolbox import _native as N

import conv_parity_util as P
from gpu_util import conv_desc, krsc, nhwc, stream, to_nchw, vp
from test_dgrad_d2s_gpu import TAPS, _class, _desc as d2s_desc, _pack

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(autouse=True)
def _a_device_error_ends_the_run():
    """a device error is sticky: every later launch of the process would fail on it, so the run ends with the first one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further launches: {e}", returncode=3)


@contextlib.contextmanager
def knobs(kv):
    try:
        for k, v in kv.items():
            N.set_knob(k, v)
        yield
    finally:
        for k in kv:
            N.set_knob(k, P.KNOB_DEFAULTS[k])


def check_name(name, want):
    for s in want:
        if s.startswith("!"):
            assert s[1:] not in name, (name, want)
        else:
            assert s in name, (name, want)


def sliced_out(shape, C_, dtype, sliced):
    """a NaN-filled [.., ld] buffer and the channel slice of it a kernel writes"""
    ld, off = (C_ + 24, 16) if sliced else (C_, 0)
    wide = torch.full(tuple(shape) + (ld,), NAN, device="cuda", dtype=P.TD[dtype])
    return wide, wide[..., off:off + C_], ld


def untouched_outside(wide, view_off, C_):
    inside = torch.zeros(wide.shape[-1], dtype=torch.bool, device="cuda")
    inside[view_off:view_off + C_] = True
    nan = torch.isnan(wide.float())
    return bool(nan[..., ~inside].all()) and not bool(nan[..., inside].any())


def run_conv(case, lat):
    """-> (y as NCHW f32 on the CPU, kernel name, statistics or None)"""
    B, Cin, Cout, k, s, H, W = case.shape
    x, w, _, _ = P.conv_operands(case.shape, case.flip, lat, case.dtype)
    sc, sh, res = P.epilogue_operands(case, lat)
    Ho, Wo = P.out_hw(case.shape)
    dt, flags = case.dtype, P.MODES[case.mode]
    xs = case.sliced and Cin != 8  # (the RGB stem kernels take a dense 16-byte pixel only)
    xd = nhwc(x, dt, ld=Cin + 16, coff=8) if xs else nhwc(x, dt)
    wd = krsc(w, dt)
    wide, y, ldy = sliced_out((B, Ho, Wo), Cout, dt, case.sliced)
    rd = (nhwc(res, dt, ld=Cout + 8, coff=8) if case.sliced else nhwc(res, dt)) if res is not None else None
    scd = sc.cuda().float().contiguous() if sc is not None else None
    shd = sh.cuda().float().contiguous() if sh is not None else None
    st = N.stats_buffer(Cout) if flags & P.STATS else None
    d = conv_desc(dt, xd, Cin, Cout, k, s, P.pad_of(k, s), ldy, flags=flags, ldr=rd.stride(2) if rd is not None else 0)
    if case.flip:
        for i in range(k * k):
            t = k * k - 1 - i
            d.dh[i], d.dw[i] = t // k, t % k
    lib = N.lib()
    with knobs(case.knobs):
        before = N.launch_count()
        if case.mode == "bnred":
            # d(y) of vt_conv_dgrad_bnred: the unit's z and BatchNorm coefficients only feed the sums (test_dgrad_bnred_gpu.py)
            zd = torch.randn(B, Ho, Wo, Cout, device="cuda").to(P.TD[dt])
            one = torch.ones(Cout, device="cuda")
            sums = N.stats_buffer(Cout)
            N.check(lib.vt_conv_dgrad_bnred(C.byref(d), vp(xd), vp(wd), vp(y), vp(zd), Cout, vp(one), vp(one), vp(one), vp(one), 1,
                                            vp(sums), stream()))
        else:
            N.check(lib.vt_conv_igemm(C.byref(d), vp(xd), vp(wd), vp(y), vp(scd), vp(shd), vp(rd), vp(st), stream()))
        torch.cuda.synchronize()
        name = N.last_kernel_name()
        assert N.launch_count() - before == 1, (name, N.launch_count() - before)
    check_name(name, case.kernel)
    assert untouched_outside(wide, 16 if case.sliced else 0, Cout), "the launch wrote outside its channel slice (or left NaN inside)"
    return to_nchw(y), name, (N.stats_decode(st).cpu() if st is not None else None)


# ---- Part A ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CONV_CASES, ids=lambda c: c.id)
def test_lattice_conv_is_exact(case):
    ref, v = P.conv_reference(case, True)
    x, w, _, _ = P.conv_operands(case.shape, case.flip, True, case.dtype)
    P.lattice_ok(ref, case.dtype, x, w, *[t for t in P.epilogue_operands(case, True)[1:] if t is not None])
    P.stored_ok(case, ref, v)
    got, name, st = run_conv(case, True)
    bad = (got != ref.float()).nonzero()
    assert torch.equal(got, ref.float()), f"{name}: {len(bad)} of {got.numel()} elements differ, first (b, c, i, j) = {bad[:8].tolist()}"
    if st is not None:  # the statistics of integers: sums of the stored values in fixed point
        r64 = ref.double()
        np.testing.assert_allclose(st[0], r64.sum((0, 2, 3)), rtol=1e-6, atol=1e-3)
        np.testing.assert_allclose(st[1], (r64 * r64).sum((0, 2, 3)), rtol=1e-6, atol=1e-3)


def run_wgrad(case, lat):
    """-> list over the layers of (dw [Cout][k][k][Cin] f32 on the CPU), kernel name"""
    B, Cin, Cout, k, s, H, W = case.shape
    dt, K = case.dtype, case.shape[3] ** 2 * Cin
    lib = N.lib()
    xs, dzs, dws, wides = [], [], [], []
    for layer in range(case.n):
        x, dz, g0, _, _ = P.wgrad_operands(case.shape, lat, dt, layer)
        xs.append(nhwc(x, dt, ld=Cin + 16, coff=8) if case.sliced else nhwc(x, dt))
        dzs.append(nhwc(dz, dt, ld=Cout + 24, coff=16) if case.sliced else nhwc(dz, dt))
        ldgw = K + 8 if case.sliced else K
        wide = torch.full((Cout, ldgw), NAN, device="cuda")
        wide[:, :K] = g0.reshape(Cout, K).cuda()  # the kernels accumulate into the gradient that is already there
        wides.append(wide)
    d = conv_desc(dt, xs[0], Cin, Cout, k, s, P.pad_of(k, s), dzs[0].stride(2))
    with knobs(case.knobs):
        before = N.launch_count()
        if case.entry == "wgrad":
            N.check(lib.vt_conv_wgrad(C.byref(d), vp(xs[0]), vp(dzs[0]), vp(wides[0]), ldgw, stream()))
        elif case.entry == "slabs":
            scratch = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
            N.check(lib.vt_conv_wgrad_slabs(C.byref(d), vp(xs[0]), vp(dzs[0]), vp(wides[0]), ldgw, vp(scratch),
                                            C.c_int64(scratch.numel()), stream()))
        else:
            arr = lambda ts: (C.c_void_p * case.n)(*[t.data_ptr() for t in ts])  # noqa: E731
            N.check(lib.vt_conv_wgrad_group(C.byref(d), case.n, arr(xs), arr(dzs), arr(wides), ldgw, stream()))
        torch.cuda.synchronize()
        name = N.last_kernel_name()
        launches = N.launch_count() - before
    check_name(name, case.kernel)
    if case.launches is not None:
        assert launches == case.launches, (name, launches)
    for wide in wides:
        assert not torch.isnan(wide[:, :K]).any() and torch.isnan(wide[:, K:]).all(), "wrote outside ldgw's first K columns"
    return [wd[:, :K].reshape(Cout, k, k, Cin).cpu() for wd in wides], name


@pytest.mark.parametrize("case", P.WGRAD_CASES, ids=lambda c: c.id)
def test_lattice_filter_gradient_is_exact(case):
    got, name = run_wgrad(case, True)
    for layer in range(case.n):
        x, dz, g0, ref, _ = P.wgrad_operands(case.shape, True, case.dtype, layer)
        P.lattice_ok(ref, P.F32, x, dz, g0)
        bad = (got[layer] != ref).nonzero()
        assert torch.equal(got[layer], ref), f"{name} layer {layer}: {len(bad)} elements differ, first (n, r, t, c) = {bad[:8].tolist()}"


def run_d2s(B, Cin, Cout, H, W, ldx, with_res, kn, lat, one_launch):
    """d(x) of a 3x3 stride-2 convolution as four parity-class launches or as ONE depth-to-space launch"""
    dz, w, res, _, _, _ = P.d2s_operands(B, Cin, Cout, H, W, lat, with_res)
    lib = N.lib()
    Hz, Wz = H // 2, W // 2
    dzd = nhwc(dz, P.BF16)
    wd = krsc(w, P.BF16).reshape(Cout, 9, Cin)  # [n][tap][c], the forward filter
    dx = torch.full((B, H, W, ldx), NAN, device="cuda", dtype=torch.bfloat16)
    rd = None
    if with_res:
        rd = torch.full((B, H, W, ldx), NAN, device="cuda", dtype=torch.bfloat16)
        rd[..., :Cin] = res.permute(0, 2, 3, 1).cuda().bfloat16()
    rflag = N.VT_CONV_RESIDUAL if with_res else 0
    names = []
    with knobs(kn):
        if one_launch:
            wd4 = torch.empty(4, Cin, 4, Cout, device="cuda", dtype=torch.bfloat16)
            for ph in range(2):
                for pw in range(2):
                    rows, cols, eh, ew = _class(ph, pw)
                    sel = []
                    for (a, b) in TAPS:
                        u, v = eh - a, ew - b
                        sel.append(rows[u] * 3 + cols[v] if 0 <= u < len(rows) and 0 <= v < len(cols) else -1)
                    _pack(lib, wd, wd4[2 * ph + pw], sel, Cout, Cin)
            d = d2s_desc(B, Hz, Wz, Cout, Cout, H, W, 4 * Cin, ldx, ldx, 4, TAPS, N.VT_CONV_D2S | rflag)
            N.check(lib.vt_conv_igemm(C.byref(d), vp(dzd), vp(wd4), vp(dx), None, None, vp(rd), None, stream()))
            names.append(N.last_kernel_name())
        else:
            keep = []
            for ph in range(2):
                for pw in range(2):
                    rows, cols, eh, ew = _class(ph, pw)
                    sel = [r * 3 + t for r in rows for t in cols]
                    offs = [(eh - u, ew - v) for u in range(len(rows)) for v in range(len(cols))]
                    wc = torch.empty(Cin, len(sel), Cout, device="cuda", dtype=torch.bfloat16)
                    keep.append(wc)
                    _pack(lib, wd, wc, sel, Cout, Cin)
                    d = d2s_desc(B, Hz, Wz, Cout, Cout, H, W, Cin, ldx, ldx, len(sel), offs, rflag, ph, pw)
                    N.check(lib.vt_conv_igemm(C.byref(d), vp(dzd), vp(wc), vp(dx), None, None, vp(rd), None, stream()))
                    names.append(N.last_kernel_name())
        torch.cuda.synchronize()
    assert untouched_outside(dx, 0, Cin)
    return to_nchw(dx[..., :Cin]), names


@pytest.mark.parametrize("one_launch", [False, True], ids=["four_class_launches", "one_d2s_launch"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,ldx,with_res,kn,kernel,class_kernel", P.D2S_CASES)
def test_lattice_stride2_data_gradient_is_exact(B, Cin, Cout, H, W, ldx, with_res, kn, kernel, class_kernel, one_launch):
    dz, w, res, ref, v, _ = P.d2s_operands(B, Cin, Cout, H, W, True, with_res)
    P.lattice_ok(ref, P.BF16, dz, w, res)
    assert torch.equal(v.bfloat16().float(), v)
    got, names = run_d2s(B, Cin, Cout, H, W, ldx, with_res, kn, True, one_launch)
    for name in names:  # one name, or the four class launches
        check_name(name, kernel if one_launch else class_kernel)
    bad = (got != ref).nonzero()
    assert torch.equal(got, ref), f"{names}: {len(bad)} elements differ, first (b, c, i, j) = {bad[:8].tolist()}"


# ---- Part B ----------------------------------------------------------------------------------------------------------
def report(kind, name, case_id, ratio, of_bound):
    """one line per Part B launch (pytest -s): the worst (|got - ref| - r |ref|) / ((K + 1) u S) and the worst |got - ref| / bound"""
    print(f"\nPARTB {kind} | {name} | {case_id} | {ratio:.3f} | {of_bound:.3f}")


@pytest.mark.parametrize("case", [c for c in P.CONV_CASES if c.partb], ids=lambda c: c.id)
def test_conv_elementwise_bound(case):
    ref, _ = P.conv_reference(case, False)
    bound = P.conv_bound(case, P.A_MFMA)
    got, name, _ = run_conv(case, False)
    _, _, z, S = P.conv_operands(case.shape, case.flip, False, case.dtype)
    nbad, worst = P.within(got, ref, bound)
    # (the ratio to (K + 1) u S is that of the accumulator alone where the epilogue is plain: else the epilogue's own counted
    #  roundings are in it, and the bound is the figure to read)
    report("conv", name, case.id, P.worst_ratio(got, ref, S, case.shape[1] * case.shape[3] ** 2, case.dtype), worst)
    assert nbad == 0, f"{name}: {nbad} of {got.numel()} elements outside the bound, worst {worst:.3f} x"


@pytest.mark.parametrize("case", [c for c in P.WGRAD_CASES if c.partb], ids=lambda c: c.id)
def test_filter_gradient_elementwise_bound(case):
    got, name = run_wgrad(case, False)
    Ho, Wo = P.out_hw(case.shape)
    for layer in range(case.n):
        _, _, g0, ref, S = P.wgrad_operands(case.shape, False, case.dtype, layer)
        bound = P.wgrad_bound(case.shape, case.dtype, layer, P.A_MFMA)
        nbad, worst = P.within(got[layer], ref, bound)
        report("wgrad", name, case.id, P.worst_ratio(got[layer], ref, S, case.shape[0] * Ho * Wo, P.F32), worst)
        assert nbad == 0, f"{name} layer {layer}: {nbad} elements outside the bound, worst {worst:.3f} x"


@pytest.mark.parametrize("one_launch", [False, True], ids=["four_class_launches", "one_d2s_launch"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,ldx,with_res,kn,kernel,class_kernel", P.D2S_CASES[1:])
def test_stride2_data_gradient_elementwise_bound(B, Cin, Cout, H, W, ldx, with_res, kn, kernel, class_kernel, one_launch):
    dz, w, res, ref, v, S = P.d2s_operands(B, Cin, Cout, H, W, False, with_res)
    bound = P.d2s_bound(B, Cin, Cout, H, W, with_res, P.A_MFMA)
    got, names = run_d2s(B, Cin, Cout, H, W, ldx, with_res, kn, False, one_launch)
    for name in names:
        check_name(name, kernel if one_launch else class_kernel)
    nbad, worst = P.within(got, ref, bound)
    report("d2s", names[-1], "x".join(map(str, (B, Cin, Cout, H, W))) + ("-res" if with_res else ""),
           P.worst_ratio(got, ref, S, 4 * Cout, P.BF16), worst)
    assert nbad == 0, f"{names}: {nbad} elements outside the bound, worst {worst:.3f} x"


# ---- grouped and depthwise kernels: lattice cases -------------------------------------------------------------------------
def _in(t, dtype, sliced):
    """NCHW cpu tensor -> device NHWC and its pixel stride (dense, or channels [8, 8 + C) of a NaN-filled buffer 16 wider)"""
    Cc = t.shape[1]
    return (nhwc(t, dtype, Cc + 16, 8), Cc + 16) if sliced else (nhwc(t, dtype), Cc)


def _grouped_launches(kind, shape, dtype, sliced):
    """forward, data gradient without and with a residual, filter gradient into the gradient that is already there"""
    B, Cc, H, W, k, s, pad, dil, groups, gw = P.grouped_geometry(kind, shape)
    c, lib = P.grouped_operands(kind, shape), N.lib()
    Ho, Wo = c["z"].shape[2:]
    (x, ldx), (dz, lddz), (res, ldr) = _in(c["x"], dtype, sliced), _in(c["dz"], dtype, sliced), _in(c["res"], dtype, sliced)
    zw, z, ldz = sliced_out((B, Ho, Wo), Cc, dtype, sliced)
    dxw, dx, lddx = sliced_out((B, H, W), Cc, dtype, sliced)
    dxrw, dxr, _ = sliced_out((B, H, W), Cc, dtype, sliced)
    dw = c["g0"].cuda().contiguous()
    if kind == "gconv":
        w = krsc(c["w"], dtype)
        geo = (B, H, W, Cc, gw, s, dtype)
        N.check(lib.vt_gconv3_fwd(vp(x), ldx, vp(w), vp(z), ldz, None, *geo, stream()))
        N.check(lib.vt_gconv3_dgrad(vp(dz), lddz, vp(w), vp(dx), lddx, None, 0, *geo, stream()))
        N.check(lib.vt_gconv3_dgrad(vp(dz), lddz, vp(w), vp(dxr), lddx, vp(res), ldr, *geo, stream()))
        nbytes = lib.vt_gconv3_wgrad_scratch_bytes(B, H, W, Cc, gw, s)
        assert nbytes > 0
        scratch = torch.full((nbytes // 4,), NAN, device="cuda")
        N.check(lib.vt_gconv3_wgrad(vp(x), ldx, vp(dz), lddz, vp(dw), vp(scratch), nbytes, *geo, stream()))
    else:
        w = c["w"].reshape(Cc, k * k).cuda().contiguous()  # the f32 master [C][k*k]
        dw = dw.reshape(Cc, k * k)
        if kind == "dwt":
            geo = (B, H, W, Cc, k, s, dtype)
            nbytes = lib.vt_dwt_shares_bytes(*geo)
            assert nbytes > 0
            N.check(lib.vt_dwt_fwd(vp(x), ldx, vp(w), vp(z), ldz, None, *geo, stream()))
            for out, r, lr in ((dxr, res, ldr), (dx, None, 0)):  # (the shares of the second launch feed the reducer)
                shares = torch.full((nbytes // 4,), NAN, device="cuda")
                N.check(lib.vt_dwt_bwd(vp(dz), lddz, vp(x), ldx, vp(w), vp(out), lddx, vp(r), lr, vp(shares), nbytes, *geo, stream()))
            N.check(lib.vt_dwt_wgrad_reduce(vp(shares), nbytes, vp(dw), *geo, stream()))
        else:
            geo = (B, H, W, Cc, k, s, pad, dil, dtype)
            N.check(lib.vt_dwconv_fwd(vp(x), ldx, vp(w), vp(z), ldz, None, *geo, stream()))
            N.check(lib.vt_dwconv_dgrad(vp(dz), lddz, vp(w), vp(dx), lddx, None, 0, *geo, stream()))
            N.check(lib.vt_dwconv_dgrad(vp(dz), lddz, vp(w), vp(dxr), lddx, vp(res), ldr, *geo, stream()))
            N.check(lib.vt_dwconv_wgrad(vp(x), ldx, vp(dz), lddz, vp(dw), *geo, stream()))
    torch.cuda.synchronize()
    off = 16 if sliced else 0
    for wide in (zw, dxw, dxrw):
        assert untouched_outside(wide, off, Cc), "wrote outside its channel slice (or left NaN inside)"
    return to_nchw(z), to_nchw(dx), to_nchw(dxr), dw.reshape(Cc, k, k, gw).cpu()


GROUPED = [("gconv", s) for s in P.GCONV_SHAPES] + [("dwt", s) for s in P.DWT_SHAPES] + [("dwconv", s) for s in P.DWCONV_CASES]


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind,shape", GROUPED, ids=[k + "-" + "x".join(map(str, s)) for k, s in GROUPED])
def test_lattice_grouped_and_depthwise_are_exact(kind, shape, dtype, sliced):
    c = P.grouped_operands(kind, shape)
    P.grouped_ok(c, dtype)
    before = N.launch_count()
    z, dx, dxr, dw = _grouped_launches(kind, shape, dtype, sliced)
    assert N.launch_count() >= before + 4  # (vt_gconv.hip, vt_dwtile.hip and vt_dwconv.hip have one kernel per entry point and
    #                                          record no name: last_kernel_name() has nothing to say about them)
    for key, got in (("z", z), ("dx", dx), ("dxr", dxr), ("dw", dw)):
        bad = (got != c[key]).nonzero()
        assert torch.equal(got, c[key]), f"{kind} {key}: {len(bad)} of {got.numel()} elements differ, first {bad[:8].tolist()}"
