"""CPU side of the convolution parity tests: (1) every lattice case of test_conv_parity_gpu.py meets the conditions that make
torch.equal a fair comparison (a bad draw is found here, not on the GPU); (2) a plain restatement of each Part B case --
F.conv2d in f32 on the dtype-rounded operands, the epilogue in f32, stored in the dtype -- stays within the Part B bound with
a = 1; (3) the new checks see what the norm of gpu_util.rel_err does not: one dropped tap, one value swapped with its
neighbouring pixel's, a truncating bf16 store all pass rel_err < tol(bf16) = 6e-3 on 71,808 outputs and fail here."""
import pytest
import torch
import torch.nn.functional as F

import conv_parity_util as P


def _rel_err(a, b):  # gpu_util.rel_err (that module loads the native library)
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


TOL_BF16 = 6e-3  # gpu_util.tol(bf16)


_F64_SEEN: dict = {}


def _f32_equals_f64(shape, flip):
    if (shape, flip) not in _F64_SEEN:
        x, w, z, _ = P.conv_operands(shape, flip, True, P.BF16)
        B, Cin, Cout, k, s, H, W = shape
        _F64_SEEN[(shape, flip)] = torch.equal(F.conv2d(x.double(), P.w_ref(w, flip).double(), None, s, P.pad_of(k, s)), z.double())
    return _F64_SEEN[(shape, flip)]


# ---- 1. lattice conditions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CONV_CASES, ids=lambda c: c.id)
def test_lattice_conv_case_is_exactly_representable(case):
    ref, v = P.conv_reference(case, True)
    x, w, z, _ = P.conv_operands(case.shape, case.flip, True, case.dtype)
    sc, sh, res = P.epilogue_operands(case, True)
    P.lattice_ok(ref, case.dtype, x, w, sh, res)
    P.stored_ok(case, ref, v)
    assert z.abs().max().item() <= 244  # (the margin the affine epilogue and the residual need: conv_parity_util docstring)
    # f32 is exact: the float64 convolution gives the same integers (once per shape and tap order: the modes share z)
    assert _f32_equals_f64(case.shape, case.flip)


@pytest.mark.parametrize("case", P.WGRAD_CASES, ids=lambda c: c.id)
def test_lattice_filter_gradient_case_is_exact_in_f32(case):
    B, Cin, Cout, k, s, H, W = case.shape
    for layer in range(case.n):
        x, dz, g0, ref, _ = P.wgrad_operands(case.shape, True, case.dtype, layer)
        P.lattice_ok(ref, P.F32, x, dz, g0)
        # the reference formula against autograd, in float64
        wz = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wz, None, s, P.pad_of(k, s)).backward(dz.double())
        assert torch.equal(wz.grad.permute(0, 2, 3, 1) + g0.double(), ref.double())


@pytest.mark.parametrize("B,Cin,Cout,H,W,ldx,with_res,kn,kernel,class_kernel", P.D2S_CASES)
def test_lattice_stride2_data_gradient_case_is_exactly_representable(B, Cin, Cout, H, W, ldx, with_res, kn, kernel, class_kernel):
    dz, w, res, ref, v, _ = P.d2s_operands(B, Cin, Cout, H, W, True, with_res)
    P.lattice_ok(ref, P.BF16, dz, w, res)
    assert torch.equal(v.bfloat16().float(), v)
    # conv_transpose2d is the autograd backward of the forward convolution
    xz = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xz, w.double(), None, 2, 1).backward(dz.double())
    assert torch.equal(xz.grad, v.double())


def test_every_forced_knob_has_a_default_to_return_to():
    for case in P.CONV_CASES + P.WGRAD_CASES:
        assert set(case.knobs) <= set(P.KNOB_DEFAULTS), case.id
    ids = [c.id for c in P.CONV_CASES] + [c.id for c in P.WGRAD_CASES]
    assert len(ids) == len(set(ids))


# ---- 2. the plain restatement within the bound, a = 1 --------------------------------------------------------------------
def _restate(case):
    x, w, z, S = P.conv_operands(case.shape, case.flip, False, case.dtype)
    sc, sh, res = P.epilogue_operands(case, False)
    B, Cin, Cout, k, s, H, W = case.shape
    T = P.TD[case.dtype]
    flags = P.MODES[case.mode]
    v = F.conv2d(x, P.w_ref(w, case.flip), None, s, P.pad_of(k, s))
    if flags & P.AFFINE:
        v = v * sc[None, :, None, None] + sh[None, :, None, None]
    if flags & P.RELU:
        v = torch.relu(v)
    if res is not None:
        v = v.to(T).float() + res
    return v.to(T).float()


@pytest.mark.parametrize("case", [c for c in P.CONV_CASES if c.partb], ids=lambda c: c.id)
def test_restatement_is_within_the_part_b_bound(case):
    ref, _ = P.conv_reference(case, False)
    nbad, worst = P.within(_restate(case), ref, P.conv_bound(case, 1.0))
    assert nbad == 0, (nbad, worst)


@pytest.mark.parametrize("case", [c for c in P.WGRAD_CASES if c.partb], ids=lambda c: c.id)
def test_filter_gradient_restatement_is_within_the_bound(case):
    B, Cin, Cout, k, s, H, W = case.shape
    x, dz, g0, ref, S = P.wgrad_operands(case.shape, False, case.dtype, 0)
    wz = torch.zeros(Cout, Cin, k, k, requires_grad=True)
    F.conv2d(x, wz, None, s, P.pad_of(k, s)).backward(dz)
    got = wz.grad.permute(0, 2, 3, 1) + g0
    nbad, worst = P.within(got, ref, P.wgrad_bound(case.shape, case.dtype, 0, 1.0))
    assert nbad == 0, (nbad, worst)


# ---- 3. what the norm does not see ---------------------------------------------------------------------------------------
BIG = P.Conv("big", (4, 32, 32, 3, 1, 33, 17), P.BF16, "plain", ())  # 71,808 outputs (test_kernels_gpu.CONV_CASES)


def _truncate_bf16(v):
    return (v.float().view(torch.int32) & ~0xFFFF).view(torch.float32)


def _corrupt(ref, x, w, how):
    """ref: NCHW; b = 1, channel 5, pixel (16, 8): interior"""
    out = ref.clone()
    if how == "dropped_tap":      # tap (0, 2) of every input channel missing at one (pixel, channel)
        out[1, 5, 16, 8] -= (x[1, :, 16 - 1, 8 + 1] * w[5, :, 0, 2]).sum().to(out.dtype)
    elif how == "neighbour":      # one value replaced by its neighbouring pixel's
        out[1, 5, 16, 8] = ref[1, 5, 16, 9]
    return out


@pytest.mark.parametrize("how", ["dropped_tap", "neighbour"])
def test_one_wrong_element_passes_the_norm_and_fails_the_lattice_equality(how):
    assert BIG.shape[0] * BIG.shape[2] * 33 * 17 >= 50000
    # free-running inputs, stored in bf16: the corruption hides in the norm
    x, w, z, S = P.conv_operands(BIG.shape, False, False, P.BF16)
    good = z.bfloat16().double()
    bad = _corrupt(z, x.double(), w.double(), how).bfloat16().double()
    assert not torch.equal(bad, good)
    assert _rel_err(bad, z) < TOL_BF16  # the old check passes
    nbad, worst = P.within(bad, z, P.conv_bound(BIG, P.A_MFMA))
    assert nbad == 1 and worst > 10  # Part B sees it
    # lattice inputs: equality sees it
    xl, wl, zl, _ = P.conv_operands(BIG.shape, False, True, P.BF16)
    badl = _corrupt(zl, xl, wl, how)
    assert _rel_err(badl, zl) < TOL_BF16
    assert not torch.equal(badl.bfloat16().float(), zl)


def test_a_truncating_store_passes_the_norm_and_fails_the_part_b_bound():
    x, w, z, S = P.conv_operands(BIG.shape, False, False, P.BF16)
    trunc = _truncate_bf16(z.float()).double()
    assert _rel_err(trunc, z) < TOL_BF16  # the old check passes
    nbad, worst = P.within(trunc, z, P.conv_bound(BIG, P.A_MFMA))
    assert nbad > z.numel() // 10 and worst > 1.5  # up to one ulp instead of half: fails on a large share of the elements
    # ... and lattice inputs cannot see it: every lattice value is a bf16 value, truncation leaves it alone
    xl, wl, zl, _ = P.conv_operands(BIG.shape, False, True, P.BF16)
    assert torch.equal(_truncate_bf16(zl), zl)
    # round to nearest even itself is within the bound
    assert P.within(z.bfloat16().double(), z, P.conv_bound(BIG, 1.0))[0] == 0


# ---- 1b. the grouped and depthwise lattice cases ----------------------------------------------------------------------------
GROUPED = [("gconv", s) for s in P.GCONV_SHAPES] + [("dwt", s) for s in P.DWT_SHAPES] + [("dwconv", s) for s in P.DWCONV_CASES]


@pytest.mark.parametrize("kind,shape", GROUPED, ids=[k + "-" + "x".join(map(str, s)) for k, s in GROUPED])
def test_lattice_grouped_case_is_exactly_representable(kind, shape):
    c = P.grouped_operands(kind, shape)
    for dtype in (P.F32, P.BF16):
        P.grouped_ok(c, dtype)
    # f32 is exact: the f32 convolution gives the float64 integers
    B, Cc, H, W, k, s, pad, dil, groups, gw = P.grouped_geometry(kind, shape)
    assert torch.equal(F.conv2d(c["x"], c["w"], None, s, pad, dil, groups), c["z"])
