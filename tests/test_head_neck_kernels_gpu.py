"""The oldest streaming kernels of vt_elementwise.hip against float64 restatements (head_neck_util.py): the resampling
kernels of the necks (four modes, forward and backward), the classifier loss with and without the MixUp / CutMix header, the
image blend on the way into NHWC, the eval-mode BatchNorm coefficients (single and batched), and wider cases of the pooling,
ESE-gate, column-sum and 2-D copy kernels.

Every kernel runs in both dtypes, dense and as channel slices (every operand its own leading dimension and channel offset) of
NaN-filled buffers whose surroundings must stay NaN, into NaN-filled outputs that must come back finite, twice with
bit-identical results.  Bounds are elementwise, k * u * S (+ 2^-8 |ref| for a bf16 store) with the k of head_neck_util.py;
where a kernel only moves or selects values the comparison is torch.equal.  Every test prints its worst error as a fraction
of its bound ("FRAC <kernel> <dtype> <fraction>")."""
import ctypes as C

import pytest
import torch

from oracle import filler
from oracle import torch_ref as R
from vision_toolbox import _native as N

import head_neck_util as U
from gpu_util import DNAME, DTYPES, TD, stream, vp

pytestmark = pytest.mark.gpu

DT_IDS = [DNAME[d] for d in DTYPES]
SLICED = pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
NAN = float("nan")
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]

assert (N.VT_F32, N.VT_BF16) == (U.F32, U.BF16)


def _place(t: torch.Tensor, dtype: int, sliced: bool, i: int = 0):
    """cpu [..., C] -> device tensor (dense, or channels [off, off + C) of a NaN-filled buffer; operand number `i` picks
    the leading dimension and the offset, so that no two operands of a launch share them); returns (view, whole buffer)"""
    d = t.to("cuda", TD[dtype]).contiguous()
    if not sliced:
        return d, d
    epc, Cc = U.EPC[dtype], d.shape[-1]
    off, ld = epc * (1 + i % 3), Cc + epc * (4 + i)
    wide = torch.full(tuple(d.shape[:-1]) + (ld,), NAN, device="cuda", dtype=TD[dtype])
    wide[..., off:off + Cc] = d
    return wide[..., off:off + Cc], wide


def _nan_out(shape, dtype: int, sliced: bool, i: int):
    return _place(torch.full(tuple(shape), NAN), dtype, sliced, i)


def _ld(v: torch.Tensor) -> int:
    return v.shape[-1] if v.is_contiguous() else v.stride(-2)


def _outside_nan(view: torch.Tensor, wide: torch.Tensor) -> bool:
    if wide is view:
        return True
    off, Cc = view.storage_offset(), view.shape[-1]
    return bool(torch.isnan(wide[..., :off]).all() and torch.isnan(wide[..., off + Cc:]).all())


def _twice(launch):
    """launch() -> tuple of (view, buffer) outputs, run twice: slices intact, outputs finite, both runs bit-identical"""
    runs = []
    for _ in range(2):
        res = launch()
        torch.cuda.synchronize()
        for view, wide in res:
            assert _outside_nan(view, wide), "wrote outside its channel slice"
            assert bool(torch.isfinite(view).all()), "an output element was not written"
        runs.append([view.clone() for view, _ in res])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    return [t.cpu() for t in runs[0]]


def _check(kernel: str, dtype: int, got, ref, bnd):
    fr = U.frac(got, ref, bnd)
    print(f"FRAC {kernel} {DNAME[dtype]} {fr:.4f}")
    assert fr <= 1.0, (kernel, DNAME[dtype], fr)


def _exact(got: torch.Tensor, want_f32: torch.Tensor, dtype: int):
    assert torch.equal(got, want_f32.to(TD[dtype]))


# ---- 1. resampling ----------------------------------------------------------------------------------------------------
RS_GEOS = U.RESAMPLE_GEOS
RS = pytest.mark.parametrize("geo", RS_GEOS, ids=_ids(RS_GEOS))
MODES = pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["nearest_up", "nearest_down", "bilinear_up", "bilinear_down"])


def _rs_case(mode, geo, dtype):
    return U.resample_case(mode, geo, dtype, "long" if geo[:3] == U.RESAMPLE_LONG else "small")


@SLICED
@DTYPE
@RS
@MODES
def test_resample_forward(mode, geo, dtype, sliced):
    c, L = _rs_case(mode, geo, dtype), N.lib()
    (B, Hd, Wd), Cc = U.resample_shapes(mode, geo)[1], geo[3] * U.EPC[dtype]
    x, _ = _place(c["x"], dtype, sliced, 0)
    o, _ = _place(c["o"], dtype, sliced, 1)
    for other in (None, o):
        def launch():
            y = _nan_out((B, Hd, Wd, Cc), dtype, sliced, 2)
            N.check(L.vt_resample2x_add_fwd(vp(x), _ld(x), vp(other), _ld(o) if other is not None else 0, vp(y[0]), _ld(y[0]),
                                            B, Hd, Wd, Cc, mode, dtype, stream()))
            return (y,)
        got, = _twice(launch)
        ref, S = (c["y"], c["Sy"]) if other is None else (c["yo"], c["Syo"])
        if mode >= 2:
            _check(f"resample_fwd_mode{mode}", dtype, got, ref, U.bound(U.K_BILINEAR_FWD, S, ref, dtype))
        elif other is None:
            _exact(got, c["y"].float(), dtype)   # the indexed source
        else:
            _exact(got, c["y"].float() + c["o"], dtype)


@SLICED
@DTYPE
@RS
@MODES
def test_resample_backward(mode, geo, dtype, sliced):
    c, L = _rs_case(mode, geo, dtype), N.lib()
    ((_, Hs, Ws), (B, Hd, Wd)), Cc = U.resample_shapes(mode, geo), geo[3] * U.EPC[dtype]
    g, _ = _place(c["g"], dtype, sliced, 0)
    for acc in (0, 1):
        def launch():
            d = _place(c["prior"], dtype, sliced, 1) if acc else _nan_out((B, Hs, Ws, Cc), dtype, sliced, 1)
            N.check(L.vt_resample2x_bwd(vp(g), _ld(g), vp(d[0]), _ld(d[0]), B, Hd, Wd, Cc, mode, acc, dtype, stream()))
            return (d,)
        got, = _twice(launch)
        if mode == 1:
            prior = c["prior"] if acc else torch.zeros_like(c["prior"])
            _exact(got[:, 1::2], prior[:, 1::2], dtype)          # odd rows: exactly 0, or their prior value
            _exact(got[:, :, 1::2], prior[:, :, 1::2], dtype)    # odd columns
            _exact(got[:, ::2, ::2], prior[:, ::2, ::2] + c["g"], dtype)   # even positions: one exact add
        else:
            ref, S = c["d"][acc], c["Sd"][acc]
            _check(f"resample_bwd_mode{mode}", dtype, got, ref, U.bound(U.resample_bwd_k(mode), S, ref, dtype))


@pytest.mark.parametrize("mode", [0, 2])
def test_resample_odd_destination_is_refused_and_launches_nothing(mode):
    L = N.lib()
    for Hd, Wd in ((3, 4), (4, 3)):
        small = torch.full((1, 2, 2, 8), NAN, device="cuda", dtype=torch.bfloat16)
        big = torch.full((1, Hd, Wd, 8), NAN, device="cuda", dtype=torch.bfloat16)
        before = N.launch_count()
        assert L.vt_resample2x_add_fwd(vp(small), 8, None, 0, vp(big), 8, 1, Hd, Wd, 8, mode, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
        assert L.vt_resample2x_bwd(vp(big), 8, vp(small), 8, 1, Hd, Wd, 8, mode, 0, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert N.launch_count() == before
        assert bool(torch.isnan(small).all() and torch.isnan(big).all())


# the modules on non-square maps, against the float64 neck of the oracle (pinned to the reference fixtures by
# test_necks.py::test_oracle_necks_match_reference_fixtures); bounds: the f32 `ty` / `tg` of test_necks.py
NECK_SIZES = [(12, 20), (6, 10), (3, 5)]
NECKS = [("fpn", (16, 32, 64), 32, True), ("fpn", (16, 32, 64), 32, False), ("pan", (16, 24, 40), 16, True)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("neck", NECKS, ids=["fpn_td", "fpn_bu", "pan"])
def test_neck_modules_on_non_square_maps_match_the_float64_oracle(neck, interp):
    from vision_toolbox import necks

    kind, ins, outc, td = neck
    name = f"hn.{kind}{int(td)}{interp}"
    m = (necks.FPN(list(ins), outc, interpolation_mode=interp, top_down=td) if kind == "fpn"
         else necks.PAN(list(ins), outc, interpolation_mode=interp))
    filler.fill_module(m, name + ".")
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    params = {k: sd[k].requires_grad_(True) for k, _ in m.named_parameters()}
    xs = [filler.tensor(f"{name}.x{i}", (2, c, h, w)) for i, (c, (h, w)) in enumerate(zip(ins, NECK_SIZES))]
    rs = [filler.tensor(f"{name}.r{i}", (2, outc, h, w)) for i, (h, w) in enumerate(NECK_SIZES)]
    xr = [x.double().requires_grad_(True) for x in xs]
    yr = R.fpn(sd, "", xr, td, True, "sum", interp) if kind == "fpn" else R.pan(sd, "", xr, True, "sum", interp)
    sum((y * r.double()).sum() for y, r in zip(yr, rs)).backward()

    m = m.cuda().train()
    xg = [x.cuda().requires_grad_(True) for x in xs]
    before = N.launch_count()
    yg = m(xg)
    sum((y.float() * r.cuda()).sum() for y, r in zip(yg, rs)).backward()
    torch.cuda.synchronize()
    assert N.launch_count() > before, "HIP path did not run"
    ty, tg = 5e-5, 2e-4
    for i, (a, b) in enumerate(zip(yg, yr)):
        assert tuple(a.shape) == tuple(b.shape) and _rel(a.detach().cpu(), b.detach()) < ty, i
    for i, (a, b) in enumerate(zip(xg, xr)):
        assert _rel(a.grad.cpu(), b.grad) < tg, i
    for k, p in m.named_parameters():
        assert _rel(p.grad.cpu(), params[k].grad) < tg, k


# ---- 2. softmax cross entropy --------------------------------------------------------------------------------------------
def _xent(B, N_, dtype, z, y, eps, gs, header=None, with_grad=True):
    """one launch on logits with ldl = N + 3 and dlogits with lddl = N + 5 (NaN padding); returns (loss, dlogits [B, N])"""
    L, td = N.lib(), TD[dtype]
    zw = torch.full((B, N_ + 3), NAN, device="cuda", dtype=td)
    zw[:, :N_] = z.to("cuda", td)
    dw = torch.full((B, N_ + 5), NAN, device="cuda", dtype=td)
    loss = torch.zeros(1, device="cuda")
    yd = y.cuda()
    dl = vp(dw) if with_grad else None
    if header is None:
        N.check(L.vt_softmax_xent(vp(zw), N_ + 3, vp(yd), eps, gs, vp(loss), dl, N_ + 5, B, N_, dtype, stream()))
    else:
        mix = torch.tensor([float(header[0]), header[1], 0, 0, 0, 0], device="cuda", dtype=torch.float32)
        N.check(L.vt_softmax_xent_mix(vp(zw), N_ + 3, vp(yd), eps, gs, vp(loss), dl, N_ + 5, B, N_, dtype, vp(mix), stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(zw[:, N_:]).all() and torch.isnan(dw[:, N_:]).all()), "the padding was touched"
    if not with_grad:
        assert bool(torch.isnan(dw).all())
    return loss.cpu(), dw[:, :N_].cpu()


@DTYPE
@pytest.mark.parametrize("shape", U.XENT_SHAPES, ids=_ids(U.XENT_SHAPES))
def test_softmax_xent_plain_and_every_mix_header(shape, dtype):
    B, N_ = shape
    for eps in U.XENT_EPS:
        for gs in (1.0 / B, 3.0):
            plain = None
            for header in [None] + U.XENT_HEADERS:
                mode, lam = header if header is not None else (0, 1.0)
                c = U.xent_case(B, N_, dtype, mode, lam, eps)
                loss, dl = _xent(B, N_, dtype, c["z"], c["y"], eps, gs, header)
                loss2, dl2 = _xent(B, N_, dtype, c["z"], c["y"], eps, gs, header)
                assert torch.equal(dl, dl2), "two runs differ"
                assert bool(torch.isfinite(dl).all())
                if B <= 2:   # (the atomic adds of more rows may come in either order)
                    assert torch.equal(loss, loss2)
                # a relative bound on the loss needs a loss: with one class it is exactly 0, and the bound is on |z| there
                scale = abs(c["loss"]) if N_ > 1 else c["z"].abs().mean().item()
                lfrac = abs(loss.item() - c["loss"]) / (U.XENT_LOSS_REL * scale)
                print(f"FRAC xent_loss {DNAME[dtype]} {lfrac:.4f}")
                assert lfrac <= 1.0, (header, eps, gs, loss.item(), c["loss"])
                ref = c["dz_unit"] * U.f32r(gs)
                _check("xent_grad" if header is None else "xent_mix_grad", dtype, dl, ref,
                       U.XENT_R[dtype] * (c["p"] + c["q"]) * abs(gs))
                if header is None:
                    plain = (loss, dl)
                elif mode == 0:   # an inactive header is the plain kernel
                    assert torch.equal(dl, plain[1])
                    if B == 1:
                        assert torch.equal(loss, plain[0])
                    else:
                        assert loss.item() == pytest.approx(plain[0].item(), rel=1e-6)


@DTYPE
def test_softmax_xent_bad_labels_poison_the_loss_and_nothing_else(dtype):
    B, N_ = 4, 10
    z = U.vals("hn.xebad", (B, N_), dtype, 3.0)
    good = filler.labels(B, N_)
    for row, value, header in ((0, N_, None), (0, -1, (0, 1.0)), (0, N_, (1, 0.3)), (1, N_ + 5, (1, 0.3)), (1, -2, (2, 0.5))):
        y = good.clone()
        y[row] = value   # (with a mixing header a bad label in row 1 poisons rows 1 and 2: own label and partner)
        loss, dl = _xent(B, N_, dtype, z, y, 0.1, 1.0 / B, header)
        assert bool(torch.isnan(loss).all()), (row, value, header)
        assert bool(torch.isfinite(dl).all()), (row, value, header)


@DTYPE
@pytest.mark.parametrize("shape", [(2, 257), (7, 1000)], ids=_ids([(2, 257), (7, 1000)]))
def test_softmax_xent_without_a_gradient_gives_the_same_loss(shape, dtype):
    B, N_ = shape
    for header in (None, (1, 0.3)):
        c = U.xent_case(B, N_, dtype, header[0] if header else 0, header[1] if header else 1.0, 0.1)
        with_grad, _ = _xent(B, N_, dtype, c["z"], c["y"], 0.1, 1.0 / B, header)
        without, _ = _xent(B, N_, dtype, c["z"], c["y"], 0.1, 1.0 / B, header, with_grad=False)
        if B <= 2:
            assert torch.equal(with_grad, without)
        else:   # the same row losses, summed by atomics in either order
            assert without.item() == pytest.approx(with_grad.item(), rel=1e-6)


# ---- 3. MixUp / CutMix on the way into NHWC ------------------------------------------------------------------------------
def _mix(x, shape, dtype, header):
    B, Cc, H, W, Cpad = shape
    def launch():
        y = torch.full((B, H, W, Cpad), NAN, device="cuda", dtype=TD[dtype])
        mix = torch.tensor([float(v) for v in header], device="cuda", dtype=torch.float32)
        N.check(N.lib().vt_mix_nchw_to_nhwc(vp(x), vp(y), B, Cc, H, W, Cpad, dtype, vp(mix), stream()))
        return ((y, y),)
    return _twice(launch)[0]


@DTYPE
@pytest.mark.parametrize("shape", U.MIX_SHAPES, ids=_ids(U.MIX_SHAPES))
def test_mix_nchw_to_nhwc_modes_boxes_and_padding(shape, dtype):
    B, Cc, H, W, Cpad = shape
    xc = U.mix_images(shape)
    x = xc.cuda()
    plain = torch.full((B, H, W, Cpad), NAN, device="cuda", dtype=TD[dtype])
    N.check(N.lib().vt_nchw_to_nhwc(vp(x), vp(plain), B, Cc, H, W, Cpad, dtype, stream()))
    got = _mix(x, shape, dtype, (0, 0.3, 0, 0, W, H))
    assert torch.equal(got, plain.cpu())
    _exact(got, U.mix_ref(xc, 0, 1.0, (0, 0, 0, 0), Cpad)[0].float(), dtype)
    for box in U.mix_boxes(H, W):
        got = _mix(x, shape, dtype, (2, 0.5) + box)
        _exact(got, U.mix_ref(xc, 2, 0.5, box, Cpad)[0].float(), dtype)   # selected f32 pixels, rounded once
    for lam in U.MIX_LAMS:
        got = _mix(x, shape, dtype, (1, lam, 0, 0, W, H))   # (a box in the header of a MixUp step is ignored)
        ref, S = U.mix_ref(xc, 1, lam, (0, 0, 0, 0), Cpad)
        _check("mix_nchw_to_nhwc_mixup", dtype, got, ref, U.bound(U.K_MIXUP, S, ref, dtype))
        assert bool((got[..., Cc:] == 0).all()), "pad channels"


# ---- 4. eval-mode BatchNorm coefficients ---------------------------------------------------------------------------------
GUARD = 8


def _guarded(Cc):
    return torch.full((Cc + GUARD,), NAN, device="cuda")


def _bn_single(g, b, rm, rv, Cc, with_mi):
    outs = [_guarded(Cc) for _ in range(4)]
    sc, sf, mean, istd = outs
    N.check(N.lib().vt_bn_eval_coeffs(vp(g), vp(b), vp(rm), vp(rv), U.BN_EPS, Cc, vp(sc), vp(sf), vp(mean) if with_mi else None,
                                      vp(istd) if with_mi else None, stream()))
    torch.cuda.synchronize()
    return outs


def _bn_check(outs, g, b, rm, rv, Cc, with_mi):
    sc, sf, mean, istd = [t.cpu() for t in outs]
    for t in (sc, sf, mean, istd):
        assert bool(torch.isnan(t[Cc:]).all()), "guard bytes"
    scale, shift, invstd, S = U.bn_ref(g, b, rm, rv)
    _check("bn_eval_scale", N.VT_F32, sc[:Cc], scale, U.K_BN_SCALE * U.U * scale.abs())
    _check("bn_eval_shift", N.VT_F32, sf[:Cc], shift, U.K_BN_SHIFT * U.U * S)
    if with_mi:
        _check("bn_eval_invstd", N.VT_F32, istd[:Cc], invstd, U.K_BN_SCALE * U.U * invstd)
        assert torch.equal(mean[:Cc], rm)
    else:
        assert bool(torch.isnan(mean).all() and torch.isnan(istd).all())


@pytest.mark.parametrize("with_mi", [False, True], ids=["coeffs", "mean_invstd"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("Cc", U.BN_CS)
def test_bn_eval_coeffs(Cc, affine, with_mi):
    g, b, rm, rv = U.bn_inputs(Cc)
    if not affine:
        g = b = None
    dev = [t.cuda() if t is not None else None for t in (g, b, rm, rv)]
    first = _bn_single(*dev, Cc, with_mi)
    second = _bn_single(*dev, Cc, with_mi)
    for a, c in zip(first, second):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "two runs differ"
    _bn_check(first, g, b, rm, rv, Cc, with_mi)


class BnEvalItem(C.Structure):
    """vt_bn_eval_item"""

    _fields_ = [(n, C.c_void_p) for n in ("gamma", "beta", "running_mean", "running_var", "scale", "shift", "mean", "invstd")] + \
               [("C", C.c_int32), ("eps", C.c_float)]


def test_bn_eval_coeffs_batch_equals_the_single_launches():
    """41 items, one more than VT_PACK_BATCH (40): two launches.  Item 17 has 600 channels among items of 8 (three blocks
    per item, two of them idle for the narrow ones); gamma / beta and mean / invstd are absent in some items."""
    n = 41
    cycle = [8, 8, 8, 1, 8, 255, 8, 257, 8, 256]
    items = (BnEvalItem * n)()
    keep, single = [], []
    for k in range(n):
        Cc = 600 if k == 17 else 257 if k == 40 else cycle[k % len(cycle)]
        g, b, rm, rv = (t.cuda() for t in U.bn_inputs(Cc, f".b{k}"))
        if k % 3 == 0:
            g = b = None
        with_mi = k % 4 != 0
        single.append(_bn_single(g, b, rm, rv, Cc, with_mi))
        outs = [_guarded(Cc) for _ in range(4)]
        it = items[k]
        it.gamma, it.beta = (g.data_ptr(), b.data_ptr()) if g is not None else (None, None)
        it.running_mean, it.running_var, it.scale, it.shift = rm.data_ptr(), rv.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()
        it.mean, it.invstd = (outs[2].data_ptr(), outs[3].data_ptr()) if with_mi else (None, None)
        it.C, it.eps = Cc, U.BN_EPS
        keep.append((g, b, rm, rv, outs))
    before = N.launch_count()
    N.check(N.lib().vt_bn_eval_coeffs_batch(C.byref(items), n, stream()))
    torch.cuda.synchronize()
    assert N.launch_count() == before + 2
    for (g, b, rm, rv, outs), ref in zip(keep, single):
        for a, c in zip(outs, ref):   # (bit patterns: the untouched guards and absent outputs are NaN on both sides)
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# ---- 5. pooling, ESE gate, column sums, 2-D copies ---------------------------------------------------------------------
def _pool_fwd(c, shape, dtype, sliced):
    B, HW, _ = shape
    Cc, L = c["C"], N.lib()
    x, _ = _place(c["x"], dtype, sliced, 0)
    def launch():
        y = _nan_out((B, Cc), dtype, sliced, 1)
        N.check(L.vt_global_avgpool_fwd(vp(x), _ld(x), vp(y[0]), _ld(y[0]), B, HW, Cc, dtype, stream()))
        return (y,)
    got, = _twice(launch)
    _check("global_avgpool_fwd", dtype, got, c["mean"],
           U.bound(U.pool_k(Cc, dtype, HW), c["Smean"], c["mean"], dtype, U.pool_quantum(Cc, dtype, HW) / HW))


def _pool_bwd(c, shape, dtype, sliced):
    B, HW, _ = shape
    Cc, L = c["C"], N.lib()
    g, _ = _place(c["g"], dtype, sliced, 0)
    for acc in (0, 1):
        def launch():
            dx = _place(c["prior"], dtype, sliced, 1) if acc else _nan_out((B, HW, Cc), dtype, sliced, 1)
            N.check(L.vt_global_avgpool_bwd(vp(g), _ld(g), vp(dx[0]), _ld(dx[0]), B, HW, Cc, acc, dtype, stream()))
            return (dx,)
        got, = _twice(launch)
        _check("global_avgpool_bwd", dtype, got, c["pb"][acc], U.bound(U.K_POOL_BWD, c["Spb"][acc], c["pb"][acc], dtype))


def _ese_fwd(c, shape, dtype, sliced):
    B, HW, _ = shape
    Cc, L = c["C"], N.lib()
    x, _ = _place(c["x"], dtype, sliced, 0)
    s, _ = _place(c["s"], dtype, sliced, 1)
    r, _ = _place(c["r"], dtype, sliced, 2)
    for res in (None, r):
        def launch():
            y = _nan_out((B, HW, Cc), dtype, sliced, 3)
            N.check(L.vt_ese_gate_fwd(vp(x), _ld(x), vp(s), _ld(s), vp(res), _ld(r) if res is not None else 0, vp(y[0]), _ld(y[0]),
                                      B, HW, Cc, dtype, stream()))
            return (y,)
        got, = _twice(launch)
        ref, S = (c["y"], c["Sy"]) if res is not None else (c["y"] - c["r"].double(), c["Sy"] - c["r"].double().abs())
        _check("ese_gate_fwd", dtype, got, ref, U.bound(U.K_ESE, S, ref, dtype))


def _ese_bwd(c, shape, dtype, sliced):
    B, HW, _ = shape
    Cc, L = c["C"], N.lib()
    dy, _ = _place(c["dy"], dtype, sliced, 0)
    x, _ = _place(c["x"], dtype, sliced, 1)
    s, _ = _place(c["s"], dtype, sliced, 2)
    for acc in (0, 1):
        def launch():
            dx = _place(c["prior"], dtype, sliced, 3) if acc else _nan_out((B, HW, Cc), dtype, sliced, 3)
            ds = torch.full((B, Cc), NAN, device="cuda")
            N.check(L.vt_ese_gate_bwd(vp(dy), _ld(dy), vp(x), _ld(x), vp(s), _ld(s), vp(dx[0]), _ld(dx[0]), vp(ds), B, HW, Cc, acc,
                                      dtype, stream()))
            return (dx, (ds, ds))
        dx, ds = _twice(launch)
        _check("ese_gate_bwd_dx", dtype, dx, c["dx"][acc], U.bound(U.K_ESE, c["Sdx"][acc], c["dx"][acc], dtype))
        _check("ese_gate_bwd_ds", dtype, ds, c["ds"],
               U.bound(U.ese_ds_k(Cc, dtype, HW), c["Sds"], c["ds"], N.VT_F32, U.pool_quantum(Cc, dtype, HW) / 6))
        closed = c["s"].abs() >= 3   # the derivative's interval is open: exactly 0 at +-3, as F.hardsigmoid's autograd
        assert bool(closed.any()) and bool((ds[closed] == 0).all()) and bool((c["ds"][closed] == 0).all())


@SLICED
@DTYPE
@pytest.mark.parametrize("shape", U.POOL_SHAPES, ids=_ids(U.POOL_SHAPES))
def test_global_avgpool_and_ese_gate_across_column_groups(shape, dtype, sliced):
    c = U.pool_case(shape, dtype, "small")
    _pool_fwd(c, shape, dtype, sliced)
    _pool_bwd(c, shape, dtype, sliced)
    _ese_fwd(c, shape, dtype, sliced)
    _ese_bwd(c, shape, dtype, sliced)


@SLICED
@DTYPE
def test_ese_gate_forward_and_avgpool_backward_long_rowmap(dtype, sliced):
    shape = (2, U.LONG_ROWS // 2, 257)
    c = U.pool_case(shape, dtype, "long")
    _ese_fwd(c, shape, dtype, sliced)
    _pool_bwd(c, shape, dtype, sliced)


@DTYPE
@pytest.mark.parametrize("cpr", U.COLSUM_CPRS)
@pytest.mark.parametrize("M", U.COLSUM_MS)
def test_colsum_strided_rows_and_accumulation(M, cpr, dtype):
    c, Cc = U.colsum_case(M, cpr, dtype), cpr * U.EPC[dtype]
    bnd = U.colsum_k(Cc, dtype, M) * U.U * c["S"]
    for sliced in (False, True):
        a, _ = _place(c["a"], dtype, sliced, 0)
        for start in (torch.zeros(Cc), c["out0"]):
            out = torch.full((Cc + GUARD,), NAN, device="cuda")
            out[:Cc] = start.cuda()
            N.check(N.lib().vt_colsum(vp(a), _ld(a), M, Cc, dtype, vp(out), stream()))
            torch.cuda.synchronize()
            assert bool(torch.isnan(out[Cc:]).all())
            ref = c["ref"] - c["out0"].double() + start.double()
            _check("colsum", dtype, out[:Cc].cpu(), ref, bnd)   # (the bound with |out0| in S holds for both starts)


@pytest.mark.parametrize("shape", U.COPY_SHAPES, ids=_ids(U.COPY_SHAPES))
@pytest.mark.parametrize("dst_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("src_dtype", DTYPES, ids=DT_IDS)
def test_copy2d_every_dtype_pair(src_dtype, dst_dtype, shape):
    rows, cols = shape
    lds, ldd = cols + 3, cols + 5
    src = U.vals(f"hn.cp{rows}x{cols}s", shape, src_dtype)
    old = U.vals(f"hn.cp{rows}x{cols}d", shape, dst_dtype)
    sw = torch.full((rows, lds), NAN, device="cuda", dtype=TD[src_dtype])
    sw[:, :cols] = src.cuda()
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            dw = torch.full((rows, ldd), NAN, device="cuda", dtype=TD[dst_dtype])
            if acc:
                dw[:, :cols] = old.cuda()
            N.check(N.lib().vt_copy2d(vp(sw), src_dtype, lds, vp(dw), dst_dtype, ldd, rows, cols, acc, stream()))
            torch.cuda.synchronize()
            assert bool(torch.isnan(dw[:, cols:]).all())
            runs.append(dw[:, :cols].cpu())
        assert torch.equal(*runs)
        _exact(runs[0], src + old if acc else src, dst_dtype)


def test_copy2d_refuses_an_unknown_dtype():
    t = torch.zeros(4, 4, device="cuda")
    before = N.launch_count()
    for pair in ((7, N.VT_F32), (N.VT_F32, 7), (N.VT_I64, N.VT_BF16)):
        assert N.lib().vt_copy2d(vp(t), pair[0], 4, vp(t), pair[1], 4, 4, 4, 0, stream()) == N.VT_ERR_UNSUPPORTED
    assert N.launch_count() == before
