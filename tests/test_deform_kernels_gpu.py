"""vt_deform_fwd / vt_deform_bwd / vt_deform_wgrad through the C-ABI against the float64 restatement of
tests/deform_util.py (no reference fixture exists: torchvision is not installed), run on the STORED (dtype-rounded) x,
offsets, mask logits, filter and dy.  The bias is f32 in both dtypes.

Shapes (B, H, W, Cin, Cout, k, s, p, d): deform_util.KERNEL_SHAPES -- baseline; stride 2, non-square, two K-steps; dilation
with one chunk; several 16-pixel tiles with a partial last one and Cout no multiple of 16; k = 1 with K zero-padded to 32;
and a shape of whole f32 chunks only.  Offsets are N(0, 1.5^2): at least 10 % of the samples have no corner inside the map
(asserted).  Every shape runs without a mask, with an identity mask and with a sigmoid mask.

Bounds: relative L2 within gpu_util.tol(dtype) (2e-5 f32, 6e-3 bf16: the bound of tests/test_gconv_kernels_gpu.py) for y,
dx, d(offset), d(mask logit), dw and dbias; dx accumulated onto a random prior gradient within twice that (two roundings:
the rule of tests/test_layernorm_gpu.py).  Every output except dx is bit-identical between two runs; dx leaves through float
atomics and is compared by the bound in both runs.  As channel slices of NaN-filled buffers every output has the bits of
the dense run (dx: the bound) and the surroundings stay NaN; the offset / mask maps and their gradients always have a pixel
stride greater than their logical width (dense: the next whole chunk, zero padded, as the launch list holds them; sliced:
at an odd element offset of a NaN-filled buffer)."""
import pytest
import torch
import torch.nn.functional as F

import deform_util as DU
from gpu_util import TD, rel_err, rounded, stream, tol, vp
from vision_toolbox import _native as N

pytestmark = pytest.mark.gpu

CODE = {"f32": N.VT_F32, "bf16": N.VT_BF16}
CASES = [pytest.param(shape, CODE[tag], id="x".join(map(str, shape)) + "-" + tag) for shape, tags in DU.KERNEL_SHAPES for tag in tags]
MASKS = {"none": None, "identity": 0, "sigmoid": 1}
PAD, OFF = 16, 8   # x, y, dy, dx as a channel slice: pixel stride + 16, operand at element 8
SIDE_OFF = 5       # the offset / mask maps as a slice: an odd element offset


def _inputs(shape, mode, dtype, offsets=None):
    """stored inputs (NCHW, f32 holding dtype values) of one case; `offsets` overrides the N(0, 1.5^2) draw"""
    B, H, W, Ci, Co, k, s, p, d = shape
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    g = torch.Generator().manual_seed(sum(shape) + 17 * len(mode))
    x = rounded(torch.randn(B, Ci, H, W, generator=g), dtype)
    off = rounded(torch.randn(B, 2 * k * k, Ho, Wo, generator=g) * DU.OFFSET_STD, dtype) if offsets is None else offsets
    logit = rounded(torch.randn(B, k * k, Ho, Wo, generator=g), dtype) if mode != "none" else None
    w = rounded(torch.randn(Co, Ci, k, k, generator=g) / (k * k * Ci) ** 0.5, dtype)
    bias = torch.randn(Co, generator=g)
    dy = rounded(torch.randn(B, Co, Ho, Wo, generator=g), dtype)
    prior = rounded(torch.randn(B, Ci, H, W, generator=g), dtype)
    return x, off, logit, w, bias, dy, prior


def _float64(shape, mode, inputs):
    """y, dx, d(offset), d(mask logit), dw, dbias of the restatement in float64"""
    s, p, d = shape[6:]
    x, off, logit, w, bias, dy, _ = inputs
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, off, logit, w, bias)]
    x64, o64, l64, w64, b64 = leaves
    mask = None if mode == "none" else (torch.sigmoid(l64) if mode == "sigmoid" else l64)
    y = DU.deform_conv2d_ref(x64, o64, mask, w64, b64, s, p, d)
    grads = torch.autograd.grad((y * dy.double()).sum(), [t for t in leaves if t is not None])
    it = iter(grads)
    dx, do, dl, dw, db = [next(it) if t is not None else None for t in leaves]
    return dict(y=y.detach(), dx=dx, doff=do, dmask=dl, dw=dw, db=db)


_REFS = {}


def _reference(shape, mode, dtype):
    """inputs and the float64 yardstick of one case, computed once and shared (never modified)"""
    key = (shape, mode, dtype)
    if key not in _REFS:
        inputs = _inputs(shape, mode, dtype)
        _REFS[key] = (inputs, _float64(shape, mode, inputs))
    return _REFS[key]


def _dev(t_nchw, dtype, sliced=False, off=OFF, pad=PAD):
    """NCHW cpu tensor -> (buffer, NHWC operand view): dense, or a channel slice of a NaN-filled wider buffer"""
    v = t_nchw.permute(0, 2, 3, 1).contiguous().to("cuda", TD[dtype])
    if not sliced:
        return v, v
    wide = torch.full((*v.shape[:3], v.shape[3] + pad), float("nan"), device="cuda", dtype=TD[dtype])
    wide[..., off : off + v.shape[3]] = v
    return wide, wide[..., off : off + v.shape[3]]


def _side(t_nchw, dtype, sliced):
    """an offset / mask map: dense = zero padded to the next whole chunk (pixel stride > logical width), sliced = at an odd
    element offset of a NaN-filled buffer"""
    if t_nchw is None:
        return None, None
    if sliced:
        return _dev(t_nchw, dtype, True, SIDE_OFF, PAD)
    C, epc = t_nchw.shape[1], 8 if dtype == N.VT_BF16 else 4
    Cp = -(-(C + 1) // epc) * epc
    v = t_nchw.permute(0, 2, 3, 1).contiguous().to("cuda", TD[dtype])
    wide = torch.zeros((*v.shape[:3], Cp), device="cuda", dtype=TD[dtype])
    wide[..., :C] = v
    return wide, wide[..., :C]


def _nchw64(v):
    return v.double().permute(0, 3, 1, 2).cpu()


def _nan_around(wide, view):
    """everything of `wide` outside `view`'s channels is still NaN (or `wide` is the view itself)"""
    if wide.shape[-1] == view.shape[-1]:
        return True
    c0 = (view.data_ptr() - wide.data_ptr()) // wide.element_size()
    return bool(torch.isnan(wide[..., :c0]).all() and torch.isnan(wide[..., c0 + view.shape[-1]:]).all())


def _geom(shape, mode, dtype):
    B, H, W, Ci, Co, k, s, p, d = shape
    return [B, H, W, Ci, Co, k, s, p, d, MASKS[mode] or 0, dtype]


def _ld(v):
    return v.stride(2) if v is not None else 0


def _run(shape, mode, dtype, sliced=False, inputs=None):
    """every launch twice -> dict of NCHW float64 results and the buffers; asserts bit-identity of all outputs but dx"""
    B, H, W, Ci, Co, k, s, p, d = shape
    K2 = k * k
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    x, off, logit, w, bias, dy, prior = inputs if inputs is not None else _reference(shape, mode, dtype)[0]
    lib, geom = N.lib(), _geom(shape, mode, dtype)
    xw, xv = _dev(x, dtype, sliced)
    ow, ov = _side(off, dtype, sliced)
    lw, lv = _side(logit, dtype, sliced)
    gw, gv = _dev(dy, dtype, sliced)
    wd = w.permute(0, 2, 3, 1).contiguous().to("cuda", TD[dtype])
    bd = bias.cuda()
    out, bufs = {}, [(xw, xv), (ow, ov), (gw, gv)] + ([(lw, lv)] if lv is not None else [])

    ys = []
    for _ in range(2):
        yw, yv = _dev(torch.zeros(B, Co, Ho, Wo), dtype, sliced)
        if sliced:
            yv.fill_(float("nan"))
        N.check(lib.vt_deform_fwd(vp(xv), _ld(xv), vp(ov), _ld(ov), vp(lv), _ld(lv), vp(wd), vp(bd), vp(yv), _ld(yv), *geom, stream()))
        ys.append((yw, yv))
    torch.cuda.synchronize()
    assert torch.equal(ys[0][1], ys[1][1])
    out["y"] = _nchw64(ys[0][1])
    bufs.append(ys[0])

    plane = torch.full((B * H * W * Ci,), float("nan"), device="cuda")  # (cleared by the call)
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            dxw, dxv = _dev(prior, dtype, sliced)
            dow, dov = _side(torch.full_like(off, float("nan")), dtype, sliced)
            dlw, dlv = _side(torch.full_like(logit, float("nan")) if logit is not None else None, dtype, sliced)
            N.check(lib.vt_deform_bwd(vp(gv), _ld(gv), vp(xv), _ld(xv), vp(ov), _ld(ov), vp(lv), _ld(lv), vp(wd), vp(dov), _ld(dov),
                                      vp(dlv), _ld(dlv), vp(dxv), _ld(dxv), acc, vp(plane), *geom, stream()))
            runs.append(((dxw, dxv), (dow, dov), (dlw, dlv)))
        torch.cuda.synchronize()
        assert torch.equal(runs[0][1][1], runs[1][1][1])
        assert logit is None or torch.equal(runs[0][2][1], runs[1][2][1])
        out[f"dx{acc}"], out[f"dx{acc}_again"] = _nchw64(runs[0][0][1]), _nchw64(runs[1][0][1])
        if acc == 0:
            out["doff"] = _nchw64(runs[0][1][1])
            out["dmask"] = _nchw64(runs[0][2][1]) if logit is not None else None
            bufs += [runs[0][0], runs[0][1]] + ([runs[0][2]] if logit is not None else [])

    nbytes = int(lib.vt_deform_wgrad_scratch_bytes(B, H, W, Ci, Co, k, s, p, d))
    assert nbytes > 0
    scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
    dws = []
    for _ in range(2):
        dw, db = torch.zeros(Co, K2, Ci, device="cuda"), torch.zeros(Co, device="cuda")
        N.check(lib.vt_deform_wgrad(vp(gv), _ld(gv), vp(xv), _ld(xv), vp(ov), _ld(ov), vp(lv), _ld(lv), vp(dw), vp(db), vp(scratch),
                                    nbytes, *geom, stream()))
        dws.append((dw, db))
    torch.cuda.synchronize()
    assert torch.equal(dws[0][0], dws[1][0]) and torch.equal(dws[0][1], dws[1][1])
    out["dw"] = dws[0][0].view(Co, k, k, Ci).permute(0, 3, 1, 2).double().cpu()
    out["db"] = dws[0][1].double().cpu()
    return out, bufs


@pytest.mark.parametrize("mode", list(MASKS))
@pytest.mark.parametrize("shape,dtype", CASES)
def test_against_float64(shape, dtype, mode):
    (x, off, logit, w, bias, dy, prior), ref = _reference(shape, mode, dtype)
    B, H, W, Ci, Co, k, s, p, d = shape
    outside = DU.outside_fraction(off, H, W, k, s, p, d)
    assert outside >= 0.10, outside
    got, _ = _run(shape, mode, dtype)
    bound, bad = tol(dtype), []
    checks = [("y", got["y"], ref["y"], 1), ("dx", got["dx0"], ref["dx"], 1), ("dx again", got["dx0_again"], ref["dx"], 1),
              ("dx accumulated", got["dx1"], ref["dx"] + prior.double(), 2),
              ("dx accumulated again", got["dx1_again"], ref["dx"] + prior.double(), 2),
              ("doff", got["doff"], ref["doff"], 1), ("dw", got["dw"], ref["dw"], 1), ("db", got["db"], ref["db"], 1)]
    if mode != "none":
        checks.append(("dmask", got["dmask"], ref["dmask"], 1))
    for name, a, b, factor in checks:
        assert a.shape == b.shape, name
        err = rel_err(a, b)
        print(f"{shape} {mode} {name}: {err:.2e} (bound {factor * bound:.0e}); outside {outside:.2f}")
        if not err < factor * bound:
            bad.append((name, err))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["none", "sigmoid"])
@pytest.mark.parametrize("shape,dtype", CASES)
def test_channel_slices_of_nan_filled_buffers(shape, dtype, mode):
    """every map a channel slice of a wider NaN-filled buffer: the bits of the dense run (dx: the bound), surroundings still NaN"""
    ref = _reference(shape, mode, dtype)[1]
    dense, _ = _run(shape, mode, dtype)
    sliced, bufs = _run(shape, mode, dtype, sliced=True)
    for k_ in ("y", "doff", "dw", "db") + (("dmask",) if mode != "none" else ()):
        assert torch.equal(sliced[k_], dense[k_]), k_
    assert rel_err(sliced["dx0"], ref["dx"]) < tol(dtype)
    for wide, view in bufs:
        assert wide.shape[-1] > view.shape[-1] and view.stride(2) == wide.shape[-1]
        assert _nan_around(wide, view)
    assert not any(torch.isnan(sliced[k_]).any() for k_ in ("y", "dx0", "dx1", "doff"))


@pytest.mark.parametrize("shape,dtype", CASES)
def test_zero_offsets_without_a_mask_are_a_convolution(shape, dtype):
    B, H, W, Ci, Co, k, s, p, d = shape
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    inputs = _inputs(shape, "none", dtype, offsets=torch.zeros(B, 2 * k * k, Ho, Wo))
    x, _, _, w, bias, dy, _ = inputs
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    y = F.conv2d(x64, w64, b64, s, p, d)
    dx, dw, db = torch.autograd.grad((y * dy.double()).sum(), [x64, w64, b64])
    got, _ = _run(shape, "none", dtype, inputs=inputs)
    for name, a, b in (("y", got["y"], y.detach()), ("dx", got["dx0"], dx), ("dw", got["dw"], dw), ("db", got["db"], db)):
        err = rel_err(a, b)
        print(f"{shape} zero offsets {name}: {err:.2e}")
        assert err < tol(dtype), name


@pytest.mark.parametrize("shape,dtype", CASES)
def test_integer_offsets(shape, dtype):
    """sampling positions exactly on the grid: the floor cell carries the whole weight, d(offset) is the right-hand derivative"""
    B, H, W, Ci, Co, k, s, p, d = shape
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    offsets = torch.randint(-2, 3, (B, 2 * k * k, Ho, Wo), generator=torch.Generator().manual_seed(5)).float()
    inputs = _inputs(shape, "sigmoid", dtype, offsets=offsets)
    ref = _float64(shape, "sigmoid", inputs)
    got, _ = _run(shape, "sigmoid", dtype, inputs=inputs)
    for name, key in (("y", "y"), ("dx0", "dx"), ("doff", "doff"), ("dmask", "dmask"), ("dw", "dw")):
        err = rel_err(got[name], ref[key])
        print(f"{shape} integer offsets {name}: {err:.2e}")
        assert err < tol(dtype), name


@pytest.mark.parametrize("shape,dtype", CASES)
def test_all_offsets_beyond_the_map(shape, dtype):
    """no corner of any sample inside: y is the bias, dx, d(offset), d(mask) and dw are exactly zero"""
    B, H, W, Ci, Co, k, s, p, d = shape
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    inputs = _inputs(shape, "sigmoid", dtype, offsets=torch.full((B, 2 * k * k, Ho, Wo), 1000.0))  # (a bf16 value)
    bias = inputs[4]
    got, _ = _run(shape, "sigmoid", dtype, inputs=inputs)
    assert torch.equal(got["y"], rounded(bias, dtype).double().view(1, Co, 1, 1).expand(B, Co, Ho, Wo))
    for name in ("dx0", "doff", "dmask", "dw"):
        assert float(got[name].abs().max()) == 0.0, name
    assert torch.equal(got["dx1"], inputs[6].double())  # accumulate: the prior gradient, untouched
    assert rel_err(got["db"], inputs[5].double().sum((0, 2, 3))) < tol(dtype)


def test_supported_and_arguments_are_checked():
    lib = N.lib()
    assert all(lib.vt_deform_supported(k, s, 16, 24, N.VT_BF16) == 1 for k in (1, 3) for s in (1, 2))
    assert lib.vt_deform_supported(3, 1, 12, 20, N.VT_F32) == 1 and lib.vt_deform_supported(3, 1, 12, 16, N.VT_BF16) == 0
    assert lib.vt_deform_supported(5, 1, 16, 16, N.VT_BF16) == 0 and lib.vt_deform_supported(3, 3, 16, 16, N.VT_BF16) == 0
    assert lib.vt_deform_supported(3, 1, 16, 16, 7) == 0
    bf = torch.bfloat16
    x = torch.zeros(1, 6, 6, 16, device="cuda", dtype=bf)
    off = torch.zeros(1, 6, 6, 24, device="cuda", dtype=bf)
    msk = torch.zeros(1, 6, 6, 16, device="cuda", dtype=bf)
    w = torch.zeros(16, 9, 16, device="cuda", dtype=bf)
    y, dy, dx, do, dm = (torch.zeros_like(t) for t in (x, x, x, off, msk))
    plane = torch.zeros(6 * 6 * 16, device="cuda")
    dw, db = torch.zeros(16 * 9 * 16, device="cuda"), torch.zeros(16, device="cuda")
    nbytes = int(lib.vt_deform_wgrad_scratch_bytes(1, 6, 6, 16, 16, 3, 1, 1, 1))
    scratch = torch.zeros(nbytes // 4, device="cuda")

    def geom(Ci=16, Co=16, k=3, s=1, p=1, d=1, act=1, dt=N.VT_BF16):
        return [1, 6, 6, Ci, Co, k, s, p, d, act, dt]

    def fwd(xp=x, ldx=16, ldo=24, ldm=16, yp=y, mis=0, **g):
        return lib.vt_deform_fwd(x.data_ptr() + mis if xp is x else vp(xp), ldx, vp(off), ldo, vp(msk), ldm, vp(w), None, vp(yp), 16,
                                 *geom(**g), stream())

    def bwd(xp=x, ldx=16, ldo=24, ldm=16, dxp=dx, pl=plane, mis=0, **g):
        return lib.vt_deform_bwd(vp(dy), 16, x.data_ptr() + mis if xp is x else vp(xp), ldx, vp(off), ldo, vp(msk), ldm, vp(w),
                                 vp(do), 24, vp(dm), 16, vp(dxp), 16, 0, vp(pl), *geom(**g), stream())

    def wgrad(xp=x, ldx=16, ldo=24, ldm=16, nb=nbytes, mis=0, **g):
        return lib.vt_deform_wgrad(vp(dy), 16, x.data_ptr() + mis if xp is x else vp(xp), ldx, vp(off), ldo, vp(msk), ldm, vp(dw),
                                   vp(db), vp(scratch), nb, *geom(**g), stream())

    for call, name in ((fwd, "vt_deform_fwd"), (bwd, "vt_deform_bwd"), (wgrad, "vt_deform_wgrad")):
        assert call(k=5) == N.VT_ERR_UNSUPPORTED and name in N.last_error() and "kernel_size 5" in N.last_error()
        assert call(s=3) == N.VT_ERR_UNSUPPORTED and "stride 3" in N.last_error()
        assert call(act=2) == N.VT_ERR_UNSUPPORTED and "mask_act 2" in N.last_error()
        assert call(Ci=12) == N.VT_ERR_UNSUPPORTED and call(Co=12) == N.VT_ERR_UNSUPPORTED and call(dt=7) == N.VT_ERR_UNSUPPORTED
        assert call(mis=2) == N.VT_ERR_INVALID and name in N.last_error() and "misaligned" in N.last_error()
        assert call(xp=None) == N.VT_ERR_INVALID
        assert call(ldx=8) == N.VT_ERR_INVALID and "stride" in N.last_error()
        assert call(ldo=16) == N.VT_ERR_INVALID and "offset" in N.last_error()  # < 2 k^2
        assert call(ldm=8) == N.VT_ERR_INVALID and "mask" in N.last_error()  # < k^2
        assert call(p=0, d=3) == N.VT_ERR_INVALID and "smaller than the dilated kernel" in N.last_error()
    assert fwd(yp=None) == N.VT_ERR_INVALID
    assert bwd(pl=None) == N.VT_ERR_INVALID and "plane" in N.last_error()  # d(x) needs the plane
    assert wgrad(nb=nbytes - 4) == N.VT_ERR_INVALID and "scratch" in N.last_error()
    assert lib.vt_deform_wgrad_scratch_bytes(1, 6, 6, 16, 16, 5, 1, 1, 1) == -1
    N.check(fwd())
    N.check(bwd())
    N.check(bwd(dxp=None, pl=None))  # no d(x): no scatter, no plane
    N.check(wgrad())
    torch.cuda.synchronize()
