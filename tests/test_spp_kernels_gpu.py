"""vt_spp_fwd / vt_spp_bwd through the C-ABI against torch on the CPU in float64, run on the same stored (dtype-rounded)
inputs: the cascade of F.max_pool2d / F.avg_pool2d(k, 1, (k-1)/2), their concat, and its autograd.

Shapes (B, H, W, C, k, repeats): (1, 4, 5, 8, 5, 3) a map smaller than k; (2, 7, 7, 16, 5, 3) smaller than the 13-window;
(2, 13, 11, 24, 5, 3) odd, non-square, three chunks; (1, 20, 20, 64, 5, 3) crosses tile borders in both directions (tiles
are at most 16 pixels a side, balanced over the map: 2 x 10 here, 3 x 11 and 2 x 9 for 33 x 17) and holds more chunks than one
slab; (1, 33, 17, 8, 3, 4); (1, 18, 18, 16, 9, 2); (2, 9, 9, 32, 13, 1); (1, 9, 10, 8, 5, 4), four stages at the largest
halo; (1, 12, 12, 8, 11, 1) and (1, 12, 12, 8, 15, 1), the windows that run on the run-time-k instantiation, the second with
the largest tap a byte has to hold (14 * 15 + 14 = 224); (1, 16, 16, 8, 9, 2), a full 16 x 16 tile at halo 8: the largest LDS
plan (32 x 32 pixels, 72 KB in the bf16 backward -- over the slab budget at one chunk and over the 64 KB default limit of
dynamic LDS).  Both dtypes, both pools.  Inputs are relu(randn) rounded to bf16 in both dtypes, so that ties abound.

Bounds: max forward torch.equal.  avg forward gpu_util.tol (2e-5 f32, 6e-3 bf16, relative L2): bf16 against the float64
cascade with gpu_util.rounded between stages (the kernel's stage s+1 reads the stored values of stage s), f32 against the
plain float64 cascade.  dx within tol of float64 autograd, twice tol with accumulate = 1 onto a random prior gradient (two
roundings: the rule of tests/test_layernorm_gpu.py).  The tie rule on its own: a constant map, dx EQUAL to torch's.  Every
launch run twice is bit-identical."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import TD, rel_err, rounded, stream, tol, vp
from vision_toolbox import _native as N

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 5, 8, 5, 3), (2, 7, 7, 16, 5, 3), (2, 13, 11, 24, 5, 3), (1, 20, 20, 64, 5, 3), (1, 33, 17, 8, 3, 4),
          (1, 18, 18, 16, 9, 2), (2, 9, 9, 32, 13, 1), (1, 9, 10, 8, 5, 4), (1, 12, 12, 8, 11, 1), (1, 12, 12, 8, 15, 1),
          (1, 16, 16, 8, 9, 2)]
POOLS = {"max": 0, "avg": 1}
PAD, OFF = 16, 8  # a channel slice: pixel stride + 16, operand at element 8


def _pool(t, k, pool):
    return F.max_pool2d(t, k, 1, (k - 1) // 2) if pool == 0 else F.avg_pool2d(t, k, 1, (k - 1) // 2)


def _cascade(x_nchw, k, repeats, pool, between=None):
    """[p_1 .. p_repeats] of an NCHW tensor; `between` is applied to every stage's output before the next stage reads it"""
    outs, t = [], x_nchw
    for _ in range(repeats):
        t = _pool(t, k, pool)
        if between is not None:
            t = between(t)
        outs.append(t)
    return outs


_REFS = {}


def _reference(shape, pool, dtype):
    """inputs and the float64 yardstick of one (shape, pool, dtype), computed once and shared (never modified)"""
    key = (shape, pool, dtype)
    if key not in _REFS:
        B, H, W, C, k, repeats = shape
        g = torch.Generator().manual_seed(sum(shape) + 131 * pool)
        x = torch.relu(torch.randn(B, C, H, W, generator=g)).to(torch.bfloat16).float()  # bf16 values in both dtypes
        dy = rounded(torch.randn(B, repeats * C, H, W, generator=g), dtype)
        prior = rounded(torch.randn(B, C, H, W, generator=g), dtype)
        x64 = x.double().requires_grad_(True)
        y64 = torch.cat(_cascade(x64, k, repeats, pool), 1)
        (y64 * dy.double()).sum().backward()
        y_staged = None
        if pool == 1 and dtype == N.VT_BF16:
            y_staged = torch.cat(_cascade(x.double(), k, repeats, pool, between=lambda t: rounded(t, dtype).double()), 1)
        _REFS[key] = (x, dy, prior, y64.detach(), x64.grad, y_staged)
    return _REFS[key]


def _dev(t_nchw, dtype, sliced=False):
    """NCHW cpu tensor -> (buffer, NHWC operand view) on the device: dense, or a channel slice of a NaN-filled wider buffer"""
    v = t_nchw.permute(0, 2, 3, 1).contiguous().to("cuda", TD[dtype])
    if not sliced:
        return v, v
    wide = torch.full((*v.shape[:3], v.shape[3] + PAD), float("nan"), device="cuda", dtype=TD[dtype])
    wide[..., OFF : OFF + v.shape[3]] = v
    return wide, wide[..., OFF : OFF + v.shape[3]]


def _nchw64(v):
    return v.double().permute(0, 3, 1, 2).cpu()


def _surroundings_stay_nan(wide, C):
    return wide.shape[-1] == C or bool(torch.isnan(wide[..., :OFF]).all() and torch.isnan(wide[..., OFF + C :]).all())


def _fwd(x, y, taps, shape, pool, dtype):
    B, H, W, C, k, repeats = shape
    return N.lib().vt_spp_fwd(vp(x), x.stride(2), vp(y), y.stride(2), vp(taps), B, H, W, C, k, repeats, pool, dtype, stream())


def _bwd(dy, taps, dx, acc, shape, pool, dtype):
    B, H, W, C, k, repeats = shape
    return N.lib().vt_spp_bwd(vp(dy), dy.stride(2), vp(taps), vp(dx), dx.stride(2), acc, B, H, W, C, k, repeats, pool, dtype,
                              stream())


def _run(shape, pool, dtype, sliced=False):
    """forward twice, backward with accumulate 0 and 1 twice each -> (buffers, y, taps, {acc: dx}); asserts bit-identity"""
    B, H, W, C, k, repeats = shape
    x, dy, prior, *_ = _reference(shape, pool, dtype)
    xw, xv = _dev(x, dtype, sliced)
    gw, gv = _dev(dy, dtype, sliced)
    ys, tapss = [], []
    for _ in range(2):
        yw, yv = _dev(torch.zeros(B, repeats * C, H, W), dtype, sliced)
        taps = torch.full((repeats, B, H, W, C), 255, dtype=torch.uint8, device="cuda") if pool == 0 else None
        N.check(_fwd(xv, yv, taps, shape, pool, dtype))
        ys.append((yw, yv))
        tapss.append(taps)
    torch.cuda.synchronize()
    assert torch.equal(ys[0][1], ys[1][1]) and (pool == 1 or torch.equal(tapss[0], tapss[1]))
    dxs, bufs = {}, [xw, gw, ys[0][0]]
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            dw, dv = _dev(prior, dtype, sliced)
            N.check(_bwd(gv, tapss[0], dv, acc, shape, pool, dtype))
            runs.append((dw, dv))
        torch.cuda.synchronize()
        assert torch.equal(runs[0][1], runs[1][1]), acc
        dxs[acc] = runs[0][1]
        bufs.append(runs[0][0])
    return bufs, ys[0][1], tapss[0], dxs


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pool", sorted(POOLS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spp_matches_torch_float64(shape, pool, dtype):
    B, H, W, C, k, repeats = shape
    code, t_ = POOLS[pool], tol(dtype)
    x, dy, prior, y64, dx64, y_staged = _reference(shape, code, dtype)
    _, y, taps, dxs = _run(shape, code, dtype)
    got = _nchw64(y)
    if code == 0:
        assert torch.equal(got, y64)
        assert int(taps.max()) < k * k
    else:
        want = y_staged if y_staged is not None else y64
        err = rel_err(got, want)
        print(f"{shape} {pool} {dtype}: y rel {err:.2e} (bound {t_:.0e})")
        assert err < t_
    e0, e1 = rel_err(_nchw64(dxs[0]), dx64), rel_err(_nchw64(dxs[1]), dx64 + prior.double())
    print(f"{shape} {pool} {dtype}: dx rel {e0:.2e} (bound {t_:.0e}), accumulated {e1:.2e} (bound {2 * t_:.0e})")
    assert e0 < t_ and e1 < 2 * t_


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_taps_point_at_the_first_maximum(dtype):
    """every tap, decoded, is the first maximum of its clipped window in row-major order (checked against a direct scan)"""
    shape = (2, 7, 7, 16, 5, 3)
    B, H, W, C, k, repeats = shape
    x = _reference(shape, 0, dtype)[0]
    _, y, taps, _ = _run(shape, 0, dtype)
    h = (k - 1) // 2
    stage_in = x.double()
    t = taps.cpu().permute(0, 1, 4, 2, 3).long()  # [repeats][B][C][H][W]
    for s in range(repeats):
        padded = F.pad(stage_in, (h, h, h, h), value=float("-inf"))
        win = padded.unfold(2, k, 1).unfold(3, k, 1).reshape(B, C, H, W, k * k)
        first = (win == win.max(-1, keepdim=True).values).long().argmax(-1)  # argmax of a 0/1 tensor: the first 1
        assert torch.equal(t[s], first), s
        stage_in = win.max(-1).values


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_tie_rule_on_a_constant_map(dtype):
    """a constant 7 x 7 map, dy all ones, max, k = 5, repeats = 3: the whole gradient of an output goes to the first element of
    its clipped window.  The values are small integers, exact in bf16: dx must EQUAL torch's."""
    shape = (1, 7, 7, 8, 5, 3)
    B, H, W, C, k, repeats = shape
    x = torch.full((B, C, H, W), 0.5)
    x64 = x.double().requires_grad_(True)
    torch.cat(_cascade(x64, k, repeats, 0), 1).sum().backward()
    assert x64.grad.max() > 9 and (x64.grad == x64.grad.round()).all()
    _, xv = _dev(x, dtype)
    _, yv = _dev(torch.zeros(B, repeats * C, H, W), dtype)
    _, gv = _dev(torch.ones(B, repeats * C, H, W), dtype)
    _, dv = _dev(torch.zeros(B, C, H, W), dtype)
    taps = torch.empty(repeats, B, H, W, C, dtype=torch.uint8, device="cuda")
    N.check(_fwd(xv, yv, taps, shape, 0, dtype))
    N.check(_bwd(gv, taps, dv, 0, shape, 0, dtype))
    torch.cuda.synchronize()
    assert torch.equal(_nchw64(dv), x64.grad)
    # one 5 x 5 stage over an all-zero 6 x 6 map: 9 in the corner, 3 along the first row and column, 1 inside the first window
    shape1 = (1, 6, 6, 8, 5, 1)
    _, xv = _dev(torch.zeros(1, 8, 6, 6), dtype)
    _, yv = _dev(torch.zeros(1, 8, 6, 6), dtype)
    _, gv = _dev(torch.ones(1, 8, 6, 6), dtype)
    _, dv = _dev(torch.zeros(1, 8, 6, 6), dtype)
    taps = torch.empty(1, 1, 6, 6, 8, dtype=torch.uint8, device="cuda")
    N.check(_fwd(xv, yv, taps, shape1, 0, dtype))
    N.check(_bwd(gv, taps, dv, 0, shape1, 0, dtype))
    torch.cuda.synchronize()
    d = _nchw64(dv)[0, 0]
    want = torch.tensor([[9, 3, 3, 3, 0, 0], [3, 1, 1, 1, 0, 0], [3, 1, 1, 1, 0, 0], [3, 1, 1, 1, 0, 0], [0] * 6, [0] * 6],
                        dtype=torch.float64)
    assert torch.equal(d, want)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pool", sorted(POOLS))
def test_channel_slices_of_nan_filled_buffers(pool, dtype):
    """x, y, dy and dx as channel slices of wider NaN-filled buffers (ld > C): the same bits as dense, surroundings still NaN"""
    shape = (2, 13, 11, 24, 5, 3)
    C, repeats, code = shape[3], shape[5], POOLS[pool]
    _, y, taps, dxs = _run(shape, code, dtype)
    bufs, ys, tapss, dxss = _run(shape, code, dtype, sliced=True)
    assert ys.stride(2) == repeats * C + PAD and dxss[0].stride(2) == C + PAD
    assert torch.equal(ys, y) and torch.equal(dxss[0], dxs[0]) and torch.equal(dxss[1], dxs[1])
    assert code == 1 or torch.equal(tapss, taps)
    xw, gw, yw, d0, d1 = bufs
    assert _surroundings_stay_nan(xw, C) and _surroundings_stay_nan(d0, C) and _surroundings_stay_nan(d1, C)
    assert _surroundings_stay_nan(gw, repeats * C) and _surroundings_stay_nan(yw, repeats * C)


def test_inference_launch_takes_no_taps():
    shape = (1, 20, 20, 64, 5, 3)
    x = _reference(shape, 0, N.VT_BF16)[0]
    _, xv = _dev(x, N.VT_BF16)
    _, yv = _dev(torch.zeros(1, 192, 20, 20), N.VT_BF16)
    N.check(_fwd(xv, yv, None, shape, 0, N.VT_BF16))
    torch.cuda.synchronize()
    assert torch.equal(_nchw64(yv), _reference(shape, 0, N.VT_BF16)[3])


def test_arguments_are_checked():
    lib = N.lib()
    x = torch.zeros(1, 6, 6, 16, device="cuda", dtype=torch.bfloat16)
    y = torch.zeros(1, 6, 6, 48, device="cuda", dtype=torch.bfloat16)
    d = torch.zeros_like(x)
    taps = torch.zeros(3, 1, 6, 6, 16, dtype=torch.uint8, device="cuda")

    def fwd(xp=x, ldx=16, yp=y, ldy=48, tp=taps, C=16, k=5, r=3, pool=0, dt=N.VT_BF16, off=0):
        return lib.vt_spp_fwd(x.data_ptr() + off if xp is x else vp(xp), ldx, vp(yp), ldy, vp(tp), 1, 6, 6, C, k, r, pool, dt, stream())

    def bwd(gp=y, ldg=48, tp=taps, dp=d, ldd=16, C=16, k=5, r=3, pool=0, dt=N.VT_BF16, off=0):
        return lib.vt_spp_bwd(vp(gp), ldg, vp(tp), d.data_ptr() + off if dp is d else vp(dp), ldd, 0, 1, 6, 6, C, k, r, pool, dt,
                              stream())

    for call, name in ((fwd, "vt_spp_fwd"), (bwd, "vt_spp_bwd")):
        assert call(k=4) == N.VT_ERR_UNSUPPORTED and name in N.last_error() and "k=4" in N.last_error()  # even k
        for k, r in ((11, 2), (7, 3), (5, 5), (5, 0), (1, 1), (17, 1)):  # (17: a tap 16*17+16 does not fit a byte)
            assert call(k=k, r=r) == N.VT_ERR_UNSUPPORTED and name in N.last_error(), (k, r)
        assert call(C=12) == N.VT_ERR_UNSUPPORTED and call(dt=7) == N.VT_ERR_UNSUPPORTED and call(pool=2) == N.VT_ERR_UNSUPPORTED
        assert call(off=2) == N.VT_ERR_INVALID and name in N.last_error() and "misaligned" in N.last_error()
    assert fwd(ldx=8) == N.VT_ERR_INVALID and "vt_spp_fwd" in N.last_error() and "stride" in N.last_error()  # ld < C
    assert fwd(ldy=40) == N.VT_ERR_INVALID and fwd(yp=None) == N.VT_ERR_INVALID  # ldy < repeats * C
    assert bwd(ldd=8) == N.VT_ERR_INVALID and "vt_spp_bwd" in N.last_error() and "stride" in N.last_error()
    assert bwd(ldg=40) == N.VT_ERR_INVALID and bwd(tp=None) == N.VT_ERR_INVALID  # max needs the taps
    N.check(fwd())
    N.check(bwd())
    N.check(fwd(tp=None))  # inference: no taps
    N.check(fwd(pool=1, tp=None))
    N.check(bwd(pool=1, tp=None))  # avg ignores them
    torch.cuda.synchronize()
