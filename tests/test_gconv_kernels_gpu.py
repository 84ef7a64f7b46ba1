"""vt_gconv.hip against float64 torch: the one-launch grouped 3x3 convolution (forward with batch statistics, data gradient,
filter gradient) against F.conv2d(groups=...) and its autograd, and the Squeeze-Excitation MLP against plain matrix
products, all on storage-rounded operands.

Every case is launched twice and must be bit-identical (no float atomics), and runs once dense and once as a channel slice
of a wider NaN-filled buffer whose surroundings must stay NaN.  Bounds: relative L2 within gpu_util.tol(dtype) -- 2e-5 for
the exact-f32 instantiation, which pins the index maps, 6e-3 for bf16 -- for z, the statistics, dx and dw.  The reference
of a (shape, dtype) is computed once and shared."""
import pytest
import torch
import torch.nn.functional as F

from oracle import filler
from vision_toolbox import _native as N

from gpu_util import DNAME, DTYPES, TD, krsc, nhwc, rel_err, rounded, stream, to_nchw, tol, vp

pytestmark = pytest.mark.gpu

# (B, H, W, C, gw, stride): a map smaller than any tile; non-square with odd extents under stride 2; an even extent, where
# the far padding row is never read; one 48-wide and one 56-wide group width (masked rows of the last 16-row tile); 13 groups
# (no multiple of the four waves of a workgroup); several pixel tiles and several filter-gradient slabs
SHAPES = [(2, 7, 7, 16, 8, 1), (3, 13, 11, 48, 16, 1), (3, 13, 11, 48, 16, 2), (2, 14, 14, 72, 24, 2), (1, 20, 20, 96, 48, 1),
          (2, 8, 8, 112, 56, 2), (2, 10, 10, 104, 8, 1), (4, 28, 28, 32, 16, 1)]
SE_SHAPES = [(3, 48, 8), (2, 104, 12), (4, 208, 26), (2, 440, 110), (2, 896, 224)]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
DT_IDS = [DNAME[d] for d in DTYPES]
_CASES: dict = {}


def _case(shape, dtype):
    key = (shape, dtype)
    if key not in _CASES:
        B, H, W, Cc, gw, s = shape
        tag = "gconv" + "x".join(map(str, shape))
        x = rounded(filler.tensor(tag + "x", (B, Cc, H, W)), dtype)
        w = rounded(filler.tensor(tag + "w", (Cc, gw, 3, 3)) * (2.0 / (9 * gw)) ** 0.5, dtype)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        z = F.conv2d(xd, wd, None, s, 1, 1, Cc // gw)
        dz = rounded(filler.tensor(tag + "dz", tuple(z.shape)), dtype)
        z.backward(dz.double())
        zs = rounded(z.detach().float(), dtype).double()  # the statistics are those of the STORED z
        _CASES[key] = dict(x=x, w=w, dz=dz, z=z.detach(), dx=xd.grad, dw=wd.grad.permute(0, 2, 3, 1).contiguous(),
                           stats=torch.stack([zs.sum((0, 2, 3)), (zs * zs).sum((0, 2, 3))]))
    return _CASES[key]


def _dev(t, dtype, sliced):
    """NCHW cpu tensor -> device NHWC (dense, or channels [8, 8 + C) of a NaN-filled buffer 16 channels wider)"""
    return nhwc(t, dtype, t.shape[1] + 16, 8) if sliced else nhwc(t, dtype)


def _out(B, H, W, Cc, dtype, sliced):
    wide = torch.full((B, H, W, Cc + 16 if sliced else Cc), float("nan"), device="cuda", dtype=TD[dtype])
    return wide, (wide[..., 8:8 + Cc] if sliced else wide)


def _surroundings_nan(wide, Cc, sliced):
    return (not sliced) or bool(torch.isnan(wide[..., :8]).all() and torch.isnan(wide[..., 8 + Cc:]).all())


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_grouped_conv_forward_statistics_dgrad_wgrad(shape, dtype, sliced):
    before = N.launch_count()
    B, H, W, Cc, gw, s = shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    c, lib, bound = _case(shape, dtype), N.lib(), tol(dtype)
    x, dz, w = _dev(c["x"], dtype, sliced), _dev(c["dz"], dtype, sliced), krsc(c["w"], dtype)
    assert tuple(c["z"].shape) == (B, Cc, Ho, Wo)
    geo = (B, H, W, Cc, gw, s, dtype)

    runs = []
    for _ in range(2):
        zw, z = _out(B, Ho, Wo, Cc, dtype, sliced)
        st = N.stats_buffer(Cc)
        N.check(lib.vt_gconv3_fwd(vp(x), x.stride(2), vp(w), vp(z), z.stride(2), vp(st), *geo, stream()))
        dxw, dx = _out(B, H, W, Cc, dtype, sliced)
        N.check(lib.vt_gconv3_dgrad(vp(dz), dz.stride(2), vp(w), vp(dx), dx.stride(2), None, 0, *geo, stream()))
        nbytes = lib.vt_gconv3_wgrad_scratch_bytes(B, H, W, Cc, gw, s)
        assert nbytes > 0
        scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
        dw = torch.zeros(Cc, 3, 3, gw, device="cuda")
        N.check(lib.vt_gconv3_wgrad(vp(x), x.stride(2), vp(dz), dz.stride(2), vp(dw), vp(scratch), nbytes, *geo, stream()))
        torch.cuda.synchronize()
        assert _surroundings_nan(zw, Cc, sliced) and _surroundings_nan(dxw, Cc, sliced), "wrote outside its channel slice"
        runs.append((z.clone(), N.stats_decode(st).cpu(), dx.clone(), dw.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    z, st, dx, dw = runs[0]
    errs = dict(z=rel_err(to_nchw(z), c["z"]), sum=rel_err(st[0], c["stats"][0]), sumsq=rel_err(st[1], c["stats"][1]),
                dx=rel_err(to_nchw(dx), c["dx"]), dw=rel_err(dw.cpu(), c["dw"]))
    print(shape, DNAME[dtype], "slice" if sliced else "dense", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < bound, (k, v, bound)
    assert N.launch_count() >= before + 8


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dgrad_adds_a_residual_that_aliases_dx(dtype):
    shape = SHAPES[2]
    B, H, W, Cc, gw, s = shape
    c, lib = _case(shape, dtype), N.lib()
    r = rounded(filler.tensor("gconv.res", (B, Cc, H, W)), dtype)
    dz, w, dx = nhwc(c["dz"], dtype), krsc(c["w"], dtype), nhwc(r, dtype)
    N.check(lib.vt_gconv3_dgrad(vp(dz), Cc, vp(w), vp(dx), Cc, vp(dx), Cc, B, H, W, Cc, gw, s, dtype, stream()))
    torch.cuda.synchronize()
    assert rel_err(to_nchw(dx), c["dx"] + r.double()) < tol(dtype)


def test_group_widths_outside_the_range_are_refused_with_a_message():
    lib = N.lib()
    t = torch.zeros(1, 4, 4, 144, device="cuda", dtype=torch.bfloat16)
    for gw in (4, 12, 72):
        rc = lib.vt_gconv3_fwd(vp(t), 144, vp(t), vp(t), 144, None, 1, 4, 4, 144, gw, 1, N.VT_BF16, stream())
        assert rc == N.VT_ERR_UNSUPPORTED
        with pytest.raises(RuntimeError, match="group width"):
            N.check(rc)
    assert lib.vt_gconv3_fwd(vp(t), 144, vp(t), vp(t), 144, None, 1, 4, 4, 144, 16, 3, N.VT_BF16, stream()) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_gconv3_wgrad_scratch_bytes(1, 4, 4, 144, 72, 1) < 0


# ---- the Squeeze-Excitation MLP -----------------------------------------------------------------------------------------
def _se_case(shape, dtype):
    key = ("se", shape, dtype)
    if key not in _CASES:
        B, Cc, S = shape
        tag = "semlp" + "x".join(map(str, shape))
        p = rounded(filler.tensor(tag + "p", (B, Cc)).abs(), dtype)
        w1 = rounded(filler.tensor(tag + "w1", (S, Cc)) * Cc ** -0.5 * 2, dtype)
        w2 = rounded(filler.tensor(tag + "w2", (Cc, S)) * S ** -0.5 * 2, dtype)
        b1, b2 = filler.tensor(tag + "b1", (S,)) * 0.2, filler.tensor(tag + "b2", (Cc,)) * 0.2
        dl = rounded(filler.tensor(tag + "dl", (B, Cc)), dtype)
        leaves = [t.double().requires_grad_(True) for t in (p, w1, b1, w2, b2)]
        pd, w1d, b1d, w2d, b2d = leaves
        h = torch.relu(pd @ w1d.t() + b1d)
        logits = h @ w2d.t() + b2d
        logits.backward(dl.double())
        assert 0.2 < (h > 0).double().mean() < 0.95, "the case exercises both sides of the ReLU"
        _CASES[key] = dict(p=p, w1=w1, b1=b1, w2=w2, b2=b2, dl=dl, h=h.detach(), logits=logits.detach(),
                           grads=[t.grad for t in leaves])
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SE_SHAPES, ids=_ids(SE_SHAPES))
def test_se_mlp_forward_and_backward(shape, dtype):
    before = N.launch_count()
    B, Cc, S = shape
    c, lib, td, bound = _se_case(shape, dtype), N.lib(), TD[dtype], tol(dtype)
    p, dl = c["p"].to("cuda", td), c["dl"].to("cuda", td)
    w1, b1, w2, b2 = (c[k].cuda() for k in ("w1", "b1", "w2", "b2"))
    runs = []
    for _ in range(2):
        hid = torch.full((B, S), float("nan"), device="cuda")
        logits = torch.full((B, Cc), float("nan"), device="cuda", dtype=td)
        N.check(lib.vt_se_mlp_fwd(vp(p), Cc, vp(w1), vp(b1), vp(w2), vp(b2), vp(hid), vp(logits), Cc, B, Cc, S, dtype, stream()))
        dhid = torch.full((B, S), float("nan"), device="cuda")
        dp = torch.full((B, Cc), float("nan"), device="cuda", dtype=td)
        grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
        N.check(lib.vt_se_mlp_bwd(vp(dl), Cc, vp(p), Cc, vp(w1), vp(w2), vp(hid), vp(dhid), vp(dp), Cc, *[vp(g) for g in grads],
                                  B, Cc, S, dtype, stream()))
        torch.cuda.synchronize()
        runs.append([hid, logits, dp, *grads])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    hid, logits, dp, dw1, db1, dw2, db2 = [t.float().cpu() for t in runs[0]]
    want = c["grads"]
    errs = dict(hidden=rel_err(hid, c["h"]), logits=rel_err(logits, c["logits"]), dp=rel_err(dp, want[0]), dw1=rel_err(dw1, want[1]),
                db1=rel_err(db1, want[2]), dw2=rel_err(dw2, want[3]), db2=rel_err(db2, want[4]))
    print(shape, DNAME[dtype], {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < bound, (k, v, bound)
    assert N.launch_count() >= before + 6
