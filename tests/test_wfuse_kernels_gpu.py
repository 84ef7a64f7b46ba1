"""vt_wfuse_fwd / vt_wfuse_bwd / vt_wfuse_finalize through the C-ABI against float64 torch on the stored operands.

Shapes (B, H, W, C), the smallest that cross a boundary: (1, 2, 2, 8) an x2 source of one pixel; (3, 6, 10, 24) non-square,
a chunk count that is no power of two; (2, 14, 14, 64) several workgroups; (2, 5, 7, 88) an odd output grid with an x0.5
source (partial 2x2 blocks in backward).  Code sets (0, 1), (0, 0, 2), (0, 2) and (0, 0, 0) (the bilinear route); each dense and
as a channel slice of a NaN-filled wider buffer whose surroundings must stay NaN.  Weights: all ones, a negative entry, a zero
entry, all non-positive (then out, every input gradient and d w are exactly 0).  accumulate 0 and 1 for every input.

Bounds: (a) gpu_util.tol (2e-5 f32, 6e-3 bf16, relative L2) for out and the input gradients, twice that where accumulate = 1
adds a second rounding (the rule tests/test_layernorm_gpu.py uses with a residual); (b) |d w_i - ref| <= 4e-6 S_i in both
dtypes, S_i = sum |g| (|R_i(x_i)| + |out|) / (sum + eps): each f32 term carries a few ulp of |g| (|x| + |out|), a per-thread
f32 partial of at most 32 terms adds 32 * 2^-24 = 1.9e-6 of the sum of magnitudes, the double fold and the fixed-point
hand-over add nothing visible.  Every launch run twice is bit-identical."""
import pytest
import torch

from gpu_util import TD, rel_err, stream, tol, vp
from vision_toolbox import _native as N

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(1e-4, dtype=torch.float32))
SHAPES = [(1, 2, 2, 8), (3, 6, 10, 24), (2, 14, 14, 64), (2, 5, 7, 88)]
CODES = [(0, 1), (0, 0, 2), (0, 2), (0, 0, 0)]
GEOM = [(s, c) for s in SHAPES for c in CODES if not (1 in c and (s[1] % 2 or s[2] % 2))]
WEIGHTS = {2: [(1.0, 1.0), (1.25, -0.5), (0.0, 0.75), (-0.25, 0.0)],
           3: [(1.0, 1.0, 1.0), (0.5, -0.5, 1.5), (0.75, 0.0, 1.25), (-1.0, 0.0, -0.5)]}
PAD, OFF = 16, 8  # a channel slice: pixel stride C + 16, operand at element 8


def _map(shape, td, sliced, fill="randn"):
    """(the buffer, the operand view): dense, or a channel slice of a NaN-filled wider buffer"""
    v = (torch.randn(*shape, device="cuda") if fill == "randn" else torch.zeros(*shape, device="cuda")).to(td)
    if not sliced:
        return v, v
    wide = torch.full((*shape[:3], shape[3] + PAD), float("nan"), device="cuda", dtype=td)
    wide[..., OFF : OFF + shape[3]] = v
    return wide, wide[..., OFF : OFF + shape[3]]


def _surroundings_stay_nan(wide, C):
    return wide.shape[-1] == C or bool(torch.isnan(wide[..., :OFF]).all() and torch.isnan(wide[..., OFF + C :]).all())


def _src_shape(shape, code):
    B, H, W, C = shape
    return (B, H, W, C) if code == 0 else ((B, H // 2, W // 2, C) if code == 1 else (B, 2 * H, 2 * W, C))


def _resample(x, code):
    if code == 1:
        return x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return x[:, ::2, ::2] if code == 2 else x


def _resample_t(g, code):
    B, H, W, C = g.shape
    if code == 1:
        return g.view(B, H // 2, 2, W // 2, 2, C).sum((2, 4))
    if code == 2:
        z = torch.zeros(B, 2 * H, 2 * W, C, dtype=g.dtype, device=g.device)
        z[:, ::2, ::2] = g
        return z
    return g


def _args3(n, views, codes):
    """(pointer, pixel stride, code) of three inputs, the third NULL for n = 2"""
    out = []
    for k in range(3):
        out += [vp(views[k]), views[k].stride(2), codes[k]] if k < n else [None, 0, 0]
    return out


def _fwd(n, xs, codes, w, out, shape, dtype):
    B, H, W, C = shape
    return N.lib().vt_wfuse_fwd(n, *_args3(n, xs, codes), vp(w), EPS, vp(out), out.stride(2), B, H, W, C, dtype, stream())


def _bwd(n, g, xs, codes, w, dxs, accs, sums, shape, dtype):
    B, H, W, C = shape
    grads = []
    for k in range(3):
        grads += [vp(dxs[k]), dxs[k].stride(2), accs[k]] if k < n and dxs[k] is not None else [None, 0, 0]
    return N.lib().vt_wfuse_bwd(n, vp(g), g.stride(2), *_args3(n, xs, codes), vp(w), EPS, *grads, vp(sums), B, H, W, C, dtype,
                                stream())


def _sums(n):
    return torch.zeros(N.VT_STAT_REPLICAS * n * 2, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", GEOM, ids=lambda g: "x".join(map(str, g[0])) + "-" + "".join(map(str, g[1])))
def test_wfuse_matches_torch_float64(geom, dtype, sliced):
    shape, codes = geom
    n, td, t_, C = len(codes), TD[dtype], tol(dtype), shape[3]
    torch.manual_seed(sum(shape) + 7 * n + sum(codes))
    xw, xs = zip(*[_map(_src_shape(shape, c), td, sliced) for c in codes])
    gw, g = _map(shape, td, sliced)
    x64 = [_resample(x.double(), c) for x, c in zip(xs, codes)]
    g64 = g.double()
    for wv in WEIGHTS[n]:
        w = torch.tensor(wv, device="cuda")
        r = torch.relu(w.double())
        den = r.sum() + EPS
        out_ref = sum(ri * xi for ri, xi in zip(r, x64)) / den
        dead = bool((w <= 0).all())
        # ---- forward, twice
        outs = [_map(shape, td, sliced, "zeros") for _ in range(2)]
        for ow, o in outs:
            N.check(_fwd(n, xs, codes, w, o, shape, dtype))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][1], outs[1][1])
        assert _surroundings_stay_nan(outs[0][0], C)
        out = outs[0][1]
        if dead:
            assert (out == 0).all()
        else:
            assert rel_err(out, out_ref) < t_, wv
        # ---- backward with accumulate 0 and 1 for every input, each twice
        dw_ref = torch.stack([(g64 * (xi - out_ref)).sum() / den * (1.0 if wi > 0 else 0.0) for xi, wi in zip(x64, wv)])
        scale = torch.stack([(g64.abs() * (xi.abs() + out_ref.abs())).sum() / den for xi in x64])
        first = {}
        for acc in (0, 1):
            pre = [_map(_src_shape(shape, c), td, sliced) for c in codes]  # what the gradient buffers hold before
            runs = []
            for _ in range(2):
                bufs = [(pw.clone(), None) for pw, _ in pre]
                bufs = [(bw, bw[..., OFF : OFF + C] if sliced else bw) for bw, _ in bufs]
                sums, dw = _sums(n), torch.zeros(n, device="cuda")
                N.check(_bwd(n, g, xs, codes, w, [v for _, v in bufs], [acc] * n, sums, shape, dtype))
                N.check(N.lib().vt_wfuse_finalize(vp(sums), vp(w), EPS, n, vp(dw), stream()))
                runs.append((bufs, sums, dw))
            torch.cuda.synchronize()
            first[acc] = runs[0]
            (bufs, sums, dw), (bufs2, sums2, dw2) = runs
            assert torch.equal(sums, sums2) and torch.equal(dw, dw2)
            for k, c in enumerate(codes):
                bw, dx = bufs[k]
                assert torch.equal(dx, bufs2[k][1]), k
                assert _surroundings_stay_nan(bw, C), k
                before = pre[k][1]
                want = (r[k] / den) * _resample_t(g64, c) + (before.double() if acc else 0.0)
                if dead and not acc:
                    assert (dx == 0).all(), k
                elif dead:
                    assert torch.equal(dx, before), k
                else:
                    assert rel_err(dx, want) < (2 * t_ if acc else t_), (wv, k, acc)
                if c == 2:  # the three pixels of each 2x2 source block that no output pixel reads
                    odd = torch.ones(dx.shape[1], dx.shape[2], dtype=torch.bool, device="cuda")
                    odd[::2, ::2] = False
                    if acc:
                        assert torch.equal(dx[:, odd], before[:, odd]), k  # bit-unchanged
                    else:
                        assert (dx[:, odd] == 0).all(), k
            err = (dw.double() - dw_ref).abs()
            print(f"{shape} {codes} {wv} acc={acc}: |dw - ref| / S = {[f'{v:.1e}' for v in (err / scale).tolist()]}")
            assert (err <= 4e-6 * scale).all(), (wv, dw.tolist(), dw_ref.tolist(), scale.tolist())
            for k, wi in enumerate(wv):
                if wi <= 0:
                    assert dw[k].item() == 0.0, k  # relu'(w <= 0) = 0, as torch gives
        # a NULL gradient pointer skips that input; the weight sums do not depend on it
        sums = _sums(n)
        only = [None] * (n - 1) + [torch.zeros(_src_shape(shape, codes[-1]), device="cuda", dtype=td)]
        N.check(_bwd(n, g, xs, codes, w, only, [0] * n, sums, shape, dtype))
        torch.cuda.synchronize()
        assert torch.equal(sums, first[0][1])
        assert torch.equal(only[-1], first[0][0][-1][1])
    assert all(_surroundings_stay_nan(b, C) for b in (*xw, gw))


def test_finalize_adds_to_the_gradient_slots():
    """d w accumulates (+=) and a weight that is not positive leaves its slot untouched"""
    w = torch.tensor([0.5, -1.0, 0.0], device="cuda")
    sums = _sums(3)
    enc = sums.view(N.VT_STAT_REPLICAS, 3, 2)
    enc[0, :, 1] = torch.tensor([3, -5, 7], device="cuda") * (1 << 33)  # T = 3, -5, 7 in replica 0
    enc[5, 0, 0] = 1  # + 4096 in the high limb of another replica
    dw = torch.tensor([10.0, 20.0, 30.0], device="cuda")
    N.check(N.lib().vt_wfuse_finalize(vp(sums), vp(w), EPS, 3, vp(dw), stream()))
    torch.cuda.synchronize()
    assert dw[1].item() == 20.0 and dw[2].item() == 30.0
    assert dw[0].item() == pytest.approx(10.0 + 4099.0 / (0.5 + EPS), rel=1e-6)


def test_arguments_are_checked():
    lib = N.lib()
    x = torch.zeros(1, 4, 4, 16, device="cuda", dtype=torch.bfloat16)
    h = torch.zeros(1, 2, 2, 16, device="cuda", dtype=torch.bfloat16)
    y, d = torch.zeros_like(x), torch.zeros_like(x)
    w = torch.ones(3, device="cuda")
    s = _sums(3)

    def fwd(n=2, x0=x, ld0=16, c0=0, x1=h, ld1=16, c1=1, out=y, ldo=16, H=4, W=4, C=16, dt=N.VT_BF16, wt=w):
        return lib.vt_wfuse_fwd(n, vp(x0), ld0, c0, vp(x1), ld1, c1, None, 0, 0, vp(wt), EPS, vp(out), ldo, 1, H, W, C, dt, stream())

    def bwd(n=2, g=y, dx0=d, ld0=16, dx1=None, sums=s, C=16, c1=1, H=4):
        return lib.vt_wfuse_bwd(n, vp(g), 16, vp(x), 16, 0, vp(h), 16, c1, None, 0, 0, vp(w), EPS, vp(dx0), ld0, 0, vp(dx1), 16, 0,
                                None, 0, 0, vp(sums), 1, H, 4, C, N.VT_BF16, stream())

    assert fwd(n=1) == N.VT_ERR_UNSUPPORTED and fwd(n=4) == N.VT_ERR_UNSUPPORTED
    assert fwd(C=12) == N.VT_ERR_UNSUPPORTED  # C % 8
    assert fwd(C=6, dt=N.VT_F32) == N.VT_ERR_UNSUPPORTED  # C % 4
    assert fwd(c1=3) == N.VT_ERR_UNSUPPORTED and fwd(dt=7) == N.VT_ERR_UNSUPPORTED
    assert fwd(ld0=8) == N.VT_ERR_INVALID  # ld < C
    assert fwd(out=None) == N.VT_ERR_INVALID and fwd(x1=None) == N.VT_ERR_INVALID and fwd(wt=None) == N.VT_ERR_INVALID
    assert fwd(H=3) == N.VT_ERR_INVALID  # an x2 source under an odd grid
    assert fwd(out=x) == N.VT_ERR_INVALID  # out aliases an input
    assert "vt_wfuse_fwd" in N.last_error() and "aliases" in N.last_error()
    assert bwd(n=5) == N.VT_ERR_UNSUPPORTED and bwd(C=12) == N.VT_ERR_UNSUPPORTED
    assert bwd(sums=None) == N.VT_ERR_INVALID and bwd(g=None) == N.VT_ERR_INVALID and bwd(ld0=8) == N.VT_ERR_INVALID
    assert bwd(dx0=y) == N.VT_ERR_INVALID  # dx aliases g
    assert bwd(dx0=d, dx1=d) == N.VT_ERR_INVALID and bwd(H=3) == N.VT_ERR_INVALID
    assert "vt_wfuse_bwd" in N.last_error()
    assert lib.vt_wfuse_finalize(vp(s), vp(w), EPS, 4, vp(w), stream()) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_wfuse_finalize(vp(s), vp(w), EPS, 3, None, stream()) == N.VT_ERR_INVALID
    assert "vt_wfuse_finalize" in N.last_error()
    N.check(fwd())
    N.check(bwd())
    torch.cuda.synchronize()
