"""vt_mbconv.hip and the SiLU form of the SE MLP against float64 torch autograd, through the C-ABI.

* The BatchNorm passes with a per-image keep factor, y = keep[b] * act(z*scale + shift) + r: forward (ready coefficients and
  the finalize step inside the launch), the backward reduction and the backward apply pass (both forms), activation codes 0
  and 3, for keep rows of ones, zeros, (0, 1.25, 0, ...) and the non-binary (0.5, 2, 0.5, ...).  The rows of a dropped image
  that a pass must not read are NaN on the device: y of such an image is r bit for bit, and the sums stay finite.  The backward
  passes also with the per-(image, channel) addend, g = (keep[b] * dy + add[b][c] / HW) * act'(.), with and without a keep row.
* The normalise + activation + per-image average pool pass: y bit-identical to vt_bn_act_apply's, pooled against the
  float64 mean of that stored y.  (2, 2000, 64) is the shape at which an image is cut into several row slabs (the
  fixed-point scratch and the finishing launch); the others have one owner per (image, channel group).
* vt_se_mlp_act_fwd / _bwd with SiLU; with code 1 they equal vt_se_mlp_fwd / _bwd bit for bit.

Operands are dense or channel slices (ld > C) of NaN-filled buffers whose surroundings must stay NaN; every launch runs twice
and must be bit-identical.  Bounds: those of test_resnet_kernels_gpu.py / test_dwtile_kernels_gpu.py (2e-5 f32 / 6e-3 bf16
relative, 1e-4 on the statistics)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import filler
from vision_toolbox import _native as N

from gpu_util import DNAME, DTYPES, TD, rel_err, rounded, short_grids, stream, tol, vp

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
# (B, HW, C).  (3, 25, 136): channel groups with a remainder, image boundaries inside a row block; (5, 1, 64): one pixel per
# image; (2, 700, 24): more rows than one workgroup walks in a sweep; (2, 9, 256): the reduction's channel groups of 64 and two
# finalize groups in both dtypes; (2, 25, 1032): 258 chunks per row in f32, more than a block has threads -- a second pass of
# the column loop with two live columns -- and no finalize group, the two launches
KEEP_SHAPES = [(3, 25, 8), (3, 25, 136), (5, 1, 64), (2, 700, 24), (2, 9, 256), (2, 25, 1032)]
# on a grid of two row blocks per channel group: several trips of every thread's row loop, the last one partial (7 / 14 at 72
# channels, 25 with two finalize groups and 13 with the reduction's four groups at 256), 194 live rows in the last block, and
# the image boundary at row 130 inside the first block's band -- with a dropped, a kept and a rescaled image
SHORT_GRIDS = [(3, 130, 72), (3, 130, 256)]
KEEP_SHAPES += SHORT_GRIDS
KEEP_ROWS = {"ones": lambda B: [1.0] * B, "zeros": lambda B: [0.0] * B,
             "alternate": lambda B: [0.0 if b % 2 == 0 else 1.25 for b in range(B)],
             "fractions": lambda B: [0.5 if b % 2 == 0 else 2.0 for b in range(B)]}
SHORT_GRID_ROWS = {"mixed": lambda B: [(0.0, 1.0, 1.25)[b % 3] for b in range(B)]}
ACTS = {0: lambda u: u, 3: F.silu}
POOL_SHAPES = [(3, 49, 96), (3, 1, 8), (2, 130, 200), (4, 9, 672), (2, 2000, 64)]
SE_SHAPES = [(3, 96, 4), (2, 144, 6), (2, 40, 1), (3, 1152, 48)]
_ids = lambda shapes: [f"{a}x{b}x{c}" for a, b, c in shapes]


@pytest.fixture(autouse=True)
def _grid_of_the_case(request):
    """the SHORT_GRIDS cases run with two row blocks per channel group (gpu_util.short_grids)"""
    params = getattr(request.node, "callspec", None)
    with short_grids(params is not None and params.params.get("shape") in SHORT_GRIDS):
        yield


def _place(t, dtype, sliced):
    """device copy of the [M, C] cpu tensor t: dense, or a channel slice of a wider buffer filled with NaN"""
    v = t.to("cuda", TD[dtype])
    if not sliced:
        return v, v, t.shape[1]
    pad = 16
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device="cuda", dtype=TD[dtype])
    wide[:, pad : pad + t.shape[1]] = v
    return wide, wide[:, pad : pad + t.shape[1]], wide.shape[1]


def _inner(wide, Cc, sliced):
    return wide[:, 16 : 16 + Cc] if sliced else wide


def _surroundings_are_nan(wide, Cc):
    return bool(torch.isnan(wide[:, :16]).all() and torch.isnan(wide[:, 16 + Cc :]).all())


def _same(a, b):
    a, b = a.float(), b.float()
    return torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _stats(z):
    """a statistics buffer holding sum z, sum z^2 per channel, spread over the replicas"""
    st = N.stats_buffer(z.shape[1])
    zz = z.float().double()
    for rep, idx in enumerate(torch.chunk(torch.arange(z.shape[0], device="cuda"), N.VT_STAT_REPLICAS)):
        if idx.numel():
            N.stats_encode(st, 0, zz[idx].sum(0), rep)
            N.stats_encode(st, 1, (zz[idx] ** 2).sum(0), rep)
    return st


def _inputs(shape, dtype):
    B, HW, Cc = shape
    M, key = B * HW, f"mbconv{shape}"
    z = rounded(filler.tensor(key + "z", (M, Cc)) * 1.5 + 0.3, dtype)
    r = rounded(filler.tensor(key + "r", (M, Cc)), dtype)
    dy = rounded(filler.tensor(key + "dy", (M, Cc)), dtype)
    gamma = filler.tensor(key + "g", (Cc,)) * 0.2 + 1.0
    beta = filler.tensor(key + "b", (Cc,)) * 0.2
    rm, rv = filler.tensor(key + "rm", (Cc,)) * 0.1, filler.tensor(key + "rv", (Cc,)).abs() + 0.5
    return z, r, dy, gamma, beta, rm, rv


_REFS: dict = {}


def _reference(shape, dtype, kind, act, train, with_add=False):
    """float64 autograd of y = keep[b] * act(bn(z)) + r: y, running statistics, (scale, shift, mean, invstd), the sums of the
    backward reduction and the gradients of z, gamma, beta; computed once per case.  with_add: the per-image mean of act(bn(z))
    receives the gradient `add` [B, C] as well (kind None: no keep row, factor 1)"""
    key = (shape, dtype, kind, act, train, with_add)
    if key not in _REFS:
        B, HW, Cc = shape
        z, r, dy, gamma, beta, rm, rv = _inputs(shape, dtype)
        keep = torch.tensor({**KEEP_ROWS, **SHORT_GRID_ROWS}[kind](B) if kind else [1.0] * B, dtype=torch.float64)
        add = rounded(filler.tensor(f"mbconv{shape}add", (B, Cc)) * HW ** 0.5, dtype) if with_add else torch.zeros(B, Cc)
        zd = z.double().requires_grad_(True)
        g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rm_, rv_ = rm.double().clone(), rv.double().clone()
        bn = F.batch_norm(zd.t().reshape(1, Cc, -1, 1), rm_, rv_, g, b, bool(train), MOM, EPS).reshape(Cc, -1).t()
        u = bn.detach().clone().requires_grad_(True)
        a = ACTS[act](u)
        a.backward(torch.ones_like(a))
        a_ = ACTS[act](bn)
        y = keep.repeat_interleave(HW)[:, None] * a_ + r.double()
        ((y * dy.double()).sum() + (a_.reshape(B, HW, Cc).mean(1) * add.double()).sum()).backward()
        mean, var = (z.double().mean(0), z.double().var(0, unbiased=False)) if train else (rm.double(), rv.double())
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = gamma.double() * invstd
        coefs = torch.stack([scale, beta.double() - mean * scale, mean, invstd]).float()
        # g = (keep[b] * dy + add[b][c] / HW) * act'(u)
        gg = (keep.repeat_interleave(HW)[:, None] * dy.double() + add.double().repeat_interleave(HW, 0) / HW) * u.grad
        xhat = (z.double() - mean) * invstd
        _REFS[key] = dict(y=y.detach(), rm=rm_, rv=rv_, coefs=coefs, s1=gg.sum(0), s2=(gg * xhat).sum(0), dz=zd.grad, dg=g.grad,
                          db=b.grad, keep=keep.float(), add=add)
    return _REFS[key]


def _poison(view, keep, HW, which):
    """NaN in the rows of every image whose keep factor is zero (which=True), in place"""
    if which:
        for b, k in enumerate(keep.tolist()):
            if k == 0.0:
                view[b * HW : (b + 1) * HW] = float("nan")


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", KEEP_SHAPES, ids=_ids(KEEP_SHAPES))
def test_keep_forward(shape, dtype):
    B, HW, Cc = shape
    M, lib = B * HW, N.lib()
    z, r, dy, gamma, beta, rm, rv = _inputs(shape, dtype)
    gd, bd = gamma.cuda(), beta.cuda()
    for kind in (SHORT_GRID_ROWS if shape in SHORT_GRIDS else KEEP_ROWS):
        for act in ACTS:
            for fin in (False, True):
                ref = _reference(shape, dtype, kind, act, 1 if fin else 0)  # (ready coefficients: the eval-mode ones)
                keep = ref["keep"].cuda()
                for sliced in (False, True):
                    what = f"{kind} act={act} fin={fin} sliced={sliced}"
                    runs = []
                    for _ in range(2):
                        zw, zv, ldz = _place(z, dtype, sliced)
                        st = _stats(zv) if fin else None  # (a dropped image takes part in the batch statistics)
                        _poison(zv, ref["keep"], HW, True)  # ... and the pass does not read its z
                        rw, rvw, ldr = _place(r, dtype, sliced)
                        yw, yv, ldy = _place(torch.full((M, Cc), float("nan")), dtype, sliced)
                        if fin:
                            rmd, rvd = rm.cuda(), rv.cuda()
                            nbt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
                            coef = torch.zeros(4, Cc, device="cuda")
                            N.check(lib.vt_bn_keep_finalize_apply(vp(st), Cc, float(M), vp(gd), vp(bd), EPS, MOM, vp(rmd), vp(rvd),
                                                                  vp(nbt), vp(coef[0]), vp(coef[1]), vp(coef[2]), vp(coef[3]), vp(zv),
                                                                  ldz, vp(rvw), ldr, vp(yv), ldy, vp(keep), HW, M, act, dtype, stream()))
                            extra = (coef, rmd, rvd, nbt)
                        else:
                            cd = ref["coefs"].cuda()
                            N.check(lib.vt_bn_keep_apply(vp(zv), ldz, vp(cd[0]), vp(cd[1]), vp(rvw), ldr, vp(yv), ldy, vp(keep), HW, M,
                                                         Cc, act, dtype, stream()))
                            extra = ()
                        torch.cuda.synchronize()
                        runs.append((yw, *extra))
                    for a, b in zip(*runs):
                        assert _same(a, b), what
                    y = _inner(runs[0][0], Cc, sliced).float().cpu()
                    err = rel_err(y, ref["y"])
                    print(f"{shape} {DNAME[dtype]} {what}: y rel err {err:.3e}")
                    assert err < tol(dtype), what
                    for b_, k in enumerate(ref["keep"].tolist()):
                        if k == 0.0:  # a dropped image: y is r, bit for bit
                            assert torch.equal(y[b_ * HW : (b_ + 1) * HW], r[b_ * HW : (b_ + 1) * HW]), what
                    if sliced:
                        assert _surroundings_are_nan(runs[0][0], Cc) and _surroundings_are_nan(rw, Cc), what
                    if fin:
                        coef, rmd, rvd, nbt = runs[0][1:]
                        assert rel_err(coef.cpu(), ref["coefs"]) < 2e-5, what
                        np.testing.assert_allclose(rmd.cpu(), ref["rm"], rtol=1e-5, atol=1e-6)
                        np.testing.assert_allclose(rvd.cpu(), ref["rv"], rtol=1e-4, atol=1e-6)
                        assert nbt.item() == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", KEEP_SHAPES, ids=_ids(KEEP_SHAPES))
def test_keep_backward(shape, dtype):
    B, HW, Cc = shape
    M, lib = B * HW, N.lib()
    z, r, dy, gamma, beta, rm, rv = _inputs(shape, dtype)
    # every keep row without an addend; then the addend (the gradient of a per-image average pool of act(bn(z))) with no keep
    # row at all (factor 1: the depthwise unit of an MBConv block) and beside a row that drops images
    rows, both = (SHORT_GRID_ROWS, "mixed") if shape in SHORT_GRIDS else (KEEP_ROWS, "alternate")
    for kind, with_add in [(k, False) for k in rows] + [(None, True), (both, True)]:
        for act in ACTS:
            for train in (1, 0):
                ref = _reference(shape, dtype, kind, act, train, with_add)
                keep, cd = (ref["keep"].cuda() if kind else None), ref["coefs"].cuda()
                aw, av, lda = _place(ref["add"], dtype, False) if with_add else (None, None, 0)
                for sliced in (False, True):
                    # the reduction, twice: bit-identical sums.  dy and z of a dropped image are NaN: neither is read
                    gw, gv, ldg = _place(dy, dtype, sliced)
                    zw, zv, ldz = _place(z, dtype, sliced)
                    _poison(gv, ref["keep"], HW, True)
                    _poison(zv, ref["keep"], HW, not with_add)  # (with an addend a dropped image's z is read)
                    sums = [N.stats_buffer(Cc), N.stats_buffer(Cc)]
                    for s_ in sums:
                        N.check(lib.vt_bn_keep_bwd_reduce(vp(gv), ldg, vp(zv), ldz, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), vp(keep),
                                                          vp(av), lda, HW, M, Cc, act, dtype, vp(s_), stream()))
                    torch.cuda.synchronize()
                    assert torch.equal(sums[0], sums[1])
                    got = N.stats_decode(sums[0]).cpu()
                    np.testing.assert_allclose(got[0], ref["s1"], rtol=1e-4, atol=1e-4)
                    np.testing.assert_allclose(got[1], ref["s2"], rtol=1e-4, atol=1e-4)
                    # the apply pass needs z of every image (dz of a dropped one is not zero under batch statistics), not its dy
                    zw, zv, ldz = _place(z, dtype, sliced)
                    for fin in (False, True):
                        what = f"{kind} add={with_add} act={act} train={train} sliced={sliced} fin={fin}"
                        runs = []
                        for _ in range(2):
                            dzw, dzv, lddz = _place(torch.full((M, Cc), float("nan")), dtype, sliced)
                            dg, db = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
                            bc = torch.zeros(3, Cc, device="cuda")
                            if fin:
                                N.check(lib.vt_bn_keep_bwd_finalize_apply(
                                    vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), train, vp(dg), vp(db),
                                    vp(bc), vp(gv), ldg, vp(zv), ldz, vp(keep), vp(av), lda, HW, vp(dzv), lddz, M, act, dtype, stream()))
                            else:
                                N.check(lib.vt_bn_bwd_finalize(vp(sums[0]), Cc, float(M), 1.0, vp(cd[0]), vp(cd[2]), vp(cd[3]), train,
                                                               vp(dg), vp(db), vp(bc), stream()))
                                N.check(lib.vt_bn_keep_bwd_apply(vp(gv), ldg, vp(zv), ldz, vp(cd[1]), vp(bc), vp(keep), vp(av), lda, HW, vp(dzv),
                                                                 lddz, M, Cc, act, dtype, stream()))
                            torch.cuda.synchronize()
                            runs.append((dzw, dg, db, bc))
                        for a, b in zip(*runs):
                            assert _same(a, b), what
                        dzw, dg, db, bc = runs[0]
                        dz_got = _inner(dzw, Cc, sliced).float().cpu()
                        e_dz = rel_err(dz_got, ref["dz"]) if ref["dz"].abs().max() > 0 else dz_got.abs().max().item()
                        print(f"{shape} {DNAME[dtype]} {what}: dz rel err {e_dz:.3e}")
                        assert e_dz < tol(dtype), what
                        np.testing.assert_allclose((dg - 1).cpu(), ref["dg"], rtol=1e-4, atol=1e-4)
                        np.testing.assert_allclose((db - 1).cpu(), ref["db"], rtol=1e-4, atol=1e-4)
                        if sliced:
                            assert _surroundings_are_nan(dzw, Cc) and _surroundings_are_nan(gw, Cc) and _surroundings_are_nan(zw, Cc)


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_ids(POOL_SHAPES))
def test_normalise_activation_average_pool(shape, dtype):
    B, HW, Cc = shape
    M, lib, td = B * HW, N.lib(), TD[dtype]
    z, r, dy, gamma, beta, rm, rv = _inputs(shape, dtype)
    gd, bd = gamma.cuda(), beta.cuda()
    sb = lib.vt_bn_act_avgpool_scratch_bytes(B, HW, Cc, dtype)
    assert sb == (B * Cc * 16 if shape == (2, 2000, 64) else 0), "which shapes cut an image into row slabs"
    mean, var = z.double().mean(0), z.double().var(0, unbiased=False)
    scale = gamma.double() / torch.sqrt(var + EPS)
    cd = torch.stack([scale, beta.double() - mean * scale]).float().cuda()
    for act in ACTS:
        for sliced in (False, True):
            zw, zv, ldz = _place(z, dtype, sliced)
            # the yardstick: vt_bn_act_apply on the same operands, and the float64 mean of the y it stored
            y0 = torch.empty(M, Cc, device="cuda", dtype=td)
            N.check(lib.vt_bn_act_apply(vp(zv), ldz, vp(cd[0]), vp(cd[1]), None, 0, vp(y0), Cc, M, Cc, act, dtype, stream()))
            st = _stats(zv)
            coef0 = torch.zeros(4, Cc, device="cuda")
            N.check(lib.vt_bn_finalize(vp(st), Cc, float(M), vp(gd), vp(bd), EPS, MOM, None, None, None, vp(coef0[0]), vp(coef0[1]),
                                       vp(coef0[2]), vp(coef0[3]), stream()))
            y1 = torch.empty(M, Cc, device="cuda", dtype=td)
            N.check(lib.vt_bn_act_apply(vp(zv), ldz, vp(coef0[0]), vp(coef0[1]), None, 0, vp(y1), Cc, M, Cc, act, dtype, stream()))
            torch.cuda.synchronize()
            for fin, y_want in ((False, y0), (True, y1)):
                what = f"act={act} sliced={sliced} fin={fin}"
                p_want = y_want.double().reshape(B, HW, Cc).mean(1).cpu()
                runs = []
                for _ in range(2):
                    yw, yv, ldy = _place(torch.full((M, Cc), float("nan")), dtype, sliced)
                    pw, pv, ldp = _place(torch.full((B, Cc), float("nan")), dtype, sliced)
                    scratch = torch.zeros(max(sb, 16) // 8, dtype=torch.int64, device="cuda")
                    if fin:
                        coef = torch.zeros(4, Cc, device="cuda")
                        N.check(lib.vt_bn_act_avgpool_finalize_apply(
                            vp(st), Cc, float(M), vp(gd), vp(bd), EPS, MOM, None, None, None, vp(coef[0]), vp(coef[1]), vp(coef[2]),
                            vp(coef[3]), vp(zv), ldz, vp(yv), ldy, vp(pv), ldp, vp(scratch) if sb else None, B, HW, act, dtype, stream()))
                    else:
                        coef = cd
                        N.check(lib.vt_bn_act_avgpool_apply(vp(zv), ldz, vp(cd[0]), vp(cd[1]), vp(yv), ldy, vp(pv), ldp,
                                                            vp(scratch) if sb else None, B, HW, Cc, act, dtype, stream()))
                    torch.cuda.synchronize()
                    runs.append((yw, pw, coef))
                for a, b in zip(*runs):
                    assert _same(a, b), what
                yw, pw, coef = runs[0]
                assert torch.equal(_inner(yw, Cc, sliced), y_want), what
                if fin:
                    assert torch.equal(coef, coef0), what
                err = rel_err(_inner(pw, Cc, sliced).float().cpu(), p_want)
                print(f"{shape} {DNAME[dtype]} {what}: pooled rel err {err:.3e}")
                assert err < tol(dtype), what
                if sliced:
                    assert _surroundings_are_nan(yw, Cc) and _surroundings_are_nan(pw, Cc) and _surroundings_are_nan(zw, Cc), what


_SE: dict = {}


def _se_case(shape, dtype):
    key = (shape, dtype)
    if key not in _SE:
        B, Cc, S = shape
        tag = f"mbse{shape}"
        p = rounded(filler.tensor(tag + "p", (B, Cc)).abs(), dtype)
        w1 = rounded(filler.tensor(tag + "w1", (S, Cc)) * Cc ** -0.5 * 2, dtype)
        w2 = rounded(filler.tensor(tag + "w2", (Cc, S)) * S ** -0.5 * 2, dtype)
        b1, b2 = filler.tensor(tag + "b1", (S,)) * 0.2, filler.tensor(tag + "b2", (Cc,)) * 0.2
        dl = rounded(filler.tensor(tag + "dl", (B, Cc)), dtype)
        leaves = [t.double().requires_grad_(True) for t in (p, w1, b1, w2, b2)]
        pd, w1d, b1d, w2d, b2d = leaves
        logits = F.silu(pd @ w1d.t() + b1d) @ w2d.t() + b2d
        logits.backward(dl.double())
        _SE[key] = dict(p=p, w1=w1, b1=b1, w2=w2, b2=b2, dl=dl, logits=logits.detach(), grads=[t.grad for t in leaves])
    return _SE[key]


def _se_run(lib, c, shape, dtype, act, legacy=False):
    B, Cc, S = shape
    td = TD[dtype]
    p, dl = c["p"].to("cuda", td), c["dl"].to("cuda", td)
    w1, b1, w2, b2 = (c[k].cuda() for k in ("w1", "b1", "w2", "b2"))
    hid = torch.full((2 if act == 3 else 1, B, S), float("nan"), device="cuda")
    logits = torch.full((B, Cc), float("nan"), device="cuda", dtype=td)
    dhid = torch.full((B, S), float("nan"), device="cuda")
    dp = torch.full((B, Cc), float("nan"), device="cuda", dtype=td)
    grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
    code = () if legacy else (act,)
    fwd, bwd = (lib.vt_se_mlp_fwd, lib.vt_se_mlp_bwd) if legacy else (lib.vt_se_mlp_act_fwd, lib.vt_se_mlp_act_bwd)
    N.check(fwd(vp(p), Cc, vp(w1), vp(b1), vp(w2), vp(b2), vp(hid), vp(logits), Cc, B, Cc, S, *code, dtype, stream()))
    N.check(bwd(vp(dl), Cc, vp(p), Cc, vp(w1), vp(w2), vp(hid), vp(dhid), vp(dp), Cc, *[vp(g) for g in grads], B, Cc, S, *code, dtype,
                stream()))
    torch.cuda.synchronize()
    return [hid, logits, dp, *grads]


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("shape", SE_SHAPES, ids=_ids(SE_SHAPES))
def test_se_mlp_with_silu(shape, dtype):
    c, lib = _se_case(shape, dtype), N.lib()
    runs = [_se_run(lib, c, shape, dtype, 3) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    _, logits, dp, dw1, db1, dw2, db2 = [t.float().cpu() for t in runs[0]]
    want = c["grads"]
    errs = dict(logits=rel_err(logits, c["logits"]), dp=rel_err(dp, want[0]), dw1=rel_err(dw1, want[1]), db1=rel_err(db1, want[2]),
                dw2=rel_err(dw2, want[3]), db2=rel_err(db2, want[4]))
    print(shape, DNAME[dtype], {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < tol(dtype), (k, v)
    # code 1 is the existing entry points, bit for bit
    for a, b in zip(_se_run(lib, c, shape, dtype, 1), _se_run(lib, c, shape, dtype, 1, legacy=True)):
        assert torch.equal(a, b), "act = 1 differs from vt_se_mlp_fwd / _bwd"


def test_bad_arguments_return_an_error_code():
    lib = N.lib()
    B, HW, Cc, dt = 2, 5, 16, N.VT_BF16
    M = B * HW
    t = lambda: torch.zeros(M, Cc, device="cuda", dtype=torch.bfloat16)
    z, r, y, dy, dz, pooled = t(), t(), t(), t(), t(), t()
    f = torch.zeros(4, Cc, device="cuda")
    keep = torch.ones(B, device="cuda")
    sums = N.stats_buffer(Cc)
    s = stream()
    odd = C.c_void_p(z.data_ptr() + 2)  # misaligned
    bad = [
        lib.vt_bn_keep_apply(None, Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(keep), HW, M, Cc, 0, dt, s),
        lib.vt_bn_keep_apply(odd, Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(keep), HW, M, Cc, 0, dt, s),
        lib.vt_bn_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, None, HW, M, Cc, 0, dt, s),  # no keep row
        lib.vt_bn_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(keep), 3, M, Cc, 0, dt, s),  # M % HW
        lib.vt_bn_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(keep), HW, M, Cc, 9, dt, s),  # activation code
        lib.vt_bn_keep_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(r), Cc, vp(y), Cc, vp(keep), HW, M, 12, 0, dt, s),  # C no multiple of 8
        lib.vt_bn_keep_finalize_apply(None, Cc, float(M), None, None, EPS, MOM, None, None, None, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]),
                                      vp(z), Cc, vp(r), Cc, vp(y), Cc, vp(keep), HW, M, 0, dt, s),
        lib.vt_bn_keep_bwd_reduce(vp(dy), Cc, vp(z), Cc, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]), vp(keep), None, 0, HW, M, Cc, 0, dt, None, s),
        lib.vt_bn_keep_bwd_reduce(vp(dy), Cc, vp(z), Cc, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]), None, None, 0, HW, M, Cc, 0, dt, vp(sums), s),  # neither
        lib.vt_bn_keep_bwd_reduce(vp(dy), Cc, vp(z), Cc, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]), None, vp(pooled), 8, HW, M, Cc, 0, dt, vp(sums), s),  # lda < C
        lib.vt_bn_keep_bwd_apply(vp(dy), Cc, vp(z), Cc, vp(f[1]), None, vp(keep), None, 0, HW, vp(dz), Cc, M, Cc, 0, dt, s),
        lib.vt_bn_keep_bwd_finalize_apply(vp(sums), Cc, float(M), 1.0, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]), 1, None, None, None, vp(dy),
                                          Cc, vp(z), Cc, vp(keep), None, 0, HW, vp(dz), Cc, M, 0, dt, s),  # no coefficient buffer
        lib.vt_bn_act_avgpool_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(y), Cc, None, Cc, None, B, HW, Cc, 3, dt, s),  # no pooled row
        lib.vt_bn_act_avgpool_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(y), Cc, vp(pooled), 8, None, B, HW, Cc, 3, dt, s),  # ldp < C
        lib.vt_bn_act_avgpool_apply(vp(z), Cc, vp(f[0]), vp(f[1]), vp(y), Cc, vp(pooled), Cc, None, 1, 4000, Cc, 3, dt, s),  # slabs, no scratch
        lib.vt_se_mlp_act_fwd(vp(pooled), Cc, vp(f[0]), vp(f[1]), vp(f[2]), vp(f[3]), vp(f), vp(y), Cc, 1, Cc, 1, 2, dt, s),  # code 2
    ]
    torch.cuda.synchronize()
    for k, rc in enumerate(bad):
        assert rc != 0, k
    assert N.last_error()
    assert lib.vt_bn_act_avgpool_scratch_bytes(1, 4000, Cc, dt) > 0 and lib.vt_bn_act_avgpool_scratch_bytes(1, 4, 12, dt) < 0
