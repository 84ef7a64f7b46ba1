"""References, inputs and bounds of test_head_neck_kernels_gpu.py checked without a GPU: for every bound of
head_neck_util.py a plain-torch restatement of the kernel's arithmetic -- f32 operations in the kernel's order, one bf16
store where the dtype is bf16 -- must stay within HALF of the bound's f32 part (head_neck_util.half_bound) of the float64
reference, on the very inputs the GPU test uses.  A kernel that computes what its source says then has the other half as
margin for contraction into FMAs and the device's expf / logf.
"""
import pytest
import torch

import head_neck_util as U

DTYPES = [U.F32, U.BF16]
DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=[U.DNAME[d] for d in DTYPES])
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def store(v: torch.Tensor, dtype: int) -> torch.Tensor:
    return v.to(U.TD[dtype]).float()


def fma(a, b, c):
    """one rounding: the product of two f32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


_MISSES: list = []


def within(got, ref, half, what: str = "") -> float:
    """the worst error as a fraction of `half`; beyond 1 it is noted, and settle() at the end of the test fails with all
    of them, so that one miss does not hide the checks behind it"""
    fr = U.frac(got, ref, half)
    if not fr <= 1.0:
        _MISSES.append((what, round(fr, 3)))
    return fr


def settle():
    misses = list(_MISSES)
    _MISSES.clear()
    assert not misses, f"restatements beyond half of their bound (as fractions of the half): {misses}"


# ---- 1. resampling ----------------------------------------------------------------------------------------------------
def _taps(nd: int, ns: int, down: bool):
    d = torch.arange(nd)
    if down:
        return 2 * d, 2 * d + 1, torch.full((nd,), 0.5)
    k, odd = d >> 1, (d & 1).bool()
    t0 = torch.where(odd, k, (k - 1).clamp_min(0))
    t1 = torch.where(odd, (k + 1).clamp_max(ns - 1), k)
    return t0, t1, torch.where(odd, 0.75, 0.25).float()


def resample_fwd(x, other, mode, Hd, Wd):
    B, Hs, Ws, _ = x.shape
    if mode < 2:
        i, j = torch.arange(Hd), torch.arange(Wd)
        si, sj = (2 * i, 2 * j) if mode & 1 else (i >> 1, j >> 1)
        v = x[:, si][:, :, sj]
    else:
        i0, i1, wi = _taps(Hd, Hs, bool(mode & 1))
        j0, j1, wj = _taps(Wd, Ws, bool(mode & 1))
        wi, wj = wi[None, :, None, None], wj[None, None, :, None]
        a, c, d, e = x[:, i0][:, :, j0], x[:, i0][:, :, j1], x[:, i1][:, :, j0], x[:, i1][:, :, j1]
        v = wi * (wj * a + (1 - wj) * c) + (1 - wi) * (wj * d + (1 - wj) * e)
    return v + other if other is not None else v


def _wup(d, s, n):
    k, odd = d >> 1, (d & 1).bool()
    t0 = torch.where(odd, k, (k - 1).clamp_min(0))
    t1 = torch.where(odd, (k + 1).clamp_max(n - 1), k)
    w0 = torch.where(odd, 0.75, 0.25).float()
    return (t0 == s) * w0 + (t1 == s) * (1 - w0)


def resample_bwd(g, prior, mode, Hs, Ws):
    B, Hd, Wd, _ = g.shape
    a = prior.clone() if prior is not None else torch.zeros(B, Hs, Ws, g.shape[-1])
    i, j = torch.arange(Hs), torch.arange(Ws)
    if mode == 0:
        for di in range(2):
            for dj in range(2):
                a = a + g[:, 2 * i + di][:, :, 2 * j + dj]
    elif mode == 1:
        a[:, ::2, ::2] = a[:, ::2, ::2] + g
    elif mode == 2:
        for oi in range(-1, 3):
            di = 2 * i + oi
            wi = _wup(di.clamp(0, Hd - 1), i, Hs) * ((di >= 0) & (di < Hd))
            for oj in range(-1, 3):
                dj = 2 * j + oj
                wj = _wup(dj.clamp(0, Wd - 1), j, Ws) * ((dj >= 0) & (dj < Wd))
                w = (wi[:, None] * wj[None, :])[None, :, :, None]
                a = fma(w, g[:, di.clamp(0, Hd - 1)][:, :, dj.clamp(0, Wd - 1)], a)
    else:
        a = fma(torch.tensor(0.25), g[:, i >> 1][:, :, j >> 1], a)
    return a


RS_GEOS = U.RESAMPLE_GEOS


@DTYPE
@pytest.mark.parametrize("geo", RS_GEOS, ids=_ids(RS_GEOS))
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_resample_restatement_within_half_the_bounds(mode, geo, dtype):
    c = U.resample_case(mode, geo, dtype, "long" if geo[:3] == U.RESAMPLE_LONG else "small")
    (_, Hs, Ws), (_, Hd, Wd) = U.resample_shapes(mode, geo)
    for other, ref, S in ((None, c["y"], c["Sy"]), (c["o"], c["yo"], c["Syo"])):
        got = store(resample_fwd(c["x"], other, mode, Hd, Wd), dtype)
        if mode >= 2:
            within(got, ref, U.half_bound(U.K_BILINEAR_FWD, S, ref, dtype), f"fwd other={other is not None}")
        elif other is None:
            assert torch.equal(got.double(), ref)   # moved values: the reference itself is exact
        else:
            assert torch.equal(got, store(c["y"].float() + other, dtype))
    for acc in (0, 1):
        got = store(resample_bwd(c["g"], c["prior"] if acc else None, mode, Hs, Ws), dtype)
        ref, S = c["d"][acc], c["Sd"][acc]
        if mode == 1:   # what the GPU test asserts exactly is what the float64 reference says, rounded once
            assert torch.equal(got, store(ref.float(), dtype))
            start = c["prior"].double() if acc else torch.zeros_like(ref)
            assert torch.equal(ref[:, 1::2], start[:, 1::2]) and torch.equal(ref[:, :, 1::2], start[:, :, 1::2])
        else:
            within(got, ref, U.half_bound(U.resample_bwd_k(mode), S, ref, dtype), f"bwd accumulate={acc}")
            if mode == 0:   # 8-bit values, or f32 on NEAREST_UP_BWD_GRID: the four adds are exact
                assert torch.equal(got, store(ref.float(), dtype)) and (dtype == U.BF16 or torch.equal(got.double(), ref))
    settle()


# ---- 2. softmax cross entropy --------------------------------------------------------------------------------------------
def xent(z, y, eps, gs, mode, lam, dtype):
    """xent_kernel: 256 strided partial sums, the xor butterfly of a wave, the four waves in order"""
    B, N_ = z.shape
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    eps, gs, lam = f(eps), f(gs), f(lam if mode else 1.0)
    mx = z.max(1).values
    pad = (-N_) % U.THREADS
    e = torch.cat([torch.exp(z - mx[:, None]), torch.zeros(B, pad)], 1).view(B, -1, U.THREADS)
    zz = torch.cat([z, torch.zeros(B, pad)], 1).view(B, -1, U.THREADS)

    def block_sum(t):
        s = torch.zeros(B, U.THREADS)
        for it in range(t.shape[1]):
            s = s + t[:, it]
        s = s.view(B, 4, 64)
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ o]
        tot = torch.zeros(B)
        for w in range(4):
            tot = tot + s[:, w, 0]
        return tot

    tse, tsz = block_sum(e), block_sum(zz)
    lse = mx + torch.log(tse)
    yp = y.roll(1, 0) if mode else y
    rows = torch.arange(B)
    zy = lam * z[rows, y] + (1 - lam) * z[rows, yp]
    l = lse - (1 - eps) * zy - (eps / f(float(N_))) * tsz
    loss = torch.zeros(())
    for b in range(B):
        loss = loss + l[b] / f(float(B))
    pr = torch.exp(z - lse[:, None])
    q = (eps / f(float(N_))).expand(B, N_).clone()
    q[rows, y] += (1 - eps) * lam
    q[rows, yp] += (1 - eps) * (1 - lam)
    return loss.item(), store((pr - q) * gs, dtype)


@DTYPE
@pytest.mark.parametrize("shape", U.XENT_SHAPES, ids=_ids(U.XENT_SHAPES))
def test_xent_restatement_within_half_the_bounds(shape, dtype):
    B, N_ = shape
    worst = 0.0
    for eps in U.XENT_EPS:
        for gs in (1.0 / B, 3.0):
            for mode, lam in U.XENT_HEADERS:
                c = U.xent_case(B, N_, dtype, mode, lam, eps)
                loss, dl = xent(c["z"], c["y"], eps, gs, mode, lam, dtype)
                scale = abs(c["loss"]) if N_ > 1 else c["z"].abs().mean().item()
                assert abs(loss - c["loss"]) <= 0.5 * U.XENT_LOSS_REL * scale, (loss, c["loss"])
                # f32: under 4e-6 (p + q) + 2 u (p + q) < 5e-6 (p + q), half of r.  bf16: r = 2^-8 is the store alone -- round to
                # nearest even moves a value v by at most u / (1 + u) |v|, u = 2^-8, which it attains -- so what the bound
                # leaves to the f32 arithmetic is 2^-8 - u / (1 + u) = 2^-16 = 1.5e-5 relative; the restatement may use the
                # store's whole share and half of the f32 bound, and that must fit under the bound the GPU test asserts
                ref, pq = c["dz_unit"] * U.f32r(gs), (c["p"] + c["q"]) * abs(gs)
                half = 0.5 * U.XENT_R[U.F32] * pq
                if dtype == U.BF16:
                    rne = U.BF16_U / (1 + U.BF16_U)
                    half = rne * ref.abs() + half * (1 + rne)
                    assert bool((half <= U.XENT_R[U.BF16] * pq).all())
                worst = max(worst, within(dl, ref, half, f"eps={eps} gs={gs:.3f} header=({mode}, {lam})"))
    print("worst fraction of half the bound", worst)
    settle()


def test_xent_inputs_have_the_rows_the_issue_asks_for():
    for B, N_ in U.XENT_SHAPES:
        z, y = U.xent_logits(B, N_, U.BF16), U.xent_labels(B, N_)
        assert z.abs().max() <= 12 or (z[0].abs() == 40).all()
        assert (z[1:].abs() <= 12).all()
        if B > 1 and N_ > 1:
            assert z[0, y[0]] == 40 and (z[0] == -40).sum() == N_ - 1
            assert (y != y.roll(1, 0)).any(), "a partner label that differs"
        if N_ > 2:
            assert (z[B - 1] == z[B - 1].max()).sum() >= 2, "a tie at the maximum"
    # the partner of row b is row b - 1
    t = U.xent_target(torch.tensor([0, 1, 2]), 3, 1, 0.25)
    assert torch.equal(t, torch.tensor([[0.25, 0, 0.75], [0.75, 0.25, 0], [0, 0.75, 0.25]], dtype=torch.float64))


# ---- 3. MixUp ------------------------------------------------------------------------------------------------------------
@DTYPE
@pytest.mark.parametrize("shape", U.MIX_SHAPES, ids=_ids(U.MIX_SHAPES))
def test_mixup_restatement_within_half_the_bound(shape, dtype):
    x, Cpad = U.mix_images(shape), shape[4]
    for lam in U.MIX_LAMS:
        l = torch.tensor(lam, dtype=torch.float32)
        v = x * l + x.roll(1, 0) * (1 - l)
        got = store(torch.nn.functional.pad(v.permute(0, 2, 3, 1), (0, Cpad - shape[1])), dtype)
        ref, S = U.mix_ref(x, 1, lam, (0, 0, 0, 0), Cpad)
        within(got, ref, U.half_bound(U.K_MIXUP, S, ref, dtype), f"lam={lam}")
    for box in U.mix_boxes(shape[2], shape[3]):   # the boxes are what their names say
        x1, y1, x2, y2 = box
        assert 0 <= x1 <= x2 <= shape[3] and 0 <= y1 <= y2 <= shape[2]
    ref = U.mix_ref(x, 2, 0.5, U.mix_boxes(shape[2], shape[3])[0], Cpad)[0]
    assert torch.equal(ref[..., :shape[1]], x.roll(1, 0).permute(0, 2, 3, 1).double())   # the whole image: the partner's
    settle()


# ---- 4. eval-mode BatchNorm coefficients ---------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("Cc", U.BN_CS)
def test_bn_eval_restatement_within_half_the_bounds(Cc, affine):
    g, b, rm, rv = U.bn_inputs(Cc)
    assert bool((torch.frexp(g)[0].abs() == 0.5).all()), "gamma: powers of two (K_BN_SCALE)"
    assert Cc < 8 or bool((g[1:] != g[:-1]).float().mean() > 0.5), "that differ from channel to channel"
    if not affine:
        g = b = None
    istd = 1.0 / torch.sqrt(rv + torch.tensor(U.BN_EPS, dtype=torch.float32))
    sc = g * istd if affine else istd
    sf = fma(-rm, sc, b if affine else torch.zeros(Cc))
    scale, shift, invstd, S = U.bn_ref(g, b, rm, rv)
    assert rv[0] == 0 and (Cc == 1 or rv[Cc - 1] == 1e-12)
    within(sc, scale, 0.5 * U.K_BN_SCALE * U.U * scale.abs(), "scale")
    within(istd, invstd, 0.5 * U.K_BN_SCALE * U.U * invstd, "invstd")
    within(sf, shift, 0.5 * U.K_BN_SHIFT * U.U * S, "shift")
    settle()


# ---- 5. pooling, ESE gate, column sums ---------------------------------------------------------------------------------
def _lane_sums(t, rt):
    """[B, HW, C] -> [B, lanes, C]: row lane r adds rows r, r + RT, .. in order"""
    B, HW, Cc = t.shape
    lanes = min(rt, HW)
    s = torch.zeros(B, lanes, Cc)
    for hw in range(HW):
        s[:, hw % rt] = s[:, hw % rt] + t[:, hw]
    return s


def _fix_sum(s):
    """lds_fix_add / lds_fix_get: every lane rounded to 2^-32, summed exactly, converted once"""
    q = torch.round(s.double() * 2.0 ** 32)
    return (q.sum(1) * 2.0 ** -32).float()


def _hsig(v):
    return (v * torch.tensor(1.0 / 6.0, dtype=torch.float32) + 0.5).clamp(0.0, 1.0)


@DTYPE
@pytest.mark.parametrize("shape", U.POOL_SHAPES + [(2, U.LONG_ROWS // 2, 257)], ids=_ids(U.POOL_SHAPES + [(2, 2112, 257)]))
def test_pool_and_ese_restatements_within_half_the_bounds(shape, dtype):
    B, HW, _ = shape
    long = HW > 1000
    c = U.pool_case(shape, dtype, "long" if long else "small")
    Cc = c["C"]
    rt = U.THREADS // U.pool_ct(Cc, dtype)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(HW), dtype=torch.float32)
    gate = _hsig(c["s"])[:, None, :]
    for res in (None, c["r"]):
        y = c["x"] * gate
        y = y + res if res is not None else y
        ref, S = (c["y"], c["Sy"]) if res is not None else (c["y"] - c["r"].double(), c["Sy"] - c["r"].double().abs())
        within(store(y, dtype), ref, U.half_bound(U.K_ESE, S, ref, dtype), "ese_gate_fwd")
    for acc in (0, 1):
        a = c["prior"] if acc else torch.zeros(B, HW, Cc)
        within(store(a + c["g"][:, None, :] * inv, dtype), c["pb"][acc], U.half_bound(U.K_POOL_BWD, c["Spb"][acc], c["pb"][acc], dtype), f"avgpool_bwd accumulate={acc}")
    if long:
        settle()
        return
    q = U.pool_quantum(Cc, dtype, HW)
    mean = _fix_sum(_lane_sums(c["x"], rt)) * inv
    within(store(mean, dtype), c["mean"], U.half_bound(U.pool_k(Cc, dtype, HW), c["Smean"], c["mean"], dtype, q / HW), "avgpool_fwd")
    for acc in (0, 1):
        a = c["prior"] if acc else torch.zeros(B, HW, Cc)
        within(store(a + c["dy"] * gate, dtype), c["dx"][acc], U.half_bound(U.K_ESE, c["Sdx"][acc], c["dx"][acc], dtype), f"ese_gate_bwd dx accumulate={acc}")
    d = ((c["s"] > -3) & (c["s"] < 3)) * torch.tensor(1.0 / 6.0, dtype=torch.float32)
    ds = _fix_sum(_lane_sums(c["dy"] * c["x"], rt)) * d
    within(ds, c["ds"], U.half_bound(U.ese_ds_k(Cc, dtype, HW), c["Sds"], c["ds"], U.F32, q / 6), "ese_gate_bwd ds")
    settle()
    closed = c["s"].abs() >= 3
    assert bool(closed.any()) and bool((c["ds"][closed] == 0).all()), "s = +-3 planted, and the reference's derivative is 0 there"
    assert bool(((c["s"].abs() < 3) & (c["s"].abs() > 2.9)).any()), "and a value just inside"


@DTYPE
@pytest.mark.parametrize("cpr", U.COLSUM_CPRS)
@pytest.mark.parametrize("M", U.COLSUM_MS)
def test_colsum_restatement_within_half_the_bound(M, cpr, dtype):
    c, Cc = U.colsum_case(M, cpr, dtype), cpr * U.EPC[dtype]
    rm = U.rowmap(Cc, dtype, M, 256)
    per_block = rm["RT"] * rm["iters"]
    out = c["out0"].clone()
    for r0 in range(0, M, per_block):   # block after block, row lane after row lane: one order the atomics may take
        blk = c["a"][r0:r0 + per_block]
        for r in range(min(rm["RT"], blk.shape[0])):
            s = torch.zeros(Cc)
            for row in blk[r::rm["RT"]]:
                s = s + row
            out = out + s
    within(out, c["ref"], 0.5 * U.colsum_k(Cc, dtype, M) * U.U * c["S"], "colsum")
    settle()


def test_rowmap_restatement_gives_the_cases_their_names():
    assert U.rowmap(24, U.BF16, 100) == dict(CPR=3, CT=3, RT=85, iters=1)
    assert U.rowmap(2056, U.BF16, 80)["CT"] == 256 and U.rowmap(1028, U.F32, 80)["CPR"] == 257
    assert U.rowmap(2056, U.BF16, U.LONG_ROWS)["iters"] == 2 and U.rowmap(2056, U.BF16, 4096)["iters"] == 1
    assert [U.pool_ct(8 * n, U.BF16) for n in (1, 3, 65, 130)] == [1, 4, 64, 64]
    B, h, w = U.RESAMPLE_LONG
    assert B * 2 * h * 2 * w == U.LONG_ROWS
