"""The two-limb fixed-point accumulator of vt_common.h (vt_stat_add / vt_stat_sum: value = hi * 2^12 + lo / 2^33) and the
2^-32 LDS fixed point of the global average pool / ESE gate, tested directly:

  * the raw limbs of vt_colsum_fixed against an exact integer reference, vt_fixed_to_f32, vt_stat_fold and
    vt_channel_sums_to_f32 through the C-ABI;
  * THE MARKER CONTRACT (include/vt_amd.h at VT_STAT_REPLICAS): a contribution that is NaN, +-Inf or has |v| >= 2^50 adds
    2^40 to the hi limb, and every decoder returns NaN for an entry whose summed hi limb has |hi| >= 2^38.

One rule for every consumer of a non-finite / out-of-range contribution (`_rule`): with `ref` the float64 torch result on
the stored operands and `got` the kernel's, (1) where ref is non-finite, got is non-finite (NaN where torch gives +-inf is
fine: the marker carries no sign); (2) where got is finite it matches ref; (3) entries that received no bad contribution
are BIT-IDENTICAL to the same call on operands whose bad cells were replaced by ordinary values -- the marker does not
leak, and that clean run is checked against float64 at the tolerance of the kernel's existing test.  A finite, wrong
result is the only failure."""
from fractions import Fraction

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import TD, conv_desc, stream, vp
from test_stem_bwd_gpu import _reference as _stem_reference

pytestmark = pytest.mark.gpu

R = N.VT_STAT_REPLICAS
MARK = 1 << 40
INF, NAN = float("inf"), float("nan")
WHERE = ["replica0", "last_replica", "folded"]
THREADS = 256  # VT_EW_THREADS


@pytest.fixture(autouse=True)
def _lib_loaded():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _encode(v):
    """values -> int64 [..., 2] limbs by the split of vt_stat_add: hi = trunc(v / 4096), lo = round((v - hi * 4096) * 2^33)
    (exact in float64 for f32 / bf16 values; round half to even as the kernel's conversion)"""
    v = v.double()
    hi = torch.trunc(v / 4096.0)
    lo = torch.round((v - hi * 4096.0) * float(1 << 33))
    return torch.stack([hi.to(torch.int64), lo.to(torch.int64)], -1)


def _decode(q):
    return q[..., 0].double() * 4096.0 + q[..., 1].double() / float(1 << 33)


def _rowmap(Cc, epc, M, target):
    """RowMap::make(C, epc, M, target) of vt_rowmap.h: (chunks per row, threads along the row, row lanes, rows per thread,
    workgroups)"""
    cpr = Cc // epc
    ct = min(cpr, THREADS)
    rt = THREADS // ct
    iters = min(max((M + rt * target - 1) // (rt * target), 1), 64)
    return cpr, ct, rt, iters, (M + rt * iters - 1) // (rt * iters)


def _epc(dtype):
    return 8 if dtype == N.VT_BF16 else 4


def _slice(mat, ld, off):
    """[M][C] device matrix as a channel slice of a wider NaN-filled [M][ld] buffer"""
    wide = torch.full((mat.shape[0], ld), NAN, device="cuda", dtype=mat.dtype)
    wide[:, off:off + mat.shape[1]] = mat
    return wide[:, off:off + mat.shape[1]]


def _colsum_fixed(a, dtype):
    q = torch.zeros(a.shape[1], 2, dtype=torch.int64, device="cuda")
    N.check(N.lib().vt_colsum_fixed(vp(a), a.stride(0), a.shape[0], a.shape[1], dtype, vp(q), stream()))
    return q


def _to_f32(q, n, accumulate=0, dst=None):
    dst = torch.full((n,), 7.0, device="cuda") if dst is None else dst
    N.check(N.lib().vt_fixed_to_f32(vp(q), vp(dst), n, accumulate, stream()))
    return dst


def _mark(buf, where, entries):
    """add the marker (sign * 2^40) to the hi limb of `entries` = [(index into the dims between replica and limb, sign)] of
    the int64 buffer [replicas][...][2]: in replica 0, in the last replica, or in the last replica and then folded into
    replica 0 by vt_stat_fold"""
    r = 0 if where == "replica0" else buf.shape[0] - 1
    for idx, sign in entries:
        buf[(r, *idx, 0)] += sign * MARK
    if where == "folded":
        limbs = buf[0].numel()
        assert buf.shape[0] == R and limbs % 4 == 0  # vt_stat_fold(C) folds 16 replicas of 4 * C limbs
        N.check(N.lib().vt_stat_fold(vp(buf), limbs // 4, stream()))
        assert not buf[1:].any()


def _nan_else_equal(bad, clean, nan):
    """`bad` is NaN exactly where `nan` says and bit-identical to `clean` (all finite) everywhere else"""
    assert torch.isfinite(clean.float()).all()
    assert torch.equal(torch.isnan(bad.float()), nan.expand_as(bad)), torch.isnan(bad.float()).nonzero().tolist()
    keep = ~nan.expand_as(bad)
    assert torch.equal(bad[keep], clean[keep])


def _rule(got, ref, touched, clean, rtol=1e-5):
    """the rule of the module docstring: `touched` marks the entries that received a bad contribution, `clean` is the result
    of the same call without the bad cells; a touched entry that is finite is dominated by the bad value and matches the
    float64 reference to `rtol` (f32 arithmetic; 2^-8 where the output is bf16)"""
    got, ref = got.double(), ref.double()
    fin = torch.isfinite(got)
    assert not (fin & ~torch.isfinite(ref)).any(), "finite where the float64 reference is not"
    assert torch.allclose(got[fin & touched], ref[fin & touched], rtol=rtol, atol=0), (got[fin & touched], ref[fin & touched])
    assert torch.equal(got[~touched], clean.double()[~touched]), "an entry without a bad contribution changed"
    assert fin[~touched].all()


def _bn_stats(z):
    """statistics buffer with sum z, sum z^2 per channel, the rows dealt to the replicas"""
    st = N.stats_buffer(z.shape[1])
    zz = z.double()
    for r, idx in enumerate(torch.chunk(torch.arange(z.shape[0], device="cuda"), R)):
        N.stats_encode(st, 0, zz[idx].sum(0), r)
        N.stats_encode(st, 1, (zz[idx] ** 2).sum(0), r)
    return st


# ---- vt_colsum_fixed: exact limbs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cc,dtype,ld,off", [(37, 24, N.VT_F32, 24, 0), (300, 8, N.VT_BF16, 8, 0), (61, 40, N.VT_BF16, 56, 8)],
                         ids=["37x24_f32", "300x8_bf16_two_workgroups", "61x40_bf16_slice"])
def test_colsum_fixed_limbs_are_the_exact_integer_sums(M, Cc, dtype, ld, off):
    """Shapes at which RowMap::make(C, epc, M, 256) gives iters == 1: a thread adds ONE stored element to 0.f (exact), so the
    limbs are the integer sums of the per-element limbs hi = trunc(v / 4096), lo = round((v - hi * 4096) * 2^33).  Values of
    magnitude 2^-20 .. 2^16 in both signs (lo rounds below 2^-33; hi != 0 above 4096), +-4096 exactly, the values just
    below it, multiples of 4096 and zeros.  Raw limbs EQUAL the int64 reference; two runs give the same bits."""
    cpr, ct, rt, iters, blocks = _rowmap(Cc, _epc(dtype), M, 256)
    assert iters == 1 and blocks == {37: 1, 300: 2, 61: 2}[M]
    g = torch.Generator().manual_seed(M * 100 + Cc)
    v = torch.exp2(torch.rand(M, Cc, generator=g, dtype=torch.float64) * 36 - 20)
    v = v * torch.where(torch.rand(M, Cc, generator=g) < 0.5, -1.0, 1.0)
    special = torch.tensor([4096.0, -4096.0, 4095.99609375, -4095.99609375, 4095.999755859375, -4095.999755859375, 4080.0,
                            -4080.0, 0.0, -0.0, 8192.0, -12288.0, 65536.0, 2.0 ** -20], dtype=torch.float64)
    where = torch.randperm(M * Cc, generator=g)[: 4 * special.numel()]
    v.view(-1)[where] = special.repeat(4)
    a = _slice(v.to(TD[dtype]).cuda(), ld, off)
    stored = a.double()
    assert (stored.abs() >= 4096).any() and (stored.abs() < 2.0 ** -14).any() and (stored == 4096).any()
    want = _encode(stored).sum(0)  # int64 [C][2]
    q1, q2 = _colsum_fixed(a, dtype), _colsum_fixed(a, dtype)
    assert torch.equal(q1, want), (q1 - want).abs().max().item()
    assert torch.equal(q1, q2)


def test_colsum_fixed_with_several_rows_per_thread():
    """(M, C) = (2100, 256) f32: CPR = CT = 64, RT = 4, iters = ceil(2100 / (4 * 256)) = 3 rows per thread.  A thread adds its
    (at most) `iters` elements in f32 before the exact split: iters - 1 roundings of at most 2^-24 of a partial sum that is
    bounded by the thread's sum of |terms|; the split rounds lo to 2^-33 (2^-34 per contribution, at most M of them) and the
    integer sums are exact.  So per column |sum - float64 sum| <= iters * 2^-24 * sum |a| + M * 2^-34."""
    M, Cc = 2100, 256
    cpr, ct, rt, iters, blocks = _rowmap(Cc, 4, M, 256)
    assert (cpr, ct, rt, iters) == (64, 64, 4, 3) and blocks == 175
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(M, Cc, generator=g) * torch.exp2(torch.randint(-6, 12, (1, Cc), generator=g).float())).cuda()
    got = _decode(_colsum_fixed(a, N.VT_F32))
    ref, mass = a.double().sum(0), a.double().abs().sum(0)
    bound = iters * 2.0 ** -24 * mass + M * 2.0 ** -34
    assert ((got - ref).abs() <= bound).all(), ((got - ref).abs() / bound).max().item()


# ---- vt_fixed_to_f32 -------------------------------------------------------------------------------------------------------
def test_fixed_to_f32_decodes_both_limbs():
    """Hand-written limbs: values 1e-9 .. 1e12 of both signs, hi / lo pairs of opposite sign, single lo units.  The kernel
    forms (double)hi * 4096 + (double)lo / 2^33 -- both products exact, ONE rounding to double -- and rounds that to float:
    at most 1 ulp from the exact rational value rounded to f32.  accumulate = 1 adds that float to dst: dst + (float)v exactly."""
    vals = [1e-9, -1e-9, 3.3e-7, -2.5e-4, 0.5, -1.0, 4095.9, -4095.9, 4096.0, -4097.25, 123456.789, -9.87654321e6, 3.0e9,
            -7.7e11, 1e12, -1e12]
    limbs = []
    for v in vals:
        hi = int(v / 4096.0)
        limbs.append((hi, round((v - hi * 4096.0) * (1 << 33))))
    limbs += [(5, -(3 << 33)), (-7, (1 << 44) + 12345), (0, 1), (0, -1), (1 << 27, -(1 << 45) + 1), (-(1 << 27), (1 << 45) - 1),
              (0, 0), (1, -1), (-1, 1)]
    q = torch.tensor(limbs, dtype=torch.int64, device="cuda")
    n = len(limbs)
    exact = [Fraction(hi * (1 << 45) + lo, 1 << 33) for hi, lo in limbs]
    ref = torch.tensor([float(x) for x in exact], dtype=torch.float64).float()  # correctly rounded double, then f32
    got = _to_f32(q, n).cpu()
    ulps = (got.view(torch.int32).long() - ref.view(torch.int32).long()).abs()
    assert (torch.sign(got) == torch.sign(ref)).all() and ulps.max().item() <= 1, ulps.tolist()
    assert got[n - 3].item() == 0.0 and got[16].item() == 5 * 4096.0 - 3.0
    dst0 = torch.linspace(-3.0, 1e6, n, device="cuda")
    acc = _to_f32(q, n, accumulate=1, dst=dst0.clone())
    assert torch.equal(acc, dst0 + got.cuda())


# ---- vt_stat_fold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [24, 1, 70])
def test_stat_fold_sums_the_replicas_into_replica_0(Cc):
    """int64[16][2][C][2] with random limbs of both signs in every replica: afterwards replica 0 EQUALS the int64 sum over the
    replicas, replicas 1 .. 15 are zero.  C = 70: 280 limbs, a full and a partly filled 256-thread workgroup; C = 1: four."""
    g = torch.Generator().manual_seed(Cc)
    buf = torch.stack([torch.randint(-(1 << 30), 1 << 30, (R, 2, Cc), generator=g, dtype=torch.int64),
                       torch.randint(-(1 << 44), 1 << 44, (R, 2, Cc), generator=g, dtype=torch.int64)], -1).cuda()
    buf[R - 1, 0, 0, 0] += MARK  # the marker is part of the hi limb: folded like any value
    guard = torch.full((R * 2 * Cc * 2 + 64,), 0x5A5A, dtype=torch.int64, device="cuda")  # nothing behind the buffer is touched
    guard[: buf.numel()] = buf.view(-1)
    want = buf.sum(0)
    N.check(N.lib().vt_stat_fold(vp(guard), Cc, stream()))
    after = guard[: buf.numel()].view(R, 2, Cc, 2)
    assert torch.equal(after[0], want)
    assert torch.equal(after[1:], torch.zeros_like(after[1:]))
    assert (guard[buf.numel():] == 0x5A5A).all()
    dec = N.stats_decode(after)
    assert torch.isnan(dec[0, 0]) and torch.isfinite(dec.view(-1)[1:]).all()


# ---- vt_channel_sums_to_f32 -------------------------------------------------------------------------------------------------
def test_channel_sums_to_f32_with_a_null_destination():
    """rows = 3, the middle destination NULL: dst_0 and dst_2 gain the float64 sum over the replicas rounded to f32 (the
    kernel adds (float)sum to dst: two f32 roundings), the tensor between them is not touched."""
    Cc = 24
    g = torch.Generator().manual_seed(11)
    parts = torch.randn(R, 3, Cc, generator=g, dtype=torch.float64) * torch.tensor([1e-3, 1.0, 5e4]).view(1, 3, 1)
    sums = _encode(parts).cuda()
    ref = _decode(sums.sum(0)).cpu()
    d = torch.full((3, Cc), 0.25, device="cuda")
    N.check(N.lib().vt_channel_sums_to_f32(vp(sums), 3, Cc, vp(d[0]), None, vp(d[2]), stream()))
    got = d.cpu().double()
    assert (got[1] == 0.25).all()
    for k in (0, 2):
        want = 0.25 + ref[k]
        assert ((got[k] - want).abs() <= 2.0 ** -23 * (ref[k].abs() + 0.25)).all()


# ---- producers: a non-finite contribution travels to the consumer's output --------------------------------------------------
def test_bias_gradient_of_a_non_finite_dz_is_not_finite():
    """vt_colsum_fixed -> vt_fixed_to_f32 (the bias gradient of deterministic mode) on (150, 24) f32: RT = 42, four
    workgroups.  +Inf (row 5, column 2), -Inf (row 50, column 4), NaN (row 100, column 6), and +Inf and -Inf of different
    workgroups in column 8 (float64: NaN; two markers).  Clean run: f32 output of an exact sum, 2^-23 of sum |a| per column."""
    M, Cc = 150, 24
    assert _rowmap(Cc, 4, M, 256)[2:] == (42, 1, 4)
    g = torch.Generator().manual_seed(3)
    a0 = torch.randn(M, Cc, generator=g).cuda()
    a = a0.clone()
    a[5, 2], a[50, 4], a[100, 6], a[6, 8], a[130, 8] = INF, -INF, NAN, INF, -INF
    touched = torch.zeros(Cc, dtype=torch.bool, device="cuda")
    touched[[2, 4, 6, 8]] = True
    clean = _to_f32(_colsum_fixed(a0, N.VT_F32), Cc)
    assert ((clean.double() - a0.double().sum(0)).abs() <= 2.0 ** -23 * a0.double().abs().sum(0)).all()
    q = _colsum_fixed(a, N.VT_F32)
    assert (q[touched, 0] >= MARK).all() and (q[~touched, 0].abs() < 1 << 38).all()
    got = _to_f32(q, Cc)
    _rule(got, a.double().sum(0), touched, clean)
    assert not torch.isfinite(got[touched]).any()  # (this reference is non-finite in all four columns)


@pytest.mark.parametrize("value", [1e25, 3e15], ids=["1e25", "3e15"])
def test_contributions_beyond_the_legitimate_range_never_decode_to_a_wrong_finite_sum(value):
    """Range edge of the encoder: (300, 8) bf16 (CPR = 1: 256 row lanes, iters == 1), two rows of `value` in column 0 (two
    threads, two contributions into one entry) and one row of -value in column 3.  float64: 2 * value and -value, finite;
    the kernel may return those to f32 rounding or a non-finite value.  1e25 / 4096 is beyond int64 (two such conversions
    summed wrap); 3e15 is just above the legitimate 2^50 = 1.1e15."""
    M, Cc = 300, 8
    assert _rowmap(Cc, 8, M, 256)[2:4] == (256, 1)
    g = torch.Generator().manual_seed(8)
    a0 = torch.randn(M, Cc, generator=g).to(torch.bfloat16).cuda()
    a = a0.clone()
    a[0, 0] = a[1, 0] = value
    a[2, 3] = -value
    touched = torch.zeros(Cc, dtype=torch.bool, device="cuda")
    touched[[0, 3]] = True
    clean = _to_f32(_colsum_fixed(a0, N.VT_BF16), Cc)
    got = _to_f32(_colsum_fixed(a, N.VT_BF16), Cc)
    ref = a.double().sum(0)
    assert torch.isfinite(ref).all() and abs(ref[0].item() / value - 2.0) < 0.02  # (bf16 rounding of `value`)
    _rule(got, ref, touched, clean)


def test_bn_backward_sums_of_a_non_finite_dy_give_nan_coefficients():
    """vt_bn_act_bwd_reduce -> vt_bn_bwd_finalize, (2000, 24) f32, ReLU: +Inf / -Inf / NaN in dy at rows of different
    workgroups, columns 2 / 4 / 6 (z there makes the ReLU mask pass).  Float64 reference: sums s1 = sum g, s2 = sum g * xhat,
    then dgamma += s2, dbeta += s1, coef = (a, b = a * s2 / M * invstd, d = b * mean - a * s1 / M).  Clean run: the decoded
    sums within 1e-5 of sum |terms| (a workgroup adds its n rows in f32, n * 2^-24 of sum |terms|: 1e-5 covers n = 160, RT = 42 here), dgamma / dbeta
    at rtol = atol = 1e-4 as test_batchnorm_relu_forward_backward_chain, b and d within that bound on the sums carried through
    their formulas."""
    M, Cc = 2000, 24
    g = torch.Generator().manual_seed(21)
    dy0 = torch.randn(M, Cc, generator=g).cuda()
    z = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).cuda()
    scale, shift = (torch.rand(Cc, generator=g) + 0.5).cuda(), (torch.randn(Cc, generator=g) * 0.2).cuda()
    mean, invstd = (torch.randn(Cc, generator=g) * 0.1 + 0.3).cuda(), (torch.rand(Cc, generator=g) + 0.5).cuda()
    cells = [(3, 2, INF), (700, 4, -INF), (1500, 6, NAN)]
    dy = dy0.clone()
    for r, c, v in cells:
        z[r, c] = 2.0  # scale >= 0.5, |shift| small: the mask is on
        dy[r, c] = v
    touched = torch.zeros(Cc, dtype=torch.bool, device="cuda")
    touched[[2, 4, 6]] = True
    lib = N.lib()

    def run(dyv):
        sums = N.stats_buffer(Cc)
        N.check(lib.vt_bn_act_bwd_reduce(vp(dyv), Cc, vp(z), Cc, vp(scale), vp(shift), vp(mean), vp(invstd), M, Cc, 1, N.VT_F32,
                                         vp(sums), stream()))
        out = torch.zeros(5, Cc, device="cuda")  # dgamma, dbeta, coef a, b, d
        out[0], out[1] = 0.25, -0.5
        N.check(lib.vt_bn_bwd_finalize(vp(sums), Cc, float(M), 1.0, vp(scale), vp(mean), vp(invstd), 1, vp(out[0]), vp(out[1]),
                                       vp(out[2:]), stream()))
        return sums, out

    def reference(dyv):
        on = torch.addcmul(shift, z, scale) > 0
        gg = torch.where(on, dyv.double(), torch.zeros_like(dyv, dtype=torch.float64))
        t2 = gg * (z.double() - mean.double()) * invstd.double()
        s1, s2 = gg.sum(0), t2.sum(0)
        a = scale.double()
        b = a * (s2 / M) * invstd.double()
        d = b * mean.double() - a * (s1 / M)
        return (s1, s2, gg.abs().sum(0), t2.abs().sum(0)), torch.stack([0.25 + s2, -0.5 + s1, a, b, d])

    sums0, clean = run(dy0)
    (s1, s2, m1, m2), ref0 = reference(dy0)
    dec = N.stats_decode(sums0)
    assert ((dec[0] - s1).abs() <= 1e-5 * m1).all() and ((dec[1] - s2).abs() <= 1e-5 * m2).all()
    a64, i64 = scale.double(), invstd.double()
    tol_b = a64 * i64 * 1e-5 * m2 / M + 1e-6 * ref0[3].abs()  # the bound on s2 through b = a * s2 / M * invstd, f32 rounding
    tol_d = mean.double().abs() * tol_b + a64 * 1e-5 * m1 / M + 1e-6 * ref0[4].abs()
    assert torch.allclose(clean[0].double(), ref0[0], rtol=1e-4, atol=1e-4) and torch.allclose(clean[1].double(), ref0[1], rtol=1e-4, atol=1e-4)
    assert torch.equal(clean[2], scale)
    assert ((clean[3].double() - ref0[3]).abs() <= tol_b).all() and ((clean[4].double() - ref0[4]).abs() <= tol_d).all()
    sums, got = run(dy)
    assert torch.equal(torch.isnan(N.stats_decode(sums)).any(0), touched)
    touched5 = touched.expand(5, Cc).clone()
    touched5[2] = False  # a = scale: no sum enters it
    _rule(got, reference(dy)[1], touched5, clean)
    assert torch.isnan(got[:, touched][[0, 1, 3, 4]]).all()


def test_batch_statistics_of_an_overflowing_convolution_give_nan_coefficients():
    """A BatchNorm statistics producer -> vt_bn_finalize: the 1x1 bf16 vt_conv_igemm with VT_CONV_STATS of
    test_conv_forward_and_stats' smallest case (2 x 16 -> 32 x 8 x 8).  A NaN or Inf PIXEL would reach every output channel
    (0 * Inf), so the bad values are made by the convolution itself: the pixels (image 0: 3, 4) and (image 1: 6, 1) hold 1e38
    in input channels 0 / 1, whose filter columns are zero except w[5][0] = 8 and w[11][1] = -8 -- the f32 accumulator and
    the stored y of channel 5 / 11 are +Inf / -Inf there, every other channel is clean.  (A NaN contribution: the other
    producers of this file.)  Reference: float64 statistics of the STORED y; by the rule mean, invstd, scale, shift and both
    running statistics of the two channels are non-finite, the others bit-identical to the run with those pixels zeroed.
    Clean run: sums at rtol 1e-4 / atol 1e-3 as test_conv_forward_and_stats, the finalize outputs against the float64
    arithmetic on the decoded sums at rtol 1e-5 (running variance 1e-4) as test_batchnorm_relu_forward_backward_chain."""
    B, Cin, Cout, H, W = 2, 16, 32, 8, 8
    M = B * H * W
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(Cout, 1, 1, Cin, generator=g) * 0.35).to(torch.bfloat16).cuda()
    w[:, 0, 0, 0:2] = 0.0
    w[5, 0, 0, 0], w[11, 0, 0, 1] = 8.0, -8.0
    x0[..., 0:2] = 0.0
    x = x0.clone()
    x[0, 3, 4, 0], x[1, 6, 1, 1] = 1e38, 1e38
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.2).cuda()
    touched = torch.zeros(Cout, dtype=torch.bool, device="cuda")
    touched[[5, 11]] = True
    lib = N.lib()

    def run(xv):
        y = torch.full((B, H, W, Cout), NAN, device="cuda", dtype=torch.bfloat16)
        st = N.stats_buffer(Cout)
        d = conv_desc(N.VT_BF16, xv, Cin, Cout, 1, 1, 0, Cout, flags=N.VT_CONV_STATS)
        N.check(lib.vt_conv_igemm(C.byref(d), vp(xv), vp(w), vp(y), None, None, None, vp(st), stream()))
        out = torch.zeros(6, Cout, device="cuda")  # scale, shift, mean, invstd, running mean, running var
        out[4], out[5] = 0.1, 0.9
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        N.check(lib.vt_bn_finalize(vp(st), Cout, float(M), vp(gamma), vp(beta), 1e-5, 0.1, vp(out[4]), vp(out[5]), vp(nbt),
                                   vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]), stream()))
        return y, st, out

    def finalize64(s, ss):
        mu = s / M
        var = (ss / M - mu * mu).clamp_min(0.0)
        istd = 1.0 / torch.sqrt(var + 1e-5)
        sc = gamma.double() * istd
        return torch.stack([sc, beta.double() - mu * sc, mu, istd, 0.9 * 0.1 + 0.1 * mu, 0.9 * 0.9 + 0.1 * var * M / (M - 1)])

    y0, st0, clean = run(x0)
    yy = y0.double().reshape(M, Cout)
    dec = N.stats_decode(st0)
    assert torch.allclose(dec[0], yy.sum(0), rtol=1e-4, atol=1e-3) and torch.allclose(dec[1], (yy * yy).sum(0), rtol=1e-4, atol=1e-3)
    ref0 = finalize64(dec[0], dec[1])
    for k, rtol in enumerate([1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 1e-4]):
        assert torch.allclose(clean[k].double(), ref0[k], rtol=rtol, atol=1e-6), k
    y, st, got = run(x)
    yy = y.double().reshape(M, Cout)
    assert yy[3 * W + 4, 5] == INF and yy[H * W + 6 * W + 1, 11] == -INF and torch.isfinite(yy[:, ~touched]).all()
    assert torch.equal(torch.isnan(N.stats_decode(st)).any(0), touched)
    ref = finalize64(yy.sum(0), (yy * yy).sum(0))
    assert not torch.isfinite(ref[:, touched]).any()
    _rule(got, ref, touched.expand(6, Cout), clean)


def _stem_operands(seed, y_form):
    """the smallest case of test_stem_bwd_gpu.py, (B, H, W, lddy, ldz, relu) = (3, 13, 17, 32, 32, 1): one workgroup.  +Inf,
    -Inf and NaN in dy at three pixels of the output channels 5, 9 and 13 (the ReLU mask is on there)."""
    torch.manual_seed(seed)
    dev, B, H, W, Cc = "cuda", 3, 13, 17, 32
    x = torch.zeros(B, H, W, 8, device=dev, dtype=torch.bfloat16)
    x[..., :3] = torch.randn(B, H, W, 3, device=dev).to(torch.bfloat16)
    dy0 = torch.randn(B, H, W, Cc, device=dev).to(torch.bfloat16)
    sc, sf = torch.randn(Cc, device=dev) * 0.8, torch.randn(Cc, device=dev) * 0.5
    mu, istd = torch.randn(Cc, device=dev) * 0.3 + 0.4, torch.rand(Cc, device=dev) + 0.5
    coef = torch.randn(3, Cc, device=dev) * torch.tensor([[1.0], [0.05], [0.02]], device=dev)
    wq = torch.zeros(Cc, 9, 8, device=dev, dtype=torch.bfloat16)
    wq[..., :3] = (torch.randn(Cc, 9, 3, device=dev) * 0.3).to(torch.bfloat16)
    cells = [((0, 4, 7), 5, INF), ((1, 6, 10), 9, -INF), ((2, 9, 3), 13, NAN)]  # interior pixels: all nine taps see them
    for _, n, _ in cells:
        sc[n], sf[n] = 0.8, 0.1
    if y_form:
        z_true = F.conv2d(x[..., :3].double().permute(0, 3, 1, 2), wq[..., :3].double().reshape(Cc, 3, 3, 3).permute(0, 3, 1, 2),
                          padding=1).permute(0, 2, 3, 1)
        zy = (z_true.float() * sc + sf).clamp_min(0).to(torch.bfloat16).contiguous()  # the unit's output y, NHWC in memory
    else:
        z_true = None
        zy = (torch.randn(B, H, W, Cc, device=dev) * 1.5 + 0.4).to(torch.bfloat16)  # the pre-activation z
    dy = dy0.clone()
    for (b, i, j), n, v in cells:
        zy[b, i, j, n] = 2.0  # z * 0.8 + 0.1 > 0 / y > 0
        dy[b, i, j, n] = v
    touched = torch.zeros(Cc, dtype=torch.bool, device=dev)
    touched[[n for _, n, _ in cells]] = True
    return (B, H, W, Cc), x, dy0, dy, zy, z_true, sc, sf, mu, istd, coef, wq, touched


def test_stem_backward_z_form_carries_a_non_finite_dy_into_sums_and_dw():
    """vt_stem_bn_bwd_reduce (fixed = 1) -> vt_stem_bn_bwd_combine against `_reference` of test_stem_bwd_gpu.py: sums[:, n] and
    dW[n] of the three bad output channels n are non-finite (the combine kernel reads the marker of G[n]; `coef` is finite),
    every other n is bit-identical to the run on the clean dy, which meets the 2e-5 of test_stem_backward_matches_float64."""
    (B, H, W, Cc), x, dy0, dy, z, _, sc, sf, mu, istd, coef, _, touched = _stem_operands(41, False)
    lib = N.lib()

    def run(dyv):
        sums = N.stats_buffer(Cc)
        gzx = torch.zeros(lib.vt_stem_bn_bwd_scratch_bytes(Cc) // 4, device="cuda")
        dw = torch.full((Cc, 9, 3), 0.25, device="cuda")
        N.check(lib.vt_stem_bn_bwd_reduce(N.VT_BF16, B, H, W, Cc, vp(x), vp(dyv), Cc, vp(z), Cc, vp(sc), vp(sf), vp(mu), vp(istd),
                                          1, vp(sums), vp(gzx), 1, stream()))
        N.check(lib.vt_stem_bn_bwd_combine(Cc, 3, vp(gzx), vp(coef), vp(dw), 1, stream()))
        return N.stats_decode(sums), dw

    s0, dw0 = run(dy0)
    ref_s, ref_dw = _stem_reference(x, dy0, z, sc, sf, mu, istd, coef, 1)
    assert ((s0 - ref_s).abs() / ref_s.abs().max(dim=1, keepdim=True).values).max().item() < 2e-5
    assert ((dw0.double() - 0.25) - ref_dw).abs().max().item() / ref_dw.abs().max().item() < 2e-5
    s, dw = run(dy)
    ref_s, ref_dw = _stem_reference(x, dy, z, sc, sf, mu, istd, coef, 1)
    assert not torch.isfinite(ref_s[:, touched]).any() and not torch.isfinite(ref_dw[touched]).any()
    _rule(s, ref_s, touched.expand(2, Cc), s0)
    _rule(dw, ref_dw + 0.25, touched.view(Cc, 1, 1).expand(Cc, 9, 3), dw0)


def test_stem_backward_y_form_carries_a_non_finite_dy_into_sums_and_dw():
    """the y form (fixed | 2): vt_stem_bn_bwd_reduce -> vt_stem_bn_bwd_s2 (sum g * xhat from G: it must re-mark sums[1][n]) ->
    vt_stem_bn_bwd_combine_y.  Reference as test_stem_backward_from_the_units_output (z = the float64 conv of the operands)."""
    (B, H, W, Cc), x, dy0, dy, y, z_true, sc, sf, mu, istd, coef, wq, touched = _stem_operands(43, True)
    lib = N.lib()

    def run(dyv):
        sums = N.stats_buffer(Cc)
        gzx = torch.zeros(lib.vt_stem_bn_bwd_scratch_bytes(Cc) // 4, device="cuda")
        dw = torch.full((Cc, 9, 3), 0.25, device="cuda")
        N.check(lib.vt_stem_bn_bwd_reduce(N.VT_BF16, B, H, W, Cc, vp(x), vp(dyv), Cc, vp(y), Cc, vp(sc), vp(sf), vp(mu), vp(istd),
                                          1, vp(sums), vp(gzx), 1 | 2, stream()))
        N.check(lib.vt_stem_bn_bwd_s2(Cc, vp(gzx), vp(wq), vp(mu), vp(istd), vp(sums), 1, stream()))
        N.check(lib.vt_stem_bn_bwd_combine_y(Cc, 3, vp(gzx), vp(coef), vp(wq), vp(dw), 1, stream()))
        return N.stats_decode(sums), dw

    def reference(dyv):
        gg = torch.where(y.float() > 0, dyv.double(), torch.zeros_like(dyv, dtype=torch.float64))
        ref_s = torch.stack([gg.sum((0, 1, 2)), (gg * (z_true - mu.double())).sum((0, 1, 2)) * istd.double()])
        a, b, d = (coef[i].double() for i in range(3))
        wt = torch.zeros(32, 3, 3, 3, dtype=torch.float64, device="cuda", requires_grad=True)
        F.conv2d(x[..., :3].double().permute(0, 3, 1, 2), wt, padding=1).backward((a * gg - b * z_true + d).permute(0, 3, 1, 2))
        return ref_s, wt.grad.permute(0, 2, 3, 1).reshape(32, 9, 3)

    s0, dw0 = run(dy0)
    ref_s, ref_dw = reference(dy0)
    assert ((s0 - ref_s).abs() / ref_s.abs().max(dim=1, keepdim=True).values).max().item() < 2e-5
    assert ((dw0.double() - 0.25) - ref_dw).abs().max().item() / ref_dw.abs().max().item() < 2e-5
    s, dw = run(dy)
    ref_s, ref_dw = reference(dy)
    assert not torch.isfinite(ref_s[:, touched]).any() and not torch.isfinite(ref_dw[touched]).any()
    _rule(s, ref_s, touched.expand(2, Cc), s0)
    _rule(dw, ref_dw + 0.25, touched.view(Cc, 1, 1).expand(Cc, 9, 3), dw0)


# ---- decoders in isolation: the marker written by hand -----------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("fused", [False, True], ids=["vt_bn_finalize", "vt_bn_finalize_apply"])
def test_forward_finalize_returns_nan_for_a_marked_entry(fused, where):
    """statistics of a (150, 24) f32 z spread over the replicas; +2^40 in the hi limb of `sum` of channel 2 and -2^40 in that
    of `sum of squares` of channel 5.  Channel 2: scale, shift, mean, invstd and both running statistics are NaN; channel 5:
    the mean and the running mean are untouched, everything that needs the variance is NaN; every other channel is
    bit-identical to the unmarked call.  vt_bn_finalize_apply (no activation: ReLU is fmaxf, which drops a NaN) also stores y."""
    M, Cc = 150, 24
    g = torch.Generator().manual_seed(51)
    z = (torch.randn(M, Cc, generator=g) * 1.7 + 0.3).cuda()
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).cuda(), (torch.randn(Cc, generator=g) * 0.2).cuda()
    lib = N.lib()

    def run(marked):
        st = _bn_stats(z)
        if marked:
            _mark(st, where, [((0, 2), 1), ((1, 5), -1)])
        out = torch.zeros(6, Cc, device="cuda")  # scale, shift, mean, invstd, running mean, running var
        out[4], out[5] = 0.1, 0.9
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        y = torch.full((M, Cc), 3.0, device="cuda")
        if fused:
            N.check(lib.vt_bn_finalize_apply(vp(st), Cc, float(M), vp(gamma), vp(beta), 1e-5, 0.1, vp(out[4]), vp(out[5]), vp(nbt),
                                             vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]), vp(z), Cc, None, Cc, vp(y), Cc, M, 0,
                                             N.VT_F32, stream()))
        else:
            N.check(lib.vt_bn_finalize(vp(st), Cc, float(M), vp(gamma), vp(beta), 1e-5, 0.1, vp(out[4]), vp(out[5]), vp(nbt),
                                       vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]), stream()))
        return out, y

    clean, y0 = run(False)
    bad, y = run(True)
    nan = torch.zeros(6, Cc, dtype=torch.bool, device="cuda")
    nan[:, 2] = True
    nan[[0, 1, 3, 5], 5] = True
    _nan_else_equal(bad, clean, nan)
    if fused:
        _nan_else_equal(y, y0, nan[0].view(1, Cc))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("fused", [False, True], ids=["vt_bn_bwd_finalize", "vt_bn_bwd_finalize_apply"])
def test_backward_finalize_returns_nan_for_a_marked_entry(fused, where):
    """sums of a (150, 24) f32 backward reduction, then -2^40 in `sum g` of channel 2 and +2^40 in `sum g * xhat` of channel 5:
    dbeta and d of channel 2, dgamma, b and d of channel 5 are NaN, everything else is bit-identical to the unmarked call;
    vt_bn_bwd_finalize_apply also stores dz = a * g - b * z + d."""
    M, Cc = 150, 24
    g = torch.Generator().manual_seed(52)
    dy, z = torch.randn(M, Cc, generator=g).cuda(), (torch.randn(M, Cc, generator=g) * 1.7 + 0.3).cuda()
    scale, shift = (torch.rand(Cc, generator=g) + 0.5).cuda(), (torch.randn(Cc, generator=g) * 0.2).cuda()
    mean, invstd = (torch.randn(Cc, generator=g) * 0.1 + 0.3).cuda(), (torch.rand(Cc, generator=g) + 0.5).cuda()
    lib = N.lib()

    def run(marked):
        sums = N.stats_buffer(Cc)
        N.check(lib.vt_bn_act_bwd_reduce(vp(dy), Cc, vp(z), Cc, vp(scale), vp(shift), vp(mean), vp(invstd), M, Cc, 1, N.VT_F32,
                                         vp(sums), stream()))
        if marked:
            _mark(sums, where, [((0, 2), -1), ((1, 5), 1)])
        out = torch.zeros(5, Cc, device="cuda")  # dgamma, dbeta, coef a, b, d
        out[0], out[1] = 0.25, -0.5
        dz = torch.full((M, Cc), 3.0, device="cuda")
        if fused:
            N.check(lib.vt_bn_bwd_finalize_apply(vp(sums), Cc, float(M), 1.0, vp(scale), vp(shift), vp(mean), vp(invstd), 1, vp(out[0]),
                                                 vp(out[1]), vp(out[2:]), vp(dy), Cc, vp(z), Cc, vp(dz), Cc, M, 1, N.VT_F32, stream()))
        else:
            N.check(lib.vt_bn_bwd_finalize(vp(sums), Cc, float(M), 1.0, vp(scale), vp(mean), vp(invstd), 1, vp(out[0]), vp(out[1]),
                                           vp(out[2:]), stream()))
        return out, dz

    clean, dz0 = run(False)
    bad, dz = run(True)
    nan = torch.zeros(5, Cc, dtype=torch.bool, device="cuda")
    nan[[1, 4], 2] = True
    nan[[0, 3, 4], 5] = True
    _nan_else_equal(bad, clean, nan)
    if fused:
        _nan_else_equal(dz, dz0, nan[4].view(1, Cc))


@pytest.mark.parametrize("sign", [1, -1], ids=["plus", "minus"])
def test_fixed_to_f32_returns_nan_for_a_marked_entry(sign):
    """int64[n][2] has no replicas: the marker in the hi limb of entries 1 and 300 (another workgroup) of 600 valid ones, set
    and accumulated; the neighbours are bit-identical to the unmarked call."""
    n = 600
    g = torch.Generator().manual_seed(53)
    q = _encode(torch.randn(n, generator=g, dtype=torch.float64) * 3e4).cuda()
    nan = torch.zeros(n, dtype=torch.bool, device="cuda")
    nan[[1, 300]] = True
    qm = q.clone()
    qm[nan, 0] += sign * MARK
    for accumulate in (0, 1):
        dst = torch.linspace(-5.0, 5.0, n, device="cuda")
        _nan_else_equal(_to_f32(qm, n, accumulate, dst.clone()), _to_f32(q, n, accumulate, dst.clone()), nan)


@pytest.mark.parametrize("where", WHERE)
def test_channel_sums_to_f32_returns_nan_for_a_marked_entry(where):
    """int64[16][3][24][2]: the marker in (row 0, channel 3) and, negative, (row 2, channel 23)"""
    Cc = 24
    g = torch.Generator().manual_seed(54)
    sums = _encode(torch.randn(R, 3, Cc, generator=g, dtype=torch.float64) * 100).cuda()

    def run(marked):
        s = sums.clone()
        if marked:
            _mark(s, where, [((0, 3), 1), ((2, 23), -1)])
        d = torch.full((3, Cc), 0.25, device="cuda")
        N.check(N.lib().vt_channel_sums_to_f32(vp(s), 3, Cc, vp(d[0]), vp(d[1]), vp(d[2]), stream()))
        return d

    nan = torch.zeros(3, Cc, dtype=torch.bool, device="cuda")
    nan[0, 3] = nan[2, 23] = True
    _nan_else_equal(run(True), run(False), nan)


@pytest.mark.parametrize("where", WHERE)
def test_wfuse_finalize_returns_nan_for_a_marked_entry(where):
    """vt_wfuse_finalize, n = 2 (int64[16][2][2]: four limbs per replica, which vt_stat_fold(C = 1) folds): the marker in
    entry 0 makes d w[0] NaN, d w[1] is bit-identical to the unmarked call"""
    g = torch.Generator().manual_seed(55)
    sums = _encode(torch.randn(R, 2, generator=g, dtype=torch.float64) * 50).cuda()
    w = torch.tensor([0.5, 1.25], device="cuda")

    def run(marked):
        s = sums.clone()
        if marked:
            _mark(s, where, [((0,), 1)])
        dw = torch.tensor([10.0, 20.0], device="cuda")
        N.check(N.lib().vt_wfuse_finalize(vp(s), vp(w), 1e-4, 2, vp(dw), stream()))
        return dw

    _nan_else_equal(run(True), run(False), torch.tensor([True, False], device="cuda"))


@pytest.mark.parametrize("replica", [0, 7], ids=["replica0", "last_replica"])
def test_stem_combine_kernels_return_nan_for_a_marked_entry(replica):
    """`gzx` = int64[8][2C + 16][96][2] written by hand (8 replicas: vt_stat_fold does not apply), with the marker in
      G[n = 4] at tap 2, channel 1 (column 17)    -> dW[4][2][1] (z and y form) and sums[1][4] of vt_stem_bn_bwd_s2,
      row C + 6 at tap 4, channel 0 (column 40)    -> z form: Z[6]: dW[6][4][0];  y form: a patch row, used by every n: dW[:][4][0],
      X (row 2C) at tap 8, channel 2 (column 82)   -> dW[:][8][2] in both forms,
    and vt_stem_bn_bwd_s2 with the marker in sums[0][9] (sum g) instead: sums[1][9].  vt_stem_bn_bwd_s2 RE-MARKS: the entry it
    writes decodes to NaN in N.stats_decode and in vt_bn_bwd_finalize.  Everything else is bit-identical to the unmarked call."""
    Cc, rows = 32, 2 * 32 + 16
    lib = N.lib()
    assert lib.vt_stem_bn_bwd_scratch_bytes(Cc) == 8 * rows * 96 * 16
    g = torch.Generator().manual_seed(56)
    gzx = _encode(torch.randn(8, rows, 96, generator=g, dtype=torch.float64) * 300).cuda()
    coef = (torch.randn(3, Cc, generator=g) * torch.tensor([[1.0], [0.05], [0.02]])).cuda()
    wq = torch.zeros(Cc, 9, 8, dtype=torch.bfloat16)
    wq[..., :3] = (torch.randn(Cc, 9, 3, generator=g) * 0.3).to(torch.bfloat16)
    wq = wq.cuda()
    mu, istd = (torch.randn(Cc, generator=g) * 0.3).cuda(), (torch.rand(Cc, generator=g) + 0.5).cuda()
    s1 = _encode(torch.randn(R, Cc, generator=g, dtype=torch.float64) * 20).cuda()
    col = lambda t, c: (t // 3) * 32 + (t % 3) * 8 + c  # noqa: E731

    def run(mark_gzx, mark_s1):
        q = gzx.clone()
        if mark_gzx:
            q[replica, 4, col(2, 1), 0] += MARK
            q[replica, Cc + 6, col(4, 0), 0] -= MARK
            q[replica, 2 * Cc, col(8, 2), 0] += MARK
        sums = N.stats_buffer(Cc)
        sums[:, 0] = s1
        if mark_s1:
            sums[2 * replica + 1, 0, 9, 0] += MARK
        dwz, dwy = torch.full((Cc, 9, 3), 0.25, device="cuda"), torch.full((Cc, 9, 3), 0.25, device="cuda")
        N.check(lib.vt_stem_bn_bwd_combine(Cc, 3, vp(q), vp(coef), vp(dwz), 1, stream()))
        N.check(lib.vt_stem_bn_bwd_s2(Cc, vp(q), vp(wq), vp(mu), vp(istd), vp(sums), 1, stream()))
        N.check(lib.vt_stem_bn_bwd_combine_y(Cc, 3, vp(q), vp(coef), vp(wq), vp(dwy), 1, stream()))
        fin = torch.zeros(5, Cc, device="cuda")
        N.check(lib.vt_bn_bwd_finalize(vp(sums), Cc, 1000.0, 1.0, vp(istd), vp(mu), vp(istd), 1, vp(fin[0]), vp(fin[1]), vp(fin[2:]),
                                       stream()))
        return dwz, dwy, N.stats_decode(sums), fin[0]

    dwz0, dwy0, s0, dg0 = run(False, False)
    dwz, dwy, s, dg = run(True, False)
    nz = torch.zeros(Cc, 9, 3, dtype=torch.bool, device="cuda")
    nz[4, 2, 1] = nz[6, 4, 0] = True
    nz[:, 8, 2] = True
    ny = nz.clone()
    ny[:, 4, 0] = True
    ns = torch.zeros(2, Cc, dtype=torch.bool, device="cuda")
    ns[1, 4] = True
    _nan_else_equal(dwz, dwz0, nz)
    _nan_else_equal(dwy, dwy0, ny)
    _nan_else_equal(s, s0, ns)
    _nan_else_equal(dg, dg0, ns[1])
    dwz, dwy, s, dg = run(False, True)
    ns = torch.zeros(2, Cc, dtype=torch.bool, device="cuda")
    ns[:, 9] = True
    assert torch.equal(dwz, dwz0) and torch.equal(dwy, dwy0)
    _nan_else_equal(s, s0, ns)
    _nan_else_equal(dg, dg0, ns[1])


# ---- global average pool and ESE gate: the 2^-32 LDS fixed point --------------------------------------------------------------
def _pool_rt(Cc, epc):
    """row lanes of avgpool_fwd_kernel / ese_bwd_kernel: 256 / pool_ct(C, epc)"""
    ct = 1
    while ct < Cc // epc and ct < 64:
        ct <<= 1
    return THREADS // ct


POOL_CASES = [(24, N.VT_F32, 32), (40, N.VT_BF16, 56)]
POOL_IDS = ["24_f32", "40_bf16"]
# (image, pixel, channel, value): +Inf, NaN and a finite value beyond the 2^31 range of the 2^-32 fixed point
POOL_CELLS = [(0, 3, 2, INF), (1, 20, 5, NAN), (2, 40, 9, 3e9)]


@pytest.mark.parametrize("Cc,dtype,ld", POOL_CASES, ids=POOL_IDS)
def test_global_avgpool_of_a_non_finite_map_is_not_finite(Cc, dtype, ld):
    """vt_global_avgpool_fwd, B = 3, HW = 7 * 7, x a channel slice (ldx > C).  The three cells (image, channel) that hold a bad
    pixel follow the rule (3e9: float64 gives 6.1e7, the kernel that or NaN), every other cell is bit-identical to the clean
    run, which is within tol * mean |x| of float64 per cell (tol = 1e-6 f32 / 6e-3 bf16 of test_global_avgpool_and_ese_gate)."""
    B, HW = 3, 49
    g = torch.Generator().manual_seed(61)
    x0 = _slice(torch.randn(B * HW, Cc, generator=g).to(TD[dtype]).cuda(), ld, 8).view(B, HW, Cc)
    touched = torch.zeros(B, Cc, dtype=torch.bool, device="cuda")

    def run(xv):
        y = torch.full((B, ld), 9.0, device="cuda", dtype=TD[dtype])
        N.check(N.lib().vt_global_avgpool_fwd(vp(xv), ld, vp(y[:, 8:]), ld, B, HW, Cc, dtype, stream()))
        assert (y[:, :8] == 9.0).all() and (y[:, 8 + Cc:] == 9.0).all()
        return y[:, 8:8 + Cc].clone()

    clean = run(x0)
    tol = 1e-6 if dtype == N.VT_F32 else 6e-3
    assert ((clean.double() - x0.double().mean(1)).abs() <= tol * x0.double().abs().mean(1)).all()
    for b, hw, c, v in POOL_CELLS:
        x0[b, hw, c] = v  # (x0 is a view of the wide buffer: the clean run is done)
        touched[b, c] = True
    ref = x0.double().mean(1)
    assert torch.isfinite(ref[2, 9]) and not torch.isfinite(ref[0, 2]) and torch.isnan(ref[1, 5])
    _rule(run(x0), ref, touched, clean, rtol=1e-5 if dtype == N.VT_F32 else 2.0 ** -8)


@pytest.mark.parametrize("Cc,dtype,ld", POOL_CASES, ids=POOL_IDS)
def test_ese_gate_backward_of_a_non_finite_gradient_is_not_finite(Cc, dtype, ld):
    """vt_ese_gate_bwd with the bad values in dy: ds[b][c] = hsig'(s) * sum_hw dy * x follows the rule in the three cells and is
    bit-identical to the clean run elsewhere; dx = dy * hsig(s) is elementwise: bit-identical to the clean run in every
    element but the three bad ones.  Clean run: dx at rel. L2 1e-6 / 6e-3, ds at 1e-5 as test_global_avgpool_and_ese_gate."""
    B, HW = 3, 49
    g = torch.Generator().manual_seed(62)
    td = TD[dtype]
    x = _slice(torch.randn(B * HW, Cc, generator=g).to(td).cuda(), ld, 8).view(B, HW, Cc)
    dy0 = _slice(torch.randn(B * HW, Cc, generator=g).to(td).cuda(), ld, 8).view(B, HW, Cc)
    s = _slice((torch.randn(B, Cc, generator=g) * 2).to(td).cuda(), ld, 8)
    for b, _, c, _ in POOL_CELLS:
        s[b, c] = 0.5  # hsig'(s) = 1/6 in the bad cells: the sum itself reaches ds
    gate = F.hardsigmoid(s.double())
    dgate = ((s.double() > -3) & (s.double() < 3)).double() / 6.0

    def run(dyv):
        dx = torch.full((B * HW, ld), 9.0, device="cuda", dtype=td)
        ds = torch.full((B, Cc), 9.0, device="cuda")
        N.check(N.lib().vt_ese_gate_bwd(vp(dyv), ld, vp(x), ld, vp(s), ld, vp(dx[:, 8:]), ld, vp(ds), B, HW, Cc, 0, dtype, stream()))
        assert (dx[:, :8] == 9.0).all() and (dx[:, 8 + Cc:] == 9.0).all()
        return dx[:, 8:8 + Cc].clone().view(B, HW, Cc), ds

    dx0, ds0 = run(dy0)
    ref_dx, ref_ds = dy0.double() * gate[:, None, :], (dy0.double() * x.double()).sum(1) * dgate
    assert ((dx0.double() - ref_dx).norm() / ref_dx.norm()).item() < (1e-6 if dtype == N.VT_F32 else 6e-3)
    assert ((ds0.double() - ref_ds).norm() / ref_ds.norm()).item() < 1e-5
    touched = torch.zeros(B, Cc, dtype=torch.bool, device="cuda")
    elem = torch.zeros(B, HW, Cc, dtype=torch.bool, device="cuda")
    for b, hw, c, v in POOL_CELLS:
        dy0[b, hw, c] = v
        touched[b, c] = elem[b, hw, c] = True
    dx, ds = run(dy0)
    ref_ds = (dy0.double() * x.double()).sum(1) * dgate
    assert torch.isfinite(ref_ds[2, 9]) and not torch.isfinite(ref_ds[0, 2]) and torch.isnan(ref_ds[1, 5])
    _rule(ds, ref_ds, touched, ds0)
    assert torch.equal(dx[~elem], dx0[~elem])
    assert not torch.isfinite(dx[0, 3, 2]) and torch.isnan(dx[1, 20, 5])


@pytest.mark.parametrize("Cc,dtype,ld", POOL_CASES, ids=POOL_IDS)
def test_global_avgpool_and_ese_sums_of_a_small_channel(Cc, dtype, ld):
    """Channel 1 holds values of order 1e-7 beside channels of order 1, each channel checked on its own.  The bound from the
    code: a row lane (RT = 256 / pool_ct(C, epc) of them) adds its k = ceil(HW / RT) values in f32 ((k - 1) roundings of
    2^-24 of at most the lane's sum |v|), rounds that partial sum to the 2^-32 grid (2^-33) and the integer sum is exact:
        |sum - float64 sum| <= RT * 2^-33 + (k - 1) * 2^-24 * sum |v|.
    The result is rounded to float, scaled (1 / HW, resp. hsig') in f32 and stored: 3 * 2^-24 relative, plus 2^-8 for a
    bf16 pooled value.  For ds the terms are the f32 products dy * x: one more 2^-24 * sum |dy * x|."""
    B, HW = 3, 49
    rt = _pool_rt(Cc, _epc(dtype))
    k = -(-HW // rt)
    assert rt == 32 and k == 2
    g = torch.Generator().manual_seed(63)
    td = TD[dtype]
    mag = torch.ones(Cc)
    mag[1], mag[Cc - 2] = 1e-7, 3e-5
    x = _slice((torch.randn(B * HW, Cc, generator=g) * mag).to(td).cuda(), ld, 8).view(B, HW, Cc)
    dy = _slice(torch.randn(B * HW, Cc, generator=g).to(td).cuda(), ld, 8).view(B, HW, Cc)
    s = _slice((torch.randn(B, Cc, generator=g) * 0.5).to(td).cuda(), ld, 8)  # |s| < 3: hsig' = 1/6
    assert (s.float().abs() < 3).all()
    y = torch.zeros(B, Cc, device="cuda", dtype=td)
    N.check(N.lib().vt_global_avgpool_fwd(vp(x), ld, vp(y), Cc, B, HW, Cc, dtype, stream()))
    xd = x.double()
    ref, mass = xd.mean(1), xd.abs().sum(1)
    out_eps = 3 * 2.0 ** -24 + (2.0 ** -8 if dtype == N.VT_BF16 else 0.0)
    bound = (rt * 2.0 ** -33 + (k - 1) * 2.0 ** -24 * mass) / HW + out_eps * ref.abs()
    err = (y.double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max().item()
    assert (ref[:, 1].abs() < 1e-6).all() and (err[:, 1] <= 1e-2 * xd[:, :, 1].abs().mean(1)).all()  # the small channel resolves
    dx = torch.zeros(B * HW, Cc, device="cuda", dtype=td)
    ds = torch.zeros(B, Cc, device="cuda")
    N.check(N.lib().vt_ese_gate_bwd(vp(dy), ld, vp(x), ld, vp(s), ld, vp(dx), Cc, vp(ds), B, HW, Cc, 0, dtype, stream()))
    prod = dy.double() * xd
    ref, mass = prod.sum(1) / 6.0, prod.abs().sum(1)
    bound = (rt * 2.0 ** -33 + k * 2.0 ** -24 * mass) / 6.0 + 3 * 2.0 ** -24 * ref.abs()
    err = (ds.double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max().item()
