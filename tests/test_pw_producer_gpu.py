"""The producer fold of the pointwise kernels (vt_pointwise.hip, vt_pw_desc::pcoef / psums) through the C-ABI, and the
CSPDarknet-53 program that uses it.

A pointwise launch that is the only reader of a BatchNorm unit's output y0 reads that unit's stored pre-activation z0
instead and applies y0 = act(z0 * scale + shift), rounded to bf16, as it loads; its backward launch, where it is the only
writer of d(y0), also forms the producer's BatchNorm-backward sums.  y0 comes from the library's own vt_bn_act_apply on z0.

1. Bit equality with the unfolded path: the four passes with the producer operand on z0 against the same passes on the
   stored y0 -- statistics and sums buffers as raw fixed-point words, y of every group, dx; dW to the rounding of its f32
   atomics (the bound of test_apply_passes_that_finalize_for_themselves_are_bit_identical); the coefficients and running
   statistics of the in-prologue finalize against vt_bn_finalize.
2. Parity that counts: the float64 reference of test_pointwise_unit_matches_float64_reference built on y0, with that
   test's tolerances; the producer's sums against float64 on the dx the kernel stored and against the separate
   vt_bn_act_bwd_reduce on the same operands, with the bounds of test_dgrad_bnred_gpu.py (1e-5 / 2e-5 of the column's
   absolute sum).

Every case has a producer channel with scale exactly 0, one with a negative scale and one whose shift masks every pixel.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vision_toolbox import _native as N

from gpu_util import rel_err, stream, vp

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _lib_loaded():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


def _rows(M, Cc, slack, gen, scale=1.0, shift=0.0):
    """[M][Cc] bf16 rows inside a wider NaN-filled buffer when slack > 0 (a channel slice of a concat buffer)"""
    wide = torch.full((M, Cc + slack), float("nan"), device="cuda", dtype=BF)
    view = wide[:, slack // 2: slack // 2 + Cc] if slack else wide
    view.copy_((torch.randn(M, Cc, device="cuda", generator=gen) * scale + shift).to(BF))
    return view


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _vps(ts):
    return _arr(C.c_void_p, [C.c_void_p(t.data_ptr()) if t is not None else None for t in ts])


def _desc(x, ws, relu, pcoef=None, pact=0, psums=None):
    d = N.PwDesc()
    d.dtype, d.K, d.ngroups, d.relu, d.M = N.VT_BF16, ws[0].shape[1], len(ws), int(relu), x.shape[0]
    d.x, d.ldx = x.data_ptr(), x.stride(0)
    for g, w in enumerate(ws):
        d.C[g], d.w[g], d.ldw[g] = w.shape[0], w.data_ptr(), w.stride(0)
    if pcoef is not None:
        d.pcoef, d.pact = pcoef.data_ptr(), int(pact)
    if psums is not None:
        d.psums = psums.data_ptr()
    return d


SHAPES = [
    # (M, K, [C per group], slack of x)
    (592, 32, [32], 0),
    (1000, 64, [32, 32], 0),   # the stage-0 pair; tail tile: 1000 = 62 * 16 + 8
    (2085, 64, [64], 32),      # x is a channel slice (ld > K)
    (40, 64, [32, 32], 0),     # M < 64: some waves have no unit
]


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "no_act"])
@pytest.mark.parametrize("pact", [1, 0], ids=["prod_relu", "prod_no_act"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"M{s[0]}_K{s[1]}_C{'+'.join(map(str, s[2]))}_s{s[3]}")
def test_passes_on_the_pre_activation_equal_the_passes_on_the_stored_output(shape, pact, relu):
    M, K, Cs, slack = shape
    G, Nn = len(Cs), sum(Cs)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(M * 7 + K + 2 * pact + relu)
    lib, st = N.lib(), stream()
    assert lib.vt_pw_supported(N.VT_BF16, K, Cs[0], Cs[1] if G > 1 else 0) == 2
    offs = [0, Cs[0]]
    ldy = _arr(C.c_int32, Cs)

    # ---- the producer: z0, its batch statistics (spread over two replicas), its BatchNorm parameters ----------------------
    z0 = _rows(M, K, slack, gen, 1.5, 0.3)
    z64 = z0.double()
    pstats = N.stats_buffer(K)
    half = M // 2
    N.stats_encode(pstats, 0, z64[:half].sum(0), 0)
    N.stats_encode(pstats, 0, z64[half:].sum(0), 5)
    N.stats_encode(pstats, 1, (z64 * z64)[:half].sum(0), 3)
    N.stats_encode(pstats, 1, (z64 * z64)[half:].sum(0), 15)
    pgamma = torch.rand(K, device="cuda", generator=gen) + 0.5
    pbeta = torch.randn(K, device="cuda", generator=gen) * 0.3
    pgamma[1] = 0.0     # scale exactly 0
    pgamma[2] = -0.75   # a negative scale
    pgamma[3], pbeta[3] = 0.01, -6.0  # the shift masks every pixel (under the producer's ReLU)

    def producer_state():
        return (torch.full((4, K), float("nan"), device="cuda"), torch.full((K,), 0.1, device="cuda"),
                torch.full((K,), 0.9, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda"))

    # reference: vt_bn_finalize, then the library's own normalise pass stores y0
    pc_ref, rm_ref, rv_ref, nbt_ref = producer_state()
    N.check(lib.vt_bn_finalize(vp(pstats), K, float(M), vp(pgamma), vp(pbeta), 1e-5, 0.1, vp(rm_ref), vp(rv_ref), vp(nbt_ref),
                               pc_ref[0].data_ptr(), pc_ref[1].data_ptr(), pc_ref[2].data_ptr(), pc_ref[3].data_ptr(), st))
    y0 = torch.full((M, K), float("nan"), device="cuda", dtype=BF)
    N.check(lib.vt_bn_act_apply(vp(z0), z0.stride(0), pc_ref[0].data_ptr(), pc_ref[1].data_ptr(), None, 0, vp(y0), K, M, K, pact,
                                N.VT_BF16, st))
    torch.cuda.synchronize()
    assert pc_ref[0, 1].item() == 0.0 and pc_ref[0, 2].item() < 0
    if pact:
        assert (y0[:, 3] == 0).all()

    ws = [(torch.randn(c, K, device="cuda", generator=gen) * (2.0 / K) ** 0.5).to(BF) for c in Cs]
    d_ref = _desc(y0, ws, relu)

    # ---- statistics: in-prologue finalize of the producer, and the separate-finalize route ---------------------------------
    stats_ref = [N.stats_buffer(c) for c in Cs]
    N.check(lib.vt_pw_fwd_stats(C.byref(d_ref), _vps(stats_ref), st))
    pc, rm, rv, nbt = producer_state()
    d = _desc(z0, ws, relu, pc, pact)
    stats = [N.stats_buffer(c) for c in Cs]
    pfin = N.BnFinFwd(pstats.data_ptr(), float(M), pgamma.data_ptr(), pbeta.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(),
                      nbt.data_ptr())
    before = N.launch_count()
    N.check(lib.vt_pw_fwd_stats_finalize(C.byref(d), C.byref(pfin), _vps(stats), st))
    torch.cuda.synchronize()
    assert N.launch_count() - before == 1
    for a, b in ((pc, pc_ref), (rm, rm_ref), (rv, rv_ref), (nbt, nbt_ref)):
        assert torch.equal(a, b)  # coefficients, running statistics, batch counter: vt_bn_finalize bit for bit
    stats_alt = [N.stats_buffer(c) for c in Cs]
    N.check(lib.vt_pw_fwd_stats(C.byref(_desc(z0, ws, relu, pc_ref, pact)), _vps(stats_alt), st))
    for a, b, c in zip(stats, stats_alt, stats_ref):
        assert torch.equal(a, c) and torch.equal(b, c)  # raw fixed-point words

    # float64 on y0 (the reference of test_pointwise_unit_matches_float64_reference)
    W = torch.cat(ws, 0).double()
    zb = (y0.double() @ W.T).to(BF).double()
    got = torch.cat([N.stats_decode(s) for s in stats], 1)
    ref = torch.stack([zb.sum(0), (zb * zb).sum(0)])
    assert ((got - ref).abs() / ref.abs().max(1, keepdim=True).values).max().item() < 1e-3

    # ---- normalise ------------------------------------------------------------------------------------------------------
    mean = zb.mean(0)
    invstd = 1.0 / torch.sqrt(zb.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(Nn, device="cuda", generator=gen).double() + 0.5
    beta = torch.randn(Nn, device="cuda", generator=gen).double() * 0.3
    coef = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]).float().contiguous()
    scale, shift, mean, invstd = [c.double() for c in coef]  # what the kernels read

    def apply(desc):
        ys = [torch.full((M, c), float("nan"), device="cuda", dtype=BF) for c in Cs]
        N.check(lib.vt_pw_fwd_apply(C.byref(desc), coef.data_ptr(), _vps(ys), ldy, _vps([None] * G), _arr(C.c_int32, [0] * G), st))
        return ys

    ys_ref, ys = apply(d_ref), apply(d)
    torch.cuda.synchronize()
    pre = zb * scale + shift
    yref = torch.relu(pre) if relu else pre
    for g, c in enumerate(Cs):
        assert torch.equal(ys[g], ys_ref[g])
        r = yref[:, offs[g]: offs[g] + c]
        assert rel_err(ys[g], r) < 4e-3
        assert ((ys[g].double() - r).abs() / (r.abs() + 1.0)).max().item() < 0.05

    # ---- backward reduction ---------------------------------------------------------------------------------------------
    dys = [_rows(M, c, 0, gen) for c in Cs]

    def reduce(desc):
        sums = [N.stats_buffer(c) for c in Cs]
        N.check(lib.vt_pw_bwd_reduce(C.byref(desc), coef.data_ptr(), _vps(dys), ldy, _vps(sums), st))
        return sums

    sums_ref, sums = reduce(d_ref), reduce(d)
    for a, b in zip(sums, sums_ref):
        assert torch.equal(a, b)
    dy = torch.cat([t.double() for t in dys], 1)
    g_ = dy * (pre > 0) if relu else dy
    got = torch.cat([N.stats_decode(s) for s in sums], 1)
    ref = torch.stack([g_.sum(0), (g_ * (zb - mean) * invstd).sum(0)])
    assert ((got - ref).abs() / ref.abs().max(1, keepdim=True).values.clamp_min(1.0)).max().item() < 3e-3

    # ---- backward apply: dx, dW, and the producer's sums -------------------------------------------------------------------
    b_ = torch.randn(Nn, device="cuda", generator=gen) * 0.05
    d_ = torch.randn(Nn, device="cuda", generator=gen) * 0.05
    bcoefs = [torch.stack([coef[0, o: o + c], b_[o: o + c], d_[o: o + c]]).contiguous() for o, c in zip(offs, Cs)]

    def bwd(desc, addend=None):
        dx = torch.full((M, K), float("nan"), device="cuda", dtype=BF)
        dws = [torch.full((c, K), 0.5, device="cuda") for c in Cs]
        rc = lib.vt_pw_bwd_apply(C.byref(desc), coef.data_ptr(), _vps(dys), ldy, _vps(bcoefs), dx.data_ptr(), K,
                                 addend.data_ptr() if addend is not None else None, K, _vps(dws), _arr(C.c_int32, [K] * G),
                                 _vps([None] * G), _arr(C.c_int32, [0] * G), st)
        return rc, dx, dws

    rc, dx_ref, dws_ref = bwd(d_ref)
    N.check(rc)
    psums = N.stats_buffer(K)
    d_b = _desc(z0, ws, relu, pc_ref, pact, psums)
    rc, dx, dws = bwd(d_b)
    N.check(rc)
    rc, dx_a, dws_a = bwd(d)  # (the producer operand without its sums)
    N.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref) and torch.equal(dx_a, dx_ref)
    for a, a2, b in zip(dws, dws_a, dws_ref):  # (f32 atomics across workgroups: equal up to the order of the partial sums)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * b.abs().max().item())
        torch.testing.assert_close(a2, b, rtol=1e-4, atol=1e-4 * b.abs().max().item())
    a_ = torch.cat([b[0] for b in bcoefs]).double()
    dzref = (a_ * g_ - b_.double() * zb + d_.double()).to(BF).double()
    assert rel_err(dx, dzref @ W) < 4e-3
    for g, c in enumerate(Cs):
        dwref = dzref[:, offs[g]: offs[g] + c].T @ y0.double()
        assert rel_err(dws[g].double() - 0.5, dwref) < 2e-3

    # the producer's sums: against the separate pass on the stored dx, and against float64 on the stored dx
    sep = N.stats_buffer(K)
    N.check(lib.vt_bn_act_bwd_reduce(vp(dx), K, vp(z0), z0.stride(0), pc_ref[0].data_ptr(), pc_ref[1].data_ptr(),
                                     pc_ref[2].data_ptr(), pc_ref[3].data_ptr(), M, K, pact, N.VT_BF16, vp(sep), st))
    torch.cuda.synchronize()
    a, b = N.stats_decode(sep), N.stats_decode(psums)
    mask = (torch.addcmul(pc_ref[1], z0.float(), pc_ref[0]) > 0).double() if pact else torch.ones_like(z64)
    gp = dx.double() * mask
    pmu, pis = pc_ref[2].double(), pc_ref[3].double()
    ref = torch.stack([gp.sum(0), (gp * (z64 - pmu)).sum(0) * pis])
    col = torch.stack([gp.abs().sum(0), (gp * (z64 - pmu)).abs().sum(0) * pis]).clamp_min(1e-30)
    print(f"producer sums: vs separate {((b - a).abs() / col).max().item():.3e}, vs float64 {((b - ref).abs() / col).max().item():.3e}, "
          f"separate vs float64 {((a - ref).abs() / col).max().item():.3e}")
    assert ((b - a).abs() / col).max().item() < 1e-5
    assert ((b - ref).abs() / col).max().item() < 2e-5
    assert ((a - ref).abs() / col).max().item() < 2e-5
    if pact:
        assert (b[:, 3] == 0).all()  # the masked channel contributes nothing

    # with an addend the kernel is not the only writer of dx: the producer's sums are refused, the fold alone is not
    add = _rows(M, K, 0, gen, 0.5)
    rc, _, _ = bwd(d_b, add)
    assert rc == N.VT_ERR_UNSUPPORTED
    rc, dx_add, _ = bwd(d, add)
    N.check(rc)
    rc, dx_add_ref, _ = bwd(d_ref, add)
    N.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(dx_add, dx_add_ref)


def test_shapes_without_the_filter_gradient_in_the_kernel_are_refused():
    """the mode-1 shape (CSP stage 1: 128 -> 64 | 64) hands dz to the filter-gradient kernel, which needs the stored y0"""
    M, K, Cs = 2048, 128, [64, 64]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    lib, st = N.lib(), stream()
    assert lib.vt_pw_supported(N.VT_BF16, K, *Cs) == 1
    z0 = _rows(M, K, 0, gen)
    ws = [(torch.randn(c, K, device="cuda", generator=gen) * 0.1).to(BF) for c in Cs]
    pc = torch.stack([torch.ones(K), torch.zeros(K), torch.zeros(K), torch.ones(K)]).cuda().contiguous()
    d = _desc(z0, ws, 1, pc, 1)
    stats = [N.stats_buffer(c) for c in Cs]
    assert lib.vt_pw_fwd_stats(C.byref(d), _vps(stats), st) == N.VT_ERR_UNSUPPORTED
    coef = torch.stack([torch.ones(128), torch.zeros(128), torch.zeros(128), torch.ones(128)]).cuda().contiguous()
    ys = [torch.empty(M, c, device="cuda", dtype=BF) for c in Cs]
    ldy = _arr(C.c_int32, Cs)
    assert lib.vt_pw_fwd_apply(C.byref(d), coef.data_ptr(), _vps(ys), ldy, _vps([None, None]), _arr(C.c_int32, [0, 0]),
                               st) == N.VT_ERR_UNSUPPORTED
    assert lib.vt_pw_bwd_reduce(C.byref(d), coef.data_ptr(), _vps(ys), ldy, _vps(stats), st) == N.VT_ERR_UNSUPPORTED
    # (and activation codes beyond ReLU on a shape that has the kernels)
    d64 = _desc(z0[:, :64], [w[:32, :64].contiguous() for w in ws], 1, pc, 2)
    assert lib.vt_pw_fwd_stats(C.byref(d64), _vps([N.stats_buffer(32), N.stats_buffer(32)]), st) == N.VT_ERR_UNSUPPORTED
    # the same descriptor without the producer operand runs
    N.check(lib.vt_pw_fwd_stats(C.byref(_desc(z0, ws, 1)), _vps(stats), st))


# ---- model level -----------------------------------------------------------------------------------------------------------
def test_cspdarknet53_train_step_with_the_fold(golden_dir, monkeypatch):
    """CSPDarknet-53 with the fold's size threshold at 0 (stage 0: CSPDarknetStage.conv -> conv1 | conv2) against the golden
    vectors, with the tolerances of test_modules_gpu.py::test_model_bf16_tracks_reference; the forward is bit-identical to
    the unfolded program's by construction."""
    from oracle import filler
    from torch import nn
    from vision_toolbox import backbones

    gm = np.load(golden_dir / "models.npz")
    name = "cspdarknet53"
    x, y = filler.images(4, 64).cuda(), filler.labels(4, 16).cuda()

    def run(fold_mb):
        monkeypatch.setenv("VT_PW_MIN_MB", "0")
        monkeypatch.setenv("VT_PW_FOLD_MIN_MB", fold_mb)
        bb = getattr(backbones, name)()
        model = nn.Sequential(bb, nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), nn.Linear(bb.get_last_out_channels(), 16))
        filler.fill_module(model, name + ".")
        bb.compute_dtype = torch.bfloat16
        model = model.cuda().train()
        logits = model[3](model[2](model[1](model[0](x).float())))
        loss = F.cross_entropy(logits, y, label_smoothing=0.1)
        loss.backward()
        torch.cuda.synchronize()
        hist = dict(bb._vt_runner().program(x, N.VT_BF16, True, True).kind_histogram)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items() if "running" in k}
        return logits.detach(), loss.item(), dict(model.named_parameters()), hist, sd

    logits, loss, params, hist, sd = run("0")
    logits0, loss0, _, hist0, sd0 = run("1e9")
    assert hist["bn_fin_apply"] == hist0["bn_fin_apply"] - 1 and hist["bn_bwd_reduce"] == hist0["bn_bwd_reduce"] - 1
    assert torch.equal(logits, logits0) and loss == loss0
    for k in sd:
        assert torch.equal(sd[k], sd0[k]), k
    assert loss == pytest.approx(float(gm[f"{name}.train.loss"]), rel=5e-2)
    keys = list(gm[f"{name}.train.grad_keys"])
    norms = gm[f"{name}.train.grad_norms"]
    got = np.array([params[k].grad.double().norm().item() for k in keys])
    big = norms > 1e-3 * norms.max()
    assert np.median(np.abs(got[big] / norms[big] - 1)) < 0.15
