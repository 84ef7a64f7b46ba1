"""The gradient-norm, clipping and LAMB kernels through the C-ABI, against the float64 yardstick of tests/lamb_util.py.
The bounds are the counted ones of that module (C_NORM, C_SUM, C_U in units of 2^-24) and the AdamW kernel's elementwise
rtol = atol = 1e-6; tests/test_lamb_cpu.py holds a float32 restatement of the same arithmetic on the same inputs below half
of each.  Every test prints its figures before it asserts; NOTEBOOK.md section "LAMB and clipping" records them."""
import math

import numpy as np
import pytest
import torch

from oracle import filler
from vision_toolbox import _native as N

import lamb_util as LU
from gpu_util import stream, vp

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64  # NaN-filled elements in front of and behind every operand


def _in_nan(t: torch.Tensor, dtype=None) -> torch.Tensor:
    """a device copy of `t` inside a NaN-filled allocation (the view keeps 256-byte alignment)"""
    buf = torch.full((t.numel() + 2 * PAD,), NAN, device="cuda", dtype=dtype or t.dtype)
    buf[PAD: PAD + t.numel()] = t.to(buf.dtype)
    return buf


def _norm(g_buf, n, s, C, M):
    """vt_grad_sumsq + vt_clip_coef over g_buf[PAD: PAD + n] -> (N, factor, partials, ctl), with the guards checked"""
    L = N.lib()
    items = N.opt_items(n)
    part = torch.full((items + 2,), NAN, device="cuda", dtype=torch.float64)
    ctl = torch.full((16,), NAN, device="cuda")
    ctl[:4] = torch.tensor([C, M, NAN, NAN])
    keep = g_buf.clone()
    N.check(L.vt_grad_sumsq(vp(g_buf[PAD:]), n, vp(part[1:]), stream()))
    N.check(L.vt_clip_coef(vp(part[1:]), items, s, vp(ctl), stream()))
    torch.cuda.synchronize()
    assert torch.equal(g_buf.view(torch.int32), keep.view(torch.int32))  # the gradient is only read
    assert math.isnan(part[0].item()) and math.isnan(part[-1].item()) and ctl[4:].isnan().all()
    assert ctl[0].item() == np.float32(C) and ctl[1].item() == np.float32(M)  # thresholds are only read
    return ctl[N.VT_CTL_NORM].item(), ctl[N.VT_CTL_FACTOR].item(), part[1:-1].cpu(), ctl.cpu()


# ---- vt_grad_sumsq + vt_clip_coef ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LU.SUMSQ_LENGTHS)
def test_grad_norm_of_every_length(n):
    g = LU.sumsq_input(n)
    want = float(LU.grad_norm([g.double()]))
    buf = _in_nan(g)
    before = N.launch_count()
    got, factor, part, ctl = _norm(buf, n, 1.0, 0.0, 0.0)
    assert N.launch_count() == before + 2
    rel = abs(got - want) / want
    print(f"n={n}: N {got!r} against {want!r}: {rel / LU.U24:.2f} u (bound {LU.C_NORM} u), {part.numel()} partials")
    assert LU.C_NORM * LU.U24 <= 1e-5
    assert rel <= LU.C_NORM * LU.U24
    assert factor == 1.0  # both thresholds off: exactly grad_scale
    # one partial per item, each the sum over its own elements (the last one over the tail only)
    assert part.numel() == N.opt_items(n)
    for i in (0, part.numel() - 1):
        w = float((g[i * LU.I: (i + 1) * LU.I].double() ** 2).sum())
        assert abs(part[i].item() - w) <= 16 * LU.U24 * w
    # bit-identical from run to run
    got2, factor2, part2, ctl2 = _norm(buf, n, 1.0, 0.0, 0.0)
    assert torch.equal(part, part2) and torch.equal(ctl[:4].view(torch.int32), ctl2[:4].view(torch.int32))


def test_clip_factor_cases():
    n = 3 * LU.I + 8
    g = LU.sumsq_input(n)
    buf = _in_nan(g)
    n1 = float(LU.grad_norm([g.double()]))
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (the thresholds as the device holds them)
    inf = float("inf")
    cases = [  # (tag, s, C, M)
        ("both off", 1.0, 0.0, 0.0), ("off as inf / negative", 1.0, inf, -1.0), ("C above N", 1.0, f32(2 * n1), 0.0),
        ("C below N", 1.0, f32(n1 / 2), 0.0), ("M above N'", 1.0, 0.0, f32(2 * n1)), ("M below N'", 1.0, 0.0, f32(n1 / 3)),
        ("both active", 1.0, f32(n1 / 2), f32(n1 / 8)), ("C active, M above N'", 1.0, f32(n1 / 2), f32(n1)),
        ("grad_scale 0.5, off", 0.5, 0.0, 0.0), ("grad_scale 0.5, C between", 0.5, f32(0.75 * n1), 0.0),
        ("grad_scale 0.5, both", 0.5, f32(n1 / 4), f32(n1 / 16)),
    ]
    for tag, s, C, M in cases:
        got_n, got_f, _, _ = _norm(buf, n, s, C, M)
        c1, c2 = LU.clip_factors(s * n1, C, M)
        want_f = s * c1 / c2
        rel_n, rel_f = abs(got_n - s * n1) / (s * n1), abs(got_f - want_f) / want_f
        print(f"{tag}: N {got_n!r} ({rel_n / LU.U24:.2f} u), factor {got_f!r} against {want_f!r} ({rel_f / LU.U24:.2f} u), "
              f"c1 {c1:.6f} c2 {c2:.6f}")
        assert rel_n <= LU.C_NORM * LU.U24
        if c1 == 1.0 and c2 == 1.0:
            assert got_f == s  # nothing clips: exactly grad_scale
        else:
            assert rel_f <= LU.C_NORM * LU.U24 and got_f < s
    # (the cases did what their names say)
    assert LU.clip_factors(n1, f32(n1 / 2), f32(n1))[1] == 1.0 and LU.clip_factors(0.5 * n1, f32(0.75 * n1), 0.0)[0] == 1.0


def test_a_nan_gradient_element():
    n = LU.I + 4
    g = LU.sumsq_input(n).clone()
    g[n - 2] = NAN
    buf = _in_nan(g)
    got_n, got_f, part, _ = _norm(buf, n, 0.5, 1.0, 1.0)
    assert math.isnan(got_n) and math.isnan(got_f)  # c1 is NaN, as torch.clamp keeps it
    assert not math.isnan(part[0].item()) and math.isnan(part[1].item())
    got_n, got_f, _, _ = _norm(buf, n, 0.5, 0.0, 1.0)
    assert math.isnan(got_n) and got_f == 0.5  # c2's comparison is false: 1


# ---- vt_sgd_momentum_clip / vt_adamw_clip -----------------------------------------------------------------------------------
def _run_opt(name, clip, n, p0, grads, factor, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.05, mu=0.9):
    """five steps of the plain entry (clip=False: `factor` is the immediate grad_scale) or its *_clip twin (`factor` comes
    from a device scalar), as tests/test_adamw_gpu.py runs vt_adamw"""
    n_pad = (n + 3) // 4 * 4
    p, m, v = (torch.zeros(n_pad, device="cuda") for _ in range(3))
    p[:n] = p0.cuda()
    mirror = torch.zeros(n_pad, device="cuda", dtype=torch.bfloat16)
    hyper = torch.zeros(16, device="cuda")
    hyper[:4] = lr
    coef = torch.full((8,), NAN, device="cuda")
    coef[2] = factor
    L = N.lib()
    for g in grads:
        gd = torch.zeros(n_pad, device="cuda")
        gd[:n] = g.cuda()
        if name == "SGD":
            if clip:
                N.check(L.vt_sgd_momentum_clip(vp(p), vp(gd), vp(m), vp(mirror), N.VT_BF16, n, 0.0, mu, wd, vp(coef[2:]),
                                               vp(hyper), stream()))
            else:
                N.check(L.vt_sgd_momentum(vp(p), vp(gd), vp(m), vp(mirror), N.VT_BF16, n, 0.0, mu, wd, factor, vp(hyper),
                                          stream()))
            continue
        N.check(L.vt_adam_tick(vp(hyper), betas[0], betas[1], stream()))
        if clip:
            N.check(L.vt_adamw_clip(vp(p), vp(gd), vp(m), vp(v), vp(mirror), N.VT_BF16, n, betas[0], betas[1], eps, wd,
                                    vp(coef[2:]), int(name == "AdamW"), vp(hyper), stream()))
        else:
            N.check(L.vt_adamw(vp(p), vp(gd), vp(m), vp(v), vp(mirror), N.VT_BF16, n, betas[0], betas[1], eps, wd, factor,
                               int(name == "AdamW"), vp(hyper), stream()))
    torch.cuda.synchronize()
    return p[:n].cpu(), m[:n].cpu(), v[:n].cpu(), mirror[:n].cpu()


@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_clipped_entries_against_the_plain_ones_and_torch(name):
    n = 100_003  # tests/test_adamw_gpu.py's case (odd tail: n % 4 == 3)
    p0 = filler.tensor("adamw.p", (n,))
    grads = [s * filler.tensor(f"adamw.g{k}", (n,)) for k, s in enumerate([1.0, -0.5, 2.0, 0.25, -1.5])]
    # the factor equal to grad_scale: the same bits as the unclipped entry
    for gs in (1.0, 0.5):
        plain, clipped = _run_opt(name, False, n, p0, grads, gs), _run_opt(name, True, n, p0, grads, gs)
        for a, b in zip(plain, clipped):
            assert torch.equal(a, b)
    # a factor of 0.37 against float64 torch fed 0.37 g
    f = float(np.float32(0.37))
    p, m, v, mir = _run_opt(name, True, n, p0, grads, f)
    ref = torch.nn.Parameter(p0.double())
    if name == "SGD":
        opt = torch.optim.SGD([ref], lr=1e-3, momentum=0.9, weight_decay=0.05)
    else:
        opt = getattr(torch.optim, name)([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    for g in grads:
        ref.grad = f * g.double()
        opt.step()
    st = opt.state[ref]
    pairs = [("p", p, ref.data), ("m", m, st["momentum_buffer" if name == "SGD" else "exp_avg"])]
    if name != "SGD":
        pairs.append(("v", v, st["exp_avg_sq"]))
    for tag, got, want in pairs:
        d = (got.double() - want).abs()
        print(f"{name} clipped, factor 0.37: {tag} worst |diff| {d.max().item():.3e}, outside the bound "
              f"{(d > 1e-6 + 1e-6 * want.abs()).sum().item()} of {n}")
        torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-6)
    assert torch.equal(mir, p.to(torch.bfloat16))


# ---- LAMB -------------------------------------------------------------------------------------------------------------------
class _LambRun:
    def __init__(self, variant, mirror_dtype=torch.bfloat16):
        self.trust, self.adapt, self.M = LU.LAMB_VARIANTS[variant]
        self.offs, self.n_total = LU.lamb_offsets()
        self.lo, self.hi = self.offs[0], self.offs[-1] + LU.LAMB_SIZES[-1]
        table, self.n_items = N.lamb_table(self.offs, LU.LAMB_SIZES, LU.LAMB_WD)
        self.table = torch.from_numpy(table).cuda()
        dev = lambda dt=torch.float32: torch.full((self.n_total,), NAN, device="cuda", dtype=dt)  # noqa: E731
        self.p, self.g, self.m, self.v = dev(), dev(), dev(), dev()
        self.mirror = dev(mirror_dtype) if mirror_dtype is not None else None
        self.mirror_code = N.VT_F32 if mirror_dtype == torch.float32 else N.VT_BF16
        self.m[self.lo: self.hi] = 0
        self.v[self.lo: self.hi] = 0
        self.part = torch.full((2 * self.n_items + 4,), NAN, device="cuda", dtype=torch.float64)
        self.sq = torch.full((N.opt_items(self.hi - self.lo) + 2,), NAN, device="cuda", dtype=torch.float64)
        self.hyper = torch.zeros(16, device="cuda")
        self.hyper[:4] = LU.LAMB_LR
        self.ctl = torch.zeros(8, device="cuda")
        self.ctl[N.VT_CTL_LAMB_MAX] = 0.0 if self.M is None else self.M
        self.flags = (N.VT_LAMB_TRUST_CLIP if self.trust else 0) | (N.VT_LAMB_ALWAYS_ADAPT if self.adapt else 0)

    def put(self, buf, tensors):
        for o, t in zip(self.offs, tensors):
            buf[o: o + t.numel()] = t.cuda()

    def get(self, buf):
        return [buf[o: o + n].float().cpu() for o, n in zip(self.offs, LU.LAMB_SIZES)]

    def step(self, grads):
        L = N.lib()
        self.put(self.g, grads)
        n = self.hi - self.lo
        N.check(L.vt_adam_tick(vp(self.hyper), *LU.LAMB_BETAS, stream()))
        N.check(L.vt_grad_sumsq(vp(self.g[self.lo:]), n, vp(self.sq[1:]), stream()))
        N.check(L.vt_clip_coef(vp(self.sq[1:]), N.opt_items(n), 1.0, vp(self.ctl), stream()))
        N.check(L.vt_lamb_moments(vp(self.p), vp(self.g), vp(self.m), vp(self.v), vp(self.table), len(self.offs), self.n_items,
                                  self.n_total, vp(self.part[2:]), vp(self.ctl[N.VT_CTL_FACTOR:]), *LU.LAMB_BETAS, LU.LAMB_EPS,
                                  self.flags, vp(self.hyper), stream()))
        N.check(L.vt_lamb_apply(vp(self.p), vp(self.m), vp(self.v), vp(self.mirror), self.mirror_code, vp(self.table),
                                len(self.offs), self.n_items, self.n_total, vp(self.part[2:]), LU.LAMB_EPS, self.flags,
                                vp(self.hyper), stream()))

    def sums(self):
        """(sum p^2, sum u^2) per tensor: its partials added on the host in double"""
        part = self.part[2:-2].cpu().view(-1, 2)
        out, i = [], 0
        for n in LU.LAMB_SIZES:
            c = N.opt_items(n)
            out.append((float(part[i: i + c, 0].sum()), float(part[i: i + c, 1].sum())))
            i += c
        assert i == self.n_items
        return out


def _lamb_five_steps(variant, mirror_dtype=torch.bfloat16):
    p0, grads = LU.lamb_inputs()
    run = _LambRun(variant, mirror_dtype)
    run.put(run.p, p0)
    for k, g in enumerate(grads):
        if k == len(grads) - 1:
            torch.cuda.synchronize()
            p_before = run.get(run.p)
        run.step(g)
    torch.cuda.synchronize()
    return run, p_before


@pytest.mark.parametrize("variant", list(LU.LAMB_VARIANTS))
def test_lamb_five_steps_against_float64(variant):
    p0, grads = LU.lamb_inputs()
    trust, adapt, M = LU.LAMB_VARIANTS[variant]
    ref = LU.Lamb([p.double() for p in p0], LU.LAMB_WD, lr=LU.LAMB_LR, betas=LU.LAMB_BETAS, eps=LU.LAMB_EPS, M=M,
                  trust_clip=trust, always_adapt=adapt)
    for g in grads:
        info = ref.step([x.double() for x in g])
    before = N.launch_count()
    run, p_before = _lamb_five_steps(variant)
    assert N.launch_count() == before + 5 * len(grads)
    for tag, buf, want in (("p", run.p, ref.p), ("m", run.m, ref.m), ("v", run.v, ref.v)):
        got = run.get(buf)
        worst = max(((a.double() - b).abs() / (LU.ATOL + LU.RTOL * b.abs())).max().item() for a, b in zip(got, want))
        print(f"{variant}: {tag} at {worst:.3f} of the elementwise bound")
        for a, b in zip(got, want):
            torch.testing.assert_close(a.double(), b, rtol=LU.RTOL, atol=LU.ATOL)
    assert (M is None) == (info["c2"] == 1.0)
    assert abs(run.ctl[N.VT_CTL_FACTOR].item() - info["factor"]) <= LU.C_NORM * LU.U24 * info["factor"]
    # each tensor's two sums of the last step, from the kernel's own float32 operands
    bc1, bc2s = run.hyper[5].item(), run.hyper[6].item()
    assert int(run.hyper[4:5].view(torch.int32).item()) == len(grads)
    m, v = run.get(run.m), run.get(run.v)
    for k, (sp, su) in enumerate(run.sums()):
        want_p = float((p_before[k].double() ** 2).sum())
        u = LU.lamb_u(p_before[k].double(), m[k].double(), v[k].double(), bc1, bc2s, LU.LAMB_EPS, LU.LAMB_WD[k])
        want_u = float((u ** 2).sum())
        bound_u = LU.sum_u_bound(p_before[k], m[k], v[k], bc1, bc2s, LU.LAMB_EPS, LU.LAMB_WD[k])
        print(f"{variant}: tensor {k}: sum p^2 {sp!r} ({abs(sp - want_p) / max(want_p, 1e-300) / LU.U24:.2f} u of {LU.C_SUM}), "
              f"sum u^2 {su!r} (at {abs(su - want_u) / bound_u:.3f} of its bound)")
        assert abs(sp - want_p) <= LU.C_SUM * LU.U24 * want_p
        assert abs(su - want_u) <= bound_u
    # the mirror is the RNE cast of the new weights; nothing outside the table's range was written; g was only read
    assert torch.equal(run.mirror[run.lo: run.hi], run.p[run.lo: run.hi].to(torch.bfloat16))
    for buf in (run.p, run.m, run.v, run.mirror):
        assert buf[: run.lo].isnan().all() and buf[run.hi:].isnan().all() and not buf[run.lo: run.hi].isnan().any()
    assert torch.equal(torch.cat(run.get(run.g)), torch.cat(grads[-1])) and run.g[: run.lo].isnan().all()
    assert run.part[:2].isnan().all() and run.part[-2:].isnan().all()
    # bit-identical from run to run
    again, _ = _lamb_five_steps(variant)
    for a, b in ((run.p, again.p), (run.m, again.m), (run.v, again.v), (run.mirror, again.mirror)):
        assert torch.equal(a[run.lo: run.hi], b[run.lo: run.hi])
    assert torch.equal(run.part[2:-2], again.part[2:-2]) and torch.equal(run.ctl, again.ctl)


def test_lamb_special_segments_and_mirror_kinds():
    """all-zero weights move by the plain step (r = 1); zero gradient and state leave u = wd p; the f32 mirror and no
    mirror give the same weights as the bf16 one"""
    p0, grads = LU.lamb_inputs()
    runs = {}
    for md in (torch.bfloat16, torch.float32, None):
        run = _LambRun("plain", md)
        run.put(run.p, p0)
        run.step(grads[0])
        torch.cuda.synchronize()
        runs[md] = run
    a = runs[torch.bfloat16]
    p, m, v = a.get(a.p), a.get(a.m), a.get(a.v)
    bc1, bc2s = a.hyper[5].item(), a.hyper[6].item()
    k = LU.LAMB_ZERO_P
    u = LU.lamb_u(p0[k].double(), m[k].double(), v[k].double(), bc1, bc2s, LU.LAMB_EPS, LU.LAMB_WD[k])
    torch.testing.assert_close(p[k].double(), -LU.LAMB_LR * u, rtol=LU.RTOL, atol=LU.ATOL)  # r = 1, not 0 / ||u||
    assert a.sums()[k][0] == 0.0 and a.sums()[k][1] > 0.0
    k = LU.LAMB_ZERO_G
    assert not m[k].any() and not v[k].any()
    torch.testing.assert_close(p[k].double(), p0[k].double() * (1 - LU.LAMB_LR), rtol=LU.RTOL, atol=LU.ATOL)  # r = 1 / wd
    for md in (torch.float32, None):
        assert torch.equal(runs[md].p[a.lo: a.hi], a.p[a.lo: a.hi])
    f = runs[torch.float32]
    assert torch.equal(f.mirror[a.lo: a.hi], f.p[a.lo: a.hi]) and f.mirror[: a.lo].isnan().all()


def test_a_table_entry_outside_the_buffers_is_not_addressed():
    """the kernels check a segment against n_total before they address anything with it: NaN partials, no update (the
    allocations here are larger than the n_total the calls declare)"""
    n = 256
    p, g, m, v = (torch.ones(n + 512, device="cuda") for _ in range(4))
    table, items = N.lamb_table([0, 128], [128, 192], [0.05, 0.05])  # the second segment ends at 320 > n_total = 256
    table = torch.from_numpy(table).cuda()
    part = torch.zeros(2 * items, device="cuda", dtype=torch.float64)
    hyper = torch.zeros(16, device="cuda")
    hyper[:4] = 1e-3
    ctl = torch.ones(8, device="cuda")
    L = N.lib()
    N.check(L.vt_adam_tick(vp(hyper), 0.9, 0.999, stream()))
    N.check(L.vt_lamb_moments(vp(p), vp(g), vp(m), vp(v), vp(table), 2, items, n, vp(part), vp(ctl[2:]), 0.9, 0.999, 1e-6, 0,
                              vp(hyper), stream()))
    N.check(L.vt_lamb_apply(vp(p), vp(m), vp(v), None, N.VT_BF16, vp(table), 2, items, n, vp(part), 1e-6, 0, vp(hyper),
                            stream()))
    torch.cuda.synchronize()
    assert not part[:2].isnan().any() and part[2:].isnan().all()
    assert (p[:128] != 1).all() and (p[128:] == 1).all() and (m[128:] == 1).all() and (v[128:] == 1).all()


def test_entries_refuse_bad_arguments():
    L = N.lib()
    f = torch.zeros(256, device="cuda")
    d = torch.zeros(64, device="cuda", dtype=torch.float64)
    t = torch.zeros(64, device="cuda", dtype=torch.int32)
    hyper, ctl = torch.zeros(16, device="cuda"), torch.zeros(8, device="cuda")
    bad = N.VT_ERR_INVALID
    assert L.vt_grad_sumsq(vp(f[1:]), 64, vp(d), stream()) == bad  # not 16-byte aligned
    assert L.vt_grad_sumsq(None, 64, vp(d), stream()) == bad and L.vt_grad_sumsq(vp(f), 64, None, stream()) == bad
    assert L.vt_grad_sumsq(vp(f), 0, vp(d), stream()) == bad
    assert L.vt_clip_coef(vp(d), 1, 1.0, None, stream()) == bad and L.vt_clip_coef(None, 1, 1.0, vp(ctl), stream()) == bad
    assert L.vt_clip_coef(vp(d), 1, 1.0, vp(ctl[1:]), stream()) == bad
    sgd = lambda p, coef: L.vt_sgd_momentum_clip(p, vp(f), vp(f), None, N.VT_BF16, 64, 0.1, 0.9, 0.0, coef, None, stream())  # noqa: E731
    assert sgd(vp(f), None) == bad and sgd(vp(f[1:]), vp(ctl)) == bad
    adam = lambda p, coef, h: L.vt_adamw_clip(p, vp(f), vp(f), vp(f), None, N.VT_BF16, 64, 0.9, 0.999, 1e-8, 0.0, coef, 1, h,  # noqa: E731
                                              stream())
    assert adam(vp(f), None, vp(hyper)) == bad and adam(vp(f), vp(ctl), None) == bad and adam(vp(f[1:]), vp(ctl), vp(hyper)) == bad
    mom = lambda p, tab, coef, h: L.vt_lamb_moments(p, vp(f), vp(f), vp(f), tab, 1, 1, 64, vp(d), coef, 0.9, 0.999, 1e-6, 0, h,  # noqa: E731
                                                    stream())
    assert mom(vp(f[1:]), vp(t), vp(ctl), vp(hyper)) == bad and mom(vp(f), None, vp(ctl), vp(hyper)) == bad
    assert mom(vp(f), vp(t), None, vp(hyper)) == bad and mom(vp(f), vp(t), vp(ctl), None) == bad
    assert mom(vp(f), vp(t[1:]), vp(ctl), vp(hyper)) == bad
    app = lambda p, tab, h, mir=None: L.vt_lamb_apply(p, vp(f), vp(f), mir, N.VT_BF16, tab, 1, 1, 64, vp(d), 1e-6, 0, h,  # noqa: E731
                                                      stream())
    assert app(vp(f[1:]), vp(t), vp(hyper)) == bad and app(vp(f), None, vp(hyper)) == bad and app(vp(f), vp(t), None) == bad
    assert app(vp(f), vp(t), vp(hyper), vp(torch.zeros(64, device="cuda", dtype=torch.bfloat16)[1:])) == bad
    torch.cuda.synchronize()
