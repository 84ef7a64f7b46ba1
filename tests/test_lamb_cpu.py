"""LAMB and global-norm clipping without a GPU: the float64 yardstick of tests/lamb_util.py against torch itself, the
optimiser launch lists TrainStep builds for the new arguments (plan_only, device="cpu"), and the float32 restatement of
each kernel's arithmetic against half of every bound the GPU tests use (the rule of tests/test_head_neck_refs_cpu.py)."""
import ctypes
import math
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import ConvNeXt
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import lamb_util as LU

WD, NORM_WD, BIAS_WD = 0.05, 0.01, 0.02


# ---- the yardstick itself ---------------------------------------------------------------------------------------------
def _tensors(tag, shapes=((7, 5), (33,), (4, 3, 3, 3))):
    return [filler.tensor(f"lamb.cpu.{tag}.{k}", s).double() for k, s in enumerate(shapes)]


def test_yardstick_without_decay_and_clips_is_torch_adam():
    p0 = _tensors("p")
    ref = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.Adam(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-6)
    lamb = LU.Lamb(p0, [0.0] * 3, 1e-3, eps=1e-6, C=None, M=None)
    for step in range(5):
        g = _tensors(f"g{step}")
        for r, gg in zip(ref, g):
            r.grad = gg.clone()
        opt.step()
        info = lamb.step(g)
        assert info["r"] == [1.0] * 3 and info["factor"] == 1.0
    for k, r in enumerate(ref):
        st = opt.state[r]
        for got, want in ((lamb.p[k], r.data), (lamb.m[k], st["exp_avg"]), (lamb.v[k], st["exp_avg_sq"])):
            assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_yardstick_adapted_step_has_the_length_of_the_weights():
    p0 = _tensors("p")
    lamb = LU.Lamb(p0, [0.05, 0.0, 0.01], 1e-2, M=None, always_adapt=True)
    for step in range(3):
        before = [p.clone() for p in lamb.p]
        lamb.step(_tensors(f"g{step}"))
        for b, a in zip(before, lamb.p):
            assert abs((a - b).norm().item() / (1e-2 * b.norm().item()) - 1.0) <= 1e-12
    # without always_adapt the wd = 0 tensor takes the plain step (r = 1), and trust_clip caps r at 1
    lamb = LU.Lamb(p0, [0.05, 0.0, 0.01], 1e-2, M=None)
    assert lamb.step(_tensors("g0"))["r"][1] == 1.0
    big = [100.0 * p for p in p0]
    assert all(r > 1.0 for r in LU.Lamb(big, [0.05] * 3, 1e-2, M=None).step(_tensors("g0"))["r"])
    assert LU.Lamb(big, [0.05] * 3, 1e-2, M=None, trust_clip=True).step(_tensors("g0"))["r"] == [1.0] * 3


def test_yardstick_max_grad_norm_and_clip_grad_norm():
    p0, g = _tensors("p"), _tensors("g0")
    n0 = float(LU.grad_norm(g))
    # M active: the gradient the moments see has norm M exactly
    info = LU.Lamb(p0, [0.05] * 3, 1e-3, M=n0 / 3).step(g)
    assert abs(float(LU.grad_norm(info["used"])) / (n0 / 3) - 1.0) <= 1e-12
    # M above the norm, off (None, 0, inf): untouched
    for M in (2 * n0, None, 0.0, float("inf")):
        assert LU.Lamb(p0, [0.05] * 3, 1e-3, M=M).step(g)["factor"] == 1.0
    # C active: torch.nn.utils.clip_grad_norm_ on the same tensors
    for C in (n0 / 2, 2 * n0):
        ps = [torch.nn.Parameter(p.clone()) for p in p0]
        for p, gg in zip(ps, g):
            p.grad = gg.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, C)
        info = LU.Lamb(p0, [0.05] * 3, 1e-3, C=C, M=None).step(g)
        assert abs(info["norm"] - total.item()) <= 1e-12 * n0
        for used, p in zip(info["used"], ps):
            assert (used - p.grad).abs().max().item() <= 1e-12
    # both: LAMB's clip sees the already clipped gradient; grad_scale averages first
    info = LU.Lamb(p0, [0.05] * 3, 1e-3, s=0.5, C=n0 / 4, M=n0 / 16).step(g)
    assert abs(info["norm"] - n0 / 2) <= 1e-12 * n0
    assert abs(info["c1"] - (n0 / 4) / (n0 / 2 + 1e-6)) <= 1e-15 and abs(info["c2"] - info["c1"] * (n0 / 2) / (n0 / 16)) <= 1e-12
    assert abs(float(LU.grad_norm(info["used"])) / (n0 / 16) - 1.0) <= 1e-12
    # NaN: c1 is NaN (torch.clamp keeps it), c2's comparison is false
    c1, c2 = LU.clip_factors(float("nan"), 1.0, 1.0)
    assert math.isnan(c1) and c2 == 1.0


# ---- plans --------------------------------------------------------------------------------------------------------------
def _opt(ts):
    return [ts.opt_ops[k] for k in range(ts.n_opt)]


def _convnext_step(dtype=torch.bfloat16, **kw):
    return TrainStep(ConvNeXt(24, (1, 2)), 10, 3, 64, dtype, device="cpu", plan_only=True, lr=1e-3, weight_decay=WD,
                     norm_weight_decay=NORM_WD, bias_weight_decay=BIAS_WD, include_pool=False, **kw)


def _ptr(op, k):
    return (op.ptr[k].base, op.ptr[k].offset)


def _check_norm_ops(ts, ops, world=1):
    total = ts.store.pflat.numel()
    sumsq, coef = ops
    assert (sumsq.kind, coef.kind) == (N.OP_GRAD_SUMSQ, N.OP_CLIP_COEF)
    assert _ptr(sumsq, 0) == (E.GRADS, 0) and sumsq.ptr[1].base == E.OPTWS and int(sumsq.f[0]) == total
    assert _ptr(coef, 0) == _ptr(sumsq, 1) and _ptr(coef, 1) == (E.OPTWS, 0)
    assert int(coef.f[0]) == N.opt_items(total) and coef.f[1] == 1.0 / world
    # the partials lie behind the control floats and inside the buffer
    assert sumsq.ptr[1].offset >= 32 and sumsq.ptr[1].offset % 8 == 0
    assert sumsq.ptr[1].offset + 8 * N.opt_items(total) <= ts._optws.numel()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_lamb_optimiser_list_and_work_table(dtype):
    ts = _convnext_step(dtype, optimizer="Lamb", betas=(0.8, 0.95), eps=1e-6, trust_clip=True)
    ops = _opt(ts)
    assert [op.kind for op in ops] == [N.OP_ADAM_TICK, N.OP_GRAD_SUMSQ, N.OP_CLIP_COEF, N.OP_LAMB_MOMENTS, N.OP_LAMB_APPLY]
    assert _ptr(ops[0], 0) == (E.HYPER, 0) and (ops[0].f[0], ops[0].f[1]) == (0.8, 0.95)
    _check_norm_ops(ts, ops[1:3])
    mom, app = ops[3], ops[4]
    st = ts.store
    total, n_segs = st.pflat.numel(), len(st.params)
    factor = (E.OPTWS, 4 * N.VT_CTL_FACTOR)
    assert [_ptr(mom, k) for k in range(4)] == [(E.PARAMS, 0), (E.GRADS, 0), (E.MOMENTUM, 0), (E.MOMENT2, 0)]
    assert _ptr(mom, 6) == factor and _ptr(mom, 7) == (E.HYPER, 0)
    assert [_ptr(app, k) for k in range(3)] == [(E.PARAMS, 0), (E.MOMENTUM, 0), (E.MOMENT2, 0)]
    assert _ptr(app, 3) == ((E.MIRROR, 0) if dtype == torch.bfloat16 else (-1, 0)) and _ptr(app, 6) == (E.HYPER, 0)
    assert _ptr(mom, 4) == _ptr(app, 4) and _ptr(mom, 5) == _ptr(app, 5)  # one table, one scratch
    assert (mom.i[0], mom.i[1]) == (n_segs, N.VT_LAMB_TRUST_CLIP) and (app.i[1], app.i[2]) == (n_segs, N.VT_LAMB_TRUST_CLIP)
    assert (mom.f[2], mom.f[3], mom.f[4], app.f[2]) == (0.8, 0.95, 1e-6, 1e-6)
    # ONE table: a segment per parameter slot of the store, its decay by the three-group rule
    tab = ts.lamb_table.numpy()
    segs = tab[: 4 * n_segs].reshape(n_segs, 4)
    assert list(segs[:, 0]) == list(st.offsets) and list(segs[:, 1]) == list(st.slots)
    groups = param_groups(ts.model)
    wd_of = {GROUP_OTHER: WD, GROUP_NORM: NORM_WD, GROUP_BIAS: BIAS_WD}
    want_wd = np.array([wd_of[groups[id(p)]] for p in st.params], dtype=np.float32)
    assert np.array_equal(segs[:, 3].copy().view(np.float32), want_wd) and len(set(want_wd)) == 3
    items = [N.opt_items(n) for n in st.slots]
    assert list(segs[:, 2]) == list(np.cumsum([0] + items[:-1]))
    item_seg = tab[4 * n_segs:]
    assert list(item_seg) == [k for k, c in enumerate(items) for _ in range(c)]
    assert int(mom.f[0]) == int(app.f[0]) == len(item_seg) and int(mom.f[1]) == int(app.f[1]) == total
    assert max(items) > 1  # (a tensor of more than one item is in the plan)
    # the device copy of the table is the host one, at the offset the ops name; partials (2 doubles per item) before it
    off = mom.ptr[4].offset
    assert off % 16 == 0 and torch.equal(ts._optws[off: off + 4 * len(tab)].view(torch.int32), ts.lamb_table)
    assert mom.ptr[5].offset % 8 == 0 and mom.ptr[5].offset + 16 * len(item_seg) <= off
    assert mom.ptr[5].offset >= ops[1].ptr[1].offset + 8 * N.opt_items(total)
    # thresholds: clip off, LAMB's own at its default 1.0
    ctl = ts._optws[:32].view(torch.float32)
    assert ctl[N.VT_CTL_CLIP] == 0.0 and ctl[N.VT_CTL_LAMB_MAX] == 1.0
    assert ts.vflat is not None and ts.opt_steps() == 0
    with pytest.raises(RuntimeError, match="clip_grad_norm"):
        ts.set_clip_grad_norm(1.0)
    none = _convnext_step(dtype, optimizer="Lamb", lamb_max_grad_norm=None, always_adapt=True)
    assert none._optws[:32].view(torch.float32)[N.VT_CTL_LAMB_MAX] == 0.0
    assert _opt(none)[3].i[1] == N.VT_LAMB_ALWAYS_ADAPT


@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_clipped_optimiser_lists(name):
    ts = _convnext_step(optimizer=name, clip_grad_norm=5.0, eps=1e-6)
    plain = _convnext_step(optimizer=name, eps=1e-6)
    ops, pops = _opt(ts), _opt(plain)
    head = 1 if name != "SGD" else 0
    assert [op.kind for op in ops[:head]] == [N.OP_ADAM_TICK] * head
    _check_norm_ops(ts, ops[head: head + 2])
    upd, pupd = ops[head + 2:], pops[head:]
    kind = N.OP_SGD_CLIP if name == "SGD" else N.OP_ADAMW_CLIP
    assert [op.kind for op in upd] == [kind] * len(ts.segments) and len(upd) == len(pupd) == 3
    factor = (E.OPTWS, 4 * N.VT_CTL_FACTOR)
    nptr = 5 if name == "SGD" else 6
    for op, pop in zip(upd, pupd):
        # the same ranges, pointers and scalars as the unclipped launch; the factor pointer in the place of grad_scale
        assert [_ptr(op, k) for k in range(nptr)] == [_ptr(pop, k) for k in range(nptr)]
        assert _ptr(op, nptr) == factor and pop.ptr[nptr].base == -1
        nf = 4 if name == "SGD" else 5
        assert [op.f[k] for k in range(nf)] == [pop.f[k] for k in range(nf)] and pop.f[nf] == 1.0
        assert [op.i[k] for k in range(2)] == [pop.i[k] for k in range(2)]
    ctl = ts._optws[:32].view(torch.float32)
    assert ctl[N.VT_CTL_CLIP] == 5.0 and ctl[N.VT_CTL_LAMB_MAX] == 0.0
    ts.set_clip_grad_norm(2.5)  # a device value, like the learning rate: the list is not rebuilt
    assert ctl[N.VT_CTL_CLIP] == 2.5 and [op.kind for op in _opt(ts)] == [op.kind for op in ops]
    with pytest.raises(ValueError):
        ts.set_clip_grad_norm(-1.0)
    # inf builds the ops too (with a factor of exactly grad_scale at run time)
    inf = _convnext_step(optimizer=name, clip_grad_norm=float("inf"))
    assert [op.kind for op in _opt(inf)] == [op.kind for op in ops]
    assert math.isinf(inf._optws[:32].view(torch.float32)[N.VT_CTL_CLIP].item())


def test_defaults_build_the_parent_optimiser_list():
    raw = lambda t: ctypes.string_at(ctypes.addressof(t.opt_ops), t.n_opt * ctypes.sizeof(N.Op))  # noqa: E731
    for name in ("SGD", "AdamW", "Adam"):
        a = _convnext_step(optimizer=name)
        b = _convnext_step(optimizer=name, clip_grad_norm=None, lamb_max_grad_norm=1.0, trust_clip=True, always_adapt=True)
        assert raw(a) == raw(b) and a._optws is None
        kinds = {op.kind for op in _opt(a)}
        assert kinds == ({N.OP_SGD} if name == "SGD" else {N.OP_ADAM_TICK, N.OP_ADAMW})
        assert a.bases[E.OPTWS] is None
        with pytest.raises(RuntimeError):
            a.last_grad_norm()
    # the kinds a parent list can hold keep their numbers: the new ones are appended
    assert (N.OP_SGD, N.OP_ADAM_TICK, N.OP_ADAMW, N.OP_DEFORM_WGRAD) == (19, 54, 55, 115)
    assert [N.OP_GRAD_SUMSQ, N.OP_CLIP_COEF, N.OP_SGD_CLIP, N.OP_ADAMW_CLIP, N.OP_LAMB_MOMENTS, N.OP_LAMB_APPLY] == \
        list(range(116, 122))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_one_rank_group_carries_the_world_in_the_factor_op(monkeypatch):
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        for kw in (dict(optimizer="Lamb"), dict(optimizer="AdamW", clip_grad_norm=1.0), dict(clip_grad_norm=1.0)):
            ts = _convnext_step(exchange="allreduce", bucket_mb=0.05, **kw)
            assert ts.dp and ts.bucketer is not None
            ops = _opt(ts)
            coef = next(op for op in ops if op.kind == N.OP_CLIP_COEF)
            assert coef.f[1] == 1.0 / dist.get_world_size()
            _check_norm_ops(ts, ops[ops.index(coef) - 1: ops.index(coef) + 1], dist.get_world_size())
        for kw in (dict(optimizer="Lamb"), dict(clip_grad_norm=1.0)):
            with pytest.raises(NotImplementedError, match=r"(?s)exchange='sharded'.*Lamb.*clip_grad_norm"):
                TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True,
                          exchange="sharded", **kw)
    finally:
        dist.destroy_process_group()


def test_refusals():
    mk = lambda **kw: TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="SGD, AdamW, Adam"):
        mk(optimizer="RMSprop")
    with pytest.raises(ValueError, match="clip_grad_norm"):
        mk(clip_grad_norm=-1.0)
    with pytest.raises(ValueError, match="lamb_max_grad_norm"):
        mk(optimizer="Lamb", lamb_max_grad_norm=-0.5)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        mk(clip_grad_norm=float("nan"))
    for kw in (dict(optimizer="Lamb"), dict(clip_grad_norm=1.0)):
        with pytest.raises(NotImplementedError, match=r"(?s)exchange='sharded'.*Lamb.*clip_grad_norm"):
            mk(exchange="sharded", **kw)
    assert mk(optimizer="Lamb").optimizer == "Lamb"


def test_library_has_the_new_symbols_and_the_item_size():
    lib = N.lib()
    for name in ("vt_grad_sumsq", "vt_clip_coef", "vt_sgd_momentum_clip", "vt_adamw_clip", "vt_lamb_moments", "vt_lamb_apply",
                 "vt_opt_item"):
        assert name in N.SYMBOLS and getattr(lib, name) is not None
    assert lib.vt_opt_item() == N.VT_OPT_ITEM == LU.I and N.VT_OPT_ITEM % 64 == 0
    with pytest.raises(ValueError):
        N.lamb_table([0, 96], [96, 64], [0.0, 0.0])  # not multiples of 64: an item would cut a 16-byte chunk's tensor


# ---- bounds: the float32 restatement stays within half of what the GPU tests allow ----------------------------------------
@pytest.mark.parametrize("n", LU.SUMSQ_LENGTHS)
def test_f32_norm_within_half_the_counted_bound(n):
    g = LU.sumsq_input(n)
    want = float(LU.grad_norm([g.double()]))
    # the kernel's order of summation: 16-term float32 chains per lane, double above
    pad = torch.zeros(N.opt_items(n) * LU.I)
    pad[:n] = g
    lanes = pad.view(-1, LU.I // 1024, 256, 4).permute(0, 2, 1, 3).reshape(-1, 16)
    acc = torch.zeros(lanes.shape[0])
    for k in range(16):
        acc = torch.addcmul(acc, lanes[:, k], lanes[:, k])  # (one rounding more per term than the kernel's fmaf)
    got = float(np.float32(math.sqrt(float(acc.double().sum()))))
    rel = abs(got - want) / want
    print(f"n={n}: float32-lane norm {got!r} against {want!r}: {rel / LU.U24:.2f} u (bound {LU.C_NORM} u)")
    assert LU.C_NORM * LU.U24 <= 1e-5
    assert rel <= 0.5 * LU.C_NORM * LU.U24
    # what the bound has to catch: a dropped or doubled 4-element tail
    tail = float((g[-4:].double() ** 2).sum())
    moved = abs(math.sqrt(max(want * want - tail, 0.0)) - want) / want
    assert moved > (10 if n < 100_000 else 1) * LU.C_NORM * LU.U24, moved


@pytest.mark.parametrize("variant", list(LU.LAMB_VARIANTS))
def test_f32_lamb_within_half_the_elementwise_bound(variant):
    trust, adapt, M = LU.LAMB_VARIANTS[variant]
    p0, grads = LU.lamb_inputs()
    kw = dict(lr=LU.LAMB_LR, betas=LU.LAMB_BETAS, eps=LU.LAMB_EPS, M=M, trust_clip=trust, always_adapt=adapt)
    r64 = LU.Lamb([p.double() for p in p0], LU.LAMB_WD, **kw)
    r32 = LU.Lamb(p0, LU.LAMB_WD, **kw)
    first = None
    for g in grads:
        p_before = [p.clone() for p in r32.p]
        i64 = r64.step([x.double() for x in g])
        r32.step(g)
        first = first or i64
    worst = {}
    for tag, a, b in (("p", r32.p, r64.p), ("m", r32.m, r64.m), ("v", r32.v, r64.v)):
        w = max(((x.double() - y).abs() / (LU.ATOL + LU.RTOL * y.abs())).max().item() for x, y in zip(a, b))
        worst[tag] = w
    print(f"{variant}: float32 restatement at {worst} of the elementwise bound; r = {[round(r, 4) for r in i64['r']]}")
    assert all(w <= 0.5 for w in worst.values())
    # all-zero weights take r = 1 (their first step), the wd = 0 tensor too unless always_adapt
    assert first["r"][LU.LAMB_ZERO_P] == 1.0 and i64["r"][LU.LAMB_ZERO_P] != 1.0
    assert (i64["r"][LU.LAMB_PLAIN] == 1.0) == (not adapt or trust)  # (its r is above 1, which trust_clip caps)
    assert (M is None) == (i64["c2"] == 1.0)
    # the sums of the last step: float32 chains against the float64 sums of the float64 u of the same float32 operands
    t = len(grads)
    bc1, bc2s = float(np.float32(1 - LU.LAMB_BETAS[0] ** t)), float(np.float32(math.sqrt(1 - LU.LAMB_BETAS[1] ** t)))
    for k in range(len(p0)):
        pb, m, v, wd = p_before[k], r32.m[k], r32.v[k], LU.LAMB_WD[k]
        u32 = LU.lamb_u(pb, m, v, bc1, bc2s, LU.LAMB_EPS, wd)
        want = float((LU.lamb_u(pb.double(), m.double(), v.double(), bc1, bc2s, LU.LAMB_EPS, wd) ** 2).sum())
        got = float((u32.double() ** 2).sum())
        assert abs(got - want) <= 0.5 * LU.sum_u_bound(pb, m, v, bc1, bc2s, LU.LAMB_EPS, wd), (k, got, want)
