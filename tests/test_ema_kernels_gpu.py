"""vt_ema_tick / vt_ema_update / vt_ema_copy through the C-ABI, against the float64 restatement of tests/ema_util.py.

The bound is counted, not measured: a blend rounds twice (p - e, then one fma), so one update is within
C_BLEND * u * (|e| + |p|) with C_BLEND = 2 and u = 2^-24, and an error already in e enters the next blend times 1 - alpha
(ema_util.run carries exactly that sum; it never exceeds min(t, 1 / alpha) of the largest term).  The copy is exact.

The large length: the grid of vt_ema_update is capped at 2048 workgroups of 256 lanes, one 16-byte chunk per lane and round
(vt_ema_grid_cap() = 2 097 152 elements); at N_LOOP = 2 * cap + 4097 every workgroup takes three rounds, the last one
partial, and a tail of one element is left over."""
import numpy as np
import pytest
import torch

from vision_toolbox import _native as N

import ema_util as EU
from gpu_util import stream, vp

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64  # guard elements in front of and behind every operand
GRID_CAP = 2048 * 256 * 4
N_LOOP = 2 * GRID_CAP + 4097
LENGTHS = [1, 3, 4, 4095, 4096, 4097, 8 * 4096 + 5, N_LOOP]


@pytest.fixture(autouse=True)
def _lib_launched():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, device="cuda", dtype=dtype)
    return buf, buf[PAD: PAD + n]


def _guards_kept(buf, n, fill):
    lo, hi = buf[:PAD], buf[PAD + n:]
    want = torch.full_like(lo, fill)
    return torch.equal(lo.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)) and \
        torch.equal(hi.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32),
                    want.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32))


def _ctl(alpha, period=1):
    """a control buffer as the trainer builds it, followed by guard words"""
    ctl = torch.zeros(16, device="cuda", dtype=torch.float32)
    ctl[N.VT_EMA_ALPHA] = alpha
    ci = ctl.view(torch.int32)
    ci[N.VT_EMA_PERIOD] = period
    ci[8:] = 0x7FC00123
    return ctl


def _inputs(n, k):
    g = torch.Generator().manual_seed(100 + k)
    return (torch.randn(n, generator=g) * (1.0 + k)).cuda()


@pytest.mark.parametrize("alpha", [0.1, 2e-5])
@pytest.mark.parametrize("mirror", [False, True], ids=["f32", "mirror"])
@pytest.mark.parametrize("n", LENGTHS)
def test_copy_then_three_blends(n, mirror, alpha):
    L = N.lib()
    assert L.vt_ema_grid_cap() == GRID_CAP and N_LOOP > 2 * GRID_CAP and N_LOOP % 4 == 1  # the cap this file states
    a32 = float(np.float32(alpha))
    ctl = _ctl(alpha)
    assert ctl[N.VT_EMA_ALPHA].item() == a32
    ebuf, e = _guarded(n, torch.float32, NAN)
    mbuf, m = _guarded(n, torch.bfloat16, 7.0) if mirror else (None, None)
    ps = [_inputs(n, k) for k in range(4)]
    pbufs = []
    for p in ps:
        pb, pv = _guarded(n, torch.float32, NAN)
        pv.copy_(p)
        pbufs.append((pb, pv))
    want = EU.run([p.cpu() for p in ps], a32)
    worst = 0.0
    for k, (pb, pv) in enumerate(pbufs):
        before = N.launch_count()
        N.check(L.vt_ema_tick(vp(ctl), stream()))
        e_in = e.clone()
        N.check(L.vt_ema_update(vp(e), vp(pv), vp(m), n, vp(ctl), stream()))
        assert N.launch_count() == before + 2
        got = e.clone()
        ci = ctl.view(torch.int32)
        assert ci[N.VT_EMA_MODE].item() == (N.VT_EMA_COPY if k == 0 else N.VT_EMA_BLEND)
        assert ci[N.VT_EMA_COUNT].item() == ci[N.VT_EMA_STEP].item() == k + 1
        # the same launch again on the same inputs: bit-identical (the mode is still this step's)
        e.copy_(e_in)
        if mirror:
            m_first = m.clone()
            m.fill_(7.0)
        N.check(L.vt_ema_update(vp(e), vp(pv), vp(m), n, vp(ctl), stream()))
        assert torch.equal(e.view(torch.int32), got.view(torch.int32))
        ref, bound = want[k]
        err = (got.cpu().double() - ref).abs()
        if k == 0:
            assert torch.equal(got.view(torch.int32), pv.view(torch.int32))  # update 0 is a copy
        else:
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert (err <= bound).all(), (k, float((err / bound.clamp_min(1e-300)).max()))
        if mirror:
            assert torch.equal(m.view(torch.int16), m_first.view(torch.int16))
            assert torch.equal(m, got.to(torch.bfloat16))  # round-to-nearest-even cast of the NEW e, same pass
            assert _guards_kept(mbuf, n, 7.0)
        # p is only read; nothing is written outside [0, n)
        assert torch.equal(pv.view(torch.int32), ps[k].view(torch.int32)) and _guards_kept(pb, n, NAN)
        assert _guards_kept(ebuf, n, NAN)
    ci = ctl.view(torch.int32)
    assert ctl[N.VT_EMA_ALPHA].item() == a32 and ci[N.VT_EMA_PERIOD].item() == 1 and (ci[8:] == 0x7FC00123).all()
    print(f"n={n} mirror={mirror} alpha={alpha}: worst error / bound over 3 blends {worst:.3f} "
          f"(bound: {EU.C_BLEND} u (|e| + |p|) per blend, carried by the recurrence)")


@pytest.mark.parametrize("mirror", [False, True], ids=["f32", "mirror"])
def test_skip_steps_touch_neither_buffer(mirror):
    L = N.lib()
    n = 8 * 4096 + 5
    ctl = _ctl(0.25, period=3)
    ci = ctl.view(torch.int32)
    ebuf, e = _guarded(n, torch.float32, NAN)
    mbuf, m = _guarded(n, torch.bfloat16, 7.0) if mirror else (None, None)
    nbuf, nsrc = _guarded(6, torch.int64, -1)
    dbuf, ndst = _guarded(6, torch.int64, -2)
    p0, p3 = _inputs(n, 0), _inputs(n, 3)
    nan_p = torch.full((n,), NAN, device="cuda")
    modes = []
    for s, p in enumerate([p0, nan_p, nan_p, p3]):
        nsrc.fill_(10 + s)
        e_in = e.clone()
        m_in = m.clone() if mirror else None
        d_in = ndst.clone()
        N.check(L.vt_ema_tick(vp(ctl), stream()))
        N.check(L.vt_ema_update(vp(e), vp(p), vp(m), n, vp(ctl), stream()))
        N.check(L.vt_ema_copy(vp(ndst), vp(nsrc), 48, vp(ctl), stream()))
        modes.append(ci[N.VT_EMA_MODE].item())
        if modes[-1] == N.VT_EMA_SKIP:
            assert torch.equal(e.view(torch.int32), e_in.view(torch.int32)) and torch.equal(ndst, d_in)
            assert not mirror or torch.equal(m.view(torch.int16), m_in.view(torch.int16))
            assert p.isnan().all()
        else:
            assert torch.equal(ndst, nsrc)  # integer buffers are copied on the steps that update
    assert modes == [N.VT_EMA_COPY, N.VT_EMA_SKIP, N.VT_EMA_SKIP, N.VT_EMA_BLEND] == EU.modes(4, 3)
    assert ci[N.VT_EMA_COUNT].item() == 2 and ci[N.VT_EMA_STEP].item() == 4
    ref, bound = EU.run([p0.cpu(), nan_p.cpu(), nan_p.cpu(), p3.cpu()], 0.25, period=3)[-1]
    assert not e.isnan().any() and ((e.cpu().double() - ref).abs() <= bound).all()
    assert not mirror or torch.equal(m, e.to(torch.bfloat16))
    assert _guards_kept(ebuf, n, NAN) and (not mirror or _guards_kept(mbuf, n, 7.0))
    assert (nbuf[:PAD] == -1).all() and (nbuf[PAD + 6:] == -1).all() and (dbuf[:PAD] == -2).all() and (dbuf[PAD + 6:] == -2).all()


def test_argument_checks_name_the_function():
    L = N.lib()
    ctl = _ctl(0.5)
    e, p = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    m = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    before = N.launch_count()
    cases = [
        ("vt_ema_tick", lambda: L.vt_ema_tick(None, stream())),
        ("vt_ema_tick", lambda: L.vt_ema_tick(vp(ctl[1:]), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(None, vp(p), None, 64, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), None, None, 64, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), vp(p), None, 64, None, stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), vp(p), None, 0, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e[1:]), vp(p), None, 60, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), vp(p[2:]), None, 60, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), vp(p), vp(m[1:]), 60, vp(ctl), stream())),
        ("vt_ema_update", lambda: L.vt_ema_update(vp(e), vp(e), None, 64, vp(ctl), stream())),
        ("vt_ema_copy", lambda: L.vt_ema_copy(None, vp(p), 64, vp(ctl), stream())),
        ("vt_ema_copy", lambda: L.vt_ema_copy(vp(e), vp(p), 24, vp(ctl), stream())),
        ("vt_ema_copy", lambda: L.vt_ema_copy(vp(e), vp(p), 64, None, stream())),
    ]
    for who, call in cases:
        assert call() == N.VT_ERR_INVALID and N.last_error().startswith(who + ":"), (who, N.last_error())
    assert N.launch_count() == before  # a refused call launches nothing
    N.check(L.vt_ema_tick(vp(ctl), stream()))
