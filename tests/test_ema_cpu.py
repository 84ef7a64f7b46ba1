"""Weight EMA in the fused train step, host side: symbols and constants, the optimiser launch list with and without the
average (plan_only TrainSteps on the CPU), every refusal by name, alpha formed in double, the state_dict round trip on the
shadow buffers, and the float64 restatement of tests/ema_util.py against its closed form."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import ViT
from vision_toolbox.trainer import TrainStep

import ema_util as EU

ROOT = Path(__file__).resolve().parents[1]


def _plan(dtype=torch.bfloat16, **kw):
    return TrainStep(backbones.darknet_yolov5n(), 16, 2, 64, dtype, device="cpu", plan_only=True, **kw)


def _vit_plan(dtype=torch.bfloat16, **kw):
    return TrainStep(ViT(64, 1, 2, 4, 16, layer_scale_init=0.5), 10, 3, 16, dtype, device="cpu", plan_only=True,
                     include_pool=False, **kw)


def _bytes(arr, n):
    return ctypes.string_at(ctypes.addressof(arr), n * ctypes.sizeof(N.Op))


def _lists(ts):
    p = ts.prog
    return (_bytes(ts.opt_ops, ts.n_opt), bytes(ts.zero_ops), _bytes(p.fwd_ops, p.n_fwd), _bytes(p.bwd_ops, p.n_bwd))


def _ptr(op, k):
    return (op.ptr[k].base, op.ptr[k].offset)


def test_symbols_and_constants():
    lib = N.lib()
    for name, nargs in (("vt_ema_tick", 2), ("vt_ema_update", 6), ("vt_ema_copy", 5), ("vt_ema_grid_cap", 0)):
        assert name in N.SYMBOLS and len(N.SYMBOLS[name][1]) == nargs and getattr(lib, name) is not None
    # appended behind the parent's kinds: no earlier op code moves
    assert N.OP_EMA_TICK == N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY + 1 == 128
    assert (N.OP_EMA_UPDATE, N.OP_EMA_COPY) == (129, 130)
    assert [N.OP_NAMES[k] for k in (128, 129, 130)] == ["ema_tick", "ema_update", "ema_copy"]
    text = (ROOT / "include" / "vt_amd.h").read_text()
    for name in ("VT_EMA_ALPHA", "VT_EMA_MODE", "VT_EMA_COUNT", "VT_EMA_PERIOD", "VT_EMA_STEP", "VT_EMA_SKIP", "VT_EMA_COPY",
                 "VT_EMA_BLEND"):
        m = re.search(rf"#define {name} (\d+)", text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert len({N.VT_EMA_ALPHA, N.VT_EMA_MODE, N.VT_EMA_COUNT, N.VT_EMA_PERIOD, N.VT_EMA_STEP}) == 5
    assert (N.VT_EMA_SKIP, N.VT_EMA_COPY, N.VT_EMA_BLEND) == (EU.SKIP, EU.COPY, EU.BLEND)
    assert "int vt_ema_update(float* ema, const float* p, void* ema_mirror, int64_t n, const float* ctl, void* stream);" in text
    assert E.EMA == E.NUM_BASES - 1 < N.VT_MAX_BASES
    # the grid cap the kernel tests take their large n from: no host call launches anything
    before = N.launch_count()
    assert lib.vt_ema_grid_cap() == 2048 * 256 * 4 and N.launch_count() == before


OPTS = [("SGD", {}), ("AdamW", {"optimizer": "AdamW"}), ("SGD+clip", {"clip_grad_norm": 1.0}), ("Lamb", {"optimizer": "Lamb"})]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("tag,kw", OPTS, ids=[t for t, _ in OPTS])
def test_ema_ops_follow_an_unchanged_optimiser_list(tag, kw, dtype):
    plain = _plan(dtype, **kw)
    ts = _plan(dtype, ema_decay=0.999, ema_steps=4, **kw)
    a, b = _lists(plain), _lists(ts)
    assert b[0][: len(a[0])] == a[0] and ts.n_opt == plain.n_opt + 4  # byte-identical prefix
    assert a[1:] == b[1:]  # forward, backward and the memset do not know about the average
    tick, up_p, up_s, cp_n = (ts.opt_ops[plain.n_opt + i] for i in range(4))
    assert [o.kind for o in (tick, up_p, up_s, cp_n)] == [N.OP_EMA_TICK, N.OP_EMA_UPDATE, N.OP_EMA_UPDATE, N.OP_EMA_COPY]
    st = ts.store
    n_p, n_s, n_n = st.pflat.numel(), st.sflat.numel(), st.nflat.numel()
    ctl = (E.EMA, 0)
    assert _ptr(tick, 0) == ctl and tick.ptr[1].base == -1
    # parameters: shadow behind the 64 control bytes, the bf16 mirror of the shadow behind every f32 / int64 shadow
    assert _ptr(up_p, 0) == (E.EMA, 64) and _ptr(up_p, 1) == (E.PARAMS, 0) and _ptr(up_p, 3) == ctl and int(up_p.f[0]) == n_p
    s_off = 64 + 4 * n_p
    assert _ptr(up_s, 0) == (E.EMA, s_off) and _ptr(up_s, 1) == (E.STATE, 0) and up_s.ptr[2].base == -1
    assert _ptr(up_s, 3) == ctl and int(up_s.f[0]) == n_s
    n_off = s_off + 4 * n_s
    assert n_off % 16 == 0 and _ptr(cp_n, 0) == (E.EMA, n_off) and _ptr(cp_n, 1) == (E.COUNTERS, 0) and _ptr(cp_n, 2) == ctl
    assert int(cp_n.f[0]) == 8 * n_n and (8 * n_n) % 16 == 0
    m_off = n_off + 8 * n_n
    if dtype == torch.bfloat16:
        assert _ptr(up_p, 2) == (E.EMA, m_off) and m_off % 16 == 0 and ts._ema.numel() == m_off + 2 * n_p
        assert ts.ema_mirror.numel() == n_p and ts.ema_mirror.dtype == torch.bfloat16
    else:
        assert up_p.ptr[2].base == -1 and ts._ema.numel() == m_off and ts.ema_mirror is None
    # the shadow views are those slices, and the base is bound
    assert ts.ema_pflat.data_ptr() == ts._ema.data_ptr() + 64 and ts.ema_pflat.numel() == n_p
    assert ts.ema_sflat.data_ptr() == ts._ema.data_ptr() + s_off and ts.ema_nflat.data_ptr() == ts._ema.data_ptr() + n_off
    assert ts.bases[E.EMA] == ts._ema.data_ptr() and plain.bases[E.EMA] is None
    # control words as built: alpha, period, everything else zero
    ci = ts._ema_ctl_i
    assert ts._ema_ctl_f[N.VT_EMA_ALPHA].item() == EU.alpha_f32(0.999) and ci[N.VT_EMA_PERIOD].item() == 4
    assert ci[N.VT_EMA_MODE].item() == ci[N.VT_EMA_COUNT].item() == ci[N.VT_EMA_STEP].item() == 0


def test_a_model_without_batchnorm_still_carries_every_ema_op():
    plain, ts = _vit_plan(optimizer="AdamW"), _vit_plan(optimizer="AdamW", ema_decay=0.5)
    assert _lists(ts)[0][: len(_lists(plain)[0])] == _lists(plain)[0]
    kinds = [ts.opt_ops[i].kind for i in range(plain.n_opt, ts.n_opt)]
    assert kinds == [N.OP_EMA_TICK, N.OP_EMA_UPDATE, N.OP_EMA_UPDATE, N.OP_EMA_COPY]
    # (the store's statistics and counter buffers are never empty: 64 floats, 2 int64 at the least)
    assert int(ts.opt_ops[plain.n_opt + 2].f[0]) == ts.store.sflat.numel() >= 64
    assert int(ts.opt_ops[plain.n_opt + 3].f[0]) == 8 * ts.store.nflat.numel() >= 16


def test_defaults_given_equal_defaults_omitted():
    assert _lists(_plan()) == _lists(_plan(ema_decay=None, ema_steps=1, accumulate_grad_batches=1))
    ts = _plan()
    assert ts._ema is None and ts.steps_done == 0 and ts.micro_steps_done == 0


def test_alpha_is_formed_in_double():
    d = 0.99998
    ts = _plan(ema_decay=d)
    got = ts._ema_ctl_f[N.VT_EMA_ALPHA].item()
    assert got == float(np.float32(1.0 - d)) == EU.alpha_f32(d)
    # what vt_amd.h warns against: the decay rounded to f32 first moves alpha by 3e-3 of its value
    wrong = float(np.float32(1.0) - np.float32(d))
    assert abs(wrong - (1.0 - d)) / (1.0 - d) > 1e-3 > abs(got - (1.0 - d)) / (1.0 - d) * 1e4
    ts.set_ema_decay(0.9)
    assert ts._ema_ctl_f[N.VT_EMA_ALPHA].item() == EU.alpha_f32(0.9) and ts.ema_decay == 0.9
    assert ts._ema_ctl_i[N.VT_EMA_PERIOD].item() == 1  # (the neighbours are not touched)


def test_refusals_name_their_argument():
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            _plan(ema_decay=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="ema_steps"):
            _plan(ema_decay=0.9, ema_steps=bad)
    with pytest.raises(ValueError, match="ema_steps"):
        _plan(ema_steps=0)  # checked even where no average is kept
    with pytest.raises(NotImplementedError, match="ema_decay"):
        _plan(ema_decay=0.9, exchange="sharded")
    plain = _plan()
    assert plain.ema_decay is None  # (the attribute exists without an average too)
    for call in (lambda: plain.set_ema_decay(0.9), plain.ema_updates, plain.ema_state_dict,
                 lambda: plain.load_ema_state_dict({}), lambda: plain.validate(ema=True)):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    ts = _plan(ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay"):
        ts.set_ema_decay(1.0)
    with pytest.raises(RuntimeError, match="no update"):
        ts.ema_state_dict()  # before the first update
    assert ts.ema_updates() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_state_dict_round_trip_on_the_shadow_buffers(dtype):
    ts = _plan(dtype, ema_decay=0.9)
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 99, v.shape, generator=g))
          for k, v in ts.model.state_dict().items()}
    with pytest.raises(KeyError, match="load_ema_state_dict"):
        ts.load_ema_state_dict({k: v for k, v in list(sd.items())[1:]})
    ts.load_ema_state_dict(sd)
    assert ts.ema_updates() == 1  # the next update blends
    back = ts.ema_state_dict()
    model_sd = ts.model.state_dict()
    assert list(back) == list(model_sd)
    for k, v in back.items():
        assert v.shape == model_sd[k].shape and v.dtype == model_sd[k].dtype and torch.equal(v, sd[k]), k
    # a 4-D weight lies channels_last in the shadow, where the parameter lies in pflat
    key, w = next((k, p) for k, p in ts.model.named_parameters() if p.dim() == 4 and p.shape[1] > 1 and p.shape[2] > 1)
    _, off, n = ts.store.where(w)
    assert torch.equal(ts.ema_pflat[off: off + n], sd[key].permute(0, 2, 3, 1).reshape(-1))
    if dtype == torch.bfloat16:
        assert torch.equal(ts.ema_mirror, ts.ema_pflat.to(torch.bfloat16))
    # the model's own weights were not touched, and a second round trip keeps every bit of the buffer
    assert not torch.equal(model_sd[key], sd[key])
    keep = ts._ema.clone()
    ts.load_ema_state_dict(back, updates=7)
    keep[:32].view(torch.int32)[N.VT_EMA_COUNT] = 7
    assert torch.equal(ts._ema, keep) and ts.ema_updates() == 7
    # `steps` restores the phase of ema_steps > 1 as well; without it the step count stays as it is
    ts.load_ema_state_dict(back, updates=7, steps=65)
    keep[:32].view(torch.int32)[N.VT_EMA_STEP] = 65
    assert torch.equal(ts._ema, keep)


def test_restatement_against_the_closed_form():
    g = torch.Generator().manual_seed(11)
    e0, p = torch.randn(257, generator=g), torch.randn(257, generator=g)
    for decay in (0.9, 0.99998):
        a = EU.alpha_f32(decay)
        for period in (1, 3):
            t_blends = 5
            steps = [e0] + [p] * (t_blends * period + period - 1)  # updates at 0, period, .., t_blends * period
            out = EU.run(steps, a, period)
            assert len(out) == len(steps)
            want = EU.closed_form(e0, p, a, t_blends)
            e, bound = out[t_blends * period]  # the last updating step
            assert torch.allclose(e, want, rtol=1e-13, atol=1e-15)
            assert torch.equal(out[-1][0], e)  # the skipped steps behind it keep the value
            assert (bound <= min(t_blends, 1.0 / a) * EU.C_BLEND * EU.U24 * (e0.abs().double() + p.abs().double()) + 1e-30).all()
    assert EU.modes(4, 3) == [EU.COPY, EU.SKIP, EU.SKIP, EU.BLEND] and EU.modes(3, 1) == [EU.COPY, EU.BLEND, EU.BLEND]
    out = EU.run([e0, p, p], 0.5, period=2)
    assert torch.equal(out[1][0], e0.double()) and torch.equal(out[2][0], (e0.double() + p.double()) / 2)
