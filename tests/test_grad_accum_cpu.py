"""accumulate_grad_batches in the fused train step, host side (plan_only TrainSteps on the CPU): every 1 / world of the
optimiser list reads 1 / (world * k), nothing else in any launch list moves, the defaults are the lists without the
argument byte for byte, and a bad value is refused by name."""
import ctypes

import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.trainer import TrainStep


def _plan(**kw):
    return TrainStep(backbones.darknet_yolov5n(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, **kw)


def _bytes(arr, n):
    return ctypes.string_at(ctypes.addressof(arr), n * ctypes.sizeof(N.Op))


def _lists(ts):
    p = ts.prog
    return (_bytes(ts.opt_ops, ts.n_opt), bytes(ts.zero_ops), _bytes(p.fwd_ops, p.n_fwd), _bytes(p.bwd_ops, p.n_bwd))


# (optimiser arguments, the op kind that carries the gradient scale, its slot in op.f)
CASES = [
    ("SGD", {}, N.OP_SGD, 4),
    ("AdamW", {"optimizer": "AdamW"}, N.OP_ADAMW, 5),
    ("SGD+clip", {"clip_grad_norm": 1.0}, N.OP_CLIP_COEF, 1),
    ("Lamb", {"optimizer": "Lamb"}, N.OP_CLIP_COEF, 1),
]


@pytest.mark.parametrize("tag,kw,kind,slot", CASES, ids=[c[0] for c in CASES])
def test_grad_scale_reads_one_over_world_times_k(tag, kw, kind, slot):
    one, three = _plan(**kw), _plan(accumulate_grad_batches=3, **kw)
    assert one.world == three.world == 1 and one.n_opt == three.n_opt
    seen = 0
    for i in range(one.n_opt):
        a, b = one.opt_ops[i], three.opt_ops[i]
        assert a.kind == b.kind
        if a.kind == kind:
            seen += 1
            assert a.f[slot] == 1.0 / one.world and b.f[slot] == 1.0 / (three.world * 3)
            b.f[slot] = a.f[slot]
        # nothing but that immediate differs
        assert ctypes.string_at(ctypes.addressof(a), ctypes.sizeof(N.Op)) == ctypes.string_at(ctypes.addressof(b), ctypes.sizeof(N.Op))
    assert seen >= 1
    if kind == N.OP_CLIP_COEF:  # the consumers behind it read the device factor: no immediate of their own
        assert all(one.opt_ops[i].kind not in (N.OP_SGD, N.OP_ADAMW) for i in range(one.n_opt))
    assert _lists(one)[1:] == _lists(three)[1:]  # memset, forward and backward lists are the k = 1 lists


def test_defaults_given_equal_defaults_omitted():
    for kw in ({}, {"optimizer": "AdamW"}, {"clip_grad_norm": 2.0}, {"optimizer": "Lamb"}):
        assert _lists(_plan(**kw)) == _lists(_plan(accumulate_grad_batches=1, ema_decay=None, ema_steps=1, **kw))
    ts = _plan()
    assert ts.steps_done == 0 and ts.micro_steps_done == 0 and ts._accum == 1


def test_accumulation_and_ema_compose():
    ts = _plan(accumulate_grad_batches=4, ema_decay=0.99, ema_steps=2)
    plain = _plan(accumulate_grad_batches=4)
    assert _lists(ts)[0][: len(_lists(plain)[0])] == _lists(plain)[0]
    assert [ts.opt_ops[i].kind for i in range(plain.n_opt, ts.n_opt)] == \
        [N.OP_EMA_TICK, N.OP_EMA_UPDATE, N.OP_EMA_UPDATE, N.OP_EMA_COPY]  # in the optimiser list: once per OPTIMISER step
    assert ts.bases[E.EMA] is not None


def test_bad_values_are_refused_by_name():
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            _plan(accumulate_grad_batches=bad)
    with pytest.raises(RuntimeError, match="plan_only"):
        _plan(accumulate_grad_batches=2).step()
