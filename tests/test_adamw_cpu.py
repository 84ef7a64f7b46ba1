"""Host logic of the Adam-family optimiser list and of `include_pool=False` (no GPU: plan_only, device="cpu" as
tests/test_host_cpu.py does).  What the kernels compute is tests/test_adamw_gpu.py's subject; here: which launches a
step issues, over which ranges of the flat buffers, with which scalars."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import ConvNeXt
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, HYPER_STEP, TrainStep, param_groups

WD, NORM_WD, BIAS_WD = 0.05, 0.01, 0.02  # three different values: a segment carrying another group's decay shows


def _opt(ts):
    return [ts.opt_ops[k] for k in range(ts.n_opt)]


def _ranges(ops):
    return sorted((op.ptr[0].offset // 4, op.ptr[0].offset // 4 + int(op.f[0])) for op in ops)


def _convnext_step(dtype=torch.bfloat16, **kw):
    return TrainStep(ConvNeXt(24, (1, 2)), 10, 3, 64, dtype, device="cpu", plan_only=True, lr=1e-3, weight_decay=WD,
                     norm_weight_decay=NORM_WD, bias_weight_decay=BIAS_WD, **kw)


@pytest.mark.parametrize("name,decoupled", [("AdamW", 1), ("Adam", 0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_adam_family_optimiser_list(name, decoupled, dtype):
    ts = _convnext_step(dtype, optimizer=name, include_pool=False, betas=(0.8, 0.95), eps=1e-6)
    ops = _opt(ts)
    kinds = [op.kind for op in ops]
    # the counter op exactly once, first; then one VT_OP_ADAMW per weight-decay segment
    assert kinds[0] == N.OP_ADAM_TICK and kinds.count(N.OP_ADAM_TICK) == 1
    assert (ops[0].ptr[0].base, ops[0].ptr[0].offset) == (E.HYPER, 0) and (ops[0].f[0], ops[0].f[1]) == (0.8, 0.95)
    upd = ops[1:]
    assert [op.kind for op in upd] == [N.OP_ADAMW] * len(ts.segments) and len(ts.segments) == 3
    total = ts.store.pflat.numel()
    r = _ranges(upd)
    assert r[0][0] == 0 and r[-1][1] == total and all(a[1] == b[0] for a, b in zip(r, r[1:]))  # [0, total) exactly once
    # every segment carries its own group's decay: the group of each parameter decides, not the position
    groups = param_groups(ts.model)
    wd_of = {GROUP_OTHER: WD, GROUP_NORM: NORM_WD, GROUP_BIAS: BIAS_WD}
    for p, off in zip(ts.store.params, ts.store.offsets):
        op = next(o for o in upd if o.ptr[0].offset // 4 <= off < o.ptr[0].offset // 4 + int(o.f[0]))
        assert op.f[4] == wd_of[groups[id(p)]]
    for op in upd:
        lo = op.ptr[0].offset
        assert [(op.ptr[k].base, op.ptr[k].offset) for k in range(4)] == \
            [(E.PARAMS, lo), (E.GRADS, lo), (E.MOMENTUM, lo), (E.MOMENT2, lo)]
        if dtype == torch.bfloat16:
            assert (op.ptr[4].base, op.ptr[4].offset) == (E.MIRROR, lo // 2)
        else:
            assert op.ptr[4].base == -1
        assert (op.ptr[5].base, op.ptr[5].offset) == (E.HYPER, 0)  # learning rate and step count come from the device
        assert op.i[1] == decoupled
        assert (op.f[1], op.f[2], op.f[3], op.f[5]) == (0.8, 0.95, 1e-6, 1.0)
        assert lo % 16 == 0
    assert ts.vflat is not None and ts.vflat.shape == ts.store.pflat.shape
    assert ts.opt_steps() == 0 and HYPER_STEP == 4
    ts.set_lr(3e-4)  # the learning rate stays a device value: nothing of the list is rebuilt, the step slots are untouched
    assert [op.kind for op in _opt(ts)] == kinds and ts.opt_steps() == 0
    assert torch.equal(ts.lr_dev[:4], torch.full((4,), 3e-4)) and not ts.lr_dev[4:].any()


def test_sgd_stays_the_default_and_keeps_its_list():
    a = TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True)
    b = TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, optimizer="SGD")
    assert a.optimizer == "SGD" and a.vflat is None and b.vflat is None
    assert a.n_opt == b.n_opt == len(a.segments)
    import ctypes

    raw = [ctypes.string_at(ctypes.addressof(t.opt_ops), t.n_opt * ctypes.sizeof(N.Op)) for t in (a, b)]
    assert raw[0] == raw[1]
    assert all(op.kind == N.OP_SGD for op in _opt(a))


def test_include_pool_false_is_the_reference_assembly():
    ts = _convnext_step(optimizer="AdamW", include_pool=False)
    keys = list(ts.model.state_dict().keys())
    assert keys[-2:] == ["1.weight", "1.bias"] and all(k.startswith(("0.", "1.")) for k in keys)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 48) and tuple(ts.model[1].bias.shape) == (10,)
    kinds = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    # head norm -> head GEMM with no pooling launch in between (the only pooling op is the backbone's own, in front
    # of the head norm), and the loss is the last op
    ln = max(i for i, k in enumerate(kinds) if k == N.OP_LAYERNORM_FWD)
    gemm = max(i for i, k in enumerate(kinds) if k == N.OP_CONV_IGEMM)
    assert ln < gemm and N.OP_AVGPOOL_FWD not in kinds[ln:] and kinds.count(N.OP_AVGPOOL_FWD) == 1
    assert kinds[-1] == N.OP_XENT and ts.prog.fwd_ops[ts.prog.n_fwd - 1].i[3] == 10  # the loss reads 10 classes
    # include_pool=True keeps the four-child assembly and its pooling launch
    tp = _convnext_step(optimizer="AdamW", include_pool=True)
    assert list(tp.model.state_dict().keys())[-2:] == ["3.weight", "3.bias"]
    kp = [tp.prog.fwd_ops[k].kind & 0xFFFF for k in range(tp.prog.n_fwd)]
    assert kp.count(N.OP_AVGPOOL_FWD) == 2


def test_a_class_count_off_the_chunk_reserves_zero_rows():
    """10 classes: the head runs as the next whole 16-byte chunk of rows (16 in bf16, 12 in f32) over zeros the flat
    store reserves behind the parameter; the parameter itself keeps its shape"""
    for dtype, rows in ((torch.bfloat16, 16), (torch.float32, 12)):
        ts = _convnext_step(dtype, optimizer="AdamW", include_pool=False)
        st = ts.store
        i = next(k for k, p in enumerate(st.params) if p is ts.model[1].weight)
        assert st.slots[i] >= rows * 48 and st.slots[i] % 64 == 0
        assert not st.pflat[st.offsets[i] + 480: st.offsets[i] + st.slots[i]].any()
        assert st.offsets[i] + st.slots[i] == st.total  # nothing overlaps the reserved rows
    # a class count on the chunk changes nothing
    ts = TrainStep(ConvNeXt(24, (1, 2)), 16, 3, 64, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    assert ts.store.slots == [E._round_up(p.numel(), 64) for p in ts.store.params]


def test_refusals():
    with pytest.raises(ValueError, match="include_pool=False"):
        TrainStep(backbones.cspdarknet53(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    with pytest.raises(ValueError, match="SGD, AdamW, Adam"):
        TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, optimizer="RMSprop")
    # the ConvNeXt refusals are hit when the program is built
    with pytest.raises(NotImplementedError, match="GlobalResponseNorm"):
        TrainStep(ConvNeXt(16, (1, 1), v2=True), 16, 2, 32, torch.bfloat16, device="cpu", plan_only=True,
                  optimizer="AdamW", include_pool=False)
    with pytest.raises(NotImplementedError, match="stochastic_depth"):
        TrainStep(ConvNeXt(16, (1, 1), stochastic_depth=0.1), 16, 2, 32, torch.bfloat16, device="cpu", plan_only=True,
                  optimizer="AdamW", include_pool=False)
    with pytest.raises(NotImplementedError, match="deterministic"):
        TrainStep(ConvNeXt(16, (1, 1)), 16, 2, 32, torch.bfloat16, device="cpu", plan_only=True, optimizer="AdamW",
                  include_pool=False, deterministic=True)


# ---- sharded exchange: each rank updates its shards only, with the same step count -----------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sharded_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "vision-toolbox_amd"), str(root)]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vision_toolbox import _native as N_
        from vision_toolbox import backbones as bk
        from vision_toolbox.trainer import TrainStep as TS

        torch.manual_seed(7)
        ts = TS(bk.darknet_yolov5n(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, bucket_mb=0.5,
                exchange="sharded", optimizer="AdamW", weight_decay=0.05, norm_weight_decay=0.01, bias_weight_decay=0.02)
        ops = [ts.opt_ops[k] for k in range(ts.n_opt)]
        kinds = [op.kind for op in ops]
        ok_tick = kinds[0] == N_.OP_ADAM_TICK and kinds.count(N_.OP_ADAM_TICK) == 1 and set(kinds[1:]) == {N_.OP_ADAMW}
        touched = sorted((op.ptr[0].offset // 4, op.ptr[0].offset // 4 + int(op.f[0]), op.f[4]) for op in ops[1:])
        ok_own = all(any(s0 <= lo and hi <= s1 for s0, s1 in ts.bucketer.shards) for lo, hi, _ in touched)
        ok_scale = all(op.f[5] == 1.0 / world for op in ops[1:])
        q.put((rank, bool(ok_tick), bool(ok_own), bool(ok_scale), touched, list(ts.segments), ts.store.total,
               ts.store.pflat.numel()))
    finally:
        dist.destroy_process_group()


def test_sharded_exchange_refuses_a_convnext(monkeypatch):
    """its layer scales and depthwise filters are f32-read parameters outside the head bucket the sharded exchange refreshes
    in f32: refused, not silently stale (a one-rank gloo group stands in for the job)"""
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            _convnext_step(optimizer="AdamW", include_pool=False, exchange="sharded")
        ts = _convnext_step(optimizer="AdamW", include_pool=False, exchange="allreduce", bucket_mb=0.05)
        assert ts.dp and ts.bucketer is not None and _opt(ts)[0].kind == N.OP_ADAM_TICK
    finally:
        dist.destroy_process_group()


def test_sharded_exchange_ranks_tile_the_buffer_with_adamw():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == [0, 1]
    for r in results:
        assert all(r[1:4]), r[:4]
    segments, total, padded = results[0][5], results[0][6], results[0][7]
    assert results[1][5:] == results[0][5:] and padded % (64 * world) == 0
    # the two ranks' ranges tile the parameters' part of the buffer exactly once (beyond it there is only padding) ...
    pieces = sorted(t for r in results for t in r[4])
    assert pieces[0][0] == 0 and pieces[-1][1] == total and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
    assert all(len(r[4]) > 0 for r in results)
    # ... and every piece lies inside one weight-decay segment and carries that segment's decay
    for lo, hi, wd in pieces:
        assert any(s0 <= lo and hi <= s1 and wd == swd for s0, s1, swd in segments), (lo, hi, wd)
