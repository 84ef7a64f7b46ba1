"""loss="bce" without a GPU: the float64 yardstick of tests/bce_util.py against torch itself, the launch lists TrainStep builds
for the new arguments (plan_only, device="cpu"), the refusals, the digests of the default lists, the float32 restatement of
the kernel's arithmetic against half of every bound the GPU tests use (the rule of tests/test_head_neck_refs_cpu.py), and the
learning rates of the GPU step tests (the rule of NOTEBOOK 23.3)."""
import ctypes
import importlib.util
import os
import socket
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.trainer import LOSSES, TrainStep

import bce_util as BU

ROOT = Path(__file__).resolve().parents[1]


# ---- the yardstick itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BU.SHAPES, ids=str)
def test_yardstick_is_torch_bce_with_logits_on_explicit_targets(shape):
    B, N_ = shape
    y = BU.labels(B, N_)
    for header, s, thr, sum_classes in BU.combos():
        assert BU.margin_ok(N_, header, s, thr)
        # the target, written out by hand
        mode, lam = header if header is not None else (0, 1.0)
        lam = BU.f32r(lam) if mode else 1.0
        t = torch.zeros(B, N_, dtype=torch.float64)
        for b in range(B):
            t[b, y[b]] += lam
            t[b, y[(b - 1) % B]] += 1 - lam
        t = (1 - BU.f32r(s)) * t + BU.f32r(s) / N_
        if thr is not None:
            t = (t > BU.f32r(thr)).double()
        c = BU.case(B, N_, BU.F32, header, s, thr, sum_classes, 1.0 / B)
        assert torch.equal(c["t"], t) or (c["t"] - t).abs().max().item() <= 1e-15
        if B > 1 and mode and thr is None:
            assert c["t"][1, y[0]].item() == pytest.approx((1 - BU.f32r(s)) + BU.f32r(s) / N_, abs=1e-15)  # equal labels add
        x = c["x"].double().requires_grad_(True)
        D = B if sum_classes else B * N_
        loss = F.binary_cross_entropy_with_logits(x, t, reduction="none").sum() / D
        loss.backward()
        assert abs(c["loss"] - loss.item()) <= 1e-12 * abs(loss.item())
        # dlogits = d(loss) / d(x) * (B * grad_scale): the trainer hands grad_scale = 1 / B, which the kernel sees as a float
        want = x.grad * (B * BU.f32r(1.0 / B))
        assert (c["grad"] - want).abs().max().item() <= 1e-12 * want.abs().max().item() + 1e-300
        assert bool(torch.isfinite(c["grad"]).all()) and abs(c["loss"]) < 3.4e38


def test_inputs_have_the_values_the_kernel_tests_need():
    for B, N_ in BU.SHAPES:
        for dtype in (BU.F32, BU.BF16):
            x = BU.logits(B, N_, dtype)
            if (B, N_) in BU.PLAIN:
                assert float(x.abs().max()) <= 12.0
                continue
            assert bool(torch.isfinite(x).all()) and bool((x.abs() > 2.9e38).any())
            if B * N_ >= 5:
                for v in (80.0, -80.0, 0.0):
                    assert bool((x == v).any()), (B, N_, v)
                assert bool((x > 2.9e38).any()) and bool((x < -2.9e38).any())
        y = BU.labels(B, N_)
        if B > 1:
            assert y[1] == y[0]
        if B > 2 and N_ > 1:
            assert y[2] != y[1]
    assert (4, 1027) in BU.SHAPES and 1027 > 4 * 256  # a fifth round for three threads
    # every shape but the one-row one has a row of ordinary logits, whose row term is held to a bound of ordinary size
    for B, N_ in BU.SHAPES:
        if B > 1 and N_ > 1:
            assert bool((BU.logits(B, N_, BU.F32).abs().max(1).values <= 80.0).any()), (B, N_)
    # one header puts the threshold between the partner's weight and the own label's, for both smoothings
    lam = BU.f32r(0.9)
    assert (1, 0.9) in BU.HEADERS and BU.THRESHOLDS == (None, 0.2)
    for s_ in BU.SMOOTHING:
        for N_ in (10, 16, 33, 1000, 1027):
            assert (1 - s_) * (1 - lam) + s_ / N_ < 0.2 - BU.THR_MARGIN and (1 - s_) * lam + s_ / N_ > 0.2 + BU.THR_MARGIN


# ---- launch lists ---------------------------------------------------------------------------------------------------------
def _step(classes=16, dtype=torch.bfloat16, **kw):
    return TrainStep(backbones.vovnet19_slim_ese(), classes, 2, 64, dtype, device="cpu", plan_only=True, **kw)


def _ptr(op, k):
    return (op.ptr[k].base, op.ptr[k].offset)


def _raw(op):
    return ctypes.string_at(ctypes.addressof(op), ctypes.sizeof(N.Op))


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bce_swaps_the_one_loss_op(dtype, mix):
    ce = _step(dtype=dtype, mix=mix)
    ts = _step(dtype=dtype, mix=mix, loss="bce", bce_target_threshold=0.2, bce_sum_classes=True, label_smoothing=0.1)
    assert ts.loss_name == "bce" and ce.loss_name == "ce"
    n = ts.prog.n_fwd
    assert n == ce.prog.n_fwd and ts.prog.n_bwd == ce.prog.n_bwd and ts.n_opt == ce.n_opt
    # every forward op in front of the loss is the cross-entropy list's, byte for byte
    # (but for the filter packs of the data gradients, hoisted into it: their buffers are reserved behind the loss's)
    for k in range(n - 1):
        assert ts.prog.fwd_ops[k].kind == ce.prog.fwd_ops[k].kind
        if (ts.prog.fwd_ops[k].kind & 0xFFFF) != N.OP_PACK_DGRAD:
            assert _raw(ts.prog.fwd_ops[k]) == _raw(ce.prog.fwd_ops[k]), k
    assert [ts.prog.bwd_ops[k].kind for k in range(ts.prog.n_bwd)] == [ce.prog.bwd_ops[k].kind for k in range(ce.prog.n_bwd)]
    op, cop = ts.prog.fwd_ops[n - 1], ce.prog.fwd_ops[n - 1]
    assert (op.kind, cop.kind) == (N.OP_BCE, N.OP_XENT)
    assert ts.prog.kind_histogram["bce"] == 1 and "xent" not in ts.prog.kind_histogram
    # logits, labels, loss, dlogits and the mix block where xent has them
    assert [_ptr(op, k) for k in range(5)] == [_ptr(cop, k) for k in range(5)]
    assert _ptr(op, 1) == (E.LABELS, 0) and (op.ptr[4].base == E.HYPER) == mix
    assert [op.i[k] for k in range(5)] == [cop.i[k] for k in range(5)]
    assert op.i[2] == 2 and op.i[3] == 16 and op.i[5] == N.VT_BCE_SUM_CLASSES | N.VT_BCE_THRESHOLD
    assert (op.f[0], op.f[1], op.f[2]) == (0.1, 0.5, 0.2) and (cop.f[0], cop.f[1]) == (0.1, 0.5)
    # the row terms: double[B] of its own in the arena
    base, off = _ptr(op, 5)
    assert base == E.ARENA and off % 8 == 0 and off + 8 * 2 <= ts.prog.arena_bytes
    taken = [(_ptr(o, k), k) for o in (ts.prog.fwd_ops[j] for j in range(n - 1)) for k in range(N.VT_OP_MAX_PTR)
             if o.ptr[k].base == E.ARENA]
    assert all(not (off <= p[1] < off + 16) for p, _ in taken)
    plain = _step(dtype=dtype, mix=mix, loss="bce")
    pop = plain.prog.fwd_ops[n - 1]
    assert pop.i[5] == 0 and pop.f[2] == 0.0


def test_widened_head_reads_ten_classes():
    ts = _step(classes=10, loss="bce")
    n = ts.prog.n_fwd
    op, memset = ts.prog.fwd_ops[n - 1], ts.prog.fwd_ops[n - 2]
    assert op.kind == N.OP_BCE and op.i[3] == 10 and op.i[0] == op.i[1] == 16  # 16 columns, 10 of them classes
    assert memset.kind == N.OP_MEMSET and _ptr(memset, 0) == _ptr(op, 3) and int(memset.f[0]) == 2 * 16 * 2
    ce = _step(classes=10)
    assert _raw(ce.prog.fwd_ops[n - 2]) == _raw(memset)


def test_every_optimiser_and_clip_builds_with_bce():
    for kw in (dict(optimizer="SGD"), dict(optimizer="AdamW"), dict(optimizer="Adam"), dict(optimizer="Lamb"),
               dict(clip_grad_norm=1.0), dict(deterministic=True), dict(use_graphs=True), dict(mix=True, optimizer="Lamb")):
        ts = _step(loss="bce", **kw)
        ce = _step(**kw)
        assert ts.prog.fwd_ops[ts.prog.n_fwd - 1].kind == N.OP_BCE
        raw = lambda t: ctypes.string_at(ctypes.addressof(t.opt_ops), t.n_opt * ctypes.sizeof(N.Op))  # noqa: E731
        assert raw(ts) == raw(ce)  # the optimiser list does not know the loss


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_data_parallel_plan_under_gloo(monkeypatch):
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        ts = _step(loss="bce", mix=True, exchange="allreduce", bucket_mb=0.05)
        ce = _step(mix=True, exchange="allreduce", bucket_mb=0.05)
        assert ts.dp and ts.bucketer is not None and len(ts.bwd_cuts) > 1
        assert ts.prog.fwd_ops[ts.prog.n_fwd - 1].kind == N.OP_BCE
        assert ts.prog.fwd_ops[ts.prog.n_fwd - 1].f[1] == 0.5  # the rank's own batch: the all-reduce averages over ranks
        assert list(ts.bwd_cuts) == list(ce.bwd_cuts) and ts.cut_buckets == ce.cut_buckets
    finally:
        dist.destroy_process_group()


def test_refusals():
    assert LOSSES == ("ce", "bce")
    for bad in ("BCE", "mse", None):
        with pytest.raises(ValueError, match="ce, bce"):
            _step(loss=bad)
    with pytest.raises(ValueError, match="loss='bce'"):
        _step(bce_target_threshold=0.2)
    with pytest.raises(ValueError, match="loss='bce'"):
        _step(loss="ce", bce_sum_classes=True)
    with pytest.raises(ValueError, match="bce_target_threshold"):
        _step(loss="bce", bce_target_threshold=float("nan"))
    with pytest.raises(ValueError, match="SGD, AdamW, Adam"):  # the refusals that were there stay
        _step(loss="bce", optimizer="RMSprop")


def test_library_has_the_symbol_and_the_op():
    assert "vt_sigmoid_bce" in N.SYMBOLS and N.lib().vt_sigmoid_bce is not None
    assert N.OP_BCE == N.OP_LAMB_APPLY + 1 == 122 and N.OP_NAMES[N.OP_BCE] == "bce"  # appended behind the parent's kinds
    assert (N.OP_XENT, N.OP_XENT_EVAL) == (18, 39)  # the kinds a parent list can hold keep their numbers
    text = (ROOT / "include" / "vt_amd.h").read_text()
    assert "#define VT_BCE_SUM_CLASSES 1" in text and "#define VT_BCE_THRESHOLD 2" in text
    assert (N.VT_BCE_SUM_CLASSES, N.VT_BCE_THRESHOLD) == (1, 2)


# tests/golden/program_digests.txt: every digest tools/program_digest.py prints on the parent commit (478 lines, one label printed twice; the tool's
# 479th output line is gloo's greeting).  The whole
# comparison is `python tools/program_digest.py | grep -v Gloo | cmp - tests/golden/program_digests.txt` (a minute: too long for a test, run
# before merge, NOTEBOOK 37.2); here every trainer plan of the small model, with both settings of VT_PW_MIN_MB.
def _golden():
    out = {}
    for line in (ROOT / "tests" / "golden" / "program_digests.txt").read_text().splitlines():
        label, _, digest = line.rpartition(" ")
        out[label] = digest
    return out


def test_default_arguments_build_the_parent_lists():
    spec = importlib.util.spec_from_file_location("program_digest", ROOT / "tools" / "program_digest.py")
    pd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd)
    golden = _golden()
    assert len(golden) >= 477 and not any("RAISES" in k for k in golden)
    saved = {k: os.environ.get(k) for k in pd.SWITCHES}
    checked = 0
    try:
        for vname, variant in pd.PLAN_VARIANTS:
            for env, tag in (({}, ""), ({"VT_PW_MIN_MB": "0"}, " VT_PW_MIN_MB=0")):
                label = f"plan vovnet19_slim_ese {vname}{tag}"
                want = golden[label]
                kw = dict(variant)
                classes, dtype = kw.pop("classes", 16), kw.pop("dtype", torch.bfloat16)

                def mk(**more):
                    pd.set_env(env)
                    return TrainStep(backbones.vovnet19_slim_ese(), classes, 2, 64, dtype, device="cpu", plan_only=True, **kw, **more)

                assert pd.plan_digest(mk()) == want, label
                assert pd.plan_digest(mk(loss="ce", bce_target_threshold=None, bce_sum_classes=False)) == want, label
                if not tag:
                    assert pd.plan_digest(mk(loss="bce")) != want, label
                checked += 1
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert checked == 14


# ---- bounds: the float32 restatement stays within half of what the GPU tests allow ----------------------------------------
@pytest.mark.parametrize("dtype", [BU.F32, BU.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", BU.SHAPES, ids=str)
def test_f32_restatement_within_half_the_counted_bounds(shape, dtype):
    B, N_ = shape
    worst_g = worst_l = 0.0
    for header, s, thr, sum_classes in BU.combos():
        for gs in (1.0 / B, 3.0):
            c = BU.case(B, N_, dtype, header, s, thr, sum_classes, gs)
            t32 = BU.target(c["y"], N_, header, s, thr, torch.float32)
            loss, grad, _, _, rows, _ = BU.bce(c["x"], t32, gs, sum_classes)
            assert bool(((rows - c["rows"]).abs() <= 0.5 * c["row_bounds"]).all())
            assert loss.dtype == torch.float32 and grad.dtype == torch.float32
            assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss))
            lfrac = abs(loss.item() - c["loss"]) / (0.5 * c["loss_bound"])
            half = 0.5 * c["grad_f32_part"] + BU.TINY  # (the subnormal floor is the format's as well)
            if dtype == BU.BF16:  # the store is the format's, not an estimate: it stays whole (head_neck_util.half_bound)
                grad = grad.to(torch.bfloat16).float()
                half = half + BU.BF16_U * c["grad"].abs()
            err = (grad.double() - c["grad"]).abs()
            ok = half > 0
            gfrac = (err[ok] / half[ok]).max().item() if bool(ok.any()) else 0.0
            assert not bool((err[~ok] > 0).any())
            worst_g, worst_l = max(worst_g, gfrac), max(worst_l, lfrac)
            assert lfrac <= 1.0 and gfrac <= 1.0, (header, s, thr, sum_classes, gs, lfrac, gfrac)
            # what the bounds have to catch: a gradient that lost its 1 / N, a loss that dropped its smoothing
            if N_ > 1 and not sum_classes:
                assert bool(((c["grad"] * N_ - c["grad"]).abs() > 4 * c["grad_bound"]).any())
    print(f"{shape} {BU.DNAME[dtype]}: float32 restatement at {worst_g:.3f} (gradient) and {worst_l:.3f} (loss) of half the bounds")


def test_bounds_are_no_wider_than_the_cross_entropy_ones():
    # tests/head_neck_util.py holds xent's gradient to 1e-5 (p + q): the counted bound here is a tenth of that
    assert BU.K_GRAD * BU.U < 1e-6 and BU.K_LOSS * BU.U < 1.1e-6


# ---- the learning rates of the GPU step tests -------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["SGD", "Lamb"])
def test_step_learning_rates_keep_the_f32_restatement_within_a_tenth_of_the_tolerance(optimizer):
    want = BU.ref_steps(optimizer, torch.float64)
    got = BU.ref_steps(optimizer, torch.float32)
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print(f"{optimizer} lr {BU.STEP_LR[optimizer]}: float64 losses {want}, the float32 run off by {rel}")
    assert all(r <= 0.1 * BU.STEP_RTOL for r in rel)
    # the rates are not so small that the tolerance would pass an optimiser that does nothing
    frozen = BU.ref_steps(optimizer, torch.float64, lr=0.0)
    print(f"{optimizer} without updates: {frozen}")
    assert frozen[0] == want[0] and abs(frozen[2] - want[2]) > 2 * BU.STEP_RTOL * abs(want[2])
