"""loss="bce" through the fused train step: three steps of SGD and of Lamb on darknet_yolov5n at batch 4 @64 with a different
mix block per step against the float64 restatement of tests/bce_util.py, deterministic steps bit for bit (the loss scalar
included: vt_sigmoid_bce adds it in a fixed order), and a captured graph that follows a changed mix block."""
import numpy as np
import pytest
import torch

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.trainer import TrainStep

import bce_util as BU

pytestmark = pytest.mark.gpu


def _step(dtype, **kw):
    ts = TrainStep(getattr(backbones, BU.STEP_MODEL)(), BU.STEP_CLASSES, BU.STEP_BATCH, BU.STEP_SIZE, dtype, momentum=0.9,
                   weight_decay=BU.STEP_WD, label_smoothing=BU.STEP_SMOOTHING, device="cuda", mix=True, loss="bce", **kw)
    filler.fill_module(ts.model, "bce.")
    ts.weights_changed()
    return ts


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("optimizer", ["SGD", "Lamb"])
def test_train_steps_match_float64_losses(optimizer, dtype):
    """The losses of three steps within 1e-2 of the float64 restatement's, the bound of the step tests of
    tests/test_resnet_gpu.py, in both dtypes; in f32 the first loss (forward only) within 1e-4, as there.  The learning rates
    are those at which the restatement's own float32 run stays within a tenth of the bound (tests/test_bce_cpu.py)."""
    x, y = BU.step_inputs()
    want = BU.ref_steps(optimizer)
    extra = dict(eps=BU.LAMB_EPS, lamb_max_grad_norm=1.0) if optimizer == "Lamb" else {}
    ts = _step(dtype, lr=BU.STEP_LR[optimizer], optimizer=optimizer, **extra)
    assert ts.prog.kind_histogram["bce"] == 1 and "xent" not in ts.prog.kind_histogram
    before = N.launch_count()
    got = []
    for i in range(3):
        ts.set_mix(*BU.STEP_MIX[i])
        ts.step(x.cuda(), y.cuda())
        got.append(ts.loss())
    assert N.launch_count() > before
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print(f"bce steps {optimizer} {dtype}: {got} against {want}: off by {rel}")
    np.testing.assert_allclose(got, want, rtol=BU.STEP_RTOL)
    if dtype == torch.float32:
        assert got[0] == pytest.approx(want[0], rel=1e-4)
    val = ts.validate(x.cuda(), y.cuda())  # unchanged: plain cross-entropy in eval mode
    assert np.isfinite(val["loss"]) and val["count"] == BU.STEP_BATCH


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_steps_are_bit_identical_with_their_losses(dtype):
    x, y = BU.step_inputs()
    x, y = x.cuda(), y.cuda()
    states = []
    for _ in range(2):
        ts = _step(dtype, lr=1e-2, deterministic=True, bce_target_threshold=0.2, bce_sum_classes=True)
        losses = []
        for i in range(3):
            ts.set_mix(*BU.STEP_MIX[i])
            ts.step(x, y)
            losses.append(ts.loss())
        torch.cuda.synchronize()
        states.append((losses, ts.store.pflat.clone(), ts.gflat.clone(), ts.mflat.clone(), ts.store.sflat.clone()))
        del ts
    for a, b in zip(states[0][1:], states[1][1:]):
        assert torch.equal(a, b)
    assert states[0][0] == states[1][0] and all(np.isfinite(l) for l in states[0][0])  # the loss too: no float atomic
    assert len(set(states[0][0])) == 3


def test_captured_graph_follows_a_changed_mix_block():
    x, y = BU.step_inputs()
    x, y = x.cuda(), y.cuda()
    runs = {}
    for graphs in (False, True):
        ts = TrainStep(getattr(backbones, BU.STEP_MODEL)(), BU.STEP_CLASSES, BU.STEP_BATCH, BU.STEP_SIZE, torch.float32, lr=0.0,
                       momentum=0.0, weight_decay=0.0, label_smoothing=BU.STEP_SMOOTHING, device="cuda", mix=True, loss="bce",
                       use_graphs=graphs)
        filler.fill_module(ts.model, "bce.")
        ts.weights_changed()
        losses, head = [], None
        for mode, lam, box in [("none", 1.0, (0, 0, 0, 0))] + BU.STEP_MIX:
            ts.set_mix(mode, lam, box)
            ts.step(x, y)
            losses.append(ts.loss())
            if graphs:
                head = head or ts._graphs["head"]
                assert ts._graphs["head"] is head  # replayed, not re-captured
        runs[graphs] = losses
    print(f"bce under graphs: {runs[True]} against eager {runs[False]}")
    # lr = 0: the weights stay, every loss is the forward pass of its own mix block
    assert runs[True] == pytest.approx(runs[False], rel=1e-6)
    assert len({round(v, 4) for v in runs[True]}) == 4
    want = BU.ref_steps("SGD", torch.float64, lr=0.0)
    assert runs[True][1:] == pytest.approx(want, rel=1e-4)
