"""Weight EMA of the fused train step on the device: the shadow buffers against the float64 recurrence of tests/ema_util.py
over SNAPSHOTS of the trained buffers (so the check does not depend on the model's arithmetic), skipped steps, captured
graphs, validate(ema=True) against a twin that loaded the average, and the state_dict round trip.

Models: darknet_yolov5n (BatchNorm: the running statistics are averaged, the batch counters copied) and the smallest ViT
of tests/test_vit_gpu.py (no BatchNorm; AdamW), f32 and bf16."""
import pytest
import torch

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.backbones import ViT
from vision_toolbox.trainer import TrainStep

import ema_util as EU

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MODELS = ["darknet_yolov5n", "vit"]
DECAY = 0.9  # alpha = 0.1: four steps move the average visibly


@pytest.fixture(autouse=True)
def _lib_launched():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


def _make(model, dtype, **kw):
    if model == "vit":
        ts = TrainStep(ViT(64, 1, 2, 4, 16, layer_scale_init=0.5), 10, 3, 16, dtype, lr=1e-2, weight_decay=0.0,
                       optimizer="AdamW", include_pool=False, deterministic=True, device="cuda", **kw)
    else:
        ts = TrainStep(backbones.darknet_yolov5n(), 16, 2, 64, dtype, lr=0.05, deterministic=True, device="cuda", **kw)
    with torch.no_grad():
        filler.fill_module(ts.model, "ema.")
    ts.weights_changed()
    return ts


def _batch(model, k):
    b, s, c = (3, 16, 10) if model == "vit" else (2, 64, 16)
    x = filler.images(b, s)
    return torch.roll(x, k, dims=-1).cuda(), ((filler.labels(b, c) + k) % c).cuda()


def _same_validation(a: dict, b: dict) -> bool:
    """two validate() results of bit-identical logits: hits and rows are equal; the loss is vt_softmax_xent_eval's sum of one
    f32 atomicAdd per row, whose order -- and with three or more rows its last bit -- varies from run to run on the SAME
    logits (the ViT here has three rows; two terms commute).  So the logits carry the bit-exact check and the loss is
    held to the rounding of that sum: B - 1 adds of at most u = 2^-24 of the (positive) total in either run."""
    rows = a["count"]
    return a["correct"] == b["correct"] and rows == b["count"] and a["acc"] == b["acc"] and \
        abs(a["loss"] - b["loss"]) <= 2 * (rows - 1) * 2.0 ** -24 * max(abs(a["loss"]), abs(b["loss"]))


def _snap(ts):
    torch.cuda.synchronize()
    return ts.store.pflat.clone(), ts.store.sflat.clone(), ts.store.nflat.clone()


def _run(ts, model, n, hook=None):
    snaps, emas = [], []
    for k in range(n):
        if hook is not None:
            hook(ts, k)
        ts.step(*_batch(model, k))
        snaps.append(_snap(ts))
        emas.append(ts._ema.clone())
    return snaps, emas


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("model", MODELS)
def test_shadow_buffers_follow_the_recurrence_over_snapshots(model, dtype):
    ts = _make(model, dtype, ema_decay=DECAY)
    with pytest.raises(RuntimeError, match="no update"):
        ts.validate(*_batch(model, 0), ema=True)
    before = N.launch_count()
    snaps, _ = _run(ts, model, 4)
    assert N.launch_count() > before and ts.ema_updates() == 4 == ts.steps_done
    assert not torch.equal(snaps[0][0], snaps[3][0])  # lr > 0: the weights moved, the recurrence has something to follow
    a = EU.alpha_f32(DECAY)
    for which, got in ((0, ts.ema_pflat), (1, ts.ema_sflat)):
        ref, bound = EU.run([s[which].cpu() for s in snaps], a)[-1]
        err = (got.cpu().double() - ref).abs()
        print(f"{model} {['pflat', 'sflat'][which]}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
              f"moved {float((got - snaps[3][which]).abs().max()):.3e}")
        assert (err <= bound).all()
    if model != "vit":
        assert not torch.equal(ts.ema_sflat, snaps[3][1])  # BatchNorm running statistics are averaged, not copied
    assert torch.equal(ts.ema_nflat, snaps[3][2])  # the batch counters are copied
    if dtype == torch.bfloat16:
        assert torch.equal(ts.ema_mirror, ts.ema_pflat.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("model", MODELS)
def test_ema_steps_two_skips_every_second_step(model, dtype):
    ts = _make(model, dtype, ema_decay=DECAY, ema_steps=2)
    snaps, emas = _run(ts, model, 4)
    words = slice(64, None)  # everything behind the control words
    assert torch.equal(emas[1][words], emas[0][words]) and torch.equal(emas[3][words], emas[2][words])
    assert not torch.equal(emas[2][words], emas[1][words])
    assert ts.ema_updates() == 2 and ts.steps_done == 4
    assert torch.equal(emas[0][64: 64 + 4 * ts.store.pflat.numel()].view(torch.float32), snaps[0][0])  # update 0 is a copy
    ref, bound = EU.run([s[0].cpu() for s in snaps], EU.alpha_f32(DECAY), period=2)[-1]
    assert ((ts.ema_pflat.cpu().double() - ref).abs() <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("model", MODELS)
def test_captured_graph_equals_the_eager_list(model, dtype):
    def hook(ts, k):
        if k == 2:
            ts.set_ema_decay(0.5)  # like set_lr: alpha lives on the device, the captured graph follows

    _, eager = _run(_make(model, dtype, ema_decay=DECAY, ema_steps=2), model, 4, hook)
    ts = _make(model, dtype, ema_decay=DECAY, ema_steps=2, use_graphs=True)
    _, graph = _run(ts, model, 4, hook)
    for k in range(4):
        assert torch.equal(eager[k], graph[k]), k
    assert ts._graphs is not None and ts._ema_ctl_f[N.VT_EMA_ALPHA].item() == 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("model", MODELS)
def test_validate_ema_equals_a_twin_that_loaded_the_average(model, dtype):
    ts = _make(model, dtype, ema_decay=DECAY)
    plain = _make(model, dtype)  # built without ema_decay, trained alike
    for k in range(3):
        ts.step(*_batch(model, k))
        plain.step(*_batch(model, k))
    x, y = _batch(model, 7)
    # the average does not disturb training: the raw weights validate as a twin's without ema_decay
    raw = ts.validate(x, y)
    raw_logits = ts.eval_logits().clone()
    assert _same_validation(raw, plain.validate(x, y)) and torch.equal(raw_logits, plain.eval_logits())
    # ... and validate(ema=True) is the same program over the shadow buffers
    avg = ts.validate(x, y, ema=True)
    avg_logits = ts.eval_logits().clone()
    twin = _make(model, dtype)
    twin.model.load_state_dict(ts.ema_state_dict())
    twin.weights_changed()
    assert _same_validation(avg, twin.validate(x, y)) and torch.equal(avg_logits, twin.eval_logits())
    assert not torch.equal(avg_logits, raw_logits)
    assert _same_validation(ts.validate(x, y), raw) and torch.equal(ts.eval_logits(), raw_logits)  # the bases went back


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_state_dict_round_trip_and_resume(dtype):
    model = "darknet_yolov5n"
    ts = _make(model, dtype, ema_decay=DECAY)
    _run(ts, model, 2)
    sd = ts.ema_state_dict()
    assert list(sd) == list(ts.model.state_dict()) and all(v.shape == ts.model.state_dict()[k].shape for k, v in sd.items())
    other = _make(model, dtype, ema_decay=DECAY)
    other.load_ema_state_dict(sd, updates=ts.ema_updates())
    torch.cuda.synchronize()
    assert torch.equal(other._ema[64:], ts._ema[64:]) and other.ema_updates() == 2
    back = other.ema_state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # resuming: with the trained state loaded as well, the next step blends exactly as the original's next step does
    other.model.load_state_dict(ts.model.state_dict())
    other.mflat.copy_(ts.mflat)
    other.weights_changed()
    ts.step(*_batch(model, 2))
    other.step(*_batch(model, 2))
    torch.cuda.synchronize()
    assert torch.equal(other._ema[64:], ts._ema[64:]) and other.ema_updates() == 3
