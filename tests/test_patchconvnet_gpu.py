"""PatchConvNet through the module API and the fused train step on the GPU against the fixtures of
tools/gen_golden_patchconvnet.py / tools/gen_golden_patchconvnet_train.py (the unmodified reference on CPU behind the two
torchvision stand-ins): cases a, b, c x their modes x {f32, bf16}.

Bounds are those of tests/test_cait_gpu.py, unchanged.  f32: F32_TOL 2e-4 forward, 4 x for dx and parameter gradients, with the
clamp_min(1e-3 sqrt(numel)) denominator.  bf16: forward BF16_TOL 3e-2; dx and parameter gradients min(4 x the stored floor of
the SAME array, 0.25).  Arrays of more than 4096 elements are compared on the 4096 elements the fixture holds
(patchconvnet_util.stored).  Case c also holds the BatchNorm buffers after one training forward: compared at F32_TOL / BF16_TOL.
Train step: the three losses at rtol 1e-3 (f32) / 1e-2 (bf16), the step-1 gradients at the bounds above."""
import numpy as np
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox.backbones import PatchConvNet
from vision_toolbox.trainer import TrainStep

from oracle import filler

import patchconvnet_util as U

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 2e-4, 3e-2
DTYPES = [torch.float32, torch.bfloat16]
_IDS = [f"{n}-{mode}" for n, mode in U.CASE_MODES]


def _gtol(g, dtype, mode, key):
    if dtype == torch.float32:
        return 4 * F32_TOL
    return min(4 * float(g[f"floor/bf16/{mode}/{key}"]), 0.25)


def _setup(name, dtype, mode):
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    m = m.cuda().train(mode == "train")
    m.compute_dtype = dtype
    return g, m, x.cuda().requires_grad_(True), r.cuda()


def _check_grads(g, m, x, dtype, mode, tag, frozen=()):
    worst = 0.0
    if x.grad is not None:
        e, b = U.gerr(U.stored("dx", x.grad), U.t(g[f"{mode}/dx"])), _gtol(g, dtype, mode, "dx")
        print(f"{tag}: dx {e:.3e} (bound {b:.3e})")
        assert e < b, "dx"
    for k, p in m.named_parameters():
        if k.startswith(frozen):
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        e, b = U.gerr(U.stored("grad/" + k, p.grad), U.t(g[f"{mode}/grad/{k}"])), _gtol(g, dtype, mode, "grad/" + k)
        worst = max(worst, e / b)
        print(f"{tag}: grad {k} {e:.3e} (bound {b:.3e})")
        assert e < b, f"grad {k}: {e} >= {b}"
    print(f"{tag}: worst parameter gradient at {worst:.2f} of its bound")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,mode", U.CASE_MODES, ids=_IDS)
def test_forward_backward_match_the_reference(name, mode, dtype):
    """train-mode and eval-mode BatchNorm (cases a, c), LayerNorm blocks (case b); the running statistics after the training
    forward (case c)"""
    g, m, x, r = _setup(name, dtype, mode)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    y = m(x)
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"
    assert tuple(y.shape) == g[f"{mode}/y"].shape and y.dim() == 2 and y.dtype == dtype
    ey = U.rel(y.detach().float().cpu(), U.t(g[f"{mode}/y"]))
    print(f"{name}/{mode}/{dtype}: y {ey:.3e} (bound {tol:.1e})")
    assert ey < tol
    _check_grads(g, m, x, dtype, mode, f"{name}/{mode}/{dtype}")
    if name == "c" and mode == "train":
        bufs = dict(m.named_buffers())
        keys = [k[len("train/running/"):] for k in g.files if k.startswith("train/running/")]
        assert sorted(keys) == sorted(bufs) and len(keys) == 3
        for k in keys:
            want = U.t(g["train/running/" + k])
            if k.endswith("num_batches_tracked"):
                assert int(bufs[k]) == int(want) == 1
                continue
            e = U.rel(bufs[k].float().cpu(), want)
            print(f"c/train/{dtype}: {k} {e:.3e} (bound {tol:.1e})")
            assert e < tol, k


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_no_grad_forward(name, dtype):
    g, m, x, _ = _setup(name, dtype, "eval")
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    before = N.launch_count()
    with torch.no_grad():
        y = m(x)
        maps = m.get_feature_maps(x)
    torch.cuda.synchronize()
    assert N.launch_count() > before
    e = U.rel(y.float().cpu(), U.t(g["eval/y"]))
    print(f"{name}/{dtype} no-grad: y {e:.3e} (bound {tol:.1e})")
    assert not y.requires_grad and tuple(y.shape) == g["eval/y"].shape and e < tol
    assert len(maps) == 1 and torch.equal(maps[0], y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_frozen_stem(dtype):
    g, m, x, r = _setup("a", dtype, "train")
    m.stem.requires_grad_(False)
    x = x.detach()  # nothing in front of the trunk needs a gradient: no stem data or filter gradients
    before = N.launch_count()
    y = m(x)
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    assert N.launch_count() > before
    _check_grads(g, m, x, dtype, "train", f"frozen stem/{dtype}", frozen=("stem.",))


def test_refusals_on_a_cuda_tensor():
    before = N.launch_count()
    x = torch.randn(2, 3, 32, 32, device="cuda")
    m = PatchConvNet(64, 1).cuda().train()  # the reference default drop_path = 0.3
    with pytest.raises(NotImplementedError, match="drop_path"):
        m(x)
    assert m.eval()(x).shape == (2, 64)  # (unused in eval mode)
    with pytest.raises(NotImplementedError, match="drop_path"):
        m.train()(x)  # (the refusal does not depend on what was compiled before)
    m = PatchConvNet(32, 1, drop_path=0.0).cuda().eval()  # embed_dim // 8 = 4: a chunk of f32, not of bf16
    assert m(x).shape == (2, 32)
    with pytest.raises(NotImplementedError, match="embed_dim"):
        m(x.bfloat16())
    with pytest.raises(NotImplementedError, match="embed_dim"):
        PatchConvNet(16, 1, drop_path=0.0).cuda().eval()(x)
    with pytest.raises(NotImplementedError, match="too large"):
        PatchConvNet(64, 1, drop_path=0.0).cuda().eval()(torch.zeros(1, 3, 1536, 1536, device="cuda"))
    # (exchange="sharded" needs a process group: tests/test_patchconvnet_cpu.py refuses it under a one-rank gloo group)
    with pytest.raises(NotImplementedError, match="drop_path"):
        TrainStep(PatchConvNet(64, 1), 10, 2, 32, torch.bfloat16, include_pool=False, device="cuda")
    assert N.launch_count() > before


def _train_step(g, dtype, **kw):
    lr, wd, norm_wd, bias_wd, smooth, _ = [float(v) for v in g["hyper"]]
    m = PatchConvNet(*U.TRAIN_ARGS, **U.TRAIN_KW)
    ts = TrainStep(m, U.TRAIN_CLASSES, U.TRAIN_BATCH, U.TRAIN_SIZE, dtype, lr=lr, weight_decay=wd, norm_weight_decay=norm_wd,
                   bias_weight_decay=bias_wd, label_smoothing=smooth, optimizer="AdamW", include_pool=False, device="cuda", **kw)
    pre = str(g["recipe"][0])
    with torch.no_grad():
        filler.fill_module(ts.model, pre)
        for k, p in ts.model[0].named_parameters():
            if (p.dim() == 1 and k.endswith(("weight", "gamma"))) or k.rsplit(".", 1)[-1].startswith("layer_scale"):
                p.add_(1.0)
    ts.weights_changed()
    assert list(ts.model.state_dict().keys()) == [str(k) for k in g["keys"]]
    return ts


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_three_adamw_steps_match_the_reference(dtype, deterministic):
    g = np.load(U.GOLDEN / "patchconvnet_train.npz")
    assert len(g["zero_grad_keys"]) == 0
    ts = _train_step(g, dtype, deterministic=deterministic)
    images = filler.images(U.TRAIN_BATCH, U.TRAIN_SIZE).cuda()
    labels = filler.labels(U.TRAIN_BATCH, U.TRAIN_CLASSES).cuda()
    rtol = 1e-3 if dtype == torch.float32 else 1e-2
    losses = []
    for step in range(3):
        before = N.launch_count()
        ts.step(images, labels)
        losses.append(ts.loss())
        assert N.launch_count() > before
        if step == 0:
            torch.cuda.synchronize()
            worst = 0.0
            for k, p in ts.model.named_parameters():
                _, off, n = ts.store.where(p)
                got = ts.gflat[off:off + n].view(p.shape if p.dim() != 4 else (p.shape[0], p.shape[2], p.shape[3], p.shape[1]))
                if p.dim() == 4:
                    got = got.permute(0, 3, 1, 2)
                b = 4 * F32_TOL if dtype == torch.float32 else min(4 * float(g[f"floor/bf16/grad/{k}"]), 0.25)
                e = U.gerr(got, U.t(g["grad/" + k]).float())
                worst = max(worst, e / b)
                print(f"train/{dtype}: step-1 grad {k} {e:.3e} (bound {b:.3e})")
                assert e < b, k
            print(f"train/{dtype}: worst step-1 gradient at {worst:.2f} of its bound")
    want = [float(v) for v in g["loss64"]]
    for a, b in zip(losses, want):
        print(f"train/{dtype} deterministic={deterministic}: loss {a:.6f} reference {b:.6f} rel {abs(a - b) / b:.2e} (rtol {rtol:.0e})")
    for a, b in zip(losses, want):
        assert abs(a - b) <= rtol * abs(b)


def test_deterministic_steps_are_bit_identical():
    g = np.load(U.GOLDEN / "patchconvnet_train.npz")
    images = filler.images(U.TRAIN_BATCH, U.TRAIN_SIZE).cuda()
    labels = filler.labels(U.TRAIN_BATCH, U.TRAIN_CLASSES).cuda()
    finals = []
    before = N.launch_count()
    for _ in range(2):
        ts = _train_step(g, torch.bfloat16, deterministic=True)
        for _ in range(2):
            ts.step(images, labels)
        torch.cuda.synchronize()
        finals.append(ts.store.pflat.clone())
    assert torch.equal(finals[0], finals[1]) and N.launch_count() > before
