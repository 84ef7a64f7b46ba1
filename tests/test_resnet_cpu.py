"""ResNetExtractor without a GPU: module surface (state_dict keys, shapes, parameter counts), the eager path against the
plain-torch restatement of torchvision's ResNet (tests/resnet_util.py -- a restatement, not a reference fixture: the
reference class only wraps torchvision, which is not installed), the checkpoint loader, refusals, the launch lists as the
builder compiles them on the CPU, and the 7x7 -> 4x4 space-to-depth rewrite of the stem against F.conv2d."""
import importlib.util
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import resnet_util
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.backbones import BasicBlock, Bottleneck, ResNetExtractor
from vision_toolbox.trainer import TrainStep

ROOT = Path(__file__).resolve().parents[1]
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _keys(depths, convs_per_block):
    """torchvision's state_dict keys without fc.*, under the extractor's prefix, in registration order"""
    keys = ["conv1.weight"] + [f"bn1.{s}" for s in BN]
    for li, n in enumerate(depths, 1):
        for bi in range(n):
            p = f"layer{li}.{bi}."
            for k in range(1, convs_per_block + 1):
                keys.append(f"{p}conv{k}.weight")
                keys += [f"{p}bn{k}.{s}" for s in BN]
            # the first block of a layer changes the width (Bottleneck: always) or the stride (BasicBlock: layers 2-4)
            if bi == 0 and (convs_per_block == 3 or li > 1):
                keys.append(f"{p}downsample.0.weight")
                keys += [f"{p}downsample.1.{s}" for s in BN]
    return ["feat_extractor." + k for k in keys]


def test_state_dict_keys_are_torchvisions():
    k18 = list(ResNetExtractor("resnet18").state_dict())
    assert k18 == _keys((2, 2, 2, 2), 2)
    assert k18[:6] == ["feat_extractor.conv1.weight", "feat_extractor.bn1.weight", "feat_extractor.bn1.bias",
                       "feat_extractor.bn1.running_mean", "feat_extractor.bn1.running_var",
                       "feat_extractor.bn1.num_batches_tracked"]
    assert "feat_extractor.layer2.0.downsample.1.running_var" in k18 and "feat_extractor.layer1.0.downsample.0.weight" not in k18
    k50 = list(ResNetExtractor("resnet50").state_dict())
    assert k50 == _keys((3, 4, 6, 3), 3)
    assert "feat_extractor.layer1.0.downsample.0.weight" in k50 and "feat_extractor.layer4.2.conv3.weight" in k50
    assert not any("fc." in k or "avgpool" in k for k in k18 + k50)
    # ... and the restatement's own keys are the same ones plus fc.*
    ref_keys = [k for k in resnet_util.RefResNet("resnet50").state_dict() if not k.startswith("fc.")]
    assert ["feat_extractor." + k for k in ref_keys] == k50


@pytest.mark.parametrize("name,count", [("resnet18", 11_176_512), ("resnet34", 21_284_672), ("resnet50", 23_508_032),
                                        ("resnet101", 42_500_160)])
def test_parameter_counts_without_fc(name, count):
    """torchvision's published totals minus the 1000-class fc"""
    assert sum(p.numel() for p in ResNetExtractor(name).parameters()) == count


def test_surface():
    m = ResNetExtractor("resnet18")
    assert m.out_channels_list == (64, 64, 128, 256, 512) and m.stride == 32 and m.get_last_out_channels() == 512
    assert ResNetExtractor("resnet50").out_channels_list == (64, 256, 512, 1024, 2048)
    assert ResNetExtractor("wide_resnet50_2").out_channels_list == (64, 256, 512, 1024, 2048)
    assert [n for n, _ in m.feat_extractor.named_children()] == ["conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3",
                                                                 "layer4"]
    assert isinstance(m.feat_extractor.layer1[0], BasicBlock) and BasicBlock.expansion == 1 and Bottleneck.expansion == 4
    b = ResNetExtractor("resnet50").feat_extractor.layer2[0]
    assert isinstance(b, Bottleneck) and b.conv2.stride == (2, 2) and b.conv1.stride == (1, 1)  # v1.5: the stride on conv2
    w = ResNetExtractor("wide_resnet50_2").feat_extractor.layer1[0]
    assert w.conv2.in_channels == 128 and w.conv3.out_channels == 256
    x = ResNetExtractor("resnext50_32x4d").feat_extractor.layer1[0]
    assert x.conv2.groups == 32 and x.conv2.in_channels == 128
    m.eval()
    with torch.no_grad():
        maps = m.get_feature_maps(torch.rand(1, 3, 64, 64))
        assert [tuple(t.shape) for t in maps] == [(1, 64, 32, 32), (1, 64, 16, 16), (1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 2, 2)]
        assert torch.equal(m(torch.ones(1, 3, 64, 64)), m.get_feature_maps(torch.ones(1, 3, 64, 64))[-1])
    # torchvision's initialisation: kaiming-normal fan_out, BatchNorm 1 / 0, eps 1e-5, momentum 0.1
    bn = m.feat_extractor.bn1
    assert (bn.weight == 1).all() and (bn.bias == 0).all() and bn.eps == 1e-5 and bn.momentum == 0.1
    big = ResNetExtractor("resnet50").feat_extractor.layer4[0].conv2.weight
    assert abs(big.std().item() / (2.0 / (512 * 9)) ** 0.5 - 1) < 0.02


def test_refusals():
    with pytest.raises(NotImplementedError, match="pretrained"):
        ResNetExtractor("resnet18", pretrained=True)
    with pytest.raises(ValueError, match="resnet19"):
        ResNetExtractor("resnet19")


@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (4, 3, 65, 61)], ids=str)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_eager_path_matches_the_restatement(name, training, shape):
    ref, sd = resnet_util.make_pair(name)
    m = ResNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.train(training)
    ref.train(training)
    x = filler.images(shape[0], max(shape[2:]))[:, :, : shape[2], : shape[3]].contiguous()
    got = m.get_feature_maps(x)
    with torch.no_grad():
        want = ref.maps(x.double())
    assert len(got) == 5
    # f32 against float64 at the bounds tests/test_modules_gpu.py sets for f32 models: 2e-4 (F32_TOL) with running
    # statistics, 1e-3 in train mode (batch statistics over 16 samples per channel in layer4 amplify f32 rounding ~100x)
    bound = 1e-3 if training else 2e-4
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert ((g.double() - w).norm() / w.norm()).item() < bound
    if training:  # the running statistics moved the same way
        # (first BatchNorm tightly, the last one at the forward bound: as test_modules_gpu.py checks them)
        got_sd, ref_sd = m.state_dict(), ref.state_dict()
        assert torch.allclose(got_sd["feat_extractor.bn1.running_mean"].double(), ref_sd["bn1.running_mean"], rtol=1e-4, atol=1e-5)
        last, want_last = got_sd["feat_extractor.layer4.1.bn2.running_var"].double(), ref_sd["layer4.1.bn2.running_var"]
        assert ((last - want_last).norm() / want_last.norm()).item() < bound


def test_load_torchvision_ckpt(tmp_path):
    ref, sd = resnet_util.make_pair("resnet18")
    assert "fc.weight" in sd
    m = ResNetExtractor("resnet18")
    m.load_torchvision_ckpt(sd)  # fc.* is dropped, the prefix added
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k[len("feat_extractor."):]]), k
    path = tmp_path / "resnet18.pth"
    torch.save(sd, path)
    m2 = ResNetExtractor("resnet18")
    m2.load_torchvision_ckpt(path)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(KeyError, match="unexpected"):
        m.load_torchvision_ckpt(dict(sd, **{"layer9.0.conv1.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing"):
        m.load_torchvision_ckpt({k: v for k, v in sd.items() if k != "layer3.1.bn2.bias"})


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
NEW_OPS = {N.OP_BN_ADD_ACT_APPLY, N.OP_BN_ADD_ACT_FIN_APPLY, N.OP_BN_ADD_ACT_BWD_REDUCE, N.OP_BN_ADD_ACT_BWD_APPLY,
           N.OP_BN_ADD_ACT_BWD_FIN_APPLY, N.OP_STEM7_S2D, N.OP_STEM7_PACK_FILTER, N.OP_STEM7_UNPACK_WGRAD}


def _program(make, dtype, training=True, need_grad=True, size=64):
    m = make()
    m.train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(2, 3, size, size), dtype, True, need_grad)


def _kinds(prog):
    return [op.kind & 0xFFFF for op in list(prog.fwd_ops)[: prog.n_fwd]], [op.kind & 0xFFFF for op in list(prog.bwd_ops)[: prog.n_bwd]]


def test_new_op_codes_are_appended():
    assert [N.OP_BN_ADD_ACT_APPLY, N.OP_BN_ADD_ACT_FIN_APPLY, N.OP_BN_ADD_ACT_BWD_REDUCE, N.OP_BN_ADD_ACT_BWD_APPLY,
            N.OP_BN_ADD_ACT_BWD_FIN_APPLY, N.OP_STEM7_S2D, N.OP_STEM7_PACK_FILTER, N.OP_STEM7_UNPACK_WGRAD] == list(range(85, 93))
    assert N.OP_PREFIX_POOL_BWD == 84 and N.OP_NAMES[N.OP_BN_ADD_ACT_BWD_FIN_APPLY] == "bn_add_act_bwd_fin_apply"


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,blocks", [("resnet18", 8), ("resnet50", 16)])
def test_launch_lists(name, blocks, dtype):
    """the pre-activation sites (one per block) run the new passes; every other site runs what it runs in a Darknet or a
    VoVNet (whose stages open with the fused max pool)"""
    fwd, bwd = _kinds(_program(lambda: ResNetExtractor(name), dtype))
    assert fwd.count(N.OP_BN_ADD_ACT_FIN_APPLY) == blocks and fwd.count(N.OP_BN_ADD_ACT_APPLY) == 0
    assert bwd.count(N.OP_BN_ADD_ACT_BWD_REDUCE) == blocks and bwd.count(N.OP_BN_ADD_ACT_BWD_FIN_APPLY) == blocks
    assert [fwd.count(k) for k in (N.OP_STEM7_S2D, N.OP_STEM7_PACK_FILTER)] == [1, 1] and bwd.count(N.OP_STEM7_UNPACK_WGRAD) == 1
    known = set()
    for other in ("darknet53", "cspdarknet53", "vovnet39"):
        f, b = _kinds(_program(getattr(backbones, other), dtype))
        known |= set(f) | set(b)
    assert (set(fwd) | set(bwd)) - NEW_OPS <= known
    # no site adds its residual BEHIND the activation: the Darknet form of the passes never gets a residual operand here
    prog = _program(lambda: ResNetExtractor(name), dtype)
    for op in list(prog.fwd_ops)[: prog.n_fwd]:
        k = op.kind & 0xFFFF
        if k == N.OP_BN_ACT_APPLY:
            assert op.ptr[3].base == -1
        if k == N.OP_BN_FIN_APPLY:
            assert op.ptr[11].base == -1
        if k == N.OP_CONV_IGEMM:
            assert not (op.i[N.ConvDesc.flags.offset // 4] & N.VT_CONV_RESIDUAL)
    # eval without gradients: ready coefficients, and the fused inference epilogue is not taken at the block ends
    fwd_e, _ = _kinds(_program(lambda: ResNetExtractor(name), dtype, training=False, need_grad=False))
    assert fwd_e.count(N.OP_BN_ADD_ACT_APPLY) == blocks and fwd_e.count(N.OP_BN_ADD_ACT_FIN_APPLY) == 0
    # an odd image size compiles too
    _program(lambda: ResNetExtractor(name), dtype, size=61)


def test_frozen_bn_and_sync_bn_take_the_ready_coefficient_form():
    def frozen():
        m = ResNetExtractor("resnet18")
        m.train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eval()
        return m

    m = frozen()
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    fwd, bwd = _kinds(r.program(torch.zeros(2, 3, 64, 64), N.VT_BF16, True, True))
    assert fwd.count(N.OP_BN_ADD_ACT_APPLY) == 8 and fwd.count(N.OP_BN_ADD_ACT_FIN_APPLY) == 0
    assert bwd.count(N.OP_BN_ADD_ACT_BWD_FIN_APPLY) == 8  # (train = 0 inside: the statistics are constants)


@pytest.mark.parametrize("kw", [{}, {"optimizer": "AdamW"}, {"deterministic": True}, {"mix": True}, {"freeze_bn": True},
                                {"dtype": torch.float32}], ids=str)
def test_train_step_plans(kw):
    kw = dict(kw)
    dtype = kw.pop("dtype", torch.bfloat16)
    ts = TrainStep(ResNetExtractor("resnet18"), 10, 2, 64, dtype, device="cpu", plan_only=True, **kw)
    fwd, bwd = _kinds(ts.prog)
    assert bwd.count(N.OP_BN_ADD_ACT_BWD_REDUCE) == 8 and fwd.count(N.OP_STEM7_S2D) == 1
    assert ts.n_units == 20 + 1  # the stem, 16 block convolutions, 3 downsample convolutions; and the head


def test_image_gradient_and_resnext_are_refused_by_name():
    m = ResNetExtractor("resnet18")
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        r.program(torch.zeros(2, 3, 64, 64, requires_grad=True), N.VT_F32, True, True)
    mx = ResNetExtractor("resnext50_32x4d")
    rx = mx._vt_runner()
    rx.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="resnext50_32x4d"):
        rx.program(torch.zeros(2, 3, 64, 64), N.VT_BF16, True, True)
    with torch.no_grad():  # ... and it runs on CPU tensors
        assert mx.eval()(torch.rand(1, 3, 64, 64)).shape == (1, 2048, 2, 2)


# digests of existing families' programs as tools/program_digest.py prints them on the parent commit
PARENT_DIGESTS = {
    "cspdarknet53 bf16 train+grad": "bef2bf25f139a1480ef8e95a5366067cdfca2c0e69d6c591ee17c94d849012da",
    "vit_a f32 train+grad": "a690064da8cc4613f360f8472924d6b93fb1040e898c763e1194f459d2b8f85b",
}


def test_existing_programs_keep_their_digests():
    spec = importlib.util.spec_from_file_location("program_digest", ROOT / "tools" / "program_digest.py")
    pd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd)

    def digest(make, dt, size):
        pd.set_env({})
        m = make()
        m.train(True)
        r = m._vt_runner()
        r.store.ensure(torch.device("cpu"))
        return pd.program_digest(r.program(torch.zeros(2, 3, size, size), dt, True, True), r.store)

    import os

    saved = {k: os.environ.get(k) for k in pd.SWITCHES}
    try:
        assert digest(backbones.cspdarknet53, N.VT_BF16, 64) == PARENT_DIGESTS["cspdarknet53 bf16 train+grad"]
        assert digest(pd.vit("a"), N.VT_F32, pd.vit_size("a")) == PARENT_DIGESTS["vit_a f32 train+grad"]
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- the stem rewrite, restated on the host ------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(32, 32), (33, 31), (17, 18)], ids=str)
def test_stem_space_to_depth_rewrite(hw):
    """Conv2d(3, C, 7, 2, 3) == the 4x4 stride-1 convolution, taps at offsets -2 .. +1, over the 12-channel space-to-depth
    image with the filter padded to 8x8 by a zero first row and column: what vt_stem7_s2d / vt_stem7_pack_filter lay out"""
    H, W = hw
    x = filler.tensor(f"s2d{hw}", (2, 3, H, W)).double()
    w = filler.tensor("s2dw", (8, 3, 7, 7)).double()
    want = F.conv2d(x, w, None, 2, 3)
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (0, 2 * Ws - W, 0, 2 * Hs - H))  # odd: one zero row / column at the far edge
    xs = xp.reshape(2, 3, Hs, 2, Ws, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 12, Hs, Ws)  # channel (py, px, c)
    w8 = F.pad(w, (1, 0, 1, 0))  # [C, 3, 8, 8], zero first row and column
    w4 = w8.reshape(8, 3, 4, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(8, 12, 4, 4)
    got = F.conv2d(F.pad(xs, (2, 1, 2, 1)), w4)  # offsets -2 .. +1
    assert got.shape == want.shape == (2, 8, Hs, Ws)
    assert ((got - want).norm() / want.norm()).item() < 1e-12
