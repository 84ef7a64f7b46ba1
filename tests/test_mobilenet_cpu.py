"""MobileNetExtractor without a GPU: torchvision's keys and parameter counts, the five returned nodes, the eager path against
the float64 restatement of tests/mobilenet_util.py, checkpoints, refusals, and the launch lists compiled on the CPU."""
import pytest
import torch
from torch import nn

import mobilenet_util as MU
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import MobileNetExtractor
from vision_toolbox.components import ConvNormAct
from vision_toolbox.trainer import TrainStep

BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
DWT_OPS = {N.OP_DWT_FWD, N.OP_DWT_BWD, N.OP_DWT_WGRAD_REDUCE}
DWCONV_OPS = {N.OP_DWCONV_FWD, N.OP_DWCONV_DGRAD, N.OP_DWCONV_WGRAD}
# depthwise units and Squeeze-Excitations per model
UNITS = {"mobilenet_v2": (17, 0), "mobilenet_v3_large": (15, 8), "mobilenet_v3_small": (11, 9)}


def test_state_dict_keys_are_torchvisions():
    for name in MU.NAMES:
        ref, sd = MU.make_pair(name)
        own = list(MobileNetExtractor(name).state_dict())
        assert own == ["feat_extractor." + k for k in sd if not k.startswith("fc.")], name
        assert not any("classifier" in k for k in own)
        assert sum(k.endswith("num_batches_tracked") for k in own) == sum(isinstance(m, nn.BatchNorm2d) for m in ref.modules())
    v2 = set(MobileNetExtractor("mobilenet_v2").state_dict())
    # t = 1: conv.0.{0,1} is the depthwise unit, conv.1 the projection, conv.2 its BatchNorm
    for k in (["features.0.0.weight", "features.1.conv.0.0.weight", "features.1.conv.1.weight", "features.2.conv.2.weight",
               "features.17.conv.1.0.weight", "features.18.0.weight"] + [f"features.1.conv.2.{s}" for s in BN] +
              [f"features.2.conv.0.1.{s}" for s in BN] + [f"features.2.conv.3.{s}" for s in BN] + [f"features.18.1.{s}" for s in BN]):
        assert "feat_extractor." + k in v2, k
    assert "feat_extractor.features.1.conv.3.weight" not in v2 and "feat_extractor.features.19.0.weight" not in v2
    large = set(MobileNetExtractor("mobilenet_v3_large").state_dict())
    for k in ("features.1.block.0.0.weight", "features.1.block.1.0.weight", "features.4.block.2.fc1.bias", "features.4.block.2.fc2.weight",
              "features.4.block.3.1.num_batches_tracked", "features.2.block.2.1.running_var", "features.16.0.weight"):
        assert "feat_extractor." + k in large, k
    assert "feat_extractor.features.1.block.2.0.weight" not in large and "feat_extractor.features.2.block.2.fc1.bias" not in large
    small = set(MobileNetExtractor("mobilenet_v3_small").state_dict())
    for k in ("features.1.block.0.0.weight", "features.1.block.1.fc1.weight", "features.1.block.2.0.weight", "features.12.1.bias"):
        assert "feat_extractor." + k in small, k


@pytest.mark.parametrize("name", MU.NAMES)
def test_parameter_counts_and_surface(name):
    m = MobileNetExtractor(name)
    assert sum(p.numel() for p in m.parameters()) == MU.PARAMS[name]
    stages, last = MU.NODES[name]
    block = "conv" if name == "mobilenet_v2" else "block"
    assert m.node_names == tuple(f"features.{i}.{block}.0" for i in stages) + (f"features.{last}",)
    assert m.out_channels_list == MU.CHANNELS[name] and m.stride == 32 and m.get_last_out_channels() == MU.CHANNELS[name][-1]
    m.eval()
    with torch.no_grad():
        for size in (64, 224):
            maps = m.get_feature_maps(torch.rand(1, 3, size, size))
            assert [tuple(t.shape) for t in maps] == [(1, c, size // s, size // s) for c, s in zip(MU.CHANNELS[name], MU.STRIDES[name])]
        assert torch.equal(m(torch.ones(1, 3, 64, 64)), m.get_feature_maps(torch.ones(1, 3, 64, 64))[-1])
    bns = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    want = (1e-5, 0.1) if name == "mobilenet_v2" else (1e-3, 0.01)
    assert all((b.eps, b.momentum) == want and bool((b.weight == 1).all()) and bool((b.bias == 0).all()) for b in bns)
    # torchvision's initialisation: kaiming_normal_(fan_out) -> std sqrt(2 / (k k out_channels)); biases zero
    w = m.feat_extractor.features[-1][0].weight
    assert abs(w.std().item() / (2.0 / w.shape[0]) ** 0.5 - 1) < 0.03
    assert all(bool((c.bias == 0).all()) for c in m.modules() if isinstance(c, nn.Conv2d) and c.bias is not None)


def test_v3_small_returns_two_maps_at_stride_4():
    m = MobileNetExtractor("mobilenet_v3_small")
    first = m.feat_extractor.features[1].block[0]
    assert first[0].groups == 16 and first[0].stride == (2, 2)  # the depthwise unit IS the first child: no expansion


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", MU.NAMES)
def test_eager_path_matches_the_restatement(name, training):
    """both in float64: 1e-5 pins the wiring (an f32 run differs from float64 by more than that after ~50 BatchNorm layers)"""
    ref, sd = MU.make_pair(name)
    m = MobileNetExtractor(name)
    m.load_torchvision_ckpt(MU.torchvision_layout(sd))
    m.double().train(training)
    ref.train(training)
    x = filler.images(4, 64).double()
    with torch.no_grad():
        got, want = m.get_feature_maps(x), ref.maps(x)
    assert len(got) == 5
    for g, w in zip(got, want):
        assert g.shape == w.shape and ((g - w).norm() / w.norm()).item() < 1e-5
    if training:  # the running statistics moved the same way
        k = [k for k in ref.state_dict() if k.endswith("running_var")][-1]
        a, b_ = m.state_dict()["feat_extractor." + k], ref.state_dict()[k]
        assert ((a - b_).norm() / b_.norm()).item() < 1e-5


def test_load_torchvision_ckpt(tmp_path):
    _, sd = MU.make_pair("mobilenet_v3_large")
    tv = MU.torchvision_layout(sd)
    assert "classifier.1.weight" in tv
    m = MobileNetExtractor("mobilenet_v3_large")
    m.load_torchvision_ckpt(tv)  # classifier.* is dropped, the prefix added
    for k, v in m.state_dict().items():
        assert torch.equal(v, tv[k[len("feat_extractor."):]]), k
    path = tmp_path / "mobilenet_v3_large.pth"
    torch.save(tv, path)
    m2 = MobileNetExtractor("mobilenet_v3_large")
    m2.load_torchvision_ckpt(path)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(KeyError, match="unexpected"):
        m.load_torchvision_ckpt(dict(tv, **{"features.17.0.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing"):
        m.load_torchvision_ckpt({k: v for k, v in tv.items() if k != "features.4.block.2.fc1.bias"})


def test_refusals():
    with pytest.raises(NotImplementedError, match="pretrained"):
        MobileNetExtractor("mobilenet_v2", pretrained=True)
    with pytest.raises(ValueError, match="mobilenet_v4"):
        MobileNetExtractor("mobilenet_v4")
    m = MobileNetExtractor("mobilenet_v2")
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        r.program(torch.zeros(2, 3, 64, 64, requires_grad=True), N.VT_F32, True, True)


@pytest.mark.parametrize("name", ["mobilenet_v2", "mobilenet_v3_small"])
def test_sharded_exchange_is_refused_by_name(name, monkeypatch):
    """(a one-rank gloo group on the loopback interface, as tests/test_deit_cpu.py does)"""
    import socket

    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match=f"sharded.*{name}.*depthwise filters"):
            TrainStep(MobileNetExtractor(name), 10, 2, 64, torch.bfloat16, device="cpu", plan_only=True, exchange="sharded")
    finally:
        dist.destroy_process_group()


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
def _program(make, dtype, training=True, need_grad=True, size=64):
    m = make()
    m.train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(2, 3, size, size), dtype, True, need_grad)


def _kinds(prog):
    return [op.kind & 0xFFFF for op in list(prog.fwd_ops)[: prog.n_fwd]], [op.kind & 0xFFFF for op in list(prog.bwd_ops)[: prog.n_bwd]]


def test_new_op_codes_are_appended():
    assert [N.OP_DWT_FWD, N.OP_DWT_BWD, N.OP_DWT_WGRAD_REDUCE] == [98, 99, 100] and N.OP_SE_MLP_BWD == 97
    assert [N.OP_NAMES[k] for k in (98, 99, 100)] == ["dwt_fwd", "dwt_bwd", "dwt_wgrad_reduce"]
    for sym in ("vt_dwt_fwd", "vt_dwt_bwd", "vt_dwt_wgrad_reduce", "vt_dwt_shares_bytes", "vt_dwt_tile"):
        assert sym in N.SYMBOLS


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", MU.NAMES)
def test_launch_lists(name, dtype):
    """one dwt_fwd per depthwise unit, one dwt_bwd + one dwt_wgrad_reduce per depthwise unit, no dwconv_* op; the hardsigmoid
    gate and the SE MLP once per Squeeze-Excitation; every other op is one an existing family runs"""
    dw, se = UNITS[name]
    prog = _program(lambda: MobileNetExtractor(name), dtype)
    fwd, bwd = _kinds(prog)
    assert fwd.count(N.OP_DWT_FWD) == dw and bwd.count(N.OP_DWT_BWD) == dw and bwd.count(N.OP_DWT_WGRAD_REDUCE) == dw
    assert not (set(fwd) | set(bwd)) & DWCONV_OPS
    assert fwd.count(N.OP_ESE_FWD) == se and bwd.count(N.OP_ESE_BWD) == se
    assert fwd.count(N.OP_SE_MLP_FWD) == se and bwd.count(N.OP_SE_MLP_BWD) == se and fwd.count(N.OP_AVGPOOL_FWD) == se
    # each reducer directly follows the launch that fills its scratch, on the main stream
    ops = list(prog.bwd_ops)[: prog.n_bwd]
    for i, op in enumerate(ops):
        if op.kind & 0xFFFF == N.OP_DWT_BWD:
            assert ops[i + 1].kind == N.OP_DWT_WGRAD_REDUCE and not op.kind & N.OP_SIDE_STREAM
    known = set()
    for make in (backbones.cspdarknet53, backbones.vovnet39_ese, lambda: backbones.RegNetExtractor("regnet_y_400mf")):
        f, b = _kinds(_program(make, dtype))
        known |= set(f) | set(b)
    known |= {N.OP_PW_STATS, N.OP_PW_APPLY, N.OP_PW_REDUCE, N.OP_PW_BWD, N.OP_PW_APPLY_FIN, N.OP_PW_BWD_FIN, N.OP_BN_FINALIZE,
              N.OP_BN_ACT_APPLY, N.OP_BN_BWD_REDUCE, N.OP_BN_BWD_FINALIZE, N.OP_BN_BWD_APPLY}
    assert (set(fwd) | set(bwd)) - known == DWT_OPS
    # per-block op sequence of the forward pass: a depthwise unit is dwt_fwd -> bn_finalize -> bn_act_apply with its code
    code = {"mobilenet_v2": {5}, "mobilenet_v3_large": {1, 6}, "mobilenet_v3_small": {1, 6}}[name]
    fops = list(prog.fwd_ops)[: prog.n_fwd]
    seen = set()
    for i, op in enumerate(fops):
        if op.kind & 0xFFFF == N.OP_DWT_FWD:
            assert [o.kind & 0xFFFF for o in fops[i + 1: i + 3]] == [N.OP_BN_FINALIZE, N.OP_BN_ACT_APPLY]
            seen.add(fops[i + 2].i[4])
    assert seen == code
    # eval without gradients, and an odd image size, compile too
    fwd_e, bwd_e = _kinds(_program(lambda: MobileNetExtractor(name), dtype, training=False, need_grad=False))
    assert fwd_e.count(N.OP_DWT_FWD) == dw and not bwd_e and N.OP_BN_FINALIZE not in fwd_e
    _program(lambda: MobileNetExtractor(name), dtype, size=61)


@pytest.mark.parametrize("kw", [{}, {"optimizer": "AdamW"}, {"optimizer": "Adam"}, {"deterministic": True}, {"mix": True},
                                {"dtype": torch.float32}], ids=str)
@pytest.mark.parametrize("name", MU.NAMES)
def test_train_step_plans(name, kw):
    kw = dict(kw)
    dtype = kw.pop("dtype", torch.bfloat16)
    dw, se = UNITS[name]
    ts = TrainStep(MobileNetExtractor(name), 10, 2, 64, dtype, device="cpu", plan_only=True, **kw)
    fwd, bwd = _kinds(ts.prog)
    assert fwd.count(N.OP_DWT_FWD) == dw and bwd.count(N.OP_DWT_BWD) == dw and bwd.count(N.OP_DWT_WGRAD_REDUCE) == dw
    assert bwd.count(N.OP_SE_MLP_BWD) == se and bwd.count(N.OP_ESE_BWD) == se
    convs = sum(isinstance(m, nn.Conv2d) for m in ts.model[0].modules()) - 2 * se
    assert ts.n_units == convs + 1  # every convolution outside the SE MLPs is a unit; and the head


def test_conv_norm_act_keeps_the_untiled_depthwise_kernels():
    mod = ConvNormAct(32, 32, 3, groups=32)
    mod.train(True)
    r = mod._vt_runner()
    r.store.ensure(torch.device("cpu"))
    fwd, bwd = _kinds(r.program(torch.zeros(2, 32, 8, 8, requires_grad=True), N.VT_BF16, True, True))
    kinds = set(fwd) | set(bwd)
    assert DWCONV_OPS <= kinds and not kinds & DWT_OPS


def test_builder_refuses_what_the_tiled_unit_does_not_take():
    for conv, pat in ((nn.Conv2d(32, 32, 7, 1, 3, groups=32, bias=False), "kernel_size=7"),
                      (nn.Conv2d(32, 32, 3, 3, 1, groups=32, bias=False), "stride=3"),
                      (nn.Conv2d(32, 32, 3, 1, 2, dilation=2, groups=32, bias=False), "dilation=2"),
                      (nn.Conv2d(32, 32, 3, 1, 1, groups=4, bias=False), "groups=C"),
                      (nn.Conv2d(32, 32, 3, 1, 1, groups=32, bias=True), "bias=False"),
                      (nn.Conv2d(12, 12, 3, 1, 1, groups=12, bias=False), "12 channels")):
        mod = nn.Sequential(conv, nn.BatchNorm2d(conv.out_channels))
        b = E.Builder(E.ParamStore(mod), N.VT_BF16, True, True)
        x = b.act(2, 8, 8, conv.in_channels, "x")
        with pytest.raises(NotImplementedError, match=pat):
            b.depthwise_unit(x, mod[0], mod[1], 1)
    mod = nn.Sequential(nn.Conv2d(8, 8, 5, 1, 2, groups=8, bias=False), nn.BatchNorm2d(8))
    b = E.Builder(E.ParamStore(mod), N.VT_BF16, True, True)
    with pytest.raises(NotImplementedError, match="Wi=1000"):
        b.depthwise_unit(b.act(1, 4, 1000, 8, "x"), mod[0], mod[1], 1)
