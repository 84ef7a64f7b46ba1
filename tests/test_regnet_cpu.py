"""RegNetExtractor without a GPU: module surface (state_dict keys, the width quantisation, parameter counts, squeeze widths),
the eager path against the plain-torch restatement of torchvision's RegNet (tests/regnet_util.py -- a restatement, not a
reference fixture: the reference class only wraps torchvision, which is not installed), the checkpoint loader, refusals, and
the launch lists as the builder compiles them on the CPU."""
import importlib.util
from pathlib import Path

import pytest
import torch

import regnet_util
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.backbones import RegNetBlock, RegNetExtractor, regnet_block_params
from vision_toolbox.trainer import TrainStep

ROOT = Path(__file__).resolve().parents[1]
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")

# name: (widths, depths, group widths, trunk parameters without fc) -- torchvision's published totals minus the 1000-class fc
TABLE = {
    "regnet_x_400mf": ((32, 64, 160, 400), (1, 2, 7, 12), (16,) * 4, 5_094_976),
    "regnet_x_800mf": ((64, 128, 288, 672), (1, 3, 7, 5), (16,) * 4, 6_586_656),
    "regnet_y_400mf": ((48, 104, 208, 440), (1, 3, 6, 6), (8,) * 4, 3_903_144),
    "regnet_y_800mf": ((64, 144, 320, 784), (1, 3, 8, 2), (16,) * 4, 5_647_512),
    "regnet_y_8gf": ((224, 448, 896, 2016), (2, 4, 10, 1), (56,) * 4, 37_364_472),
    "regnet_x_8gf": ((80, 240, 720, 1920), (2, 5, 15, 1), (80, 120, 120, 120), 37_651_648),
}
NAMES = ["regnet_y_400mf", "regnet_y_800mf", "regnet_y_1_6gf", "regnet_y_3_2gf", "regnet_y_8gf", "regnet_y_16gf", "regnet_y_32gf",
         "regnet_x_400mf", "regnet_x_800mf", "regnet_x_1_6gf", "regnet_x_3_2gf", "regnet_x_8gf", "regnet_x_16gf", "regnet_x_32gf"]


def _keys(widths, depths, se):
    """torchvision's state_dict keys without fc.*, under the extractor's prefix, in registration order"""
    keys = ["stem.0.weight"] + [f"stem.1.{s}" for s in BN]
    cin = 32
    for i, (w, d) in enumerate(zip(widths, depths), 1):
        for j in range(d):
            p = f"trunk_output.block{i}.block{i}-{j}."
            units = (["proj"] if j == 0 else []) + ["f.a", "f.b"]  # every stage has stride 2: its first block projects
            for u in units:
                keys.append(f"{p}{u}.0.weight")
                keys += [f"{p}{u}.1.{s}" for s in BN]
            if se:
                keys += [f"{p}f.se.fc1.weight", f"{p}f.se.fc1.bias", f"{p}f.se.fc2.weight", f"{p}f.se.fc2.bias"]
            keys.append(f"{p}f.c.0.weight")
            keys += [f"{p}f.c.1.{s}" for s in BN]
        cin = w
    return ["feat_extractor." + k for k in keys]


def test_state_dict_keys_are_torchvisions():
    for name in ("regnet_x_400mf", "regnet_y_400mf"):
        widths, depths, _, _ = TABLE[name]
        got = list(RegNetExtractor(name).state_dict())
        assert got == _keys(widths, depths, "_y_" in name)
        ref_keys = [k for k in regnet_util.RefRegNet(name).state_dict() if not k.startswith("fc.")]
        assert ["feat_extractor." + k for k in ref_keys] == got
        assert not any("fc." in k or "avgpool" in k for k in got)
    ky = list(RegNetExtractor("regnet_y_400mf").state_dict())
    assert "feat_extractor.trunk_output.block4.block4-5.f.se.fc2.bias" in ky
    assert "feat_extractor.trunk_output.block2.block2-1.proj.0.weight" not in ky


@pytest.mark.parametrize("name", list(TABLE))
def test_quantisation_table_and_parameter_counts(name):
    widths, depths, gws, count = TABLE[name]
    m = RegNetExtractor(name)
    assert (m.widths, m.depths, m.group_widths) == (widths, depths, gws)
    assert m.out_channels_list == (32, *widths) and m.stride == 32 and m.get_last_out_channels() == widths[-1]
    assert sum(p.numel() for p in m.parameters()) == count
    ref = regnet_util.RefRegNet(name)  # ... and the restatement's own rule agrees
    assert (tuple(ref.widths), tuple(ref.depths), tuple(ref.group_widths)) == (widths, depths, gws)


def test_every_variant_of_the_table_quantises_like_the_restatement():
    from vision_toolbox.backbones.regnet import _VARIANTS

    assert list(_VARIANTS) == NAMES and "regnet_y_128gf" not in _VARIANTS
    for name, (*init, se) in _VARIANTS.items():
        w, d, g = regnet_block_params(*init)
        assert (w, d, g) == tuple(regnet_util.block_params(*init)), name
        assert len(w) == 4 and sum(d) == init[0] and all(wi % gi == 0 for wi, gi in zip(w, g))
        assert (se == 0.25) == ("_y_" in name)


def test_surface():
    m = RegNetExtractor("regnet_y_400mf")
    fe = m.feat_extractor
    assert [n for n, _ in fe.named_children()] == ["stem", "trunk_output"]
    assert [n for n, _ in fe.trunk_output.named_children()] == ["block1", "block2", "block3", "block4"]
    assert [n for n, _ in fe.trunk_output.block2.named_children()] == ["block2-0", "block2-1", "block2-2"]
    blk = fe.trunk_output.block2[0]
    assert isinstance(blk, RegNetBlock) and [n for n, _ in blk.f.named_children()] == ["a", "b", "se", "c"]
    assert blk.proj[0].stride == (2, 2) and blk.f.a[0].stride == (1, 1) and blk.f.b[0].stride == (2, 2)
    assert blk.f.b[0].groups == 104 // 8 and blk.f.b[0].kernel_size == (3, 3) and fe.trunk_output.block2[1].proj is None
    assert fe.stem[0].out_channels == 32 and fe.stem[0].stride == (2, 2) and fe.stem[0].bias is None
    # squeeze widths round(0.25 * width_in): the first block of a stage sees 32 / 48 / 104 / 208, the later ones their own width
    assert [fe.trunk_output[i][0].f.se.fc1.out_channels for i in range(4)] == [8, 12, 26, 52]
    assert [b.f.se.fc1.out_channels for b in list(fe.trunk_output.block4)[1:]] == [110] * 5
    assert not hasattr(RegNetExtractor("regnet_x_400mf").feat_extractor.trunk_output.block1[0].f, "se")
    m.eval()
    with torch.no_grad():
        maps = m.get_feature_maps(torch.rand(1, 3, 64, 64))
        assert [tuple(t.shape) for t in maps] == [(1, 32, 32, 32), (1, 48, 16, 16), (1, 104, 8, 8), (1, 208, 4, 4), (1, 440, 2, 2)]
        assert torch.equal(m(torch.ones(1, 3, 64, 64)), m.get_feature_maps(torch.ones(1, 3, 64, 64))[-1])
    # torchvision's initialisation: normal(0, sqrt(2 / (k k out_channels))), BatchNorm 1 / 0, eps 1e-5, momentum 0.1
    bn = fe.stem[1]
    assert (bn.weight == 1).all() and (bn.bias == 0).all() and bn.eps == 1e-5 and bn.momentum == 0.1
    big = fe.trunk_output.block4[0].f.b[0].weight
    assert abs(big.std().item() / (2.0 / (440 * 9)) ** 0.5 - 1) < 0.03
    assert fe.trunk_output.block4[1].f.se.fc1.bias.abs().max() > 0  # torch's default, not zeros


def test_refusals():
    with pytest.raises(NotImplementedError, match="pretrained"):
        RegNetExtractor("regnet_x_400mf", pretrained=True)
    with pytest.raises(ValueError, match="regnet_x_401mf"):
        RegNetExtractor("regnet_x_401mf")
    with pytest.raises(ValueError, match="divisible"):
        RegNetExtractor._from_stages([48, 100], [1, 1], 16)


@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (2, 3, 65, 61)], ids=str)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", ["regnet_x_400mf", "regnet_y_400mf"])
def test_eager_path_matches_the_restatement(name, training, shape):
    ref, sd = regnet_util.make_pair(name)
    m = RegNetExtractor(name)
    m.load_torchvision_ckpt(sd)
    m.train(training)
    ref.train(training)
    x = filler.images(shape[0], max(shape[2:]))[:, :, : shape[2], : shape[3]].contiguous()
    got = m.get_feature_maps(x)
    with torch.no_grad():
        want = ref.maps(x.double())
    assert len(got) == 5
    # f32 against float64 at the bounds of tests/test_resnet_cpu.py: 2e-4 with running statistics, 1e-3 in train mode
    # (batch statistics over few samples per channel in the last stage amplify f32 rounding)
    bound = 1e-3 if training else 2e-4
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert ((g.double() - w).norm() / w.norm()).item() < bound
    if training:  # the running statistics moved the same way
        got_sd, ref_sd = m.state_dict(), ref.state_dict()
        assert torch.allclose(got_sd["feat_extractor.stem.1.running_mean"].double(), ref_sd["stem.1.running_mean"], rtol=1e-4, atol=1e-5)
        k = "trunk_output.block4.block4-1.f.b.1.running_var"
        last, want_last = got_sd["feat_extractor." + k].double(), ref_sd[k]
        assert ((last - want_last).norm() / want_last.norm()).item() < bound


def test_private_constructor_matches_the_restatement():
    stages = ([96, 192], [1, 2], 96, 0.25)
    ref, sd = regnet_util.make_pair(stages=stages, prefix="regnet.wide.")
    m = RegNetExtractor._from_stages(*stages)
    m.load_torchvision_ckpt(sd)
    assert m.out_channels_list == (32, 96, 192) and m.stride == 8 and m.group_widths == (96, 96)
    m.eval(), ref.eval()
    x = filler.images(2, 32)
    with torch.no_grad():
        for g, w in zip(m.get_feature_maps(x), ref.maps(x.double())):
            assert ((g.double() - w).norm() / w.norm()).item() < 2e-4


def test_load_torchvision_ckpt(tmp_path):
    ref, sd = regnet_util.make_pair("regnet_y_400mf")
    assert "fc.weight" in sd
    m = RegNetExtractor("regnet_y_400mf")
    m.load_torchvision_ckpt(sd)  # fc.* is dropped, the prefix added
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k[len("feat_extractor."):]]), k
    path = tmp_path / "regnet_y_400mf.pth"
    torch.save(sd, path)
    m2 = RegNetExtractor("regnet_y_400mf")
    m2.load_torchvision_ckpt(path)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(KeyError, match="unexpected"):
        m.load_torchvision_ckpt(dict(sd, **{"trunk_output.block9.block9-0.f.a.0.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing"):
        m.load_torchvision_ckpt({k: v for k, v in sd.items() if k != "trunk_output.block3.block3-1.f.se.fc1.bias"})


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
GCONV_OPS = {N.OP_GCONV3_FWD, N.OP_GCONV3_DGRAD, N.OP_GCONV3_WGRAD}
SE_OPS = {N.OP_SE_MLP_FWD, N.OP_SE_MLP_BWD}


def _program(make, dtype, training=True, need_grad=True, size=64):
    m = make()
    m.train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(2, 3, size, size), dtype, True, need_grad)


def _kinds(prog):
    return [op.kind & 0xFFFF for op in list(prog.fwd_ops)[: prog.n_fwd]], [op.kind & 0xFFFF for op in list(prog.bwd_ops)[: prog.n_bwd]]


def test_new_op_codes_are_appended():
    assert [N.OP_GCONV3_FWD, N.OP_GCONV3_DGRAD, N.OP_GCONV3_WGRAD, N.OP_SE_MLP_FWD, N.OP_SE_MLP_BWD] == list(range(93, 98))
    assert N.OP_STEM7_UNPACK_WGRAD == 92 and N.OP_NAMES[N.OP_GCONV3_WGRAD] == "gconv3_wgrad" and N.OP_NAMES[N.OP_SE_MLP_BWD] == "se_mlp_bwd"
    assert min(GCONV_OPS | SE_OPS) >= 93
    for sym in ("vt_gconv3_fwd", "vt_gconv3_dgrad", "vt_gconv3_wgrad", "vt_gconv3_wgrad_scratch_bytes", "vt_se_mlp_fwd", "vt_se_mlp_bwd"):
        assert sym in N.SYMBOLS


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,blocks", [("regnet_x_400mf", 22), ("regnet_y_400mf", 16)])
def test_launch_lists(name, blocks, dtype):
    """one grouped launch per block and pass, none of the per-group composition; the SE ops only in Y; every other site runs
    what it runs in a Darknet, a VoVNet, a ResNet or (the gate, the pool) a PatchConvNet"""
    fwd, bwd = _kinds(_program(lambda: RegNetExtractor(name), dtype))
    se = blocks if "_y_" in name else 0
    assert fwd.count(N.OP_GCONV3_FWD) == blocks and bwd.count(N.OP_GCONV3_DGRAD) == blocks and bwd.count(N.OP_GCONV3_WGRAD) == blocks
    assert fwd.count(N.OP_SE_MLP_FWD) == se and bwd.count(N.OP_SE_MLP_BWD) == se
    assert fwd.count(N.OP_SE_GATE_FWD) == se and fwd.count(N.OP_AVGPOOL_FWD) == se
    assert fwd.count(N.OP_BN_ADD_ACT_FIN_APPLY) == blocks and bwd.count(N.OP_BN_ADD_ACT_BWD_REDUCE) == blocks
    # convolutions on the general kernel: the stem, f.a and f.c of every block, and four projections -- no per-group unit
    # (bf16: some of the 1x1 units take the pointwise passes instead)
    units = 1 + 2 * blocks + 4
    assert fwd.count(N.OP_CONV_IGEMM) == units if dtype == N.VT_F32 else fwd.count(N.OP_CONV_IGEMM) <= units
    assert bwd.count(N.OP_CONV_WGRAD) == units if dtype == N.VT_F32 else bwd.count(N.OP_CONV_WGRAD) <= units
    known = set()
    for make in (backbones.darknet53, backbones.cspdarknet53, backbones.vovnet39, lambda: backbones.ResNetExtractor("resnet50")):
        f, b = _kinds(_program(make, dtype))
        known |= set(f) | set(b)
    known |= {N.OP_SE_GATE_FWD, N.OP_SE_GATE_BWD, N.OP_AVGPOOL_FWD, N.OP_AVGPOOL_BWD}
    # (bf16 with the tests' VT_PW_MIN_MB=0: the 1x1 units f.a may take the pointwise passes, as in every family)
    known |= {N.OP_PW_STATS, N.OP_PW_APPLY, N.OP_PW_REDUCE, N.OP_PW_BWD, N.OP_PW_APPLY_FIN, N.OP_PW_BWD_FIN}
    new = (set(fwd) | set(bwd)) - known
    assert new == (GCONV_OPS | SE_OPS if se else GCONV_OPS) and min(new) >= 93
    # the filter gradients run on the side stream
    prog = _program(lambda: RegNetExtractor(name), dtype)
    for op in list(prog.bwd_ops)[: prog.n_bwd]:
        if op.kind & 0xFFFF == N.OP_GCONV3_WGRAD:
            assert op.kind & N.OP_SIDE_STREAM
    # eval without gradients, and an odd image size, compile too
    fwd_e, bwd_e = _kinds(_program(lambda: RegNetExtractor(name), dtype, training=False, need_grad=False))
    assert fwd_e.count(N.OP_GCONV3_FWD) == blocks and not bwd_e
    _program(lambda: RegNetExtractor(name), dtype, size=61)


def test_wide_groups_keep_the_per_group_path():
    """regnet_x_8gf: 80 channels in one group (a plain unit), then 120 per group (per-group units): no new convolution op"""
    fwd, bwd = _kinds(_program(lambda: RegNetExtractor("regnet_x_8gf"), N.VT_BF16))
    assert not (set(fwd) | set(bwd)) & (GCONV_OPS | SE_OPS)
    groups = 2 * 1 + 5 * 2 + 15 * 6 + 1 * 16
    assert fwd.count(N.OP_CONV_IGEMM) == 1 + 2 * 23 + 4 + groups


@pytest.mark.parametrize("kw", [{}, {"optimizer": "AdamW"}, {"deterministic": True}, {"mix": True}, {"freeze_bn": True},
                                {"dtype": torch.float32}], ids=str)
@pytest.mark.parametrize("name,blocks", [("regnet_x_400mf", 22), ("regnet_y_400mf", 16)])
def test_train_step_plans(name, blocks, kw):
    kw = dict(kw)
    dtype = kw.pop("dtype", torch.bfloat16)
    ts = TrainStep(RegNetExtractor(name), 10, 2, 64, dtype, device="cpu", plan_only=True, **kw)
    fwd, bwd = _kinds(ts.prog)
    assert fwd.count(N.OP_GCONV3_FWD) == blocks and bwd.count(N.OP_GCONV3_WGRAD) == blocks and bwd.count(N.OP_GCONV3_DGRAD) == blocks
    assert bwd.count(N.OP_SE_MLP_BWD) == (blocks if "_y_" in name else 0)
    assert ts.n_units == 1 + 3 * blocks + 4 + 1  # the stem, three convolutions per block, four projections; and the head


def test_image_gradient_is_refused_by_name():
    m = RegNetExtractor("regnet_x_400mf")
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        r.program(torch.zeros(2, 3, 64, 64, requires_grad=True), N.VT_F32, True, True)


def test_builder_refuses_what_the_grouped_unit_does_not_take():
    from torch import nn

    from vision_toolbox import engine as E

    for conv, pat in ((nn.Conv2d(64, 64, 3, 1, 1, groups=16, bias=False), "channels per group"),
                      (nn.Conv2d(144, 144, 3, 1, 1, groups=2, bias=False), "channels per group"),
                      (nn.Conv2d(64, 64, 5, 1, 2, groups=4, bias=False), "one-launch grouped unit"),
                      (nn.Conv2d(64, 64, 3, 1, 1, groups=4, bias=True), "one-launch grouped unit")):
        mod = nn.Sequential(conv, nn.BatchNorm2d(conv.out_channels))
        b = E.Builder(E.ParamStore(mod), N.VT_BF16, True, True)
        x = b.act(2, 8, 8, conv.in_channels, "x")
        with pytest.raises(NotImplementedError, match=pat):
            b.grouped3x3_unit(x, mod[0], mod[1])


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
