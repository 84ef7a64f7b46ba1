"""EfficientNetExtractor without a GPU: torchvision's keys and parameter counts, the five returned nodes, the stochastic-depth
rates, the eager path against the float64 restatement of tests/efficientnet_util.py with a set keep table, checkpoints,
refusals, and the launch lists compiled on the CPU (one keep pass per residual block in training mode and none in eval mode,
one fused pool pass per Squeeze-Excitation, the keep table's place in the program cache key, the trainer's plans and seed)."""
import copy

import pytest
import torch
from torch import nn

import efficientnet_util as EU
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import EfficientNetExtractor
from vision_toolbox.trainer import TrainStep

BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
KEEP_OPS = {N.OP_BN_KEEP_APPLY, N.OP_BN_KEEP_FIN_APPLY, N.OP_BN_KEEP_BWD_REDUCE, N.OP_BN_KEEP_BWD_APPLY, N.OP_BN_KEEP_BWD_FIN_APPLY}
POOL_OPS = {N.OP_BN_ACT_AVGPOOL_APPLY, N.OP_BN_ACT_AVGPOOL_FIN_APPLY}
SMALL = ("efficientnet_b0", "efficientnet_v2_s")
# (blocks, residual blocks, Squeeze-Excitations) of the two models the launch-list tests compile
UNITS = {"efficientnet_b0": (16, 9, 16), "efficientnet_v2_s": (40, 35, 30)}


def test_state_dict_keys_are_torchvisions():
    for name in SMALL + ("efficientnet_b3", "efficientnet_v2_m"):
        ref, sd = EU.make_pair(name)
        own = list(EfficientNetExtractor(name).state_dict())
        assert own == ["feat_extractor." + k for k in sd if not k.startswith("fc.")], name
        assert not any("classifier" in k or "avgpool" in k for k in own)
        assert sum(k.endswith("num_batches_tracked") for k in own) == sum(isinstance(m, nn.BatchNorm2d) for m in ref.modules())
    b0 = set(EfficientNetExtractor("efficientnet_b0").state_dict())
    # features.1.0 has expand ratio 1: block.0 is the depthwise unit, block.1 the SE, block.2 the projection
    for k in (["features.0.0.weight", "features.1.0.block.0.0.weight", "features.1.0.block.1.fc1.weight", "features.1.0.block.1.fc2.bias",
               "features.1.0.block.2.0.weight", "features.2.0.block.0.0.weight", "features.2.1.block.2.fc1.bias",
               "features.7.0.block.3.0.weight", "features.8.0.weight"] + [f"features.0.1.{s}" for s in BN] +
              [f"features.2.0.block.3.1.{s}" for s in BN] + [f"features.8.1.{s}" for s in BN]):
        assert "feat_extractor." + k in b0, k
    assert "feat_extractor.features.1.0.block.3.0.weight" not in b0 and "feat_extractor.features.9.0.weight" not in b0
    v2 = set(EfficientNetExtractor("efficientnet_v2_s").state_dict())
    # FusedMBConv: expand ratio 1 is block.0 alone; with expansion block.0 (3x3) and block.1 (1x1); no SE before stage 4
    for k in ("features.1.0.block.0.0.weight", "features.2.0.block.1.0.weight", "features.4.0.block.2.fc1.weight", "features.7.1.bias"):
        assert "feat_extractor." + k in v2, k
    assert "feat_extractor.features.1.0.block.1.0.weight" not in v2 and "feat_extractor.features.2.0.block.2.0.weight" not in v2


@pytest.mark.parametrize("name", EU.NAMES)
def test_parameter_counts_and_surface(name):
    m = EfficientNetExtractor(name)
    assert sum(p.numel() for p in m.parameters()) == EU.PARAMS[name]
    last = len(m.feat_extractor.features) - 1
    assert m.node_names == tuple(f"features.{i}.0.block.0" for i in (2, 3, 4, 6)) + (f"features.{last}",)
    assert m.out_channels_list == EU.CHANNELS[name] and m.stride == 32 and m.get_last_out_channels() == EU.CHANNELS[name][-1]
    bns = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    want = (1e-3, 0.1) if "_v2_" in name else ((1e-3, 0.01) if name[-2:] in ("b5", "b6", "b7") else (1e-5, 0.1))
    assert all((b.eps, b.momentum) == want and bool((b.weight == 1).all()) and bool((b.bias == 0).all()) for b in bns)
    # torchvision's initialisation: kaiming_normal_(fan_out) -> std sqrt(2 / (k k out_channels)); biases zero
    w = m.feat_extractor.features[-1][0].weight
    assert abs(w.std().item() / (2.0 / w.shape[0]) ** 0.5 - 1) < 0.03
    assert all(bool((c.bias == 0).all()) for c in m.modules() if isinstance(c, nn.Conv2d) and c.bias is not None)
    # the stochastic-depth rate of block i of n is sd_prob * i / n, counted over every block of the net
    rates = m.drop_rates()
    assert rates == pytest.approx([EU.SD_PROB[name] * i / len(rates) for i in range(len(rates))])


@pytest.mark.parametrize("name", SMALL)
def test_shapes_and_strides(name):
    m = EfficientNetExtractor(name).eval()
    with torch.no_grad():
        for size in (64, 96):
            maps = m.get_feature_maps(torch.rand(1, 3, size, size))
            assert [tuple(t.shape) for t in maps] == [(1, c, size // s, size // s) for c, s in zip(EU.CHANNELS[name], EU.strides(name))]
        assert torch.equal(m(torch.ones(1, 3, 64, 64)), m.get_feature_maps(torch.ones(1, 3, 64, 64))[-1])


def test_b0_drop_rates_and_sites():
    m = EfficientNetExtractor("efficientnet_b0")
    assert m.drop_rates() == pytest.approx([0.2 * i / 16 for i in range(16)]) and len(m.drop_rates()) == 16
    assert m.n_keep_sites == 9  # the second and later blocks of stages 2 .. 6
    assert m.train()._vt_keep_rates() == pytest.approx([0.2 * i / 16 for i in (2, 4, 6, 7, 9, 10, 12, 13, 14)])
    assert m.eval()._vt_keep_rates() == ()  # eval mode: no table
    for blk in m.blocks():
        blk.stochastic_depth.p = 0.0
    assert m.train()._vt_keep_rates() == ()  # a zero rate: no table


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", SMALL)
def test_eager_path_matches_the_restatement(name, training):
    """both in float64, the keep table set (train) or ignored (eval): 1e-5 pins the wiring"""
    ref, sd = EU.make_pair(name)
    m = EfficientNetExtractor(name)
    m.load_torchvision_ckpt(EU.torchvision_layout(sd))
    m.double().train(training)
    ref.train(training)
    x = filler.images(4, 64).double()
    keep = EU.keep_table(name, 4)
    assert (keep == 0).any(1).sum() >= 3 and (keep[:, -1] > 0).all() and keep.shape == (m.n_keep_sites, 4)
    m.set_keep_factors(keep)
    with torch.no_grad():
        other = copy.deepcopy(ref).maps(x, None if training else keep)
        got, want = m.get_feature_maps(x), ref.maps(x, keep if training else None)
    assert len(got) == 5
    for g, w in zip(got, want):
        assert g.shape == w.shape and ((g - w).norm() / w.norm()).item() < 1e-5
    assert ((got[-1] - other[-1]).norm() / other[-1].norm()).item() > 1e-3  # the table matters in training mode only
    if training:  # the running statistics moved the same way
        k = [k for k in ref.state_dict() if k.endswith("running_var")][-1]
        a, b_ = m.state_dict()["feat_extractor." + k], ref.state_dict()[k]
        assert ((a - b_).norm() / b_.norm()).item() < 1e-5


def test_eager_path_draws_when_no_table_is_set():
    m = EfficientNetExtractor("efficientnet_b0").train()
    for blk in m.blocks():
        blk.stochastic_depth.p = min(0.9, blk.stochastic_depth.p * 8)  # (so that four images almost surely differ)
    x = filler.images(4, 64)
    with torch.no_grad():
        a, b_ = m(x), m(x)
        m.set_keep_factors(torch.ones(9, 4))
        c, d = m(x), m(x)
    assert not torch.equal(a, b_) and torch.equal(c, d) and torch.isfinite(a).all()
    with pytest.raises(ValueError, match="9 residual"):
        m.set_keep_factors(torch.ones(8, 4))
    m.set_keep_factors(None)


def test_load_torchvision_ckpt(tmp_path):
    _, sd = EU.make_pair("efficientnet_b0")
    tv = EU.torchvision_layout(sd)
    assert "classifier.1.weight" in tv
    m = EfficientNetExtractor("efficientnet_b0")
    m.load_torchvision_ckpt(tv)  # classifier.* is dropped, the prefix added
    for k, v in m.state_dict().items():
        assert torch.equal(v, tv[k[len("feat_extractor."):]]), k
    path = tmp_path / "efficientnet_b0.pth"
    torch.save(tv, path)
    m2 = EfficientNetExtractor("efficientnet_b0")
    m2.load_torchvision_ckpt(path)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(KeyError, match="unexpected"):
        m.load_torchvision_ckpt(dict(tv, **{"features.9.0.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing"):
        m.load_torchvision_ckpt({k: v for k, v in tv.items() if k != "features.2.0.block.2.fc1.bias"})


def test_refusals():
    with pytest.raises(NotImplementedError, match="pretrained"):
        EfficientNetExtractor("efficientnet_b0", pretrained=True)
    with pytest.raises(ValueError, match="efficientnet_b8"):
        EfficientNetExtractor("efficientnet_b8")
    m = EfficientNetExtractor("efficientnet_b0")
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="EfficientNetExtractor.*requires_grad"):
        r.program(torch.zeros(2, 3, 64, 64, requires_grad=True), N.VT_F32, True, True)
    assert "EfficientNetExtractor" in backbones.__dict__


def test_sharded_exchange_is_refused_by_name(monkeypatch):
    """(a one-rank gloo group on the loopback interface, as tests/test_mobilenet_cpu.py does); the per-rank seed too"""
    import socket

    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="sharded.*efficientnet_b0.*depthwise filters"):
            TrainStep(EfficientNetExtractor("efficientnet_b0"), 10, 2, 64, torch.bfloat16, device="cpu", plan_only=True,
                      exchange="sharded")
        ts = TrainStep(EfficientNetExtractor("efficientnet_b0"), 10, 2, 64, torch.bfloat16, device="cpu", plan_only=True, drop_seed=5)
        assert ts.dp and ts.drop_seed == 5 + dist.get_rank()  # data parallel: every rank adds its rank to the seed
    finally:
        dist.destroy_process_group()


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
def _runner(name, training=True):
    m = EfficientNetExtractor(name)
    m.train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return m, r


def _kinds(prog):
    return [op.kind & 0xFFFF for op in list(prog.fwd_ops)[: prog.n_fwd]], [op.kind & 0xFFFF for op in list(prog.bwd_ops)[: prog.n_bwd]]


def test_new_op_codes_are_appended():
    assert [N.OP_BN_KEEP_APPLY, N.OP_BN_KEEP_FIN_APPLY, N.OP_BN_KEEP_BWD_REDUCE, N.OP_BN_KEEP_BWD_APPLY, N.OP_BN_KEEP_BWD_FIN_APPLY,
            N.OP_BN_ACT_AVGPOOL_APPLY, N.OP_BN_ACT_AVGPOOL_FIN_APPLY] == list(range(101, 108)) and N.OP_DWT_WGRAD_REDUCE == 100
    assert N.OP_NAMES[101] == "bn_keep_apply" and N.OP_NAMES[107] == "bn_act_avgpool_fin_apply"
    for sym in ("vt_bn_keep_apply", "vt_bn_keep_finalize_apply", "vt_bn_keep_bwd_reduce", "vt_bn_keep_bwd_apply",
                "vt_bn_keep_bwd_finalize_apply", "vt_bn_act_avgpool_scratch_bytes", "vt_bn_act_avgpool_apply",
                "vt_bn_act_avgpool_finalize_apply", "vt_se_mlp_act_fwd", "vt_se_mlp_act_bwd"):
        assert sym in N.SYMBOLS


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", SMALL)
def test_launch_lists(name, dtype):
    blocks, sites, se = UNITS[name]
    m, r = _runner(name)
    assert (len(m.blocks()), m.n_keep_sites) == (blocks, sites)
    prog = r.program(torch.zeros(2, 3, 64, 64), dtype, True, True)
    fwd, bwd = _kinds(prog)
    # training mode: one keep pass per residual block in forward, one reduce + one apply in backward
    # (and the same backward passes once per Squeeze-Excitation, with no keep row: the pool's gradient joins d(y) inside them)
    assert fwd.count(N.OP_BN_KEEP_FIN_APPLY) == sites and fwd.count(N.OP_BN_KEEP_APPLY) == 0
    assert bwd.count(N.OP_BN_KEEP_BWD_REDUCE) == sites + se and bwd.count(N.OP_BN_KEEP_BWD_FIN_APPLY) == sites + se
    b = prog.builder
    assert len(b.keep_rates) == sites and b.keep_B == 2 and b.keep_buf.nbytes == sites * 2 * 4
    rows = [(op.ptr[13].base, op.ptr[13].offset) for op in list(prog.fwd_ops)[: prog.n_fwd] if op.kind & 0xFFFF == N.OP_BN_KEEP_FIN_APPLY]
    assert rows == [(E.ARENA, b.keep_buf.offset + 8 * i) for i in range(sites)]  # one row per block, in emission order
    red = [op for op in list(prog.bwd_ops)[: prog.n_bwd] if op.kind & 0xFFFF == N.OP_BN_KEEP_BWD_REDUCE]
    back = [(op.ptr[7].base, op.ptr[7].offset) for op in red if op.ptr[7].base >= 0]
    assert back == rows[::-1]  # ... and the backward reads the same rows
    pool = [op for op in red if op.ptr[7].base < 0]  # the depthwise units: no keep row, the gradient of the pooled row as addend
    assert len(pool) == se and all(op.ptr[8].base == E.ARENA and op.i[4] == 3 and op.i[6] > 0 for op in pool)
    assert all(op.ptr[8].base < 0 for op in red if op.ptr[7].base >= 0)
    # one fused pool pass per Squeeze-Excitation, no separate average pool inside a block; the MLP carries SiLU's code
    assert fwd.count(N.OP_BN_ACT_AVGPOOL_FIN_APPLY) == se and N.OP_AVGPOOL_FWD not in fwd and N.OP_AVGPOOL_BWD not in bwd
    assert fwd.count(N.OP_SE_MLP_FWD) == se and fwd.count(N.OP_SE_GATE_FWD) == se and bwd.count(N.OP_SE_MLP_BWD) == se
    for op in list(prog.fwd_ops)[: prog.n_fwd]:
        if op.kind & 0xFFFF == N.OP_SE_MLP_FWD:
            assert op.i[6] == 3
        if op.kind & 0xFFFF == N.OP_BN_KEEP_FIN_APPLY:
            assert op.i[5] in ((0, 3) if "_v2_" in name else (0,))  # (code 3: the FusedMBConv with expand ratio 1)
    if "_v2_" in name:
        assert sum(op.i[5] == 3 for op in list(prog.fwd_ops)[: prog.n_fwd] if op.kind & 0xFFFF == N.OP_BN_KEEP_FIN_APPLY) == 2
    # every other op is one an existing family runs
    known = set()
    for make in (backbones.cspdarknet53, lambda: backbones.MobileNetExtractor("mobilenet_v3_large"),
                 lambda: backbones.RegNetExtractor("regnet_y_400mf")):
        mod = make().train()
        rr = mod._vt_runner()
        rr.store.ensure(torch.device("cpu"))
        f, b_ = _kinds(rr.program(torch.zeros(2, 3, 64, 64), dtype, True, True))
        known |= set(f) | set(b_)
    known |= {N.OP_PW_STATS, N.OP_PW_APPLY, N.OP_PW_REDUCE, N.OP_PW_BWD, N.OP_PW_APPLY_FIN, N.OP_PW_BWD_FIN, N.OP_BN_FINALIZE,
              N.OP_BN_ACT_APPLY, N.OP_BN_BWD_REDUCE, N.OP_BN_BWD_FINALIZE, N.OP_BN_BWD_APPLY, N.OP_SE_GATE_FWD, N.OP_SE_GATE_BWD}
    assert (set(fwd) | set(bwd)) - known == {N.OP_BN_KEEP_FIN_APPLY, N.OP_BN_KEEP_BWD_REDUCE, N.OP_BN_KEEP_BWD_FIN_APPLY,
                                             N.OP_BN_ACT_AVGPOOL_FIN_APPLY}


@pytest.mark.parametrize("name", SMALL)
def test_eval_mode_has_no_table_and_its_own_program(name):
    _, sites, se = UNITS[name]
    m, r = _runner(name)
    x = torch.zeros(2, 3, 64, 64)
    train = r.program(x, N.VT_BF16, True, True)
    m.eval()
    ev = r.program(x, N.VT_BF16, True, False)
    assert ev is not train and ev.builder.keep_buf is None and ev.builder.keep_rates == ()
    fwd, bwd = _kinds(ev)
    assert not (set(fwd) & KEEP_OPS) and not bwd and N.OP_BN_FINALIZE not in fwd
    assert fwd.count(N.OP_BN_ACT_AVGPOOL_APPLY) == se and N.OP_AVGPOOL_FWD not in fwd
    # eval mode WITH gradients (fine-tuning a frozen net): still no table, the ordinary residual passes
    evg = r.program(x, N.VT_BF16, True, True)
    # (the backward passes of that family still run once per SE, for the pool's gradient, with no keep row)
    assert evg.builder.keep_buf is None and not set(_kinds(evg)[0]) & KEEP_OPS
    slot = {N.OP_BN_KEEP_BWD_REDUCE: 7, N.OP_BN_KEEP_BWD_APPLY: 5, N.OP_BN_KEEP_BWD_FIN_APPLY: 11}
    back = [op for op in list(evg.bwd_ops)[: evg.n_bwd] if op.kind & 0xFFFF in slot]
    assert len(back) == 2 * se and all(op.ptr[slot[op.kind & 0xFFFF]].base < 0 for op in back)
    # back in training mode the cached program with the table is found again; a zero rate compiles one without
    m.train()
    assert r.program(x, N.VT_BF16, True, True) is train
    for blk in m.blocks():
        blk.stochastic_depth.p = 0.0
    flat = r.program(x, N.VT_BF16, True, True)
    assert flat is not train and flat.builder.keep_buf is None and not set(_kinds(flat)[0]) & KEEP_OPS


def test_frozen_batchnorm_and_the_separate_launch_forms():
    """a frozen bn.eval() on a residual block's projection: the keep pass with ready coefficients; VT_BN_FIN_APPLY=0: the
    finalize launches of their own in front of the keep and pool passes"""
    m, r = _runner("efficientnet_b0")
    m.feat_extractor.features[2][1].block[3][1].eval()
    fwd, bwd = _kinds(r.program(torch.zeros(2, 3, 64, 64), N.VT_F32, True, True))
    assert fwd.count(N.OP_BN_KEEP_APPLY) == 1 and fwd.count(N.OP_BN_KEEP_FIN_APPLY) == 8 and bwd.count(N.OP_BN_KEEP_BWD_FIN_APPLY) == 9 + 16


def test_separate_finalize_launches(monkeypatch):
    monkeypatch.setenv("VT_BN_FIN_APPLY", "0")
    m, r = _runner("efficientnet_b0")
    fwd, bwd = _kinds(r.program(torch.zeros(2, 3, 64, 64), N.VT_BF16, True, True))
    assert fwd.count(N.OP_BN_KEEP_APPLY) == 9 and fwd.count(N.OP_BN_ACT_AVGPOOL_APPLY) == 16 and bwd.count(N.OP_BN_KEEP_BWD_APPLY) == 9 + 16
    assert not {N.OP_BN_KEEP_FIN_APPLY, N.OP_BN_ACT_AVGPOOL_FIN_APPLY, N.OP_BN_KEEP_BWD_FIN_APPLY} & (set(fwd) | set(bwd))


def test_builder_refuses_what_the_keep_pass_does_not_take():
    mod = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, bias=False), nn.BatchNorm2d(16))
    store = E.ParamStore(mod)
    store.ensure(torch.device("cpu"))
    b = E.Builder(store, N.VT_BF16, True, True)
    x = b.act(2, 8, 8, 16, "x")
    row = b.keep_table([0.1], 2)[0]
    with pytest.raises(NotImplementedError, match="keep is keep"):
        b.conv_unit(x, mod[0], mod[1], 0, keep=row)  # no residual
    with pytest.raises(NotImplementedError, match="keep is keep"):
        b.conv_unit(x, mod[0], None, 0, residual=x, keep=row)  # no BatchNorm
    with pytest.raises(AssertionError, match="one keep table"):
        b.keep_table([0.1], 2)
    with pytest.raises(NotImplementedError, match="activation code 2"):
        b.se_mlp(b.act(2, 1, 1, 16, "p"), nn.Conv2d(16, 4, 1), nn.Conv2d(4, 16, 1), act=2)
    y = b.conv_unit(x, mod[0], mod[1], 3, residual=x, keep=row, name="u")  # SiLU in front of the factor: code 3
    assert (y.B, y.H, y.W, y.C) == (2, 8, 8, 16) and b.fwd[-1].kind == N.OP_BN_KEEP_FIN_APPLY and b.fwd[-1].i[5] == 3


@pytest.mark.parametrize("kw", [{}, {"optimizer": "AdamW"}, {"optimizer": "Adam"}, {"deterministic": True}, {"mix": True},
                                {"dtype": torch.float32}], ids=str)
@pytest.mark.parametrize("name", SMALL)
def test_train_step_plans(name, kw):
    kw = dict(kw)
    dtype = kw.pop("dtype", torch.bfloat16)
    _, sites, se = UNITS[name]
    ts = TrainStep(EfficientNetExtractor(name), 10, 2, 64, dtype, device="cpu", plan_only=True, **kw)
    fwd, bwd = _kinds(ts.prog)
    assert fwd.count(N.OP_BN_KEEP_FIN_APPLY) == sites and bwd.count(N.OP_BN_KEEP_BWD_REDUCE) == sites + se
    assert fwd.count(N.OP_BN_ACT_AVGPOOL_FIN_APPLY) == se and bwd.count(N.OP_SE_MLP_BWD) == se
    assert fwd.count(N.OP_AVGPOOL_FWD) == 1  # the head's pool alone
    assert len(ts._keep_rates) == sites and ts._keep_buf is not None and ts.drop_seed == 0
    convs = sum(isinstance(m, nn.Conv2d) for m in ts.model[0].modules()) - 2 * se
    assert ts.n_units == convs + 1  # every convolution outside the SE MLPs is a unit; and the head
    with pytest.raises(ValueError, match=f"{sites} sites"):
        ts.set_keep_factors(torch.ones(sites + 1, 2))
    ts.set_keep_factors(torch.ones(sites, 2))
    ts.set_keep_factors(None)


def test_a_trainer_without_stochastic_depth_has_no_table():
    ts = TrainStep(backbones.MobileNetExtractor("mobilenet_v2"), 10, 2, 64, torch.bfloat16, device="cpu", plan_only=True, drop_seed=3)
    assert ts._keep_buf is None and ts.keep_factors() is None
    with pytest.raises(RuntimeError, match="no keep table"):
        ts.set_keep_factors(torch.ones(1, 2))
