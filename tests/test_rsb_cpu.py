"""Stochastic depth of ResNetExtractor without a GPU: the model surface (keys, parameter counts, rates), the eager path with
fixed factors against tests/rsb_util.py, the launch lists (keep ops exactly at the blocks with p > 0, in training mode only; the
finalize-inside and VT_BN_FIN_APPLY=0 forms; a frozen BatchNorm), the program cache key, the digests of the existing
programs, and the learning rates of the GPU step tests (the rule of NOTEBOOK 23.3)."""
import importlib.util
import os
from pathlib import Path

import pytest
import torch
from torch import nn

import resnet_util
import rsb_util as RU
from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox import engine as E
from vision_toolbox.backbones import ResNetExtractor
from vision_toolbox.program import mode_signature
from vision_toolbox.trainer import TrainStep

ROOT = Path(__file__).resolve().parents[1]
KEEP_FWD = (N.OP_BN_ADD_ACT_KEEP_APPLY, N.OP_BN_ADD_ACT_KEEP_FIN_APPLY)
PLAIN_FWD = (N.OP_BN_ADD_ACT_APPLY, N.OP_BN_ADD_ACT_FIN_APPLY)


# ---- model surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_the_argument_adds_no_parameter_and_sets_the_rates(name):
    plain, m = ResNetExtractor(name), ResNetExtractor(name, pretrained=False, stochastic_depth=0.1)
    assert list(plain.state_dict()) == list(m.state_dict())
    assert sum(p.numel() for p in plain.parameters()) == sum(p.numel() for p in m.parameters())
    n = sum(resnet_util.CONFIGS[name][1])
    assert len(m.blocks()) == n and m.drop_rates() == pytest.approx(RU.rates(name, 0.1), abs=0)
    assert m.drop_rates()[0] == 0.0 and m.drop_rates()[-1] == 0.1 and m.n_keep_sites == n - 1
    assert plain.drop_rates() == (0.0,) * n and plain.n_keep_sites == 0 and plain._vt_keep_rates() == ()
    # downsample blocks are included; eval mode has no site
    assert any(blk.downsample is not None and blk.drops() for blk in m.train().blocks())
    assert m._vt_keep_rates() == m.drop_rates()[1:] and m.eval()._vt_keep_rates() == ()
    _, sd = resnet_util.make_pair(name)
    m.load_torchvision_ckpt(sd)  # a torchvision checkpoint loads as before
    with pytest.raises(ValueError, match="stochastic_depth"):
        ResNetExtractor(name, stochastic_depth=1.0)
    with pytest.raises(ValueError, match="dropping blocks"):
        m.set_keep_factors(torch.ones(n, 2))
    with pytest.raises(NotImplementedError, match="pretrained"):
        ResNetExtractor(name, pretrained=True, stochastic_depth=0.1)


def test_eager_path_with_fixed_factors_matches_the_restatement():
    name, B = "resnet18", 3
    ref, sd = resnet_util.make_pair(name)
    m = ResNetExtractor(name, stochastic_depth=0.2)
    m.load_torchvision_ckpt(sd)
    m = m.double().train()
    ref.train()
    x = filler.images(B, 64).double()
    table = RU.table(RU.rates(name, 0.2), B)
    assert (table == 0).any(1).sum() >= 3 and not (table == 0).all(1).any()
    m.set_keep_factors(table)
    got = m.get_feature_maps(x)
    want = RU.maps(ref, x, RU.rates(name, 0.2), table.double())
    for g, w in zip(got, want):
        assert g.shape == w.shape and (g - w).abs().max().item() <= 1e-10 * w.abs().max().item()
    # the factors matter, and eval mode ignores them
    ref2, _ = resnet_util.make_pair(name)
    ref2.train()
    plain = RU.maps(ref2, x, RU.rates(name, 0.2), None)
    assert (plain[-1] - want[-1]).abs().max().item() > 1e-3 * want[-1].abs().max().item()
    m.eval(), ref.eval()
    for g, w in zip(m.get_feature_maps(x), RU.maps(ref, x, RU.rates(name, 0.2), None)):
        assert (g - w).abs().max().item() <= 1e-10 * w.abs().max().item()
    # a drawn table: every factor is 0 or 1 / (1 - p)
    m.train()
    m.set_keep_factors(None)
    torch.manual_seed(0)
    assert m.get_feature_maps(x)[-1].shape == want[-1].shape


# ---- launch lists -------------------------------------------------------------------------------------------------------------
def _program(m, dtype=N.VT_BF16, B=2, need_grad=True):
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(B, 3, 64, 64), dtype, True, need_grad)


def _kinds(prog):
    return ([prog.fwd_ops[k].kind & 0xFFFF for k in range(prog.n_fwd)], [prog.bwd_ops[k].kind & 0xFFFF for k in range(prog.n_bwd)])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_keep_ops_sit_exactly_at_the_blocks_that_drop(name, monkeypatch):
    n = sum(resnet_util.CONFIGS[name][1])
    m = ResNetExtractor(name, stochastic_depth=0.1).train()
    prog = _program(m)
    fwd, bwd = _kinds(prog)
    assert fwd.count(N.OP_BN_ADD_ACT_KEEP_FIN_APPLY) == n - 1 and fwd.count(N.OP_BN_ADD_ACT_FIN_APPLY) == 1
    assert bwd.count(N.OP_BN_ADD_ACT_KEEP_BWD_REDUCE) == n - 1 and bwd.count(N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY) == n - 1
    assert bwd.count(N.OP_BN_ADD_ACT_BWD_REDUCE) == 1 and bwd.count(N.OP_BN_ADD_ACT_BWD_FIN_APPLY) == 1
    # block ends in network order: the first is plain, the others carry the rows of the table in order, HW of their map
    ends = [prog.fwd_ops[k] for k in range(prog.n_fwd) if (prog.fwd_ops[k].kind & 0xFFFF) in KEEP_FWD + PLAIN_FWD]
    assert (ends[0].kind & 0xFFFF) == N.OP_BN_ADD_ACT_FIN_APPLY
    b = prog.builder
    assert b.keep_rates == m.drop_rates()[1:] and b.keep_B == 2
    for row, op in enumerate(ends[1:]):
        assert (op.ptr[13].base, op.ptr[13].offset) == (E.ARENA, b.keep_buf.offset + row * 2 * 4)
        assert op.i[5] * 2 == int(op.f[3])  # HW * B = M
    # the sites of backward, in reverse
    rows = [prog.bwd_ops[k].ptr[12].offset for k in range(prog.n_bwd)
            if (prog.bwd_ops[k].kind & 0xFFFF) == N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY]
    assert rows == sorted(rows, reverse=True) and len(set(rows)) == n - 1
    # eval mode, rate 0: what was always emitted, and no table
    for other in (ResNetExtractor(name, stochastic_depth=0.1).eval(), ResNetExtractor(name, stochastic_depth=0.0).train()):
        p2 = _program(other, need_grad=other.training)
        f2, b2 = _kinds(p2)
        assert not set(f2 + b2) & {N.OP_BN_ADD_ACT_KEEP_APPLY, N.OP_BN_ADD_ACT_KEEP_FIN_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_REDUCE,
                                   N.OP_BN_ADD_ACT_KEEP_BWD_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY}
        assert p2.builder.keep_buf is None
    # the separate launches
    monkeypatch.setenv("VT_BN_FIN_APPLY", "0")
    fwd, bwd = _kinds(_program(ResNetExtractor(name, stochastic_depth=0.1).train()))
    assert fwd.count(N.OP_BN_ADD_ACT_KEEP_APPLY) == n - 1 and bwd.count(N.OP_BN_ADD_ACT_KEEP_BWD_APPLY) == n - 1
    assert not {N.OP_BN_ADD_ACT_KEEP_FIN_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY} & set(fwd + bwd)


def test_frozen_batchnorm_takes_the_ready_coefficient_form():
    m = ResNetExtractor("resnet18", stochastic_depth=0.1).train()
    for k in ("layer3.0.bn1", "layer3.0.bn2", "layer3.0.downsample.1", "layer3.1.bn1", "layer3.1.bn2"):
        m.feat_extractor.get_submodule(k).eval()
    fwd, bwd = _kinds(_program(m))
    assert fwd.count(N.OP_BN_ADD_ACT_KEEP_APPLY) == 2 and fwd.count(N.OP_BN_ADD_ACT_KEEP_FIN_APPLY) == 5
    assert bwd.count(N.OP_BN_ADD_ACT_KEEP_BWD_REDUCE) == 7
    ts = TrainStep(ResNetExtractor("resnet18", stochastic_depth=0.1), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True,
                   freeze_bn=True, loss="bce", optimizer="Lamb")
    hist = ts.prog.kind_histogram
    assert hist["bn_add_act_keep_apply"] == 7 and "bn_add_act_keep_fin_apply" not in hist and hist["bce"] == 1
    assert ts._keep_rates == ts.model[0].drop_rates()[1:]


def test_builder_accepts_keep_with_residual_pre_act_and_refuses_the_rest_as_before():
    mod = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, bias=False), nn.BatchNorm2d(16))
    store = E.ParamStore(mod)
    store.ensure(torch.device("cpu"))
    b = E.Builder(store, N.VT_BF16, True, True)
    x = b.act(2, 8, 8, 16, "x")
    row = b.keep_table([0.1], 2)[0]
    with pytest.raises(NotImplementedError, match="keep is keep"):
        b.conv_unit(x, mod[0], mod[1], 0, keep=row)
    with pytest.raises(NotImplementedError, match="residual_pre_act is relu"):
        b.conv_unit(x, mod[0], mod[1], 3, residual=x, residual_pre_act=True, keep=row)  # not ReLU
    with pytest.raises(NotImplementedError, match="residual_pre_act is relu"):
        b.conv_unit(x, mod[0], mod[1], 1, residual_pre_act=True, keep=row)  # no residual
    y = b.conv_unit(x, mod[0], mod[1], 1, residual=x, residual_pre_act=True, keep=row, name="u")
    op = b.fwd[-1]
    assert (y.B, y.H, y.W, y.C) == (2, 8, 8, 16) and op.kind == N.OP_BN_ADD_ACT_KEEP_FIN_APPLY and op.i[5] == 64
    assert (op.ptr[13].base, op.ptr[13].offset) == row


def test_program_cache_key_changes_with_the_rates():
    sigs = []
    for sd in (0.0, 0.1, 0.2):
        m = ResNetExtractor("resnet18", stochastic_depth=sd).train()
        r = m._vt_runner()
        r.store.ensure(torch.device("cpu"))
        sigs.append(mode_signature(m, r.store))
    assert len(set(sigs)) == 3 and sigs[0][2] == ()
    m.eval()
    assert mode_signature(m, r.store)[2] == ()
    # the ops keep their numbers: the new ones are appended behind the loss op
    assert (N.OP_BN_ADD_ACT_APPLY, N.OP_BN_ADD_ACT_BWD_FIN_APPLY, N.OP_BN_KEEP_APPLY) == (85, 89, 101)
    assert [N.OP_BN_ADD_ACT_KEEP_APPLY, N.OP_BN_ADD_ACT_KEEP_FIN_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_REDUCE,
            N.OP_BN_ADD_ACT_KEEP_BWD_APPLY, N.OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY] == list(range(123, 128))
    for name in ("vt_bn_add_act_keep_apply", "vt_bn_add_act_keep_finalize_apply", "vt_bn_add_act_keep_bwd_reduce",
                 "vt_bn_add_act_keep_bwd_apply", "vt_bn_add_act_keep_bwd_finalize_apply"):
        assert name in N.SYMBOLS and getattr(N.lib(), name) is not None


# digests of existing programs as tools/program_digest.py prints them on the parent commit (resnet18: computed there the same way)
PARENT_DIGESTS = {
    "cspdarknet53 bf16 train+grad": "bef2bf25f139a1480ef8e95a5366067cdfca2c0e69d6c591ee17c94d849012da",
    "resnet18 bf16 train+grad": "56defe35b193a57a69d4220c214c300cde95ac1cb0656732e3ce4bc54b89c478",
    "resnet50 f32 eval": "5a68e2fbfa3c2da8938377ad45c8657559fe07ff7d368cd93af8b7a8205169ff",
}


def test_existing_programs_keep_their_digests():
    spec = importlib.util.spec_from_file_location("program_digest", ROOT / "tools" / "program_digest.py")
    pd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd)

    def digest(make, dt, training):
        pd.set_env({})
        m = make()
        m.train(training)
        r = m._vt_runner()
        r.store.ensure(torch.device("cpu"))
        return pd.program_digest(r.program(torch.zeros(2, 3, 64, 64), dt, True, training), r.store)

    saved = {k: os.environ.get(k) for k in pd.SWITCHES}
    try:
        assert digest(backbones.cspdarknet53, N.VT_BF16, True) == PARENT_DIGESTS["cspdarknet53 bf16 train+grad"]
        for make in (lambda: ResNetExtractor("resnet18"), lambda: ResNetExtractor("resnet18", stochastic_depth=0.0)):
            assert digest(make, N.VT_BF16, True) == PARENT_DIGESTS["resnet18 bf16 train+grad"]
        for make in (lambda: ResNetExtractor("resnet50"), lambda: ResNetExtractor("resnet50", stochastic_depth=0.3)):
            assert digest(make, N.VT_F32, False) == PARENT_DIGESTS["resnet50 f32 eval"]  # eval mode: the argument changes nothing
        assert digest(lambda: ResNetExtractor("resnet18", stochastic_depth=0.1), N.VT_BF16, True) != \
            PARENT_DIGESTS["resnet18 bf16 train+grad"]
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- the learning rates of the GPU step tests -------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["SGD", "Lamb"])
def test_step_learning_rates_keep_the_f32_restatement_within_a_tenth_of_the_tolerance(optimizer):
    want = RU.ref_steps(optimizer, torch.float64)
    got = RU.ref_steps(optimizer, torch.float32)
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print(f"{optimizer} lr {RU.STEP_LR[optimizer]}: float64 losses {want}, the float32 run off by {rel}")
    assert all(r <= 0.1 * RU.STEP_RTOL for r in rel)
    frozen = RU.ref_steps(optimizer, torch.float64, lr=0.0)
    assert frozen[0] == want[0] and abs(frozen[2] - want[2]) > 2 * RU.STEP_RTOL * abs(want[2])
    assert len(set(frozen)) == 3  # a different table per step moves the loss by itself
