"""ConvNeXt without a GPU: the state_dict contract against the fixtures of tools/gen_golden_convnext.py (the unmodified
reference on CPU), the CPU eager path, the official-checkpoint loader, the stated refusals' CPU side, and the op list of a
compiled program ("ConvNeXt")."""
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox.backbones import ConvNeXt, ConvNeXtBlock, GlobalResponseNorm
from vision_toolbox.components import LayerScale, Permute, StochasticDepth

import convnext_util as U


@pytest.mark.parametrize("name", list(U.CASES))
def test_state_dict_keys_and_shapes_match_the_reference(name):
    g = U.load(name)
    sd = U.build(name).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]


def test_from_config_tiny_parameter_count_and_child_indices():
    m = ConvNeXt.from_config("T")
    assert sum(p.numel() for p in m.parameters()) == 27_820_128
    assert isinstance(m.stem[0], torch.nn.Conv2d) and isinstance(m.stem[1], Permute) and isinstance(m.stem[2], torch.nn.LayerNorm)
    assert isinstance(m.stages[0][0], torch.nn.Identity)
    assert isinstance(m.stages[1][0][0], torch.nn.LayerNorm) and isinstance(m.stages[1][0][2], torch.nn.Conv2d)
    blk = m.stages[2][9]
    assert isinstance(blk, ConvNeXtBlock) and isinstance(blk.layers[8], LayerScale) and isinstance(blk.layers[9], StochasticDepth)
    assert [len(s) - 1 for s in m.stages] == [3, 3, 9, 3]
    with pytest.raises(KeyError):
        ConvNeXt.from_config("Z")
    assert ConvNeXt.from_config("A", v2=True).stages[0][1].layers[6].gamma.shape == (160,)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cpu_eager_matches_the_reference(name):
    g = U.load(name)
    m = U.build(name)
    pre, x, r, rf = U.inputs(g)
    U.fill(m, pre)
    x.requires_grad_(True)
    y = m(x)
    f = m.get_feature_maps(x)
    assert isinstance(f, list) and len(f) == 1
    f = f[0]
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2
    assert tuple(f.shape) == g["f"].shape and f.dim() == 4 and f.shape[-1] == y.shape[-1]
    torch.testing.assert_close(y.detach(), U.t(g["y"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(f.detach(), U.t(g["f"]), rtol=1e-5, atol=1e-5)
    ((y * r).sum() + (f * rf).sum()).backward()
    assert U.rel(x.grad, U.t(g["dx"])) < 1e-5
    for k, p in m.named_parameters():
        assert U.rel(p.grad, U.t(g["grad/" + k])) < 1e-5, k


def test_fixture_floors_are_stored():
    for name in U.CASES:
        g = U.load(name)
        for k in ("y", "f", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-6
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 3e-2
        assert float(g["floor/min_grad_norm64"]) > 1.0  # no parameter gradient sits at the noise floor


def _official_dict(m: ConvNeXt, head_norm=True):
    """a synthetic checkpoint in the official key layout, built from the mapping rule (not from the module's own names)"""
    sd, gen = {}, torch.Generator().manual_seed(3)

    def put(key, shape):
        sd[key] = torch.randn(shape, generator=gen)

    def wb(key, mod):
        put(key + ".weight", mod.weight.shape)
        put(key + ".bias", mod.bias.shape)

    wb("downsample_layers.0.0", m.stem[0])
    wb("downsample_layers.0.1", m.stem[2])
    for i, stage in enumerate(m.stages):
        if i > 0:
            wb(f"downsample_layers.{i}.0", stage[0][0])
            wb(f"downsample_layers.{i}.1", stage[0][2])
        for j in range(len(stage) - 1):
            L = stage[j + 1].layers
            for leaf, idx in (("dwconv", 1), ("norm", 3), ("pwconv1", 4), ("pwconv2", 7)):
                wb(f"stages.{i}.{j}.{leaf}", L[idx])
            if isinstance(L[6], GlobalResponseNorm):
                put(f"stages.{i}.{j}.grn.gamma", (1, 1, 1, L[6].gamma.numel()))  # (the official V2 layout)
                put(f"stages.{i}.{j}.grn.beta", (1, 1, 1, L[6].beta.numel()))
            if isinstance(L[8], LayerScale):
                put(f"stages.{i}.{j}.gamma", L[8].gamma.shape)
    if head_norm:
        wb("norm", m.norm)
    return sd


@pytest.mark.parametrize("v2", [False, True])
def test_load_official_ckpt(v2):
    m = ConvNeXt(16, (1, 2, 1), v2=v2)
    sd = _official_dict(m, head_norm=not v2)
    src = {k: v.clone() for k, v in sd.items()}
    m.load_official_ckpt(sd)
    own = m.state_dict()
    assert torch.equal(own["stem.0.weight"], src["downsample_layers.0.0.weight"])
    assert torch.equal(own["stem.2.bias"], src["downsample_layers.0.1.bias"])
    assert torch.equal(own["stages.1.0.0.weight"], src["downsample_layers.1.0.weight"])
    assert torch.equal(own["stages.2.0.2.bias"], src["downsample_layers.2.1.bias"])
    assert torch.equal(own["stages.1.2.layers.1.weight"], src["stages.1.1.dwconv.weight"])
    assert torch.equal(own["stages.1.2.layers.3.weight"], src["stages.1.1.norm.weight"])
    assert torch.equal(own["stages.1.1.layers.4.bias"], src["stages.1.0.pwconv1.bias"])
    assert torch.equal(own["stages.2.1.layers.7.weight"], src["stages.2.0.pwconv2.weight"])
    if v2:
        assert torch.equal(own["stages.0.1.layers.6.gamma"], src["stages.0.0.grn.gamma"].flatten())
    else:
        assert torch.equal(own["stages.0.1.layers.8.gamma"], src["stages.0.0.gamma"])
        assert torch.equal(own["norm.weight"], src["norm.weight"])
    # every tensor of the checkpoint landed somewhere: the multisets of values agree
    skip = ("norm.",) if v2 else ()
    mine = sorted(float(v.double().sum()) for k, v in own.items() if not k.startswith(skip))
    assert mine == sorted(float(v.double().sum()) for v in src.values())
    bad = dict(src)
    bad["stages.0.0.extra"] = torch.zeros(1)
    with pytest.raises(KeyError):
        ConvNeXt(16, (1, 2, 1), v2=v2).load_official_ckpt(bad)
    short = dict(src)
    del short["stages.1.1.pwconv2.bias"]
    with pytest.raises(KeyError):
        ConvNeXt(16, (1, 2, 1), v2=v2).load_official_ckpt(short)


def test_v2_and_stochastic_depth_run_on_cpu():
    x = torch.randn(2, 3, 32, 32)
    m = ConvNeXt(16, (1, 1), v2=True)
    assert all(isinstance(b.layers[8], torch.nn.Identity) for s in m.stages for b in list(s)[1:])
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.2)
    assert torch.isfinite(m(x)).all() and m.get_feature_maps(x)[0].shape == (2, 4, 4, 32)
    m = ConvNeXt(16, (2, 2), stochastic_depth=0.5).train()
    assert [round(b.layers[9].p, 4) for s in m.stages for b in list(s)[1:]] == [0.0, 0.1667, 0.3333, 0.5]
    assert m(x).shape == (2, 32)
    m.eval()
    assert torch.equal(m(x), m(x))


def _dry_program(name, dtype, need_grad, all_maps=True):
    g = U.load(name)
    m = U.build(name)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad)
    return m, r.program(x, dtype, all_maps, need_grad)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_program_op_list(dtype):
    """DESIGN.md, "ConvNeXt": per block dwconv (no bias pass) -> layernorm -> conv + GELU pass -> conv -> scale_residual"""
    m, p = _dry_program("a", dtype, True)
    h = p.kind_histogram
    n_ln = sum(isinstance(c, torch.nn.LayerNorm) for c in m.modules())
    n_blocks = sum(isinstance(c, ConvNeXtBlock) for c in m.modules())
    assert (n_ln, n_blocks) == (7, 3)
    assert h["layernorm_fwd"] == n_ln and h["layernorm_bwd"] == n_ln
    assert h["dwconv_fwd"] == n_blocks and h["dwconv_dgrad"] == n_blocks
    assert h["scale_residual_fwd"] == n_blocks and h["scale_residual_bwd"] == n_blocks
    assert h["channel_sums"] == n_ln + n_blocks  # one fold per LayerNorm (gamma, beta, pre_bias) and per layer scale
    assert h["bn_act_apply"] == n_blocks  # the GELU pass alone: no pass for the depthwise bias, none for the layer scale
    assert h["bn_bwd_apply"] == n_blocks  # GELU'
    assert h["avgpool_fwd"] == 1 and h["avgpool_bwd"] == 1
    assert h["colsum"] == 3 + 2 * n_blocks  # bias gradients: stem, two downsamples, two Linear per block
    for k in ("bn_finalize", "bn_fin_apply", "bn_bwd_reduce", "bn_bwd_fin_apply", "bn_eval_coeffs"):
        assert k not in h, k  # the first model here without BatchNorm
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in p.fwd_ops[: p.n_fwd]]
    first = fwd.index("dwconv_fwd")
    assert fwd[first : first + 7] == ["dwconv_fwd", "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm",
                                      "scale_residual_fwd", "layernorm_fwd"]
    assert len(p.outs) == 2 and (p.outs[0].B, p.outs[0].H, p.outs[0].W, p.outs[0].C) == (2, 2, 2, 64)
    assert (p.outs[1].H, p.outs[1].W, p.outs[1].C) == (1, 1, 64)


def test_program_without_layer_scale_and_inference():
    _, p = _dry_program("c", N.VT_BF16, True)
    assert p.kind_histogram["scale_residual_fwd"] == 2 and "scale_residual_bwd" not in p.kind_histogram
    _, p = _dry_program("b", N.VT_BF16, False, all_maps=False)
    assert p.n_bwd == 0 and len(p.outs) == 1 and p.kind_histogram["layernorm_fwd"] == 6


def test_channel_counts_outside_a_chunk_raise():
    m = ConvNeXt(12, (1,))
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        r.program(torch.zeros(1, 3, 16, 16), N.VT_BF16, True, False)
