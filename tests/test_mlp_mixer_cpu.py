"""MLP-Mixer without a GPU: the state_dict contract against the fixtures of tools/gen_golden_mlp_mixer.py (the unmodified
reference on CPU), the CPU eager path at the f32 bounds, the Flax checkpoint loader, the compiled programs' op lists
("MLP-Mixer"), the train step's plans and the stated refusals."""
import numpy as np
import pytest
import torch

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import MLP, MixerBlock, MLPMixer
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import mlp_mixer_util as U

F32_TOL = 2e-4


@pytest.mark.parametrize("name", list(U.CASES))
def test_state_dict_keys_and_shapes_match_the_reference(name):
    g = U.load(name)
    sd = U.build(name).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]


def test_from_config_small_has_196_by_256_token_weights():
    m = MLPMixer.from_config("S", 16, 224)
    assert len(m.layers) == 8 and m.get_last_out_channels() == 512
    blk = m.layers[3]
    assert isinstance(blk, MixerBlock) and isinstance(blk.token_mixing, MLP)
    assert tuple(blk.token_mixing.linear1.weight.shape) == (256, 196)  # tokens_mlp_dim = 0.5 * d_model, over 196 tokens
    assert tuple(blk.token_mixing.linear2.weight.shape) == (196, 256)
    assert tuple(blk.channel_mixing.linear1.weight.shape) == (2048, 512)
    assert tuple(m.patch_embed.weight.shape) == (512, 3, 16, 16)
    # 393,728 (patch embedding) + 8 * (2 * 1,024 + 100,804 + 2,099,712) (blocks) + 1,024 (head norm): the 18.0 M of Mixer-S/16
    assert sum(p.numel() for p in m.parameters()) == 18_015_264
    assert [len(MLPMixer.from_config(v, 32, 224).layers) for v in "BLH"] == [12, 24, 32]
    with pytest.raises(KeyError):
        MLPMixer.from_config("Z", 16, 224)
    with pytest.raises(ValueError):
        MLPMixer(1, 16, 16, 100)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cpu_eager_matches_the_reference(name):
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    zero = U.zero_keys(g, U.CASES[name][0][0])
    x.requires_grad_(True)
    y = m(x)
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2
    ey = U.rel(y.detach(), U.t(g["y"]))
    (y * r).sum().backward()
    ex = U.gerr(x.grad, U.t(g["dx"]))
    print(f"{name}: y {ey:.3e} (bound {F32_TOL:.1e}) dx {ex:.3e} (bound {4 * F32_TOL:.1e})")
    assert ey < F32_TOL and ex < 4 * F32_TOL
    for k, p in m.named_parameters():
        if k in zero:
            continue
        e = U.gerr(p.grad, U.t(g["grad/" + k]))
        assert e < 4 * F32_TOL, f"grad {k}: {e}"


def test_fixture_floors_are_stored():
    for name in U.CASES:
        g = U.load(name)
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-6
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 3e-2
        assert 4 * float(g["floor/bf16/grad_max"]) < 0.25


def test_load_jax_weights_reproduces_the_reference_state_dict(tmp_path):
    g = np.load(U.GOLDEN / "mlp_mixer_flax.npz")
    m = MLPMixer(*[int(v) for v in g["args"]])
    src = {k[5:]: g[k] for k in g.files if k.startswith("flax/")}
    path = str(tmp_path / "ckpt.npz")
    np.savez(path, **src)
    m.load_jax_weights(path)
    sd = m.state_dict()
    want = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, U.t(want[k])), k
    # a classifier head may remain; anything else, or a missing array, is an error
    np.savez(path, **src, **{"head/kernel": np.zeros((16, 10), np.float32), "head/bias": np.zeros(10, np.float32)})
    m.load_jax_weights(path)
    np.savez(path, **src, extra=np.zeros(1, np.float32))
    with pytest.raises(KeyError):
        m.load_jax_weights(path)
    short = dict(src)
    del short["MixerBlock_1/token_mixing/Dense_1/bias"]
    np.savez(path, **short)
    with pytest.raises(KeyError):
        m.load_jax_weights(path)


def _dry_program(name, dtype, need_grad, x_grad=None):
    g = U.load(name)
    m = U.build(name)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad if x_grad is None else x_grad)
    return m, r, r.program(x, dtype, False, need_grad)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_program_op_list(dtype):
    """DESIGN.md, "MLP-Mixer": patchify + one GEMM, then per block layernorm -> token_mix (GELU fused) -> token_mix (shortcut
    fused) -> layernorm -> conv + GELU pass -> conv -> plain add; layernorm before the pool"""
    m, r, p = _dry_program("a", dtype, True)
    h = p.kind_histogram
    n = len(m.layers)
    assert h["patchify_fwd"] == 1 and h["patchify_bwd"] == 1
    assert h["token_mix"] == 2 * n + 2 * n  # forward, and the same kernel over W^T for the data gradients
    assert h["token_wgrad"] == 2 * n
    assert h["layernorm_fwd"] == 2 * n + 1 and h["layernorm_bwd"] == 2 * n + 1
    assert h["bn_act_apply"] == n  # the channel MLP's GELU pass alone: the token MLP's GELU is in its launch
    assert h["bn_bwd_apply"] == 2 * n  # GELU' of both MLPs
    assert h["scale_residual_fwd"] == n and "scale_residual_bwd" not in h
    assert h["avgpool_fwd"] == 1 and h["avgpool_bwd"] == 1
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    first = fwd.index("patchify_fwd")
    block = ["layernorm_fwd", "token_mix", "token_mix", "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm",
             "scale_residual_fwd"]
    assert fwd[first:] == ["patchify_fwd", "conv_igemm"] + block * n + ["layernorm_fwd", "avgpool_fwd"]
    # the patch embedding never becomes a convolution with more taps than the descriptor holds
    for op in fwd_ops + [p.bwd_ops[k] for k in range(p.n_bwd)]:
        if (op.kind & 0xFFFF) == N.OP_CONV_IGEMM:
            d = N.ConvDesc.from_buffer_copy(bytes(memoryview(op.i))[: E.C.sizeof(N.ConvDesc)])
            assert 1 <= d.ntaps <= N.VT_MAX_TAPS
    # token weights: bf16 programs address the mirror, f32 programs the masters; biases are f32 masters in both
    lin = m.layers[0].token_mixing.linear1
    _, off, _ = r.store.where(lin.weight)
    _, boff, _ = r.store.where(lin.bias)
    tm = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_TOKEN_MIX][0]
    want = (E.MIRROR, off * 2) if dtype == N.VT_BF16 else (E.PARAMS, off * 4)
    assert (tm.ptr[1].base, tm.ptr[1].offset) == want
    assert (tm.ptr[2].base, tm.ptr[2].offset) == (E.PARAMS, boff * 4)
    assert [tm.i[k] for k in (6, 8, 9, 10)] == [4, 25, 16, 32]  # GELU, K = 25 tokens, M = 16, C = 32
    assert len(p.outs) == 1 and (p.outs[0].B, p.outs[0].H, p.outs[0].W, p.outs[0].C) == (3, 1, 1, 32)


def test_program_without_image_gradient_and_inference():
    _, _, p = _dry_program("b", N.VT_BF16, True, x_grad=False)
    assert "patchify_bwd" not in p.kind_histogram and p.kind_histogram["token_wgrad"] == 4
    _, _, p = _dry_program("c", N.VT_BF16, False)
    assert p.n_bwd == 0 and p.kind_histogram["token_mix"] == 2 and "token_wgrad" not in p.kind_histogram


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(MLPMixer(2, 32, 4, 20), 10, 3, 20, dtype, device="cpu", plan_only=True, include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW", "Adam"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 32)
    groups = param_groups(ts.model)
    count = {g: sum(1 for p in ts.model.parameters() if groups[id(p)] == g) for g in (GROUP_NORM, GROUP_BIAS, GROUP_OTHER)}
    # 2 blocks: 2 * 2 + 1 LayerNorms (weight, bias); patch_embed + 4 Linear per block + head biases; as many weights
    assert count == {GROUP_NORM: 10, GROUP_BIAS: 10, GROUP_OTHER: 10}
    assert len(ts.segments) == 3
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_TOKEN_MIX) == 4 and fwd.count(N.OP_AVGPOOL_FWD) == 1 and fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd)]
    wg = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_TOKEN_WGRAD]
    assert len(wg) == 4 and all(op.kind & N.OP_SIDE_STREAM for op in wg)  # on the filter-gradient stream
    assert all(op.ptr[2].base == E.GRADS and op.ptr[3].base == E.GRADS for op in wg)


def test_train_step_deterministic_mix_and_validate_build():
    ts = _step(deterministic=True, optimizer="AdamW", mix=True)
    assert ts.deterministic
    assert ts.prog.kind_histogram["token_wgrad"] == 4


def test_include_pool_gate_still_refuses_map_returning_families():
    from vision_toolbox import backbones

    with pytest.raises(ValueError, match="include_pool=False"):
        TrainStep(backbones.vovnet19_slim_ese(), 16, 2, 64, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)


def test_refusals():
    m = MLPMixer(1, 16, 4, 16, dropout=0.1)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    m.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        r.program(torch.zeros(1, 3, 16, 16), N.VT_BF16, False, False)
    m.eval()
    r.program(torch.zeros(1, 3, 16, 16), N.VT_BF16, False, False)  # (dropout unused in eval mode)
    assert m.train()(torch.randn(2, 3, 16, 16)).shape == (2, 16)  # and CPU tensors run it in training mode
    with pytest.raises(ValueError, match="img_size"):
        r.program(torch.zeros(1, 3, 32, 32), N.VT_BF16, False, False)
    for d_model, dtype in ((12, N.VT_BF16), (20, N.VT_BF16), (6, N.VT_F32)):
        m = MLPMixer(1, d_model, 4, 16)
        r = m._vt_runner()
        r.store.ensure(torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="d_model"):
            r.program(torch.zeros(1, 3, 16, 16), dtype, False, False)
    # 3 * p * p values per patch off the chunk: p = 2 gives 12, no multiple of 8
    m = MLPMixer(1, 16, 2, 8)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="values per patch"):
        r.program(torch.zeros(1, 3, 8, 8), N.VT_BF16, False, False)
    r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)  # (12 is a multiple of the f32 chunk)
