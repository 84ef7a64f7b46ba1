"""PatchConvNet without a GPU: the state_dict contract against the fixtures of tools/gen_golden_patchconvnet.py (the unmodified
reference on CPU behind the two torchvision stand-ins), the CPU eager path at the f32 bounds of tests/test_cait_cpu.py,
from_config, the compiled programs' op lists, the train step's plans, the stated refusals, and the import of the
package where torchvision is absent."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import AttentionPooling, PatchConvBlockBN, PatchConvBlockLN, PatchConvNet, SqueezeExcitation
from vision_toolbox.components import StochasticDepth
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import patchconvnet_util as U

F32_TOL = 2e-4


def test_state_dict_keys_and_shapes_match_the_reference():
    for name in U.CASES:
        g, sd = U.load(name), U.build(name).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["keys"]], name
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]], name
    g = np.load(U.GOLDEN / "patchconvnet_train.npz")
    sd = torch.nn.Sequential(PatchConvNet(*U.TRAIN_ARGS, **U.TRAIN_KW), torch.nn.Linear(64, 10)).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    bn, ln = U.build("a").state_dict(), U.build("b").state_dict()
    assert {"stem.0.weight", "stem.6.weight", "trunk.1.layers.0.running_var", "trunk.1.layers.1.bias", "trunk.1.layers.3.weight",
            "trunk.1.layers.5.fc1.weight", "trunk.1.layers.5.fc2.bias", "trunk.1.layers.6.weight", "trunk.1.layer_scale",
            "pool.cls_token", "pool.attn.in_proj_weight", "pool.attn.in_proj_bias", "pool.attn.out_proj.weight",
            "pool.norm_3.bias", "pool.mlp.2.weight", "pool.layer_scale_2"} <= set(bn)
    assert {"trunk.2.layers.0.weight", "trunk.2.layers.1.weight", "trunk.2.layers.4.weight", "trunk.2.layers.6.fc1.bias",
            "trunk.2.layers.8.bias"} <= set(ln)
    assert tuple(bn["trunk.1.layer_scale"].shape) == (64, 1, 1) and tuple(ln["trunk.1.layer_scale"].shape) == (64,)
    assert tuple(bn["pool.cls_token"].shape) == (64,) and tuple(bn["pool.attn.in_proj_weight"].shape) == (192, 64)
    assert tuple(bn["trunk.1.layers.3.weight"].shape) == (64, 1, 3, 3) and tuple(bn["trunk.1.layers.5.fc1.weight"].shape) == (16, 64, 1, 1)


def test_from_config_and_the_modules():
    for variant, dim in (("S", 384), ("B", 768), ("L", 1024)):
        with torch.device("meta"):
            m = PatchConvNet.from_config(variant, 2)
        assert m.out_channels_list == (dim,) and m.stride == 16 and m.get_last_out_channels() == dim
        assert m.norm_type == "bn" and len(m._blocks()) == 2 and isinstance(m.trunk[1], PatchConvBlockBN)
        assert isinstance(m.trunk[1].drop_path, StochasticDepth) and m.trunk[1].drop_path.p == 0.3  # the reference default
        assert isinstance(m.pool, AttentionPooling) and m.pool.mlp[0].out_features == 3 * dim
        assert m.stem[0].out_channels == dim // 8 and m.stem[0].bias is None
    with pytest.raises(KeyError):
        PatchConvNet.from_config("XL", 2)
    with pytest.raises(ValueError):
        PatchConvNet.from_config("S", 2, pretrained=True)
    m = PatchConvNet(64, 1, drop_path=0.0, norm_type="ln")
    blk = m.trunk[1]
    assert isinstance(blk, PatchConvBlockLN) and isinstance(blk.drop_path, torch.nn.Identity)
    assert isinstance(m.pool.drop_path1, torch.nn.Identity) and float(blk.layer_scale.detach()[0]) == pytest.approx(1e-6)
    se = blk.layers[6]
    assert isinstance(se, SqueezeExcitation) and [n for n, _ in se.named_children()] == ["avgpool", "fc1", "fc2", "activation",
                                                                                         "scale_activation"]
    x = torch.randn(2, 64, 3, 5)
    want = torch.sigmoid(se.fc2(torch.relu(se.fc1(x.mean((2, 3), keepdim=True))))) * x
    assert torch.allclose(se(x), want, atol=1e-6)
    assert m(torch.randn(2, 3, 80, 48)).shape == (2, 64)  # non-square, batch > 1
    assert float(m.pool.attn.in_proj_bias.detach().abs().max()) == 0.0 and 0.01 < float(m.stem[6].weight.detach().std()) < 0.03


@pytest.mark.parametrize("name,mode", U.CASE_MODES, ids=[f"{n}-{mode}" for n, mode in U.CASE_MODES])
def test_cpu_eager_matches_the_reference(name, mode):
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    m.train(mode == "train")
    x.requires_grad_(True)
    y = m(x)
    (y * r).sum().backward()
    assert tuple(y.shape) == g[f"{mode}/y"].shape and y.dim() == 2
    ey, ex = U.rel(y.detach(), U.t(g[f"{mode}/y"])), U.gerr(U.stored("dx", x.grad), U.t(g[f"{mode}/dx"]))
    print(f"{name}/{mode}: y {ey:.3e} (bound {F32_TOL:.1e}) dx {ex:.3e} (bound {4 * F32_TOL:.1e})")
    assert ey < F32_TOL and ex < 4 * F32_TOL
    for k, p in m.named_parameters():
        e = U.gerr(U.stored("grad/" + k, p.grad), U.t(g[f"{mode}/grad/{k}"]))
        assert e < 4 * F32_TOL, f"grad {k}: {e}"
    if name == "c" and mode == "train":
        for k, v in m.named_buffers():
            assert torch.allclose(v.float(), U.t(g["train/running/" + k]).float(), rtol=1e-5, atol=1e-6), k


def test_fixture_floors_and_conditions_are_stored():
    for name, mode in U.CASE_MODES:
        g = U.load(name)
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{mode}/{k}"]) < 1e-5
            assert 1e-3 < float(g[f"floor/bf16/{mode}/{k}"]) < 0.3
        ratio, gmin, gmax, gstd, sstd = [float(v) for v in g[f"cond/{mode}"]]
        assert ratio >= 0.15 and 0.05 < gmin < gmax < 0.95 and gstd >= 0.02 and 0.25 <= sstd <= 3.0
        assert [str(s) for s in g["modes"]] == list(U.CASES[name][2])
    g = np.load(U.GOLDEN / "patchconvnet_train.npz")
    assert float(g["floor/f32/grad_max"]) < 1e-5 and float(g["floor/bf16/grad_max"]) < 0.25 / 4
    assert PatchConvNet is not None


def _dry_program(name, dtype, need_grad, training):
    g = U.load(name)
    m = U.build(name).train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad)
    return g, m, r, r.program(x, dtype, False, need_grad)


STEM = ["conv_igemm", "bn_act_apply"] * 3 + ["conv_igemm"]
BLOCK_TAIL = ["conv_igemm", "bn_act_apply", "dw3_gelu_pool_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "se_gate_fwd",
              "conv_igemm", "scale_residual_fwd"]
# (eval mode: the coefficients from the running statistics; a lone bn_eval_coeffs stays where it was emitted)
BN_TRAIN, BN_EVAL, LN = ["channel_stats", "bn_fin_apply"], ["bn_eval_coeffs", "bn_act_apply"], ["layernorm_fwd"]
POOL = ["token_prepend_fwd", "token_select_fwd", "layernorm_fwd", "token_select_fwd", "conv_igemm", "conv_igemm", "pool_attn_fwd",
        "conv_igemm", "scale_residual_fwd", "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "scale_residual_fwd",
        "layernorm_fwd"]


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,training", [("a", True), ("a", False), ("b", False), ("c", True)],
                         ids=["a-train", "a-eval", "b-eval", "c-train"])
def test_program_op_sequence_and_histogram(name, training, dtype, need_grad):
    """per block the norm, 1x1 + GELU, ONE dw3_gelu_pool launch, fc1 + ReLU, fc2, the gate, 1x1, the scaled
    residual; no depthwise filter gradient with atomics, no separate pooling, no hard-sigmoid gate"""
    g, m, r, p = _dry_program(name, dtype, need_grad, training)
    h, depth = p.kind_histogram, U.CASES[name][0][1]
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    first = fwd.index("conv_igemm")
    norm = LN if name == "b" else (BN_TRAIN if training else BN_EVAL)
    assert fwd[first:] == STEM + (norm + BLOCK_TAIL) * depth + POOL
    assert h.get("bn_eval_coeffs", 0) == (depth if (name != "b" and not training) else 0)
    assert h["dw3_gelu_pool_fwd"] == depth and h["se_gate_fwd"] == depth and h["pool_attn_fwd"] == 1
    for bad in ("dwconv_fwd", "dwconv_wgrad", "dwconv_dgrad", "avgpool_fwd", "avgpool_bwd", "ese_fwd", "ese_bwd", "cls_attn_fwd"):
        assert bad not in h, bad
    Cc, B = U.CASES[name][0][0], int(g["x_shape"][0])
    H, W = int(g["x_shape"][2]) // 16, int(g["x_shape"][3]) // 16
    esize = 2 if dtype == N.VT_BF16 else 4
    # the depthwise filter and its bias are f32 masters of the parameter store in both dtypes
    dwop = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_DW3_GELU_POOL_FWD][0]
    blk = m._blocks()[0]
    conv = blk.layers[blk._IDX[2]]
    for slot, prm in ((1, conv.weight), (2, conv.bias)):
        _, off, _ = r.store.where(prm)
        assert (dwop.ptr[slot].base, dwop.ptr[slot].offset) == (E.PARAMS, off * 4)
    assert [dwop.i[k] for k in range(8)] == [Cc, Cc, Cc, B, H, W, Cc, dtype]
    # attention pooling: the q GEMM and the k | v GEMM read row slices of the ONE in_proj parameter; k | v are the two
    # halves of one [B, 1, Lk, 2C] buffer; one head as wide as the embedding
    att = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_POOL_ATTN_FWD][0]
    assert [att.i[k] for k in range(8)] == [Cc, 2 * Cc, 2 * Cc, Cc, B, H * W + 1, Cc, dtype] and att.f[0] == Cc ** -0.5
    assert att.ptr[2].offset - att.ptr[1].offset == Cc * esize and att.ptr[1].base == att.ptr[2].base
    ia = fwd_ops.index(att)
    qop, kvop = fwd_ops[ia - 2], fwd_ops[ia - 1]
    _, woff, _ = r.store.where(m.pool.attn.in_proj_weight)
    _, boff, _ = r.store.where(m.pool.attn.in_proj_bias)
    wbase = E.MIRROR if dtype == N.VT_BF16 else E.PARAMS
    assert (qop.ptr[1].base, qop.ptr[1].offset) == (wbase, woff * esize)
    assert (kvop.ptr[1].base, kvop.ptr[1].offset) == (wbase, (woff + Cc * Cc) * esize)
    assert (qop.ptr[4].base, qop.ptr[4].offset) == (E.PARAMS, boff * 4)
    assert (kvop.ptr[4].base, kvop.ptr[4].offset) == (E.PARAMS, (boff + Cc) * 4)
    dq, dkv = N.ConvDesc.from_buffer_copy(bytes(qop.i)[:96 + 72]), N.ConvDesc.from_buffer_copy(bytes(kvop.i)[:96 + 72])
    assert (dq.B, dq.Wi, dq.Cin, dq.Cout) == (B, 1, Cc, Cc) and (dkv.B, dkv.Wi, dkv.Cin, dkv.Cout) == (B, H * W + 1, Cc, 2 * Cc)
    # the class token is the f32 master, broadcast by the prepend
    pre = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_FWD][0]
    _, off, _ = r.store.where(m.pool.cls_token)
    assert pre.ptr[1].base < 0 and (pre.ptr[2].base, pre.ptr[2].offset) == (E.PARAMS, off * 4)
    if not need_grad:
        assert p.n_bwd == 0 and "dw3_gelu_pool_bwd" not in h
        return
    assert h["dw3_gelu_pool_bwd"] == depth and h["se_gate_bwd"] == depth and h["pool_attn_bwd"] == 1
    assert h["token_prepend_bwd"] == 1 and h["token_select_bwd"] == 2
    bwd_ops = [p.bwd_ops[k] for k in range(p.n_bwd)]
    db = [op for op in bwd_ops if (op.kind & 0xFFFF) == N.OP_DW3_GELU_POOL_BWD]
    assert all(op.ptr[1].base >= 0 and op.ptr[2].base >= 0 and op.ptr[5].base >= 0 for op in db)  # d(a), d(pooled), d(u)
    assert all(op.ptr[7].base == E.ZERO_B and op.ptr[8].base == E.ZERO_B and not op.kind & N.OP_SIDE_STREAM for op in db)
    assert int(db[0].f[0]) == int(N.lib().vt_dw3_gelu_pool_bwd_scratch_bytes(B, Cc)) == B * Cc * 40
    assert len({(op.ptr[9].base, op.ptr[9].offset) for op in db}) == 1  # one scratch for every block
    if name != "b":
        assert h["bn_bwd_reduce"] == depth and h["bn_bwd_fin_apply"] == depth
    # the two in_proj GEMMs' filter gradients land in the matching row slices of the one parameter gradient
    wg = [op for op in bwd_ops if (op.kind & 0xFFFF) == N.OP_CONV_WGRAD and op.ptr[2].base == E.ZERO_B]
    offs = sorted(op.ptr[2].offset for op in wg)
    assert any(b - a == Cc * Cc * 4 for a in offs for b in offs)
    pb = [op for op in bwd_ops if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_BWD][0]
    assert pb.ptr[3].base == E.ZERO_B  # d cls_token, summed over the images by the prepend's backward


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(PatchConvNet(*U.TRAIN_ARGS, **U.TRAIN_KW), U.TRAIN_CLASSES, U.TRAIN_BATCH, U.TRAIN_SIZE, dtype, device="cpu",
                     plan_only=True, include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW", "Adam"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer, deterministic=True, mix=True)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 64) and ts.deterministic
    groups = param_groups(ts.model)
    bb = ts.model[0]
    blk = bb.trunk[1]
    for p in (bb.pool.cls_token, bb.pool.attn.in_proj_weight, bb.pool.attn.in_proj_bias, blk.layer_scale, bb.pool.layer_scale_1,
              blk.layers[3].weight):
        assert groups[id(p)] == GROUP_OTHER
    assert groups[id(blk.layers[0].weight)] == GROUP_NORM and groups[id(blk.layers[3].bias)] == GROUP_BIAS
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_DW3_GELU_POOL_FWD) == 1 and fwd.count(N.OP_POOL_ATTN_FWD) == 1 and fwd.count(N.OP_CHANNEL_STATS) == 1
    assert fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd)]
    db = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_DW3_GELU_POOL_BWD]
    assert len(db) == 1 and db[0].ptr[7].base == E.GRADS and db[0].ptr[8].base == E.GRADS  # into the flat f32 gradients
    assert not any((op.kind & 0xFFFF) == N.OP_DWCONV_WGRAD for op in bwd)  # deterministic mode admits the depthwise column
    pb = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_BWD]
    assert len(pb) == 1 and pb[0].ptr[3].base == E.GRADS  # d cls_token


def test_include_pool_false_refusal_of_a_map_backbone_lists_patchconvnet():
    from vision_toolbox import backbones

    with pytest.raises(ValueError, match="PatchConvNet"):
        TrainStep(backbones.darknet19(), 10, 2, 32, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)


def test_sharded_exchange_refuses_a_patchconvnet(monkeypatch):
    """the depthwise filters, the class token and the layer scales are f32-read parameters outside the head bucket the sharded
    exchange refreshes in f32: refused, not silently stale (a one-rank gloo group stands in for the job)"""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="sharded.*PatchConvNet"):
            _step(optimizer="AdamW", exchange="sharded")
        ts = _step(optimizer="AdamW", exchange="allreduce", bucket_mb=0.05)
        assert ts.dp and ts.bucketer is not None
    finally:
        dist.destroy_process_group()


def _refused(m, x, dtype, match):
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match=match):
        r.program(x, dtype, False, False)


def test_refusals():
    x = torch.zeros(1, 3, 32, 32)
    for nt in ("bn", "ln"):
        m = PatchConvNet(64, 1, norm_type=nt).train()  # the reference default drop_path = 0.3
        _refused(m, x, N.VT_BF16, "drop_path")
        m.eval()
        m._vt_runner().program(x, N.VT_BF16, False, False)  # (unused in eval mode)
        assert m.train()(torch.randn(2, 3, 32, 32)).shape == (2, 64)  # and CPU tensors run it in training mode
    with pytest.raises(NotImplementedError, match="drop_path"):
        TrainStep(PatchConvNet(64, 1), 10, 2, 32, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    m = PatchConvNet(32, 1, drop_path=0.0)  # embed_dim // 8 = 4: a whole chunk of f32, half a chunk of bf16
    _refused(m, x, N.VT_BF16, "embed_dim")
    m._vt_runner().program(x, N.VT_F32, False, False)
    assert m(torch.randn(2, 3, 32, 32)).shape == (2, 32)
    _refused(PatchConvNet(16, 1, drop_path=0.0), x, N.VT_F32, "embed_dim")
    # 96 x 96 tokens: the backward's two planes of one chunk do not fit 160 KiB; 32 x 32 does
    m = PatchConvNet(64, 1, drop_path=0.0)
    _refused(m, torch.zeros(1, 3, 1536, 1536), N.VT_BF16, "too large")
    m._vt_runner().program(torch.zeros(1, 3, 512, 512), N.VT_BF16, False, False)
    lib = N.lib()
    for hw in (14, 24, 32):
        assert lib.vt_dw3_gelu_pool_supported(hw, hw, N.VT_BF16) == 1 and lib.vt_dw3_gelu_pool_supported(hw, hw, N.VT_F32) == 1
    # the builder's own checks name the argument as well
    b = E.Builder(m._vt_runner().store, N.VT_BF16, False, False)
    with pytest.raises(NotImplementedError, match="depthwise 3x3"):
        b.dw3_gelu_pool(b.act(1, 4, 4, 64), torch.nn.Conv2d(64, 64, 3, padding=1))
    with pytest.raises(NotImplementedError, match="too large"):
        b.dw3_gelu_pool(b.act(1, 96, 96, 64), m.trunk[1].layers[3])
    with pytest.raises(ValueError, match="row per image"):
        b.se_gate(b.act(1, 4, 4, 64), b.act(1, 1, 2, 64))
    with pytest.raises(ValueError, match="geometry"):
        b.pool_attention(b.act(1, 1, 5, 64), b.act(1, 1, 5, 64), b.act(1, 1, 5, 64))
    with pytest.raises(NotImplementedError, match="channels"):
        b.pool_attention(b.act(1, 1, 1, 4104), b.act(1, 1, 5, 4104), b.act(1, 1, 5, 4104))
    with pytest.raises(NotImplementedError, match="BatchNorm2d"):
        b.batch_norm(b.act(1, 4, 4, 64), torch.nn.BatchNorm2d(32))


def test_the_package_imports_where_torchvision_is_absent():
    code = ("import sys; sys.modules['torchvision'] = None\n"
            "import vision_toolbox, vision_toolbox.backbones as B\n"
            "import torch\n"
            "m = B.PatchConvNet(64, 1, drop_path=0.0)\n"
            "assert m(torch.zeros(1, 3, 32, 32)).shape == (1, 64)\n"
            "assert not any(k == 'torchvision' or k.startswith('torchvision.') for k, v in sys.modules.items() if v is not None)\n"
            "print('ok')")
    pkg = str(U.GOLDEN.parents[1] / "vision-toolbox_amd")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": pkg}, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
    assert PatchConvNet.__module__ == "vision_toolbox.backbones.patchconvnet"
