"""ViT without a GPU: the state_dict contract against the fixtures of tools/gen_golden_vit.py (the unmodified reference on
CPU, one image at a time wherever there is a class token), the CPU eager path at the f32 bounds, the class token's broadcast,
the Flax checkpoint loader in both key layouts, resize_pe, the compiled programs' op lists, the train step's
plans and the stated refusals."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import MHA, MLP, MHAPooling, ViT, ViTBlock
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import vit_util as U

F32_TOL = 2e-4


def _all_fixtures():
    for name in U.CASES:
        yield name, U.load(name), U.build(name)
    g = np.load(U.GOLDEN / "vit_train.npz")
    yield "train", g, torch.nn.Sequential(ViT(*U.TRAIN_ARGS, **U.TRAIN_KW), torch.nn.Linear(64, 10))


def test_state_dict_keys_and_shapes_match_the_reference():
    for name, g, m in _all_fixtures():
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["keys"]], name
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]], name
    g = np.load(U.GOLDEN / "vit_flax.npz")
    args = [int(v) for v in g["args"]]
    for tag, kw in (("vt", {}), ("bv", {"cls_token": False, "pool_type": "mha"})):
        sd = ViT(*args, **kw).state_dict()
        want = {k[len(tag) + 4:]: g[k] for k in g.files if k.startswith(tag + "/sd/")}
        assert list(sd.keys()) == list(want.keys()), tag
        assert all(tuple(v.shape) == want[k].shape for k, v in sd.items()), tag


def test_from_config_variants_and_the_parameter_count_of_ti_16():
    m = ViT.from_config("Ti_16", 224)
    assert len(m.layers) == 12 and m.get_last_out_channels() == 192 and tuple(m.pe.shape) == (1, 196, 192)
    blk = m.layers[5]
    assert isinstance(blk, ViTBlock) and isinstance(blk.mha[1], MHA) and isinstance(blk.mlp[1], MLP)
    assert blk.mha[1].n_heads == 3 and blk.mha[1].scale == 64 ** -0.5
    assert tuple(blk.mlp[1].linear1.weight.shape) == (768, 192) and tuple(m.patch_embed.weight.shape) == (192, 3, 16, 16)
    # the reference's ViT.from_config("Ti_16", 224): 147,648 (patch embedding) + 192 (class token) + 37,632 (pe) +
    # 12 * 444,864 (blocks) + 384 (norm)
    assert sum(p.numel() for p in m.parameters()) == 5_524_224
    table = {"S_16": (384, 12, 6), "M_16": (512, 12, 8), "B_32": (768, 12, 12), "L_16": (1024, 24, 16), "H_14": (1280, 32, 16)}
    for variant, (d, depth, heads) in table.items():
        m = ViT.from_config(variant, 224)
        assert (m.d_model, len(m.layers), m.layers[0].mha[1].n_heads) == (d, depth, heads)
        assert m.patch_size == int(variant.split("_")[1])
    with pytest.raises(KeyError):
        ViT.from_config("Z_16", 224)
    with pytest.raises(ValueError, match="weights"):
        ViT.from_config("Ti_16", 224, weights="imagenet")
    with pytest.raises(ValueError):
        ViT(64, 1, 1, 16, 100)
    assert isinstance(ViT(32, 1, 1, 4, 8, cls_token=False, pool_type="mha").pooler, MHAPooling)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cpu_eager_matches_the_reference(name):
    """cases with a class token image by image, as the fixture was made (the reference cannot run them batched)"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    zero = U.zero_keys(g, U.CASES[name][0][1])
    assert int(g["per_image"]) == int(m.cls_token is not None)
    chunks = [slice(b, b + 1) for b in range(x.shape[0])] if int(g["per_image"]) else [slice(0, x.shape[0])]
    x.requires_grad_(True)
    ys = []
    for s in chunks:
        y = m(x[s])
        (y * r[s]).sum().backward()  # (parameter gradients accumulate over the images)
        ys.append(y.detach())
    y = torch.cat(ys)
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2
    ey, ex = U.rel(y, U.t(g["y"])), U.gerr(x.grad, U.t(g["dx"]))
    print(f"{name}: y {ey:.3e} (bound {F32_TOL:.1e}) dx {ex:.3e} (bound {4 * F32_TOL:.1e})")
    assert ey < F32_TOL and ex < 4 * F32_TOL
    for k, p in m.named_parameters():
        if k in zero:
            continue
        e = U.gerr(p.grad, U.t(g["grad/" + k]))
        assert e < 4 * F32_TOL, f"grad {k}: {e}"


def test_batched_eager_equals_per_image_eager():
    """the class token is broadcast over the batch: what the reference computes image by image"""
    g = U.load("a")
    m = U.build("a")
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    x.requires_grad_(True)
    y = m(x)
    (y * r).sum().backward()
    assert U.rel(y.detach(), U.t(g["y"])) < F32_TOL and U.gerr(x.grad, U.t(g["dx"])) < 4 * F32_TOL
    zero = U.zero_keys(g, 2)
    for k, p in m.named_parameters():
        if k not in zero:
            assert U.gerr(p.grad, U.t(g["grad/" + k])) < 4 * F32_TOL, k
    with torch.no_grad():
        assert torch.allclose(m(x), torch.cat([m(x[b:b + 1]) for b in range(3)]), rtol=1e-5, atol=1e-6)


def test_fixture_floors_are_stored_and_zero_keys_are_the_key_biases():
    """the windows of tests/test_mlp_mixer_cpu.py::test_fixture_floors_are_stored: the bounds of the GPU module tests carry over"""
    for name in U.CASES:
        g = U.load(name)
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-6
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 3e-2
        assert 4 * float(g["floor/bf16/grad_max"]) < 0.25
        U.zero_keys(g, U.CASES[name][0][1])
    g = np.load(U.GOLDEN / "vit_train.npz")
    U.zero_keys(g, 2, prefix="0.")
    assert float(g["floor/f32/grad_max"]) < 1e-5 and float(g["floor/bf16/grad_max"]) < 0.25 / 4


@pytest.mark.parametrize("tag", ["vt", "bv"])
def test_load_flax_ckpt_reproduces_the_reference_state_dict(tmp_path, tag):
    g = np.load(U.GOLDEN / "vit_flax.npz")
    big_vision = tag == "bv"
    kw = {"cls_token": False, "pool_type": "mha"} if big_vision else {}
    m = ViT(*[int(v) for v in g["args"]], **kw)
    src = {k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(tag + "/flax/")}
    path = str(tmp_path / "ckpt.npz")
    np.savez(path, **src)
    m.load_flax_ckpt(path, big_vision=big_vision)
    sd = m.state_dict()
    want = {k[len(tag) + 4:]: g[k] for k in g.files if k.startswith(tag + "/sd/")}
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, U.t(want[k])), k
    # under a prefix, beside arrays of another tower; a classifier head may remain
    np.savez(path, **{"params/img/" + k: v for k, v in src.items()}, **{"params/txt/x": np.zeros(1, np.float32)},
             **{"params/img/head/kernel": np.zeros((32, 10), np.float32)})
    m2 = ViT(*[int(v) for v in g["args"]], **kw)
    m2.load_flax_ckpt(path, big_vision=big_vision, prefix="params/img/")
    assert all(torch.equal(v, U.t(want[k])) for k, v in m2.state_dict().items())
    # anything else left over, or a missing array, is an error
    np.savez(path, **src, extra=np.zeros(1, np.float32))
    with pytest.raises(KeyError):
        m.load_flax_ckpt(path, big_vision=big_vision)
    short = dict(src)
    del short["Transformer/encoderblock_0/" + ("MultiHeadDotProductAttention_0" if big_vision else "MultiHeadDotProductAttention_1")
              + "/key/bias"]
    np.savez(path, **short)
    with pytest.raises(KeyError):
        m.load_flax_ckpt(path, big_vision=big_vision)


def test_resize_pe_matches_the_reference_and_invalidates_the_store():
    g = np.load(U.GOLDEN / "vit_resize.npz")
    m = ViT(*[int(v) for v in g["args"]])
    U.fill(m, str(g["recipe"][0]))
    assert torch.equal(m.pe.detach(), U.t(g["pe_before"]))
    r = m._vt_runner()
    cpu = torch.device("cpu")
    r.store.ensure(cpu)
    r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    assert not r.store.stale(cpu) and len(r.cache) == 1
    m.resize_pe(int(g["size"]))
    assert isinstance(m.pe, torch.nn.Parameter) and tuple(m.pe.shape) == g["pe_after"].shape
    assert U.rel(m.pe.detach(), U.t(g["pe_after"])) < 1e-6
    assert r.store.stale(cpu) and len(r.cache) == 0  # a replaced parameter is not something the store notices by itself
    r.store.ensure(cpu)
    # the token count follows pe: the old image size is refused, the new one compiles
    with pytest.raises(ValueError, match="patches"):
        r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    p = r.program(torch.zeros(1, 3, 16, 16), N.VT_F32, False, False)
    tok = [p.fwd_ops[k] for k in range(p.n_fwd) if (p.fwd_ops[k].kind & 0xFFFF) == N.OP_VIT_TOKENS_FWD][0]
    assert [tok.i[k] for k in (2, 3, 4)] == [1, 16, 32]  # B, T, C
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 32)


def _dry_program(name, dtype, need_grad, x_grad=None):
    g = U.load(name)
    m = U.build(name)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad if x_grad is None else x_grad)
    return m, r, r.program(x, dtype, False, need_grad)


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_program_op_histogram(name, dtype, need_grad):
    """per block 2 layernorm, 6 linear units, 1 attention forward and 1 backward; the token ops once"""
    m, r, p = _dry_program(name, dtype, need_grad)
    h, n = p.kind_histogram, len(m.layers)
    cls_pool = m.pool_type == "cls_token"
    scaled = name == "c"
    assert h["patchify_fwd"] == 1 and h["vit_tokens_fwd"] == 1
    assert h["attn_fwd"] == n and h["layernorm_fwd"] == 2 * n + 1
    assert h["bn_act_apply"] == n  # the MLP's GELU pass
    assert h["scale_residual_fwd"] == 2 * n
    assert h.get("token_select_fwd", 0) == int(cls_pool) and h.get("avgpool_fwd", 0) == int(not cls_pool)
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    block = ["layernorm_fwd", "conv_igemm", "conv_igemm", "conv_igemm", "attn_fwd", "conv_igemm", "scale_residual_fwd",
             "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "scale_residual_fwd"]
    tail = ["token_select_fwd", "layernorm_fwd"] if cls_pool else ["layernorm_fwd", "avgpool_fwd"]
    first = fwd.index("patchify_fwd")
    assert fwd[first:] == ["patchify_fwd", "conv_igemm", "vit_tokens_fwd"] + block * n + tail
    if not need_grad:
        assert p.n_bwd == 0 and "attn_bwd" not in h and h["conv_igemm"] == 6 * n + 1
        return
    assert h["attn_bwd"] == n and h["layernorm_bwd"] == 2 * n + 1 and h["vit_tokens_bwd"] == 1 and h["patchify_bwd"] == 1
    assert h["conv_wgrad"] == 6 * n + 1 and h["colsum"] == 6 * n + 1  # filter and bias gradients of the linear units
    assert h["conv_igemm"] == 2 * (6 * n + 1)  # forward, and the data gradients
    assert h.get("scale_residual_bwd", 0) == (2 * n if scaled else 0)
    assert h.get("token_select_bwd", 0) == int(cls_pool) and h.get("avgpool_bwd", 0) == int(not cls_pool)
    # q, k and v are channel slices of one buffer, as are their gradients; the scale is head_dim ** -0.5
    d_model, heads = U.CASES[name][0][0], U.CASES[name][0][2]
    att = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_ATTN_FWD][0]
    esize = 2 if dtype == N.VT_BF16 else 4
    assert [att.i[k] for k in range(9)] == [3 * d_model] * 3 + [d_model, int(U.load(name)["x_shape"][0]), heads,
                                                                 m.pe.shape[1] + int(m.cls_token is not None), d_model // heads,
                                                                 dtype]
    assert att.ptr[1].offset - att.ptr[0].offset == d_model * esize and att.ptr[2].offset - att.ptr[1].offset == d_model * esize
    assert att.f[0] == (d_model // heads) ** -0.5
    bwd = [p.bwd_ops[k] for k in range(p.n_bwd) if (p.bwd_ops[k].kind & 0xFFFF) == N.OP_ATTN_BWD][0]
    assert [bwd.i[k] for k in (5, 6, 7)] == [3 * d_model] * 3 and bwd.ptr[7].offset - bwd.ptr[6].offset == d_model * esize
    assert not bwd.kind & N.OP_SIDE_STREAM and int(bwd.f[1]) == int(N.lib().vt_attn_bwd_scratch_bytes(att.i[4], heads, att.i[6]))
    # pe and the class token are read as f32 masters in both dtypes
    tok = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_VIT_TOKENS_FWD][0]
    _, off, _ = r.store.where(m.pe)
    assert (tok.ptr[1].base, tok.ptr[1].offset) == (E.PARAMS, off * 4)
    assert (tok.ptr[2].base >= 0) == (m.cls_token is not None)


def test_program_without_image_gradient_and_with_a_frozen_embedding():
    _, _, p = _dry_program("a", N.VT_BF16, True, x_grad=False)
    assert "patchify_bwd" not in p.kind_histogram and p.kind_histogram["attn_bwd"] == 2
    m = U.build("a")
    m.patch_embed.requires_grad_(False)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    p = r.program(torch.zeros(3, 3, 16, 16), N.VT_BF16, False, True)
    assert p.kind_histogram["conv_wgrad"] == 12 and p.kind_histogram["vit_tokens_bwd"] == 1  # (pe and cls_token still train)


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(ViT(*U.TRAIN_ARGS, **U.TRAIN_KW), 10, 3, 16, dtype, device="cpu", plan_only=True, include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW", "Adam"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 64)
    groups = param_groups(ts.model)
    count = {g: sum(1 for p in ts.model.parameters() if groups[id(p)] == g) for g in (GROUP_NORM, GROUP_BIAS, GROUP_OTHER)}
    # 2 blocks: 2 * 2 + 1 LayerNorms (weight, bias); patch_embed + 6 Linear per block + head biases; as many weights, and pe
    assert count == {GROUP_NORM: 10, GROUP_BIAS: 14, GROUP_OTHER: 15}
    assert groups[id(ts.model[0].pe)] == GROUP_OTHER
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_ATTN_FWD) == 2 and fwd.count(N.OP_AVGPOOL_FWD) == 1 and fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd)]
    tok = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_VIT_TOKENS_BWD]
    assert len(tok) == 1 and tok[0].ptr[2].base == E.GRADS and tok[0].ptr[3].base < 0  # d pe into the flat gradients
    assert sum(1 for op in bwd if (op.kind & 0xFFFF) == N.OP_ATTN_BWD) == 2


def test_train_step_with_a_class_token_deterministic_mix():
    ts = TrainStep(ViT(64, 1, 2, 4, 16, layer_scale_init=0.1), 10, 3, 16, torch.bfloat16, device="cpu", plan_only=True,
                   include_pool=False, deterministic=True, optimizer="AdamW", mix=True)
    assert ts.deterministic
    groups = param_groups(ts.model)
    assert groups[id(ts.model[0].cls_token)] == GROUP_OTHER and groups[id(ts.model[0].pe)] == GROUP_OTHER
    h = ts.prog.kind_histogram
    assert h["attn_bwd"] == 1 and h["token_select_bwd"] == 1 and h["scale_residual_bwd"] == 2
    tok = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd) if (ts.prog.bwd_ops[k].kind & 0xFFFF) == N.OP_VIT_TOKENS_BWD][0]
    assert tok.ptr[2].base == E.GRADS and tok.ptr[3].base == E.GRADS and tok.i[2] == 1


def test_sharded_exchange_refuses_a_vit(monkeypatch):
    """pe, the class token and the layer scales are f32-read parameters outside the head bucket the sharded exchange
    refreshes in f32: refused, not silently stale (a one-rank gloo group stands in for the job)"""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            _step(optimizer="AdamW", exchange="sharded")
        ts = _step(optimizer="AdamW", exchange="allreduce", bucket_mb=0.05)
        assert ts.dp and ts.bucketer is not None
    finally:
        dist.destroy_process_group()


def _refused(m, x, dtype, exc, match):
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    with pytest.raises(exc, match=match):
        r.program(x, dtype, False, False)


def test_refusals():
    x = torch.zeros(1, 3, 16, 16)
    for kw, match in (({"dropout": 0.1}, "dropout"), ({"stochastic_depth": 0.1}, "stochastic_depth")):
        m = ViT(64, 1, 2, 4, 16, **kw).train()
        _refused(m, x, N.VT_BF16, NotImplementedError, match)
        m.eval()
        m._vt_runner().program(x, N.VT_BF16, False, False)  # (unused in eval mode)
        assert m.train()(torch.randn(2, 3, 16, 16)).shape == (2, 64)  # and CPU tensors run it in training mode
    m = ViT(64, 1, 2, 4, 16, cls_token=False, pool_type="mha")
    _refused(m, x, N.VT_BF16, NotImplementedError, "pool_type")
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 64)  # the pooler runs on CPU tensors
    _refused(ViT(80, 1, 1, 4, 16), x, N.VT_BF16, NotImplementedError, "head_dim")  # ViT-H's 80
    _refused(ViT(64, 1, 4, 4, 16), x, N.VT_BF16, NotImplementedError, "n_heads")  # head_dim 16
    _refused(ViT(64, 1, 2, 4, 16), torch.zeros(1, 3, 32, 32), N.VT_BF16, ValueError, "patches")
    with pytest.raises(NotImplementedError, match="head_dim"):
        TrainStep(ViT(80, 1, 1, 4, 16), 10, 2, 16, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    with pytest.raises(ValueError, match="cls_token"):
        ViT(64, 1, 2, 4, 16, cls_token=False)
    # the builder's own checks name the argument as well
    b = E.Builder(ViT(64, 1, 2, 4, 16)._vt_runner().store, N.VT_BF16, False, False)
    q = b.act(1, 1, 17, 96)
    with pytest.raises(NotImplementedError, match="head_dim"):
        b.attention(q, q, q, 2)
    with pytest.raises(ValueError, match="n_heads"):
        b.attention(q, q, q, 5)
    with pytest.raises(ValueError, match="token 17"):
        b.token_select(q, 17)
