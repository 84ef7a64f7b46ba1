"""CaiT without a GPU: the state_dict contract against the fixtures of tools/gen_golden_cait.py (the unmodified reference on
CPU, one image at a time), the CPU eager path at the f32 bounds, the class token's broadcast, the official checkpoint loader,
from_config, resize_pe, the compiled programs' op lists, the train step's plans and the stated refusals."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import CaiT, CaiTCABlock, CaiTSABlock, ClassAttention, TalkingHeadAttention
from vision_toolbox.trainer import GROUP_OTHER, TrainStep, param_groups

import cait_util as U

F32_TOL = 2e-4


def _depths(name):
    return U.CASES[name][0][1], U.CASES[name][0][2]


def test_state_dict_keys_and_shapes_match_the_reference():
    for name in U.CASES:
        g, sd = U.load(name), U.build(name).state_dict()
        assert list(sd.keys()) == [str(k) for k in g["keys"]], name
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]], name
    g = np.load(U.GOLDEN / "cait_train.npz")
    sd = torch.nn.Sequential(CaiT(*U.TRAIN_ARGS, **U.TRAIN_KW), torch.nn.Linear(96, 10)).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    keys = set(U.build("a").state_dict())
    assert {"cls_token", "pe", "patch_embed.weight", "sa_layers.0.mha.1.talking_head_proj.0.weight",
            "sa_layers.0.mha.1.talking_head_proj.2.bias", "sa_layers.0.mha.2.gamma", "ca_layers.0.mha.1.q_proj.weight",
            "ca_layers.0.mlp.2.gamma", "norm.weight"} <= keys
    assert not any(k.startswith("ca_layers.0.mha.1.talking") for k in keys)


def test_from_config_variants():
    table = {"xxs_24": (192, 24, 4), "xs_24": (288, 24, 6), "s_36": (384, 36, 8), "m_48": (768, 48, 16)}
    for variant, (d, depth, heads) in table.items():
        with torch.device("meta"):  # (m_48 holds 356 M parameters: shapes only)
            m = CaiT.from_config(variant, 224 if variant != "m_48" else 448)
        assert (m.d_model, len(m.sa_layers), len(m.ca_layers), m.sa_layers[0].mha[1].n_heads) == (d, depth, 2, heads)
        assert m.patch_size == 16 and d // heads == 48 and m.get_last_out_channels() == d
        assert m._vt_refusal() is None  # every named variant runs on the MI355X path
    m = CaiT.from_config("xxs_24", 224)
    assert tuple(m.pe.shape) == (1, 196, 192) and tuple(m.cls_token.shape) == (1, 1, 192)
    blk, ca = m.sa_layers[3], m.ca_layers[1]
    assert isinstance(blk, CaiTSABlock) and isinstance(blk.mha[1], TalkingHeadAttention)
    assert isinstance(ca, CaiTCABlock) and isinstance(ca.mha[1], ClassAttention)
    assert tuple(blk.mha[1].talking_head_proj[0].weight.shape) == (4, 4, 1, 1) and blk.mha[1].scale == 48 ** -0.5
    assert float(blk.mha[2].gamma.detach()[0]) == pytest.approx(1e-6)  # layer_scale_init of the CaiT blocks
    with pytest.raises(KeyError):
        CaiT.from_config("z_24", 224)
    with pytest.raises(NotImplementedError, match="pretrained"):
        CaiT.from_config("xxs_24", 224, pretrained=True)
    with pytest.raises(ValueError):
        CaiT(96, 1, 1, 2, 16, 100)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cpu_eager_matches_the_reference(name):
    """image by image, as the fixture was made (the reference cannot run a batch)"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    zero = U.zero_keys(g, *_depths(name))
    x.requires_grad_(True)
    ys = []
    for b in range(x.shape[0]):
        y = m(x[b:b + 1])
        (y * r[b:b + 1]).sum().backward()  # (parameter gradients accumulate over the images)
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


@pytest.mark.parametrize("name", ["a", "c"])
def test_batched_eager_equals_per_image_eager(name):
    """the class token is broadcast over the batch: what the reference computes image by image"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    x.requires_grad_(True)
    y = m(x)
    (y * r).sum().backward()
    assert U.rel(y.detach(), U.t(g["y"])) < F32_TOL and U.gerr(x.grad, U.t(g["dx"])) < 4 * F32_TOL
    zero = U.zero_keys(g, *_depths(name))
    for k, p in m.named_parameters():
        if k not in zero:
            assert U.gerr(p.grad, U.t(g["grad/" + k])) < 4 * F32_TOL, k
    with torch.no_grad():
        assert torch.allclose(m(x), torch.cat([m(x[b:b + 1]) for b in range(x.shape[0])]), rtol=1e-5, atol=1e-6)


def test_fixture_floors_are_stored_and_the_mixed_scores_are_neither_uniform_nor_one_hot():
    for name in U.CASES:
        g = U.load(name)
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-5
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 6e-2
        assert 4 * float(g["floor/bf16/grad_max"]) < 0.25
        assert 0.3 <= float(g["m_std"]) <= 3.0 and int(g["per_image"]) == 1
        U.zero_keys(g, *_depths(name))
    g = np.load(U.GOLDEN / "cait_train.npz")
    U.zero_keys(g, 1, 1, prefix="0.")
    assert float(g["floor/f32/grad_max"]) < 1e-5 and float(g["floor/bf16/grad_max"]) < 0.25 / 4


def test_load_official_ckpt_reproduces_the_reference_state_dict():
    g = np.load(U.GOLDEN / "cait_ckpt.npz")
    args = [int(v) for v in g["args"]]
    src = {k[len("official/"):]: U.t(g[k]) for k in g.files if k.startswith("official/")}
    want = {k[len("sd/"):]: g[k] for k in g.files if k.startswith("sd/")}
    assert "head.weight" in src and "head.bias" in src
    m = CaiT(*args)
    m.load_official_ckpt(src)
    assert "patch_embed.proj.weight" in src  # the caller's dict is left as it was
    sd = m.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, U.t(want[k])), k
    with pytest.raises(KeyError):
        CaiT(*args).load_official_ckpt({**src, "extra": torch.zeros(1)})
    short = dict(src)
    del short["blocks.0.attn.proj_w.bias"]
    with pytest.raises(KeyError):
        CaiT(*args).load_official_ckpt(short)
    # without LayerScale the gammas of the file are left over: an error, not a silent drop
    with pytest.raises(KeyError, match="gamma"):
        CaiT(*args, layer_scale_init=None).load_official_ckpt(src)


def test_resize_pe_invalidates_the_store_and_retargets_the_program():
    m = CaiT(96, 1, 1, 2, 4, 8)
    U.fill(m, "cait_resize.")
    before = m.pe.detach().clone()
    r = m._vt_runner()
    cpu = torch.device("cpu")
    r.store.ensure(cpu)
    r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    assert not r.store.stale(cpu) and len(r.cache) == 1
    m.resize_pe(16)
    assert isinstance(m.pe, torch.nn.Parameter) and tuple(m.pe.shape) == (1, 16, 96)
    want = torch.nn.functional.interpolate(before.unflatten(1, (2, 2)).permute(0, 3, 1, 2), (4, 4), mode="bicubic")
    assert torch.equal(m.pe.detach(), want.permute(0, 2, 3, 1).flatten(1, 2))
    assert r.store.stale(cpu) and len(r.cache) == 0
    r.store.ensure(cpu)
    with pytest.raises(ValueError, match="patches"):
        r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    p = r.program(torch.zeros(1, 3, 16, 16), N.VT_F32, False, False)
    tok = [p.fwd_ops[k] for k in range(p.n_fwd) if (p.fwd_ops[k].kind & 0xFFFF) == N.OP_VIT_TOKENS_FWD][0]
    assert [tok.i[k] for k in (2, 3, 4)] == [1, 16, 96] and tok.ptr[2].base < 0  # B, T, C; no class row in the token op
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 96)


def _dry_program(name, dtype, need_grad, x_grad=None):
    g = U.load(name)
    m = U.build(name)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad if x_grad is None else x_grad)
    return g, m, r, r.program(x, dtype, False, need_grad)


SA_BLOCK = ["layernorm_fwd", "conv_igemm", "conv_igemm", "conv_igemm", "talk_attn_fwd", "conv_igemm", "scale_residual_fwd",
            "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "scale_residual_fwd"]
CA_BLOCK = ["token_prepend_fwd", "token_select_fwd", "layernorm_fwd", "token_select_fwd", "conv_igemm", "conv_igemm", "conv_igemm",
            "cls_attn_fwd", "conv_igemm", "scale_residual_fwd", "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm",
            "scale_residual_fwd"]


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_program_op_histogram_and_forward_sequence(name, dtype, need_grad):
    """the twelve launches of a ViT block per SA block with talk_attn_fwd in place of attn_fwd, fifteen per CA
    block, one backward launch per attention"""
    g, m, r, p = _dry_program(name, dtype, need_grad)
    h, (ns, nc) = p.kind_histogram, _depths(name)
    scaled = name != "c"
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    first = fwd.index("patchify_fwd")
    assert fwd[first:] == ["patchify_fwd", "conv_igemm", "vit_tokens_fwd"] + SA_BLOCK * ns + CA_BLOCK * nc + ["layernorm_fwd"]
    assert "attn_fwd" not in h and "win_attn_fwd" not in h
    nlin = 6 * (ns + nc) + 1
    if not need_grad:
        assert p.n_bwd == 0 and "talk_attn_bwd" not in h and "cls_attn_bwd" not in h and h["conv_igemm"] == nlin
        return
    assert h["talk_attn_bwd"] == ns and h["cls_attn_bwd"] == nc and h["token_prepend_bwd"] == nc
    assert h["token_select_bwd"] == 2 * nc and h["layernorm_bwd"] == 2 * (ns + nc) + 1
    assert h["vit_tokens_bwd"] == 1 and h["patchify_bwd"] == 1
    assert h["conv_wgrad"] == nlin and h["colsum"] == nlin and h["conv_igemm"] == 2 * nlin
    assert h.get("scale_residual_bwd", 0) == (2 * (ns + nc) if scaled else 0)
    bwd_ops = [p.bwd_ops[k] for k in range(p.n_bwd)]
    d_model, heads = U.CASES[name][0][0], U.CASES[name][0][3]
    B, L = int(g["x_shape"][0]), m.pe.shape[1]
    esize = 2 if dtype == N.VT_BF16 else 4
    # talking heads: q | k | v are channel slices of one buffer, as are their gradients; the scale is head_dim ** -0.5
    att = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_TALK_ATTN_FWD][0]
    assert [att.i[k] for k in range(9)] == [3 * d_model] * 3 + [d_model, B, heads, L, 48, dtype]
    assert att.ptr[1].offset - att.ptr[0].offset == d_model * esize and att.ptr[2].offset - att.ptr[1].offset == d_model * esize
    assert att.f[0] == 48 ** -0.5
    # the mixing parameters are f32 masters of the parameter store in both dtypes, their gradients go to the f32 buffer
    th = m.sa_layers[0].mha[1].talking_head_proj
    for slot, prm in zip((5, 6, 7, 8), (th[0].weight, th[0].bias, th[2].weight, th[2].bias)):
        _, off, _ = r.store.where(prm)
        assert (att.ptr[slot].base, att.ptr[slot].offset) == (E.PARAMS, off * 4)
    tb = [op for op in bwd_ops if (op.kind & 0xFFFF) == N.OP_TALK_ATTN_BWD]
    assert [tb[0].i[k] for k in (4, 5, 6)] == [3 * d_model] * 3 and tb[0].ptr[10].offset - tb[0].ptr[9].offset == d_model * esize
    assert all(tb[0].ptr[k].base == E.ZERO_B for k in (12, 13, 14, 15)) and not tb[0].kind & N.OP_SIDE_STREAM
    want_bytes = int(N.lib().vt_talk_attn_bwd_scratch_bytes(B, heads, L))
    assert int(tb[0].f[1]) == want_bytes == 4 * (B * heads * L + B * ((L + 15) // 16) * (2 * heads * heads + 2 * heads))
    assert len({(op.ptr[16].base, op.ptr[16].offset) for op in tb}) == 1  # one scratch for every layer of that size
    # class attention: one query row per image, k | v two slices of one buffer over 1 + L keys
    ca = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_CLS_ATTN_FWD][0]
    assert [ca.i[k] for k in range(9)] == [d_model, 2 * d_model, 2 * d_model, d_model, B, heads, L + 1, 48, dtype]
    assert ca.ptr[2].offset - ca.ptr[1].offset == d_model * esize and ca.f[0] == 48 ** -0.5
    # the class token: the f32 master in the first CA block, the previous block's output afterwards
    pre_ops = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_FWD]
    _, off, _ = r.store.where(m.cls_token)
    assert pre_ops[0].ptr[1].base < 0 and (pre_ops[0].ptr[2].base, pre_ops[0].ptr[2].offset) == (E.PARAMS, off * 4)
    assert all(op.ptr[1].base >= 0 and op.ptr[2].base < 0 for op in pre_ops[1:])
    assert [pre_ops[0].i[k] for k in (3, 4, 5)] == [B, L, d_model]
    # the patch map has ca_depth consumers: the first to run in backward writes its gradient, the others accumulate
    pb = [op for op in bwd_ops if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_BWD]
    assert [op.i[2] for op in pb] == [0] + [1] * (nc - 1)
    assert pb[-1].ptr[3].base == E.ZERO_B and all(op.ptr[3].base < 0 and op.ptr[2].base >= 0 for op in pb[:-1])


def test_program_without_image_gradient_and_with_a_frozen_embedding():
    _, _, _, p = _dry_program("c", N.VT_BF16, True, x_grad=False)
    assert "patchify_bwd" not in p.kind_histogram and p.kind_histogram["talk_attn_bwd"] == 1
    m = U.build("c")
    m.patch_embed.requires_grad_(False)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    p = r.program(torch.zeros(2, 3, 36, 36), N.VT_BF16, False, True)
    assert p.kind_histogram["conv_wgrad"] == 18 and p.kind_histogram["vit_tokens_bwd"] == 1  # (pe still trains)


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(CaiT(*U.TRAIN_ARGS, **U.TRAIN_KW), 10, 3, 16, dtype, device="cpu", plan_only=True, include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW", "Adam"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer, deterministic=True)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 96) and ts.deterministic
    groups = param_groups(ts.model)
    bb = ts.model[0]
    th = bb.sa_layers[0].mha[1].talking_head_proj
    for p in (bb.pe, bb.cls_token, bb.sa_layers[0].mha[2].gamma, th[0].weight, th[2].weight):
        assert groups[id(p)] == GROUP_OTHER
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_TALK_ATTN_FWD) == 1 and fwd.count(N.OP_CLS_ATTN_FWD) == 1 and fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd)]
    tb = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_TALK_ATTN_BWD]
    assert len(tb) == 1 and all(tb[0].ptr[k].base == E.GRADS for k in (12, 13, 14, 15))  # into the flat f32 gradients
    pb = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_TOKEN_PREPEND_BWD]
    assert len(pb) == 1 and pb[0].ptr[3].base == E.GRADS  # d cls_token


def test_include_pool_false_refusal_of_a_map_backbone_lists_cait():
    from vision_toolbox import backbones

    with pytest.raises(ValueError, match="CaiT"):
        TrainStep(backbones.darknet19(), 10, 2, 32, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)


def test_sharded_exchange_refuses_a_cait(monkeypatch):
    """pe, the class token, the layer scales and the head-mixing weights are f32-read parameters outside the head bucket the
    sharded exchange refreshes in f32: refused, not silently stale (a one-rank gloo group stands in for the job)"""
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
        m = CaiT(96, 1, 1, 2, 4, 16, **kw).train()
        _refused(m, x, N.VT_BF16, NotImplementedError, match)
        m.eval()
        m._vt_runner().program(x, N.VT_BF16, False, False)  # (unused in eval mode)
        assert m.train()(torch.randn(2, 3, 16, 16)).shape == (2, 96)  # and CPU tensors run it in training mode
    m = CaiT(96, 1, 1, 2, 4, 16, bias=False)
    _refused(m, x, N.VT_BF16, NotImplementedError, "bias=False")
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 96)
    m = CaiT(64, 1, 1, 2, 4, 16)  # head_dim 32
    _refused(m, x, N.VT_BF16, NotImplementedError, "head_dim")
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 64)
    # (a d_model that is no multiple of the 16-byte chunk cannot have head_dim 48: the head_dim refusal names it first)
    _refused(CaiT(100, 1, 1, 2, 4, 16), x, N.VT_BF16, NotImplementedError, "head_dim")
    m = CaiT(48 * 17, 1, 1, 17, 4, 16)
    _refused(m, x, N.VT_BF16, NotImplementedError, "n_heads")
    assert m(torch.randn(1, 3, 16, 16)).shape == (1, 48 * 17)
    _refused(CaiT(96, 1, 0, 2, 4, 16), x, N.VT_BF16, NotImplementedError, "ca_depth")
    _refused(CaiT(96, 1, 1, 2, 4, 16), torch.zeros(1, 3, 32, 32), N.VT_BF16, ValueError, "patches")
    with pytest.raises(NotImplementedError, match="head_dim"):
        TrainStep(CaiT(64, 1, 1, 2, 4, 16), 10, 2, 16, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    # the builder's own checks name the argument as well
    model = CaiT(96, 1, 1, 2, 4, 16)
    b = E.Builder(model._vt_runner().store, N.VT_BF16, False, False)
    th = model.sa_layers[0].mha[1].talking_head_proj
    q64, q96, row = b.act(1, 1, 17, 64), b.act(1, 1, 17, 96), b.act(1, 1, 1, 96)
    with pytest.raises(NotImplementedError, match="head_dim"):
        b.talking_attention(q64, q64, q64, 2, th[0], th[2])
    big = b.act(1, 1, 17, 48 * 17)
    with pytest.raises(NotImplementedError, match="n_heads"):
        b.talking_attention(big, big, big, 17, th[0], th[2])
    with pytest.raises(ValueError, match="n_heads"):
        b.talking_attention(q96, q96, q96, 5, th[0], th[2])
    with pytest.raises(ValueError, match="proj_l"):
        b.talking_attention(q96, q96, q96, 2, torch.nn.Conv2d(3, 3, 1), th[2])
    with pytest.raises(ValueError, match="geometry"):
        b.talking_attention(q96, q96, b.act(1, 1, 18, 96), 2, th[0], th[2])
    with pytest.raises(NotImplementedError, match="head_dim"):
        b.class_attention(b.act(1, 1, 1, 80), b.act(1, 1, 17, 80), b.act(1, 1, 17, 80), 1)
    with pytest.raises(ValueError, match="geometry"):
        b.class_attention(q96, q96, q96, 2)  # the query is one row per image
    with pytest.raises(ValueError, match="n_heads"):
        b.class_attention(row, q96, q96, 5)
    with pytest.raises(ValueError, match="first token"):
        b.token_prepend(q96, b.act(1, 1, 2, 96))
    with pytest.raises(ValueError, match="first token"):
        b.token_prepend(q96, torch.nn.Parameter(torch.zeros(1, 1, 64)))
