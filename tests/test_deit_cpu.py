"""DeiT / DeiT3 without a GPU: the state_dict contract against the fixtures of tools/gen_golden_deit.py (the unmodified
reference on CPU, one image at a time), the batched CPU eager path at the f32 bounds of tests/test_vit_cpu.py, from_config, the
official checkpoint loader for both classes, resize_pe, the compiled programs' op lists (one vt_prefix_tokens_fwd and one
vt_prefix_pool_fwd in a DeiT; a DeiT3 list equal to the ViT list op for op), the train step's plans and the inherited
refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import DeiT, DeiT3, ViT
from vision_toolbox.trainer import GROUP_OTHER, TrainStep, param_groups

import deit_util as U
import test_vit_cpu as V  # (the refusal helper)

F32_TOL = 2e-4


def _all_fixtures():
    for name in U.CASES:
        yield name, U.load(name), U.build(name)
    g = np.load(U.GOLDEN / "deit_train.npz")
    yield "train", g, torch.nn.Sequential(DeiT(*U.TRAIN_ARGS, **U.TRAIN_KW), torch.nn.Linear(64, 10))


def test_state_dict_keys_order_and_shapes_match_the_reference():
    for name, g, m in _all_fixtures():
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["keys"]], name
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]], name
    # dist_token is registered after everything ViT registers, and it starts at zero
    m = U.build("a")
    assert isinstance(m, ViT) and not m.dist_token.any()
    assert [k for k, _ in m.named_parameters(recurse=False)] == ["cls_token", "pe", "dist_token"]
    assert [k for k in m.state_dict() if k != "dist_token"] == list(ViT(*U.CASES["a"][1]).state_dict().keys())
    assert list(U.build("c").state_dict().keys()) == list(ViT(*U.CASES["c"][1], layer_scale_init=1e-6).state_dict().keys())
    g = np.load(U.GOLDEN / "deit_ckpt.npz")
    args = [int(v) for v in g["args"]]
    for tag, cls in (("deit", DeiT), ("deit3", DeiT3)):
        sd = cls(*args).state_dict()
        want = {k[len(tag) + 4:]: g[k] for k in g.files if k.startswith(tag + "/sd/")}
        assert list(sd.keys()) == list(want.keys()), tag
        assert all(tuple(v.shape) == want[k].shape for k, v in sd.items()), tag


@pytest.mark.parametrize("name", list(U.CASES))
def test_batched_cpu_eager_matches_the_per_image_reference(name):
    """both tokens are broadcast over the batch: one batched run against what the reference computes image by image"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    zero = U.zero_keys(g, U.depth(name))
    assert int(g["per_image"]) == 1
    x.requires_grad_(True)
    y = m(x)
    (y * r).sum().backward()
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2
    ey, ex = U.rel(y.detach(), U.t(g["y"])), U.gerr(x.grad, U.t(g["dx"]))
    print(f"{name}: y {ey:.3e} (bound {F32_TOL:.1e}) dx {ex:.3e} (bound {4 * F32_TOL:.1e})")
    assert ey < F32_TOL and ex < 4 * F32_TOL
    for k, p in m.named_parameters():
        if k in zero:
            continue
        e = U.gerr(p.grad, U.t(g["grad/" + k]))
        assert e < 4 * F32_TOL, f"grad {k}: {e}"
    with torch.no_grad():
        assert torch.allclose(m(x), torch.cat([m(x[b:b + 1]) for b in range(x.shape[0])]), rtol=1e-5, atol=1e-6)


def test_fixture_floors_are_stored_and_below_the_cap():
    """the bf16 gradient bound of the GPU tests is min(4 x floor, 0.25): every floor is below 0.0625, the cap never binds"""
    for name in U.CASES:
        g = U.load(name)
        zero = U.zero_keys(g, U.depth(name))
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-5
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 0.0625
        for k in g.files:
            if k.startswith("floor/bf16/grad/") and k[len("floor/bf16/grad/"):] not in zero:
                assert float(g[k]) < 0.0625, k
    g = np.load(U.GOLDEN / "deit_train.npz")
    zero = U.zero_keys(g, 2, prefix="0.")
    assert float(g["floor/f32/grad_max"]) < 1e-5 and float(g["floor/bf16/grad_max"]) < 0.0625
    assert all(float(g[k]) < 0.0625 for k in g.files
               if k.startswith("floor/bf16/grad/") and k[len("floor/bf16/grad/"):] not in zero)


TABLE = {"Ti": (192, 12, 3), "S": (384, 12, 6), "M": (512, 12, 8), "B": (768, 12, 12), "L": (1024, 24, 16), "H": (1280, 32, 16)}


@pytest.mark.parametrize("cls", [DeiT, DeiT3], ids=["DeiT", "DeiT3"])
def test_from_config_covers_the_table_and_fetches_nothing(cls):
    for size, (d, depth, heads) in TABLE.items():
        with torch.device("meta"):  # (shapes only: an H model is 630 M parameters to initialise)
            m = cls.from_config(f"{size}_16", 224)
        assert type(m) is cls and isinstance(m, ViT)
        assert (m.d_model, len(m.layers), m.layers[0].mha[1].n_heads, m.patch_size) == (d, depth, heads, 16)
        assert tuple(m.pe.shape) == (1, 196, d) and m.pool_type == "cls_token" and tuple(m.cls_token.shape) == (1, 1, d)
        scaled = hasattr(m.layers[0].mha[2], "gamma")
        assert scaled == (cls is DeiT3) and hasattr(m, "dist_token") == (cls is DeiT)
    assert cls.from_config("S_32", 224).patch_size == 32
    # the parameter count of Ti_16: ViT's 5,524,224 plus the distillation token, or plus 24 layer scales of 192
    n = sum(p.numel() for p in cls.from_config("Ti_16", 224).parameters())
    assert n == 5_524_224 + (192 if cls is DeiT else 24 * 192)
    with pytest.raises(NotImplementedError, match="pretrained"):
        cls.from_config("S_16", 224, pretrained=True)
    with pytest.raises(KeyError):
        cls.from_config("Z_16", 224)


def test_deit3_defaults_and_the_class_token_requirement():
    m = DeiT3(64, 1, 1, 4, 16)
    assert float(m.layers[0].mha[2].gamma.detach()[0]) == pytest.approx(1e-6)
    assert float(m.layers[0].mlp[2].gamma.detach()[0]) == pytest.approx(1e-6)
    assert not hasattr(DeiT3(64, 1, 1, 4, 16, layer_scale_init=None).layers[0].mha[2], "gamma")
    with pytest.raises(ValueError, match="cls_token"):
        DeiT3(64, 1, 1, 4, 16, cls_token=False)


@pytest.mark.parametrize("tag", ["deit", "deit3"])
def test_load_official_ckpt_reproduces_the_reference_state_dict(tag):
    g = np.load(U.GOLDEN / "deit_ckpt.npz")
    cls = DeiT if tag == "deit" else DeiT3
    args = [int(v) for v in g["args"]]
    src = {k[len(tag) + 5:]: U.t(g[k]) for k in g.files if k.startswith(tag + "/src/")}
    want = {k[len(tag) + 4:]: g[k] for k in g.files if k.startswith(tag + "/sd/")}
    T = (args[4] // args[3]) ** 2
    assert src["pos_embed"].shape[1] == (T + 2 if cls is DeiT else T) and ("head_dist.weight" in src) == (cls is DeiT)
    m = cls(*args)
    given = dict(src)
    m.load_official_ckpt(given)
    assert given.keys() == src.keys()  # (the caller's dict is left as it was)
    sd = m.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, U.t(want[k])), k
    # the behaviours by name: the thirds of qkv, the last T rows of pos_embed, the folds
    assert torch.equal(sd["layers.0.mha.1.k_proj.weight"], src["blocks.0.attn.qkv.weight"][args[0]:2 * args[0]])
    assert torch.equal(sd["pe"], src["pos_embed"][:, -T:])
    if cls is DeiT:
        assert torch.equal(sd["cls_token"], src["cls_token"] + src["pos_embed"][:, 0])
        assert torch.equal(sd["dist_token"], src["dist_token"] + src["pos_embed"][:, 1])
    else:
        assert torch.equal(sd["cls_token"], src["cls_token"])  # (pos_embed has no class row: no fold)
    # head.* may be absent; any other leftover, or a missing key, is an error
    cls(*args).load_official_ckpt({k: v for k, v in src.items() if not k.startswith("head.")})
    with pytest.raises(KeyError, match="unexpected"):
        cls(*args).load_official_ckpt(dict(src, extra=torch.zeros(1)))
    for missing in ("blocks.0.attn.qkv.bias", "norm.weight", "pos_embed") + (("head_dist.bias", "dist_token") if cls is DeiT else
                                                                              ("blocks.0.gamma_2",)):
        with pytest.raises(KeyError):
            cls(*args).load_official_ckpt({k: v for k, v in src.items() if k != missing})


def test_resize_pe_leaves_both_tokens_untouched_and_runs():
    m = DeiT(32, 1, 1, 4, 8)
    U.fill(m, "deit_resize.")
    cls0, dist0 = m.cls_token.detach().clone(), m.dist_token.detach().clone()
    ref = ViT(32, 1, 1, 4, 8)
    ref.pe.data.copy_(m.pe.data)
    r = m._vt_runner()
    cpu = torch.device("cpu")
    r.store.ensure(cpu)
    r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    m.resize_pe(16)
    ref.resize_pe(16)
    assert tuple(m.pe.shape) == (1, 16, 32) and torch.equal(m.pe, ref.pe)  # (inherited: ViT's interpolation)
    assert torch.equal(m.cls_token, cls0) and torch.equal(m.dist_token, dist0)
    assert r.store.stale(cpu) and len(r.cache) == 0
    r.store.ensure(cpu)
    with pytest.raises(ValueError, match="patches"):
        r.program(torch.zeros(1, 3, 8, 8), N.VT_F32, False, False)
    p = r.program(torch.zeros(1, 3, 16, 16), N.VT_F32, False, False)
    tok = [p.fwd_ops[k] for k in range(p.n_fwd) if (p.fwd_ops[k].kind & 0xFFFF) == N.OP_PREFIX_TOKENS_FWD][0]
    assert [tok.i[k] for k in (2, 3, 4, 5)] == [2, 1, 16, 32]  # P, B, T, C
    assert m(torch.randn(2, 3, 16, 16)).shape == (2, 32)


def _dry_program(m, shape, dtype, need_grad):
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r, r.program(torch.zeros(*shape, requires_grad=need_grad), dtype, False, need_grad)


BLOCK = ["layernorm_fwd", "conv_igemm", "conv_igemm", "conv_igemm", "attn_fwd", "conv_igemm", "scale_residual_fwd",
         "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "scale_residual_fwd"]


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_deit_program_has_one_prefix_tokens_and_one_prefix_pool(name, dtype, need_grad):
    g, m = U.load(name), U.build(name)
    shape = [int(v) for v in g["x_shape"]]
    r, p = _dry_program(m, shape, dtype, need_grad)
    h, n = p.kind_histogram, len(m.layers)
    assert h["prefix_tokens_fwd"] == 1 and h["prefix_pool_fwd"] == 1
    assert "vit_tokens_fwd" not in h and "token_select_fwd" not in h and "token_prepend_fwd" not in h
    assert h["layernorm_fwd"] == 2 * n  # (the final norm is inside the pool launch)
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    first = fwd.index("patchify_fwd")
    assert fwd[first:] == ["patchify_fwd", "conv_igemm", "prefix_tokens_fwd"] + BLOCK * n + ["prefix_pool_fwd"]
    B, d, T = shape[0], m.d_model, m.pe.shape[1]
    tok = fwd_ops[fwd.index("prefix_tokens_fwd")]
    assert [tok.i[k] for k in range(7)] == [d, d, 2, B, T, d, dtype]  # lde ldo P B T C dtype
    for param, slot in ((m.pe, 1), (m.cls_token, 3), (m.dist_token, 4)):  # f32 masters in both dtypes
        _, off, _ = r.store.where(param)
        assert (tok.ptr[slot].base, tok.ptr[slot].offset) == (E.PARAMS, off * 4)
    assert tok.ptr[5].base < 0 and tok.ptr[6].base < 0
    pool = fwd_ops[-1]
    assert [pool.i[k] for k in range(7)] == [d, d, B, T + 2, 2, d, dtype] and pool.f[0] == m.norm.eps
    att = fwd_ops[fwd.index("attn_fwd")]
    assert att.i[6] == T + 2  # the blocks see L = T + 2 tokens
    if not need_grad:
        assert p.n_bwd == 0
        return
    assert h["prefix_tokens_bwd"] == 1 and h["prefix_pool_bwd"] == 1 and h["attn_bwd"] == n and h["layernorm_bwd"] == 2 * n
    assert "vit_tokens_bwd" not in h and "token_select_bwd" not in h and h["patchify_bwd"] == 1
    bwd_ops = [p.bwd_ops[k] for k in range(p.n_bwd)]
    bwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in bwd_ops]
    # the pool backward writes the whole d(map) (accumulate = 0: nothing was there) and its sums fold right behind it
    k = bwd.index("prefix_pool_bwd")
    assert [bwd_ops[k].i[j] for j in range(9)] == [d, d, d, 0, B, T + 2, 2, d, dtype]
    assert bwd[k + 1] == "channel_sums" and [bwd_ops[k + 1].i[j] for j in (0, 1)] == [2, d]
    assert bwd_ops[k + 1].ptr[0].offset == bwd_ops[k].ptr[4].offset and bwd_ops[k].ptr[4].base == E.ZERO_B
    tb = bwd_ops[bwd.index("prefix_tokens_bwd")]
    assert [tb.i[j] for j in range(7)] == [d, d, 2, B, T, d, dtype]
    assert all(tb.ptr[j].base >= 0 for j in range(5)) and tb.ptr[5].base < 0


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
def test_deit3_program_equals_the_vit_program_op_for_op(dtype, need_grad):
    args = U.CASES["c"][1]
    progs = []
    for m in (DeiT3(*args), ViT(*args, layer_scale_init=1e-6)):
        _, p = _dry_program(m, (2, 3, 16, 16), dtype, need_grad)
        progs.append((p.n_fwd, p.n_bwd, ctypes.string_at(ctypes.addressof(p.fwd_ops), p.n_fwd * ctypes.sizeof(N.Op)),
                      ctypes.string_at(ctypes.addressof(p.bwd_ops), p.n_bwd * ctypes.sizeof(N.Op)) if p.n_bwd else b"",
                      p.arena_bytes, dict(p.kind_histogram)))
    assert progs[0] == progs[1]
    assert "prefix_tokens_fwd" not in progs[0][5] and progs[0][5]["vit_tokens_fwd"] == 1 and progs[0][5]["token_select_fwd"] == 1


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(DeiT(*U.TRAIN_ARGS, **U.TRAIN_KW), 10, 3, 16, dtype, device="cpu", plan_only=True, include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer)
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 64)
    groups = param_groups(ts.model)
    bb = ts.model[0]
    assert all(groups[id(p)] == GROUP_OTHER for p in (bb.pe, bb.cls_token, bb.dist_token))
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_PREFIX_TOKENS_FWD) == 1 and fwd.count(N.OP_PREFIX_POOL_FWD) == 1 and fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd)]
    tok = [op for op in bwd if (op.kind & 0xFFFF) == N.OP_PREFIX_TOKENS_BWD]
    # d pe, d cls_token and d dist_token go into the flat gradients
    assert len(tok) == 1 and [tok[0].ptr[j].base for j in (2, 3, 4)] == [E.GRADS] * 3 and tok[0].ptr[5].base < 0
    pool = [k for k, op in enumerate(bwd) if (op.kind & 0xFFFF) == N.OP_PREFIX_POOL_BWD]
    assert len(pool) == 1 and (bwd[pool[0] + 1].kind & 0xFFFF) == N.OP_CHANNEL_SUMS
    assert [bwd[pool[0] + 1].ptr[j].base for j in (1, 2)] == [E.GRADS] * 2


def test_sharded_exchange_refuses_a_deit(monkeypatch):
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("VT_DP_WORLD1", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            _step(optimizer="AdamW", exchange="sharded")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cls", [DeiT, DeiT3], ids=["DeiT", "DeiT3"])
def test_inherited_refusals(cls):
    x = torch.zeros(1, 3, 16, 16)
    for kw, match in (({"dropout": 0.1}, "dropout"), ({"stochastic_depth": 0.1}, "stochastic_depth")):
        m = cls(64, 1, 2, 4, 16, **kw).train()
        V._refused(m, x, N.VT_BF16, NotImplementedError, match)
        m.eval()
        m._vt_runner().program(x, N.VT_BF16, False, False)  # (unused in eval mode)
        assert m.train()(torch.randn(2, 3, 16, 16)).shape == (2, 64)  # and CPU tensors run it in training mode
    with torch.device("meta"):  # (built without storage and cut to one of its 32 blocks, so that the test stays quick)
        h = cls.from_config("H_14", 224)
    assert "head_dim" in h._vt_refusal()
    h.layers = h.layers[:1]
    V._refused(h.to_empty(device="cpu"), torch.zeros(1, 3, 224, 224), N.VT_BF16, NotImplementedError, "head_dim")
    V._refused(cls(64, 1, 2, 4, 16, bias=False), x, N.VT_BF16, NotImplementedError, "bias=False")
    V._refused(cls(64, 1, 2, 4, 16), torch.zeros(1, 3, 32, 32), N.VT_BF16, ValueError, "patches")
    with pytest.raises(NotImplementedError, match="head_dim"):
        TrainStep(cls(80, 1, 1, 4, 16), 10, 2, 16, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)


def test_builder_checks_its_arguments():
    b = E.Builder(DeiT(64, 1, 2, 4, 16)._vt_runner().store, N.VT_BF16, False, False)
    e = b.act(1, 2, 2, 64)
    pe, tok = torch.nn.Parameter(torch.zeros(1, 4, 64)), torch.nn.Parameter(torch.zeros(1, 1, 64))
    with pytest.raises(ValueError, match="prefix tokens"):
        b.prefix_tokens(e, pe, [])
    with pytest.raises(ValueError, match="prefix tokens"):
        b.prefix_tokens(e, pe, [tok] * 5)
    with pytest.raises(ValueError, match="prefix token 1"):
        b.prefix_tokens(e, pe, [tok, torch.nn.Parameter(torch.zeros(1, 1, 32))])
    with pytest.raises(ValueError, match="pe holds"):
        b.prefix_tokens(e, torch.nn.Parameter(torch.zeros(1, 5, 64)), [tok])
    x = b.act(1, 1, 3, 64)
    with pytest.raises(ValueError, match="first 4 tokens"):
        b.prefix_pool(x, torch.nn.LayerNorm(64), 4)
    with pytest.raises(ValueError, match="first 0 tokens"):
        b.prefix_pool(x, torch.nn.LayerNorm(64), 0)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        b.prefix_pool(x, torch.nn.LayerNorm(32), 2)


def test_the_four_symbols_are_declared_and_resolve():
    names = ("vt_prefix_tokens_fwd", "vt_prefix_tokens_bwd", "vt_prefix_pool_fwd", "vt_prefix_pool_bwd")
    lib = N.lib()
    for name in names:
        assert name in N.SYMBOLS and getattr(lib, name).argtypes == N.SYMBOLS[name][1]
    # appended behind the last kind that existed: every earlier number stays
    assert [N.OP_PREFIX_TOKENS_FWD, N.OP_PREFIX_TOKENS_BWD, N.OP_PREFIX_POOL_FWD, N.OP_PREFIX_POOL_BWD] == [81, 82, 83, 84]
    assert N.OP_POOL_ATTN_BWD == 80 and N.OP_NAMES[N.OP_PREFIX_POOL_BWD] == "prefix_pool_bwd"
