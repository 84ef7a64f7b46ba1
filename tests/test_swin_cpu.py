"""Swin Transformer without a GPU: the state_dict contract against the fixtures of tools/gen_golden_swin.py (the unmodified
reference on CPU, one image at a time wherever a block is shifted), the CPU eager path at the f32 bounds of
tests/test_vit_cpu.py, the mask tiled over the batch, the official checkpoint loader, the compiled programs' op lists
(DESIGN.md 14), the train step's plans, the stated refusals, and the kernels' index maps (csrc/vt_window_index.h, compiled
into a host program) against torch's roll + window_partition and the module's own mask and index buffers."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist

from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox.backbones import (PatchMerging, SwinBlock, SwinTransformer, WindowAttention, window_partition,
                                      window_unpartition)
from vision_toolbox.backbones.swin import _axis_regions, shift_mask
from vision_toolbox.trainer import GROUP_BIAS, GROUP_NORM, GROUP_OTHER, TrainStep, param_groups

import swin_util as U

F32_TOL = 2e-4
CSRC = Path(N.__file__).resolve().parents[1] / "csrc"


def _train_model():
    return torch.nn.Sequential(SwinTransformer(*U.TRAIN_ARGS, **U.TRAIN_KW), torch.nn.Linear(64, 10))


def test_state_dict_keys_and_shapes_match_the_reference():
    fixtures = [(name, U.load(name), U.build(name)) for name in U.CASES]
    fixtures.append(("train", np.load(U.GOLDEN / "swin_train.npz"), _train_model()))
    for name, g, m in fixtures:
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["keys"]], name
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]], name
        assert not any("attn_mask" in k or "relative_pe_index" in k for k in sd), name  # non-persistent buffers


def test_from_config_variants_and_the_parameter_count_of_t():
    g = np.load(U.GOLDEN / "swin_ckpt.npz")
    m = SwinTransformer.from_config("T", 224)
    assert sum(p.numel() for p in m.parameters()) == int(g["T_224_params"]) == 27_519_354
    assert [len(s) - 1 for s in m.stages] == [2, 2, 6, 2] and m.out_channels_list == (96, 192, 384, 768) and m.stride == 32
    blk = m.stages[2][2]
    assert isinstance(blk, SwinBlock) and isinstance(blk.mha[1], WindowAttention) and isinstance(m.stages[2][0], PatchMerging)
    assert (blk.mha[1].n_heads, blk.mha[1].window_size, blk.mha[1].shift, blk.mha[1].input_size) == (12, 7, 3, 14)
    assert m.stages[3][2].mha[1].shift == 0  # a 7x7 map is one window: never shifted
    assert tuple(blk.mha[1].relative_pe_table.shape) == (1, 12, 169) and tuple(blk.mha[1].attn_mask.shape) == (4, 49, 49)
    for variant, (d, heads, depths, ws) in {"S": (96, 3, (2, 2, 18, 2), 7), "B": (128, 4, (2, 2, 18, 2), 7),
                                            "L": (192, 6, (2, 2, 18, 2), 7), "S3-T": (96, 3, (2, 2, 6, 2), 14),
                                            "S3-S": (96, 3, (2, 2, 18, 2), 14), "S3-B": (96, 3, (2, 2, 30, 2), 14)}.items():
        m = SwinTransformer.from_config(variant, 224)
        a = m.stages[2][1].mha[1]
        assert (m.out_channels_list[0], a.n_heads // 4, tuple(len(s) - 1 for s in m.stages), a.window_size) == (d, heads, depths, ws)
    assert SwinTransformer.ckpt_url("T").endswith("/v1.0.8/swin_tiny_patch4_window7_224_22k.pth")
    assert SwinTransformer.ckpt_url("S3-B").endswith("/v1.0/supernet-base.pth")
    with pytest.raises(KeyError):
        SwinTransformer.from_config("Z", 224)
    with pytest.raises(NotImplementedError):
        m.resize_pe(256)


def _eager(m, x, r, chunks):
    x.requires_grad_(True)
    ys = []
    for s in chunks:
        y = m(x[s])
        (y * r[s]).sum().backward()  # (parameter gradients accumulate over the images)
        ys.append(y.detach())
    return torch.cat(ys)


def _check_against_fixture(name, g, m, x, y):
    zero = U.zero_keys(g, m)
    assert tuple(y.shape) == g["y"].shape and y.dim() == 2
    ey, ex = U.rel(y, U.t(g["y"])), U.gerr(x.grad, U.t(g["dx"]))
    print(f"{name}: y {ey:.3e} (bound {F32_TOL:.1e}) dx {ex:.3e} (bound {4 * F32_TOL:.1e})")
    assert ey < F32_TOL and ex < 4 * F32_TOL
    for k, p in m.named_parameters():
        if k in zero:
            continue
        e = U.gerr(U.sample(p.grad), U.t(g["grad/" + k]))
        assert e < 4 * F32_TOL, f"grad {k}: {e}"


@pytest.mark.parametrize("name", list(U.CASES))
def test_cpu_eager_matches_the_reference(name):
    """cases with a shifted block image by image, as the fixture was made (the reference cannot run them batched)"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    assert int(g["per_image"]) == int(any(mod.shift > 0 for mod in m.modules() if isinstance(mod, WindowAttention)))
    assert int(g["per_image"]) == int(name != "c")
    chunks = [slice(b, b + 1) for b in range(x.shape[0])] if int(g["per_image"]) else [slice(0, x.shape[0])]
    _check_against_fixture(name, g, m, x, _eager(m, x, r, chunks))


@pytest.mark.parametrize("name", ["a", "b"])
def test_batched_eager_equals_per_image_eager(name):
    """the shift mask is tiled over the batch: what the reference computes image by image"""
    g = U.load(name)
    m = U.build(name)
    pre, x, r = U.inputs(g)
    U.fill(m, pre)
    y = _eager(m, x, r, [slice(0, x.shape[0])])
    _check_against_fixture(name, g, m, x, y)
    with torch.no_grad():
        maps = m.get_feature_maps(x)
        each = [m.get_feature_maps(x[b:b + 1]) for b in range(x.shape[0])]
    assert [list(f.shape) for f in maps] == g["map_shapes"].tolist()
    for i, f in enumerate(maps):
        assert torch.allclose(f, torch.cat([e[i] for e in each]), rtol=1e-5, atol=1e-5), i


def test_fixture_floors_are_stored_and_zero_keys_are_the_key_biases():
    for name in U.CASES:
        g = U.load(name)
        for k in ("y", "dx", "grad_max"):
            assert float(g[f"floor/f32/{k}"]) < 1e-6
            assert 1e-3 < float(g[f"floor/bf16/{k}"]) < 3e-2
        assert 4 * float(g["floor/bf16/grad_max"]) < 0.25
        U.zero_keys(g, U.build(name))
    g = np.load(U.GOLDEN / "swin_train.npz")
    U.zero_keys(g, _train_model())
    assert float(g["floor/f32/grad_max"]) < 1e-5 and float(g["floor/bf16/grad_max"]) < 0.25 / 4


def test_load_official_ckpt_reproduces_the_reference_state_dict():
    g = np.load(U.GOLDEN / "swin_ckpt.npz")
    m = SwinTransformer(*eval(str(g["args"])))  # noqa: S307  (a tuple literal the generator wrote)
    src = {k[len("official/"):]: U.t(g[k]) for k in g.files if k.startswith("official/")}
    want = {k[len("sd/"):]: g[k] for k in g.files if k.startswith("sd/")}
    m.load_official_ckpt(dict(src))
    sd = m.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, U.t(want[k])), k
    # the merging weights are permuted (dx, dy, c) -> (dy, dx, c); the table is transposed
    w = src["layers.0.downsample.reduction.weight"]
    assert torch.equal(m.stages[1][0].reduction.weight[:, 8:16], w[:, 16:24]) and not torch.equal(w[:, 8:16], w[:, 16:24])
    assert torch.equal(m.stages[0][1].mha[1].relative_pe_table[0], src["layers.0.blocks.0.attn.relative_position_bias_table"].T)
    short = dict(src)
    del short["layers.0.blocks.1.attn.qkv.bias"]
    with pytest.raises(KeyError):
        m.load_official_ckpt(short)


def test_window_partition_round_trip_and_patch_merging_order():
    x = torch.arange(2 * 6 * 9 * 2, dtype=torch.float32).view(2, 6, 9, 2)
    w, nH, nW = window_partition(x, 3)
    assert (tuple(w.shape), nH, nW) == ((12, 9, 2), 2, 3)
    assert torch.equal(w[4, 5], x[0, 3 + 1, 3 + 2])  # window (1, 1) of image 0, token (1, 2)
    assert torch.equal(window_unpartition(w, 3, nH, nW), x)
    pm = PatchMerging(2)
    with torch.no_grad():
        pm.norm.weight.fill_(1.0), pm.norm.bias.zero_(), pm.reduction.weight.copy_(torch.eye(4, 8))
    y = torch.arange(16, dtype=torch.float32).view(1, 2, 4, 2)
    got = pm(y)
    row = torch.cat([y[0, 0, 2], y[0, 0, 3], y[0, 1, 2], y[0, 1, 3]])  # (dy, dx, c)
    want = torch.nn.functional.layer_norm(row, (8,))[:4]
    assert tuple(got.shape) == (1, 1, 2, 4) and torch.allclose(got[0, 0, 1], want, atol=1e-6)


def _dry_program(name, dtype, need_grad, x_grad=None, all_maps=False):
    g = U.load(name)
    m = U.build(name)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    x = torch.zeros(*[int(v) for v in g["x_shape"]], requires_grad=need_grad if x_grad is None else x_grad)
    return m, r, r.program(x, dtype, all_maps, need_grad)


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_program_op_histogram(name, dtype, need_grad):
    """per block 2 layernorm, 6 linear units, 1 window attention forward and 1 backward; one patch gather for
    the embedding and one per merging; no global attention"""
    m, r, p = _dry_program(name, dtype, need_grad)
    (img, d_model, heads, depths, wss), kw = U.CASES[name]
    h, n, merges = p.kind_histogram, sum(depths), len(depths) - 1
    assert h["win_attn_fwd"] == n and "attn_fwd" not in h and "attn_bwd" not in h
    assert h["patchify_fwd"] == 1 + merges
    assert h["layernorm_fwd"] == 2 * n + 1 + merges + 1  # blocks, patch_norm, mergings, norm
    assert h["bn_act_apply"] == n and h["scale_residual_fwd"] == 2 * n and h["avgpool_fwd"] == 1
    fwd_ops = [p.fwd_ops[k] for k in range(p.n_fwd)]
    fwd = [N.OP_NAMES[op.kind & 0xFFFF] for op in fwd_ops]
    block = ["layernorm_fwd", "conv_igemm", "conv_igemm", "conv_igemm", "win_attn_fwd", "conv_igemm", "scale_residual_fwd",
             "layernorm_fwd", "conv_igemm", "bn_act_apply", "conv_igemm", "scale_residual_fwd"]
    want = ["patchify_fwd", "conv_igemm", "layernorm_fwd"]
    for s, depth in enumerate(depths):
        want += (["patchify_fwd", "layernorm_fwd", "conv_igemm"] if s else []) + block * depth
    assert fwd[fwd.index("patchify_fwd"):] == want + ["layernorm_fwd", "avgpool_fwd"]
    # every block's geometry: q | k | v are channel slices of one buffer, ws and shift as the module holds them
    esize, B = 2 if dtype == N.VT_BF16 else 4, int(U.load(name)["x_shape"][0])
    atts = [op for op in fwd_ops if (op.kind & 0xFFFF) == N.OP_WIN_ATTN_FWD]
    blocks = [mod for mod in m.modules() if isinstance(mod, SwinBlock)]
    for op, blk in zip(atts, blocks):
        a = blk.mha[1]
        C = a.q_proj.in_features
        assert [op.i[k] for k in range(12)] == [3 * C] * 3 + [C, B, a.input_size, a.input_size, a.n_heads, 32, a.window_size,
                                                              a.shift, dtype]
        assert op.ptr[1].offset - op.ptr[0].offset == C * esize and op.ptr[2].offset - op.ptr[1].offset == C * esize
        assert op.f[0] == 32 ** -0.5
        _, off, _ = r.store.where(a.relative_pe_table)
        assert (op.ptr[5].base, op.ptr[5].offset) == (E.PARAMS, off * 4)  # the f32 master in both dtypes
    assert [a.i[10] for a in atts] == {"a": [0, 2, 0, 1], "b": [0, 3, 0], "c": [0, 0]}[name]
    if not need_grad:
        assert p.n_bwd == 0 and "win_attn_bwd" not in h and h["conv_igemm"] == 6 * n + 1 + merges
        return
    assert h["win_attn_bwd"] == n and h["layernorm_bwd"] == 2 * n + 2 + merges and h["patchify_bwd"] == 1 + merges
    assert h["conv_wgrad"] == 6 * n + 1 + merges and h["colsum"] == 6 * n + 1  # (the reductions have no bias)
    assert h.get("scale_residual_bwd", 0) == (2 * n if "layer_scale_init" in kw else 0) and h["avgpool_bwd"] == 1
    bwds = [p.bwd_ops[k] for k in range(p.n_bwd) if (p.bwd_ops[k].kind & 0xFFFF) == N.OP_WIN_ATTN_BWD]
    for op, blk in zip(reversed(bwds), blocks):
        a = blk.mha[1]
        C = a.q_proj.in_features
        assert [op.i[k] for k in (5, 6, 7)] == [3 * C] * 3 and op.ptr[8].offset - op.ptr[7].offset == C * esize
        assert [op.i[k] for k in range(8, 16)] == [B, a.input_size, a.input_size, a.n_heads, 32, a.window_size, a.shift, dtype]
        assert not op.kind & N.OP_SIDE_STREAM and op.ptr[10].base >= 0  # d table
        assert int(op.f[1]) == int(N.lib().vt_win_attn_bwd_scratch_bytes(B, a.input_size, a.input_size, a.n_heads, a.window_size))


def test_program_with_all_maps_and_a_frozen_table():
    m, r, p = _dry_program("a", N.VT_BF16, True, all_maps=True)
    assert [(t.B, t.H, t.W, t.C) for t in p.outs] == [(2, 12, 12, 32), (2, 6, 6, 64), (2, 1, 1, 64)]
    m = U.build("a")
    for mod in m.modules():
        if isinstance(mod, WindowAttention):
            mod.relative_pe_table.requires_grad_(False)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    p = r.program(torch.zeros(2, 3, 48, 48), N.VT_BF16, False, True)
    bwds = [p.bwd_ops[k] for k in range(p.n_bwd) if (p.bwd_ops[k].kind & 0xFFFF) == N.OP_WIN_ATTN_BWD]
    assert len(bwds) == 4 and all(op.ptr[10].base < 0 for op in bwds)


def _step(dtype=torch.bfloat16, **kw):
    return TrainStep(SwinTransformer(*U.TRAIN_ARGS, **U.TRAIN_KW), 10, 2, 48, dtype, device="cpu", plan_only=True,
                     include_pool=False, **kw)


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW", "Adam"])
def test_train_step_plans(optimizer):
    ts = _step(optimizer=optimizer, deterministic=optimizer == "Adam")
    assert len(ts.model) == 2 and tuple(ts.model[1].weight.shape) == (10, 64)
    groups = param_groups(ts.model)
    count = {g: sum(1 for p in ts.model.parameters() if groups[id(p)] == g) for g in (GROUP_NORM, GROUP_BIAS, GROUP_OTHER)}
    # 4 blocks: 2 * 4 + patch_norm + merging + norm LayerNorms (weight, bias); patch_embed + 6 Linear per block + head biases;
    # as many weights, the bias-free reduction and the 4 tables
    assert count == {GROUP_NORM: 22, GROUP_BIAS: 26, GROUP_OTHER: 31}
    tables = [mod.relative_pe_table for mod in ts.model.modules() if isinstance(mod, WindowAttention)]
    assert len(tables) == 4 and all(groups[id(p)] == GROUP_OTHER for p in tables)  # decayed, as classifier.py:122-155 has it
    kinds = [ts.opt_ops[k].kind for k in range(ts.n_opt)]
    assert kinds == ([N.OP_SGD] * 3 if optimizer == "SGD" else [N.OP_ADAM_TICK] + [N.OP_ADAMW] * 3)
    fwd = [ts.prog.fwd_ops[k].kind & 0xFFFF for k in range(ts.prog.n_fwd)]
    assert fwd.count(N.OP_WIN_ATTN_FWD) == 4 and fwd.count(N.OP_AVGPOOL_FWD) == 1 and fwd[-1] == N.OP_XENT
    bwd = [ts.prog.bwd_ops[k] for k in range(ts.prog.n_bwd) if (ts.prog.bwd_ops[k].kind & 0xFFFF) == N.OP_WIN_ATTN_BWD]
    assert len(bwd) == 4 and all(op.ptr[10].base == E.GRADS for op in bwd)  # d table into the flat gradients


def test_sharded_exchange_refuses_a_swin(monkeypatch):
    """the tables and layer scales are f32-read parameters outside the head bucket the sharded exchange refreshes in f32:
    refused, not silently stale (a one-rank gloo group stands in for the job)"""
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
    x = torch.zeros(1, 3, 32, 32)
    args = (32, 32, 1, (2,), (4,))
    for kw, match in (({"dropout": 0.1}, "dropout"), ({"stochastic_depth": 0.1}, "stochastic_depth")):
        m = SwinTransformer(*args, **kw).train()
        _refused(m, x, N.VT_BF16, NotImplementedError, match)
        m.eval()
        m._vt_runner().program(x, N.VT_BF16, False, False)  # (unused in eval mode)
        assert m.train()(torch.randn(2, 3, 32, 32)).shape == (2, 32)  # and CPU tensors run it in training mode
    m = SwinTransformer(224, 32, 1, (2,), (14,))  # the S3 window: 196 tokens
    _refused(m, torch.zeros(1, 3, 224, 224), N.VT_BF16, NotImplementedError, "window_size=14")
    with torch.no_grad():
        assert m(torch.randn(1, 3, 224, 224)).shape == (1, 32)
    _refused(SwinTransformer(32, 64, 1, (1,), (4,)), x, N.VT_BF16, NotImplementedError, "head_dim")  # 64
    _refused(SwinTransformer(32, 32, 2, (1,), (4,)), x, N.VT_BF16, NotImplementedError, "head_dim")  # 16
    _refused(SwinTransformer(32, 32, 1, (1,), (4,), bias=False), x, N.VT_BF16, NotImplementedError, "bias=False")
    assert SwinTransformer(32, 32, 1, (1,), (4,), bias=False)(torch.randn(1, 3, 32, 32)).shape == (1, 32)
    _refused(SwinTransformer(*args), torch.zeros(1, 3, 64, 64), N.VT_BF16, ValueError, "64x64")
    with pytest.raises(NotImplementedError, match="head_dim"):
        TrainStep(SwinTransformer(32, 64, 1, (1,), (4,)), 10, 2, 32, torch.bfloat16, device="cpu", plan_only=True, include_pool=False)
    m = SwinTransformer(*args)
    with pytest.raises(NotImplementedError):
        m.resize_pe(64)
    # the builder's own checks name the argument as well
    b = E.Builder(m._vt_runner().store, N.VT_BF16, False, False)
    table = m.stages[0][1].mha[1].relative_pe_table
    q = b.act(1, 8, 8, 32)
    with pytest.raises(ValueError, match="shift=4"):
        b.window_attention(q, q, q, 1, table, 4, 4)
    with pytest.raises(ValueError, match="window_size=3"):
        b.window_attention(q, q, q, 1, table, 3, 0)
    with pytest.raises(ValueError, match="table"):
        b.window_attention(q, q, q, 1, table, 8, 0)
    with pytest.raises(NotImplementedError, match="head_dim"):
        b.window_attention(q, q, q, 2, table, 4, 0)
    q14 = b.act(1, 14, 14, 32)
    with pytest.raises(NotImplementedError, match="window_size=14"):
        b.window_attention(q14, q14, q14, 1, table, 14, 0)
    with pytest.raises(NotImplementedError, match="bias-free"):
        b.patch_merging(q, torch.nn.LayerNorm(128), torch.nn.Linear(128, 64))


_INDEX_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "vt_window_index.h"
int main(int argc, char** argv) {
    const int H = atoi(argv[1]), W = atoi(argv[2]), ws = atoi(argv[3]), shift = atoi(argv[4]);
    for (int wy = 0; wy < H / ws; ++wy)
        for (int wx = 0; wx < W / ws; ++wx)
            for (int t = 0; t < ws * ws; ++t) {
                int y, x;
                vt_win_pixel(wy, wx, t, ws, shift, H, W, &y, &x);
                printf("%d %d %d\n", y, x, vt_win_token_region(wy, wx, t, ws, shift, H, W));
            }
    for (int q = 0; q < ws * ws; ++q)
        for (int k = 0; k < ws * ws; ++k) printf("%d\n", vt_win_rel_index(q / ws, q % ws, k / ws, k % ws, ws));
    return 0;
}
"""


@pytest.fixture(scope="module")
def index_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the index-map test"
    d = tmp_path_factory.mktemp("win_index")
    (d / "main.cpp").write_text(_INDEX_MAIN)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(CSRC), str(d / "main.cpp"), "-o", str(d / "win_index")], check=True)
    return str(d / "win_index")


@pytest.mark.parametrize("H,W,ws,shift", [(14, 14, 7, 3), (12, 12, 4, 2), (6, 6, 3, 1), (8, 12, 4, 2), (16, 16, 8, 0)])
def test_index_maps_match_roll_and_window_partition(index_program, H, W, ws, shift):
    """the header the kernels are built from, run on the host: the pixel of every (window, token) against torch's roll +
    window_partition of a map of pixel numbers, the regions and the mask they give against the package's shift_mask (the
    module's own attn_mask where the map is square; the reference's masks are in swin_ckpt.npz, which load_official_ckpt
    compares), the relative index against the module's relative_pe_index"""
    out = subprocess.run([index_program, str(H), str(W), str(ws), str(shift)], check=True, capture_output=True, text=True).stdout
    vals = [[int(v) for v in line.split()] for line in out.splitlines()]
    L, nw = ws * ws, (H // ws) * (W // ws)
    tok = torch.tensor(vals[:nw * L]).view(nw, L, 3)
    rel = torch.tensor([v[0] for v in vals[nw * L:]]).view(L, L)
    assert len(vals) == nw * L + L * L
    pix = torch.arange(H * W).view(1, H, W, 1)
    want, _, _ = window_partition(pix.roll((-shift, -shift), (1, 2)), ws)
    assert torch.equal(tok[:, :, 0] * W + tok[:, :, 1], want[:, :, 0])
    # 3 r_y + r_x per token, from the package's region rule on the rolled map
    ry, rx = _axis_regions(H, ws, shift), _axis_regions(W, ws, shift)
    regions, _, _ = window_partition((3 * ry.view(H, 1) + rx.view(1, W)).view(1, H, W, 1), ws)
    assert torch.equal(tok[:, :, 2], regions[:, :, 0])
    mask = torch.where(tok[:, :, 2].unsqueeze(2) != tok[:, :, 2].unsqueeze(1), -100.0, 0.0)
    assert torch.equal(mask, shift_mask(H, W, ws, shift))
    a = WindowAttention(H, 32, 1, ws, shift > 0)
    assert a.shift == shift and torch.equal(rel, a.relative_pe_index)
    if H == W and shift > 0:
        assert torch.equal(mask, a.attn_mask)
    assert bool(mask.any()) == (shift > 0)
