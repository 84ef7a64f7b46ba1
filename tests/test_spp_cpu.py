"""SPPBlock without a GPU: the reference's contract (constructor, child, empty state_dict, errors), the eager path against
fixtures of the unmodified reference (tools/gen_golden_spp.py), the launch lists compiled on the CPU and every refusal by
name.

Bounds: the eager path is plain torch on both sides, the same ops in the same order, so every case is compared with
torch.equal in float32; the chain (two ConvNormAct units around the block) with the CPU bounds of tests/test_bifpn_cpu.py --
relative L2 below 1e-6 for the map and the running statistics, 1e-5 for every gradient."""
import pytest
import torch
from torch import nn

import spp_util as SU
from vision_toolbox import _native as N
from vision_toolbox import components
from vision_toolbox import engine as E
from vision_toolbox.components import ConvNormAct, HipModule, SPPBlock

CASES = list(SU.CASES)


@pytest.fixture(scope="module")
def gold():
    return SU.load()


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class Chain(HipModule):
    """cv1 -> spp -> cv2 as one compiled program: the three `_vt_emit`s chained"""

    def __init__(self, children):
        super().__init__()
        for k, m in children.items():
            self.add_module(k, m)

    def _vt_emit_maps(self, b, x):
        h = self.cv1._vt_emit(b, x, name="cv1")
        h = self.spp._vt_emit(b, h, name="spp")
        return [self.cv2._vt_emit(b, h, name="cv2")]

    def _eager_maps(self, x):
        return [self.cv2(self.spp(self.cv1(x)))]


# ---- the reference's contract ------------------------------------------------------------------------------------------
def test_constructor_child_and_state_dict_are_the_reference_s():
    assert "SPPBlock" in components.__all__ and "DeformableConv2d" not in components.__all__
    m = SPPBlock()
    assert isinstance(m.pool, nn.MaxPool2d) and (m.pool.kernel_size, m.pool.stride, m.pool.padding) == (5, 1, 2)
    assert m.repeats == 3 and [n for n, _ in m.named_children()] == ["pool"]
    assert len(m.state_dict()) == 0 and not list(m.parameters())
    a = SPPBlock(7, 2, "avg")
    assert isinstance(a.pool, nn.AvgPool2d) and (a.pool.kernel_size, a.pool.stride, a.pool.padding) == (7, 1, 3) and a.repeats == 2
    assert a.pool.count_include_pad and a.pool.divisor_override is None
    assert SPPBlock(pool="max", repeats=1, kernel_size=13).pool.padding == 6
    with pytest.raises(KeyError):
        SPPBlock(pool="median")


def test_even_kernel_size_cannot_be_concatenated():
    """the maps shrink by a pixel per stage and the reference's torch.cat raises; with one stage there is nothing to concat"""
    with pytest.raises(RuntimeError, match="even kernel_size"):
        SPPBlock(4, 2)(torch.zeros(1, 8, 9, 9))
    assert SPPBlock(4, 1)(torch.zeros(1, 8, 9, 9)).shape == (1, 8, 8, 8)
    with pytest.raises(RuntimeError, match="even kernel_size"):
        _program(SPPBlock(4, 2), (1, 8, 9, 9))


# ---- the eager path against the reference's fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_eager_path_equals_the_reference_fixtures(gold, case):
    m = SU.build(components, case)
    x = SU.inputs(case)
    y = m(x)  # a CPU tensor: the eager path
    SU.loss(case, y).backward()
    (k, repeats, _), shape, _ = SU.CASES[case]
    assert y.shape == (shape[0], repeats * shape[1], *shape[2:])
    assert torch.equal(y.detach(), torch.from_numpy(gold[f"{case}/y"]))
    assert torch.equal(x.grad, torch.from_numpy(gold[f"{case}/dx"]))


def test_fixture_case_c_is_not_a_big_window(gold):
    """AvgPool2d pads every stage with zeros and divides by k^2: the cascade differs from 9- and 13-windows over x"""
    x = SU.inputs("c").detach()
    y = torch.from_numpy(gold["c/y"])
    C = x.shape[1]
    assert torch.equal(y[:, :C], nn.functional.avg_pool2d(x, 5, 1, 2))
    assert (y[:, C : 2 * C] - nn.functional.avg_pool2d(x, 9, 1, 4)).abs().max() > 0.05


def test_fixture_max_cases_are_the_big_windows(gold):
    x = SU.inputs("a").detach()
    y = torch.from_numpy(gold["a/y"])
    for s, k in enumerate((5, 9, 13)):
        assert torch.equal(y[:, 16 * s : 16 * (s + 1)], nn.functional.max_pool2d(x, k, 1, k // 2))


def test_chain_matches_the_reference_fixtures(gold):
    m = SU.build_chain(components, Chain).train()
    assert list(m.state_dict().keys()) == list(gold["chain/keys"])
    SU.fill(m)
    x = SU.inputs("chain")
    y = m(x)
    SU.loss("chain", y).backward()
    assert rel(y.detach(), gold["chain/y"]) < 1e-6 and rel(x.grad, gold["chain/dx"]) < 1e-5
    zero = set(gold["chain/zero_grad_keys"])
    assert zero == {"cv1.norm.bias"}
    for k, p in m.named_parameters():
        if k in zero:  # zero in exact arithmetic (tools/gen_golden_spp.py): noise of the sums on both sides
            assert p.grad.abs().max() < 1e-4 * float(m.cv1.norm.weight.grad.norm())
        else:
            assert rel(p.grad, gold[f"chain/grad/{k}"]) < 1e-5, k
    for k, v in m.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert rel(v, gold[f"chain/state/{k}"]) < 1e-6, k


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
def _program(m, shape, dtype=N.VT_F32, need_grad=True, training=True):
    m.train(training)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(*shape, requires_grad=need_grad), dtype, False, need_grad)


def _ops(prog):
    return list(prog.fwd_ops)[: prog.n_fwd], list(prog.bwd_ops)[: prog.n_bwd]


def _of(ops, kind):
    return [op for op in ops if op.kind & 0xFFFF == kind]


def test_new_op_codes_are_appended_and_the_library_exports_the_entry_points():
    assert [N.OP_SPP_FWD, N.OP_SPP_BWD] == [111, 112] and N.OP_WFUSE_FIN == 110
    assert [N.OP_NAMES[k] for k in (111, 112)] == ["spp_fwd", "spp_bwd"]
    lib = N.lib()
    for sym in ("vt_spp_fwd", "vt_spp_bwd", "vt_spp_supported"):
        assert sym in N.SYMBOLS and getattr(lib, sym) is not None
    ok = [(5, 3), (3, 4), (7, 2), (9, 2), (13, 1), (11, 1), (15, 1), (3, 1), (5, 4)]
    bad = [(7, 3), (11, 2), (5, 5), (4, 2), (4, 1), (1, 1), (17, 1), (19, 1), (5, 0)]  # (17: a tap 16*17+16 does not fit a byte)
    assert all(lib.vt_spp_supported(k, r) == 1 for k, r in ok) and all(lib.vt_spp_supported(k, r) == 0 for k, r in bad)


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_one_forward_and_one_backward_launch(case, dtype):
    (k, repeats, pool), shape, _ = SU.CASES[case]
    B, C, H, W = shape
    prog = _program(SU.build(components, case), shape, dtype)
    fwd, bwd = _ops(prog)
    (f,), (g,) = _of(fwd, N.OP_SPP_FWD), _of(bwd, N.OP_SPP_BWD)
    code = 0 if pool == "max" else 1
    # i: ldx ldy B H W C k repeats pool dtype | lddy lddx accumulate B H W C k repeats pool dtype
    assert list(f.i[:10]) == [C, repeats * C, B, H, W, C, k, repeats, code, dtype]
    assert list(g.i[:11]) == [repeats * C, C, 0, B, H, W, C, k, repeats, code, dtype]
    # the block is the two launches; the rest is what every stand-alone module has (layout conversions of the NCHW input and
    # its gradient, the copy of the caller's seed gradient, the stream join): no pooling op, nothing per stage
    names = {N.OP_NAMES[op.kind & 0xFFFF] for op in fwd + bwd}
    assert names <= {"spp_fwd", "spp_bwd", "nchw_to_nhwc", "nhwc_to_nchw", "memset", "copy2d", "join"}, names
    assert len(fwd) <= 3 and len(bwd) <= 5, (len(fwd), len(bwd))
    # taps: one byte per element and stage, only for max, shared by the two launches.  The same block with avg pooling
    # allocates everything else the same way, so the arenas differ by exactly the taps buffer.
    other = _program(SPPBlock(k, repeats, "avg" if pool == "max" else "max"), shape, dtype)
    diff = abs(prog.builder.arena_top - other.builder.arena_top)
    assert diff == E._round_up(repeats * B * H * W * C, E.ALIGN)
    if pool == "max":
        assert f.ptr[2].base == E.ARENA and (g.ptr[1].base, g.ptr[1].offset) == (f.ptr[2].base, f.ptr[2].offset)
        assert prog.builder.arena_top > other.builder.arena_top
    else:
        assert f.ptr[2].base == -1 and g.ptr[1].base == -1


@pytest.mark.parametrize("case", CASES)
def test_inference_program_has_no_taps_and_no_backward(case):
    shape = SU.CASES[case][1]
    prog = _program(SU.build(components, case), shape, N.VT_BF16, need_grad=False, training=False)
    fwd, bwd = _ops(prog)
    (f,) = _of(fwd, N.OP_SPP_FWD)
    assert f.ptr[2].base == -1 and not bwd
    # and the arena holds the input and the output only: nothing of the size of a taps buffer was allocated
    B, C, H, W = shape
    repeats = SU.CASES[case][0][1]
    assert prog.builder.arena_top <= E._round_up(B * H * W * C * 2, E.ALIGN) + E._round_up(B * H * W * C * repeats * 2, E.ALIGN)


def test_chain_program_holds_the_two_conv_units_around_the_block():
    m = SU.build_chain(components, Chain)
    prog = _program(m, SU.CHAIN_SHAPE, N.VT_F32)
    fwd, bwd = _ops(prog)
    assert prog.n_units == 2
    kf = [op.kind & 0xFFFF for op in fwd]
    assert kf.count(N.OP_SPP_FWD) == 1 and [op.kind & 0xFFFF for op in bwd].count(N.OP_SPP_BWD) == 1
    i = kf.index(N.OP_SPP_FWD)
    convs = [j for j, k in enumerate(kf) if N.OP_NAMES[k].startswith(("conv_", "pw_"))]
    assert convs and min(convs) < i < max(convs), [N.OP_NAMES[k] for k in kf]
    (f,), (g,) = _of(fwd, N.OP_SPP_FWD), _of(bwd, N.OP_SPP_BWD)
    B, _, H, W = SU.CHAIN_SHAPE
    assert list(f.i[:10]) == [16, 48, B, H, W, 16, 5, 3, 0, N.VT_F32]
    assert list(g.i[3:11]) == [B, H, W, 16, 5, 3, 0, N.VT_F32]


def test_builder_spp_writes_into_a_given_slice_and_accumulates_for_a_second_consumer():
    b = E.Builder(E.ParamStore(nn.Identity()), N.VT_BF16, True, True)
    x = b.act(2, 6, 6, 16, "x")
    wide = b.act(2, 6, 6, 64, "wide")
    y = b.spp(x, 5, 3, "max", out=wide.sl(16, 48))
    assert y.ld == 64 and y.coff == 16 and y.C == 48
    (f,) = _of(b.fwd, N.OP_SPP_FWD)
    assert list(f.i[:2]) == [16, 64] and f.ptr[1].offset == wide.buf.offset + 16 * 2
    y2 = b.spp(x, 3, 2, "avg")
    b.seed_output_grads([y, y2])
    b.build_backward()
    g = _of(b.bwd, N.OP_SPP_BWD)
    assert [op.i[2] for op in g] == [0, 1]  # the first writer of d(x) writes, the second adds
    assert g[0].ptr[2].offset == g[1].ptr[2].offset and g[0].ptr[1].base == -1 and g[1].ptr[1].base == E.ARENA


# ---- refusals, by name ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,repeats", [(7, 3), (11, 2), (3, 5), (17, 1)])
def test_unsupported_geometry_is_refused_by_name(k, repeats):
    """halo 9, halo 10, five stages, a window whose taps do not fit a byte.  (5, 4) has the halo of (9, 2), 8, and therefore runs: test_spp_kernels_gpu.py checks it)"""
    with pytest.raises(NotImplementedError, match=rf"k={k} and repeats={repeats}"):
        _program(SPPBlock(k, repeats), (1, 8, 9, 9))
    b = E.Builder(E.ParamStore(nn.Identity()), N.VT_F32, False, False)
    with pytest.raises(NotImplementedError, match=rf"k={k} and repeats={repeats}"):
        b.spp(b.act(1, 9, 9, 8, "x"), k, repeats, "max")


def test_other_refusals():
    b = E.Builder(E.ParamStore(nn.Identity()), N.VT_BF16, False, False)
    with pytest.raises(KeyError):
        b.spp(b.act(1, 9, 9, 8, "x"), 5, 3, "median")
    with pytest.raises(NotImplementedError, match="12 channels"):
        b.spp(b.act(1, 9, 9, 12, "x"), 5, 3, "max")
    with pytest.raises(NotImplementedError, match="3 channels"):  # an image padded to a chunk: the concat would hold padding
        _program(SPPBlock(), (1, 3, 9, 9))
    with pytest.raises(NotImplementedError, match="square"):
        m = SPPBlock()
        m.pool = nn.MaxPool2d((3, 5), 1, (1, 2))
        _program(m, (1, 8, 9, 9))
