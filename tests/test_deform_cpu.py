"""DeformableConv2d without a GPU: the module's surface (children, state_dict keys, initialisation, the mask_act fallback),
the float64 restatement of tests/deform_util.py against a second form and against convolutions, the eager CPU path and its
autograd against the restatement, the launch lists compiled on the CPU, every refusal, and the exported symbols.  There is
no fixture of the reference: torchvision is not installed, so its class cannot be imported (tests/deform_util.py)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import deform_util as DU
from vision_toolbox import _native as N
from vision_toolbox import components
from vision_toolbox import engine as E
from vision_toolbox.components import DeformableConv2d, DeformConv2d, HipModule


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- the module's surface -------------------------------------------------------------------------------------------------
def test_children_state_dict_and_initialisation():
    torch.manual_seed(0)
    m = DeformableConv2d(16, 24, 3, stride=2, padding=1, dilation=1)
    assert isinstance(m, HipModule) and isinstance(m.conv, DeformConv2d)
    assert list(m.state_dict().keys()) == ["conv_offset.weight", "conv_offset.bias", "conv_mask.0.weight", "conv_mask.0.bias",
                                           "conv.weight", "conv.bias"]
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"conv_offset.weight": (18, 16, 3, 3), "conv_offset.bias": (18,), "conv_mask.0.weight": (9, 16, 3, 3),
                      "conv_mask.0.bias": (9,), "conv.weight": (24, 16, 3, 3), "conv.bias": (24,)}
    for c in (m.conv_offset, m.conv_mask[0]):
        assert (c.kernel_size, c.stride, c.padding, c.dilation) == ((3, 3), (2, 2), (1, 1), (1, 1))
    assert isinstance(m.conv_mask[1], nn.Sigmoid)
    # torchvision's initialisation: kaiming_uniform_(a=sqrt(5)) is U(+-1/sqrt(fan_in)), and so is the bias
    bound = 1 / math.sqrt(16 * 9)
    w, b = m.conv.weight.detach(), m.conv.bias.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.95 * bound and abs(float(w.mean())) < 0.1 * bound
    assert float(b.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / math.sqrt(3), rel=0.05)
    g = DeformableConv2d(16, 24, 3, groups=2, bias=False)
    assert tuple(g.conv.weight.shape) == (24, 8, 3, 3) and g.conv.bias is None and "conv.bias" not in g.state_dict()
    assert tuple(DeformableConv2d(8, 8, (3, 1)).conv_offset.weight.shape) == (6, 8, 3, 1)


def test_mask_act_fallback_v1_and_mask_init_bias():
    assert isinstance(DeformableConv2d(8, 8, 3).conv_mask[1], nn.Sigmoid)  # nn.Sigmoid(inplace=True) is a TypeError
    relu = DeformableConv2d(8, 8, 3, mask_act=nn.ReLU).conv_mask[1]
    assert isinstance(relu, nn.ReLU) and relu.inplace  # an activation that takes `inplace` gets it, as in the reference
    assert isinstance(DeformableConv2d(8, 8, 3, mask_act=nn.Identity).conv_mask[1], nn.Identity)
    v1 = DeformableConv2d(8, 8, 3, v2=False)
    assert v1.conv_mask is None and list(v1.state_dict().keys()) == ["conv_offset.weight", "conv_offset.bias", "conv.weight",
                                                                      "conv.bias"]
    torch.manual_seed(1)
    a = DeformableConv2d(8, 8, 3, mask_init_bias=0)
    torch.manual_seed(1)
    b = DeformableConv2d(8, 8, 3, mask_init_bias=5.0)  # accepted and unused, as in the reference
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))


def test_defined_in_components_but_not_listed():
    """tests/test_spp_cpu.py pins `"DeformableConv2d" not in components.__all__`: the class is importable by name only"""
    assert components.DeformableConv2d is DeformableConv2d and "DeformableConv2d" not in components.__all__
    assert "DeformableConv2d" in components.__doc__


# ---- the restatement ---------------------------------------------------------------------------------------------------------
GEOMETRIES = [(2, 6, 9, 9, 8, 3, 1, 1, 1, 1.5), (1, 4, 7, 10, 6, 3, 2, 1, 1, 3.0), (2, 4, 5, 5, 4, 3, 1, 2, 2, 4.0)]


def _case(geo, groups=1, seed=0):
    B, C, H, W, Co, k, s, p, d, std = geo
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = DU.out_size(H, W, k, s, p, d)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    leaves = [rnd(B, C, H, W), rnd(B, 2 * k * k, Ho, Wo) * std, rnd(B, k * k, Ho, Wo), rnd(Co, C // groups, k, k), rnd(Co)]
    return [t.requires_grad_(True) for t in leaves], rnd(B, Co, Ho, Wo)


def _all(y, r, leaves):
    return [y.detach()] + list(torch.autograd.grad((y * r).sum(), leaves))


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_restatement_equals_the_grid_sample_form(geo):
    s, p, d = geo[6:9]
    leaves, r = _case(geo)
    x, off, logit, w, b = leaves
    assert DU.outside_fraction(off.detach(), geo[2], geo[3], geo[5], s, p, d) >= 0.10
    a = _all(DU.deform_conv2d_ref(x, off, torch.sigmoid(logit), w, b, s, p, d), r, leaves)
    c = _all(DU.deform_conv2d_ref(x, off, torch.sigmoid(logit), w, b, s, p, d, form=DU.columns_grid_sample), r, leaves)
    for name, u, v in zip(("y", "dx", "doffset", "dmask", "dw", "db"), a, c):
        assert rel(u, v) < 1e-12, name


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_zero_offsets_are_a_convolution_and_unit_offsets_a_shifted_one(geo):
    B, C, H, W, Co, k, s, p, d, _ = geo
    (x, off, logit, w, b), r = _case(geo)
    zero = torch.zeros_like(off)
    assert rel(DU.deform_conv2d_ref(x, zero, None, w, b, s, p, d).detach(), F.conv2d(x, w, b, s, p, d).detach()) < 1e-13
    # offsets of exactly +1.0: every tap reads one pixel further down and right, i.e. the convolution over the image shifted
    # up and left by one: a zero border of p - 1 at the near edges and p + 1 at the far ones
    want = F.conv2d(F.pad(x, (p - 1, p + 1, p - 1, p + 1)), w, b, s, 0, d)
    assert rel(DU.deform_conv2d_ref(x, zero + 1.0, None, w, b, s, p, d).detach(), want.detach()) < 1e-13
    assert rel(components.deform_conv2d(x, zero + 1.0, w, b, (s, s), (p, p), (d, d)).detach(), want.detach()) < 1e-13


# ---- the eager path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_eager_op_and_its_autograd_match_the_restatement(geo, groups):
    s, p, d = geo[6:9]
    leaves, r = _case(geo, groups)
    x, off, logit, w, b = leaves
    a = _all(DU.deform_conv2d_ref(x, off, torch.sigmoid(logit), w, b, s, p, d), r, leaves)
    c = _all(components.deform_conv2d(x, off, w, b, (s, s), (p, p), (d, d), torch.sigmoid(logit)), r, leaves)
    for name, u, v in zip(("y", "dx", "doffset", "dmask", "dw", "db"), a, c):
        assert rel(v, u) < 1e-12, name


@pytest.mark.parametrize("v2", [True, False])
def test_module_on_cpu_tensors_matches_the_restatement(v2):
    m = DU.init_module(DeformableConv2d(**DU.BLOCK_ARGS, v2=v2))
    x = DU.module_input(DU.BLOCK_SHAPE).requires_grad_(True)
    y = m(x)
    assert y.shape == (2, 24, 12, 12)
    r = DU.loss_weights(y.shape)
    (y * r).sum().backward()
    m64 = copy.deepcopy(m).double()
    m64.zero_grad()
    x64 = x.detach().double().requires_grad_(True)
    y64 = DU.model_ref(m64, x64)
    (y64 * r.double()).sum().backward()
    assert rel(y.detach(), y64.detach()) < 1e-5 and rel(x.grad, x64.grad) < 1e-4
    for (k, pa), (_, pb) in zip(m.named_parameters(), m64.named_parameters()):
        assert rel(pa.grad, pb.grad) < 1e-4, k
    # everything the GPU path refuses runs here: 5x5, stride 3, groups, a non-square kernel, another mask activation
    for kw in (dict(kernel_size=5, padding=2), dict(kernel_size=3, stride=3), dict(kernel_size=3, groups=2),
               dict(kernel_size=(3, 1), padding=(1, 0)), dict(kernel_size=3, mask_act=nn.Tanh)):
        out = DeformableConv2d(16, 16, **kw)(x.detach())
        assert out.shape[:2] == (2, 16) and torch.isfinite(out).all()


# ---- launch lists, compiled on the CPU -----------------------------------------------------------------------------------------
class Chain(HipModule):
    def __init__(self, children):
        super().__init__()
        for k, m in children.items():
            self.add_module(k, m)

    def _vt_emit_maps(self, b, x):
        h = self.cv1._vt_emit(b, x, name="cv1")
        h = self.dcn._vt_emit(b, h, name="dcn")
        return [self.cv2._vt_emit(b, h, name="cv2")]

    def _eager_maps(self, x):
        return [self.cv2(self.dcn(self.cv1(x)))]


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
    assert [N.OP_DEFORM_FWD, N.OP_DEFORM_BWD, N.OP_DEFORM_WGRAD] == [113, 114, 115] and N.OP_SPP_BWD == 112
    assert [N.OP_NAMES[k] for k in (113, 114, 115)] == ["deform_fwd", "deform_bwd", "deform_wgrad"]
    lib = N.lib()
    for sym in ("vt_deform_supported", "vt_deform_fwd", "vt_deform_bwd", "vt_deform_wgrad", "vt_deform_wgrad_scratch_bytes"):
        assert sym in N.SYMBOLS and getattr(lib, sym) is not None
    assert lib.vt_deform_supported(3, 1, 16, 24, N.VT_BF16) == 1 and lib.vt_deform_supported(1, 2, 12, 20, N.VT_F32) == 1
    assert lib.vt_deform_supported(5, 1, 16, 16, N.VT_BF16) == 0 and lib.vt_deform_supported(3, 3, 16, 16, N.VT_BF16) == 0
    assert lib.vt_deform_supported(3, 1, 12, 16, N.VT_BF16) == 0


@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("v2", [True, False])
def test_block_launch_list(v2, dtype):
    B, C, H, W = DU.BLOCK_SHAPE
    prog = _program(DeformableConv2d(**DU.BLOCK_ARGS, v2=v2), DU.BLOCK_SHAPE, dtype)
    fwd, bwd = _ops(prog)
    (f,), (g,), (wg,) = _of(fwd, N.OP_DEFORM_FWD), _of(bwd, N.OP_DEFORM_BWD), _of(bwd, N.OP_DEFORM_WGRAD)
    epc = 8 if dtype == N.VT_BF16 else 4
    ldo, ldm = E._round_up(18, epc), (E._round_up(9, epc) if v2 else 0)
    geom = [B, H, W, 16, 24, 3, 1, 1, 1, 1 if v2 else 0, dtype]
    # i: ldx ldo ldm ldy geometry | lddy ldx ldo ldm lddo lddm lddx accumulate geometry | lddy ldx ldo ldm geometry
    assert list(f.i[:15]) == [16, ldo, ldm, 24, *geom]
    assert list(g.i[:19]) == [24, 16, ldo, ldm, ldo, ldm, 16, 0, *geom]
    assert list(wg.i[:15]) == [24, 16, ldo, ldm, *geom]
    assert (f.ptr[2].base == -1) == (not v2) and (g.ptr[3].base == -1) == (not v2) and (g.ptr[6].base == -1) == (not v2)
    assert g.ptr[7].base == E.ARENA and g.ptr[8].base == E.ARENA  # d(x) and its f32 plane
    assert int(wg.f[0]) == N.lib().vt_deform_wgrad_scratch_bytes(B, H, W, 16, 24, 3, 1, 1, 1)
    # the offset / mask maps come from ordinary conv units, and their data gradients join d(x) after the scatter's flush
    assert prog.n_units == (2 if v2 else 1) and len(_of(fwd, N.OP_CONV_IGEMM)) == (2 if v2 else 1)
    kb = [op.kind & 0xFFFF for op in bwd]
    assert kb.index(N.OP_DEFORM_WGRAD) < kb.index(N.OP_DEFORM_BWD) < kb.index(N.OP_CONV_WGRAD)
    # the maps are wider than their logical channel counts: their gradients' padding channels are cleared before the launch
    memsets = [i for i, k in enumerate(kb) if k == N.OP_MEMSET and 0 < i < kb.index(N.OP_DEFORM_BWD)]
    assert len(memsets) == (2 if v2 else 1)


def test_inference_program_has_no_backward_and_reserved_rows_are_zero():
    m = DeformableConv2d(**DU.BLOCK_ARGS)
    prog = _program(m, DU.BLOCK_SHAPE, N.VT_BF16, need_grad=False, training=False)
    fwd, bwd = _ops(prog)
    assert len(_of(fwd, N.OP_DEFORM_FWD)) == 1 and not bwd
    # the 18 and 9 output channels run as 24 and 16: the rows beyond the parameters' own are zeros their slots reserve
    store = m._vt_runner().store
    for conv, rows in ((m.conv_offset, 24), (m.conv_mask[0], 16)):
        _, off, n = store.where(conv.weight)
        assert store.reserve[id(conv.weight)] == rows * 9 * 16 and store.reserve[id(conv.bias)] == rows
        assert float(store.pflat[off + n : off + rows * 9 * 16].abs().max()) == 0.0
        assert torch.equal(store.pflat[off : off + n].view(conv.out_channels, 3, 3, 16).permute(0, 3, 1, 2), conv.weight.data)


def test_chain_program_holds_the_block_between_the_two_units():
    m = DU.build_chain(components, Chain)
    prog = _program(m, DU.CHAIN_SHAPE, N.VT_F32)
    fwd, bwd = _ops(prog)
    assert prog.n_units == 4  # cv1, conv_offset, conv_mask.0, cv2
    kf = [op.kind & 0xFFFF for op in fwd]
    assert kf.count(N.OP_DEFORM_FWD) == 1 and [op.kind & 0xFFFF for op in bwd].count(N.OP_DEFORM_BWD) == 1
    (g,) = _of(bwd, N.OP_DEFORM_BWD)
    assert g.ptr[7].base == E.ARENA  # cv1's output needs a gradient: the scatter runs


def test_builder_deform_conv_writes_into_a_given_slice_and_accumulates_for_a_second_consumer():
    m = DeformableConv2d(16, 16, 3, padding=1)
    store = E.ParamStore(m)
    store.ensure(torch.device("cpu"))
    b = E.Builder(store, N.VT_BF16, True, True)
    x = b.act(2, 6, 6, 16, "x")
    wide = b.act(2, 6, 6, 64, "wide")
    y = m._vt_emit(b, x, out=wide.sl(16, 16))
    assert y.ld == 64 and y.coff == 16 and y.C == 16
    (f,) = _of(b.fwd, N.OP_DEFORM_FWD)
    assert f.i[3] == 64 and f.ptr[5].offset == wide.buf.offset + 16 * 2
    y2 = b.spp(x, 3, 1, "avg")
    b.seed_output_grads([y, y2])
    b.build_backward()
    (g,) = _of(b.bwd, N.OP_DEFORM_BWD)
    assert g.i[7] == 1  # the pooling block wrote d(x) first (backward runs in reverse): the flush accumulates


# ---- refusals, by name -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(kernel_size=5, padding=2), r"kernel_size=\(5, 5\)"), (dict(kernel_size=(3, 1)), r"kernel_size=\(3, 1\)"),
    (dict(kernel_size=3, stride=3), r"stride=\(3, 3\)"), (dict(kernel_size=3, stride=(1, 2)), r"stride=\(1, 2\)"),
    (dict(kernel_size=3, padding=(1, 2)), r"padding=\(1, 2\)"), (dict(kernel_size=3, dilation=(1, 2), padding=2), r"dilation=\(1, 2\)"),
    (dict(kernel_size=3, groups=2), "groups=2"), (dict(kernel_size=3, mask_act=nn.Tanh), "mask_act=Tanh"),
    (dict(kernel_size=3, conv_fn=lambda *a, **kw: nn.Sequential(nn.Conv2d(*a, **kw))), "conv_fn=Sequential"),
])
def test_unsupported_arguments_are_refused_by_name(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _program(DeformableConv2d(16, 16, **kw), (1, 16, 9, 9))


def test_other_refusals():
    with pytest.raises(NotImplementedError, match="conv_fn: conv_offset"):  # an nn.Conv2d of another geometry
        m = DeformableConv2d(16, 16, 3, padding=1)
        m.conv_offset = nn.Conv2d(16, 18, 3, padding=2)
        _program(m, (1, 16, 9, 9))
    with pytest.raises(NotImplementedError, match="out_channels=12"):
        _program(DeformableConv2d(16, 12, 3, padding=1), (1, 16, 9, 9), N.VT_BF16)
    with pytest.raises(NotImplementedError, match="in_channels=12"):
        _program(DeformableConv2d(12, 16, 3, padding=1), (1, 12, 9, 9), N.VT_BF16)
    with pytest.raises(NotImplementedError, match="in_channels=3"):  # an image whose channels were padded to a chunk
        _program(DeformableConv2d(3, 16, 3, padding=1), (1, 3, 9, 9))
    _program(DeformableConv2d(12, 20, 3, padding=1), (1, 12, 9, 9), N.VT_F32)  # whole f32 chunks
    m = DeformableConv2d(16, 16, 3, padding=1)
    store = E.ParamStore(m)
    store.ensure(torch.device("cpu"))
    b = E.Builder(store, N.VT_BF16, True, True, deterministic=True)
    with pytest.raises(NotImplementedError, match="deterministic"):
        m._vt_emit(b, b.act(1, 9, 9, 16, "x"))
