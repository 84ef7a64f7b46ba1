"""DeformableConv2d on CUDA tensors against the float64 restatement of tests/deform_util.py (no reference fixture exists:
torchvision is not installed): the block alone, with and without the mask branch (v2), and inside the chain
ConvNormAct(8, 16, 1) -> DeformableConv2d(16, 24, 3, padding=1) -> ConvNormAct(24, 16, 1) in training mode, compiled as ONE
program by a small HipModule that chains the three `_vt_emit`s; batch 2 on 12 x 12 maps, both dtypes; the output, d(x) and
every parameter gradient.

f32: the bounds tests/test_modules_gpu.py applies to ConvNormAct chains -- relative L2 2e-4 for y, 8e-4 for dx and (clamped
denominator) every parameter gradient.  d(offset) is discontinuous where a sampling position crosses an integer, so the test
first asserts that no float64 sampling position of its seed lies within 1e-4 of one: a condition on the input, not on the code.
bf16: every quantity within twice the error of the restatement run in float64 with bf16 stores (image, filters, the offset map,
the mask logits, every stored z and y, and their gradients on the way back) against the plain float64 run -- the rule of
tests/test_resnet_gpu.py; it already prices the few floor cells that flip under rounded offsets.
Two runs give the same bits for the output and for the gradients of the deformable convolution's own filter and bias (the new
launches); d(x) leaves through float atomics and is compared by the bound.  In the chain, `dcn.conv.bias` feeds a training-mode
BatchNorm: its gradient is zero in exact arithmetic and is checked by magnitude (ZERO_GRADS).

Measured on an MI355X (relative L2, worst quantity): f32 1.3e-6 (y 8.4e-7); bf16 y 1.0e-2 and gradients 1.6e-3 .. 0.21, each
at 0.45 .. 0.52 of its bound, i.e. at the emulation's own error."""
import copy

import pytest
import torch
from torch import nn

import deform_util as DU
from vision_toolbox import _native as N
from vision_toolbox import components
from vision_toolbox.components import DeformableConv2d, HipModule

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(autouse=True)
def _hip_path_ran():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


class Chain(HipModule):
    """cv1 -> dcn -> cv2 as one compiled program: the three `_vt_emit`s chained"""

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


def _build(kind):
    if kind == "chain":
        return DU.init_module(DU.build_chain(components, Chain), DU.SEEDS[kind]).train(), DU.CHAIN_SHAPE
    return DU.init_module(DeformableConv2d(**DU.BLOCK_ARGS, v2=(kind == "v2")), DU.SEEDS[kind]).train(), DU.BLOCK_SHAPE


# a bias in front of a training-mode BatchNorm has a gradient that is zero in exact arithmetic: both sides hold rounding noise
# of the sums, and it is checked by magnitude against the gradient of the filter it belongs to (sums of the same terms)
ZERO_GRADS = {"chain": {"grad/dcn.conv.bias": "grad/dcn.conv.weight"}}


_REFS = {}


def _reference(kind):
    """float64 results of the restatement, plain and with bf16 stores; once per model, shared, never modified"""
    if kind not in _REFS:
        m, shape = _build(kind)
        m64 = copy.deepcopy(m).double()
        out = {}
        for emulate in (False, True):
            m64.zero_grad()
            x = DU.module_input(shape, DU.SEEDS[kind]).double().requires_grad_(True)
            y = DU.model_ref(m64, x, emulate_bf16=emulate)
            (y * DU.loss_weights(y.shape).double()).sum().backward()
            out["bf16" if emulate else "f64"] = {"y": y.detach(), "dx": x.grad, **{"grad/" + k: p.grad.clone() for k, p in m64.named_parameters()}}
        off, dcn = DU.offset_map(m64, DU.module_input(shape, DU.SEEDS[kind]).double())
        c = dcn.conv
        out["distance"] = DU.min_integer_distance(off.detach(), c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0])
        out["outside"] = DU.outside_fraction(off.detach(), *off.shape[-2:], c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0])
        _REFS[kind] = out
    return _REFS[kind]


def _run(kind, dtype):
    m, shape = _build(kind)
    m = m.cuda()
    m.compute_dtype = dtype
    x = DU.module_input(shape, DU.SEEDS[kind]).cuda().requires_grad_(True)
    y = m(x)
    (y.float() * DU.loss_weights(y.shape).cuda()).sum().backward()
    return m, {"y": y.detach(), "dx": x.grad, **{"grad/" + k: p.grad for k, p in m.named_parameters()}}


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["v2", "v1", "chain"])
def test_against_the_restatement(kind, tag):
    ref = _reference(kind)
    print(f"{kind}: nearest sampling position to an integer {ref['distance']:.2e}; {ref['outside']:.2f} of the samples outside")
    if tag == "f32":
        assert ref["distance"] > 1e-4, "the seed puts a float64 sampling position within 1e-4 of an integer: pick another"
    m, got = _run(kind, DT[tag])
    assert got["y"].dtype == DT[tag] and set(got) == set(ref["f64"])
    bad = []
    for k, v in got.items():
        if k in ZERO_GRADS.get(kind, {}):
            scale = float(ref["f64"][ZERO_GRADS[kind][k]].norm())
            assert float(ref["f64"][k].abs().max()) < 1e-9 * scale
            err = float(v.float().abs().max())
            bound = 8e-4 * scale if tag == "f32" else 2 * float(ref["bf16"][k].abs().max())
        else:
            err = DU.gerr(v.float().cpu(), ref["f64"][k])
            bound = (2e-4 if k == "y" else 8e-4) if tag == "f32" else 2 * DU.gerr(ref["bf16"][k], ref["f64"][k])
        print(f"{kind} {tag} {k}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((k, err, bound))
    assert not bad, bad
    # a second run: the same bits for what the new launches alone decide -- the output and the gradients of the deformable
    # convolution's own filter and bias; d(x) (float atomics) within the bound again.  (The other parameter gradients are not
    # claimed: the offset / mask units' column sums and filter gradients use float atomics outside deterministic mode, and
    # whatever lies upstream of d(x) inherits its last bits.)
    _, again = _run(kind, DT[tag])
    prefix = "grad/dcn." if kind == "chain" else "grad/"
    for k in ("y", prefix + "conv.weight", prefix + "conv.bias"):
        assert torch.equal(again[k], got[k]), k
    err = DU.gerr(again["dx"].float().cpu(), ref["f64"]["dx"])
    assert err < ((8e-4) if tag == "f32" else 2 * DU.gerr(ref["bf16"]["dx"], ref["f64"]["dx"]))
    # inference: no backward list, the same map for the block alone (the chain's BatchNorms switch to running statistics)
    with torch.no_grad():
        ye = m.eval()(DU.module_input(_build(kind)[1], DU.SEEDS[kind]).cuda())
    assert ye.shape == got["y"].shape and (kind == "chain" or torch.equal(ye, got["y"]))


def test_identity_mask_and_stride_two():
    """mask_act=nn.Identity and stride 2 with dilation 2 through the module (f32)"""
    m = DU.init_module(DeformableConv2d(8, 8, 3, stride=2, padding=2, dilation=2, mask_act=nn.Identity), DU.SEEDS["strided"]).train()
    m64 = copy.deepcopy(m).double()
    x = DU.module_input((2, 8, 11, 9), DU.SEEDS["strided"])
    x64 = x.double().requires_grad_(True)
    y64 = DU.model_ref(m64, x64)
    (y64 * DU.loss_weights(y64.shape).double()).sum().backward()
    off, _ = DU.offset_map(m64, x.double())
    assert DU.min_integer_distance(off.detach(), 3, 2, 2, 2) > 1e-4
    m = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    (y * DU.loss_weights(y.shape).cuda()).sum().backward()
    assert DU.gerr(y.detach().cpu(), y64.detach()) < 2e-4 and DU.gerr(xg.grad.cpu(), x64.grad) < 8e-4
    for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
        assert DU.gerr(p.grad.cpu(), q.grad) < 8e-4, k


def test_refusals_by_name():
    x = torch.zeros(1, 16, 9, 9, device="cuda")
    cases = [(dict(kernel_size=5, padding=2), "kernel_size"), (dict(kernel_size=3, stride=3), "stride"),
             (dict(kernel_size=3, groups=2), "groups"), (dict(kernel_size=(3, 1)), "kernel_size"),
             (dict(kernel_size=3, mask_act=nn.Tanh), "mask_act=Tanh"),
             (dict(kernel_size=3, conv_fn=lambda *a, **kw: nn.Sequential(nn.Conv2d(*a, **kw))), "conv_fn")]
    for kw, word in cases:
        with pytest.raises(NotImplementedError, match=word):
            DeformableConv2d(16, 16, **kw).cuda()(x)
    with pytest.raises(NotImplementedError, match="out_channels=12"):
        m = DeformableConv2d(16, 12, 3, padding=1).cuda()
        m.compute_dtype = torch.bfloat16
        m(x)
    with pytest.raises(NotImplementedError, match="in_channels=12"):
        m = DeformableConv2d(12, 16, 3, padding=1).cuda()
        m.compute_dtype = torch.bfloat16
        m(torch.zeros(1, 12, 9, 9, device="cuda"))
    y = DeformableConv2d(12, 20, 3, padding=1).cuda()(torch.randn(1, 12, 9, 9, device="cuda"))  # whole f32 chunks: runs in f32
    assert y.shape == (1, 20, 9, 9) and torch.isfinite(y).all()
