"""SPPBlock on CUDA tensors against fixtures of the unmodified reference (tools/gen_golden_spp.py, tests/spp_util.py).

Cases a-d, the block alone.  The fixtures' inputs hold bf16 values, so both dtypes pool the very same numbers: y of a max
case is EQUAL to the fixture in f32 and in bf16; everything else -- y of the avg case, every dx -- is within
gpu_util.tol (2e-5 f32, 6e-3 bf16, relative L2; the bf16 path rounds every stage it stores, the seed gradient and dx).

The chain ConvNormAct(8, 16, 1) -> SPPBlock() -> ConvNormAct(48, 16, 1) in training mode, compiled as ONE program by a small
HipModule that chains the three `_vt_emit`s.  f32: the bounds tests/test_modules_gpu.py applies to ConvNormAct chains --
relative L2 2e-4 for y, 8e-4 for dx and (clamped denominator) every parameter gradient, running statistics rtol = atol =
2e-3.  bf16: every quantity within twice the bf16 floor the fixture records for the reference itself (the rule of
tests/test_resnet_gpu.py / test_bifpn_gpu.py; the margin of 2 covers the different rounding points).  `cv1.norm.bias` has
a gradient that is zero in exact arithmetic (tools/gen_golden_spp.py): it is checked by magnitude against the gradient of
`cv1.norm.weight`, a sum of the same terms -- 2e-4 of its norm in f32 (the tolerance above), twice the magnitude the
reference's own bf16 run leaves there in bf16."""
import numpy as np
import pytest
import torch
from torch import nn

import spp_util as SU
from gpu_util import rel_err, tol
from vision_toolbox import _native as N
from vision_toolbox import components
from vision_toolbox.components import HipModule, SPPBlock

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, N.VT_F32), "bf16": (torch.bfloat16, N.VT_BF16)}


@pytest.fixture(scope="module")
def gold():
    return SU.load()


@pytest.fixture(autouse=True)
def _hip_path_ran():
    N.lib()
    before = N.launch_count()
    yield
    torch.cuda.synchronize()
    assert N.launch_count() > before, "no libvt_amd launch happened: the HIP path did not run"


def _t(a):
    return torch.from_numpy(np.asarray(a))


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


def _run_block(case, dtype):
    m = SU.build(components, case).cuda()
    m.compute_dtype = dtype
    x = SU.inputs(case, device="cuda")
    y = m(x)
    SU.loss(case, y).backward()
    return m, x, y


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(SU.CASES))
def test_block_vs_reference(gold, case, tag):
    dtype, code = DT[tag]
    m, x, y = _run_block(case, dtype)
    assert y.dtype == dtype and y.shape == tuple(gold[f"{case}/y"].shape)
    got, want = y.detach().float().cpu(), _t(gold[f"{case}/y"])
    if SU.CASES[case][0][2] == "max":
        assert torch.equal(got, want)
    else:
        err = rel_err(got, want)
        print(f"{case} {tag}: y rel {err:.2e} (bound {tol(code):.0e})")
        assert err < tol(code)
    err = rel_err(x.grad.float().cpu(), _t(gold[f"{case}/dx"]))
    print(f"{case} {tag}: dx rel {err:.2e} (bound {tol(code):.0e})")
    assert err < tol(code)
    # inference mode gives the same map, and a second training run the same bits
    with torch.no_grad():
        ye = m.eval()(x.detach())
    assert torch.equal(ye, y.detach())
    m.train()
    x2 = SU.inputs(case, device="cuda")
    y2 = m(x2)
    SU.loss(case, y2).backward()
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(x2.grad, x.grad)


def _run_chain(dtype):
    m = SU.build_chain(components, Chain)
    SU.fill(m)
    m = m.cuda().train()
    m.compute_dtype = dtype
    x = SU.inputs("chain", device="cuda")
    y = m(x)
    SU.loss("chain", y).backward()
    return m, x, y


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_chain_vs_reference(gold, tag):
    dtype, code = DT[tag]
    m, x, y = _run_chain(dtype)
    zero = set(gold["chain/zero_grad_keys"])
    assert zero == {"cv1.norm.bias"}
    got = {"y": y.detach(), "dx": x.grad, **{"grad/" + k: p.grad for k, p in m.named_parameters()}}
    assert set(got) == {k[len("chain/floor/f32/"):] for k in gold if k.startswith("chain/floor/f32/")}
    f32_bound = {"y": 2e-4}
    bad = []
    for k, v in got.items():
        v = v.float().cpu()
        if k[5:] in zero:
            scale = float(m.cv1.norm.weight.grad.norm())
            err, bound = float(v.abs().max()), (2e-4 * scale if tag == "f32" else 2 * float(gold[f"chain/floor/bf16/{k}"]))
        else:
            err = SU.gerr(v, _t(gold[f"chain/{k}"]))
            bound = f32_bound.get(k, 8e-4) if tag == "f32" else 2 * float(gold[f"chain/floor/bf16/{k}"])
        print(f"chain {tag} {k}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((k, err, bound))
    assert not bad, bad
    if tag == "f32":
        for k, v in m.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                np.testing.assert_allclose(v.cpu().numpy(), gold[f"chain/state/{k}"], rtol=2e-3, atol=2e-3, err_msg=k)
            elif k.endswith("num_batches_tracked"):
                assert int(v) == int(gold[f"chain/state/{k}"])
    # a second run of the chain: the same bits for the map and the data gradient
    m2, x2, y2 = _run_chain(dtype)
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(x2.grad, x.grad)
    # inference mode of the block inside the chain: the program has no backward list and the map follows the running statistics
    with torch.no_grad():
        ye = m.eval()(x.detach())
    assert ye.shape == y.shape and torch.isfinite(ye.float()).all()


def test_refusals_by_name():
    x = torch.zeros(1, 8, 9, 9, device="cuda")
    for k, repeats in ((7, 3), (11, 2), (3, 5), (17, 1)):
        with pytest.raises(NotImplementedError, match=rf"k={k} and repeats={repeats}"):
            SPPBlock(k, repeats).cuda()(x)
    with pytest.raises(RuntimeError, match="even kernel_size"):
        SPPBlock(4, 2).cuda()(x)
    with pytest.raises(NotImplementedError, match="3 channels"):
        SPPBlock().cuda()(torch.zeros(1, 3, 9, 9, device="cuda"))
    # four stages at the largest halo run
    y = SPPBlock(5, 4).cuda()(torch.relu(torch.randn(1, 8, 9, 9, device="cuda")))
    assert y.shape == (1, 32, 9, 9)
