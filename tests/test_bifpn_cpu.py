"""BiFPN / SeparableConv2d without a GPU: the state_dict contract and the eager path against fixtures of the unmodified
reference (tools/gen_golden_bifpn.py, `block=ConvNormAct` -- the only block the reference's BiFPN can be built with), the
restatement of tests/bifpn_util.py against the same fixtures (which ties it to the reference), the default separable block
against that restatement, the launch lists compiled on the CPU, and every refusal by name.

Bounds: those of tests/test_necks.py on the CPU -- relative L2 below 1e-6 for the maps and running statistics, 1e-5 for
every gradient."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bifpn_util as BU
from vision_toolbox import _native as N
from vision_toolbox import engine as E
from vision_toolbox import necks
from vision_toolbox.components import ConvNormAct, SeparableConv2d
from vision_toolbox.necks import BiFPN, BiFPNLayer, WeightedFeatureFusion

CASES = list(BU.CASES)


@pytest.fixture(scope="module")
def gold():
    out = {}
    for c in CASES:
        out.update(BU.load_fixture(c))
    return out


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _module(case, block=ConvNormAct, **kw):
    ins, outc, _, layers = BU.CASES[case]
    m = BiFPN(list(ins), outc, num_layers=layers, block=block, **kw)
    BU.fill(m, f"bifpn_{case}.", case)
    return m


def _check_against_fixture(gold, case, mode, ys, dxs, grads, state):
    name = f"bifpn_{case}"
    for i, y in enumerate(ys):
        assert rel(y, gold[f"{name}/{mode}/y{i}"]) < 1e-6, i
    for i, dx in enumerate(dxs):
        assert rel(dx, gold[f"{name}/{mode}/dx{i}"]) < 1e-5, i
    want = {k[len(f"{name}/{mode}/grad/"):] for k in gold if k.startswith(f"{name}/{mode}/grad/")}
    assert set(grads) == want
    for k, g in grads.items():
        assert rel(g, gold[f"{name}/{mode}/grad/{k}"]) < 1e-5, k
    if mode == "train":
        for k, v in state.items():
            assert rel(v, gold[f"{name}/train/state/{k}"]) < 1e-6, k


# ---- the reference's contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(gold, case):
    sd = _module(case).state_dict()
    assert list(sd.keys()) == list(gold[f"bifpn_{case}/keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(gold[f"bifpn_{case}/shapes"])
    assert float(gold[f"bifpn_{case}/min_weight_sum"]) >= BU.MIN_WEIGHT_SUM
    assert "BiFPN" in necks.__all__ and "SeparableConv2d" in __import__("vision_toolbox.components").components.__all__


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", CASES)
def test_eager_path_matches_the_reference_fixtures(gold, case, mode):
    m = _module(case).train(mode == "train")
    xs = BU.inputs(case)
    ys = m(xs)  # CPU tensors: the eager path
    BU.loss(case, ys).backward()
    state = {k: v for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    _check_against_fixture(gold, case, mode, [y.detach() for y in ys], [x.grad for x in xs],
                           {k: p.grad for k, p in m.named_parameters()}, state)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_fixtures(gold, case, mode):
    ref = BU.make_ref(case, "cna", f"bifpn_{case}.", case, dtype=torch.float32)
    assert list(ref.state_dict().keys()) == list(gold[f"bifpn_{case}/keys"])
    ys, dxs, grads, scales, state = BU.run_ref(ref, case, mode == "train")
    _check_against_fixture(gold, case, mode, ys, dxs, grads, state)
    assert set(scales) == {k for k in grads if k.endswith(".weights")}
    for k, s in scales.items():  # S_i bounds the gradient it scales: |d w_i| <= S_i
        assert (grads[k].abs().double() <= s * (1 + 1e-6)).all(), k


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", CASES)
def test_default_block_matches_the_separable_restatement(case, mode):
    m = _module(case, block=SeparableConv2d).train(mode == "train")
    ref = BU.make_ref(case, "sep", f"bifpn_{case}.", case, dtype=torch.float32)
    assert list(ref.state_dict().keys()) == list(m.state_dict().keys())
    for (k, a), b in zip(m.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k
    rys, rdxs, rgrads, _, rstate = BU.run_ref(ref, case, mode == "train")
    xs = BU.inputs(case)
    ys = m(xs)
    BU.loss(case, ys).backward()
    for y, r in zip(ys, rys):
        assert rel(y.detach(), r) < 1e-6
    for x, r in zip(xs, rdxs):
        assert rel(x.grad, r) < 1e-5
    for k, p in m.named_parameters():
        assert rel(p.grad, rgrads[k]) < 1e-5, k
    if mode == "train":
        for k, v in rstate.items():
            assert rel(m.state_dict()[k], v) < 1e-6, k


def test_default_block_is_separable_and_the_small_modules_run_alone():
    m = BiFPN([8, 16], 8)
    assert isinstance(m.layers[0].td_fuses[0].conv, SeparableConv2d)
    layer = BiFPNLayer(3, 8)
    outs = layer([torch.randn(1, 8, s, s) for s in (8, 4, 2)])
    assert [tuple(o.shape) for o in outs] == [(1, 8, s, s) for s in (8, 4, 2)]
    node = WeightedFeatureFusion(8, num_inputs=3)
    assert tuple(node([torch.randn(1, 8, 4, 4) for _ in range(3)]).shape) == (1, 8, 4, 4)


# ---- SeparableConv2d ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,stride", [(8, 16, 3, 1), (16, 8, 5, 2)])
def test_separable_conv2d(cin, cout, k, stride):
    m = SeparableConv2d(cin, cout, kernel_size=k, stride=stride, padding=(k - 1) // 2)
    assert list(m.state_dict().keys()) == [f"{u}.{s}" for u in ("dw", "pw") for s in
                                           ("conv.weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var",
                                            "norm.num_batches_tracked")]
    assert sum(p.numel() for p in m.parameters()) == cin * k * k + 2 * cin + cin * cout + 2 * cout
    assert isinstance(m.dw.act, nn.ReLU6) and isinstance(m.pw.act, nn.ReLU6) and m.dw.conv.bias is None and m.pw.conv.bias is None
    BU.filler.fill_module(m, "sep.")
    m.eval()
    x = BU.filler.tensor("sep.x", (2, cin, 9, 9))
    sd = m.state_dict()
    h = F.conv2d(x, sd["dw.conv.weight"], None, stride, (k - 1) // 2, 1, cin)
    h = F.relu6(F.batch_norm(h, sd["dw.norm.running_mean"], sd["dw.norm.running_var"], sd["dw.norm.weight"], sd["dw.norm.bias"]))
    h = F.conv2d(h, sd["pw.conv.weight"])
    h = F.relu6(F.batch_norm(h, sd["pw.norm.running_mean"], sd["pw.norm.running_var"], sd["pw.norm.weight"], sd["pw.norm.bias"]))
    assert rel(m(x).detach(), h) < 1e-6
    # torch's default Conv2d initialisation (kaiming_uniform(a = sqrt 5)): |w| <= 1 / sqrt(fan_in)
    fresh = SeparableConv2d(cin, cout, kernel_size=k, padding=(k - 1) // 2)
    assert fresh.dw.conv.weight.abs().max() <= 1 / k + 1e-6 and fresh.pw.conv.weight.abs().max() <= cin ** -0.5 + 1e-6


# ---- launch lists, compiled on the CPU ---------------------------------------------------------------------------------
def _program(m, shapes, dtype=N.VT_F32, need_grad=True, training=True):
    m.train(training)
    r = necks._NeckRunner(m)
    r.store.ensure(torch.device("cpu"))
    return r.program([torch.zeros(*s, requires_grad=need_grad) for s in shapes], dtype, need_grad)


def _ops(prog):
    return list(prog.fwd_ops)[: prog.n_fwd], list(prog.bwd_ops)[: prog.n_bwd]


def _shapes(case):
    ins, _, sizes, _ = BU.CASES[case]
    return [(BU.BATCH, c, s, s) for c, s in zip(ins, sizes)]


def test_new_op_codes_are_appended():
    assert [N.OP_WFUSE_FWD, N.OP_WFUSE_BWD, N.OP_WFUSE_FIN] == [108, 109, 110] and N.OP_BN_ACT_AVGPOOL_FIN_APPLY == 107
    assert [N.OP_NAMES[k] for k in (108, 109, 110)] == ["wfuse_fwd", "wfuse_bwd", "wfuse_fin"]
    for sym in ("vt_wfuse_fwd", "vt_wfuse_bwd", "vt_wfuse_finalize"):
        assert sym in N.SYMBOLS


@pytest.mark.parametrize("block", [ConvNormAct, SeparableConv2d], ids=["cna", "sep"])
@pytest.mark.parametrize("dtype", [N.VT_F32, N.VT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_one_fusion_launch_per_node_and_no_resampling_launch(case, dtype, block):
    ins, _, _, layers = BU.CASES[case]
    nodes = 2 * layers * (len(ins) - 1)
    fwd, bwd = _ops(_program(_module(case, block=block), _shapes(case), dtype))
    kf, kb = [op.kind & 0xFFFF for op in fwd], [op.kind & 0xFFFF for op in bwd]
    assert kf.count(N.OP_WFUSE_FWD) == nodes
    assert kb.count(N.OP_WFUSE_BWD) == nodes and kb.count(N.OP_WFUSE_FIN) == nodes
    assert not {N.OP_RESAMPLE_FWD, N.OP_RESAMPLE_BWD} & (set(kf) | set(kb))
    if block is SeparableConv2d:  # the tiled depthwise unit, one per node
        assert kf.count(N.OP_DWT_FWD) == nodes and kb.count(N.OP_DWT_BWD) == nodes
    # inference: the same forward nodes, no backward list
    fwd, bwd = _ops(_program(_module(case, block=block), _shapes(case), dtype, need_grad=False, training=False))
    assert [op.kind & 0xFFFF for op in fwd].count(N.OP_WFUSE_FWD) == nodes and not bwd


def test_accumulate_flags_of_a_three_consumer_map():
    """case a, one layer over three levels: the top-down map of the middle level feeds td_fuses.1 (upsampled, code 1),
    out_fuses.0 (code 0) and last_out_fuse (subsampled, code 2).  Backward meets them in the reverse order: the first writer
    initialises the gradient (accumulate 0 -- with code 2 it also zeroes the pixels nobody reads), the other two accumulate."""
    _, bwd = _ops(_program(_module("a"), _shapes("a")))
    writers = {}
    for op in bwd:
        if op.kind & 0xFFFF != N.OP_WFUSE_BWD:
            continue
        n = op.i[0]
        for k in range(n):
            if op.ptr[5 + k].base >= 0:
                writers.setdefault((op.ptr[5 + k].base, op.ptr[5 + k].offset), []).append((op.i[5 + k], op.i[11 + k]))
    three = [w for w in writers.values() if len(w) == 3]
    assert len(three) == 1 and three[0] == [(2, 0), (0, 1), (1, 1)]  # (code, accumulate) in backward order
    # every gradient buffer is initialised by its first writer and accumulated into by the others
    for w in writers.values():
        assert [acc for _, acc in w][1:] == [1] * (len(w) - 1)


def test_bilinear_materialises_the_resampled_maps():
    m = _module("a", interpolation_mode="bilinear")
    fwd, bwd = _ops(_program(m, _shapes("a")))
    kf = [op.kind & 0xFFFF for op in fwd]
    assert kf.count(N.OP_RESAMPLE_FWD) == 4 and kf.count(N.OP_WFUSE_FWD) == 4  # two x2 and two x0.5 maps per layer
    assert all(list(op.i[4:7]) == [0, 0, 0] for op in fwd if op.kind & 0xFFFF == N.OP_WFUSE_FWD)
    assert [op.kind & 0xFFFF for op in bwd].count(N.OP_RESAMPLE_BWD) == 4


# ---- refusals, by name -------------------------------------------------------------------------------------------------
def _builder(dtype=N.VT_F32):
    w = nn.Module()
    w.w2, w.w3, w.w4 = nn.Parameter(torch.ones(2)), nn.Parameter(torch.ones(3)), nn.Parameter(torch.ones(4))
    return E.Builder(E.ParamStore(w), dtype, True, True), w


def test_weighted_fuse_refusals():
    b, w = _builder()
    x = [b.act(2, 8, 8, 8, f"x{i}") for i in range(4)]
    with pytest.raises(NotImplementedError, match="fz: weighted_fuse takes 2 or 3 inputs"):
        b.weighted_fuse(x[:1], [0], w.w2, 1e-4, "fz")
    with pytest.raises(NotImplementedError, match="fz: weighted_fuse takes 2 or 3 inputs"):
        b.weighted_fuse(x, [0, 0, 0, 0], w.w4, 1e-4, "fz")
    with pytest.raises(NotImplementedError, match="resample codes"):
        b.weighted_fuse(x[:2], [0, 3], w.w2, 1e-4, "fz")
    with pytest.raises(ValueError, match="fz: 2 inputs but 3 fusion weights"):
        b.weighted_fuse(x[:2], [0, 0], w.w3, 1e-4, "fz")
    with pytest.raises(ValueError, match="fz: .*exact factor 2 apart"):  # 8x8 beside an upsampled 5x5
        b.weighted_fuse([x[0], b.act(2, 5, 5, 8, "small")], [0, 1], w.w2, 1e-4, "fz")
    with pytest.raises(ValueError, match="exact factor 2 apart"):  # 8x8 beside a subsampled 12x12
        b.weighted_fuse([x[0], b.act(2, 12, 12, 8, "large")], [0, 2], w.w2, 1e-4, "fz")
    with pytest.raises(NotImplementedError, match="fz: x0.5 resampling of an odd-sized map"):
        b.weighted_fuse([b.act(2, 3, 3, 8, "top"), b.act(2, 7, 7, 8, "odd")], [0, 2], w.w2, 1e-4, "fz")
    with pytest.raises(ValueError, match="fz: the same map is fused twice"):
        b.weighted_fuse([x[0], x[0]], [0, 0], w.w2, 1e-4, "fz")
    with pytest.raises(NotImplementedError, match="fz: 12 channels must be a multiple of 8"):
        bb, w16 = _builder(N.VT_BF16)
        bb.weighted_fuse([bb.act(2, 4, 4, 12, "a"), bb.act(2, 4, 4, 12, "b")], [0, 0], w16.w2, 1e-4, "fz")
    with pytest.raises(NotImplementedError, match="fz: 6 channels must be a multiple of 4"):
        b.weighted_fuse([b.act(2, 4, 4, 6, "a"), b.act(2, 4, 4, 6, "b")], [0, 0], w.w2, 1e-4, "fz")


def test_separable_conv2d_refusals():
    def program(mod, c=8):
        r = mod._vt_runner()
        r.store.ensure(torch.device("cpu"))
        return r.program(torch.zeros(2, c, 8, 8), N.VT_F32, True, True)

    with pytest.raises(NotImplementedError, match=r"sep\.dw: activation GELU.*Identity, ReLU, SiLU, ReLU6 and Hardswish"):
        program(SeparableConv2d(8, 8, act_fn=nn.GELU))
    with pytest.raises(NotImplementedError, match=r"sep\.dw: kernel_size=7"):  # depthwise_unit's own message
        program(SeparableConv2d(8, 8, kernel_size=7, padding=3))
    with pytest.raises(NotImplementedError, match=r"sep\.dw: .*dilation=2"):
        program(SeparableConv2d(8, 8, padding=2, dilation=2))
    for act in (nn.Identity, nn.ReLU, nn.SiLU, nn.ReLU6, nn.Hardswish):  # ... and the five codes compile
        program(SeparableConv2d(8, 16, act_fn=act))


def test_bifpn_refusals():
    shapes = _shapes("c")
    with pytest.raises(NotImplementedError, match=r"bifpn\.layers\.0\.td_fuses\.0\.conv: block Conv2d"):
        _program(BiFPN([8, 16], 8, block=lambda a, b: nn.Conv2d(a, b, 3, padding=1)), shapes)
    with pytest.raises(NotImplementedError, match="interpolation_mode='bicubic'"):
        _program(BiFPN([8, 16], 8, interpolation_mode="bicubic"), shapes)
    with pytest.raises(ValueError, match="BiFPN: 1 feature maps for 2 lateral convs"):
        _program(BiFPN([8, 16], 8), shapes[:1])
    with pytest.raises(ValueError, match="exact factor 2 apart"):  # torch's add would raise as well
        _program(BiFPN([8, 16], 8), [(2, 8, 8, 8), (2, 16, 3, 3)])
    with pytest.raises(ValueError, match="exact factor 2 apart"):  # (7 -> 3: the top-down add of 7 and 6 comes first)
        _program(BiFPN([8, 16], 8), [(2, 8, 7, 7), (2, 16, 3, 3)])
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _program(BiFPN([8, 16], 6), shapes)
    # FPN / PAN keep refusing every block but ConvNormAct
    with pytest.raises(NotImplementedError, match="neck blocks other than ConvNormAct"):
        _program(necks.FPN([8, 16], 8, block=SeparableConv2d), shapes)
