"""vt_sigmoid_bce through the C-ABI against the float64 yardstick of tests/bce_util.py: every shape, mix block, smoothing,
threshold and sum_classes setting of bce_util, both dtypes, logits and gradients as slices of NaN-filled buffers whose
surroundings must stay NaN, every launch twice with bit-identical loss and gradient.  Bounds are the counted ones of
bce_util (K_GRAD, K_LOSS; the bf16 store's 2^-8 on top).  Every test prints its worst error as a fraction of its bound."""
import pytest
import torch

from oracle import filler
from vision_toolbox import _native as N

import bce_util as BU
from gpu_util import DNAME, DTYPES, TD, stream, vp

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
assert (N.VT_F32, N.VT_BF16) == (BU.F32, BU.BF16)


def _bce(B, N_, dtype, x, y, s, gs, header, thr, sum_classes, with_grad=True, loss0=0.0):
    """one launch on logits with ldl = N + 3, dlogits with lddl = N + 5 and B + 2 row cells (NaN padding everywhere);
    returns (loss [1], dlogits [B, N])"""
    L, td = N.lib(), TD[dtype]
    xw = torch.full((B, N_ + 3), NAN, device="cuda", dtype=td)
    xw[:, :N_] = x.to("cuda", td)
    dw = torch.full((B, N_ + 5), NAN, device="cuda", dtype=td)
    loss = torch.full((4,), NAN, device="cuda")
    loss[0] = loss0
    rows = torch.full((B + 2,), NAN, device="cuda", dtype=torch.float64)
    yd = y.cuda()
    mix = None
    if header is not None:
        mix = torch.tensor([float(header[0]), header[1], 0, 0, 0, 0, 0, 0], device="cuda", dtype=torch.float32)
    flags = (N.VT_BCE_SUM_CLASSES if sum_classes else 0) | (N.VT_BCE_THRESHOLD if thr is not None else 0)
    N.check(L.vt_sigmoid_bce(vp(xw), N_ + 3, vp(yd), s, gs, vp(loss), vp(dw) if with_grad else None, N_ + 5, B, N_, dtype,
                             vp(mix), flags, 0.0 if thr is None else thr, vp(rows), stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(xw[:, N_:]).all() and torch.isnan(dw[:, N_:]).all()), "the padding was touched"
    assert bool(torch.isnan(loss[1:]).all() and torch.isnan(rows[B:]).all()), "wrote behind the loss cell or the row terms"
    if not with_grad:
        assert bool(torch.isnan(dw).all())
    return loss[:1].cpu(), dw[:, :N_].cpu(), rows[:B].cpu()


@DTYPE
@pytest.mark.parametrize("shape", BU.SHAPES, ids=str)
def test_sigmoid_bce_every_setting(shape, dtype):
    B, N_ = shape
    worst_g = worst_l = worst_r = 0.0
    for header, s, thr, sum_classes in BU.combos():
        assert BU.margin_ok(N_, header, s, thr)  # every value t can take lies more than 1e-3 from the threshold
        for gs in (1.0 / B, 3.0):
            c = BU.case(B, N_, dtype, header, s, thr, sum_classes, gs)
            loss, dl, rows = _bce(B, N_, dtype, c["x"], c["y"], s, gs, header, thr, sum_classes)
            loss2, dl2, rows2 = _bce(B, N_, dtype, c["x"], c["y"], s, gs, header, thr, sum_classes)
            assert torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(rows, rows2), "two runs differ"
            assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(loss).all()), (header, s, thr, sum_classes)
            lfrac = abs(loss.item() - c["loss"]) / c["loss_bound"]
            err = (dl.double() - c["grad"]).abs()
            gfrac = (err / c["grad_bound"]).max().item()
            worst_g, worst_l = max(worst_g, gfrac), max(worst_l, lfrac)
            assert lfrac <= 1.0 and gfrac <= 1.0, (header, s, thr, sum_classes, gs, lfrac, gfrac, loss.item(), c["loss"])
            # every row term against float64, with the row's own S: tight for the rows of ordinary logits
            rfrac = ((rows - c["rows"]).abs() / c["row_bounds"]).max().item()
            worst_r = max(worst_r, rfrac)
            assert rfrac <= 1.0, (header, s, thr, sum_classes, gs, rfrac)
            # the loss is the row terms added in ascending order in double
            total = 0.0
            for b in range(B):
                total += rows[b].item()
            D = B if sum_classes else B * N_
            assert loss.item() == torch.tensor(total * (1.0 / D), dtype=torch.float64).float().item()
    print(f"FRAC sigmoid_bce_grad {DNAME[dtype]} {shape} {worst_g:.4f}")
    print(f"FRAC sigmoid_bce_loss {DNAME[dtype]} {shape} {worst_l:.4f}")
    print(f"FRAC sigmoid_bce_rows {DNAME[dtype]} {shape} {worst_r:.4f}")


@DTYPE
def test_sigmoid_bce_bad_labels_poison_the_loss_and_nothing_else(dtype):
    B, N_ = 4, 10
    x = (filler.tensor("bce.bad", (B, N_)) * 3).to(TD[dtype]).float()
    good = filler.labels(B, N_)
    for row, value, header in ((0, N_, None), (0, -1, (0, 1.0)), (0, N_, (1, 0.3)), (1, N_ + 5, (1, 0.3)), (1, -2, (2, 0.5)),
                               (3, 1 << 40, None), (2, -(1 << 62), (1, 0.3))):
        y = good.clone()
        y[row] = value
        for thr in BU.THRESHOLDS:
            loss, dl, rows = _bce(B, N_, dtype, x, y, 0.1, 1.0 / B, header, thr, False)
            assert bool(torch.isnan(loss).all()), (row, value, header)
            assert bool(torch.isfinite(dl).all()), (row, value, header)
            # the row itself, and with a mixing header the row whose partner it is
            bad = {row} | ({(row + 1) % B} if header is not None and header[0] != 0 else set())
            assert {b for b in range(B) if torch.isnan(rows[b])} == bad


@DTYPE
def test_sigmoid_bce_adds_to_the_loss_cell_and_runs_without_a_gradient(dtype):
    B, N_ = 5, 1000
    for header in (None, (1, 0.3)):
        c = BU.case(B, N_, dtype, header, 0.1, None, False, 1.0 / B)
        base, _, _ = _bce(B, N_, dtype, c["x"], c["y"], 0.1, 1.0 / B, header, None, False)
        without, _, _ = _bce(B, N_, dtype, c["x"], c["y"], 0.1, 1.0 / B, header, None, False, with_grad=False)
        assert torch.equal(base, without)
        added, _, _ = _bce(B, N_, dtype, c["x"], c["y"], 0.1, 1.0 / B, header, None, False, loss0=2.0)
        assert added.item() == (torch.tensor(2.0) + base).item()


def test_sigmoid_bce_refuses_bad_arguments():
    L = N.lib()
    x = torch.zeros(2, 8, device="cuda")
    y = torch.zeros(2, dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, device="cuda")
    rows = torch.zeros(3, dtype=torch.float64, device="cuda")
    call = lambda **kw: L.vt_sigmoid_bce(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("x", vp(x)), ("ldl", 8), ("y", vp(y)), ("s", 0.1), ("gs", 0.5), ("loss", vp(loss)), ("dl", None), ("lddl", 8), ("B", 2),
        ("N", 8), ("dtype", N.VT_F32), ("mix", None), ("flags", 0), ("thr", 0.0), ("rows", vp(rows)), ("stream", stream()))])
    assert call() == N.VT_OK
    assert call(ldl=7) == N.VT_ERR_INVALID and call(rows=None) == N.VT_ERR_INVALID and call(flags=4) == N.VT_ERR_INVALID
    assert call(dl=vp(x), lddl=7) == N.VT_ERR_INVALID and call(s=1.5) == N.VT_ERR_INVALID
    assert call(flags=N.VT_BCE_THRESHOLD, thr=NAN) == N.VT_ERR_INVALID
    assert call(rows=__import__("ctypes").c_void_p(rows.data_ptr() + 4)) == N.VT_ERR_INVALID
    assert call(dtype=7) == N.VT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
