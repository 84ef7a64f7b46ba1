"""vt_augment_batch through the C-ABI against the float64 restatement (tests/augment_util.py) of the same uint8 bytes, and
GPUBatchTransform on top of it.

The ragged batch: noise images of (37, 53), (64, 48), (9, 7), (131, 97), (20, 20) and (300, 400).  Cases: whole images to
16 x 16 (down- and upsampling in one launch); to 24 x 24 with boxes at every corner and edge, a 1 x 1 crop, a 2 x 3 crop and
the (300, 400) image whole (a scale factor near 19); a non-square 16 x 24 output; flips on even and odd widths; the
validation geometry (resize 20, crop 16) on portrait, landscape and square sources; antialias off; mean / std; erase boxes;
and a 37 x 300 output, which takes several row bands and two column tiles per image.

Bounds: relative L2 within gpu_util.tol (2e-5, f32) and every element within 2e-5 of the reference's largest magnitude; the
same for the random erase against the numpy restatement of the generator.  Every case also runs with lds_bytes so low that
the LDS plane holds TWO source rows (a band of 16 output rows of a 37-row source then takes 19 chunks, every band of the
cases at least 3 wherever it reads 5 source rows or more): an output adds its taps in ascending row order whatever the
chunking, so the result must be torch.equal to the default plan's -- and it is asserted so.  Every launch runs twice and
must be bit-identical."""
import math

import numpy as np
import pytest
import torch

import augment_util as AU
from gpu_util import stream, tol, vp
from vision_toolbox import _native as N
from vision_toolbox import data as D

pytestmark = pytest.mark.gpu

IMAGES = AU.make_images()
MEAN_STD = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
_REF = {}


def lds_for_rows(Sh, Sw, rows):
    """lds_bytes at which the plane holds `rows` source rows: 16 bytes per column and row of a tile for the tables (tile:
    CW = min(S_w, 256) columns, R = min(S_h, 8 * min(256 // CW, 32)) rows), 12 * CW bytes per source row"""
    CW = min(Sw, 256)
    R = min(Sh, 8 * min(256 // CW, 32))
    return 16 * (CW + R) + 12 * CW * rows


def whole(i, Sh, Sw, **kw):
    H, W = AU.SIZES[i]
    return AU.row(0, 0, H, W, Sh, Sw, **kw)


def _cases():
    c = {}
    c["whole16"] = (list(range(6)), [whole(i, 16, 16) for i in range(6)], 16, 16, True, None)
    # corners and edges of the (37, 53) and (131, 97) images, then the special crops
    boxes = [(0, (0, 0, 20, 30)), (0, (0, 23, 20, 30)), (0, (17, 0, 20, 30)), (0, (17, 23, 20, 30)), (0, (0, 10, 37, 5)),
             (0, (30, 0, 7, 53)), (3, (0, 0, 100, 90)), (3, (31, 7, 100, 90)), (3, (130, 96, 1, 1)), (2, (4, 3, 1, 1)),
             (2, (3, 2, 2, 3)), (5, (0, 0, 300, 400)), (4, (0, 0, 20, 20))]
    c["boxes24"] = ([i for i, _ in boxes], [AU.row(*b, 24, 24) for _, b in boxes], 24, 24, True, None)
    c["nonsquare"] = (list(range(6)), [whole(i, 16, 24) for i in range(6)], 16, 24, True, None)
    c["flips"] = ([0, 1, 2, 4, 0, 1], [whole(0, 16, 24, flip=1), whole(1, 16, 24, flip=1), whole(2, 16, 24, flip=1),
                                        whole(4, 16, 24, flip=0), AU.row(3, 4, 30, 41, 16, 24, flip=1),
                                        AU.row(3, 4, 30, 40, 16, 24, flip=1)], 16, 24, True, None)
    c["flips_odd"] = ([0, 1, 2], [whole(0, 15, 17, flip=1), whole(1, 15, 17, flip=0), whole(2, 15, 17, flip=1)], 15, 17, True, None)
    ev = [0, 1, 4, 3]
    c["validation"] = (ev, D.eval_params([AU.SIZES[i] for i in ev], 20, 16).tolist(), 16, 16, True, None)
    c["bilinear"] = (list(range(6)), [whole(i, 24, 24, flip=i & 1) for i in range(6)], 24, 24, False, None)
    c["meanstd"] = (list(range(6)), [whole(i, 16, 24, flip=i & 1) for i in range(6)], 16, 24, True, MEAN_STD)
    c["bands"] = ([5, 0, 2], [whole(5, 37, 300), whole(0, 37, 300, flip=1), AU.row(1, 1, 7, 5, 37, 300)], 37, 300, True, None)
    E, K = D.ERASE_RANDOM, D.ERASE_CONSTANT
    c["erase"] = ([0, 1, 2, 3, 4, 5],
                  [whole(0, 16, 24), whole(1, 16, 24, erase=(0, 0, 15, 23), mode=E, seed=3),
                   whole(2, 16, 24, erase=(9, 13, 7, 11), mode=E, seed=-7, flip=1), whole(3, 16, 24, erase=(5, 6, 1, 1), mode=E, seed=5),
                   whole(4, 16, 24, erase=(1, 1, 15, 23), mode=E, seed=2**31 - 1), whole(5, 16, 24, erase=(3, 3, 0, 5), mode=E, seed=1)],
                  16, 24, True, MEAN_STD)
    return c


CASES = _cases()


def reference(name):
    if name not in _REF:
        idx, rows, Sh, Sw, aa, ms = CASES[name]
        _REF[name] = AU.reference_batch([IMAGES[i] for i in idx], AU.params_tensor(rows), Sh, Sw, aa, ms)
    return _REF[name]


def launch(images, rows, Sh, Sw, antialias=True, mean_std=None, lds=0, out=None, raw=None, twice=True):
    batch = D.RaggedBatch.from_images(images)
    raw = batch.raw.cuda() if raw is None else raw
    table, params = batch.table.cuda(), AU.params_tensor(rows).cuda()
    ms = torch.tensor(mean_std, dtype=torch.float32, device="cuda") if mean_std is not None else None
    B = len(images)
    if out is None:
        out = torch.full((B, 3, Sh, Sw), float("nan"), device="cuda")

    def run():
        N.check(N.lib().vt_augment_batch(vp(raw), vp(table), vp(params), vp(out), B, Sh, Sw, int(antialias), vp(ms), lds, stream()))
        torch.cuda.synchronize()
        return out.clone()

    first = run()
    if twice:
        assert torch.equal(run(), first), "two launches differ"
    return first.cpu()


def check(got, ref, what):
    assert torch.isfinite(got).all(), what
    l2, linf = AU.errors(got, ref)
    print(f"{what}: relative L2 {l2:.2e} (bound {tol(N.VT_F32):.0e}), largest element error / largest magnitude {linf:.2e} (bound 2e-05)")
    assert l2 <= tol(N.VT_F32) and linf <= 2e-5, (what, l2, linf)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_float64_restatement(name):
    idx, rows, Sh, Sw, aa, ms = CASES[name]
    images = [IMAGES[i] for i in idx]
    got = launch(images, rows, Sh, Sw, aa, ms)
    check(got, reference(name), name)
    low = launch(images, rows, Sh, Sw, aa, ms, lds=lds_for_rows(Sh, Sw, 2))
    assert torch.equal(low, got), "the chunked plan changed bits"
    one = launch(images, rows, Sh, Sw, aa, ms, lds=lds_for_rows(Sh, Sw, 1), twice=False)
    assert torch.equal(one, got), "the one-row plan changed bits"


def test_erase_constant_boxes_and_untouched_surroundings():
    Sh, Sw = 16, 24
    idx = [0, 1, 2, 3, 4]
    plain = launch([IMAGES[i] for i in idx], [whole(i, Sh, Sw) for i in idx], Sh, Sw)
    boxes = [(0, 0, 0, 0), (0, 0, Sh - 1, Sw - 1), (9, 13, 7, 11), (5, 6, 1, 1), (1, 1, Sh - 1, Sw - 1)]
    vals = [0.0, 0.0, -1.5, 0.5, float(np.float32(1 / 3))]
    rows = [whole(i, Sh, Sw, erase=bx, mode=D.ERASE_CONSTANT, value_bits=AU.f32_bits(v)) for i, bx, v in zip(idx, boxes, vals)]
    got = launch([IMAGES[i] for i in idx], rows, Sh, Sw)
    for b, ((ei, ej, eh, ew), v) in enumerate(zip(boxes, vals)):
        inside = torch.zeros(3, Sh, Sw, dtype=torch.bool)
        inside[:, ei : ei + eh, ej : ej + ew] = True
        assert inside.sum().item() == 3 * eh * ew
        assert torch.equal(got[b][inside], torch.full((3 * eh * ew,), v)), b
        assert torch.equal(got[b][~inside], plain[b][~inside]), b
    # erase mode 0 with a box, and a box with ew = 0: nothing is erased
    rows = [whole(0, Sh, Sw, erase=(1, 1, 5, 5), mode=D.ERASE_NONE), whole(1, Sh, Sw, erase=(1, 1, 5, 0), mode=D.ERASE_CONSTANT)]
    assert torch.equal(launch(IMAGES[:2], rows, Sh, Sw), plain[:2])


def test_erase_random_values_and_statistics():
    n = 3 * 24 * 24
    for seed in AU.STAT_SEEDS:
        rows = [whole(0, 24, 24, erase=(0, 0, 24, 24), mode=D.ERASE_RANDOM, seed=seed),
                whole(1, 24, 24, erase=(0, 0, 24, 24), mode=D.ERASE_RANDOM, seed=seed)]
        got = launch(IMAGES[:2], rows, 24, 24).double().numpy()
        ref = np.stack([AU.erase_normal(seed, b, 24, 24) for b in range(2)])
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"seed {seed}: random erase, largest error / largest magnitude {err:.2e} (bound 2e-05)")
        assert err <= 2e-5
        a, b = got[0].ravel(), got[1].ravel()
        for z in (a, b):
            assert abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.std() - 1) <= 4 / math.sqrt(2 * n), (seed, z.mean(), z.std())
        assert abs(np.corrcoef(a, b)[0, 1]) <= 4 / math.sqrt(n)
    # the values depend on (seed, image index), not on the launch: the same row in another batch position differs
    r = whole(0, 24, 24, erase=(0, 0, 24, 24), mode=D.ERASE_RANDOM, seed=11)
    twice = launch([IMAGES[0], IMAGES[0]], [r, r], 24, 24)
    assert not torch.equal(twice[0], twice[1])


def test_out_as_a_batch_slice_and_raw_as_the_tail_of_its_allocation():
    idx, rows, Sh, Sw, aa, ms = CASES["boxes24"]
    images = [IMAGES[i] for i in idx]
    B = len(images)
    # raw ends with its allocation and starts at an odd address; the last image's box is its bottom-right corner
    images2, rows2 = images + [IMAGES[4]], rows + [AU.row(10, 10, 10, 10, 24, 24)]
    packed = D.RaggedBatch.from_images(images2).raw
    pad = 3
    buf = torch.zeros(pad + packed.numel(), dtype=torch.uint8, device="cuda")
    buf[pad:] = packed.cuda()
    tail = buf[pad:]
    assert tail.data_ptr() % 4 == 3 and tail.data_ptr() + tail.numel() == buf.data_ptr() + buf.numel()
    big = torch.full((B + 3, 3, Sh, Sw), float("nan"), device="cuda")
    got = launch(images2, rows2, Sh, Sw, out=big[1 : B + 2], raw=tail)
    check(got[:B], reference("boxes24"), "boxes24 from the tail of an allocation into a batch slice")
    check(got[B:], AU.reference_batch([IMAGES[4]], AU.params_tensor(rows2[-1:]), Sh, Sw), "the last image's corner box")
    assert big[0].isnan().all() and big[B + 2].isnan().all() and torch.isfinite(big[1 : B + 2]).all()


def test_bad_arguments_return_invalid():
    lib = N.lib()
    batch = D.RaggedBatch.from_images(IMAGES[:2]).to("cuda")
    params = AU.params_tensor([whole(0, 16, 16), whole(1, 16, 16)]).cuda()
    out = torch.zeros(2, 3, 16, 16, device="cuda")

    def call(raw=batch.raw, table=batch.table, prm=params, o=out, B=2, Sh=16, Sw=16, lds=0):
        return lib.vt_augment_batch(vp(raw), vp(table), vp(prm), vp(o), B, Sh, Sw, 1, None, lds, stream())

    assert call() == N.VT_OK
    for kw, word in (({"raw": None}, "null"), ({"table": None}, "null"), ({"prm": None}, "null"), ({"o": None}, "null"),
                     ({"B": 0}, "size"), ({"Sh": 0}, "size"), ({"Sw": -1}, "size"), ({"lds": -1}, "lds_bytes"),
                     ({"lds": 64}, "lds_bytes"), ({"lds": lds_for_rows(16, 16, 1) - 1}, "lds_bytes")):
        assert call(**kw) == N.VT_ERR_INVALID, kw
        assert "vt_augment_batch" in N.last_error() and word in N.last_error(), (kw, N.last_error())
    assert call(lds=lds_for_rows(16, 16, 1)) == N.VT_OK
    assert call(lds=1 << 30) == N.VT_OK  # above 160 KiB means 160 KiB
    torch.cuda.synchronize()


def test_a_table_row_that_names_no_image_gives_zeros():
    """vt_amd.h: a row with H < 1, W < 1 or a negative offset reads nothing and its output is all zeros; the other images of
    the batch are what they are without it"""
    images = [IMAGES[0], IMAGES[1], IMAGES[2], IMAGES[4]]
    rows = [whole(i, 16, 24) for i in (0, 1, 2, 4)]
    plain = launch(images, rows, 16, 24)
    batch = D.RaggedBatch.from_images(images)
    table = batch.table.clone()
    table[0, 1], table[1, 2], table[2, 0] = 0, -3, -1
    raw, table, params = batch.raw.cuda(), table.cuda(), AU.params_tensor(rows).cuda()
    out = torch.full((4, 3, 16, 24), float("nan"), device="cuda")
    N.check(N.lib().vt_augment_batch(vp(raw), vp(table), vp(params), vp(out), 4, 16, 24, 1, None, 0, stream()))
    torch.cuda.synchronize()
    assert (out[:3] == 0).all() and torch.equal(out[3].cpu(), plain[3])


# ---- module level -------------------------------------------------------------------------------------------------
def test_module_on_cuda_against_its_cpu_path():
    batch = D.RaggedBatch.from_images(IMAGES)
    gen = torch.Generator().manual_seed(3)
    for S, kw in ((24, {}), ((16, 24), {"mean": MEAN_STD[:3], "std": MEAN_STD[3:]}), (16, {"antialias": False})):
        aug = D.GPUBatchTransform(S, **kw)
        params = D.sample_train_params(batch.sizes, S, erase_p=0.7, generator=gen)
        ref = aug(batch, params)
        got = aug(batch.to("cuda"), params)
        assert got.is_cuda and got.dtype == torch.float32
        check(got.cpu(), ref, f"module {S} {sorted(kw)}")
        assert torch.equal(aug(batch.to("cuda"), params.cuda()), got)  # a device table is used as it is
    ev = D.eval_params(batch.sizes, 20, 16)
    aug = D.GPUBatchTransform(16)
    check(aug(batch.to("cuda"), ev).cpu(), aug(batch, ev), "module validation geometry")
    with pytest.raises(ValueError, match=r"params\[2\]\.top"):
        bad = ev.clone()
        bad[2, D.P_TOP] = 5
        aug(batch.to("cuda"), bad)


def test_transform_feeds_the_train_step():
    """aug(batch, params, out=ts.images); ts.step() is the whole loop.  A second, identically filled TrainStep is fed
    ts.images.clone() through step(images=...).  What the trainer computes in a fixed order must be bit-equal: the resident
    batches (checked before the steps) and the logits of the step.  The loss is NOT a fixed-order sum: the loss kernel adds
    each sample's l / B to one float with atomicAdd from one workgroup per sample (csrc/vt_elementwise.hip, xent_kernel), so
    two runs on equal logits may differ by the rounding of B - 1 = 3 additions in another order -- two such steps gave
    2.3753378 and 2.3753376, one ulp apart, with the transform nowhere between them.  Each order adds positive terms with at
    most B - 1 roundings of half an ulp of the result, so the two losses are within B - 1 ulps of each other: that is the
    bound, and the loss recomputed from the (bit-equal) logits on the host is compared as well.  deterministic=True is the
    trainer's order-free mode for the backward sums; it is kept so that the whole step is reproducible, the loss sum apart."""
    import numpy as np
    import torch.nn.functional as F
    from oracle import filler
    from vision_toolbox import backbones
    from vision_toolbox.trainer import TrainStep

    B, S, ncls = 4, 32, 8
    batch = D.RaggedBatch.from_images(IMAGES[:4]).to("cuda")
    params = D.sample_train_params(batch.sizes, S, erase_p=0.5, generator=torch.Generator().manual_seed(9))
    labels = filler.labels(B, ncls).cuda()
    steps = []
    for _ in range(2):
        ts = TrainStep(backbones.darknet_yolov5n(), ncls, B, S, torch.float32, lr=0.01, device="cuda", deterministic=True)
        filler.fill_module(ts.model, "aug.")
        ts.weights_changed()
        steps.append(ts)
    a, b = steps
    aug = D.GPUBatchTransform(S)
    before = N.launch_count()
    assert aug(batch, params, out=a.images).data_ptr() == a.images.data_ptr()
    assert N.launch_count() == before + 1
    fed = a.images.clone()
    check(fed.cpu(), aug(D.RaggedBatch.from_images(IMAGES[:4]), params), "the batch in TrainStep.images")
    a.step(labels=labels)
    b.step(images=fed, labels=labels)
    assert torch.equal(a.images, fed) and torch.equal(b.images, fed)  # the step does not write its input batch
    la, lb = a.loss(), b.loss()
    assert math.isfinite(la) and math.isfinite(lb), (la, lb)
    assert torch.equal(a.logits(), b.logits())
    ulp = float(np.spacing(np.float32(max(abs(la), abs(lb)))))
    print(f"losses {la!r} {lb!r}: {abs(la - lb) / ulp:.0f} ulp apart (bound {B - 1})")
    assert abs(la - lb) <= (B - 1) * ulp, (la, lb)
    # the same loss from the logits on the host (label smoothing 0.1, the trainer's default), f32 against float64: the
    # kernel's per-sample terms are a few f32 operations each
    ref = F.cross_entropy(a.logits().double().cpu(), labels.cpu(), label_smoothing=0.1).item()
    assert abs(la - ref) <= 1e-5 * abs(ref) and abs(lb - ref) <= 1e-5 * abs(ref), (la, lb, ref)
