"""TrivialAugmentWide without a GPU: the host stage (data.trivial_augment_levels) against PIL, LEVEL FOR LEVEL, the table's
closed forms, the sampler's properties, the module's CPU path with and without a table, validate_ta and the two symbols.

The yardstick is PIL itself: torchvision's TrivialAugmentWide on PIL images dispatches onto ImageEnhance, ImageOps,
Image.transform(AFFINE) and Image.rotate (tests/trivial_augment_util.pil_apply), and on 8-bit images each of them is a fixed
sequence of integer, float32 and float64 operations, which the stage restates.  So the bound is equality: torch.equal.

Sampler bounds: 14,000 seeded draws; a count with probability q is within 5 binomial standard deviations, 5 sqrt(n q (1 -
q)) -- for the ops (q = 1 / 14) 5 * 30.47 = 152.4, i.e. +-153 around 1000."""
import math
import re
import subprocess

import pytest
import torch

import augment_util as AU
import trivial_augment_util as TU
from vision_toolbox import _native as N
from vision_toolbox import data as D

IMAGES = TU.make_images()
SETTINGS = TU.settings()


def _by_op(op):
    return [(o, m) for o, m in SETTINGS if o == op]


# ---- the stage against PIL ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", range(len(D.TA_OPS)), ids=D.TA_OPS)
def test_stage_is_pil_level_for_level(op):
    pytest.importorskip("PIL")
    sets = _by_op(op)
    assert len(sets) == (62 if op in D.TA_SIGNED else 31 if op in (D.TA_POSTERIZE, D.TA_SOLARIZE) else 1)
    for name, img in IMAGES.items():
        H, W = int(img.shape[0]), int(img.shape[1])
        ta = TU.table(sets, H, W)
        got = D.trivial_augment_levels(img[None].expand(len(sets), H, W, 3).contiguous(), ta)
        for k, ((_, mag), row) in enumerate(zip(sets, ta.tolist())):
            ref = TU.pil_apply(img, op, mag, row)
            assert torch.equal(got[k], ref), (name, D.TA_OPS[op], mag, int((got[k] != ref).sum()))


def test_the_images_reach_the_branches_they_are_there_for():
    pytest.importorskip("PIL")
    ident = D.trivial_augment_identity(1)

    def run(name, op, mag=0.0):
        img = IMAGES[name]
        return D.trivial_augment_levels(img[None], TU.table([(op, mag)], *img.shape[:2]))[0]

    # a constant image: both identity branches
    assert torch.equal(run("constant", D.TA_AUTOCONTRAST), IMAGES["constant"])
    assert torch.equal(run("constant", D.TA_EQUALIZE), IMAGES["constant"])
    # 1517 pixels: Equalize's step is (1517 - h[last]) // 255 = 5, and the table is not the identity
    n = IMAGES["noise37x41"]
    assert (37 * 41 - int(torch.bincount(n[..., 0].reshape(-1).long(), minlength=256)[int(n[..., 0].max())])) // 255 == 5
    assert not torch.equal(run("noise37x41", D.TA_EQUALIZE), n)
    # two levels: AutoContrast sends them to 0 and 255; 176 x 176: bins above 255
    two = run("twolevel", D.TA_AUTOCONTRAST)
    assert sorted(two[..., 0].unique().tolist()) == [0, 255]
    big = IMAGES["noise176"]
    assert int(torch.bincount(big[..., 0].reshape(-1).long(), minlength=256).max()) > 255
    assert int(torch.bincount(big[..., 2].reshape(-1).long(), minlength=256).max()) > 255
    # no interior: Sharpness is the identity whatever the factor
    for name in ("thin3x7", "line1x5"):
        if min(IMAGES[name].shape[:2]) < 3:
            assert torch.equal(run(name, D.TA_SHARPNESS, 0.99), IMAGES[name])
    assert torch.equal(D.trivial_augment_levels(n[None], ident)[0], n)


# ---- the table -----------------------------------------------------------------------------------------------------
def test_magnitudes_are_the_closed_forms():
    k = torch.arange(31, dtype=torch.float64)
    for op in (D.TA_SHEAR_X, D.TA_SHEAR_Y, D.TA_BRIGHTNESS, D.TA_COLOR, D.TA_CONTRAST, D.TA_SHARPNESS):
        assert torch.allclose(torch.tensor(D.ta_magnitudes(op), dtype=torch.float64), 0.99 * k / 30, rtol=0, atol=1e-7)
    for op in (D.TA_TRANSLATE_X, D.TA_TRANSLATE_Y):
        assert torch.allclose(torch.tensor(D.ta_magnitudes(op), dtype=torch.float64), 32.0 * k / 30, rtol=0, atol=4e-6)
    assert D.ta_magnitudes(D.TA_ROTATE) == [4.5 * i for i in range(31)]
    assert D.ta_magnitudes(D.TA_SOLARIZE) == [255.0 - 8.5 * i for i in range(31)]
    assert D.ta_magnitudes(D.TA_POSTERIZE) == [float(8 - round(i / 5)) for i in range(31)]
    assert D.ta_magnitudes(D.TA_POSTERIZE)[0] == 8.0 and D.ta_magnitudes(D.TA_POSTERIZE)[-1] == 2.0
    for op in (D.TA_IDENTITY, D.TA_AUTOCONTRAST, D.TA_EQUALIZE):
        assert D.ta_magnitudes(op) is None
    assert len(D.TA_OPS) == 14 and D.TA_OPS[0] == "Identity" and D.TA_OPS[5] == "Rotate" and D.TA_OPS[13] == "Equalize"


def test_rows_hold_the_matrices_and_arguments_of_the_definition():
    S = (37, 41)  # H, W
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert D.ta_row(D.TA_IDENTITY, 0.0, S) == [0.0, *ident, 0.0]
    assert D.trivial_augment_identity(3).tolist() == [[0.0, *ident, 0.0]] * 3
    # shear about (0, 0): x_in = x - m y ... the inverse of [[1, m], [0, 1]] up to the rounding of tan(atan(m))
    r = D.ta_row(D.TA_SHEAR_X, 0.33, S)
    assert r[0] == 1.0 and r[1] == 1.0 and abs(r[2] - 0.33) < 1e-15 and r[3] == 0.0 and abs(r[4]) < 1e-15 and abs(r[5] - 1) < 1e-15
    r = D.ta_row(D.TA_SHEAR_Y, -0.66, S)
    assert abs(r[4] + 0.66) < 1e-15 and abs(r[2]) < 1e-15 and r[6] == 0.0
    # translate: int() toward zero, about the image centre: x_in = x - tx
    assert D.ta_row(D.TA_TRANSLATE_X, 7.4666, S)[1:7] == [1.0, 0.0, -7.0, 0.0, 1.0, 0.0]
    assert D.ta_row(D.TA_TRANSLATE_X, -7.4666, S)[1:7] == [1.0, 0.0, 7.0, 0.0, 1.0, 0.0]
    assert D.ta_row(D.TA_TRANSLATE_Y, -0.9, S)[1:7] == ident
    assert D.ta_row(D.TA_TRANSLATE_Y, 32.0, S)[1:7] == [1.0, 0.0, 0.0, 0.0, 1.0, -32.0]
    # rotate: PIL's matrix, coefficients rounded to 15 digits, the centre (W / 2, H / 2) folded in
    r = D.ta_row(D.TA_ROTATE, 90.0, S)
    assert r[1:3] == [0.0, -1.0] and r[4:6] == [1.0, 0.0] and r[3] == 20.5 + 18.5 and r[6] == -20.5 + 18.5
    r = D.ta_row(D.TA_ROTATE, -90.0, S)
    assert r[1:3] == [0.0, 1.0] and r[4:6] == [-1.0, 0.0]
    t = -math.radians(31.5)
    r = D.ta_row(D.TA_ROTATE, 31.5, S)
    assert r[1] == round(math.cos(t), 15) and r[2] == round(math.sin(t), 15) and r[4] == round(-math.sin(t), 15)
    for op in (D.TA_BRIGHTNESS, D.TA_COLOR, D.TA_CONTRAST, D.TA_SHARPNESS):
        assert D.ta_row(op, -0.99, S) == [float(op), *ident, 1.0 - 0.99]
    assert D.ta_row(D.TA_POSTERIZE, 3.0, S)[7] == 3.0 and D.ta_row(D.TA_SOLARIZE, 246.5, S)[7] == 246.5
    with pytest.raises(ValueError):
        D.ta_row(14, 0.0, S)


# ---- the sampler ---------------------------------------------------------------------------------------------------
def test_sampler_frequencies_over_14000_draws():
    n = 14000
    ta, draws = D.sample_trivial_augment(n, 24, generator=torch.Generator().manual_seed(2026), return_draws=True)
    assert ta.dtype == torch.float64 and tuple(ta.shape) == (n, 8) and tuple(draws.shape) == (n, 3)
    D.validate_ta(ta, n)
    assert torch.equal(ta[:, 0].long(), draws[:, 0])
    ops = torch.bincount(draws[:, 0], minlength=14)
    assert ops.numel() == 14
    bound = math.ceil(5 * math.sqrt(n * (1 / 14) * (13 / 14)))
    assert bound == 153
    print("op counts", ops.tolist())
    assert int((ops - 1000).abs().max()) <= bound, ops.tolist()
    signed = torch.tensor([int(o) in D.TA_SIGNED for o in draws[:, 0].tolist()])
    ns = int(signed.sum())
    neg = int(draws[signed, 2].sum())
    print(f"signed draws {ns}, negated {neg}")
    assert abs(neg - ns / 2) <= 5 * math.sqrt(ns * 0.25)
    assert int(draws[~signed, 2].sum()) == 0
    has_bin = draws[:, 1] >= 0
    assert torch.equal(has_bin, torch.tensor([D.ta_magnitudes(int(o)) is not None for o in draws[:, 0].tolist()]))
    nb = int(has_bin.sum())
    bins = torch.bincount(draws[has_bin, 1], minlength=31)
    assert bins.numel() == 31
    assert float((bins - nb / 31).abs().max()) <= 5 * math.sqrt(nb * (1 / 31) * (30 / 31)), bins.tolist()
    # every row is the row of its draw
    for row, (op, k, neg) in list(zip(ta.tolist(), draws.tolist()))[:200]:
        mag = D.ta_magnitudes(op)[k] if k >= 0 else 0.0
        assert row == D.ta_row(op, -mag if neg else mag, 24)


def test_sampler_is_seeded_and_leaves_the_stream_of_sample_train_params_alone():
    sizes = [(37, 53), (64, 48), (375, 500)]
    gen = lambda s: torch.Generator().manual_seed(s)  # noqa: E731
    a = D.sample_trivial_augment(sizes, 16, generator=gen(5))
    assert torch.equal(a, D.sample_trivial_augment(3, (16, 16), generator=gen(5)))
    assert not torch.equal(D.sample_trivial_augment(64, 16, generator=gen(5)), D.sample_trivial_augment(64, 16, generator=gen(6)))
    # the table sample_train_params returned for this seed before TrivialAugmentWide existed
    before = [[11, 17, 21, 26, 16, 16, 0, 0, 0, 0, 0, 0, 0, 0, 434962709, 0],
              [20, 21, 23, 26, 16, 16, 0, 0, 0, 4, 9, 6, 3, 2, 188411497, 0],
              [0, 4, 374, 476, 16, 16, 0, 0, 0, 8, 9, 8, 3, 2, 2104637782, 0]]
    g = gen(2026)
    assert D.sample_train_params(sizes, 16, erase_p=0.5, generator=g).tolist() == before
    # ... and with a table drawn from a generator of its own in between, the next table is the next table
    g1, g2 = gen(2026), gen(2026)
    D.sample_train_params(sizes, 16, generator=g1), D.sample_train_params(sizes, 16, generator=g2)
    D.sample_trivial_augment(sizes, 16, generator=gen(1))
    assert torch.equal(D.sample_train_params(sizes, 16, generator=g1), D.sample_train_params(sizes, 16, generator=g2))


# ---- the module's CPU path -------------------------------------------------------------------------------------------
MEAN_STD = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _batch_and_params(S=(16, 24)):
    images = AU.make_images()
    batch = D.RaggedBatch.from_images(images)
    params = D.sample_train_params(batch.sizes, S, erase_p=0.7, generator=torch.Generator().manual_seed(3))
    return images, batch, params


def test_without_a_table_the_cpu_path_is_todays():
    images, batch, params = _batch_and_params()
    for kw in ({}, {"mean": MEAN_STD[0], "std": MEAN_STD[1]}, {"antialias": False}):
        aug = D.GPUBatchTransform((16, 24), **kw)
        today = aug._run_torch(batch, params, torch.empty(6, 3, 16, 24))  # the path as it was: no table argument
        assert torch.equal(aug(batch, params), today) and torch.equal(aug(batch, params, ta=None), today)
        ms = kw.get("mean") and (*kw["mean"], *kw["std"])
        l2, linf = AU.errors(today, AU.reference_batch(images, params, 16, 24, kw.get("antialias", True), ms))
        assert l2 <= 2e-5 and linf <= 2e-5


def test_identity_rows_give_the_rounded_levels_over_255():
    # the three downscaled sources, whole, to 16 x 24: weights that are no dyadic fractions, so no exact half levels
    images = [AU.make_images()[i] for i in (0, 3, 5)]
    batch = D.RaggedBatch.from_images(images)
    params = AU.params_tensor([AU.row(0, 0, H, W, 16, 24, flip=k & 1) for k, (H, W) in enumerate(batch.sizes)])
    aug = D.GPUBatchTransform((16, 24))
    got = aug(batch, params, ta=D.trivial_augment_identity(3))
    v255 = AU.reference_batch(images, params, 16, 24) * 255.0  # float64
    away = ((v255 - torch.floor(v255)) - 0.5).abs().min().item()
    assert away > 1e-4, away  # no value close enough to a half level for float32 to round it the other way
    levels = torch.floor(v255 + 0.5).clamp(0, 255)
    assert torch.equal(got, levels.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32))
    assert torch.equal(aug._levels_torch(batch, params), levels.permute(0, 2, 3, 1).to(torch.uint8))
    assert torch.equal(D.round_levels(torch.tensor([-3.0, 0.49999, 0.5, 1.5, 254.5, 300.0])),
                       torch.tensor([0, 0, 1, 2, 255, 255], dtype=torch.uint8))


def test_cpu_path_with_a_table_is_levels_stage_scale_meanstd_erase():
    images, batch, params = _batch_and_params()
    ta = D.sample_trivial_augment(6, (16, 24), generator=torch.Generator().manual_seed(8))
    ta[0] = torch.tensor(D.ta_row(D.TA_EQUALIZE, 0.0, (16, 24)))
    ta[1] = torch.tensor(D.ta_row(D.TA_ROTATE, 31.5, (16, 24)))
    aug = D.GPUBatchTransform((16, 24), mean=MEAN_STD[0], std=MEAN_STD[1])
    out = torch.full((8, 3, 16, 24), float("nan"))
    got = aug(batch, params, out=out[1:7], ta=ta)
    assert got.data_ptr() == out[1:7].data_ptr() and out[0].isnan().all() and out[7].isnan().all()
    levels = D.trivial_augment_levels(aug._levels_torch(batch, params), ta)
    ms = torch.tensor(MEAN_STD, dtype=torch.float32)
    erased = 0
    for b, row in enumerate(params.tolist()):
        ei, ej, eh, ew, mode, seed, _ = row[9:]
        ref = (levels[b].permute(2, 0, 1).float() * torch.tensor(1 / 255, dtype=torch.float32) - ms[0].view(3, 1, 1)) / ms[1].view(3, 1, 1)
        if mode == D.ERASE_RANDOM and eh > 0:
            ref[:, ei : ei + eh, ej : ej + ew] = D.erase_normal(seed, b, 16, 24)[:, ei : ei + eh, ej : ej + ew]
            erased += 1
        assert torch.equal(got[b], ref), b
    assert erased >= 2


# ---- refusals and symbols ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [("op", 14.0, "op"), ("op", -1.0, "op"), ("op", 2.5, "op"), ("op", float("nan"), "op"),
                                              ("m2", float("inf"), "m2"), ("m4", float("nan"), "m4"), ("arg", 0.0, "arg"),
                                              ("arg", 9.0, "arg"), ("arg", 2.5, "arg")])
def test_validate_ta_names_image_and_field(field, value, word):
    ta = D.trivial_augment_identity(3)
    ta[1] = torch.tensor(D.ta_row(D.TA_POSTERIZE, 4.0, 16))
    ta[1, D.TA_FIELDS.index(field)] = value
    with pytest.raises(ValueError, match=rf"ta\[1\]\.{word} "):
        D.validate_ta(ta)
    with pytest.raises(ValueError, match=rf"ta\[1\]\.{word} "):
        images = AU.make_images()[:3]
        D.GPUBatchTransform(16)(D.RaggedBatch.from_images(images), D.eval_params([i.shape[:2] for i in images], 16, 16), ta=ta)


def test_validate_ta_refuses_shapes_factors_and_thresholds():
    good = D.sample_trivial_augment(5, 16, generator=torch.Generator().manual_seed(1))
    D.validate_ta(good), D.validate_ta(good, 5)
    for bad in (good.float(), good[:, :7], good.reshape(-1)):
        with pytest.raises(ValueError, match="ta: expected float64"):
            D.validate_ta(bad)
    with pytest.raises(ValueError, match="ta: expected float64 \\[4, 8\\]"):
        D.validate_ta(good, 4)
    for op, arg in ((D.TA_BRIGHTNESS, -0.5), (D.TA_SHARPNESS, float("nan")), (D.TA_SOLARIZE, float("nan"))):
        t = good.clone()
        t[2] = torch.tensor(D.ta_row(op, 0.0, 16))
        t[2, 7] = arg
        with pytest.raises(ValueError, match=rf"ta\[2\]\.arg .*{D.TA_OPS[op]}"):
            D.validate_ta(t)
    with pytest.raises(ValueError, match="u8: expected uint8"):
        D.trivial_augment_levels(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), good[:2])
    with pytest.raises(ValueError, match="ta: expected float64"):
        D.trivial_augment_levels(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), good[:3])


def test_the_stage_reads_an_unvalidated_table_as_the_header_says():
    img = IMAGES["noise24"]
    rows = torch.tensor([[99.0, 1, 0, 0, 0, 1, 0, 0], [float("nan"), 1, 0, 0, 0, 1, 0, 0], [-1.0, 1, 0, 0, 0, 1, 0, 0],
                         [10.0, 1, 0, 0, 0, 1, 0, 0.0], [10.0, 1, 0, 0, 0, 1, 0, 12.0], [10.9, 1, 0, 0, 0, 1, 0, 3.7]], dtype=torch.float64)
    got = D.trivial_augment_levels(img[None].expand(6, 24, 24, 3).contiguous(), rows)
    assert torch.equal(got[0], img) and torch.equal(got[1], img) and torch.equal(got[2], img)  # not an op: Identity
    assert torch.equal(got[3], img & 128)  # 0 bits: clamped to 1
    assert torch.equal(got[4], img)        # 12 bits: clamped to 8
    assert torch.equal(got[5], img & 0xE0)  # op 10.9 -> 10, 3.7 bits -> 3


def test_symbols_are_declared_bound_and_exported():
    text = (N.LIB_PATH.parents[2] / "include" / "vt_amd.h").read_text()
    for name, nargs in (("vt_augment_batch_u8", 10), ("vt_trivial_augment", 10)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert name in N.SYMBOLS and len(N.SYMBOLS[name][1]) == nargs
        assert getattr(N.lib(), name).argtypes == N.SYMBOLS[name][1]
    assert "const uint8_t* u8, const double* ta, const int32_t* params, float* out, uint32_t* workspace" in text
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r" T vt_augment_batch_u8\b", out) and re.search(r" T vt_trivial_augment\b", out)
    assert len(N.SYMBOLS["vt_augment_batch"][1]) == 11  # the float entry keeps its signature
