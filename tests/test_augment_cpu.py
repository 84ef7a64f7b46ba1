"""The input transform without a GPU: the float64 restatement (tests/augment_util.py) against F.interpolate and PIL, the
module's plain-torch path against the restatement, the sampling rules' properties, the validation geometry, packing, the
ValueErrors and the C-ABI symbol.

Bounds.  Restatement against F.interpolate in float64: 1e-12, absolute, on values 0 .. 255 (the same sums in another order).
Restatement x 255 against PIL: 1.05 levels -- PIL rounds to 8 bits after each of its two passes (half a level each) and
uses fixed-point coefficients.  The module's float32 path against the restatement: gpu_util.tol (2e-5, relative L2).
Frequencies: four binomial standard deviations.  Area and ratio of a sampled box: the sampler rounds both sides to
integers, so a side is within 0.5 of its real value; the checks move each side by 0.5 in the favourable direction."""
import math
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_util as AU
from gpu_util import tol
from vision_toolbox import _native as N
from vision_toolbox import data as D


def _interp(crop_u8: torch.Tensor, OH: int, OW: int, antialias: bool) -> np.ndarray:
    x = crop_u8.permute(2, 0, 1)[None].double()
    return F.interpolate(x, (OH, OW), mode="bilinear", antialias=antialias, align_corners=False)[0].numpy()


# (source H, W), crop (top, left, h, w), virtual (OH, OW)
GEOMS = [((37, 53), (0, 0, 37, 53), (16, 16)), ((37, 53), (5, 7, 20, 31), (24, 24)), ((9, 7), (0, 0, 9, 7), (24, 24)),
         ((9, 7), (3, 2, 2, 3), (24, 24)), ((131, 97), (100, 60, 31, 37), (16, 24)), ((64, 48), (0, 0, 64, 48), (26, 20)),
         ((20, 20), (0, 0, 20, 20), (20, 20)), ((300, 400), (0, 0, 300, 400), (16, 21)), ((9, 7), (4, 3, 1, 1), (5, 5))]


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][2]}x{g[1][3]}-to-{g[2][0]}x{g[2][1]}")
def test_restatement_is_f_interpolate(geom, antialias):
    (H, W), (top, left, h, w), (OH, OW) = geom
    img = AU.make_images([(H, W)], seed=3)[0]
    crop = img[top : top + h, left : left + w]
    got = AU.resample(crop.numpy().astype(np.float64), OH, OW, antialias)
    ref = _interp(crop, OH, OW, antialias)
    assert np.abs(got - ref).max() <= 1e-12


def test_validation_window_is_resize_then_slice():
    for (H, W) in [(37, 53), (64, 48), (20, 20)]:
        img = AU.make_images([(H, W)], seed=4)[0]
        prm = D.eval_params([(H, W)], 20, 16)
        OH, OW, oy, ox = (int(prm[0, k]) for k in (D.P_OH, D.P_OW, D.P_OY, D.P_OX))
        ref = _interp(img, OH, OW, True)[:, oy : oy + 16, ox : ox + 16] / 255.0
        got = AU.reference_image(img, prm[0], 0, 16, 16)
        assert np.abs(got - ref).max() <= 1e-12


def test_restatement_against_pil():
    Image = pytest.importorskip("PIL.Image")
    worst = 0.0
    for (H, W), (top, left, h, w), (OH, OW) in GEOMS[:8]:
        img = AU.make_images([(H, W)], seed=5)[0]
        pil = Image.fromarray(img.numpy()).crop((left, top, left + w, top + h)).resize((OW, OH), Image.BILINEAR)
        ref = np.asarray(pil).astype(np.float64).transpose(2, 0, 1)
        got = AU.resample(img[top : top + h, left : left + w].numpy().astype(np.float64), OH, OW, True)
        worst = max(worst, np.abs(got - ref).max())
    print(f"restatement x 255 against PIL: at most {worst:.3f} levels")
    assert worst <= 1.05


# ---- the module's CPU path ----------------------------------------------------------------------------------------
def _train_rows(Sh, Sw):
    E = D.ERASE_RANDOM
    return [AU.row(0, 0, 37, 53, Sh, Sw, flip=1, erase=(2, 3, 5, 4), mode=E, seed=7),
            AU.row(10, 5, 40, 30, Sh, Sw, erase=(0, 0, Sh - 1, Sw - 1), mode=D.ERASE_CONSTANT, value_bits=AU.f32_bits(0.25)),
            AU.row(3, 2, 2, 3, Sh, Sw, flip=1),
            AU.row(0, 0, 131, 97, Sh, Sw),
            AU.row(19, 19, 1, 1, Sh, Sw, erase=(Sh - 1, Sw - 1, 1, 1), mode=E, seed=9),
            AU.row(0, 0, 300, 400, Sh, Sw, flip=1)]


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("mean_std", [None, ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))], ids=["plain", "meanstd"])
def test_module_cpu_path_is_the_restatement(antialias, mean_std):
    images = AU.make_images()
    batch = D.RaggedBatch.from_images(images)
    params = AU.params_tensor(_train_rows(16, 24))
    aug = D.GPUBatchTransform((16, 24), antialias=antialias, mean=mean_std and mean_std[0], std=mean_std and mean_std[1])
    got = aug(batch, params)
    ref = AU.reference_batch(images, params, 16, 24, antialias, mean_std and (*mean_std[0], *mean_std[1]))
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, 3, 16, 24)
    l2, linf = AU.errors(got, ref)
    assert l2 <= tol(N.VT_F32) and linf <= 2e-5, (l2, linf)
    out = torch.full((8, 3, 16, 24), float("nan"))
    assert aug(batch, params, out=out[1:7]).data_ptr() == out[1:7].data_ptr()
    assert torch.equal(out[1:7], got) and out[0].isnan().all() and out[7].isnan().all()


def test_module_cpu_validation_geometry():
    images = AU.make_images()
    batch = D.RaggedBatch.from_images(images[:2] + images[4:5])
    params = D.eval_params(batch.sizes, 20, 16)
    got = D.GPUBatchTransform(16)(batch, params)
    ref = AU.reference_batch(images[:2] + images[4:5], params, 16, 16)
    l2, linf = AU.errors(got, ref)
    assert l2 <= tol(N.VT_F32) and linf <= 2e-5, (l2, linf)


def test_erase_generator_torch_restates_numpy():
    for seed, b in ((0, 0), (7, 3), (2**31 - 1, 255), (-5, 2)):
        got = D.erase_normal(seed, b, 5, 9).double().numpy()
        ref = AU.erase_normal(seed, b, 5, 9)
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()
    assert not np.array_equal(AU.erase_normal(1, 0, 4, 4), AU.erase_normal(2, 0, 4, 4))
    assert not np.array_equal(AU.erase_normal(1, 0, 4, 4), AU.erase_normal(1, 1, 4, 4))


def test_erase_generator_statistics_for_the_seeds_of_the_gpu_test():
    """n = 3 * 24 * 24 = 1728 values per image: |mean| <= 4 / sqrt(n), |std - 1| <= 4 / sqrt(2 n), and the correlation of
    two images' boxes under one seed at most 4 / sqrt(n)."""
    n = 3 * 24 * 24
    for seed in AU.STAT_SEEDS:
        a, b = AU.erase_normal(seed, 0, 24, 24).ravel(), AU.erase_normal(seed, 1, 24, 24).ravel()
        for z in (a, b):
            assert abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.std() - 1) <= 4 / math.sqrt(2 * n), (seed, z.mean(), z.std())
        assert abs(np.corrcoef(a, b)[0, 1]) <= 4 / math.sqrt(n)


# ---- the sampling rules -------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampler_boxes_ranges_and_frequencies():
    sizes = [(375, 500), (500, 333), (37, 53), (64, 64), (9, 7)] * 600  # 3000 draws
    S, scale, ratio = 24, (0.08, 1.0), (3 / 4, 4 / 3)
    es, er = (0.02, 0.33), (0.3, 3.3)
    prm, fell = D.sample_train_params(sizes, S, erase_p=0.25, generator=_gen(1), return_fallback=True)
    assert prm.dtype == torch.int32 and tuple(prm.shape) == (3000, 16)
    D.validate_params(prm, sizes, S)  # every box inside its image, every erase box inside the output
    p = prm.tolist()
    for (H, W), r, fb in zip(sizes, p, fell.tolist()):
        top, left, h, w = r[:4]
        assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= H and left + w <= W
        assert r[D.P_OH] == S and r[D.P_OW] == S and r[D.P_OY] == 0 and r[D.P_OX] == 0
        if not fb:
            assert (h + 0.5) * (w + 0.5) >= scale[0] * H * W and (h - 0.5) * (w - 0.5) <= scale[1] * H * W
            assert (w + 0.5) / (h - 0.5) >= ratio[0] and (w - 0.5) / (h + 0.5) <= ratio[1]
        eh, ew = r[D.P_EH], r[D.P_EW]
        if eh:
            assert r[D.P_MODE] == D.ERASE_RANDOM and 0 < eh < S and 0 < ew < S
            assert (eh + 0.5) * (ew + 0.5) >= es[0] * S * S and (eh - 0.5) * (ew - 0.5) <= es[1] * S * S
            assert (eh + 0.5) / (ew - 0.5) >= er[0] and (eh - 0.5) / (ew + 0.5) <= er[1]
        else:
            assert r[D.P_MODE] == D.ERASE_NONE
    assert not fell.any()  # these shapes all admit a box of the ratio range
    n = len(sizes)
    flips = sum(r[D.P_FLIP] for r in p)
    assert abs(flips - 0.5 * n) <= 4 * math.sqrt(n * 0.25)
    # an erase draw can fail only if ten boxes in a row do not fit: at these ranges on a square output a box fits with
    # probability > 0.9 per draw, so the erase frequency is p up to 1e-10
    erases = sum(1 for r in p if r[D.P_EH] > 0)
    assert abs(erases - 0.25 * n) <= 4 * math.sqrt(n * 0.25 * 0.75)
    assert len({r[D.P_SEED] for r in p if r[D.P_EH] > 0}) > 0.9 * erases  # per-image seeds


def test_sampler_fallback_on_a_shape_outside_the_ratio_range():
    prm, fell = D.sample_train_params([(4, 400), (400, 4)] * 50, 16, generator=_gen(2), return_fallback=True)
    assert fell.all()
    for r in prm.tolist()[:2]:
        top, left, h, w = r[:4]
        H, W = (4, 400) if h == 4 else (400, 4)
        assert (h, w) in ((4, 5), (5, 4))  # the whole short side, the long side the short one times 4/3, rounded
        assert top == (H - h) // 2 and left == (W - w) // 2


def test_sampler_is_a_function_of_the_generator_seed():
    sizes = [(37, 53), (64, 48)] * 20
    a = D.sample_train_params(sizes, 16, erase_p=0.5, generator=_gen(5))
    b = D.sample_train_params(sizes, 16, erase_p=0.5, generator=_gen(5))
    c = D.sample_train_params(sizes, 16, erase_p=0.5, generator=_gen(6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    k = D.sample_train_params(sizes, 16, erase_p=1.0, erase_value=0.5, generator=_gen(5))
    assert (k[:, D.P_MODE] == D.ERASE_CONSTANT).all() and (k[:, D.P_VALUE] == AU.f32_bits(0.5)).all()
    assert (D.sample_train_params(sizes, 16, erase_p=0.0, generator=_gen(5))[:, D.P_EH] == 0).all()
    assert (D.sample_train_params(sizes, 16, flip_p=0.0, generator=_gen(5))[:, D.P_FLIP] == 0).all()
    with pytest.raises(ValueError, match="erase_value"):
        D.sample_train_params(sizes, 16, erase_value="noise")


def test_eval_params_portrait_landscape_square():
    prm = D.eval_params([(500, 375), (375, 500), (300, 300), (333, 500)]).tolist()
    # shorter side to 232, the other int(232 * long / short); the window at int(round((O - 224) / 2))
    assert prm[0][:8] == [0, 0, 500, 375, 309, 232, 42, 4]
    assert prm[1][:8] == [0, 0, 375, 500, 232, 309, 4, 42]
    assert prm[2][:8] == [0, 0, 300, 300, 232, 232, 4, 4]
    assert prm[3][:8] == [0, 0, 333, 500, 232, 348, 4, 62]
    assert all(r[8:] == [0] * 8 for r in prm)
    assert D.eval_params([(64, 48)], 20, (16, 12)).tolist()[0][:8] == [0, 0, 64, 48, 26, 20, 5, 4]
    with pytest.raises(ValueError, match="image 0"):
        D.eval_params([(64, 48)], 20, 24)


# ---- packing and refusals -----------------------------------------------------------------------------------------
def test_ragged_batch_packs_and_validates():
    images = AU.make_images()
    batch = D.RaggedBatch.from_images(images)
    assert len(batch) == 6 and batch.sizes == AU.SIZES
    assert batch.raw.dtype == torch.uint8 and batch.raw.numel() == sum(3 * H * W for H, W in AU.SIZES)
    assert batch.table.dtype == torch.int64 and tuple(batch.table.shape) == (6, 3)
    off = 0
    for im, (o, H, W) in zip(images, batch.table.tolist()):
        assert o == off and (H, W) == tuple(im.shape[:2])
        assert torch.equal(batch.raw[o : o + H * W * 3].view(H, W, 3), im)
        off += H * W * 3
    # a non-contiguous view packs like its contiguous copy
    v = images[0][::2, 1:]
    assert torch.equal(D.RaggedBatch.from_images([v]).raw, v.contiguous().view(-1))
    moved = batch.to("cpu")
    assert torch.equal(moved.raw, batch.raw) and moved.sizes == batch.sizes
    for bad, what in (([], "no images"), ([images[0].float()], "image 0.*uint8"), ([images[0], images[1][..., :2]], "image 1.*HWC"),
                      ([images[0].permute(2, 0, 1)], "image 0.*HWC"), ([images[0][:0]], "image 0.*empty")):
        with pytest.raises(ValueError, match=what):
            D.RaggedBatch.from_images(bad)


@pytest.mark.parametrize("field,value", [("top", -1), ("top", 60), ("left", 50), ("h", 0), ("w", 0), ("h", 63), ("OH", 0),
                                         ("oy", 1), ("ox", -1), ("OW", 15), ("erase_mode", 3), ("ei", 15), ("ej", -1),
                                         ("eh", 17), ("ew", -2)])
def test_bad_host_params_raise_naming_image_and_field(field, value):
    images = AU.make_images()[:2]
    batch = D.RaggedBatch.from_images(images)
    rows = [AU.row(0, 0, 37, 53, 16, 16), AU.row(2, 3, 10, 12, 16, 16, erase=(1, 1, 2, 2), mode=1)]
    rows[1][D.FIELDS.index(field)] = value
    # (a field that is only wrong through another one is reported under the field that holds the position)
    named = {"h": "h|top", "w": "w|left", "OW": "ox", "eh": "eh|ei", "ew": "ew|ej"}.get(field, field)
    with pytest.raises(ValueError, match=rf"params\[1\]\.({named}) "):
        D.GPUBatchTransform(16)(batch, AU.params_tensor(rows))


def test_transform_refuses_wrong_tables_and_outputs():
    batch = D.RaggedBatch.from_images(AU.make_images()[:2])
    good = AU.params_tensor([AU.row(0, 0, 37, 53, 16, 16), AU.row(0, 0, 64, 48, 16, 16)])
    aug = D.GPUBatchTransform(16)
    with pytest.raises(ValueError, match="params"):
        aug(batch, good[:1])
    with pytest.raises(ValueError, match="params"):
        aug(batch, good.long())
    with pytest.raises(ValueError, match="out"):
        aug(batch, good, out=torch.empty(2, 3, 16, 17))
    with pytest.raises(ValueError, match="out"):
        aug(batch, good, out=torch.empty(2, 3, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="mean and std"):
        D.GPUBatchTransform(16, mean=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="std"):
        D.GPUBatchTransform(16, mean=(0.5, 0.5, 0.5), std=(1.0, 0.0, 1.0))


def test_symbol_is_declared_bound_and_exported():
    import vision_toolbox

    assert vision_toolbox.data is D
    text = (N.LIB_PATH.parents[2] / "include" / "vt_amd.h").read_text()
    assert re.search(r"\bint vt_augment_batch\(const uint8_t\* raw, const int64_t\* table, const int32_t\* params, float\* out", text)
    assert "vt_augment_batch" in N.SYMBOLS and len(N.SYMBOLS["vt_augment_batch"][1]) == 11
    assert getattr(N.lib(), "vt_augment_batch").argtypes == N.SYMBOLS["vt_augment_batch"][1]
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r" T vt_augment_batch\b", out)
