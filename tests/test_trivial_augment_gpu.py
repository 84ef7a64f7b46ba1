"""vt_trivial_augment and vt_augment_batch_u8 through the C-ABI against the host stage (data.trivial_augment_levels, which
tests/test_trivial_augment_cpu.py holds to PIL level for level), and GPUBatchTransform(ta=...) on top of them.

Bounds.  The levels are integers and float32(level) * float32(1 / 255) is one rounding: torch.equal.  With mean / std the
relative bound of tests/test_augment_gpu.py (2e-5).  The random erase: 2e-5 of the largest magnitude, as there.
vt_augment_batch_u8 filters in float32 in another summation order than the host path, so a level may differ where the
filtered value sits within float error of x.5: at most 1 level apart on at most 1 element in 10,000 -- on cases of
test_augment_gpu.py (rows taken from its helpers) chosen so that the float64 restatement has no value within 1e-4 of a half
level, which is asserted here first.  Every launch runs twice and must be bit-identical."""
import numpy as np
import pytest
import torch

import augment_util as AU
import test_augment_gpu as TG
import trivial_augment_util as TU
from gpu_util import stream, vp
from vision_toolbox import _native as N
from vision_toolbox import data as D

pytestmark = pytest.mark.gpu

IMAGES = TU.make_images()
SETTINGS = TU.settings()
MEAN_STD = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
INV255 = torch.tensor(1.0 / 255.0, dtype=torch.float32)
_REF = {}


def settings_for(name):
    """every setting on the tiny images (2 x 31 x 9 + 31 x 2 + 3 = 623 rows a batch, mixed ops); on the 176 x 176 image every
    setting of the histogram ops and bins 3, 20 (Rotate: 90 degrees) and 30 of the others"""
    if name != "noise176":
        return SETTINGS
    keep = []
    for op in range(len(D.TA_OPS)):
        mags = D.ta_magnitudes(op)
        for o, m in SETTINGS:
            if o == op and (mags is None or op == D.TA_CONTRAST or abs(m) in (mags[3], mags[20], mags[30])):
                keep.append((o, m))
    return keep


def stage_reference(name):
    """(levels uint8 [B, H, W, 3], table [B, 8], host stage of both): computed once, shared, never written"""
    if name not in _REF:
        img = IMAGES[name]
        H, W = int(img.shape[0]), int(img.shape[1])
        ta = TU.table(settings_for(name), H, W)
        u8 = img[None].expand(ta.shape[0], H, W, 3).contiguous()
        _REF[name] = (u8, ta, D.trivial_augment_levels(u8, ta))
    return _REF[name]


def no_erase(B, S=16):
    return AU.params_tensor([AU.row(0, 0, S, S, S, S)] * B)


def run_stage(u8, ta, params, mean_std=None, guard=1):
    """vt_trivial_augment on device copies, twice (bit-identical), into the middle of a NaN-filled buffer whose guard images
    must stay NaN; returns out on the host"""
    B, H, W, _ = u8.shape
    du8, dta, dprm = u8.cuda(), ta.cuda(), params.cuda()
    work = torch.full((B, 4, 256), 0x55555555, dtype=torch.int32, device="cuda")  # garbage: the call clears it
    ms = torch.tensor(mean_std, dtype=torch.float32, device="cuda") if mean_std is not None else None
    big = torch.full((B + 2 * guard, 3, H, W), float("nan"), device="cuda")
    out = big[guard : guard + B]

    def run():
        N.check(N.lib().vt_trivial_augment(vp(du8), vp(dta), vp(dprm), vp(out), vp(work), B, H, W, vp(ms), stream()))
        torch.cuda.synchronize()
        return out.clone()

    first = run()
    assert torch.equal(run(), first), "two launches differ"
    assert big[:guard].isnan().all() and big[guard + B :].isnan().all(), "a guard image was written"
    assert torch.isfinite(first).all()
    return first.cpu()


def levels_of(out):
    """float32 [B, 3, H, W] = level / 255 -> uint8 [B, H, W, 3]; asserts that out is exactly float32(level) * float32(1 / 255)"""
    lv = torch.round(out.double() * 255.0)
    assert lv.min() >= 0 and lv.max() <= 255
    assert torch.equal(out, lv.float() * INV255), "out is not float32(level) * float32(1 / 255)"
    return lv.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ---- vt_trivial_augment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IMAGES))
def test_stage_kernel_is_the_host_stage_level_for_level(name):
    u8, ta, ref = stage_reference(name)
    got = levels_of(run_stage(u8, ta, no_erase(u8.shape[0])))
    bad = (got != ref).reshape(got.shape[0], -1).sum(1)
    wrong = [(D.TA_OPS[int(ta[b, 0])], float(ta[b, 7]), int(bad[b])) for b in bad.nonzero().reshape(-1).tolist()]
    assert not wrong, (name, len(wrong), wrong[:8])


@pytest.mark.parametrize("name", ["noise37x41", "twolevel"])
def test_stage_kernel_with_mean_std(name):
    u8, ta, ref = stage_reference(name)
    got = run_stage(u8, ta, no_erase(u8.shape[0]), MEAN_STD)
    m = torch.tensor(MEAN_STD, dtype=torch.float32).double()
    want = (ref.permute(0, 3, 1, 2).double() / 255.0 - m[:3].view(1, 3, 1, 1)) / m[3:].view(1, 3, 1, 1)
    l2, linf = AU.errors(got, want)
    print(f"{name} with mean / std: relative L2 {l2:.2e}, largest element error / largest magnitude {linf:.2e} (bounds 2e-05)")
    assert l2 <= 2e-5 and linf <= 2e-5


def test_erase_boxes_constant_and_random_as_on_the_one_launch_path():
    img = IMAGES["noise24"]
    ops = [(D.TA_IDENTITY, 0.0), (D.TA_ROTATE, 31.5), (D.TA_EQUALIZE, 0.0), (D.TA_SHARPNESS, 0.66), (D.TA_SOLARIZE, 127.5),
           (D.TA_COLOR, -0.33)]
    B, S = len(ops), 24
    ta = TU.table(ops, S, S)
    u8 = img[None].expand(B, S, S, 3).contiguous()
    plain = run_stage(u8, ta, no_erase(B, S))
    boxes = [(0, 0, 0, 0), (0, 0, S - 1, S - 1), (9, 13, 7, 11), (5, 6, 1, 1), (1, 1, S - 1, S - 1), (3, 3, 0, 5)]
    seeds = [0, 3, -7, 5, 2**31 - 1, 1]
    for mode in (D.ERASE_CONSTANT, D.ERASE_RANDOM):
        rows = [AU.row(0, 0, S, S, S, S, erase=bx, mode=mode, seed=sd, value_bits=AU.f32_bits(-1.5)) for bx, sd in zip(boxes, seeds)]
        got = run_stage(u8, ta, AU.params_tensor(rows))
        for b, ((ei, ej, eh, ew), sd) in enumerate(zip(boxes, seeds)):
            inside = torch.zeros(3, S, S, dtype=torch.bool)
            if eh > 0 and ew > 0:
                inside[:, ei : ei + eh, ej : ej + ew] = True
            assert torch.equal(got[b][~inside], plain[b][~inside]), (mode, b)
            if mode == D.ERASE_CONSTANT:
                assert torch.equal(got[b][inside], torch.full((int(inside.sum()),), -1.5)), b
            elif inside.any():
                ref = torch.from_numpy(AU.erase_normal(sd, b, S, S))[inside]
                err = ((got[b][inside].double() - ref).abs().max() / ref.abs().max()).item()
                assert err <= 2e-5, (b, err)
    # mode 0 with a box: nothing is erased
    rows = [AU.row(0, 0, S, S, S, S, erase=(1, 1, 5, 5), mode=D.ERASE_NONE)] * B
    assert torch.equal(run_stage(u8, ta, AU.params_tensor(rows)), plain)


def test_unvalidated_device_table_is_read_as_the_header_says():
    """op 99, NaN and -1 are Identity; Posterize with 0 bits keeps 1 bit, with 12 bits keeps 8; a fractional op and bit count
    are truncated; a matrix of NaNs and a huge one fill with zeros; nothing faults"""
    img = IMAGES["noise37x41"]
    nan, ident = float("nan"), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    rows = [[99.0, *ident, 0.0], [nan, *ident, 0.0], [-1.0, *ident, 0.0], [10.0, *ident, 0.0], [10.0, *ident, 12.0],
            [10.9, *ident, 3.7], [10.0, *ident, nan], [5.0, nan, nan, nan, nan, nan, nan, 0.0],
            [1.0, 1e300, 0.0, 1e300, 0.0, 1.0, 0.0, 0.0], [14.0, *ident, 0.0]]
    ta = torch.tensor(rows, dtype=torch.float64)
    u8 = img[None].expand(len(rows), 37, 41, 3).contiguous()
    got = levels_of(run_stage(u8, ta, no_erase(len(rows))))
    assert torch.equal(got, D.trivial_augment_levels(u8, ta))
    for b in (0, 1, 2, 4, 9):
        assert torch.equal(got[b], img), b
    assert torch.equal(got[3], img & 128) and torch.equal(got[6], img & 128) and torch.equal(got[5], img & 0xE0)
    assert (got[7] == 0).all() and (got[8] == 0).all()


def test_bad_arguments_return_invalid():
    lib = N.lib()
    u8 = IMAGES["noise24"][None].contiguous().cuda()
    ta, prm = D.trivial_augment_identity(1).cuda(), no_erase(1, 24).cuda()
    out, work = torch.zeros(1, 3, 24, 24, device="cuda"), torch.zeros(1, 4, 256, dtype=torch.int32, device="cuda")

    def call(u=u8, t=ta, p=prm, o=out, w=work, B=1, Sh=24, Sw=24):
        return lib.vt_trivial_augment(vp(u), vp(t), vp(p), vp(o), vp(w), B, Sh, Sw, None, stream())

    assert call() == N.VT_OK
    for kw, word in (({"u": None}, "null"), ({"t": None}, "null"), ({"p": None}, "null"), ({"o": None}, "null"),
                     ({"w": None}, "null"), ({"B": 0}, "size"), ({"Sh": 0}, "size"), ({"Sw": -1}, "size"),
                     ({"Sh": 1 << 16, "Sw": 1 << 15}, "pixels")):
        assert call(**kw) == N.VT_ERR_INVALID, kw
        assert "vt_trivial_augment" in N.last_error() and word in N.last_error(), (kw, N.last_error())
    raw = D.RaggedBatch.from_images([IMAGES["noise24"]]).to("cuda")
    assert lib.vt_augment_batch_u8(vp(raw.raw), vp(raw.table), None, vp(u8), 1, 24, 24, 1, 0, stream()) == N.VT_ERR_INVALID
    assert "vt_augment_batch_u8" in N.last_error()
    torch.cuda.synchronize()


# ---- vt_augment_batch_u8 -----------------------------------------------------------------------------------------------
# (case of test_augment_gpu.py, rows of it): downscales with weights that are no dyadic fractions, the 1 x 1 crops, flips, the
# validation window, plain bilinear; none of them has a filtered value within 1e-4 of a half level (asserted below)
U8_CASES = {"whole16": [3, 5], "boxes24": [4, 5, 6, 7, 8, 9, 10, 11], "nonsquare": [0, 3, 5], "flips": [0, 4],
            "flips_odd": [0, 1, 2], "validation": [0, 2], "bilinear": [0]}


def _u8_case(name):
    if name == "bands":  # two row bands and two column tiles an image, small enough to have no value near a half level
        return [TG.IMAGES[5]] * 2, [AU.row(4, 4, 280, 390, 9, 257), AU.row(5, 4, 280, 390, 9, 257, flip=1)], 9, 257, True
    idx, rows, Sh, Sw, aa, _ = TG.CASES[name]
    keep = U8_CASES[name]
    return [TG.IMAGES[idx[k]] for k in keep], [rows[k] for k in keep], Sh, Sw, aa


def launch_u8(images, rows, Sh, Sw, antialias=True, lds=0):
    batch = D.RaggedBatch.from_images(images).to("cuda")
    params = AU.params_tensor(rows).cuda()
    B = len(images)
    big = torch.full((B + 2, Sh, Sw, 3), 0xAB, dtype=torch.uint8, device="cuda")
    out = big[1 : B + 1]

    def run():
        N.check(N.lib().vt_augment_batch_u8(vp(batch.raw), vp(batch.table), vp(params), vp(out), B, Sh, Sw, int(antialias), lds, stream()))
        torch.cuda.synchronize()
        return out.clone()

    first = run()
    assert torch.equal(run(), first), "two launches differ"
    assert (big[0] == 0xAB).all() and (big[B + 1] == 0xAB).all()
    return first.cpu()


@pytest.mark.parametrize("name", list(U8_CASES) + ["bands"])
def test_u8_entry_gives_the_rounded_levels(name):
    images, rows, Sh, Sw, aa = _u8_case(name)
    params = AU.params_tensor(rows)
    v255 = AU.reference_batch(images, params, Sh, Sw, aa) * 255.0
    away = ((v255 - torch.floor(v255)) - 0.5).abs().min().item()
    assert away > 1e-4, (name, away)  # the choice of the cases: float32 error (< 1e-4 levels) cannot cross a half level
    host = D.GPUBatchTransform((Sh, Sw), antialias=aa)._levels_torch(D.RaggedBatch.from_images(images), params)
    assert torch.equal(host, torch.floor(v255 + 0.5).permute(0, 2, 3, 1).to(torch.uint8))
    got = launch_u8(images, rows, Sh, Sw, aa)
    diff = (got.int() - host.int()).abs()
    n = int((diff > 0).sum())
    print(f"{name}: {n} of {diff.numel()} levels differ, at most {int(diff.max())} apart (bounds: 1 in 10,000, 1 level)")
    assert int(diff.max()) <= 1 and n * 10000 <= diff.numel()
    low = launch_u8(images, rows, Sh, Sw, aa, lds=TG.lds_for_rows(Sh, Sw, 2))
    assert torch.equal(low, got), "the chunked plan changed levels"


def test_u8_entry_copies_a_source_that_is_already_the_output():
    imgs = [IMAGES["noise24"], TG.IMAGES[4]]  # 24 x 24 and 20 x 20
    for im, S in ((imgs[0], 24), (imgs[1], 20)):
        rows = [AU.row(0, 0, S, S, S, S), AU.row(0, 0, S, S, S, S, flip=1)]
        for aa in (True, False):
            got = launch_u8([im, im], rows, S, S, aa)
            assert torch.equal(got[0], im) and torch.equal(got[1], im.flip(1)), (S, aa)
    # an erase box in params is ignored, a row that names no image gives zeros
    batch = D.RaggedBatch.from_images([imgs[0], imgs[0]])
    table = batch.table.clone()
    table[1, 1] = 0
    prm = AU.params_tensor([AU.row(0, 0, 24, 24, 24, 24, erase=(2, 2, 9, 9), mode=D.ERASE_CONSTANT)] * 2).cuda()
    out = torch.full((2, 24, 24, 3), 0xAB, dtype=torch.uint8, device="cuda")
    raw, table = batch.raw.cuda(), table.cuda()  # (held in names: a temporary's memory would be reused by the next one)
    N.check(N.lib().vt_augment_batch_u8(vp(raw), vp(table), vp(prm), vp(out), 2, 24, 24, 1, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), imgs[0]) and (out[1] == 0).all()


# ---- the module ----------------------------------------------------------------------------------------------------------
def _module_case():
    images, rows, Sh, Sw, aa = _u8_case("nonsquare")  # (no value near a half level: both sides round to the same levels)
    E = D.ERASE_RANDOM
    rows = [list(r) for r in rows]
    rows[0][9:16] = [2, 3, 5, 9, E, 7, 0]
    rows[2][9:16] = [0, 0, Sh - 1, Sw - 1, D.ERASE_CONSTANT, 0, AU.f32_bits(0.25)]
    ta = TU.table([(D.TA_EQUALIZE, 0.0), (D.TA_ROTATE, -31.5), (D.TA_CONTRAST, 0.66)], Sh, Sw)
    return images, AU.params_tensor(rows), ta, Sh, Sw


def test_module_with_a_table_on_cuda_against_its_cpu_path():
    images, params, ta, Sh, Sw = _module_case()
    batch = D.RaggedBatch.from_images(images)
    for kw in ({}, {"mean": MEAN_STD[:3], "std": MEAN_STD[3:]}):
        aug = D.GPUBatchTransform((Sh, Sw), **kw)
        ref = aug(batch, params, ta=ta)
        before = N.launch_count()
        got = aug(batch.to("cuda"), params, ta=ta)
        assert N.launch_count() == before + 3  # the u8 launch, the statistics pass, the apply pass
        assert got.is_cuda and got.dtype == torch.float32
        l2, linf = AU.errors(got.cpu(), ref)
        assert l2 <= 2e-5 and linf <= 2e-5, (kw, l2, linf)
        box = torch.zeros(3, 3, Sh, Sw, dtype=torch.bool)
        box[0, :, 2:7, 3:12] = True  # the random erase: accurate f32 functions on both sides, not the same bits
        if not kw:
            assert torch.equal(got.cpu()[~box], ref[~box])
        # a device table is used as it is, the cached buffers serve the second call
        again = aug(batch.to("cuda"), params.cuda(), ta=ta.cuda())
        assert torch.equal(again, got) and len(aug._ta_buffers) == 1
    with pytest.raises(ValueError, match=r"ta\[1\]\.op"):
        bad = ta.clone()
        bad[1, 0] = 14.0
        aug(batch.to("cuda"), params, ta=bad)


def test_module_without_a_table_is_the_one_launch_path():
    images, params, _, Sh, Sw = _module_case()
    batch = D.RaggedBatch.from_images(images).to("cuda")
    aug = D.GPUBatchTransform((Sh, Sw), mean=MEAN_STD[:3], std=MEAN_STD[3:])
    before = N.launch_count()
    got = aug(batch, params, ta=None)
    assert N.launch_count() == before + 1
    direct = torch.full((3, 3, Sh, Sw), float("nan"), device="cuda")
    ms = torch.tensor(MEAN_STD, dtype=torch.float32, device="cuda")
    dprm = params.cuda()
    N.check(N.lib().vt_augment_batch(vp(batch.raw), vp(batch.table), vp(dprm), vp(direct), 3, Sh, Sw, 1, vp(ms), 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, direct) and torch.equal(aug(batch, params), direct)
