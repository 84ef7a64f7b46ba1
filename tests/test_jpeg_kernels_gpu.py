"""vt_jpeg_entropy and vt_jpeg_idct_rgb through the C-ABI against the host stage (data.jpeg_decode_coefficients / the fixture's
PIL arrays, which tests/test_jpeg_cpu.py holds to each other level for level).

Bounds: none.  Coefficients and levels are integers from one definition: torch.equal.  Every launch pair runs twice, into two
differently placed output buffers, and must give the same bits.  The coefficient scratch is pre-filled with 0xA5 bytes and lies
between 0xA5 guards; `raw` lies between 0xA5 guards at an odd byte offset the first time, and at an odd byte offset at the very
end of its allocation the second time; the per-segment statuses are pre-filled with garbage.  Guards must stay intact and every
coefficient, pixel and status must have been written.

The damaged streams run ONCE, in one batch: a handful of those that tests/test_jpeg_cpu.py has already run through the same
decoder source (csrc/vt_jpeg_bits.h) under the host sanitizers."""
import copy

import pytest
import torch

import jpeg_util as JU
from gpu_util import stream, vp
from vision_toolbox import _native as N
from vision_toolbox import data as D

pytestmark = pytest.mark.gpu

CASES = JU.cases()
GUARD = 256  # bytes
A5_16 = -23131  # 0xA5A5 as int16


def _info_of(s):
    """a Stream's header with the stream's own (possibly damaged) tables in it, for JpegBatch.from_bytes"""
    if isinstance(s, JU.Case):
        return s.info
    info = copy.copy(s.info)
    info.huff = s.huff
    info.segments = [(b, e) for b, e, _, _ in s.segments]
    assert D.jpeg_segment_table(info) == list(s.segments)
    return info


def pack(items):
    return D.JpegBatch.from_bytes([s.data for s in items], infos=[_info_of(s) for s in items])


def launch(jb, band=0, idct=True):
    """the two launches, twice; returns (coef int16 [blocks, 64], raw uint8 [raw_bytes], status int32 [S]) on the host"""
    dev = "cuda"
    data, images, segments, qtabs, hufftabs = (t.to(dev) for t in (jb.data, jb.images, jb.segments, jb.qtabs, jb.hufftabs))
    S, ncoef, g16 = segments.shape[0], jb.blocks * 64, GUARD // 2
    results = []
    for rep in range(2):
        cbuf = torch.full((g16 + ncoef + g16,), A5_16, dtype=torch.int16, device=dev)
        coef = cbuf[g16 : g16 + ncoef]
        pre = GUARD + 1
        rbuf = torch.full((pre + jb.raw_bytes + (GUARD if rep == 0 else 0),), 0xA5, dtype=torch.uint8, device=dev)
        raw = rbuf[pre : pre + jb.raw_bytes]
        assert raw.data_ptr() % 2 == 1 and coef.data_ptr() % 16 == 0
        status = torch.full((S + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        N.check(N.lib().vt_jpeg_entropy(vp(data), data.numel(), vp(images), len(jb), vp(segments), S, vp(hufftabs), hufftabs.shape[0],
                                        vp(coef), jb.blocks, vp(status[1:]), stream()))
        if idct:
            N.check(N.lib().vt_jpeg_idct_rgb(vp(coef), jb.blocks, vp(images), len(jb), vp(qtabs), qtabs.shape[0], vp(raw), jb.raw_bytes,
                                             jb.max_mcus_x, jb.max_mcus_y, band, stream()))
        torch.cuda.synchronize()
        assert bool((cbuf[:g16] == A5_16).all()) and bool((cbuf[g16 + ncoef :] == A5_16).all()), "a guard of the scratch was written"
        assert bool((rbuf[:pre] == 0xA5).all()) and bool((rbuf[pre + jb.raw_bytes :] == 0xA5).all()), "a guard of raw was written"
        assert status[0].item() == 0x5A5A5A5A and status[-1].item() == 0x5A5A5A5A
        results.append((coef.cpu().view(-1, 64), raw.cpu(), status[1:-1].cpu()))
    (c0, r0, s0), (c1, r1, s1) = results
    assert torch.equal(c0, c1) and torch.equal(r0, r1) and torch.equal(s0, s1), "two launches differ"
    return c0, r0, s0


def expect(items):
    coef = torch.cat([s.host[0] for s in items])
    status = [st for s in items for st in s.host[1]]
    return coef, status


def check_clean(items, band=0):
    jb = pack(items)
    coef, raw, status = launch(jb, band)
    want_coef, want_status = expect(items)
    assert status.tolist() == want_status == [0] * len(want_status)
    assert torch.equal(coef, want_coef), int((coef != want_coef).sum())
    ref = D.RaggedBatch.from_images([c.rgb for c in items])
    assert jb.raw_bytes == ref.raw.numel()
    assert torch.equal(raw, ref.raw), (int((raw != ref.raw).sum()), int((raw.int() - ref.raw.int()).abs().max()))
    assert jb.images[:, D.JI_OUT].tolist() == ref.table[:, 0].tolist()


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_is_the_host_stage_and_pil(name):
    check_clean([CASES[name]])


def test_mixed_batch():
    check_clean(JU.mixed())


def test_every_case_in_one_batch():
    check_clean(list(CASES.values()))


@pytest.mark.parametrize("band", [1, 2, 3, 4])
def test_band_split_does_not_change_the_result(band):
    # 40 x 48 at 4:2:0 is three MCU rows: bands of one and of two rows both cut it, the default (four) does not
    items = [CASES["420_40x48_noise_q90"], CASES["420_53x37_noise_q90_r3"], CASES["422_53x37_noise_q90"], CASES["444_53x37_noise_q5"],
             CASES["gray_17x9_noise_q90"], CASES["420_4x16_noise_q90"], CASES["420_1x16_noise_q90"], CASES["422_4x16_noise_q90"]]
    assert items[0].info.mcu_geometry[3] == 3
    check_clean(items, band)


def test_wide_image_crosses_the_column_tiles():
    # 80 x 8 gray is ten MCU columns: two tiles of eight
    assert CASES["gray_80x8_noise_q90_r1"].info.mcu_geometry[2] == 10
    check_clean([CASES["gray_80x8_noise_q90_r1"], CASES["gray_80x8_noise_q90_r3"]])


def test_idct_of_arbitrary_coefficients_is_the_host_stage():
    """vt_jpeg_idct_rgb alone on a scratch of uniform random int16 -- far beyond what an image gives, as a damaged stream can
    leave it: the kernel's arithmetic is modulo 2^32 with no signed overflow, and the host stage (exact int64 sums reduced to 32
    bits before each shift) is the same function, so the pixels are equal.  One 4:2:0 and one gray geometry, quality 5 tables
    (entries up to 255)."""
    items = [CASES["420_53x37_noise_q5"], CASES["gray_17x9_noise_q5"]]
    jb = pack(items)
    coef = torch.randint(-32768, 32768, (jb.blocks, 64), dtype=torch.int16, generator=torch.Generator().manual_seed(5))
    coef[:3] = 32767
    coef[3:6] = -32768
    want, at = [], 0
    for c in items:
        hm, vm, mx, my = c.info.mcu_geometry
        n = mx * my * (hm * vm + (2 if len(c.info.components) == 3 else 0))
        want.append(D.jpeg_pixels(coef[at : at + n], c.info).reshape(-1))
        at += n
    want = torch.cat(want)
    assert at == jb.blocks and 0 < int((want == 0).sum()) and 0 < int((want == 255).sum()) and len(want.unique()) > 200
    dcoef, images, qtabs = coef.cuda(), jb.images.cuda(), jb.qtabs.cuda()
    rbuf = torch.full((GUARD + 1 + jb.raw_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    raw = rbuf[GUARD + 1 : GUARD + 1 + jb.raw_bytes]
    for band in (0, 1):
        N.check(N.lib().vt_jpeg_idct_rgb(vp(dcoef), jb.blocks, vp(images), len(jb), vp(qtabs), qtabs.shape[0], vp(raw), jb.raw_bytes,
                                         jb.max_mcus_x, jb.max_mcus_y, band, stream()))
        torch.cuda.synchronize()
        assert torch.equal(raw.cpu(), want), int((raw.cpu() != want).sum())
    assert bool((rbuf[: GUARD + 1] == 0xA5).all()) and bool((rbuf[GUARD + 1 + jb.raw_bytes :] == 0xA5).all())


def test_damaged_streams_end_with_their_status_and_zeros():
    """one truncation, one byte of each kind, an over-subscribed table and an empty segment table per file, all in ONE batch and
    one run of the two launches"""
    every = {s.label: s for s in JU.damaged_streams()}
    picked = []
    for name in JU.DAMAGE_FILES:
        cuts = [s for l, s in every.items() if l.startswith(name + "[:")]
        picked.append(cuts[len(cuts) // 2])
        for tail in ("=00", "=FF", "=D9"):
            picked.append([s for l, s in every.items() if l.startswith(name + "[") and l.endswith(tail)][1])
        picked += [every[name + " oversubscribed"], every[name + " empty"]]
    assert len(picked) == 18
    jb = pack(picked)
    dev = "cuda"
    data, images, segments, qtabs, hufftabs = (t.to(dev) for t in (jb.data, jb.images, jb.segments, jb.qtabs, jb.hufftabs))
    S, ncoef, g16 = segments.shape[0], jb.blocks * 64, GUARD // 2
    cbuf = torch.full((g16 + ncoef + g16,), A5_16, dtype=torch.int16, device=dev)
    coef = cbuf[g16 : g16 + ncoef]
    rbuf = torch.full((GUARD + 1 + jb.raw_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    raw = rbuf[GUARD + 1 : GUARD + 1 + jb.raw_bytes]
    status = torch.full((S + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    N.check(N.lib().vt_jpeg_entropy(vp(data), data.numel(), vp(images), len(jb), vp(segments), S, vp(hufftabs), hufftabs.shape[0],
                                    vp(coef), jb.blocks, vp(status[1:]), stream()))
    N.check(N.lib().vt_jpeg_idct_rgb(vp(coef), jb.blocks, vp(images), len(jb), vp(qtabs), qtabs.shape[0], vp(raw), jb.raw_bytes,
                                     jb.max_mcus_x, jb.max_mcus_y, 0, stream()))
    torch.cuda.synchronize()
    assert bool((cbuf[:g16] == A5_16).all()) and bool((cbuf[g16 + ncoef :] == A5_16).all())
    assert bool((rbuf[: GUARD + 1] == 0xA5).all()) and bool((rbuf[GUARD + 1 + jb.raw_bytes :] == 0xA5).all())
    assert status[0].item() == 0x5A5A5A5A and status[-1].item() == 0x5A5A5A5A
    want_coef, want_status = expect(picked)
    got_status = status[1:-1].tolist()
    assert got_status == want_status
    per_image = [max(got_status[r[D.JI_SEG0] : r[D.JI_SEG0] + r[D.JI_NSEG]]) for r in jb.images.tolist()]
    assert all(st != 0 for st in per_image), per_image
    assert torch.equal(coef.cpu().view(-1, 64), want_coef)  # zeros from the failing block of a segment on included
    for s, r in zip(picked, jb.images.tolist()):
        if s.label.endswith((" oversubscribed", " empty")):  # nothing decoded: mid-gray (gray) or its colour conversion
            H, W = r[D.JI_H], r[D.JI_W]
            px = raw[r[D.JI_OUT] : r[D.JI_OUT] + H * W * 3]
            assert bool((px == 128).all()), s.label


def test_rows_out_of_range_write_nothing_but_their_status():
    """an unvalidated device table: a segment naming no image, a byte range that leaves the data, MCUs past the image, and an
    image whose blocks leave the scratch.  Each gets status 4; no coefficient, no pixel is written for it."""
    items = [CASES["gray_17x9_noise_q90"], CASES["420_17x17_noise_q90"], CASES["gray_8x8_noise_q90"]]
    jb = pack(items)
    dev = "cuda"
    seg = jb.segments.clone()
    assert seg.shape[0] == 3
    extra = seg[0].clone().repeat(4, 1)
    extra[0, 0] = len(jb)                      # no such image
    extra[1, 2] = jb.data.numel() + 1          # ends past the data
    extra[2, 1], extra[2, 2] = 40, 39          # begin > end
    extra[3, 4] = 1000                         # more MCUs than the image has
    seg = torch.cat([seg, extra])
    img = jb.images.clone()
    img[2, D.JI_COEF] = jb.blocks              # its one block would lie past the scratch
    data, images, segments, qtabs, hufftabs = (t.to(dev) for t in (jb.data, img, seg, jb.qtabs, jb.hufftabs))
    S, ncoef, g16 = segments.shape[0], jb.blocks * 64, GUARD // 2
    cbuf = torch.full((g16 + ncoef + g16,), A5_16, dtype=torch.int16, device=dev)
    coef = cbuf[g16 : g16 + ncoef]
    rbuf = torch.full((GUARD + jb.raw_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    raw = rbuf[GUARD : GUARD + jb.raw_bytes]
    status = torch.full((S,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    N.check(N.lib().vt_jpeg_entropy(vp(data), data.numel(), vp(images), len(jb), vp(segments), S, vp(hufftabs), hufftabs.shape[0],
                                    vp(coef), jb.blocks, vp(status), stream()))
    N.check(N.lib().vt_jpeg_idct_rgb(vp(coef), jb.blocks, vp(images), len(jb), vp(qtabs), qtabs.shape[0], vp(raw), jb.raw_bytes,
                                     jb.max_mcus_x, jb.max_mcus_y, 0, stream()))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 4, 4, 4, 4, 4]
    assert bool((cbuf[:g16] == A5_16).all()) and bool((cbuf[g16 + ncoef :] == A5_16).all())
    assert bool((rbuf[:GUARD] == 0xA5).all()) and bool((rbuf[GUARD + jb.raw_bytes :] == 0xA5).all())
    want = torch.cat([items[0].host[0], items[1].host[0]])
    got = coef.cpu().view(-1, 64)
    assert torch.equal(got[: want.shape[0]], want) and bool((got[want.shape[0] :] == A5_16).all())
    ref = D.RaggedBatch.from_images([c.rgb for c in items[:2]]).raw
    got_raw = raw.cpu()
    assert torch.equal(got_raw[: ref.numel()], ref) and bool((got_raw[ref.numel() :] == 0xA5).all())


def test_argument_checks():
    jb = pack([CASES["420_17x17_noise_q90"]])
    dev = "cuda"
    data, images, segments, qtabs, hufftabs = (t.to(dev) for t in (jb.data, jb.images, jb.segments, jb.qtabs, jb.hufftabs))
    coef = torch.zeros(jb.blocks * 64 + 8, dtype=torch.int16, device=dev)
    raw = torch.zeros(jb.raw_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    lib, before = N.lib(), N.launch_count()

    def entropy(**kw):
        a = dict(data=vp(data), nbytes=data.numel(), images=vp(images), B=1, segments=vp(segments), S=1, huff=vp(hufftabs),
                 NH=hufftabs.shape[0], coef=vp(coef), blocks=jb.blocks, status=vp(status))
        a.update(kw)
        return lib.vt_jpeg_entropy(a["data"], a["nbytes"], a["images"], a["B"], a["segments"], a["S"], a["huff"], a["NH"], a["coef"],
                                   a["blocks"], a["status"], stream())

    def idct(**kw):
        a = dict(coef=vp(coef), blocks=jb.blocks, images=vp(images), B=1, q=vp(qtabs), NQ=qtabs.shape[0], raw=vp(raw),
                 nbytes=jb.raw_bytes, mx=jb.max_mcus_x, my=jb.max_mcus_y, band=0)
        a.update(kw)
        return lib.vt_jpeg_idct_rgb(a["coef"], a["blocks"], a["images"], a["B"], a["q"], a["NQ"], a["raw"], a["nbytes"], a["mx"], a["my"],
                                    a["band"], stream())

    for k in ("data", "images", "segments", "huff", "coef", "status"):
        assert entropy(**{k: None}) == N.VT_ERR_INVALID and k in N.last_error().replace("hufftabs", "huff")
    for k in ("nbytes", "B", "S", "NH", "blocks"):
        assert entropy(**{k: 0}) == N.VT_ERR_INVALID and "non-positive" in N.last_error()
    assert entropy(coef=vp(coef[1:])) == N.VT_ERR_INVALID and "misaligned" in N.last_error()
    assert entropy(data=vp(data[1:])) == N.VT_ERR_INVALID and "misaligned" in N.last_error()
    assert entropy(status=vp(status.view(torch.int16)[1:])) == N.VT_ERR_INVALID
    for k in ("coef", "images", "q", "raw"):
        assert idct(**{k: None}) == N.VT_ERR_INVALID and "null" in N.last_error()
    for k in ("blocks", "B", "NQ", "nbytes", "mx", "my"):
        assert idct(**{k: 0}) == N.VT_ERR_INVALID and "non-positive" in N.last_error()
    assert idct(coef=vp(coef[4:])) == N.VT_ERR_INVALID and "misaligned" in N.last_error()
    for band in (-1, 5):
        assert idct(band=band) == N.VT_ERR_INVALID and "band_mcu_rows" in N.last_error()
    assert idct(B=65536) == N.VT_ERR_INVALID and "grid" in N.last_error()
    assert N.launch_count() == before  # nothing was launched
    assert entropy() == N.VT_OK and idct() == N.VT_OK
    torch.cuda.synchronize()
    assert N.launch_count() == before + 2
    assert torch.equal(raw.cpu(), CASES["420_17x17_noise_q90"].rgb.reshape(-1))
