"""Baseline JPEG decoding without a GPU: the host stage (data.jpeg_decode_levels) against PIL, LEVEL FOR LEVEL, the marker
parse, the segment table, the batch tables, every refusal, and the entropy stage's C++ (csrc/vt_jpeg_bits.h, the code the kernel
runs) as a stand-alone program under the host sanitizers.

The yardstick is libjpeg's default decode as PIL returns it (Image.open(...).convert("RGB")).  Both sides are integer arithmetic
from one definition (Huffman decode, jidctint, the triangle upsampling filters, the 16-bit fixed-point colour tables), so the bound
is equality: 0 differing levels, torch.equal.  The fixture (tests/golden/jpeg_cases.npz, tools/gen_golden_jpeg.py) holds PIL's
arrays, so the equality is checked where PIL is not installed too; where it is, the fixture is re-decoded and must not have moved.

The stand-alone program is compiled here with -fsanitize=address,undefined and run as a child process (nothing is preloaded);
each case's bytes live in a heap block of exactly their length.  It decodes every fixture stream and the damaged streams of
jpeg_util.damaged_streams; coefficients and statuses must equal the host stage's, and every damaged stream must end nonzero."""
import io
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import jpeg_util as JU
from vision_toolbox import _native as N
from vision_toolbox import data as D

ROOT = Path(__file__).resolve().parents[1]
CASES = JU.cases()
NAMES = list(CASES)
COLOUR = CASES["420_53x37_noise_q90"].data
GRAY = CASES["gray_17x9_noise_q90"].data


# ---- the host stage against PIL -----------------------------------------------------------------------------------------
def test_the_fixture_has_the_cases_the_kernels_can_get_wrong():
    st = [c.settings for c in CASES.values()]
    sizes = {s: {(c["W"], c["H"]) for c in st if c["sampling"] == s} for s in ("gray", "444", "422", "420")}
    assert {(1, 1), (8, 8), (7, 5), (17, 9), (80, 8)} <= sizes["gray"]
    assert {(8, 8), (53, 37)} <= sizes["444"]
    assert {(16, 8), (33, 16), (53, 37)} <= sizes["422"]
    assert {(1, 1), (2, 2), (16, 16), (17, 17), (40, 48), (53, 37)} <= sizes["420"]
    # chroma planes of one and two columns (replicated by libjpeg, not filtered) with more than one chroma row, and the first
    # widths with three columns (filtered)
    assert {(3, 5), (4, 16), (2, 9), (5, 5), (6, 3)} <= sizes["422"]
    assert {(1, 16), (3, 5), (4, 16), (2, 7), (5, 5), (6, 9)} <= sizes["420"]
    for s in ("gray", "444", "422", "420"):
        assert {c["quality"] for c in st if c["sampling"] == s} >= {5, 75, 90, 100}
        assert {c["source"] for c in st if c["sampling"] == s} == {"noise", "gradient", "constant"}
        assert any(c["optimize"] for c in st if c["sampling"] == s)
    for s, size in (("gray", (80, 8)), ("420", (53, 37))):
        assert {c["restart"] for c in st if c["sampling"] == s and (c["W"], c["H"]) == size} >= {1, 2, 3}
    assert sum(c["spliced"] for c in st) == 1
    assert len(JU.mixed()) == 7 and {c.settings["sampling"] for c in JU.mixed()} == {"gray", "444", "422", "420"}
    # noise forces byte stuffing: a stuffed FF 00 pair inside a scan
    assert any(b"\xff\x00" in c.data[c.info.scan_offset : c.info.scan_end] for c in CASES.values())
    # ten segments on 80 x 8 gray with an interval of one block: RST0 .. RST7 wraps
    assert len(D.jpeg_segment_table(CASES["gray_80x8_noise_q90_r1"].info)) == 10
    # 53 x 37 at 4:2:0 is 4 MCUs a row: an interval of 3 does not divide it
    assert CASES["420_53x37_noise_q90_r3"].info.mcu_geometry == (2, 2, 4, 3)


@pytest.mark.parametrize("name", NAMES)
def test_host_stage_is_pil_level_for_level(name):
    c = CASES[name]
    got, status = D.jpeg_decode_levels(c.data, return_status=True)
    assert status == 0
    assert got.dtype == torch.uint8 and tuple(got.shape) == (c.settings["H"], c.settings["W"], 3)
    assert torch.equal(got, c.rgb), (name, int((got != c.rgb).sum()), int((got.int() - c.rgb.int()).abs().max()))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_a_fresh_pil_decode(name):
    pytest.importorskip("PIL")
    import numpy as np
    from PIL import Image

    fresh = torch.from_numpy(np.array(Image.open(io.BytesIO(CASES[name].data)).convert("RGB")))
    assert torch.equal(fresh, CASES[name].rgb)


def test_narrow_subsampled_images_against_pil():
    """libjpeg filters a chroma plane only if it is more than two samples wide: every width from 1 to 9 (one to five chroma
    columns) at heights with one, two and many chroma rows, both sub-sampled modes, fresh from PIL"""
    pytest.importorskip("PIL")
    import numpy as np
    from PIL import Image

    for sub in (1, 2):
        for W in range(1, 10):
            for H in (1, 2, 3, 5, 16, 17):
                px = np.random.default_rng(100 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
                buf = io.BytesIO()
                Image.fromarray(px).save(buf, "JPEG", quality=90, subsampling=sub)
                ref = torch.from_numpy(np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
                got = D.jpeg_decode_levels(buf.getvalue())
                assert torch.equal(got, ref), (sub, W, H, int((got != ref).sum()))


def test_sof1_and_a_gray_frame_with_sampling_factors():
    """SOF1 with 8-bit tables is the same decode as SOF0; a single component's factors (here 2x2) only scale an MCU that is one
    block anyway, and jpeg_info reports them as 1x1 -- before and after jpeg_check, which changes nothing in the header"""
    c = CASES["420_53x37_noise_q90"]
    sof1 = c.data.replace(b"\xff\xc0", b"\xff\xc1", 1)
    assert D.jpeg_info(sof1).sof == 0xC1 and torch.equal(D.jpeg_decode_levels(sof1), c.rgb)
    g = CASES["gray_17x9_noise_q90"]
    i = g.data.index(b"\xff\xc0")
    assert g.data[i + 9] == 1 and g.data[i + 11] == 0x11
    g22 = g.data[: i + 11] + b"\x22" + g.data[i + 12 :]
    info = D.jpeg_info(g22)
    before = (list(info.components), info.mcu_geometry)
    D.jpeg_check(info)
    assert (list(info.components), info.mcu_geometry) == before == ([(1, 1, 1, 0)], (1, 1, 3, 2))
    assert torch.equal(D.jpeg_decode_levels(g22), g.rgb)
    batch = D.decode_jpeg_batch([sof1, g22], "cpu")
    assert torch.equal(batch.raw, D.RaggedBatch.from_images([c.rgb, g.rgb]).raw)


def test_bytes_behind_eoi_are_not_a_second_scan():
    """a trailer or a second image behind EOI (MPO files, appended thumbnails) is not part of this image"""
    c = CASES["420_53x37_noise_q90_r3"]
    for tail in (b"..\xff\xda..", c.data, CASES["gray_17x9_noise_q90"].data + b"\xff\xda\x00"):
        info = D.jpeg_info(c.data + tail)
        assert info.scans == 1 and info.scan_end == c.info.scan_end
        assert torch.equal(D.jpeg_decode_levels(c.data + tail), c.rgb)


def test_idct_of_coefficients_beyond_any_image_is_defined():
    """a damaged stream can leave any int16 in the scratch: the IDCT is then modulo-2^32 arithmetic, the same on both sides
    (tests/test_jpeg_kernels_gpu.py compares the kernel) -- and exactly jidctint wherever nothing wraps"""
    big = torch.full((1, 64), 32767, dtype=torch.int16)
    out = D.jpeg_idct_blocks(big, [255] * 64)
    assert out.min() >= 0 and out.max() <= 255
    # DC only, in range: every sample is (dc * q + 4) >> 3, + 128
    dc = torch.zeros((1, 64), dtype=torch.int16)
    dc[0, 0] = -37
    assert bool((D.jpeg_idct_blocks(dc, [3] * 64) == ((-37 * 3 + 4) >> 3) + 128).all())


def test_gray_is_written_to_all_three_channels():
    got = D.jpeg_decode_levels(GRAY)
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])


# ---- the marker parse ---------------------------------------------------------------------------------------------------------
SAMPLING_FACTORS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}


@pytest.mark.parametrize("name", NAMES)
def test_jpeg_info_against_the_generator_settings(name):
    c, s = CASES[name], CASES[name].settings
    info = D.jpeg_info(c.data)
    assert (info.width, info.height, info.precision) == (s["W"], s["H"], 8)
    assert info.sof in (0xC0, 0xC1) and info.scans == 1 and info.spectral == (0, 63, 0, 0)
    assert [(h, v) for _, h, v, _ in info.components] == SAMPLING_FACTORS[s["sampling"]]
    assert info.sampling == {"gray": "gray", "444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}[s["sampling"]]
    assert info.restart_interval == s["restart"]
    hm, vm = SAMPLING_FACTORS[s["sampling"]][0]
    assert info.mcu_geometry == (hm, vm, -(-s["W"] // (8 * hm)), -(-s["H"] // (8 * vm)))
    assert c.data[info.scan_offset - 2 - 2 * len(info.components) - 6 : info.scan_offset - 2 * len(info.components) - 6] == b"\xff\xda"
    assert c.data[info.scan_end : info.scan_end + 1] == b"\xff"
    for prec, tab in info.qtabs.values():
        assert prec == 8 and len(tab) == 64 and all(1 <= v <= 255 for v in tab)
    if s["quality"] == 100:
        assert all(v == 1 for _, tab in info.qtabs.values() for v in tab)
    for (tc, _), (bits, vals) in info.huff.items():
        assert tc in (0, 1) and len(bits) == 16 and sum(bits) == len(vals)
    # the standard luminance DC table has 12 values; an optimised one of a small image has fewer
    std_dc = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12)))
    assert (info.huff[(0, 0)] == std_dc) == (not s["optimize"])


def test_quantisation_tables_are_de_zigzagged():
    # the standard luminance table at quality 50 scaled to 75: its first row in natural order starts 8, 6, 5, 8 and the
    # first column 8, 6, 7, 7 (zigzag would interleave them)
    _, tab = D.jpeg_info(CASES["gray_17x9_noise_q75"].data).qtabs[0]
    assert tab[:4] == [8, 6, 5, 8] and [tab[0], tab[8], tab[16], tab[24]] == [8, 6, 7, 7]


def _direct_segments(data, begin):
    """the scan's segments by walking the bytes one at a time: (first byte, one past the last data byte) per segment"""
    segs, i, start = [], begin, begin
    while i < len(data):
        if data[i] != 0xFF:
            i += 1
            continue
        j = i
        while j < len(data) and data[j] == 0xFF:
            j += 1
        if j >= len(data):
            break
        if data[j] == 0x00 and j == i + 1:
            i = j + 1
            continue
        segs.append((start, i))  # a marker: the run of FFs from i belongs to it
        if not 0xD0 <= data[j] <= 0xD7:
            return segs
        start = i = j + 1
    segs.append((start, len(data)))
    return segs


@pytest.mark.parametrize("name", [n for n in NAMES if "_r" in n] + ["420_53x37_noise_q90", "gray_1x1_noise_q90"])
def test_segment_table_against_a_direct_marker_scan(name):
    c = CASES[name]
    info = c.info
    direct = _direct_segments(c.data, info.scan_offset)
    table = D.jpeg_segment_table(info)
    assert [(b, e) for b, e, _, _ in table] == direct
    _, _, mx, my = info.mcu_geometry
    Ri = info.restart_interval or mx * my
    assert len(table) == -(-mx * my // Ri)
    assert [m0 for _, _, m0, _ in table] == list(range(0, mx * my, Ri))
    assert sum(mc for _, _, _, mc in table) == mx * my and all(1 <= mc <= Ri for _, _, _, mc in table)
    # no segment holds a marker; the byte in front of each later segment is RSTn, n counting modulo 8
    for k, (b, e, _, _) in enumerate(table):
        assert re.search(rb"\xff[^\x00]", c.data[b:e]) is None
        if k:
            assert c.data[b - 2 : b] == bytes([0xFF, 0xD0 + (k - 1) % 8])


def test_spliced_file_has_its_fill_bytes_and_comment():
    c = CASES["420_53x37_noise_q75_r2_spliced"]
    assert c.data[2:4] == b"\xff\xfe" and b"\xff\xff\xff\xc4" in c.data and b"\xff\xff\xff\xff\xd0" in c.data and c.data.endswith(b"\xff\xff\xd9")
    table = D.jpeg_segment_table(c.info)
    assert c.data[table[0][1] : table[0][1] + 5] == b"\xff\xff\xff\xff\xd0" and table[1][0] == table[0][1] + 5


# ---- the batch tables -----------------------------------------------------------------------------------------------------------
def test_batch_tables_and_de_duplication():
    mixed = JU.mixed()
    jb = D.JpegBatch.from_bytes([c.data for c in mixed])
    B = len(mixed)
    assert jb.images.dtype == torch.int64 and tuple(jb.images.shape) == (B, D.JPEG_IMG_FIELDS)
    assert jb.segments.dtype == torch.int64 and jb.segments.shape[1] == D.JPEG_SEG_FIELDS
    assert jb.qtabs.dtype == torch.uint8 and jb.qtabs.shape[1] == 64
    assert jb.hufftabs.dtype == torch.uint8 and jb.hufftabs.shape[1] == D.JPEG_HUFF_BYTES
    # all seven were written at quality 90 with the standard tables: two quantisation tables (luma, chroma) and four Huffman
    # tables for the whole batch, though the files carry 2 * 6 + 1 and 4 * 6 + 2 of them
    assert jb.qtabs.shape[0] == 2 and jb.hufftabs.shape[0] == 4
    two = [c for c in mixed if c.settings["sampling"] == "420"][:2]
    assert two[0].settings["W"] != two[1].settings["W"]
    rows = [jb.images[mixed.index(c)].tolist() for c in two]
    assert rows[0][D.JI_Q0 : D.JI_AC2 + 1] == rows[1][D.JI_Q0 : D.JI_AC2 + 1]
    blocks = out = nseg = 0
    for b, c in enumerate(mixed):
        row, info = jb.images[b].tolist(), c.info
        hm, vm, mx, my = info.mcu_geometry
        assert row[: D.JI_Q0] == [info.height, info.width, len(info.components), hm, vm, mx, my]
        assert (row[D.JI_COEF], row[D.JI_OUT], row[D.JI_SEG0], row[D.JI_RESTART]) == (blocks, out, nseg, info.restart_interval)
        assert row[D.JI_RESTART + 1 :] == [0, 0, 0]
        for cidx, (_, _, _, tq) in enumerate(info.components):
            assert jb.qtabs[row[D.JI_Q0 + cidx]].tolist() == info.qtabs[tq][1]
        for cidx, (_, td, ta) in enumerate(info.scan_components):
            for k, key in enumerate(((0, td), (1, ta))):
                t = bytes(jb.hufftabs[row[D.JI_DC0 + 2 * cidx + k]].tolist())
                assert (t[:16], t[16 : 16 + len(info.huff[key][1])]) == info.huff[key]
        segs = D.jpeg_segment_table(info)
        assert row[D.JI_NSEG] == len(segs)
        start = jb.starts[b]
        assert start % 4 == 0 and bytes(jb.data[start : start + len(c.data)].tolist()) == c.data
        for k, (sb, se, m0, mc) in enumerate(segs):
            assert jb.segments[nseg + k].tolist() == [b, start + sb, start + se, m0, mc, 0]
        blocks += mx * my * (hm * vm + (2 if len(info.components) == 3 else 0))
        out += info.height * info.width * 3
        nseg += len(segs)
    assert (jb.blocks, jb.raw_bytes, jb.segments.shape[0]) == (blocks, out, nseg)
    assert (jb.max_mcus_x, jb.max_mcus_y) == (7, 5)  # 53 x 37 at 4:4:4


def test_cpu_batch_equals_from_images():
    mixed = JU.mixed()
    batch = D.decode_jpeg_batch([c.data for c in mixed], "cpu")
    ref = D.RaggedBatch.from_images([c.rgb for c in mixed])
    assert torch.equal(batch.raw, ref.raw) and torch.equal(batch.table, ref.table) and batch.sizes == ref.sizes
    assert batch.status.dtype == torch.int32 and batch.status.tolist() == [0] * len(mixed)


def test_image_loader_cpu(tmp_path):
    c = CASES["422_53x37_noise_q90"]
    p = tmp_path / "a.jpg"
    p.write_bytes(c.data)
    got = D.image_loader(str(p))
    assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, c.rgb.permute(2, 0, 1))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _patch_sof(data, fn):
    i = data.index(b"\xff\xc0")
    n = 2 + ((data[i + 2] << 8) | data[i + 3])
    seg = bytearray(data[i : i + n])
    fn(seg)
    return data[:i] + bytes(seg) + data[i + n :]


def _set(seg, k, v):
    seg[k] = v


def _drop_segments(data, marker):
    out, pos = bytearray(data[:2]), 2
    while data[pos + 1] != 0xDA:
        L = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] != marker:
            out += data[pos : pos + 2 + L]
        pos += 2 + L
    return bytes(out + data[pos:])


def _second_sos(data):
    info = D.jpeg_info(data)
    i = data.rindex(b"\xff\xda", 0, info.scan_offset)
    return data[: info.scan_end] + data[i : info.scan_end] + data[info.scan_end :]


def _dqt16(data):
    i = data.index(b"\xff\xdb")
    L = (data[i + 2] << 8) | data[i + 3]
    assert L == 67
    wide = bytes([0x10 | data[i + 4]]) + b"".join(bytes([0, v]) for v in data[i + 5 : i + 69])
    return data[:i] + b"\xff\xdb" + (2 + len(wide)).to_bytes(2, "big") + wide + data[i + 2 + L :]


def _one_component_scan(data):
    i = data.index(b"\xff\xda")
    L = (data[i + 2] << 8) | data[i + 3]
    return data[:i] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + data[i + 2 + L :]


REFUSALS = {  # name: (bytes, exception, a pattern naming the property)
    "12-bit": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 4, 12)), NotImplementedError, "12-bit"),
    "progressive SOF": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 1, 0xC2)), NotImplementedError, "progressive"),
    "arithmetic SOF": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 1, 0xC9)), NotImplementedError, "arithmetic"),
    "16-bit DQT": (lambda: _dqt16(COLOUR), NotImplementedError, "16-bit quantisation"),
    "sampling 4:1:1": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 11, 0x41)), NotImplementedError, "sampling 4x1"),
    "sampling 1x2": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 11, 0x12)), NotImplementedError, "sampling 1x2"),
    "chroma 2x1": (lambda: _patch_sof(COLOUR, lambda s: _set(s, 14, 0x21)), NotImplementedError, "sampling 2x2, 2x1"),
    "four components": (lambda: _patch_sof(COLOUR, lambda s: (s.extend(b"\x04\x11\x01"), _set(s, 9, 4), _set(s, 3, len(s) - 2))),
                        NotImplementedError, "4 components"),
    "second SOS": (lambda: _second_sos(COLOUR), NotImplementedError, "2 scans"),
    "non-interleaved": (lambda: _one_component_scan(COLOUR), NotImplementedError, "non-interleaved"),
    "missing DHT": (lambda: _drop_segments(COLOUR, 0xC4), ValueError, "missing Huffman table"),
    "missing DQT": (lambda: _drop_segments(COLOUR, 0xDB), ValueError, "missing quantisation table"),
    "truncated in DHT": (lambda: COLOUR[: COLOUR.index(b"\xff\xc4") + 9], ValueError, "truncated header"),
    "truncated before SOS": (lambda: COLOUR[: COLOUR.index(b"\xff\xda")], ValueError, "truncated header"),
    "not a JPEG": (lambda: b"\x89PNG\r\n\x1a\n" + bytes(32), ValueError, "not a JPEG"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_image_and_the_property(name):
    make, exc, pattern = REFUSALS[name]
    bad = make()
    with pytest.raises(exc, match=pattern):
        D.jpeg_decode_levels(bad)
    for device in ("cpu", "cuda"):  # refused on the host before anything is launched: no GPU is needed to be refused
        with pytest.raises(exc, match=r"image 1: .*" + pattern):
            D.decode_jpeg_batch([GRAY, bad, COLOUR], device)
    with pytest.raises(exc, match=r"image 0: .*" + pattern):
        D.JpegBatch.from_bytes([bad])


@pytest.mark.parametrize("name", JU.DAMAGE_FILES)
def test_every_cut_inside_the_header_is_a_truncated_header(name):
    header, _, _ = JU.truncation_offsets(name)
    assert len(header) >= 20
    for off in header:
        with pytest.raises(ValueError, match="truncated header"):
            D.jpeg_info(CASES[name].data[:off])


def _pil_file(mode, **kw):
    import numpy as np
    from PIL import Image

    px = np.random.default_rng(7).integers(0, 256, (24, 40, 4 if mode == "CMYK" else 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.frombytes(mode, (40, 24), px.tobytes()).save(buf, "JPEG", quality=90, **kw)
    return buf.getvalue()


def test_progressive_and_cmyk_files_written_by_pil_are_refused():
    pytest.importorskip("PIL")
    with pytest.raises(NotImplementedError, match=r"image 0: progressive \(SOF2\)"):
        D.decode_jpeg_batch([_pil_file("RGB", progressive=True)], "cpu")
    with pytest.raises(NotImplementedError, match=r"image 1: 4 components"):
        D.decode_jpeg_batch([GRAY, _pil_file("CMYK")], "cpu")
    with pytest.raises(ValueError, match="on_unsupported"):
        D.decode_jpeg_batch([GRAY], "cpu", on_unsupported="skip")


def test_on_unsupported_host_without_pil_raises_the_refusal(monkeypatch):
    import sys

    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)  # `from PIL import Image` now raises ImportError
    bad = _patch_sof(COLOUR, lambda s: _set(s, 1, 0xC2))
    with pytest.raises(NotImplementedError, match=r"image 1: progressive \(SOF2\)"):
        D.decode_jpeg_batch([GRAY, bad], "cpu", on_unsupported="host")


def test_on_unsupported_host_decodes_the_odd_file_with_pil():
    pytest.importorskip("PIL")
    import numpy as np
    from PIL import Image

    prog, cmyk = _pil_file("RGB", progressive=True), _pil_file("CMYK")
    files = [GRAY, prog, COLOUR, cmyk]
    batch = D.decode_jpeg_batch(files, "cpu", on_unsupported="host")
    want = [CASES["gray_17x9_noise_q90"].rgb, torch.from_numpy(np.array(Image.open(io.BytesIO(prog)).convert("RGB"))),
            CASES["420_53x37_noise_q90"].rgb, torch.from_numpy(np.array(Image.open(io.BytesIO(cmyk)).convert("RGB")))]
    ref = D.RaggedBatch.from_images(want)
    assert torch.equal(batch.raw, ref.raw) and torch.equal(batch.table, ref.table) and batch.sizes == ref.sizes
    assert batch.status.tolist() == [0, 0, 0, 0]


# ---- the symbols ------------------------------------------------------------------------------------------------------------------
def test_symbols():
    names = ("vt_jpeg_entropy", "vt_jpeg_idct_rgb", "vt_jpeg_scratch_bytes")
    for n in names:
        assert n in N.SYMBOLS and getattr(N.lib(), n) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (vt_[a-z0-9_]+)", out))
    assert N.lib().vt_jpeg_scratch_bytes(10) == 10 * 64 * 2 and N.lib().vt_jpeg_scratch_bytes(-3) == 0
    header = (ROOT / "include" / "vt_amd.h").read_text()
    for k, v in (("VT_JPEG_IMG_FIELDS", D.JPEG_IMG_FIELDS), ("VT_JPEG_SEG_FIELDS", D.JPEG_SEG_FIELDS), ("VT_JPEG_HUFF_BYTES", D.JPEG_HUFF_BYTES)):
        assert re.search(rf"#define {k} {v}\b", header)
    bits = (ROOT / "vision-toolbox_amd" / "csrc" / "vt_jpeg_bits.h").read_text()
    for k, v in (("OK", D.JPEG_OK), ("ERR_CODE", D.JPEG_ERR_CODE), ("ERR_RUN", D.JPEG_ERR_RUN), ("ERR_TRUNCATED", D.JPEG_ERR_TRUNCATED),
                 ("ERR_TABLE", D.JPEG_ERR_TABLE), ("ERR_TRAILING", D.JPEG_ERR_TRAILING)):
        assert re.search(rf"#define VT_JPEG_{k} {v}\b", bits)


# ---- the bit reader under the host sanitizers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_main(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("jpeg_host") / "decode_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "vision-toolbox_amd" / "csrc"), str(ROOT / "tests" / "jpeg_host" / "decode_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _run(exe, streams, tmp_path):
    JU.write_case_file(tmp_path / "cases.bin", streams)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == f"decoded {len(streams)} cases"
    return JU.read_result_file(tmp_path / "out.bin", streams)


def test_sanitized_host_decoder_on_every_fixture_stream(decode_main, tmp_path):
    streams = JU.clean_streams()
    assert len(streams) == len(NAMES)
    for s, (coef, status) in zip(streams, _run(decode_main, streams, tmp_path)):
        host_coef, host_status = s.host
        assert status == host_status == [0] * len(s.segments), s.label
        assert torch.equal(coef, host_coef), s.label


def test_sanitized_host_decoder_on_damaged_streams(decode_main, tmp_path):
    streams = JU.damaged_streams()
    labels = [s.label for s in streams]
    for name in JU.DAMAGE_FILES:
        assert sum(l.startswith(name + "[:") for l in labels) >= 10
        for tail in ("=00", "=FF", "=D9", " oversubscribed", " empty"):
            assert any(l.startswith(name) and l.endswith(tail) for l in labels)
    seen = set()
    for s, (coef, status) in zip(streams, _run(decode_main, streams, tmp_path)):
        host_coef, host_status = s.host
        assert status == host_status, (s.label, status, host_status)
        assert torch.equal(coef, host_coef), s.label
        assert max(status) != 0, f"{s.label}: a damaged stream decoded clean"
        if s.label.endswith(" oversubscribed"):
            assert status == [D.JPEG_ERR_TABLE] * len(status) and not coef.any()
        if s.label.endswith(" empty"):
            assert status == [D.JPEG_ERR_TRUNCATED] * len(status) and not coef.any()
        seen.update(status)
    assert {D.JPEG_ERR_TRUNCATED, D.JPEG_ERR_TABLE} <= seen


def test_a_cut_behind_the_scan_loses_nothing(decode_main, tmp_path):
    """offsets that cut only the EOI marker leave every entropy-coded byte in place: the same coefficients, status 0"""
    streams = []
    for name in JU.DAMAGE_FILES:
        c = CASES[name]
        cut = c.data[: c.info.scan_end]
        streams.append(JU.Stream(name, cut, D.jpeg_info(cut)))
    for s, (coef, status) in zip(streams, _run(decode_main, streams, tmp_path)):
        assert status == [0] * len(status) and torch.equal(coef, CASES[s.label].host[0])
