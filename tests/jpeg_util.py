"""Shared by the JPEG tests: the fixture tests/golden/jpeg_cases.npz (tools/gen_golden_jpeg.py), the damaged streams, and
the case file of the stand-alone host decoder (tests/jpeg_host/decode_main.cpp).  Nothing here needs PIL or a GPU."""
import json
import struct
from pathlib import Path

import numpy as np
import torch

from vision_toolbox import data as D

GOLDEN = Path(__file__).resolve().parent / "golden" / "jpeg_cases.npz"
_CACHE = {}

DAMAGE_FILES = ("gray_17x9_noise_q90", "422_33x16_noise_q90", "420_53x37_noise_q90_r3")


class Case:
    def __init__(self, name, settings, data, rgb):
        self.name, self.settings, self.data, self.rgb = name, settings, data, rgb
        self._info = self._coef = None

    @property
    def info(self):
        if self._info is None:
            self._info = D.jpeg_info(self.data)
            D.jpeg_check(self._info)
        return self._info

    @property
    def host(self):
        """(coefficients, statuses) of the host stage, computed once and never written"""
        if self._coef is None:
            self._coef = D.jpeg_decode_coefficients(self.data, self.info)
        return self._coef


def cases():
    """{name: Case}, in the generator's order"""
    if "cases" not in _CACHE:
        z = np.load(GOLDEN)
        out = {}
        for i, (name, st) in enumerate(zip(z["names"].tolist(), z["settings"].tolist())):
            out[name] = Case(name, json.loads(st), z[f"jpeg_{i}"].tobytes(), torch.from_numpy(z[f"rgb_{i}"].copy()))
        _CACHE["cases"] = out
        _CACHE["mixed"] = z["mixed"].tolist()
    return _CACHE["cases"]


def mixed():
    cases()
    return [cases()[n] for n in _CACHE["mixed"]]


class Stream:
    """one input of the entropy stage: bytes, the parsed header, a segment table and Huffman tables (the file's own unless a
    test damages them)"""

    def __init__(self, label, data, info, segments=None, huff=None):
        self.label, self.data, self.info = label, data, info
        self.segments = D.jpeg_segment_table(info) if segments is None else segments
        self.huff = info.huff if huff is None else huff
        self._host = None

    @property
    def host(self):
        if self._host is None:
            self._host = D.jpeg_decode_coefficients(self.data, self.info, self.segments, self.huff)
        return self._host

    def tables(self) -> bytes:
        out = bytearray(6 * D.JPEG_HUFF_BYTES)
        for c, (_, td, ta) in enumerate(self.info.scan_components):
            for k, key in enumerate(((0, td), (1, ta))):
                bits, vals = self.huff[key]
                o = (2 * c + k) * D.JPEG_HUFF_BYTES
                out[o : o + 16] = bits
                out[o + 16 : o + 16 + len(vals)] = vals
        return bytes(out)

    @property
    def blocks(self) -> int:
        hm, vm, mx, my = self.info.mcu_geometry
        return mx * my * (hm * vm + (2 if len(self.info.components) == 3 else 0))


def clean_streams():
    return [Stream(c.name, c.data, c.info) for c in cases().values()]


def truncation_offsets(name):
    """every eighth byte offset of the file: (those that cut the header, those that cut the entropy-coded data of the scan,
    those behind it, which cut nothing but the EOI marker)"""
    c = cases()[name]
    offs, lo, hi = list(range(8, len(c.data), 8)), c.info.scan_offset, c.info.scan_end
    return [o for o in offs if o < lo], [o for o in offs if lo <= o < hi], [o for o in offs if o >= hi]


def damaged_streams():
    """Streams that no decoder may decode cleanly; each must end with a nonzero status:
    * the three DAMAGE_FILES cut at every eighth byte offset inside the scan (at least one byte of entropy-coded data is missing,
      so some block needs bits past the end: status 3, or an earlier 1 / 2 on the zero bits);
    * single bytes of their scans replaced by 00, FF and D9, at 1/4, 1/2 and 3/4 of the scan, re-parsed as a host would;
    * a Huffman table whose BITS over-subscribe the code space (three codes of length 1);
    * segment tables whose ranges are empty."""
    if "damaged" in _CACHE:
        return _CACHE["damaged"]
    out = []
    for name in DAMAGE_FILES:
        c = cases()[name]
        for off in truncation_offsets(name)[1]:
            cut = c.data[:off]
            out.append(Stream(f"{name}[:{off}]", cut, D.jpeg_info(cut)))
        lo, hi = c.info.scan_offset, c.info.scan_end
        for q in (1, 2, 3):
            p = lo + (hi - lo) * q // 4
            for v in (0x00, 0xFF, 0xD9):
                bad = c.data[:p] + bytes([v]) + c.data[p + 1 :]
                out.append(Stream(f"{name}[{p}]={v:02X}", bad, D.jpeg_info(bad)))
        over = dict(c.info.huff)
        key = (0, c.info.scan_components[0][1])
        over[key] = (bytes([3] + [0] * 15), over[key][1])
        out.append(Stream(f"{name} oversubscribed", c.data, c.info, huff=over))
        out.append(Stream(f"{name} empty", c.data, c.info, segments=[(b, b, m0, mc) for b, _, m0, mc in D.jpeg_segment_table(c.info)]))
    _CACHE["damaged"] = out
    return out


def write_case_file(path, streams):
    """the input of decode_main (its header says the format)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(streams)))
        for s in streams:
            hm, vm, mx, my = s.info.mcu_geometry
            f.write(struct.pack("<8q", len(s.data), len(s.info.components), hm, vm, mx, my, len(s.segments), 0))
            f.write(s.tables())
            for seg in s.segments:
                f.write(struct.pack("<4q", *seg))
            f.write(s.data)


def read_result_file(path, streams):
    """[(coef int16 [blocks, 64], [status per segment])]"""
    raw = Path(path).read_bytes()
    out, pos = [], 0
    for s in streams:
        ns, nb = len(s.segments), s.blocks
        st = list(struct.unpack_from(f"<{ns}i", raw, pos))
        pos += 4 * ns
        coef = torch.frombuffer(bytearray(raw[pos : pos + nb * 128]), dtype=torch.int16).view(nb, 64)
        pos += nb * 128
        out.append((coef, st))
    assert pos == len(raw), (pos, len(raw))
    return out
