"""Writes tests/golden/jpeg_cases.npz: small JPEG files written by PIL (libjpeg-turbo), PIL's own decode of each, and the
encoder settings -- the fixture of tests/test_jpeg_cpu.py (which also re-decodes with PIL where PIL is installed) and of the
GPU tests (which must not need PIL).

    python tools/gen_golden_jpeg.py

Contents: names [n] (str), settings [n] (JSON: sampling, W, H, source, quality, optimize, restart, spliced), jpeg_<i> (uint8, the
file), rgb_<i> (uint8 [H, W, 3], Image.open(...).convert("RGB")), mixed [7] (names of the mixed batch).
Sources are seeded noise (which forces FF 00 stuffing: asserted), a smooth gradient and a constant image."""
import io
import json
import sys
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "jpeg_cases.npz"

SIZES = {  # (W, H): the smallest at which each mechanism can go wrong
    "gray": [(1, 1), (8, 8), (7, 5), (17, 9)],
    "444": [(8, 8), (53, 37)],
    "422": [(16, 8), (33, 16), (53, 37)],
    "420": [(1, 1), (2, 2), (16, 16), (17, 17), (40, 48), (53, 37)],
}
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
QUALITIES = (5, 75, 90, 100)
SWEEP = {"gray": (17, 9), "444": (53, 37), "422": (53, 37), "420": (53, 37)}  # the size of the quality / source sweep


def source(kind: str, W: int, H: int, seed: int) -> np.ndarray:
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "constant":
        return np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (H, W, 3)).copy()
    y, x = np.mgrid[0:H, 0:W]
    g = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], axis=2)
    return g.astype(np.uint8)


def encode(px: np.ndarray, sampling: str, quality: int, optimize: bool, restart: int) -> bytes:
    im = Image.fromarray(px)
    kw = dict(quality=quality, optimize=optimize)
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = SUBSAMPLING[sampling]
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def splice(data: bytes) -> bytes:
    """a COM segment behind SOI, and FF fill bytes in front of the first DHT marker, the first RST marker and EOI"""
    out = bytearray(data[:2]) + b"\xff\xfe" + (2 + 11).to_bytes(2, "big") + b"hello world"
    rest = bytearray(data[2:])
    i = rest.index(b"\xff\xc4")
    rest[i:i] = b"\xff\xff"
    i = rest.index(b"\xff\xd0")
    rest[i:i] = b"\xff\xff\xff"
    assert rest[-2:] == b"\xff\xd9"
    rest[-2:-2] = b"\xff"
    return bytes(out + rest)


def main():
    cases = []  # (name, settings, bytes)

    def add(sampling, W, H, src, quality=90, optimize=False, restart=0, spliced=False):
        name = f"{sampling}_{W}x{H}_{src}_q{quality}" + ("_opt" if optimize else "") + (f"_r{restart}" if restart else "") + (
            "_spliced" if spliced else "")
        if any(c[0] == name for c in cases):
            return name
        data = encode(source(src, W, H, len(cases) + 1), sampling, quality, optimize, restart)
        if spliced:
            data = splice(data)
        cases.append((name, dict(sampling=sampling, W=W, H=H, source=src, quality=quality, optimize=optimize, restart=restart,
                                 spliced=spliced), data))
        return name

    for sampling, sizes in SIZES.items():
        for W, H in sizes:
            add(sampling, W, H, "noise")
    for sampling, (W, H) in SWEEP.items():
        for q in QUALITIES:
            for src in ("noise", "gradient", "constant"):
                add(sampling, W, H, src, q)
        add(sampling, W, H, "noise", 75, optimize=True)
        add(sampling, W, H, "gradient", 90, optimize=True)
    for r in (1, 2, 3):
        add("gray", 80, 8, "noise", 90, restart=r)
        add("420", 53, 37, "noise", 90, restart=r)
    add("420", 53, 37, "noise", 75, restart=2, spliced=True)
    mixed = [add("gray", 17, 9, "noise"), add("444", 53, 37, "noise"), add("422", 33, 16, "noise"), add("420", 40, 48, "noise"),
             add("420", 53, 37, "noise", 90, restart=3), add("420", 17, 17, "noise"), add("420", 16, 16, "noise")]

    # libjpeg uses its triangle upsamplers only where the chroma plane is MORE than two samples wide and replicates a narrower
    # one: widths 1 .. 4 are one or two chroma columns (with heights that have chroma rows to interpolate between), 5 and 6
    # are the first three-column planes.  (Added behind everything else: the seeds of the cases above do not move.)
    for sampling, sizes in (("422", [(3, 5), (4, 16), (2, 9), (5, 5), (6, 3)]), ("420", [(1, 16), (3, 5), (4, 16), (2, 7), (5, 5), (6, 9)])):
        for W, H in sizes:
            add(sampling, W, H, "noise")

    arrays, stuffed = {}, 0
    for i, (name, st, data) in enumerate(cases):
        rgb = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (st["H"], st["W"], 3), (name, rgb.shape)
        arrays[f"jpeg_{i}"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"rgb_{i}"] = rgb
        sos = data.index(b"\xff\xda")
        stuffed += b"\xff\x00" in data[sos:]
    assert stuffed > 0, "no scan holds a stuffed FF 00 pair"
    arrays["names"] = np.array([c[0] for c in cases])
    arrays["settings"] = np.array([json.dumps(c[1], sort_keys=True) for c in cases])
    arrays["mixed"] = np.array(mixed)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(cases)} cases, {stuffed} with stuffed bytes, {sum(len(c[2]) for c in cases)} JPEG bytes, "
          f"{OUT.stat().st_size} bytes on disk")


if __name__ == "__main__":
    sys.exit(main())
