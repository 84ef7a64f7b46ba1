"""JPEG decoding numbers on the GPU (fails without one).

    python tools/bench_jpeg.py [--out DIR] [--batch 256] [--distinct 32] [--dir FILES]    -> jpeg_kernels.json

Without --dir the files are written here with PIL: `distinct` images of 375 x 500 (noise of amplitude 48 on a gradient),
quality 90, 4:2:0, once without restart markers and once with one restart interval per MCU row (32 MCUs); a batch repeats them
up to `batch`.  With --dir the *.jpg files of FILES/plain and FILES/restart are read instead (tools/bench_jpeg.py --write FILES
writes such a directory where PIL is installed).  Per variant:
    host_parse_ms      JpegBatch.from_bytes (markers, tables, packing into the pinned buffer), wall clock, median of 5
    h2d_ms             the compressed bytes and the tables, pinned -> device
    entropy_ms         vt_jpeg_entropy alone          idct_rgb_ms   vt_jpeg_idct_rgb alone
    device_images_per_s   batch / (h2d + entropy + idct)
    end_to_end_images_per_s   batch / wall clock of decode_jpeg_batch(files, "cuda") with a synchronize, median of 5
    pil_16_threads_images_per_s   PIL's Image.open(...).convert("RGB") of the same files on 16 threads of the same host (None
                                  without PIL)
Timing of the kernels: as tools/bench_mobilenet.py (device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows,
the variants alternating; median, min and max recorded).  Nothing is compared against a threshold.  Before anything is timed
the first image of each variant is compared with PIL (or, without PIL, with the host stage): recorded, not judged."""
import argparse
import io
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tools")]

import torch  # noqa: E402

SOURCE = (375, 500)
VARIANTS = {"plain": 0, "restart": 32}


def write_files(n):
    import numpy as np
    from PIL import Image

    H, W = SOURCE
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    for name, restart in VARIANTS.items():
        files = []
        for i in range(n):
            rng = np.random.default_rng(i)
            base = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (W + H - 2)], axis=2).astype(np.int64)
            px = np.clip(base + rng.integers(-48, 49, (H, W, 3)), 0, 255).astype(np.uint8)
            buf = io.BytesIO()
            kw = dict(restart_marker_blocks=restart) if restart else {}
            Image.fromarray(px).save(buf, "JPEG", quality=90, subsampling=2, **kw)
            files.append(buf.getvalue())
        out[name] = files
    return out


def read_files(d):
    return {name: [p.read_bytes() for p in sorted((Path(d) / name).glob("*.jpg"))] for name in VARIANTS}


def pil_rate(files):
    try:
        from PIL import Image
    except ImportError:
        return None

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB").size

    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, files[:32]))
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            list(pool.map(one, files))
            times.append(time.perf_counter() - t0)
    return len(files) / statistics.median(times)


def variant_row(files):
    from bench_mobilenet import _timed_group, vp
    from vision_toolbox import _native as N
    from vision_toolbox import data as D

    lib = N.lib()
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    row = {"batch": len(files), "compressed_bytes": sum(len(f) for f in files)}
    # agreement of the first image, recorded
    got = D.decode_jpeg_batch(files[:1], "cuda")
    H, W = got.sizes[0]
    try:
        import numpy as np
        from PIL import Image

        ref, row["compared_with"] = torch.from_numpy(np.array(Image.open(io.BytesIO(files[0])).convert("RGB"))), "PIL"
    except ImportError:
        ref, row["compared_with"] = D.jpeg_decode_levels(files[0]), "host stage"
    row["first_image_differing_levels"] = int((got.raw.cpu().view(H, W, 3) != ref).sum())
    row["first_image_status"] = got.status.tolist()

    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        jb = D.JpegBatch.from_bytes(files)
        times.append(time.perf_counter() - t0)
    row["host_parse_ms"] = 1e3 * statistics.median(times)
    row["segments"], row["blocks"], row["raw_bytes"] = int(jb.segments.shape[0]), jb.blocks, jb.raw_bytes
    host = (jb.data, jb.images, jb.segments, jb.qtabs, jb.hufftabs)
    dev = [t.to("cuda") for t in host]
    data, images, segments, qtabs, hufftabs = dev
    coef = torch.empty(jb.blocks * 64, dtype=torch.int16, device="cuda")
    raw = torch.empty(jb.raw_bytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(segments.shape[0], dtype=torch.int32, device="cuda")

    def h2d():
        for d, h in zip(dev, host):
            d.copy_(h, non_blocking=True)

    def entropy():
        N.check(lib.vt_jpeg_entropy(vp(data), data.numel(), vp(images), len(jb), vp(segments), segments.shape[0], vp(hufftabs),
                                    hufftabs.shape[0], vp(coef), jb.blocks, vp(status), st()))

    def idct():
        N.check(lib.vt_jpeg_idct_rgb(vp(coef), jb.blocks, vp(images), len(jb), vp(qtabs), qtabs.shape[0], vp(raw), jb.raw_bytes,
                                     jb.max_mcus_x, jb.max_mcus_y, 0, st()))

    entropy()
    t = _timed_group({"h2d": h2d, "entropy": entropy, "idct_rgb": idct})
    row["kernels"] = t
    row["h2d_ms"], row["entropy_ms"], row["idct_rgb_ms"] = (t[k]["ms_median"] for k in ("h2d", "entropy", "idct_rgb"))
    row["statuses_nonzero"] = int((status != 0).sum())
    row["device_images_per_s"] = len(files) / (1e-3 * (row["h2d_ms"] + row["entropy_ms"] + row["idct_rgb_ms"]))
    dec = D.GPUJpegDecoder()
    dec(files, "cuda")
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        dec(files, "cuda")
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    row["end_to_end_ms"] = 1e3 * statistics.median(times)
    row["end_to_end_images_per_s"] = len(files) / statistics.median(times)
    row["pil_16_threads_images_per_s"] = pil_rate(files)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--write", default=None, help="write the files to this directory and stop (needs PIL, no GPU)")
    a = ap.parse_args()
    if a.write:
        for name, files in write_files(a.distinct).items():
            (Path(a.write) / name).mkdir(parents=True, exist_ok=True)
            for i, f in enumerate(files):
                (Path(a.write) / name / f"{i:04d}.jpg").write_bytes(f)
        return 0
    assert torch.cuda.is_available(), "bench_jpeg.py needs a GPU"
    sets = read_files(a.dir) if a.dir else write_files(a.distinct)
    result = {"device": torch.cuda.get_device_name(0), "source": list(SOURCE), "quality": 90, "sampling": "4:2:0",
              "distinct_files": {k: len(v) for k, v in sets.items()}, "variants": {}}
    for name, files in sets.items():
        assert files, f"no files for variant {name}"
        batch = [files[i % len(files)] for i in range(a.batch)]
        result["variants"][name] = variant_row(batch)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / "jpeg_kernels.json").write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({k: {m: v[m] for m in ("host_parse_ms", "h2d_ms", "entropy_ms", "idct_rgb_ms", "device_images_per_s",
                                             "end_to_end_images_per_s", "pil_16_threads_images_per_s")}
                      for k, v in result["variants"].items()}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
