"""Input-transform kernel numbers on the GPU (fails without one).

    python tools/bench_augment.py [--out DIR] [--batch 256]    -> augment_kernels.json

f32 output, batch 256, noise images, one process.  Cases:
    train176 / train224   375 x 500 sources, boxes of sample_train_params (RandomResizedCrop, flip, RandomErasing p = 0.1)
    val232_224            375 x 500 sources, Resize(232) -> CenterCrop(224)
    short256_train224     256 x 341 sources (a dataset resized to a short side of 256), training boxes to 224
Per case, on the same device tensors:
    launch   vt_augment_batch, one launch for the batch (tables already on the device)
    torch    the torch composition: per image F.interpolate(crop.float(), antialias=True), flip, 1/255, erase (randn)
    copy     dst.copy_(src) over the algorithmic bytes: crop bytes read plus output bytes written
    pil      the reference's host path (PIL crop + resize BILINEAR, ToTensor, flip, erase with torch.randn) on 16 threads, as
             images per second by the host clock -- "not measured" without PIL
  GBps = algorithmic bytes over the median time; images_per_s = batch over the median time.

Timing: as tools/bench_mobilenet.py (device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows, the variants
ALTERNATING window by window; median, min and max recorded).  Nothing is compared against a threshold."""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_mobilenet import WINDOW_S, WINDOWS, _timed_group, vp  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402
from vision_toolbox import data as D  # noqa: E402

CASES = [("train176", (375, 500), 176, "train"), ("train224", (375, 500), 224, "train"), ("val232_224", (375, 500), 224, "val"),
         ("short256_train224", (256, 341), 224, "train")]
PIL_THREADS = 16


def torch_composition(imgs, rows, S, out):
    """imgs: device uint8 [H, W, 3] views; the same geometry through F.interpolate, image by image"""
    for b, (im, r) in enumerate(zip(imgs, rows)):
        top, left, h, w, OH, OW, oy, ox, flip, ei, ej, eh, ew, mode = r[:14]
        x = im[top : top + h, left : left + w].permute(2, 0, 1)[None].float()
        v = F.interpolate(x, (OH, OW), mode="bilinear", antialias=True, align_corners=False)[0, :, oy : oy + S, ox : ox + S]
        if flip:
            v = v.flip(2)
        v = v * (1.0 / 255.0)
        if mode and eh:
            v[:, ei : ei + eh, ej : ej + ew] = torch.randn(3, eh, ew, device=v.device)
        out[b].copy_(v)


def pil_rate(images, rows, S, passes=2):
    try:
        from PIL import Image
    except ImportError:
        return None
    import numpy as np

    pils = [Image.fromarray(im.numpy()) for im in images]

    def one(k):
        top, left, h, w, OH, OW, oy, ox, flip, ei, ej, eh, ew, mode = rows[k][:14]
        im = pils[k].crop((left, top, left + w, top + h)).resize((OW, OH), Image.BILINEAR).crop((ox, oy, ox + S, oy + S))
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        t = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div_(255.0)
        if mode and eh:
            t[:, ei : ei + eh, ej : ej + ew] = torch.randn(3, eh, ew)
        return t

    intra = torch.get_num_threads()
    torch.set_num_threads(1)  # a worker is one thread, as a DataLoader worker is: no 16 x 16 oversubscription by torch's own pool
    try:
        with ThreadPoolExecutor(PIL_THREADS) as pool:
            list(pool.map(one, range(len(pils))))  # warm-up
            t0 = time.perf_counter()
            for _ in range(passes):
                list(pool.map(one, range(len(pils))))
            dt = time.perf_counter() - t0
    finally:
        torch.set_num_threads(intra)
    return passes * len(pils) / dt


def case_row(name, size, S, kind, B):
    lib = N.lib()
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    H, W = size
    stack = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8)
    images = list(stack)
    batch = D.RaggedBatch.from_images(images)
    dev = batch.to("cuda")
    gen = torch.Generator().manual_seed(0)
    params = D.sample_train_params(batch.sizes, S, generator=gen) if kind == "train" else D.eval_params(batch.sizes, 232, S)
    D.validate_params(params, batch.sizes, S)
    rows = params.tolist()
    prm = params.cuda()
    out, out_t = torch.empty(B, 3, S, S, device="cuda"), torch.empty(B, 3, S, S, device="cuda")
    dimgs = [dev.raw[o : o + h * w * 3].view(h, w, 3) for o, h, w in batch.table.tolist()]

    def launch():
        N.check(lib.vt_augment_batch(vp(dev.raw), vp(dev.table), vp(prm), vp(out), B, S, S, 1, None, 0, st()))

    # the launch and the composition agree on these tensors before anything is timed (outside the random erase boxes)
    launch()
    torch_composition(dimgs, rows, S, out_t)
    torch.cuda.synchronize()
    keep = torch.ones(B, 1, S, S, dtype=torch.bool, device="cuda")
    for b, r in enumerate(rows):
        if r[D.P_MODE] and r[D.P_EH]:
            keep[b, :, r[D.P_EI] : r[D.P_EI] + r[D.P_EH], r[D.P_EJ] : r[D.P_EJ] + r[D.P_EW]] = False
    err = ((out - out_t) * keep).abs().max().item()  # (recorded, not judged)

    by = sum(3 * r[D.P_H] * r[D.P_W] for r in rows) + out.numel() * 4
    src, dst = torch.empty(by, device="cuda", dtype=torch.uint8), torch.empty(by, device="cuda", dtype=torch.uint8)
    res = _timed_group({"launch": launch, "torch": lambda: torch_composition(dimgs, rows, S, out_t), "copy": lambda: dst.copy_(src)})
    for v in res.values():
        v["GBps"] = by / (v["ms_median"] * 1e-3) / 1e9
        v["images_per_s"] = B / (v["ms_median"] * 1e-3)
    pil = pil_rate(images, rows, S)
    scale = [max(r[D.P_H] / r[D.P_OH], r[D.P_W] / r[D.P_OW]) for r in rows]
    row = {"case": name, "source": [H, W], "output": S, "kind": kind, "batch": B, "algorithmic_bytes": by,
           "scale_factor_median": sorted(scale)[B // 2], "scale_factor_max": max(scale), "max_abs_diff_vs_torch": err, **res,
           "pil_images_per_s_16_threads": pil if pil is not None else "not measured",
           "ratios": {"torch_over_launch": res["torch"]["ms_median"] / res["launch"]["ms_median"],
                      "copy_over_launch": res["copy"]["ms_median"] / res["launch"]["ms_median"]}}
    print(name, {k: f"{v['ms_median'] * 1e3:.1f} us, {v['GBps']:.1f} GB/s, {v['images_per_s']:.0f} img/s" for k, v in res.items()},
          f"pil {pil if pil is None else round(pil)} img/s, max |diff| vs torch {err:.2e}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    res = {"dtype": "f32 output from uint8", "window_s": WINDOW_S, "windows": WINDOWS, "pil_threads": PIL_THREADS,
           "cases": [case_row(*c, args.batch) for c in CASES]}
    path = Path(args.out) / "augment_kernels.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
