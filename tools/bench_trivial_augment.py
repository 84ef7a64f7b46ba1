"""TrivialAugmentWide kernel numbers on the GPU (fails without one).

    python tools/bench_trivial_augment.py [--out DIR] [--batch 256]    -> trivial_augment_kernels.json

Batch 256, noise sources of 375 x 500, training boxes of sample_train_params (seed 0) to 176 and to 224, one process.  Per
output size, on the same device tensors and tables:
    one_launch   vt_augment_batch (no TrivialAugmentWide): the path as it was
    two_call     vt_augment_batch_u8 + vt_trivial_augment with the uniform mix of ops (sample_trivial_augment, seed 0): the
                 price of the stage is two_call over one_launch
    u8           vt_augment_batch_u8 alone
    stage_<op>   vt_trivial_augment alone with EVERY image under that op (bin 15 of 31, positive), and stage_mix with the
                 uniform mix: each op class against stage_Identity
    copy         dst.copy_(src) over the stage's algorithmic bytes: 3 S S bytes read + 12 S S bytes written an image
  GBps = the stage's algorithmic bytes over the median time (stage_*, copy); images_per_s = batch over the median time.

Timing: as tools/bench_mobilenet.py (device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows, the variants
ALTERNATING window by window; median, min and max recorded).  Nothing is compared against a threshold.  Before anything is
timed the two-call path is compared with the module's CPU path on the first 8 images (recorded, not judged)."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import torch  # noqa: E402

from bench_mobilenet import WINDOW_S, WINDOWS, _timed_group, vp  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402
from vision_toolbox import data as D  # noqa: E402

SOURCE = (375, 500)
SIZES = (176, 224)


def size_row(S, B):
    lib = N.lib()
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    H, W = SOURCE
    images = list(torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8))
    batch = D.RaggedBatch.from_images(images)
    dev = batch.to("cuda")
    params = D.sample_train_params(batch.sizes, S, generator=torch.Generator().manual_seed(0))
    mix = D.sample_trivial_augment(B, S, generator=torch.Generator().manual_seed(0))
    prm = params.cuda()
    out = torch.empty(B, 3, S, S, device="cuda")
    u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    work = torch.empty(B, 4, 256, dtype=torch.int32, device="cuda")

    def one_launch():
        N.check(lib.vt_augment_batch(vp(dev.raw), vp(dev.table), vp(prm), vp(out), B, S, S, 1, None, 0, st()))

    def to_u8():
        N.check(lib.vt_augment_batch_u8(vp(dev.raw), vp(dev.table), vp(prm), vp(u8), B, S, S, 1, 0, st()))

    def stage(ta):
        return lambda: N.check(lib.vt_trivial_augment(vp(u8), vp(ta), vp(prm), vp(out), vp(work), B, S, S, None, st()))

    tables = {"mix": mix.cuda()}
    for op, name in enumerate(D.TA_OPS):
        mags = D.ta_magnitudes(op)
        tables[name] = torch.tensor([D.ta_row(op, mags[15] if mags else 0.0, S)] * B, dtype=torch.float64).cuda()
    mix_stage = stage(tables["mix"])

    def two_call():
        to_u8()
        mix_stage()

    # the two-call path against the module's CPU path on the first images, outside the random erase boxes
    n = min(8, B)
    two_call()
    torch.cuda.synchronize()
    ref = D.GPUBatchTransform(S)(D.RaggedBatch.from_images(images[:n]), params[:n], ta=mix[:n])
    keep = torch.ones(n, 3, S, S, dtype=torch.bool)
    for b, r in enumerate(params[:n].tolist()):
        if r[D.P_MODE] and r[D.P_EH]:
            keep[b, :, r[D.P_EI] : r[D.P_EI] + r[D.P_EH], r[D.P_EJ] : r[D.P_EJ] + r[D.P_EW]] = False
    diff = ((out[:n].cpu() - ref) * keep).abs()
    check = {"images": n, "elements_that_differ": int((diff > 0).sum()), "max_abs_diff": diff.max().item()}

    by = B * S * S * (3 + 12)
    src, dst = torch.empty(by, device="cuda", dtype=torch.uint8), torch.empty(by, device="cuda", dtype=torch.uint8)
    to_u8()
    fns = {"one_launch": one_launch, "two_call": two_call, "u8": to_u8, "copy": lambda: dst.copy_(src)}
    fns.update({f"stage_{k}": stage(t) for k, t in tables.items()})
    res = _timed_group(fns)
    for k, v in res.items():
        v["images_per_s"] = B / (v["ms_median"] * 1e-3)
        if k == "copy" or k.startswith("stage_"):
            v["GBps"] = by / (v["ms_median"] * 1e-3) / 1e9
    ident = res["stage_Identity"]["ms_median"]
    ops = torch.bincount(mix[:, 0].long(), minlength=len(D.TA_OPS)).tolist()
    row = {"output": S, "source": [H, W], "batch": B, "stage_algorithmic_bytes": by, "mix_op_counts": dict(zip(D.TA_OPS, ops)),
           "check_vs_cpu_path": check, **res,
           "ratios": {"two_call_over_one_launch": res["two_call"]["ms_median"] / res["one_launch"]["ms_median"],
                      "stage_mix_over_copy": res["stage_mix"]["ms_median"] / res["copy"]["ms_median"],
                      "stage_over_identity": {k: res[f"stage_{k}"]["ms_median"] / ident for k in tables}}}
    print(S, {k: f"{v['ms_median'] * 1e3:.1f} us" for k, v in res.items()}, check, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    res = {"dtype": "f32 output from uint8 levels", "window_s": WINDOW_S, "windows": WINDOWS,
           "sizes": [size_row(S, args.batch) for S in SIZES]}
    path = Path(args.out) / "trivial_augment_kernels.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
