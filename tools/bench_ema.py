"""Weight-EMA kernel and step numbers on the GPU (fails without one) -> profiles/ema_kernels.json.

    python tools/bench_ema.py [--out DIR] [--no-step]

Kernels: on flat buffers of the sizes a TrainStep's store gives ResNet-50 and ConvNeXt-T (every parameter in a slot of a
multiple of 64 elements, a 1000-class head), warm, back to back in ONE process, alternating; every sample is a window of
>= WINDOW_S of back-to-back launches between two device events; REPEATS windows per entry; median and spread:

  blend_f32 / blend_mirror   vt_ema_update in blend mode, without / with the bf16 mirror   12 / 14 bytes per element
  copy_f32 / copy_mirror     vt_ema_update in copy mode (update 0)                           8 / 10
  skip_f32 / skip_mirror     vt_ema_update in skip mode: the launch alone, no element is touched
  torch_copy                 torch's copy_ of the same f32 buffer                             8

Step: a ResNet-50 train step at batch 128 @224, bf16, without ema_decay and with it at ema_steps 1 and 32, alternating
windows of STEP_WINDOW steps.  No figure here is a pass criterion.
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT)]

import torch  # noqa: E402
from torch import nn  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

NCLS, REPEATS, WINDOW_S = 1000, 5, 0.2
STEP_BATCH, STEP_SIZE, STEP_WARMUP, STEP_WINDOW, STEP_REPEATS = 128, 224, 8, 10, 3
BYTES = {"blend_f32": 12, "blend_mirror": 14, "copy_f32": 8, "copy_mirror": 10, "torch_copy": 8}
vp = ctypes.c_void_p


def _models():
    from vision_toolbox.backbones import ConvNeXt, ResNetExtractor

    return {"resnet50": lambda: ResNetExtractor("resnet50"), "convnext_t": lambda: ConvNeXt.from_config("T")}


def _flat_size(bb) -> int:
    model = nn.Sequential(bb, nn.Linear(bb.get_last_out_channels(), NCLS))
    return sum((p.numel() + 63) // 64 * 64 for p in model.parameters())


def _window(fn, launches: int) -> float:
    """us per call of `fn` over `launches` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def kernels(result):
    lib, dev = N.lib(), torch.device("cuda")
    s = vp(int(torch.cuda.current_stream().cuda_stream))
    for name, make in _models().items():
        n = _flat_size(make())
        torch.manual_seed(0)
        p, e, dst = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 0.05, torch.empty(n, device=dev)
        mirror = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        ctls = {}
        for mode in (N.VT_EMA_SKIP, N.VT_EMA_COPY, N.VT_EMA_BLEND):  # (the mode a tick would leave, written by hand)
            c = torch.zeros(8, device=dev)
            c[N.VT_EMA_ALPHA] = 1.0 - 0.99998
            c.view(torch.int32)[N.VT_EMA_MODE] = mode
            ctls[mode] = c
        P, E_, MI = vp(p.data_ptr()), vp(e.data_ptr()), vp(mirror.data_ptr())

        def update(mode, with_mirror):
            ctl = vp(ctls[mode].data_ptr())
            return lambda: N.check(lib.vt_ema_update(E_, P, MI if with_mirror else None, n, ctl, s))

        fns = {"blend_f32": update(N.VT_EMA_BLEND, False), "blend_mirror": update(N.VT_EMA_BLEND, True),
               "copy_f32": update(N.VT_EMA_COPY, False), "copy_mirror": update(N.VT_EMA_COPY, True),
               "skip_f32": update(N.VT_EMA_SKIP, False), "skip_mirror": update(N.VT_EMA_SKIP, True),
               "torch_copy": lambda: dst.copy_(p)}
        launches = {}
        for k, fn in fns.items():  # warm-up, and the number of calls that fills a window
            us = _window(fn, 20)
            launches[k] = max(20, int(WINDOW_S * 1e6 / us) + 1)
        samples = {k: [] for k in fns}
        for _ in range(REPEATS):  # alternating
            for k, fn in fns.items():
                samples[k].append(_window(fn, launches[k]))
        assert torch.isfinite(e).all()
        row = {"case": name, "elements": n, "entries": {}}
        for k in fns:
            med = statistics.median(samples[k])
            row["entries"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                                 "calls_per_window": launches[k]}
            if k in BYTES:
                row["entries"][k].update(algorithmic_bytes=BYTES[k] * n, TBps=BYTES[k] * n / med / 1e6)
        tb = {k: v["TBps"] for k, v in row["entries"].items() if "TBps" in v}
        row["ratios"] = {"blend_f32_TBps_over_torch_copy": tb["blend_f32"] / tb["torch_copy"],
                         "blend_mirror_TBps_over_torch_copy": tb["blend_mirror"] / tb["torch_copy"],
                         "blend_mirror_us_over_torch_copy_us": row["entries"]["blend_mirror"]["us_median"]
                         / row["entries"]["torch_copy"]["us_median"]}
        result["kernels"].append(row)
        print(json.dumps(row), flush=True)
        del p, e, dst, mirror
        torch.cuda.empty_cache()


def step(result):
    from vision_toolbox.backbones import ResNetExtractor
    from vision_toolbox.trainer import TrainStep

    variants = {"no_ema": {}, "ema_steps_1": {"ema_decay": 0.99998}, "ema_steps_32": {"ema_decay": 0.99998, "ema_steps": 32}}
    steps = {}
    torch.manual_seed(0)
    x = torch.rand(STEP_BATCH, 3, STEP_SIZE, STEP_SIZE, device="cuda")
    y = torch.randint(0, NCLS, (STEP_BATCH,), device="cuda")
    for k, kw in variants.items():
        torch.manual_seed(1)
        ts = TrainStep(ResNetExtractor("resnet50"), NCLS, STEP_BATCH, STEP_SIZE, torch.bfloat16, lr=0.01, device="cuda", **kw)
        ts.images.copy_(x), ts.labels.copy_(y)
        for _ in range(STEP_WARMUP):
            ts.step()
        torch.cuda.synchronize()
        steps[k] = ts
    samples = {k: [] for k in variants}
    for _ in range(STEP_REPEATS):  # alternating
        for k, ts in steps.items():
            samples[k].append(_window(ts.step, STEP_WINDOW) / 1e3)
    row = {"model": "resnet50", "batch": STEP_BATCH, "image_size": STEP_SIZE, "dtype": "bf16",
           "flat_elements": steps["no_ema"].store.pflat.numel(), "steps_per_window": STEP_WINDOW, "entries": {}}
    for k in variants:
        row["entries"][k] = {"ms_median": statistics.median(samples[k]), "ms_min": min(samples[k]), "ms_max": max(samples[k]),
                             "loss": steps[k].loss()}
    base = row["entries"]["no_ema"]["ms_median"]
    row["ema_steps_1_minus_no_ema_ms"] = row["entries"]["ema_steps_1"]["ms_median"] - base
    row["ema_steps_32_minus_no_ema_ms"] = row["entries"]["ema_steps_32"]["ms_median"] - base
    row["ema_updates"] = {k: steps[k].ema_updates() for k in variants if k != "no_ema"}
    result["step"] = row
    print(json.dumps(row), flush=True)


def main(out_dir: Path, with_step: bool):
    result = {"window_s": WINDOW_S, "repeats": REPEATS, "bytes_per_element": BYTES, "grid_cap_elements": N.lib().vt_ema_grid_cap(),
              "kernels": []}
    kernels(result)
    if with_step:
        step(result)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "ema_kernels.json").write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_ema.py needs a GPU: nothing is measured without one")
    main(Path(a.out), not a.no_step)
