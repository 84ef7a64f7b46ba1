"""AdamW numbers on the GPU (fails without one) -> profiles/adamw.json.

    python tools/bench_adamw.py kernels [--out DIR]   # (a) vt_adamw against vt_sgd_momentum on the same buffers
    python tools/bench_adamw.py step [--out DIR]      # (b) ConvNeXt-T TrainStep, AdamW, include_pool=False
    python tools/bench_adamw.py trace                 # a few steps of (b), for `rocprofv3 --kernel-trace --stats -- python ...`

Both measuring modes merge their section into the same adamw.json.

(a) vt_adamw (+ its vt_adam_tick, as a step issues it) and vt_sgd_momentum alone, bf16 mirror, on the parameter counts of
ConvNeXt-T and CSPDarknet-53 (each with a 1000-class head), warm, alternating in one process; every sample is a window of
>= 0.5 s of back-to-back launches between two device events; REPEATS windows per kernel; median and spread.  Algorithmic
bytes per element: AdamW 30 (read p g m v, write p m v in f32, write the bf16 mirror), SGD 22 (no v).  The buffers of one
size are 0.4 - 0.5 GB, beyond the 256 MB memory-side cache.  The yardstick is the SGD kernel in the same run: the same
access pattern with two streams fewer.

(b) ConvNeXt-T, bf16, batch 64 @224, 1000 classes, optimizer="AdamW", include_pool=False: ms per step and images/s over
windows of >= 0.5 s after warm-up, and the optimiser list alone (tick + one vt_adamw per weight-decay segment) timed the
same way, as its share of the step.
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT)]

import torch  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

BATCH, SIZE, NCLS, REPEATS, WINDOW_S = 64, 224, 1000, 5, 0.5
BYTES = {"adamw": 30, "sgd": 22}
vp = ctypes.c_void_p


def _merge(out_dir: Path, key: str, value) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    path = out_dir / "adamw.json"
    doc = json.loads(path.read_text()) if path.exists() else {}
    doc[key] = value
    path.write_text(json.dumps(doc, indent=1))


def _param_counts():
    from vision_toolbox import backbones
    from vision_toolbox.backbones import ConvNeXt

    out = {}
    for name, bb in (("convnext_t", ConvNeXt.from_config("T")), ("cspdarknet53", backbones.cspdarknet53())):
        out[name] = sum(p.numel() for p in bb.parameters()) + (bb.get_last_out_channels() + 1) * NCLS
    return out


def _window(fn, launches: int) -> float:
    """us per launch of `fn` over `launches` back-to-back launches between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def kernels(out_dir: Path):
    lib, dev = N.lib(), torch.device("cuda")
    s = vp(int(torch.cuda.current_stream().cuda_stream))
    result = {"dtype_mirror": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "bytes_per_element": BYTES, "sizes": []}
    for name, n in _param_counts().items():
        n = (n + 63) // 64 * 64  # the flat buffers of a TrainStep are padded the same way
        torch.manual_seed(0)
        p, g, m = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3, torch.zeros(n, device=dev)
        v = torch.zeros(n, device=dev)
        mirror = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        hyper = torch.zeros(16, device=dev)
        hyper[:4] = 1e-6  # (small: thousands of timed updates must leave the values in range)
        P, G, M_, V, MI, H = (vp(t.data_ptr()) for t in (p, g, m, v, mirror, hyper))

        def adamw():
            N.check(lib.vt_adam_tick(H, 0.9, 0.999, s))
            N.check(lib.vt_adamw(P, G, M_, V, MI, N.VT_BF16, n, 0.9, 0.999, 1e-8, 0.05, 1.0, 1, H, s))

        def sgd():
            N.check(lib.vt_sgd_momentum(P, G, M_, MI, N.VT_BF16, n, 0.0, 0.9, 2e-5, 1.0, H, s))

        fns = {"adamw": adamw, "sgd": sgd}
        launches = {}
        for k, fn in fns.items():  # warm-up, and the number of launches that fills a window
            us = _window(fn, 20)
            launches[k] = max(20, int(WINDOW_S * 1e6 / us) + 1)
        samples = {k: [] for k in fns}
        for _ in range(REPEATS):  # alternating
            for k, fn in fns.items():
                samples[k].append(_window(fn, launches[k]))
        assert torch.isfinite(p).all() and torch.isfinite(v).all()
        row = {"case": name, "elements": n, "kernels": {}}
        for k in fns:
            med = statistics.median(samples[k])
            row["kernels"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                                 "algorithmic_bytes": BYTES[k] * n, "TBps": BYTES[k] * n / med / 1e6,
                                 "launches_per_window": launches[k]}
        row["adamw_over_sgd_bytes_per_s"] = row["kernels"]["adamw"]["TBps"] / row["kernels"]["sgd"]["TBps"]
        row["note"] = "the adamw figure includes its vt_adam_tick launch (one thread), as a step issues it"
        result["sizes"].append(row)
        print(json.dumps(row))
        del p, g, m, v, mirror
        torch.cuda.empty_cache()
    _merge(out_dir, "kernels", result)


def _train_step():
    from vision_toolbox.backbones import ConvNeXt
    from vision_toolbox.trainer import TrainStep

    torch.manual_seed(0)
    ts = TrainStep(ConvNeXt.from_config("T"), NCLS, BATCH, SIZE, torch.bfloat16, lr=1e-3, weight_decay=0.05,
                   optimizer="AdamW", include_pool=False, device="cuda")
    with torch.no_grad():
        for b in ts.model.modules():  # (as tools/bench_convnext.py: the 1e-6 initial layer scale hides the branches)
            if hasattr(b, "gamma") and isinstance(b.gamma, torch.nn.Parameter) and b.gamma.abs().max() < 1e-3:
                b.gamma.fill_(0.5)
    ts.weights_changed()
    ts.images.copy_(torch.randn(BATCH, 3, SIZE, SIZE, device="cuda"))
    ts.labels.copy_(torch.randint(0, NCLS, (BATCH,), device="cuda"))
    return ts


def _timed(fn, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(WINDOW_S / max(time.perf_counter() - t0, 1e-5)) + 1)
    return [_window(fn, n) / 1e3 for _ in range(REPEATS)], n  # ms per call


def step(out_dir: Path):
    ts = _train_step()
    first = None
    before = N.launch_count()
    ms, n = _timed(lambda: ts.step())
    launches = (N.launch_count() - before) / (REPEATS * n + 4)
    first = ts.loss()
    assert first == first and ts.opt_steps() == REPEATS * n + 4
    med = statistics.median(ms)
    from vision_toolbox.program import current_stream_handle

    s = current_stream_handle()
    opt_ms, n_opt = _timed(lambda: N.run_ops(ts.opt_ops, ts.n_opt, ts.bases, s))
    opt_med = statistics.median(opt_ms)
    res = {"model": "ConvNeXt-T", "batch": BATCH, "size": SIZE, "classes": NCLS, "dtype": "bf16", "optimizer": "AdamW",
           "include_pool": False, "window_s": WINDOW_S, "parameters": sum(p.numel() for p in ts.model.parameters()),
           "step": {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "images_per_s": BATCH / med * 1e3,
                    "steps_per_window": n, "launches_per_step": launches},
           "optimizer_list_alone": {"ms_median": opt_med, "ms_min": min(opt_ms), "ms_max": max(opt_ms), "launches": ts.n_opt,
                                    "calls_per_window": n_opt, "share_of_step": opt_med / med},
           "loss_after_timing": first, "kind_histogram": ts.prog.kind_histogram}
    print(json.dumps(res))
    _merge(out_dir, "train_step", res)


def trace():
    ts = _train_step()
    for _ in range(4):
        ts.step()
    torch.cuda.synchronize()
    print("loss", ts.loss(), "optimiser steps", ts.opt_steps())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step", "trace"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_adamw.py needs a GPU: nothing is measured without one")
    {"kernels": lambda: kernels(Path(a.out)), "step": lambda: step(Path(a.out)), "trace": trace}[a.what]()
