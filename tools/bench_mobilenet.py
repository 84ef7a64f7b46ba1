"""MobileNet numbers on the GPU (fails without one).

    python tools/bench_mobilenet.py kernels [--out DIR]   # the tiled depthwise kernels beside vt_dwconv_* -> mobilenet_kernels.json
    python tools/bench_mobilenet.py model [--out DIR]     # mobilenet_v2 / mobilenet_v3_large three ways   -> mobilenet_model.json

kernels, bf16, (B, H, W, C, k, stride) = the depthwise units of the two models at batch 256 @224, on the same tensors:
    fwd / fwd_untiled     vt_dwt_fwd / vt_dwconv_fwd, both with statistics
    bwd / bwd_untiled     vt_dwt_bwd + vt_dwt_wgrad_reduce / vt_dwconv_dgrad + vt_dwconv_wgrad (dw zeroed outside the timing)
    copy                  dst.copy_(src) of the input tensor: the copy bandwidth of the same box, same process
  TBps = the algorithmic bytes of a pass (forward: x + z; backward: dz + x + dx) over the median time.
model: batch 256, 224 px, bf16, train mode: forward under no_grad and forward + backward through the module API, (i) as built,
(ii) with the depthwise units on the untiled kernels (MobileNetExtractor._untiled_depthwise), (iii) the restatement of
tests/mobilenet_util.py run by torch itself (bf16 autocast, channels_last), all in one process.

Timing: device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows of >= 4 repetitions each, the variants of a
group ALTERNATING window by window; median, min and max recorded.  Nothing is compared against a threshold."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

SHAPES = [(256, 112, 112, 96, 3, 2), (256, 56, 56, 144, 3, 1), (256, 28, 28, 192, 3, 1), (256, 28, 28, 120, 5, 1),
          (256, 14, 14, 672, 5, 2), (256, 7, 7, 960, 5, 1)]
WINDOW_S, WINDOWS = 0.3, 5
vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731


def _timed_group(fns: dict, warmup=3) -> dict:
    """every variant warmed up, then WINDOWS rounds in which the variants take turns"""
    reps = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(4, int(WINDOW_S / max(time.perf_counter() - t0, 1e-5)) + 1)
    out = {name: [] for name in fns}
    for _ in range(WINDOWS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps[name])
    return {name: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "repetitions": WINDOWS * reps[name]}
            for name, v in out.items()}


def _shape(B, H, W, C, k, s):
    lib, dt, st = N.lib(), N.VT_BF16, int(torch.cuda.current_stream().cuda_stream)
    Ho, Wo, pad = (H - 1) // s + 1, (W - 1) // s + 1, (k - 1) // 2
    x = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    dz = torch.randn(B, Ho, Wo, C, device="cuda").to(torch.bfloat16)
    w = torch.randn(C, k * k, device="cuda") * (2.0 / (k * k)) ** 0.5
    z, dx, x2 = torch.empty_like(dz), torch.empty_like(x), torch.empty_like(x)
    dw = torch.zeros(C, k * k, device="cuda")
    stats = N.stats_buffer(C)
    nbytes = lib.vt_dwt_shares_bytes(B, H, W, C, k, s, dt)
    shares = torch.empty(nbytes // 4, device="cuda")
    geo, old = (B, H, W, C, k, s, dt), (B, H, W, C, k, s, pad, 1, dt)

    def fwd():
        N.check(lib.vt_dwt_fwd(vp(x), C, vp(w), vp(z), C, vp(stats), *geo, st))

    def fwd_untiled():
        N.check(lib.vt_dwconv_fwd(vp(x), C, vp(w), vp(z), C, vp(stats), *old, st))

    def bwd():
        N.check(lib.vt_dwt_bwd(vp(dz), C, vp(x), C, vp(w), vp(dx), C, None, 0, vp(shares), nbytes, *geo, st))
        N.check(lib.vt_dwt_wgrad_reduce(vp(shares), nbytes, vp(dw), *geo, st))

    def bwd_untiled():
        N.check(lib.vt_dwconv_dgrad(vp(dz), C, vp(w), vp(dx), C, None, 0, *old, st))
        N.check(lib.vt_dwconv_wgrad(vp(x), C, vp(dz), C, vp(dw), *old, st))

    r = _timed_group({"fwd": fwd, "fwd_untiled": fwd_untiled, "bwd": bwd, "bwd_untiled": bwd_untiled, "copy": lambda: x2.copy_(x)})
    nx, nz = x.numel() * 2, dz.numel() * 2
    for key, nb in (("fwd", nx + nz), ("fwd_untiled", nx + nz), ("bwd", nz + 2 * nx), ("bwd_untiled", nz + 2 * nx), ("copy", 2 * nx)):
        r[key]["TBps"] = nb / r[key]["ms_median"] * 1e-9
    rows, slab = ctypes.c_int32(), ctypes.c_int32()
    N.check(lib.vt_dwt_tile(H, W, C, k, s, dt, ctypes.byref(rows), ctypes.byref(slab)))
    return {"shape": [B, H, W, C, k, s], "rows_per_band": rows.value, "channels_per_slab": slab.value, "shares_bytes": nbytes, **r}


def kernels(out_dir: Path):
    rows = []
    for shape in SHAPES:
        rows.append(_shape(*shape))
        print(json.dumps(rows[-1]))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "mobilenet_kernels.json").write_text(json.dumps({"window_s": WINDOW_S, "windows": WINDOWS, "shapes": rows}, indent=1))


def model(out_dir: Path, batch=256, size=224):
    import mobilenet_util

    from vision_toolbox.backbones import MobileNetExtractor

    res = {"batch": batch, "size": size, "dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "models": {}}
    x = torch.randn(batch, 3, size, size, device="cuda")
    xr = x.contiguous(memory_format=torch.channels_last)
    for name in ("mobilenet_v2", "mobilenet_v3_large"):
        torch.manual_seed(0)
        m = MobileNetExtractor(name).cuda().train()
        m.compute_dtype = torch.bfloat16
        un = MobileNetExtractor(name)
        un._untiled_depthwise = True
        un = un.cuda().train()
        un.compute_dtype = torch.bfloat16
        ref = mobilenet_util.RefMobileNet(name).cuda().to(memory_format=torch.channels_last).train()

        def f(mod=m):
            with torch.no_grad():
                mod(x)

        def fb(mod=m):
            mod(x).float().square().mean().backward()

        def f_torch():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                ref.maps(xr)[-1]

        def fb_torch():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = ref.maps(xr)[-1]
            y.float().square().mean().backward()

        r = {"forward": _timed_group({"vision_toolbox": f, "untiled_depthwise": lambda: f(un), "plain_torch": f_torch}),
             "forward_backward": _timed_group({"vision_toolbox": fb, "untiled_depthwise": lambda: fb(un), "plain_torch": fb_torch})}
        for what, group in r.items():
            for k, v in group.items():
                v["images_per_s"] = batch / v["ms_median"] * 1e3
                print(name, what, k, json.dumps(v))
        res["models"][name] = r
        del m, un, ref
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "mobilenet_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_mobilenet.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
