"""EfficientNet numbers on the GPU (fails without one).

    python tools/bench_efficientnet.py kernels [--out DIR]   # the keep passes and the pool pass beside what they replace -> efficientnet_kernels.json
    python tools/bench_efficientnet.py model [--out DIR]     # efficientnet_b0 / efficientnet_v2_s three ways              -> efficientnet_model.json

kernels, bf16, back to back in one process on the same tensors:
  keep passes at (M, C) = (256*56*56, 24), (256*14*14, 112), (256*7*7, 192) -- the projections that close residual blocks of
  efficientnet_b0 at batch 256 @224 -- with a keep row that drops every eighth image and gives the others 8 / 7:
    keep_fwd / plain_fwd        vt_bn_keep_apply / vt_bn_act_apply with a residual (activation code 0)
    keep_bwd / plain_bwd        vt_bn_keep_bwd_reduce + vt_bn_keep_bwd_finalize_apply / vt_bn_act_bwd_reduce + vt_bn_bwd_finalize_apply
  pool pass at (B, HW, C) = (256, 112*112, 96), (256, 28*28, 240), (256, 7*7, 1152) -- depthwise units of the same model:
    pool_fused / pool_two       vt_bn_act_avgpool_apply / vt_bn_act_apply + vt_global_avgpool_fwd (activation code 3)
    copy                        dst.copy_(src) of the tensor: the copy bandwidth of the same box, same process
  TBps = the algorithmic bytes of a pass over the median time (keep forward: z + r + y, a dropped image's z not counted for the
  keep pass; backward: 2 (dy + z) + dz, a dropped image's dy and z not counted in the reduction; pool: z + y, and y once more
  for the two launches).
  gate_recompute: computed, not built -- the bytes per step a gate pass that recomputes y from z (so that the depthwise unit's
  y is never stored) would save at batch 256 @224, from the shapes of the two models.
model: batch 256, 224 px, bf16, train mode (keep tables drawn per forward): forward under no_grad and forward + backward through
the module API, (i) as built, (ii) with the Squeeze-Excitation pool as its own launch (EfficientNetExtractor._separate_se_pool),
(iii) the restatement of tests/efficientnet_util.py run by torch itself (bf16 autocast, channels_last, no stochastic depth),
all in one process.

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

KEEP_SHAPES = [(256, 56 * 56, 24), (256, 14 * 14, 112), (256, 7 * 7, 192)]
POOL_SHAPES = [(256, 112 * 112, 96), (256, 28 * 28, 240), (256, 7 * 7, 1152)]
WINDOW_S, WINDOWS = 0.3, 5
EPS = 1e-5
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


def _coefs(z):
    """(scale, shift, mean, invstd) of the batch statistics of z with unit gamma, as a [4][C] f32 tensor"""
    zf = z.float()
    mean, var = zf.mean(0), zf.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    return torch.stack([invstd, -mean * invstd, mean, invstd]).contiguous()


def _keep_shape(B, HW, C):
    lib, dt, st = N.lib(), N.VT_BF16, int(torch.cuda.current_stream().cuda_stream)
    M = B * HW
    z, r, dy = (torch.randn(M, C, device="cuda").to(torch.bfloat16) for _ in range(3))
    y, dz, z2 = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    cd = _coefs(z)
    keep = torch.full((B,), 8.0 / 7.0, device="cuda")
    keep[::8] = 0.0
    sums = N.stats_buffer(C)
    dg, db, bc = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(3, C, device="cuda")

    def keep_fwd():
        N.check(lib.vt_bn_keep_apply(vp(z), C, vp(cd[0]), vp(cd[1]), vp(r), C, vp(y), C, vp(keep), HW, M, C, 0, dt, st))

    def plain_fwd():
        N.check(lib.vt_bn_act_apply(vp(z), C, vp(cd[0]), vp(cd[1]), vp(r), C, vp(y), C, M, C, 0, dt, st))

    def keep_bwd():
        sums.zero_()
        N.check(lib.vt_bn_keep_bwd_reduce(vp(dy), C, vp(z), C, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), vp(keep), None, 0, HW, M, C, 0, dt,
                                          vp(sums), st))
        N.check(lib.vt_bn_keep_bwd_finalize_apply(vp(sums), C, float(M), 1.0, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), 1, vp(dg), vp(db),
                                                  vp(bc), vp(dy), C, vp(z), C, vp(keep), None, 0, HW, vp(dz), C, M, 0, dt, st))

    def plain_bwd():
        sums.zero_()
        N.check(lib.vt_bn_act_bwd_reduce(vp(dy), C, vp(z), C, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), M, C, 0, dt, vp(sums), st))
        N.check(lib.vt_bn_bwd_finalize_apply(vp(sums), C, float(M), 1.0, vp(cd[0]), vp(cd[1]), vp(cd[2]), vp(cd[3]), 1, vp(dg), vp(db),
                                             vp(bc), vp(dy), C, vp(z), C, vp(dz), C, M, 0, dt, st))

    res = _timed_group({"keep_fwd": keep_fwd, "plain_fwd": plain_fwd, "keep_bwd": keep_bwd, "plain_bwd": plain_bwd,
                        "copy": lambda: z2.copy_(z)})
    n, kept = z.numel() * 2, 7.0 / 8.0
    for key, nb in (("keep_fwd", n * (2 + kept)), ("plain_fwd", 3 * n), ("keep_bwd", n * (2 * kept + kept + 1 + 1)), ("plain_bwd", 5 * n),
                    ("copy", 2 * n)):
        res[key]["TBps"] = nb / res[key]["ms_median"] * 1e-9
    return {"shape": [B, HW, C], **res}


def _pool_shape(B, HW, C):
    lib, dt, st = N.lib(), N.VT_BF16, int(torch.cuda.current_stream().cuda_stream)
    M = B * HW
    z = torch.randn(M, C, device="cuda").to(torch.bfloat16)
    y, z2 = torch.empty_like(z), torch.empty_like(z)
    pooled = torch.empty(B, C, device="cuda", dtype=torch.bfloat16)
    cd = _coefs(z)
    sb = int(lib.vt_bn_act_avgpool_scratch_bytes(B, HW, C, dt))
    scratch = torch.zeros(max(sb, 16) // 4, device="cuda")

    def pool_fused():
        if sb:
            scratch.zero_()
        N.check(lib.vt_bn_act_avgpool_apply(vp(z), C, vp(cd[0]), vp(cd[1]), vp(y), C, vp(pooled), C, vp(scratch) if sb else None, B, HW, C,
                                            3, dt, st))

    def pool_two():
        N.check(lib.vt_bn_act_apply(vp(z), C, vp(cd[0]), vp(cd[1]), None, 0, vp(y), C, M, C, 3, dt, st))
        N.check(lib.vt_global_avgpool_fwd(vp(y), C, vp(pooled), C, B, HW, C, dt, st))

    res = _timed_group({"pool_fused": pool_fused, "pool_two": pool_two, "copy": lambda: z2.copy_(z)})
    n = z.numel() * 2
    for key, nb in (("pool_fused", 2 * n), ("pool_two", 3 * n), ("copy", 2 * n)):
        res[key]["TBps"] = nb / res[key]["ms_median"] * 1e-9
    return {"shape": [B, HW, C], "scratch_bytes": sb, **res}


def gate_recompute_bytes(name: str, batch=256, size=224) -> dict:
    """bytes per training step a gate pass that recomputes y = silu(bn(z)) of every depthwise unit from z would save: y is
    written by the pool pass and read by the gate pass in forward (recomputed: z is read instead, the same bytes, so the write
    alone is saved) and read again by the gate's backward (recomputed from z: nothing saved there); bf16"""
    from vision_toolbox.backbones import EfficientNetExtractor
    from vision_toolbox.backbones.efficientnet import MBConv

    m = EfficientNetExtractor(name)
    total, h = 0, size // 2
    for stage in list(m.feat_extractor.features)[1:-1]:
        for blk in stage:
            dw = next((u[0] for u in blk.block if isinstance(u, torch.nn.Sequential) and u[0].groups > 1), None)
            stride = max(u[0].stride[0] for u in blk.block if isinstance(u, torch.nn.Sequential))
            h = (h - 1) // stride + 1
            if isinstance(blk, MBConv):
                total += batch * h * h * dw.out_channels * 2
    return {"model": name, "batch": batch, "size": size, "y_write_bytes_saved_per_step": total}


def kernels(out_dir: Path):
    res = {"window_s": WINDOW_S, "windows": WINDOWS, "keep": [], "pool": [], "gate_recompute": []}
    for shape in KEEP_SHAPES:
        res["keep"].append(_keep_shape(*shape))
        print(json.dumps(res["keep"][-1]), flush=True)
    for shape in POOL_SHAPES:
        res["pool"].append(_pool_shape(*shape))
        print(json.dumps(res["pool"][-1]), flush=True)
    for name in ("efficientnet_b0", "efficientnet_v2_s"):
        res["gate_recompute"].append(gate_recompute_bytes(name))
        print(json.dumps(res["gate_recompute"][-1]), flush=True)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "efficientnet_kernels.json").write_text(json.dumps(res, indent=1))


def model(out_dir: Path, batch=256, size=224, names=("efficientnet_b0", "efficientnet_v2_s")):
    import efficientnet_util

    from vision_toolbox.backbones import EfficientNetExtractor

    res = {"batch": batch, "size": size, "dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "models": {}}
    x = torch.randn(batch, 3, size, size, device="cuda")
    xr = x.contiguous(memory_format=torch.channels_last)
    for name in names:
        torch.manual_seed(0)
        m = EfficientNetExtractor(name).cuda().train()
        m.compute_dtype = torch.bfloat16
        sep = EfficientNetExtractor(name)
        sep._separate_se_pool = True
        sep = sep.cuda().train()
        sep.compute_dtype = torch.bfloat16
        ref = efficientnet_util.RefEfficientNet(name).cuda().to(memory_format=torch.channels_last).train()

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

        r = {"forward": _timed_group({"vision_toolbox": f, "separate_se_pool": lambda: f(sep), "plain_torch": f_torch}),
             "forward_backward": _timed_group({"vision_toolbox": fb, "separate_se_pool": lambda: fb(sep), "plain_torch": fb_torch})}
        for what, group in r.items():
            for k, v in group.items():
                v["images_per_s"] = batch / v["ms_median"] * 1e3
                print(name, what, k, json.dumps(v), flush=True)
        res["models"][name] = r
        del m, sep, ref
        torch.cuda.empty_cache()
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "efficientnet_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--models", default="efficientnet_b0,efficientnet_v2_s")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_efficientnet.py needs a GPU: nothing is measured without one")
    if a.what == "kernels":
        kernels(Path(a.out))
    else:
        model(Path(a.out), batch=a.batch, names=tuple(a.models.split(",")))
