"""ResNet numbers on the GPU (fails without one).

    python tools/bench_resnet.py kernels [--out DIR]   # the add-then-ReLU BatchNorm passes and the 7x7 stem -> resnet_kernels.json
    python tools/bench_resnet.py model [--out DIR]     # ResNet-50 beside a plain-torch restatement             -> resnet_model.json

kernels, bf16, activation matrices (M, C) = (256*56*56, 256) and (256*7*7, 2048) -- the block ends of layer1 and layer4 of a
ResNet-50 at batch 256, 224 px:
    fwd        vt_bn_add_act_apply / _finalize_apply          beside  vt_bn_act_apply / vt_bn_finalize_apply WITH a residual
               (the same bytes: read z, read r, write y)
    bwd_reduce vt_bn_add_act_bwd_reduce                       beside  vt_bn_act_bwd_reduce (one tensor more: the stored y)
    bwd_apply  vt_bn_add_act_bwd_apply / _bwd_finalize_apply  beside  vt_bn_act_bwd_apply / vt_bn_bwd_finalize_apply (two
               tensors more: the stored y read, d(r) written)
  and the stem at 256 x 3 x 224 x 224: the image gather, the filter repack, the 4x4 convolution (vt_conv_igemm), its filter
  gradient (vt_conv_wgrad) and the repack's transpose.  The statistics buffers are not cleared between repetitions (in a
  program one memset clears all of them).
model: ResNetExtractor("resnet50") at batch 256, 224 px, bf16, train mode: forward under no_grad and forward + backward
through the module API, beside the restatement of tests/resnet_util.py run by torch itself (bf16, channels_last) on the
same GPU in the same process.

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

SHAPES = [(256 * 56 * 56, 256), (256 * 7 * 7, 2048)]
EPS, MOM, WINDOW_S, WINDOWS = 1e-5, 0.1, 0.3, 5
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


def _passes(M, C):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    torch.manual_seed(0)
    z = (torch.randn(M, C, device=dev) * 1.5 + 0.3).to(bf)
    r, dy = torch.randn(M, C, device=dev).to(bf), torch.randn(M, C, device=dev).to(bf)
    y, y_old, dz, dz_old, dr = (torch.empty(M, C, device=dev, dtype=bf) for _ in range(5))
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    coef, bcoef = torch.zeros(4, C, device=dev), torch.zeros(3, C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    stats, sums, sums_old = N.stats_buffer(C), N.stats_buffer(C), N.stats_buffer(C)
    zz = z.float().double()
    for rep, idx in enumerate(torch.chunk(torch.arange(M, device=dev), N.VT_STAT_REPLICAS)):
        N.stats_encode(stats, 0, zz[idx].sum(0), rep)
        N.stats_encode(stats, 1, (zz[idx] ** 2).sum(0), rep)
    del zz
    N.check(lib.vt_bn_finalize(vp(stats), C, float(M), vp(gamma), vp(beta), EPS, MOM, None, None, None, vp(coef[0]), vp(coef[1]),
                               vp(coef[2]), vp(coef[3]), s()))
    fin = lambda: (vp(stats), C, float(M), vp(gamma), vp(beta), EPS, MOM, vp(rm), vp(rv), vp(nbt), vp(coef[0]), vp(coef[1]),  # noqa: E731
                   vp(coef[2]), vp(coef[3]))
    bfin = lambda sm: (vp(sm), C, float(M), 1.0, vp(coef[0]))  # noqa: E731

    fns = {
        "fwd": lambda: N.check(lib.vt_bn_add_act_apply(vp(z), C, vp(coef[0]), vp(coef[1]), vp(r), C, vp(y), C, M, C, dt, s())),
        "fwd_darknet": lambda: N.check(lib.vt_bn_act_apply(vp(z), C, vp(coef[0]), vp(coef[1]), vp(r), C, vp(y_old), C, M, C, 1, dt, s())),
        "fwd_fin": lambda: N.check(lib.vt_bn_add_act_finalize_apply(*fin(), vp(z), C, vp(r), C, vp(y), C, M, dt, s())),
        "fwd_fin_darknet": lambda: N.check(lib.vt_bn_finalize_apply(*fin(), vp(z), C, vp(r), C, vp(y_old), C, M, 1, dt, s())),
        "bwd_reduce": lambda: N.check(lib.vt_bn_add_act_bwd_reduce(vp(dy), C, vp(y), C, vp(z), C, vp(coef[2]), vp(coef[3]), M, C, dt,
                                                                   vp(sums), s())),
        "bwd_reduce_darknet": lambda: N.check(lib.vt_bn_act_bwd_reduce(vp(dy), C, vp(z), C, vp(coef[0]), vp(coef[1]), vp(coef[2]),
                                                                       vp(coef[3]), M, C, 1, dt, vp(sums_old), s())),
        "bwd_apply": lambda: N.check(lib.vt_bn_add_act_bwd_apply(vp(dy), C, vp(y), C, vp(z), C, vp(bcoef), vp(dz), C, vp(dr), C, 0, M, C,
                                                                 dt, s())),
        "bwd_apply_accumulate": lambda: N.check(lib.vt_bn_add_act_bwd_apply(vp(dy), C, vp(y), C, vp(z), C, vp(bcoef), vp(dz), C, vp(dr),
                                                                            C, 1, M, C, dt, s())),
        "bwd_apply_darknet": lambda: N.check(lib.vt_bn_act_bwd_apply(vp(dy), C, vp(z), C, vp(coef[0]), vp(coef[1]), vp(bcoef),
                                                                     vp(dz_old), C, M, C, 1, dt, s())),
        "bwd_fin": lambda: N.check(lib.vt_bn_add_act_bwd_finalize_apply(*bfin(sums), vp(coef[2]), vp(coef[3]), 1, vp(dg), vp(db),
                                                                        vp(bcoef), vp(dy), C, vp(y), C, vp(z), C, vp(dz), C, vp(dr), C,
                                                                        0, M, dt, s())),
        "bwd_fin_darknet": lambda: N.check(lib.vt_bn_bwd_finalize_apply(*bfin(sums_old), vp(coef[1]), vp(coef[2]), vp(coef[3]), 1, vp(dg),
                                                                        vp(db), vp(bcoef), vp(dy), C, vp(z), C, vp(dz_old), C, M, 1, dt,
                                                                        s())),
    }
    fns["fwd"](), fns["bwd_reduce"](), fns["bwd_reduce_darknet"](), fns["bwd_fin"]()  # (y and the coefficients exist before timing)
    torch.cuda.synchronize()
    e = 2
    row = {"M": M, "C": C, "dtype": "bf16",
           "min_bytes": {"fwd": 3 * M * C * e, "fwd_darknet": 3 * M * C * e, "fwd_fin": 3 * M * C * e, "fwd_fin_darknet": 3 * M * C * e,
                         "bwd_reduce": 3 * M * C * e, "bwd_reduce_darknet": 2 * M * C * e, "bwd_apply": 5 * M * C * e,
                         "bwd_apply_accumulate": 6 * M * C * e, "bwd_apply_darknet": 3 * M * C * e, "bwd_fin": 5 * M * C * e,
                         "bwd_fin_darknet": 3 * M * C * e}}
    groups = (("fwd", "fwd_darknet"), ("fwd_fin", "fwd_fin_darknet"), ("bwd_reduce", "bwd_reduce_darknet"),
              ("bwd_apply", "bwd_apply_accumulate", "bwd_apply_darknet"), ("bwd_fin", "bwd_fin_darknet"))
    for g in groups:
        row.update(_timed_group({k: fns[k] for k in g}))
    for k in fns:
        row[k]["TBps"] = row["min_bytes"][k] / (row[k]["ms_median"] * 1e-3) / 1e12
    return row


def _stem(B=256, S=224, Cout=64):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    torch.manual_seed(0)
    Cs, Hs = lib.vt_stem7_s2d_channels(dt), S // 2
    x = torch.zeros(B, S, S, 8, device=dev, dtype=bf)
    x[..., :3] = torch.rand(B, S, S, 3, device=dev).to(bf)
    w = (torch.randn(Cout, 7, 7, 3, device=dev) * 0.1).to(bf)
    xs = torch.empty(B, Hs, Hs, Cs, device=dev, dtype=bf)
    w4 = torch.empty(Cout, 16, Cs, device=dev, dtype=bf)
    y, dz = torch.empty(B, Hs, Hs, Cout, device=dev, dtype=bf), torch.randn(B, Hs, Hs, Cout, device=dev).to(bf)
    dws, dw = torch.zeros(Cout, 16, Cs, device=dev), torch.zeros(Cout, 7, 7, 3, device=dev)
    d = N.ConvDesc()
    d.dtype = dt
    d.B, d.Hi, d.Wi, d.Cin, d.ldx = B, Hs, Hs, Cs, Cs
    d.Ho, d.Wo, d.sh, d.sw, d.h0, d.w0 = Hs, Hs, 1, 1, -2, -2
    d.Cout, d.ldy, d.oH, d.oW, d.oHs, d.oWs = Cout, Cout, Hs, Hs, 1, 1
    d.ldw, d.ntaps = 16 * Cs, 16
    for t in range(16):
        d.dh[t], d.dw[t] = t // 4, t % 4
    fns = {
        "s2d": lambda: N.check(lib.vt_stem7_s2d(vp(x), 8, vp(xs), Cs, B, S, S, dt, s())),
        "pack_filter": lambda: N.check(lib.vt_stem7_pack_filter(vp(w), dt, vp(w4), dt, Cout, s())),
        "conv4x4": lambda: N.check(lib.vt_conv_igemm(ctypes.byref(d), vp(xs), vp(w4), vp(y), None, None, None, None, s())),
        "wgrad4x4": lambda: N.check(lib.vt_conv_wgrad(ctypes.byref(d), vp(xs), vp(dz), vp(dws), 16 * Cs, s())),
        "unpack_wgrad": lambda: N.check(lib.vt_stem7_unpack_wgrad(vp(dws), Cs, vp(dw), Cout, s())),
    }
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    row = {"B": B, "size": S, "Cout": Cout, "dtype": "bf16", "conv_kernel": N.last_kernel_name(),
           "min_bytes": {"s2d": (x.numel() + xs.numel()) * 2, "conv4x4": (xs.numel() + y.numel()) * 2,
                         "wgrad4x4": (xs.numel() + dz.numel()) * 2}}
    for k, fn in fns.items():  # (nothing to alternate with)
        row.update(_timed_group({k: fn}))
    for k in row["min_bytes"]:
        row[k]["TBps"] = row["min_bytes"][k] / (row[k]["ms_median"] * 1e-3) / 1e12
    return row


def kernels(out_dir: Path):
    rows = []
    for M, C in SHAPES:
        rows.append(_passes(M, C))
        print(json.dumps(rows[-1]))
    stem = _stem()
    print(json.dumps(stem))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "resnet_kernels.json").write_text(json.dumps({"window_s": WINDOW_S, "windows": WINDOWS, "passes": rows, "stem": stem},
                                                            indent=1))


def model(out_dir: Path, batch=256, size=224):
    import resnet_util

    from vision_toolbox.backbones import ResNetExtractor

    torch.manual_seed(0)
    m = ResNetExtractor("resnet50").cuda().train()
    m.compute_dtype = torch.bfloat16
    ref = resnet_util.RefResNet("resnet50").cuda().to(torch.bfloat16).to(memory_format=torch.channels_last).train()
    x = torch.randn(batch, 3, size, size, device="cuda")
    xr = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def f():
        with torch.no_grad():
            m(x)

    def fb():
        m(x).float().square().mean().backward()

    def f_torch():
        with torch.no_grad():
            ref.maps(xr)[-1]

    def fb_torch():
        ref.maps(xr)[-1].float().square().mean().backward()

    res = {"model": "resnet50", "batch": batch, "size": size, "dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS,
           "forward": _timed_group({"vision_toolbox": f, "plain_torch": f_torch}),
           "forward_backward": _timed_group({"vision_toolbox": fb, "plain_torch": fb_torch})}
    for what in ("forward", "forward_backward"):
        for name, r in res[what].items():
            r["images_per_s"] = batch / r["ms_median"] * 1e3
            print(what, name, json.dumps(r))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "resnet_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_resnet.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
