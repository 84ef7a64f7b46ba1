"""RegNet numbers on the GPU (fails without one).

    python tools/bench_regnet.py kernels [--out DIR]   # the grouped 3x3 kernels beside their alternatives -> regnet_kernels.json
    python tools/bench_regnet.py model [--out DIR]     # regnet_x_400mf / regnet_y_400mf beside plain torch  -> regnet_model.json

kernels, bf16, (B, H, W, C, gw, stride) = (256, 56, 56, 64, 16, 2), (256, 14, 14, 400, 16, 1), (256, 28, 28, 208, 8, 1):
    fwd / dgrad / wgrad   vt_gconv3_fwd (with statistics) / vt_gconv3_dgrad / vt_gconv3_wgrad, ONE launch each
    fwd_per_group / wgrad_per_group   (a) what Builder._grouped_unit emits: C / gw launches of vt_conv_igemm (with statistics)
                          / vt_conv_wgrad over channel slices.  The per-group data gradient (repacked filters, parity classes
                          under stride 2) is not rebuilt here: the model rows carry it.
    fwd_torch / bwd_torch (b) F.conv2d(groups) in bf16 channels_last, and its autograd backward (dx and dw together)
    copy                  dst.copy_(src) of the input tensor: the copy bandwidth of the same box, same process
  TBps = the tensors a pass must move (input + output map; the filter is noise) over the median time.
model: batch 256, 224 px, bf16, train mode: forward under no_grad and forward + backward through the module API, (i) as built,
(ii) with `f.b` forced onto the per-group path (Builder.GCONV3_WIDTHS emptied), (iii) the restatement of
tests/regnet_util.py run by torch itself (bf16, channels_last), all in one process.

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
import torch.nn.functional as F  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

SHAPES = [(256, 56, 56, 64, 16, 2), (256, 14, 14, 400, 16, 1), (256, 28, 28, 208, 8, 1)]
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


def _desc(B, H, W, Ho, Wo, ci, co, s, ldx, ldy, flags=0):
    d = N.ConvDesc()
    d.dtype = N.VT_BF16
    d.B, d.Hi, d.Wi, d.Cin, d.ldx = B, H, W, ci, ldx
    d.Ho, d.Wo, d.sh, d.sw, d.h0, d.w0 = Ho, Wo, s, s, -1, -1
    d.Cout, d.ldy, d.oH, d.oW, d.oHs, d.oWs = co, ldy, Ho, Wo, 1, 1
    d.ldw, d.flags, d.ntaps = 9 * ci, flags, 9
    for t in range(9):
        d.dh[t], d.dw[t] = t // 3, t % 3
    return d


def _shape(B, H, W, C, gw, s):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    torch.manual_seed(0)
    G, Ho, Wo = C // gw, (H - 1) // s + 1, (W - 1) // s + 1
    x = torch.randn(B, H, W, C, device=dev).to(bf)
    w = (torch.randn(C, 3, 3, gw, device=dev) * (2.0 / (9 * gw)) ** 0.5).to(bf)
    z, z_pg = torch.empty(B, Ho, Wo, C, device=dev, dtype=bf), torch.empty(B, Ho, Wo, C, device=dev, dtype=bf)
    dz, dx = torch.randn(B, Ho, Wo, C, device=dev).to(bf), torch.empty(B, H, W, C, device=dev, dtype=bf)
    dw, dw_pg = torch.zeros(C, 3, 3, gw, device=dev), torch.zeros(C, 3, 3, gw, device=dev)
    stats = N.stats_buffer(C)
    nbytes = lib.vt_gconv3_wgrad_scratch_bytes(B, H, W, C, gw, s)
    scratch = torch.empty(nbytes // 4, device=dev)
    geo = (B, H, W, C, gw, s, dt)
    dfwd = _desc(B, H, W, Ho, Wo, gw, gw, s, C, C, N.VT_CONV_STATS)
    dwg = _desc(B, H, W, Ho, Wo, gw, gw, s, C, C)
    xs, zs, dzs = [x[..., g * gw:] for g in range(G)], [z_pg[..., g * gw:] for g in range(G)], [dz[..., g * gw:] for g in range(G)]
    ws, dws = [w[g * gw:] for g in range(G)], [dw_pg[g * gw:] for g in range(G)]
    # (a per-group statistics buffer of its own, as _grouped_unit allocates: one per group)
    sts = [N.stats_buffer(gw) for _ in range(G)]

    def fwd_pg():
        for g in range(G):
            N.check(lib.vt_conv_igemm(ctypes.byref(dfwd), vp(xs[g]), vp(ws[g]), vp(zs[g]), None, None, None, vp(sts[g]), st()))

    def wgrad_pg():
        for g in range(G):
            N.check(lib.vt_conv_wgrad(ctypes.byref(dwg), vp(xs[g]), vp(dzs[g]), vp(dws[g]), 9 * gw, st()))

    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)  # NCHW view of NHWC storage: channels_last
    wt = w.permute(0, 3, 1, 2).detach().requires_grad_(True)
    dzt = dz.permute(0, 3, 1, 2)
    xc = torch.empty_like(x)

    def bwd_torch():
        xt.grad = wt.grad = None
        F.conv2d(xt, wt, None, s, 1, 1, G).backward(dzt)

    def fwd_torch():
        with torch.no_grad():
            F.conv2d(xt, wt, None, s, 1, 1, G)

    fns = {
        "fwd": lambda: N.check(lib.vt_gconv3_fwd(vp(x), C, vp(w), vp(z), C, vp(stats), *geo, st())),
        "fwd_per_group": fwd_pg,
        "fwd_torch": fwd_torch,
        "dgrad": lambda: N.check(lib.vt_gconv3_dgrad(vp(dz), C, vp(w), vp(dx), C, None, 0, *geo, st())),
        "wgrad": lambda: N.check(lib.vt_gconv3_wgrad(vp(x), C, vp(dz), C, vp(dw), vp(scratch), nbytes, *geo, st())),
        "wgrad_per_group": wgrad_pg,
        "bwd_torch": bwd_torch,
        "copy": lambda: xc.copy_(x),
    }
    e = 2
    nin, nout = x.numel() * e, z.numel() * e
    row = {"B": B, "H": H, "W": W, "C": C, "gw": gw, "stride": s, "groups": G, "dtype": "bf16", "wgrad_scratch_bytes": int(nbytes),
           "min_bytes": {"fwd": nin + nout, "fwd_per_group": nin + nout, "fwd_torch": nin + nout, "dgrad": nin + nout,
                         "wgrad": nin + nout, "wgrad_per_group": nin + nout, "bwd_torch": 2 * (nin + nout), "copy": 2 * nin}}
    for grp in (("fwd", "fwd_per_group", "fwd_torch"), ("dgrad", "wgrad", "wgrad_per_group", "bwd_torch"), ("copy",)):
        row.update(_timed_group({k: fns[k] for k in grp}))
    for k in fns:
        row[k]["TBps"] = row["min_bytes"][k] / (row[k]["ms_median"] * 1e-3) / 1e12
    return row


def kernels(out_dir: Path):
    rows = []
    for shape in SHAPES:
        rows.append(_shape(*shape))
        print(json.dumps(rows[-1]))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "regnet_kernels.json").write_text(json.dumps({"window_s": WINDOW_S, "windows": WINDOWS, "shapes": rows}, indent=1))


def model(out_dir: Path, batch=256, size=224):
    import regnet_util

    from vision_toolbox import engine as E
    from vision_toolbox.backbones import RegNetExtractor

    res = {"batch": batch, "size": size, "dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "models": {}}
    x = torch.randn(batch, 3, size, size, device="cuda")
    xr = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    for name in ("regnet_x_400mf", "regnet_y_400mf"):
        torch.manual_seed(0)
        m = RegNetExtractor(name).cuda().train()
        m.compute_dtype = torch.bfloat16
        widths = E.Builder.GCONV3_WIDTHS
        E.Builder.GCONV3_WIDTHS = ()  # the programs of this instance are compiled on first use: per-group units
        pg = RegNetExtractor(name).cuda().train()
        pg.compute_dtype = torch.bfloat16
        with torch.no_grad():
            pg(x)
        pg(x).float().square().mean().backward()
        E.Builder.GCONV3_WIDTHS = widths
        ref = regnet_util.RefRegNet(name).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last).train()

        def f(mod=m):
            with torch.no_grad():
                mod(x)

        def fb(mod=m):
            mod(x).float().square().mean().backward()

        def f_torch():
            with torch.no_grad():
                ref.maps(xr)[-1]

        def fb_torch():
            ref.maps(xr)[-1].float().square().mean().backward()

        r = {"forward": _timed_group({"vision_toolbox": f, "per_group_path": lambda: f(pg), "plain_torch": f_torch}),
             "forward_backward": _timed_group({"vision_toolbox": fb, "per_group_path": lambda: fb(pg), "plain_torch": fb_torch})}
        for what, group in r.items():
            for k, v in group.items():
                v["images_per_s"] = batch / v["ms_median"] * 1e3
                print(name, what, k, json.dumps(v))
        res["models"][name] = r
        del m, pg, ref
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "regnet_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_regnet.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
