"""Gradient-norm, clipping and LAMB kernel numbers on the GPU (fails without one) -> profiles/lamb_kernels.json.

    python tools/bench_lamb.py [--out DIR]

On flat buffers laid out like a TrainStep's store (every parameter in a slot of a multiple of 64 elements, a 1000-class
head) for ConvNeXt-T, DeiT3-S/16 @224 and CSPDarknet-53, warm, back to back in ONE process, alternating; every sample is a
window of >= WINDOW_S of back-to-back launches between two device events; REPEATS windows per entry; median and spread:

  norm        vt_grad_sumsq + vt_clip_coef       against  copy: torch's copy_ of the same 4 n bytes read (it also writes them)
  adamw_clip  vt_adam_tick + vt_adamw_clip       against  adamw: vt_adam_tick + vt_adamw
  sgd_clip    vt_sgd_momentum_clip               against  sgd: vt_sgd_momentum
  lamb        vt_adam_tick + vt_lamb_moments + vt_lamb_apply over the model's own tensor table   against  adamw

Algorithmic bytes per element with a bf16 mirror: norm 4, copy 8, sgd 22, adamw 30, lamb 42 (moments: read p g m v, write
m v = 24; apply: read p m v, write p and the mirror = 18).  No figure here is a pass criterion.
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
BYTES = {"norm": 4, "copy": 8, "sgd": 22, "sgd_clip": 22, "adamw": 30, "adamw_clip": 30, "lamb": 42}
WD = {0: 0.0, 1: 0.0, 2: 0.05}  # norm / bias / other (trainer.GROUP_*): the usual recipe adapts the weights only
vp = ctypes.c_void_p


def _models():
    from vision_toolbox import backbones
    from vision_toolbox.backbones import ConvNeXt, DeiT3

    return {"convnext_t": ConvNeXt.from_config("T"), "deit3_s": DeiT3.from_config("S_16", 224),
            "cspdarknet53": backbones.cspdarknet53()}


def _layout(bb):
    """(offsets, slot sizes, weight decays) of the model + head, as a TrainStep's store lays them out"""
    from vision_toolbox.trainer import param_groups

    model = nn.Sequential(bb, nn.Linear(bb.get_last_out_channels(), NCLS))
    groups = param_groups(model)
    params = sorted(model.parameters(), key=lambda p: groups[id(p)])
    offs, sizes, wds, o = [], [], [], 0
    for p in params:
        n = (p.numel() + 63) // 64 * 64
        offs.append(o), sizes.append(n), wds.append(WD[groups[id(p)]])
        o += n
    return offs, sizes, wds, o


def _window(fn, launches: int) -> float:
    """us per call of `fn` over `launches` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def main(out_dir: Path):
    lib, dev = N.lib(), torch.device("cuda")
    s = vp(int(torch.cuda.current_stream().cuda_stream))
    result = {"dtype_mirror": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "bytes_per_element": BYTES,
              "item_elements": N.VT_OPT_ITEM, "sizes": []}
    for name, bb in _models().items():
        offs, sizes, wds, n = _layout(bb)
        table, n_items = N.lamb_table(offs, sizes, wds)
        torch.manual_seed(0)
        p, g, m = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3, torch.zeros(n, device=dev)
        v, dst = torch.zeros(n, device=dev), torch.empty(n, device=dev)
        mirror = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        hyper = torch.zeros(16, device=dev)
        hyper[:4] = 1e-6  # (small: thousands of timed updates must leave the values in range)
        ctl = torch.zeros(8, device=dev)
        ctl[N.VT_CTL_CLIP], ctl[N.VT_CTL_LAMB_MAX] = 1.0, 1.0
        sq = torch.zeros(N.opt_items(n), device=dev, dtype=torch.float64)
        part = torch.zeros(2 * n_items, device=dev, dtype=torch.float64)
        tab = torch.from_numpy(table).to(dev)
        P, G, M_, V, MI, H, CTL, SQ, PART, TAB = (vp(t.data_ptr()) for t in (p, g, m, v, mirror, hyper, ctl, sq, part, tab))
        COEF = vp(ctl.data_ptr() + 4 * N.VT_CTL_FACTOR)
        n_sq, n_segs = N.opt_items(n), len(offs)

        def norm():
            N.check(lib.vt_grad_sumsq(G, n, SQ, s))
            N.check(lib.vt_clip_coef(SQ, n_sq, 1.0, CTL, s))

        def copy():
            dst.copy_(g)

        def adamw():
            N.check(lib.vt_adam_tick(H, 0.9, 0.999, s))
            N.check(lib.vt_adamw(P, G, M_, V, MI, N.VT_BF16, n, 0.9, 0.999, 1e-8, 0.05, 1.0, 1, H, s))

        def adamw_clip():
            N.check(lib.vt_adam_tick(H, 0.9, 0.999, s))
            N.check(lib.vt_adamw_clip(P, G, M_, V, MI, N.VT_BF16, n, 0.9, 0.999, 1e-8, 0.05, COEF, 1, H, s))

        def sgd():
            N.check(lib.vt_sgd_momentum(P, G, M_, MI, N.VT_BF16, n, 0.0, 0.9, 2e-5, 1.0, H, s))

        def sgd_clip():
            N.check(lib.vt_sgd_momentum_clip(P, G, M_, MI, N.VT_BF16, n, 0.0, 0.9, 2e-5, COEF, H, s))

        def lamb():
            N.check(lib.vt_adam_tick(H, 0.9, 0.999, s))
            N.check(lib.vt_lamb_moments(P, G, M_, V, TAB, n_segs, n_items, n, PART, COEF, 0.9, 0.999, 1e-6, 0, H, s))
            N.check(lib.vt_lamb_apply(P, M_, V, MI, N.VT_BF16, TAB, n_segs, n_items, n, PART, 1e-6, 0, H, s))

        def lamb_moments():
            N.check(lib.vt_lamb_moments(P, G, M_, V, TAB, n_segs, n_items, n, PART, COEF, 0.9, 0.999, 1e-6, 0, H, s))

        def lamb_apply():
            N.check(lib.vt_lamb_apply(P, M_, V, MI, N.VT_BF16, TAB, n_segs, n_items, n, PART, 1e-6, 0, H, s))

        norm()  # (the factor the clipped entries and LAMB read)
        fns = {"norm": norm, "copy": copy, "sgd": sgd, "sgd_clip": sgd_clip, "adamw": adamw, "adamw_clip": adamw_clip,
               "lamb": lamb, "lamb_moments": lamb_moments, "lamb_apply": lamb_apply}
        launches = {}
        for k, fn in fns.items():  # warm-up, and the number of calls that fills a window
            us = _window(fn, 20)
            launches[k] = max(20, int(WINDOW_S * 1e6 / us) + 1)
        samples = {k: [] for k in fns}
        for _ in range(REPEATS):  # alternating
            for k, fn in fns.items():
                samples[k].append(_window(fn, launches[k]))
        assert torch.isfinite(p).all() and torch.isfinite(v).all() and torch.isfinite(ctl).all()
        row = {"case": name, "elements": n, "tensors": n_segs, "lamb_items": n_items, "norm_items": n_sq, "entries": {}}
        for k in fns:
            med = statistics.median(samples[k])
            row["entries"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                                 "calls_per_window": launches[k]}
            if k in BYTES:
                row["entries"][k].update(algorithmic_bytes=BYTES[k] * n, TBps=BYTES[k] * n / med / 1e6)
        us = {k: row["entries"][k]["us_median"] for k in fns}
        row["ratios"] = {"norm_over_copy": us["norm"] / us["copy"], "sgd_clip_over_sgd": us["sgd_clip"] / us["sgd"],
                         "adamw_clip_over_adamw": us["adamw_clip"] / us["adamw"], "lamb_over_adamw": us["lamb"] / us["adamw"],
                         "lamb_over_adamw_by_bytes": BYTES["lamb"] / BYTES["adamw"]}
        row["note"] = "adamw, adamw_clip and lamb include their vt_adam_tick launch (one thread), as a step issues it"
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del p, g, m, v, dst, mirror
        torch.cuda.empty_cache()
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "lamb_kernels.json").write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_lamb.py needs a GPU: nothing is measured without one")
    main(Path(a.out))
