"""SPPBlock kernel numbers on the GPU (fails without one).

    python tools/bench_spp.py [--out DIR] [--variants]    -> spp_kernels.json

bf16, (B, H, W, C) = (64, 20, 20, 512) and (64, 40, 40, 256) -- the maps behind a YOLOv5-style backbone at 640 and a stride
of 32 / 16 --, k = 5, repeats = 3, max pooling, on the same tensors in one process:
    fwd / fwd_torch   vt_spp_fwd (with taps) / three F.max_pool2d(5, 1, 2) and torch.cat on channels_last views, under no_grad
    fwd_infer         vt_spp_fwd without taps (an inference program)
    bwd / bwd_torch   vt_spp_bwd / torch.autograd.grad of that composition (the graph is built once, outside the timing)
    copy_fwd / copy_bwd   dst.copy_(src) over as many bytes as the pass's algorithmic bytes: the copy bandwidth of the same box
  TBps = algorithmic bytes over the median time.  Forward: x read once, `repeats` maps and their taps written.  Backward:
  `repeats` gradient maps and the taps read, dx written.
--variants also times the launches under other LDS budgets (knob VT_SPP_LDS_KB: the budget picks the slab width).

Timing: as tools/bench_mobilenet.py (device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows, the variants of
a group ALTERNATING window by window; median, min and max recorded).  Nothing is compared against a threshold."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_mobilenet import WINDOW_S, WINDOWS, _timed_group, vp  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402

SHAPES = [(64, 20, 20, 512), (64, 40, 40, 256)]
K, REPEATS = 5, 3
DEFAULT_KNOBS = {"VT_SPP_LDS_KB": 48}
VARIANTS = [{"VT_SPP_LDS_KB": kb} for kb in (24, 48, 80, 160)]


def shape_row(shape, variants):
    lib, dt, bf = N.lib(), N.VT_BF16, torch.bfloat16
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    B, H, W, C = shape
    x = torch.relu(torch.randn(shape, device="cuda")).to(bf)
    y = torch.empty(B, H, W, REPEATS * C, device="cuda", dtype=bf)
    dy, dx = torch.randn(B, H, W, REPEATS * C, device="cuda").to(bf), torch.empty_like(x)
    taps = torch.empty(REPEATS, B, H, W, C, device="cuda", dtype=torch.uint8)
    geo = (B, H, W, C, K, REPEATS, 0, dt)

    def fwd():
        N.check(lib.vt_spp_fwd(vp(x), C, vp(y), REPEATS * C, vp(taps), *geo, st()))

    def fwd_infer():
        N.check(lib.vt_spp_fwd(vp(x), C, vp(y), REPEATS * C, None, *geo, st()))

    def bwd():
        N.check(lib.vt_spp_bwd(vp(dy), REPEATS * C, vp(taps), vp(dx), C, 0, *geo, st()))

    tx, tg = x.permute(0, 3, 1, 2).requires_grad_(True), dy.permute(0, 3, 1, 2)

    def compose():
        outs, t = [], tx
        for _ in range(REPEATS):
            t = F.max_pool2d(t, K, 1, (K - 1) // 2)
            outs.append(t)
        return torch.cat(outs, 1)

    def fwd_torch():
        with torch.no_grad():
            compose()

    graph = compose()

    def bwd_torch():
        torch.autograd.grad(graph, [tx], tg, retain_graph=True)

    # the launches and the composition agree on these tensors before anything is timed
    fwd()
    bwd()
    torch.cuda.synchronize()
    assert torch.equal(y.permute(0, 3, 1, 2), graph.detach())
    ref_dx = torch.autograd.grad(graph, [tx], tg, retain_graph=True)[0]
    err = ((dx.permute(0, 3, 1, 2).double() - ref_dx.double()).norm() / ref_dx.double().norm()).item()  # (recorded, not judged)

    by_f = x.numel() * 2 + y.numel() * 2 + taps.numel()
    by_b = dy.numel() * 2 + taps.numel() + dx.numel() * 2
    cf, cb = (torch.empty(b // 2, device="cuda", dtype=torch.uint8) for b in (by_f, by_b))
    cf2, cb2 = torch.empty_like(cf), torch.empty_like(cb)
    res = _timed_group({"fwd": fwd, "fwd_infer": fwd_infer, "fwd_torch": fwd_torch, "bwd": bwd, "bwd_torch": bwd_torch,
                        "copy_fwd": lambda: cf2.copy_(cf), "copy_bwd": lambda: cb2.copy_(cb)})
    for k, v in res.items():
        v["TBps"] = (by_f if "fwd" in k else by_b) / (v["ms_median"] * 1e-3) / 1e12
    row = {"shape": list(shape), "k": K, "repeats": REPEATS, "pool": "max", "bytes_fwd": by_f, "bytes_bwd": by_b,
           "dx_rel_err_vs_torch": err, **res}
    row["ratios"] = {"fwd_torch_over_fwd": res["fwd_torch"]["ms_median"] / res["fwd"]["ms_median"],
                     "bwd_torch_over_bwd": res["bwd_torch"]["ms_median"] / res["bwd"]["ms_median"],
                     "copy_fwd_over_fwd": res["copy_fwd"]["ms_median"] / res["fwd"]["ms_median"],
                     "copy_bwd_over_bwd": res["copy_bwd"]["ms_median"] / res["bwd"]["ms_median"]}
    print(shape, {k: f"{v['ms_median'] * 1e3:.1f} us, {v['TBps']:.2f} TB/s" for k, v in res.items()}, flush=True)
    print(shape, {k: f"{v:.2f}" for k, v in row["ratios"].items()}, flush=True)
    if variants:
        row["variants"] = []
        for knobs in VARIANTS:
            for name, value in {**DEFAULT_KNOBS, **knobs}.items():
                N.set_knob(name, value)
            r = _timed_group({"fwd": fwd, "bwd": bwd})
            row["variants"].append({"knobs": knobs, "fwd_ms": r["fwd"]["ms_median"], "bwd_ms": r["bwd"]["ms_median"]})
            print(shape, knobs, {k: f"{v['ms_median'] * 1e3:.1f} us" for k, v in r.items()}, flush=True)
        for name, value in DEFAULT_KNOBS.items():
            N.set_knob(name, value)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--variants", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    res = {"dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "knobs": DEFAULT_KNOBS,
           "shapes": [shape_row(s, args.variants) for s in SHAPES]}
    path = Path(args.out) / "spp_kernels.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
