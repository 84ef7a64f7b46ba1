"""DeformableConv2d kernel numbers on the GPU (fails without one).

    python tools/bench_deform.py [--out DIR]    -> deform_kernels.json

bf16, (B, H, W, Cin, Cout, k, s, p) = (64, 40, 40, 256, 256, 3, 1, 1) and (64, 20, 20, 512, 512, 3, 1, 1), sigmoid mask,
offsets N(0, 1.5^2), on the same tensors in one process:
    fwd / bwd / wgrad      vt_deform_fwd, vt_deform_bwd (d(offset), d(mask logit), the scatter of d(x) and its flush),
                           vt_deform_wgrad (slabs + ordered reducer, filter and bias)
    bwd_no_dx              vt_deform_bwd with dx = NULL: the same launch without the scatter, the plane's memset and the flush.
                           scatter_share = 1 - bwd_no_dx / bwd is the share of the backward launch that is the scatter.
    fwd_torch / bwd_torch  the composition in plain torch: nine F.grid_sample calls (align_corners=True, zeros), the mask, one
                           matmul; torch.autograd.grad of it for (x, offsets, logits, filter, bias) (graph built once)
    conv_fwd / conv_wgrad  vt_conv_igemm / vt_conv_wgrad of the plain convolution of the same geometry: the floor below which no
                           deformable convolution can go.  The plain DATA gradient is not timed here (it needs a packed filter).
The LDS window of the scatter (sum in LDS, flush once) is not built: there is one scatter, plain f32 atomics.

Timing: as tools/bench_mobilenet.py (device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows, the variants of
a group ALTERNATING window by window; median, min and max recorded).  Nothing is compared against a threshold."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_mobilenet import WINDOW_S, WINDOWS, _timed_group, vp  # noqa: E402
from gpu_util import conv_desc  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402

SHAPES = [(64, 40, 40, 256, 256, 3, 1, 1), (64, 20, 20, 512, 512, 3, 1, 1)]


def shape_row(shape):
    lib, dt, bf = N.lib(), N.VT_BF16, torch.bfloat16
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    B, H, W, Ci, Co, k, s, p = shape
    K2, Ho, Wo = k * k, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, H, W, Ci, device="cuda").to(bf)
    off = (torch.randn(B, Ho, Wo, 24, device="cuda") * 1.5).to(bf)  # 2 k^2 = 18 channels of a 24-wide map
    msk = torch.randn(B, Ho, Wo, 16, device="cuda").to(bf)  # k^2 = 9 of 16
    w = (torch.randn(Co, K2, Ci, device="cuda") / (K2 * Ci) ** 0.5).to(bf)
    bias = torch.randn(Co, device="cuda")
    y = torch.empty(B, Ho, Wo, Co, device="cuda", dtype=bf)
    dy = torch.randn(B, Ho, Wo, Co, device="cuda").to(bf)
    dx, doff, dmsk = torch.empty_like(x), torch.zeros_like(off), torch.zeros_like(msk)
    plane = torch.empty(B * H * W * Ci, device="cuda")
    dw, db = torch.zeros(Co * K2 * Ci, device="cuda"), torch.zeros(Co, device="cuda")
    nbytes = int(lib.vt_deform_wgrad_scratch_bytes(B, H, W, Ci, Co, k, s, p, 1))
    scratch = torch.empty(nbytes // 4, device="cuda")
    geom = (B, H, W, Ci, Co, k, s, p, 1, 1, dt)

    def fwd():
        N.check(lib.vt_deform_fwd(vp(x), Ci, vp(off), 24, vp(msk), 16, vp(w), vp(bias), vp(y), Co, *geom, st()))

    def bwd(with_dx=True):
        N.check(lib.vt_deform_bwd(vp(dy), Co, vp(x), Ci, vp(off), 24, vp(msk), 16, vp(w), vp(doff), 24, vp(dmsk), 16,
                                  vp(dx) if with_dx else None, Ci, 0, vp(plane) if with_dx else None, *geom, st()))

    def wgrad():
        N.check(lib.vt_deform_wgrad(vp(dy), Co, vp(x), Ci, vp(off), 24, vp(msk), 16, vp(dw), vp(db), vp(scratch), nbytes, *geom,
                                    st()))

    # the plain convolution of the same geometry
    d = conv_desc(dt, x, Ci, Co, k, s, p, Co)
    dwc = torch.zeros(Co * K2 * Ci, device="cuda")

    def conv_fwd():
        N.check(lib.vt_conv_igemm(C.byref(d), vp(x), vp(w), vp(y), None, None, None, None, st()))

    def conv_wgrad():
        N.check(lib.vt_conv_wgrad(C.byref(d), vp(x), vp(dy), vp(dwc), K2 * Ci, st()))

    # the torch composition on the same tensors (NCHW views)
    tx = x.permute(0, 3, 1, 2).requires_grad_(True)
    to = off[..., : 2 * K2].permute(0, 3, 1, 2).requires_grad_(True)
    tm = msk[..., :K2].permute(0, 3, 1, 2).requires_grad_(True)
    tw, tb = w.clone().requires_grad_(True), bias.to(bf).requires_grad_(True)
    gy, gx = torch.meshgrid(torch.arange(Ho, device="cuda") * s - p, torch.arange(Wo, device="cuda") * s - p, indexing="ij")

    def compose():
        cols, m = [], torch.sigmoid(tm)
        for t in range(K2):
            py = (gy + t // k).to(bf) + to[:, 2 * t]
            px = (gx + t % k).to(bf) + to[:, 2 * t + 1]
            grid = torch.stack((2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1), dim=-1)
            v = F.grid_sample(tx, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * m[:, t : t + 1]
            cols.append(v.permute(0, 2, 3, 1))
        col = torch.stack(cols, dim=3).reshape(B * Ho * Wo, K2 * Ci)
        return (col @ tw.reshape(Co, K2 * Ci).t() + tb).view(B, Ho, Wo, Co)

    def fwd_torch():
        with torch.no_grad():
            compose()

    graph = compose()

    def bwd_torch():
        torch.autograd.grad(graph, [tx, to, tm, tw, tb], dy, retain_graph=True)

    # the launches and the composition agree on these tensors before anything is timed (recorded, not judged: the composition
    # computes its positions in bf16)
    fwd()
    torch.cuda.synchronize()
    err = ((y.double() - graph.detach().double()).norm() / graph.detach().double().norm()).item()

    res = _timed_group({"fwd": fwd, "fwd_torch": fwd_torch, "conv_fwd": conv_fwd})
    res.update(_timed_group({"bwd": bwd, "bwd_no_dx": lambda: bwd(False), "wgrad": wgrad, "bwd_torch": bwd_torch,
                             "conv_wgrad": conv_wgrad}))
    ms = {k_: v["ms_median"] for k_, v in res.items()}
    flop = 2.0 * B * Ho * Wo * Co * K2 * Ci
    row = {"shape": list(shape), "mask_act": "sigmoid", "gemm_flop": flop, "scatter_added_bytes": 4.0 * 4 * K2 * B * Ho * Wo * Ci,
           "y_rel_err_vs_torch": err, **res}
    row["ratios"] = {"fwd_torch_over_fwd": ms["fwd_torch"] / ms["fwd"], "fwd_over_conv_fwd": ms["fwd"] / ms["conv_fwd"],
                     "bwd_torch_over_bwd_plus_wgrad": ms["bwd_torch"] / (ms["bwd"] + ms["wgrad"]),
                     "wgrad_over_conv_wgrad": ms["wgrad"] / ms["conv_wgrad"],
                     "scatter_share_of_bwd": 1.0 - ms["bwd_no_dx"] / ms["bwd"],
                     "scatter_share_of_bwd_plus_wgrad": (ms["bwd"] - ms["bwd_no_dx"]) / (ms["bwd"] + ms["wgrad"])}
    row["TFLOPs"] = {k_: flop / (ms[k_] * 1e-3) / 1e12 for k_ in ("fwd", "conv_fwd", "wgrad", "conv_wgrad", "bwd_no_dx")}
    print(shape, {k_: f"{v * 1e3:.1f} us" for k_, v in ms.items()}, flush=True)
    print(shape, {k_: f"{v:.2f}" for k_, v in row["ratios"].items()}, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    res = {"dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "shapes": [shape_row(s) for s in SHAPES]}
    path = Path(args.out) / "deform_kernels.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
