"""BiFPN numbers on the GPU (fails without one).

    python tools/bench_bifpn.py kernels [--out DIR]   # vt_wfuse_fwd / _bwd beside the torch eager composition -> bifpn_kernels.json
    python tools/bench_bifpn.py model [--out DIR]     # BiFPN beside the restatement run by torch           -> bifpn_model.json

kernels, bf16, output grids (B, H, W, C) = (64, 64, 64, 64), (64, 16, 16, 64), (64, 8, 8, 88), with 2 inputs (codes 0, 1: a
top-down node) and 3 inputs (codes 0, 0, 2: a bottom-up node), on the same tensors:
    fwd / fwd_torch   vt_wfuse_fwd / relu(w), F.interpolate(nearest), x_i * w_i, sum, / (sum w + eps) on channels_last views
    bwd / bwd_torch   vt_wfuse_bwd + vt_wfuse_finalize (sums zeroed inside the timing) / torch.autograd.grad of that composition
                      for every input and the weights (the graph is built once, outside the timing)
    copy_fwd / copy_bwd   dst.copy_(src) over as many bytes as the pass's algorithmic bytes: the copy bandwidth of the same box
  TBps = algorithmic bytes (forward: the inputs at their own size + out; backward: g + the inputs + their gradients) over the
  median time.
model: BiFPN([40, 112, 320, 64, 64], 64, num_layers=3), batch 64 on 64x64 ... 4x4 maps, bf16, train mode: forward under no_grad
and forward + backward through the module API, beside the restatement of tests/bifpn_util.py run by torch itself (bf16
autocast, channels_last), in one process.

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

SHAPES = [(64, 64, 64, 64), (64, 16, 16, 64), (64, 8, 8, 88)]
CODES = {2: (0, 1), 3: (0, 0, 2)}
EPS = 1e-4


def _src(shape, code):
    B, H, W, C = shape
    return (B, H, W, C) if code == 0 else ((B, H // 2, W // 2, C) if code == 1 else (B, 2 * H, 2 * W, C))


def _resample(x, code):  # NCHW (channels_last) views
    if code == 1:
        return F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.interpolate(x, scale_factor=0.5, mode="nearest") if code == 2 else x


def kernels():
    lib, dt, bf = N.lib(), N.VT_BF16, torch.bfloat16
    st = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    rows = []
    for shape in SHAPES:
        B, H, W, C = shape
        for n, codes in CODES.items():
            xs = [torch.randn(_src(shape, c), device="cuda").to(bf) for c in codes]
            g, out = torch.randn(shape, device="cuda").to(bf), torch.empty(shape, device="cuda", dtype=bf)
            dxs = [torch.empty_like(x) for x in xs]
            w = (1.0 + 0.25 * torch.randn(n, device="cuda")).abs()
            dw, sums = torch.zeros(n, device="cuda"), torch.zeros(N.VT_STAT_REPLICAS * n * 2, dtype=torch.int64, device="cuda")
            a3 = sum(([vp(xs[k]), C, codes[k]] if k < n else [None, 0, 0] for k in range(3)), [])
            d3 = sum(([vp(dxs[k]), C, 0] if k < n else [None, 0, 0] for k in range(3)), [])

            def fwd():
                N.check(lib.vt_wfuse_fwd(n, *a3, vp(w), EPS, vp(out), C, B, H, W, C, dt, st()))

            def bwd():
                sums.zero_()
                N.check(lib.vt_wfuse_bwd(n, vp(g), C, *a3, vp(w), EPS, *d3, vp(sums), B, H, W, C, dt, st()))
                N.check(lib.vt_wfuse_finalize(vp(sums), vp(w), EPS, n, vp(dw), st()))

            tx = [x.permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
            tw, tg = w.clone().requires_grad_(True), g.permute(0, 3, 1, 2)

            def compose():
                r = F.relu(tw)
                acc = 0
                for k in range(n):
                    acc = acc + _resample(tx[k], codes[k]) * r[k]
                return acc / (r.sum() + EPS)

            def fwd_torch():
                with torch.no_grad():
                    compose()

            graph = compose()

            def bwd_torch():
                torch.autograd.grad(graph, tx + [tw], tg, retain_graph=True)

            by_f = sum(x.numel() for x in xs) * 2 + out.numel() * 2
            by_b = g.numel() * 2 + 2 * sum(x.numel() for x in xs) * 2
            cf, cb = (torch.empty(b // 2, device="cuda", dtype=torch.uint8) for b in (by_f, by_b))
            cf2, cb2 = torch.empty_like(cf), torch.empty_like(cb)
            res = _timed_group({"fwd": fwd, "fwd_torch": fwd_torch, "bwd": bwd, "bwd_torch": bwd_torch,
                                "copy_fwd": lambda: cf2.copy_(cf), "copy_bwd": lambda: cb2.copy_(cb)})
            for k, v in res.items():
                v["TBps"] = (by_f if "fwd" in k else by_b) / (v["ms_median"] * 1e-3) / 1e12
            rows.append({"shape": list(shape), "inputs": n, "codes": list(codes), "bytes_fwd": by_f, "bytes_bwd": by_b, **res})
            print(shape, n, {k: f"{v['ms_median'] * 1e3:.1f} us, {v['TBps']:.2f} TB/s" for k, v in res.items()}, flush=True)
    return {"dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS, "shapes": rows}


def model():
    import bifpn_util as BU
    from vision_toolbox.necks import BiFPN

    ins, outc, layers, B = [40, 112, 320, 64, 64], 64, 3, 64
    sizes = [64, 32, 16, 8, 4]
    m = BiFPN(ins, outc, num_layers=layers)
    BU.fill(m, "bench.")
    ref = BU.RefBiFPN(ins, outc, layers, block="sep")
    ref.load_state_dict(m.state_dict())
    m, ref = m.cuda().train(), ref.cuda().train().to(memory_format=torch.channels_last)
    xs = [torch.randn(B, c, s, s, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for c, s in zip(ins, sizes)]
    seeds = [torch.randn(B, outc, s, s, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for s in sizes]

    def run(mod, grad, autocast):
        def f():
            with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                ys = mod(xs)
            if grad:
                torch.autograd.backward(ys, [s.to(y.dtype) for s, y in zip(seeds, ys)])
        return f

    out = {"config": {"in_channels": ins, "out_channels": outc, "num_layers": layers, "batch": B, "sizes": sizes, "dtype": "bf16"},
           "window_s": WINDOW_S, "windows": WINDOWS}
    before = N.launch_count()
    for key, grad in (("forward", False), ("forward_backward", True)):
        out[key] = _timed_group({"vision_toolbox": run(m, grad, False), "plain_torch": run(ref, grad, True)})
        print(key, {k: f"{v['ms_median']:.3f} ms" for k, v in out[key].items()}, flush=True)
    assert N.launch_count() > before
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    res = kernels() if args.what == "kernels" else model()
    path = Path(args.out) / f"bifpn_{args.what}.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
