"""CaiT numbers on the GPU (fails without one).

    python tools/bench_cait.py kernels [--out DIR]   # the talking-heads kernels alone        -> cait_kernels.json
    python tools/bench_cait.py model [--out DIR]     # CaiT-XXS24 at batch 64, through the API  -> cait_model.json

kernels: vt_talk_attn_fwd and vt_talk_attn_bwd (dq, dk, dv and the four parameter gradients) at (B, H, L, D) = (64, 4, 196, 48)
and (64, 8, 196, 48), bf16, against a plain-torch restatement on the same GPU that materialises the (B, H, L, L) planes as the
reference does (matmul, einsum mix, softmax, einsum mix, matmul; the backward through autograd, timed as forward + backward
minus forward).  model: CaiT.from_config("xxs_24", 224) at batch 64, bf16, forward under no_grad and forward + backward
through the module API (the blocks' torch children refuse CUDA tensors, so there is no eager yardstick for the whole model).

Timing: device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows of >= 4 repetitions each; median, min and
max recorded.  Nothing is compared against a threshold."""
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

SHAPES = [(64, 4, 196, 48), (64, 8, 196, 48)]
WINDOW_S = 0.3
vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731


def _timed(fn, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(4, int(WINDOW_S / max(time.perf_counter() - t0, 1e-4)) + 1)
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out), "repetitions": 5 * n}


def kernels(out_dir: Path):
    lib, dev, bf = N.lib(), torch.device("cuda"), torch.bfloat16
    rows = []
    for B, H, L, D in SHAPES:
        C, scale = H * D, D ** -0.5
        torch.manual_seed(0)
        qkv = torch.randn(B, L, 3 * C, device=dev).to(bf)
        q, k, v = (qkv[:, :, i * C:(i + 1) * C] for i in range(3))
        do = torch.randn(B, L, C, device=dev).to(bf)
        o, dqkv = torch.empty(B, L, C, device=dev, dtype=bf), torch.empty(B, L, 3 * C, device=dev, dtype=bf)
        dq, dk, dv = (dqkv[:, :, i * C:(i + 1) * C] for i in range(3))
        lse = torch.empty(B, H, L, device=dev)
        wl, ww = torch.randn(H, H, device=dev) / H ** 0.5, torch.randn(H, H, device=dev) / H ** 0.5
        bl, bw = torch.randn(H, device=dev), torch.randn(H, device=dev)
        pg = [torch.zeros_like(t) for t in (wl, bl, ww, bw)]
        nbytes = int(lib.vt_talk_attn_bwd_scratch_bytes(B, H, L))
        scratch = torch.empty(nbytes // 4, device=dev)
        s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731

        def fwd():
            N.check(lib.vt_talk_attn_fwd(vp(q), 3 * C, vp(k), 3 * C, vp(v), 3 * C, vp(o), C, vp(lse), vp(wl), vp(bl), vp(ww), vp(bw),
                                         scale, B, H, L, D, N.VT_BF16, s()))

        def bwd():
            N.check(lib.vt_talk_attn_bwd(vp(q), 3 * C, vp(k), 3 * C, vp(v), 3 * C, vp(do), C, vp(lse), vp(wl), vp(bl), vp(ww), vp(bw),
                                         vp(dq), 3 * C, vp(dk), 3 * C, vp(dv), 3 * C, *[vp(g) for g in pg], vp(scratch), nbytes, scale,
                                         B, H, L, D, N.VT_BF16, s()))

        leaves = [t.detach().clone().requires_grad_(True) for t in (qkv, wl.to(bf), bl.to(bf), ww.to(bf), bw.to(bf))]

        def torch_fwd(grad=False):
            with torch.set_grad_enabled(grad):
                x, a, b_, c, d = leaves
                qh, kh, vh = (x[:, :, i * C:(i + 1) * C].reshape(B, L, H, D).transpose(1, 2) for i in range(3))
                m = torch.einsum("gh,bhij->bgij", a, qh @ (kh * scale).transpose(-1, -2)) + b_[None, :, None, None]
                r = torch.einsum("gh,bhij->bgij", c, torch.softmax(m, -1)) + d[None, :, None, None]
                return (r @ vh).transpose(1, 2).reshape(B, L, C)

        def torch_fwd_bwd():
            for t in leaves:
                t.grad = None
            torch_fwd(True).backward(do)

        row = {"B": B, "H": H, "L": L, "D": D, "dtype": "bf16", "bwd_scratch_bytes": nbytes}
        for name, fn in (("talk_attn_fwd", fwd), ("talk_attn_bwd", bwd), ("torch_fwd", torch_fwd), ("torch_fwd_bwd", torch_fwd_bwd)):
            row[name] = _timed(fn)
        row["torch_bwd_ms"] = row["torch_fwd_bwd"]["ms_median"] - row["torch_fwd"]["ms_median"]
        row["fwd_over_torch"] = row["talk_attn_fwd"]["ms_median"] / row["torch_fwd"]["ms_median"]
        row["bwd_over_torch"] = row["talk_attn_bwd"]["ms_median"] / row["torch_bwd_ms"]
        print(json.dumps(row))
        rows.append(row)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "cait_kernels.json").write_text(json.dumps({"window_s": WINDOW_S, "shapes": rows}, indent=1))


def model(out_dir: Path):
    from vision_toolbox.backbones import CaiT

    torch.manual_seed(0)
    m = CaiT.from_config("xxs_24", 224).cuda().train()
    m.compute_dtype = torch.bfloat16
    x = torch.randn(64, 3, 224, 224, device="cuda")

    def fwd():
        with torch.no_grad():
            m(x)

    def fwd_bwd():
        m(x).float().square().mean().backward()

    res = {"model": "CaiT-XXS24", "batch": 64, "size": 224, "dtype": "bf16"}
    for name, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        res[name] = _timed(fn)
        res[name]["images_per_s"] = 64 / res[name]["ms_median"] * 1e3
        print(name, json.dumps(res[name]))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "cait_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_cait.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
