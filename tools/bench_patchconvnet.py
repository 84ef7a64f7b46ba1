"""PatchConvNet numbers on the GPU (fails without one).

    python tools/bench_patchconvnet.py kernels [--out DIR]   # the new kernels alone                 -> patchconvnet_kernels.json
    python tools/bench_patchconvnet.py model [--out DIR]     # PatchConvNet-S60 at batch 64, bf16   -> patchconvnet_model.json

kernels, bf16, at the shapes of PatchConvNet-S at 224 px and batch 64 -- map (64, 14, 14, 384), 197 keys:
  * vt_dw3_gelu_pool_fwd against the existing launches it replaces, timed in the same process: vt_dwconv_fwd + the bias / GELU
    pass (vt_bn_act_apply, activation code 4) + vt_global_avgpool_fwd;
  * vt_dw3_gelu_pool_bwd against vt_bn_act_bwd_apply (the GELU backward pass) + vt_dwconv_dgrad + vt_dwconv_wgrad (f32 atomics)
    + vt_colsum;
  * vt_se_gate_fwd / _bwd, vt_channel_stats and vt_pool_attn_fwd / _bwd alone.
model: PatchConvNet.from_config("S", 60) with drop_path 0 at batch 64, 224 px, bf16: forward under no_grad and forward +
backward through the module API, and a plain-torch restatement on the same GPU (the modules' own torch children under
torch.autocast(bfloat16), channels-first as the reference runs it).

Timing: device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows of >= 4 repetitions each; median, min and
max recorded.  Nothing is compared against a threshold."""
import argparse
import copy
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

SHAPE, LK = (64, 14, 14, 384), 197
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
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    B, H, W, C = SHAPE
    HW, M = H * W, B * H * W
    torch.manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    u, da, a, z, zb, dz, du = (rnd(B, H, W, C).to(bf) for _ in range(7))
    dp, pooled, sgate = rnd(B, C).to(bf), rnd(B, C).to(bf), rnd(B, C).to(bf)
    w, bias = 0.3 * rnd(C, 9), 0.1 * rnd(C)
    dw, db, ds = torch.zeros(C, 9, device=dev), torch.zeros(C, device=dev), torch.zeros(B, C, device=dev)
    nbytes = int(lib.vt_dw3_gelu_pool_bwd_scratch_bytes(B, C))
    scratch = torch.empty(nbytes // 4, device=dev)
    stats = N.stats_buffer(C)
    q, o, do, dq = (rnd(B, C).to(bf) for _ in range(4))
    kv, dkv = rnd(B, LK, 2 * C).to(bf), torch.empty(B, LK, 2 * C, device=dev, dtype=bf)
    lse = torch.empty(B, device=dev)
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    geo = (B, H, W, C, 3, 1, 1, 1, dt)

    def fused_fwd():
        N.check(lib.vt_dw3_gelu_pool_fwd(vp(u), C, vp(w), vp(bias), vp(a), C, vp(pooled), C, B, H, W, C, dt, s()))

    def unfused_fwd():
        N.check(lib.vt_dwconv_fwd(vp(u), C, vp(w), vp(z), C, None, *geo, s()))
        N.check(lib.vt_bn_act_apply(vp(z), C, None, vp(bias), None, 0, vp(a), C, M, C, 4, dt, s()))
        N.check(lib.vt_global_avgpool_fwd(vp(a), C, vp(pooled), C, B, HW, C, dt, s()))

    def fused_bwd():
        N.check(lib.vt_dw3_gelu_pool_bwd(vp(u), C, vp(da), C, vp(dp), C, vp(w), vp(bias), vp(du), C, None, 0, vp(dw), vp(db),
                                         vp(scratch), nbytes, B, H, W, C, dt, s()))

    def unfused_bwd():
        N.check(lib.vt_bn_act_bwd_apply(vp(da), C, vp(zb), C, None, None, None, vp(dz), C, M, C, 4, dt, s()))
        N.check(lib.vt_dwconv_dgrad(vp(dz), C, vp(w), vp(du), C, None, 0, *geo, s()))
        N.check(lib.vt_dwconv_wgrad(vp(u), C, vp(dz), C, vp(dw), *geo, s()))
        N.check(lib.vt_colsum(vp(dz), C, M, C, dt, vp(db), s()))

    def se_fwd():
        N.check(lib.vt_se_gate_fwd(vp(a), C, vp(sgate), C, vp(z), C, B, HW, C, dt, s()))

    def se_bwd():
        N.check(lib.vt_se_gate_bwd(vp(da), C, vp(a), C, vp(sgate), C, vp(dz), C, vp(ds), B, HW, C, 0, dt, s()))

    def chan_stats():
        N.check(lib.vt_channel_stats(vp(u), C, M, C, dt, vp(stats), s()))

    k, v, dk, dv = kv[..., :C], kv[..., C:], dkv[..., :C], dkv[..., C:]

    def pool_fwd():
        N.check(lib.vt_pool_attn_fwd(vp(q), C, vp(k), 2 * C, vp(v), 2 * C, vp(o), C, vp(lse), C ** -0.5, B, LK, C, dt, s()))

    def pool_bwd():
        N.check(lib.vt_pool_attn_bwd(vp(q), C, vp(k), 2 * C, vp(v), 2 * C, vp(o), C, vp(do), C, vp(lse), vp(dq), C, vp(dk), 2 * C,
                                     vp(dv), 2 * C, C ** -0.5, B, LK, C, dt, s()))

    res = {"shape": list(SHAPE), "keys": LK, "dtype": "bf16", "window_s": WINDOW_S, "bwd_scratch_bytes": nbytes}
    for name, fn in (("dw3_gelu_pool_fwd", fused_fwd), ("dwconv_fwd+bias_gelu+avgpool", unfused_fwd), ("dw3_gelu_pool_bwd", fused_bwd),
                     ("gelu_bwd+dwconv_dgrad+dwconv_wgrad+colsum", unfused_bwd), ("se_gate_fwd", se_fwd), ("se_gate_bwd", se_bwd),
                     ("channel_stats", chan_stats), ("pool_attn_fwd", pool_fwd), ("pool_attn_bwd", pool_bwd)):
        res[name] = _timed(fn)
        print(name, json.dumps(res[name]))
    res["fwd_fused_over_unfused"] = res["dw3_gelu_pool_fwd"]["ms_median"] / res["dwconv_fwd+bias_gelu+avgpool"]["ms_median"]
    res["bwd_fused_over_unfused"] = (res["dw3_gelu_pool_bwd"]["ms_median"] /
                                     res["gelu_bwd+dwconv_dgrad+dwconv_wgrad+colsum"]["ms_median"])
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "patchconvnet_kernels.json").write_text(json.dumps(res, indent=1))


def _torch_forward(m, x):
    """the reference's forward restated over the modules' own torch children (their forward() refuses CUDA tensors)"""
    o = m.stem(x)
    for blk in m.trunk:
        o = blk._eager(o) if hasattr(blk, "_eager") else blk(o)
    return m.pool._eager(o.flatten(1, 2))


def model(out_dir: Path):
    from vision_toolbox.backbones import PatchConvNet

    torch.manual_seed(0)
    m = PatchConvNet(384, 60, drop_path=0.0)
    with torch.no_grad():  # (layer scales of 1e-6 would leave the trunk's backward multiplying by nothing)
        for k, p in m.named_parameters():
            if k.rsplit(".", 1)[-1].startswith("layer_scale"):
                p.fill_(0.1)
    ref = copy.deepcopy(m).cuda().train().to(memory_format=torch.channels_last)
    m = m.cuda().train()
    m.compute_dtype = torch.bfloat16
    x = torch.randn(64, 3, 224, 224, device="cuda")

    def fwd():
        with torch.no_grad():
            m(x)

    def fwd_bwd():
        m(x).float().square().mean().backward()

    def torch_fwd():
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            _torch_forward(ref, x)

    def torch_fwd_bwd():
        for p in ref.parameters():
            p.grad = None
        with torch.autocast("cuda", torch.bfloat16):
            y = _torch_forward(ref, x)
        y.float().square().mean().backward()

    res = {"model": "PatchConvNet-S60 (drop_path 0)", "batch": 64, "size": 224, "dtype": "bf16"}
    for name, fn in (("forward", fwd), ("forward_backward", fwd_bwd), ("torch_forward", torch_fwd),
                     ("torch_forward_backward", torch_fwd_bwd)):
        res[name] = _timed(fn)
        res[name]["images_per_s"] = 64 / res[name]["ms_median"] * 1e3
        print(name, json.dumps(res[name]))
    res["forward_over_torch"] = res["forward"]["ms_median"] / res["torch_forward"]["ms_median"]
    res["forward_backward_over_torch"] = res["forward_backward"]["ms_median"] / res["torch_forward_backward"]["ms_median"]
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "patchconvnet_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_patchconvnet.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
