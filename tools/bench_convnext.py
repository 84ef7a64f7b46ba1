"""ConvNeXt numbers on the GPU (fails without one).

    python tools/bench_convnext.py kernels [--out DIR]   # (a) the vt_layernorm.hip kernels alone -> convnext_kernels.json
    python tools/bench_convnext.py step [--out DIR]      # (b) ConvNeXt-T forward / forward+backward -> convnext_t_step.json
    python tools/bench_convnext.py trace                 # a few steps, for `rocprofv3 --kernel-trace --stats -- python ...`

(a) vt_layernorm_fwd / _bwd and vt_scale_residual_fwd / _bwd on the four stage shapes of ConvNeXt-T at batch 64 @224
(C = 96 / 192 / 384 / 768 at 56^2 / 28^2 / 14^2 / 7^2), bf16: microseconds, algorithmic bytes from the shapes (every operand
read or written once), TB/s.  Beside each LayerNorm forward, vt_bn_act_apply on the same tensors (one read, one write: the
same bytes), timed in the same process, alternating -- the yardstick: a LayerNorm forward adds one in-wave fold per row
to it.  Per kernel: launches are captured into a hipGraph (a Python launch costs more than the small kernels run), every
launch of a graph works on its own set of buffers so that the working set of a replay exceeds the 256 MB memory-side cache,
replays are timed with device events in windows of >= 0.5 s, REPEATS windows per kernel, alternating between the kernels of
a shape; median and spread (min, max) are recorded.

(b) ConvNeXt-T through the module API (compute_dtype = bfloat16), batch 64 @224: forward under no_grad and forward +
backward, device events around windows of >= 0.5 s after warm-up: ms and images/s.
"""
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

STAGES = [(96, 56), (192, 28), (384, 14), (768, 7)]
BATCH, REPEATS, WINDOW_S, WORKING_SET = 64, 7, 0.5, 1.0e9
vp = ctypes.c_void_p


def _graph(launches):
    """one hipGraph of the given launch closures (each takes a stream handle)"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for fn in launches[:2]:
            fn(int(st.cuda_stream))
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for fn in launches:
                fn(int(torch.cuda.current_stream().cuda_stream))
        g.replay()
        st.synchronize()
    return g, st


def _window(g, st, n_launch, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        for _ in range(replays):
            g.replay()
        e1.record(st)
        st.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * n_launch)  # us per launch


def kernels(out_dir: Path):
    lib, dev = N.lib(), torch.device("cuda")
    result = {"batch": BATCH, "dtype": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "shapes": []}
    for C, H in STAGES:
        M = BATCH * H * H
        nbytes = M * C * 2
        nset = max(2, int(WORKING_SET // (3 * nbytes)) + 1)
        bufs = [[torch.randn(M, C, device=dev).to(torch.bfloat16) for _ in range(3)] for _ in range(nset)]
        gamma, beta, bias = (torch.rand(C, device=dev) + 0.5), torch.randn(C, device=dev) * 0.1, torch.randn(C, device=dev) * 0.1
        sums = torch.zeros(N.VT_STAT_REPLICAS, 3, C, 2, dtype=torch.int64, device=dev)
        eps = 1e-6

        def mk(kind):
            fns = []
            for a, b, c in bufs:
                A, B_, C_ = vp(a.data_ptr()), vp(b.data_ptr()), vp(c.data_ptr())
                if kind == "layernorm_fwd":
                    fns.append(lambda s, A=A, B_=B_: N.check(lib.vt_layernorm_fwd(A, C, vp(bias.data_ptr()), vp(gamma.data_ptr()), vp(beta.data_ptr()), B_, C, M, C, eps, N.VT_BF16, vp(s))))
                elif kind == "bn_act_apply":
                    fns.append(lambda s, A=A, B_=B_: N.check(lib.vt_bn_act_apply(A, C, vp(gamma.data_ptr()), vp(beta.data_ptr()), None, 0, B_, C, M, C, 0, N.VT_BF16, vp(s))))
                elif kind == "layernorm_bwd":
                    fns.append(lambda s, A=A, B_=B_, C_=C_: N.check(lib.vt_layernorm_bwd(A, C, B_, C, vp(bias.data_ptr()), vp(gamma.data_ptr()), C_, C, None, 0, vp(sums.data_ptr()), M, C, eps, N.VT_BF16, vp(s))))
                elif kind == "scale_residual_fwd":
                    fns.append(lambda s, A=A, B_=B_, C_=C_: N.check(lib.vt_scale_residual_fwd(A, C, vp(gamma.data_ptr()), B_, C, C_, C, M, C, N.VT_BF16, vp(s))))
                elif kind == "scale_residual_bwd":
                    fns.append(lambda s, A=A, B_=B_, C_=C_: N.check(lib.vt_scale_residual_bwd(A, C, B_, C, vp(gamma.data_ptr()), C_, C, vp(sums.data_ptr()), M, C, N.VT_BF16, vp(s))))
            return fns

        kinds = {"layernorm_fwd": 2, "bn_act_apply": 2, "layernorm_bwd": 3, "scale_residual_fwd": 3, "scale_residual_bwd": 3}
        graphs = {k: _graph(mk(k)) for k in kinds}
        replays = {}
        for k, (g, st) in graphs.items():
            us = _window(g, st, nset, 3)
            replays[k] = max(3, int(WINDOW_S * 1e6 / (us * nset)) + 1)
        samples = {k: [] for k in kinds}
        for _ in range(REPEATS):  # alternating: every kernel of the shape once per round
            for k, (g, st) in graphs.items():
                samples[k].append(_window(g, st, nset, replays[k]))
        row = {"C": C, "H": H, "M": M, "tensor_bytes": nbytes, "buffer_sets": nset, "kernels": {}}
        for k, ntens in kinds.items():
            med = statistics.median(samples[k])
            row["kernels"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                                 "algorithmic_bytes": ntens * nbytes, "TBps": ntens * nbytes / med / 1e6,
                                 "launches_per_window": replays[k] * nset}
        ln, bn = row["kernels"]["layernorm_fwd"], row["kernels"]["bn_act_apply"]
        row["layernorm_fwd_over_bn_act_apply"] = ln["us_median"] / bn["us_median"]
        row["spread_rel"] = {k: (v["us_max"] - v["us_min"]) / v["us_median"] for k, v in row["kernels"].items()}
        result["shapes"].append(row)
        print(json.dumps(row))
        del graphs, bufs
        torch.cuda.empty_cache()
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "convnext_kernels.json").write_text(json.dumps(result, indent=1))


def _model():
    from vision_toolbox.backbones import ConvNeXt

    torch.manual_seed(0)
    m = ConvNeXt.from_config("T")
    with torch.no_grad():
        for b in m.modules():
            if hasattr(b, "gamma") and isinstance(b.gamma, torch.nn.Parameter) and b.gamma.numel() and b.gamma.abs().max() < 1e-3:
                b.gamma.fill_(0.5)  # (the 1e-6 initial layer scale would hide the branches' gradients from a sanity check)
    m = m.cuda().train()
    m.compute_dtype = torch.bfloat16
    return m, torch.randn(BATCH, 3, 224, 224, device="cuda")


def _timed(fn, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(WINDOW_S / max(time.perf_counter() - t0, 1e-4)) + 1)
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return out, n


def step(out_dir: Path):
    m, x = _model()

    def fwd():
        with torch.no_grad():
            m(x)

    def fwd_bwd():
        y = m(x)
        y.float().square().mean().backward()

    res = {"model": "ConvNeXt-T", "batch": BATCH, "size": 224, "dtype": "bf16", "window_s": WINDOW_S}
    for name, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        before = N.launch_count()
        ms, n = _timed(fn)
        med = statistics.median(ms)
        res[name] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "images_per_s": BATCH / med * 1e3,
                     "iterations_per_window": n, "launches_per_iteration": (N.launch_count() - before) / (5 * n + 4)}
        print(name, json.dumps(res[name]))
    g = next(p.grad for k, p in m.named_parameters() if k.endswith("layers.8.gamma"))
    assert torch.isfinite(m(x).float()).all() and torch.isfinite(g).all() and g.abs().max() > 0
    r = m._vt_runner()
    res["kind_histogram"] = {("forward_backward" if k[3] else "forward"): p.kind_histogram for k, p in r.cache.items()}
    res["arena_bytes"] = {("forward_backward" if k[3] else "forward"): p.arena_bytes for k, p in r.cache.items()}
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "convnext_t_step.json").write_text(json.dumps(res, indent=1))


def trace():
    m, x = _model()
    for _ in range(4):
        y = m(x)
        y.float().square().mean().backward()
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step", "trace"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_convnext.py needs a GPU: nothing is measured without one")
    {"kernels": lambda: kernels(Path(a.out)), "step": lambda: step(Path(a.out)), "trace": trace}[a.what]()
