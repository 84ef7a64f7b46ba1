"""MLP-Mixer numbers on the GPU (fails without one).

    python tools/bench_mlp_mixer.py kernels [--out DIR]   # (a) the vt_token_mix.hip kernels alone -> mlp_mixer.json["kernels"]
    python tools/bench_mlp_mixer.py step [--out DIR]      # (b) whole models and the train step   -> mlp_mixer.json["step"]
    python tools/bench_mlp_mixer.py trace                 # a few steps, for `rocprofv3 --kernel-trace --stats -- python ...`

(a) Each token-mix kernel on the Mixer-S/16 (196 tokens -> 256, d_model 512) and B/16 (196 -> 384, 768) shapes at batch 64
and 256, bf16: the fused forward (bias + pre-activation + exact GELU from one launch), the second linear with the shortcut
fused, the data gradient (W read transposed, accumulating) and the filter + bias gradient.  Per kernel: microseconds,
algorithmic bytes from the shapes (every operand read or written once; W counted once), TB/s and TFLOP/s.  Two yardsticks,
timed in the same process, alternating with the kernels:
  * torch on the same GPU: `torch.matmul(W, X) + bias` then `F.gelu` in bf16 for the forward (three passes); for the
    gradients the products autograd issues for that matmul, called directly so that no forward is timed with them
    (`W.t() @ dz` accumulated, and the batch-reduced `dz x^T` with the bias column sums);
  * vt_bn_act_apply on tensors of the same bytes (one read, one write): the library's streaming rate.
Launches are captured into a hipGraph (a Python launch costs more than a small kernel runs); every launch of a graph works on
its own buffer set so that a replay's working set exceeds the 256 MB memory-side cache; replays are timed with device events in
windows of >= 0.3 s after warm-up, REPEATS (>= 20 launches each) windows per kernel, alternating; median, min and max recorded.

(b) Mixer-S/16 and B/16, batch 64 at 224, bf16, through the module API: forward under no_grad and forward + backward, against
the module's own torch children called on CUDA tensors under bf16 autocast (`_eager_maps`: the baseline).  Then the fused
TrainStep (AdamW, include_pool=False) and the token-mixing share of it: the step's own VT_OP_TOKEN_MIX / VT_OP_TOKEN_WGRAD ops
replayed alone over the step's buffers, as a fraction of the step.
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
import torch.nn.functional as F  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

SHAPES = {"S/16": (196, 256, 512), "B/16": (196, 384, 768)}  # tokens K, hidden tokens M, channels C
BATCHES, REPEATS, WINDOW_S, WORKING_SET = (64, 256), 7, 0.3, 0.6e9
vp = ctypes.c_void_p


def _graph(launches):
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
    lib, dev, bf = N.lib(), torch.device("cuda"), torch.bfloat16
    rows = []
    for name, (K, M, C) in SHAPES.items():
        for B in BATCHES:
            xb, zb = B * K * C * 2, B * M * C * 2
            nset = max(2, int(WORKING_SET // (2 * xb + 3 * zb)) + 1)
            W = (torch.randn(M, K, device=dev) / K ** 0.5).to(bf)
            W2 = (torch.randn(K, M, device=dev) / M ** 0.5).to(bf)
            bias, bias2 = torch.randn(M, device=dev), torch.randn(K, device=dev)
            dW, db = torch.zeros(M, K, device=dev), torch.zeros(M, device=dev)
            nscr = int(lib.vt_token_mix_wgrad_scratch_bytes(B, K, M, C, N.VT_BF16))
            scratch = torch.zeros(nscr // 4, device=dev)
            sets = [dict(x=torch.randn(B, K, C, device=dev).to(bf), z=torch.empty(B, M, C, device=dev, dtype=bf),
                         a=torch.randn(B, M, C, device=dev).to(bf), y=torch.empty(B, K, C, device=dev, dtype=bf),
                         dz=torch.randn(B, M, C, device=dev).to(bf)) for _ in range(nset)]
            one = torch.ones(C, device=dev)

            def mk(kind):
                fns = []
                for s_ in sets:
                    x, z, a, y, dz = (vp(s_[k].data_ptr()) for k in ("x", "z", "a", "y", "dz"))
                    if kind == "fwd_gelu":  # linear1: z and gelu(z)
                        fns.append(lambda s, x=x, z=z, a=a: N.check(lib.vt_token_mix_fwd(
                            x, C, vp(W.data_ptr()), K, 0, vp(bias.data_ptr()), None, 0, z, C, a, C, 4, B, K, M, C, N.VT_BF16, vp(s))))
                    elif kind == "fwd_residual":  # linear2: y = x + W2 a + bias
                        fns.append(lambda s, x=x, a=a, y=y: N.check(lib.vt_token_mix_fwd(
                            a, C, vp(W2.data_ptr()), M, 0, vp(bias2.data_ptr()), x, C, y, C, None, 0, 0, B, M, K, C, N.VT_BF16, vp(s))))
                    elif kind == "dgrad":  # dx = W^T dz + dx
                        fns.append(lambda s, dz=dz, y=y: N.check(lib.vt_token_mix_fwd(
                            dz, C, vp(W.data_ptr()), K, 1, None, y, C, y, C, None, 0, 0, B, M, K, C, N.VT_BF16, vp(s))))
                    elif kind == "wgrad":
                        fns.append(lambda s, dz=dz, x=x: N.check(lib.vt_token_mix_wgrad(
                            dz, C, x, C, vp(dW.data_ptr()), vp(db.data_ptr()), vp(scratch.data_ptr()), nscr, B, K, M, C, N.VT_BF16, vp(s))))
                    elif kind == "bn_act_apply_x_to_x":  # streaming yardstick over the bytes of x -> one tensor of x's size
                        fns.append(lambda s, x=x, y=y: N.check(lib.vt_bn_act_apply(
                            x, C, vp(one.data_ptr()), vp(one.data_ptr()), None, 0, y, C, B * K, C, 0, N.VT_BF16, vp(s))))
                    elif kind == "torch_fwd_gelu":
                        def f(s, s_=s_):
                            zt = torch.matmul(W, s_["x"]) + bias.to(bf)[None, :, None]
                            s_["a"].copy_(F.gelu(zt))
                        fns.append(f)
                    elif kind == "torch_fwd_residual":
                        def f(s, s_=s_):
                            s_["y"].copy_(s_["x"] + torch.matmul(W2, s_["a"]) + bias2.to(bf)[None, :, None])
                        fns.append(f)
                    elif kind == "torch_dgrad":
                        def f(s, s_=s_):
                            s_["y"].add_(torch.matmul(W.t(), s_["dz"]))
                        fns.append(f)
                    elif kind == "torch_wgrad":
                        def f(s, s_=s_):
                            dW.add_(torch.einsum("bmc,bkc->mk", s_["dz"], s_["x"]).float())
                            db.add_(s_["dz"].float().sum((0, 2)))
                        fns.append(f)
                return fns

            flops = 2.0 * B * M * K * C
            wbytes = M * K * 2
            kinds = {  # name -> (algorithmic bytes, flops)
                "fwd_gelu": (xb + 2 * zb + wbytes, flops), "torch_fwd_gelu": (xb + 2 * zb + wbytes, flops),
                "fwd_residual": (zb + 2 * xb + wbytes, flops), "torch_fwd_residual": (zb + 2 * xb + wbytes, flops),
                "dgrad": (zb + 2 * xb + wbytes, flops), "torch_dgrad": (zb + 2 * xb + wbytes, flops),
                "wgrad": (zb + xb + M * K * 4, flops), "torch_wgrad": (zb + xb + M * K * 4, flops),
                "bn_act_apply_x_to_x": (2 * xb, 0.0),
            }
            graphs = {k: _graph(mk(k)) for k in kinds}
            replays = {}
            for k, (g, st) in graphs.items():
                us = _window(g, st, nset, 3)
                replays[k] = max(3, -(-20 // nset), int(WINDOW_S * 1e6 / (us * nset)) + 1)
            samples = {k: [] for k in kinds}
            for _ in range(REPEATS):
                for k, (g, st) in graphs.items():
                    samples[k].append(_window(g, st, nset, replays[k]))
            row = {"model": name, "batch": B, "K": K, "M": M, "C": C, "buffer_sets": nset, "wgrad_scratch_bytes": nscr, "kernels": {}}
            for k, (nb, fl) in kinds.items():
                med = statistics.median(samples[k])
                row["kernels"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                                     "algorithmic_bytes": nb, "TBps": nb / med / 1e6, "TFLOPs": fl / med / 1e6,
                                     "launches_per_window": replays[k] * nset}
            for k in ("fwd_gelu", "fwd_residual", "dgrad", "wgrad"):
                row[f"{k}_over_torch"] = row["kernels"][k]["us_median"] / row["kernels"]["torch_" + k]["us_median"]
            rows.append(row)
            print(json.dumps(row))
            del graphs, sets
            torch.cuda.empty_cache()
    _merge(out_dir, "kernels", {"dtype": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "shapes": rows})


def _merge(out_dir: Path, key: str, value) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    path = out_dir / "mlp_mixer.json"
    doc = json.loads(path.read_text()) if path.exists() else {}
    doc[key] = value
    path.write_text(json.dumps(doc, indent=1))


def _model(variant):
    from vision_toolbox.backbones import MLPMixer

    torch.manual_seed(0)
    m = MLPMixer.from_config(variant, 16, 224).cuda().train()
    m.compute_dtype = torch.bfloat16
    return m, torch.randn(64, 3, 224, 224, device="cuda")


def _timed(fn, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(4, int(WINDOW_S / max(time.perf_counter() - t0, 1e-4)) + 1)
    out = []
    for _ in range(5):  # 5 windows of n >= 4 repetitions: at least 20 timed repetitions
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out), "repetitions": 5 * n}


def step(out_dir: Path):
    from vision_toolbox import engine as E
    from vision_toolbox.trainer import TrainStep

    res = {"batch": 64, "size": 224, "dtype": "bf16", "models": {}}
    for variant in ("S", "B"):
        m, x = _model(variant)

        def fwd():
            with torch.no_grad():
                m(x)

        def fwd_bwd():
            m(x).float().square().mean().backward()

        def torch_fwd():
            with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
                m._eager_maps(x)

        def torch_fwd_bwd():
            with torch.autocast("cuda", torch.bfloat16):
                y = m._eager_maps(x)[0]
            y.float().square().mean().backward()

        row = {}
        for name, fn in (("forward", fwd), ("torch_forward", torch_fwd), ("forward_backward", fwd_bwd),
                         ("torch_forward_backward", torch_fwd_bwd)):
            row[name] = _timed(fn)
            row[name]["images_per_s"] = 64 / row[name]["ms_median"] * 1e3
            print(variant, name, json.dumps(row[name]))
        del m
        torch.cuda.empty_cache()
        from vision_toolbox.backbones import MLPMixer

        ts = TrainStep(MLPMixer.from_config(variant, 16, 224), 1000, 64, 224, torch.bfloat16, optimizer="AdamW", lr=1e-4,
                       include_pool=False, device="cuda")
        ts.images.normal_()
        ts.labels.random_(0, 1000)
        row["train_step_adamw"] = _timed(lambda: ts.step())
        # the step's own token-mixing ops, replayed alone over the step's buffers (in line, one stream)
        p = ts.prog
        tok = [op for ops, n in ((p.fwd_ops, p.n_fwd), (p.bwd_ops, p.n_bwd)) for op in (ops[i] for i in range(n))
               if (op.kind & 0xFFFF) in (N.OP_TOKEN_MIX, N.OP_TOKEN_WGRAD)]
        arr = E.ops_array(tok)
        s = int(torch.cuda.current_stream().cuda_stream)
        row["token_mixing_ops_alone"] = _timed(lambda: N.run_ops(arr, len(tok), ts.bases, s))
        row["token_mixing_ops"] = len(tok)
        row["token_mixing_share_of_step"] = row["token_mixing_ops_alone"]["ms_median"] / row["train_step_adamw"]["ms_median"]
        row["kind_histogram"] = p.kind_histogram
        print(variant, "train step", json.dumps({k: row[k] for k in ("train_step_adamw", "token_mixing_ops_alone",
                                                                      "token_mixing_share_of_step")}))
        res["models"][f"Mixer-{variant}/16"] = row
        del ts
        torch.cuda.empty_cache()
    _merge(out_dir, "step", res)


def trace():
    m, x = _model("S")
    for _ in range(4):
        m(x).float().square().mean().backward()
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step", "trace"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_mlp_mixer.py needs a GPU: nothing is measured without one")
    {"kernels": lambda: kernels(Path(a.out)), "step": lambda: step(Path(a.out)), "trace": trace}[a.what]()
