"""ViT numbers on the GPU (fails without one).

    python tools/bench_vit.py kernels [--out DIR]   # (a) vt_attn_fwd / vt_attn_bwd alone        -> vit_kernels.json
    python tools/bench_vit.py step [--out DIR]      # (b) ViT-S/16 through the module API        -> vit_step.json
    python tools/bench_vit.py trace                 # a few steps, for `rocprofv3 --kernel-trace --stats -- python ...`

(a) vt_attn_fwd and vt_attn_bwd (dQ, dK and dV) at (B, heads, L, head_dim) = (64, 6, 197, 64) and (64, 12, 197, 64), bf16,
with Q | K | V as the three channel slices of one [B][L][3 d] buffer, as the launch lists hold them.  Yardstick, timed in the
same process, alternating with the kernels: torch's F.scaled_dot_product_attention forward, and its backward alone
(torch.autograd.grad over a retained graph), on the same bf16 values in torch's own preferred layout, contiguous
(B, heads, L, head_dim) -- the transposes the reference pays to get there are NOT charged to torch.  Every launch works on its
own buffer set so that a pass over the sets exceeds the 256 MB memory-side cache.  Two ways of timing, both with device events
in windows of >= 0.3 s after warm-up, REPEATS (>= 20 launches each) windows per kernel, alternating; median, min and max
recorded: `eager` -- every kernel and every torch call issued from Python on the current stream, the like-for-like comparison
(`*_over_torch`); and `graph` -- the library's launches captured into a hipGraph and replayed, which leaves the Python launch
cost out (the library's own kernels only: the autograd engine runs a backward on its own thread and does not belong in a stream
capture).  TFLOP/s counts 4 B h L^2 D for the forward and 10 B h L^2 D for the backward (five products, the recomputed scores
included).

(b) ViT-S/16, batch 64 at 224, bf16, through the module API: forward under no_grad and forward + backward, against `TorchViT`
below -- a plain-torch restatement of the same network written for this tool (one fused qkv Linear, F.scaled_dot_product_
attention, nn.LayerNorm, F.gelu) -- under bf16 autocast on the same GPU.
"""
import argparse
import ctypes
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT)]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from vision_toolbox import _native as N  # noqa: E402

SHAPES = [(64, 6, 197, 64), (64, 12, 197, 64)]
REPEATS, WINDOW_S, WORKING_SET = 7, 0.3, 0.6e9
vp = ctypes.c_void_p
faulthandler.enable()  # a crash inside a library leaves the Python stack on stderr


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


def _eager_window(fns, reps):
    """us per call of `fns` issued from Python on the current stream, `reps` passes over the buffer sets"""
    s = int(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for fn in fns:
            fn(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(fns))


def kernels(out_dir: Path):
    lib, dev, bf = N.lib(), torch.device("cuda"), torch.bfloat16
    rows = []
    for B, H, L, D in SHAPES:
        C, scale = H * D, D ** -0.5
        per_set = B * L * C * 2 * 8  # qkv (3), o, do, dqkv (3)
        nset = max(2, int(WORKING_SET // per_set) + 1)
        nscr = int(lib.vt_attn_bwd_scratch_bytes(B, H, L))
        scratch = torch.zeros(nscr // 4, device=dev)
        sets = []
        for _ in range(nset):
            s_ = dict(qkv=torch.randn(B, L, 3 * C, device=dev).to(bf), o=torch.empty(B, L, C, device=dev, dtype=bf),
                      do=torch.randn(B, L, C, device=dev).to(bf), dqkv=torch.empty(B, L, 3 * C, device=dev, dtype=bf),
                      lse=torch.empty(B, H, L, device=dev))
            # torch's operands: the same values, contiguous (B, H, L, D), with a retained graph for the backward alone
            s_["t"] = [s_["qkv"][:, :, i * C:(i + 1) * C].reshape(B, L, H, D).transpose(1, 2).contiguous().requires_grad_(True)
                       for i in range(3)]
            s_["tdo"] = s_["do"].reshape(B, L, H, D).transpose(1, 2).contiguous()
            s_["to"] = F.scaled_dot_product_attention(*s_["t"])
            sets.append(s_)

        def mk(kind):
            fns = []
            for s_ in sets:
                q, k, v = (vp(s_["qkv"].data_ptr() + i * C * 2) for i in range(3))
                dq, dk, dv = (vp(s_["dqkv"].data_ptr() + i * C * 2) for i in range(3))
                o, do, lse = vp(s_["o"].data_ptr()), vp(s_["do"].data_ptr()), vp(s_["lse"].data_ptr())
                if kind == "attn_fwd":
                    fns.append(lambda s, q=q, k=k, v=v, o=o, lse=lse: N.check(lib.vt_attn_fwd(
                        q, 3 * C, k, 3 * C, v, 3 * C, o, C, lse, scale, B, H, L, D, N.VT_BF16, vp(s))))
                elif kind == "attn_bwd":
                    fns.append(lambda s, q=q, k=k, v=v, o=o, do=do, lse=lse, dq=dq, dk=dk, dv=dv: N.check(lib.vt_attn_bwd(
                        q, 3 * C, k, 3 * C, v, 3 * C, o, C, do, C, lse, dq, 3 * C, dk, 3 * C, dv, 3 * C, vp(scratch.data_ptr()),
                        nscr, scale, B, H, L, D, N.VT_BF16, vp(s))))
                elif kind == "torch_attn_fwd":
                    def f(s, s_=s_):
                        with torch.no_grad():
                            F.scaled_dot_product_attention(*s_["t"])
                    fns.append(f)
                elif kind == "torch_attn_bwd":
                    def f(s, s_=s_):
                        torch.autograd.grad(s_["to"], s_["t"], s_["tdo"], retain_graph=True)
                    fns.append(f)
            return fns

        kinds = {"attn_fwd": 4.0, "torch_attn_fwd": 4.0, "attn_bwd": 10.0, "torch_attn_bwd": 10.0}
        eager = {k: mk(k) for k in kinds}
        graphs = {k: _graph(eager[k]) for k in ("attn_fwd", "attn_bwd")}  # (forward first: the backward reads its o and lse)
        reps, replays = {}, {}
        for k, fns in eager.items():
            _eager_window(fns, 1)
            reps[k] = max(2, -(-20 // nset), int(WINDOW_S * 1e6 / (_eager_window(fns, 2) * nset)) + 1)
        for k, (g, st) in graphs.items():
            replays[k] = max(3, -(-20 // nset), int(WINDOW_S * 1e6 / (_window(g, st, nset, 3) * nset)) + 1)
        samples, gsamples = {k: [] for k in kinds}, {k: [] for k in graphs}
        for _ in range(REPEATS):
            for k, fns in eager.items():
                samples[k].append(_eager_window(fns, reps[k]))
            for k, (g, st) in graphs.items():
                gsamples[k].append(_window(g, st, nset, replays[k]))
        row = {"B": B, "heads": H, "L": L, "head_dim": D, "buffer_sets": nset, "eager": {}, "graph": {}}
        for mode, smp, cnt in (("eager", samples, reps), ("graph", gsamples, replays)):
            for k in smp:
                med = statistics.median(smp[k])
                row[mode][k] = {"us_median": med, "us_min": min(smp[k]), "us_max": max(smp[k]),
                                "TFLOPs": kinds[k] * B * H * L * L * D / med / 1e6, "launches_per_window": cnt[k] * nset}
        for k in ("attn_fwd", "attn_bwd"):
            row[f"{k}_over_torch"] = row["eager"][k]["us_median"] / row["eager"]["torch_" + k]["us_median"]
        rows.append(row)
        print(json.dumps(row))
        del graphs, eager, sets
        torch.cuda.empty_cache()
    _write(out_dir, "vit_kernels.json", {"dtype": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "shapes": rows})


def _write(out_dir: Path, name: str, doc) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / name).write_text(json.dumps(doc, indent=1))


class TorchBlock(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.heads = heads
        self.ln1, self.ln2 = nn.LayerNorm(d, 1e-6), nn.LayerNorm(d, 1e-6)
        self.qkv, self.proj = nn.Linear(d, 3 * d), nn.Linear(d, d)
        self.fc1, self.fc2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)

    def forward(self, x):
        B, L, d = x.shape
        q, k, v = self.qkv(self.ln1(x)).view(B, L, 3, self.heads, d // self.heads).permute(2, 0, 3, 1, 4)
        x = x + self.proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, d))
        return x + self.fc2(F.gelu(self.fc1(self.ln2(x))))


class TorchViT(nn.Module):
    """the same network in plain torch: patch embedding, class token, pe, blocks, class-token pooling"""

    def __init__(self, d, depth, heads, patch, img):
        super().__init__()
        self.embed = nn.Conv2d(3, d, patch, patch)
        self.cls = nn.Parameter(torch.zeros(1, 1, d))
        self.pe = nn.Parameter(torch.randn(1, (img // patch) ** 2, d) * 0.02)
        self.blocks = nn.Sequential(*[TorchBlock(d, heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(d, 1e-6)

    def forward(self, x):
        t = self.embed(x).flatten(2).transpose(1, 2) + self.pe
        t = torch.cat([self.cls.expand(t.shape[0], -1, -1), t], 1)
        return self.norm(self.blocks(t)[:, 0])


def _model():
    from vision_toolbox.backbones import ViT

    torch.manual_seed(0)
    m = ViT.from_config("S_16", 224).cuda().train()
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
    m, x = _model()
    ref = TorchViT(384, 12, 6, 16, 224).cuda().train()

    def fwd():
        with torch.no_grad():
            m(x)

    def fwd_bwd():
        m(x).float().square().mean().backward()

    def torch_fwd():
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            ref(x)

    def torch_fwd_bwd():
        with torch.autocast("cuda", torch.bfloat16):
            y = ref(x)
        y.float().square().mean().backward()

    row = {}
    for name, fn in (("forward", fwd), ("torch_forward", torch_fwd), ("forward_backward", fwd_bwd),
                     ("torch_forward_backward", torch_fwd_bwd)):
        row[name] = _timed(fn)
        row[name]["images_per_s"] = 64 / row[name]["ms_median"] * 1e3
        print(name, json.dumps(row[name]))
    row["forward_over_torch"] = row["forward"]["ms_median"] / row["torch_forward"]["ms_median"]
    row["forward_backward_over_torch"] = row["forward_backward"]["ms_median"] / row["torch_forward_backward"]["ms_median"]
    prog = next(iter(m._vt_runner().cache.values()))
    row["kind_histogram"] = prog.kind_histogram
    _write(out_dir, "vit_step.json", {"model": "ViT-S/16", "batch": 64, "size": 224, "dtype": "bf16", **row})


def trace():
    m, x = _model()
    for _ in range(4):
        m(x).float().square().mean().backward()
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step", "trace"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_vit.py needs a GPU: nothing is measured without one")
    {"kernels": lambda: kernels(Path(a.out)), "step": lambda: step(Path(a.out)), "trace": trace}[a.what]()
