"""Swin Transformer numbers on the GPU (fails without one).

    python tools/bench_swin.py kernels [--out DIR]   # (a) vt_win_attn_fwd / vt_win_attn_bwd alone   -> swin_kernels.json
    python tools/bench_swin.py step [--out DIR]      # (b) Swin-T through the module API             -> swin_step.json
    python tools/bench_swin.py trace                 # a few steps, for `rocprofv3 --kernel-trace --stats -- python ...`

(a) vt_win_attn_fwd and vt_win_attn_bwd (dQ, dK, dV and d table) at the four stage shapes of Swin-T at batch 64 and 224 px,
(B, H, W, heads, ws, shift) = (64, 56, 56, 3, 7, 3), (64, 28, 28, 6, 7, 3), (64, 14, 14, 12, 7, 3), (64, 7, 7, 24, 7, 0), bf16,
with Q | K | V as the three channel slices of one [B][H][W][3 C] buffer, as the launch lists hold them.  Yardstick, timed in
the same process, alternating with the kernels: torch's F.scaled_dot_product_attention with an additive `attn_mask` (bias +
shift mask, materialised once as (B windows, heads, 49, 49) bf16 outside the timed region), forward, and its backward alone
(torch.autograd.grad over a retained graph; no gradient of the bias is asked of it), on the same bf16 values already rolled,
partitioned and transposed into contiguous (B windows, heads, 49, 32) -- the roll, partition and transposes the reference pays
to get there are NOT charged to torch.  Every launch works on its own buffer set so that a pass over the sets exceeds the
256 MB memory-side cache.  Device events around windows of >= 0.3 s after warm-up, REPEATS windows per kernel (>= 20 launches
each), alternating; median, min and max recorded.

(b) Swin-T, batch 64 at 224, bf16, through the module API: forward under no_grad and forward + backward, against `TorchSwin`
below -- a plain-torch restatement of the same network written for this tool (one fused qkv Linear, roll + partition,
F.scaled_dot_product_attention with the bias, nn.LayerNorm, F.gelu) -- under bf16 autocast on the same GPU.
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
from vision_toolbox.backbones import SwinTransformer, WindowAttention, window_partition, window_unpartition  # noqa: E402

SHAPES = [(64, 56, 56, 3, 7, 3), (64, 28, 28, 6, 7, 3), (64, 14, 14, 12, 7, 3), (64, 7, 7, 24, 7, 0)]
D = 32
REPEATS, WINDOW_S, WORKING_SET = 7, 0.3, 0.6e9
vp = ctypes.c_void_p
faulthandler.enable()  # a crash inside a library leaves the Python stack on stderr


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


def _windows(t, heads, ws, shift):  # [B, H, W, heads * D] -> contiguous [B * windows, heads, L, D]
    w, _, _ = window_partition(t.roll((-shift, -shift), (1, 2)), ws)
    return w.unflatten(-1, (heads, -1)).transpose(1, 2).contiguous()


def kernels(out_dir: Path):
    lib, dev, bf = N.lib(), torch.device("cuda"), torch.bfloat16
    rows = []
    for B, H, W, heads, ws, shift in SHAPES:
        C, L, scale, n = heads * D, ws * ws, D ** -0.5, (2 * ws - 1) ** 2
        per_set = B * H * W * C * 2 * 8  # qkv (3), o, do, dqkv (3)
        nset = max(2, int(WORKING_SET // per_set) + 1)
        nscr = int(lib.vt_win_attn_bwd_scratch_bytes(B, H, W, heads, ws))
        scratch = torch.zeros(nscr // 4, device=dev)
        attn = WindowAttention(H, C, heads, ws, shift > 0)
        table = torch.randn(heads, n, device=dev)
        dtable = torch.zeros(heads, n, device=dev)
        bias = table[:, attn.relative_pe_index.to(dev)].unsqueeze(0)
        if shift:
            bias = bias + attn.attn_mask.to(dev).unsqueeze(1)
        bias = bias.repeat(B * (H // ws) * (W // ws) // bias.shape[0], 1, 1, 1).to(bf)
        sets = []
        for _ in range(nset):
            s_ = dict(qkv=torch.randn(B, H, W, 3 * C, device=dev).to(bf), o=torch.empty(B, H, W, C, device=dev, dtype=bf),
                      do=torch.randn(B, H, W, C, device=dev).to(bf), dqkv=torch.empty(B, H, W, 3 * C, device=dev, dtype=bf),
                      lse=torch.empty(B, heads, H * W, device=dev))
            s_["t"] = [_windows(s_["qkv"][..., i * C:(i + 1) * C], heads, ws, shift).requires_grad_(True) for i in range(3)]
            s_["tdo"] = _windows(s_["do"], heads, ws, shift)
            s_["to"] = F.scaled_dot_product_attention(*s_["t"], attn_mask=bias)
            sets.append(s_)

        def mk(kind):
            fns = []
            for s_ in sets:
                q, k, v = (vp(s_["qkv"].data_ptr() + i * C * 2) for i in range(3))
                dq, dk, dv = (vp(s_["dqkv"].data_ptr() + i * C * 2) for i in range(3))
                o, do, lse = vp(s_["o"].data_ptr()), vp(s_["do"].data_ptr()), vp(s_["lse"].data_ptr())
                tb, dtb = vp(table.data_ptr()), vp(dtable.data_ptr())
                if kind == "win_attn_fwd":
                    fns.append(lambda s, q=q, k=k, v=v, o=o, lse=lse: N.check(lib.vt_win_attn_fwd(
                        q, 3 * C, k, 3 * C, v, 3 * C, o, C, lse, tb, scale, B, H, W, heads, D, ws, shift, N.VT_BF16, vp(s))))
                elif kind == "win_attn_bwd":
                    fns.append(lambda s, q=q, k=k, v=v, o=o, do=do, lse=lse, dq=dq, dk=dk, dv=dv: N.check(lib.vt_win_attn_bwd(
                        q, 3 * C, k, 3 * C, v, 3 * C, o, C, do, C, lse, tb, dq, 3 * C, dk, 3 * C, dv, 3 * C, dtb,
                        vp(scratch.data_ptr()), nscr, scale, B, H, W, heads, D, ws, shift, N.VT_BF16, vp(s))))
                elif kind == "torch_win_attn_fwd":
                    def f(s, s_=s_):
                        with torch.no_grad():
                            F.scaled_dot_product_attention(*s_["t"], attn_mask=bias)
                    fns.append(f)
                elif kind == "torch_win_attn_bwd":
                    def f(s, s_=s_):
                        torch.autograd.grad(s_["to"], s_["t"], s_["tdo"], retain_graph=True)
                    fns.append(f)
            return fns

        kinds = {"win_attn_fwd": 4.0, "torch_win_attn_fwd": 4.0, "win_attn_bwd": 10.0, "torch_win_attn_bwd": 10.0}
        eager = {k: mk(k) for k in kinds}  # (forward first: the backward reads its o and lse)
        reps = {}
        for k, fns in eager.items():
            _eager_window(fns, 1)
            reps[k] = max(2, -(-20 // nset), int(WINDOW_S * 1e6 / (_eager_window(fns, 2) * nset)) + 1)
        samples = {k: [] for k in kinds}
        for _ in range(REPEATS):
            for k, fns in eager.items():
                samples[k].append(_eager_window(fns, reps[k]))
        row = {"B": B, "H": H, "W": W, "heads": heads, "ws": ws, "shift": shift, "buffer_sets": nset, "eager": {}}
        flop = B * (H // ws) * (W // ws) * heads * L * L * D
        for k in samples:
            med = statistics.median(samples[k])
            row["eager"][k] = {"us_median": med, "us_min": min(samples[k]), "us_max": max(samples[k]),
                               "TFLOPs": kinds[k] * flop / med / 1e6, "launches_per_window": reps[k] * nset}
        for k in ("win_attn_fwd", "win_attn_bwd"):
            row[f"{k}_over_torch"] = row["eager"][k]["us_median"] / row["eager"]["torch_" + k]["us_median"]
        rows.append(row)
        print(json.dumps(row))
        del eager, sets
        torch.cuda.empty_cache()
    _write(out_dir, "swin_kernels.json", {"dtype": "bf16", "window_s": WINDOW_S, "repeats": REPEATS, "shapes": rows})


def _write(out_dir: Path, name: str, doc) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / name).write_text(json.dumps(doc, indent=1))


class TorchBlock(nn.Module):
    def __init__(self, size, d, heads, ws, shift):
        super().__init__()
        self.heads, self.ws, self.shift = heads, ws, shift
        self.ln1, self.ln2 = nn.LayerNorm(d, 1e-5), nn.LayerNorm(d, 1e-5)
        self.qkv, self.proj = nn.Linear(d, 3 * d), nn.Linear(d, d)
        self.fc1, self.fc2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
        ref = WindowAttention(size, d, heads, ws, shift > 0)
        self.table = nn.Parameter(torch.randn(heads, (2 * ws - 1) ** 2) * 0.02)
        self.register_buffer("index", ref.relative_pe_index, False)
        self.register_buffer("mask", ref.attn_mask, False)

    def forward(self, x):
        B, H, W, d = x.shape
        t = self.ln1(x)
        if self.shift:
            t = t.roll((-self.shift, -self.shift), (1, 2))
        t, nH, nW = window_partition(t, self.ws)
        q, k, v = self.qkv(t).view(t.shape[0], t.shape[1], 3, self.heads, d // self.heads).permute(2, 0, 3, 1, 4)
        bias = self.table[:, self.index].unsqueeze(0)
        if self.shift:
            bias = (bias + self.mask.unsqueeze(1)).repeat(B, 1, 1, 1)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.to(q.dtype)).transpose(1, 2).reshape(t.shape)
        o = window_unpartition(self.proj(o), self.ws, nH, nW)
        if self.shift:
            o = o.roll((self.shift, self.shift), (1, 2))
        x = x + o
        return x + self.fc2(F.gelu(self.fc1(self.ln2(x))))


class TorchSwin(nn.Module):
    """the same network in plain torch: patch embedding, patch norm, stages of [merging] + blocks, norm, mean"""

    def __init__(self, img, d, heads, depths, ws):
        super().__init__()
        self.embed, self.embed_norm = nn.Conv2d(3, d, 4, 4), nn.LayerNorm(d, 1e-5)
        size, mods = img // 4, []
        for s, depth in enumerate(depths):
            if s:
                mods.append(nn.ModuleList([nn.LayerNorm(4 * d, 1e-5), nn.Linear(4 * d, 2 * d, bias=False)]))
                size, d, heads = size // 2, 2 * d, 2 * heads
            mods += [TorchBlock(size, d, heads, ws, (ws // 2) if (i % 2 and size > ws) else 0) for i in range(depth)]
        self.mods = nn.ModuleList(mods)
        self.norm = nn.LayerNorm(d, 1e-5)

    def forward(self, x):
        x = self.embed_norm(self.embed(x).permute(0, 2, 3, 1))
        for m in self.mods:
            if isinstance(m, TorchBlock):
                x = m(x)
            else:
                B, H, W, C = x.shape
                x = m[1](m[0](x.view(B, H // 2, 2, W // 2, 2, C).transpose(2, 3).flatten(-3)))
        return self.norm(x).mean((1, 2))


def _model():
    torch.manual_seed(0)
    m = SwinTransformer.from_config("T", 224).cuda().train()
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
    ref = TorchSwin(224, 96, 3, (2, 2, 6, 2), 7).cuda().train()

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
    _write(out_dir, "swin_step.json", {"model": "Swin-T", "batch": 64, "size": 224, "dtype": "bf16", **row})


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
        sys.exit("tools/bench_swin.py needs a GPU: nothing is measured without one")
    {"kernels": lambda: kernels(Path(a.out)), "step": lambda: step(Path(a.out)), "trace": trace}[a.what]()
