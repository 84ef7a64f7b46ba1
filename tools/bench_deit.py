"""DeiT numbers on the GPU (fails without one).

    python tools/bench_deit.py kernels [--out DIR]   # the prefix-token kernels against the launches they replace -> deit_kernels.json
    python tools/bench_deit.py model [--out DIR]     # DeiT-S/16, DeiT3-S/16 and ViT-S/16 in one process          -> deit_model.json

kernels, bf16, token maps (B, L, C) = (64, 198, 384) and (64, 198, 768), P = 2:
    tokens  vt_prefix_tokens_fwd / _bwd  against  vt_vit_tokens_* (one prefix row) + vt_token_prepend_* (the other): the
            composition copies the whole token map a second time, forward and backward
    pool    vt_prefix_pool_fwd / _bwd    against  2 x vt_token_select + vt_layernorm + vt_global_avgpool, and in reverse (the
            first vt_token_select_bwd zero-fills the map gradient)
The outputs of the two forms are compared before anything is timed (equal, or within bf16 rounding where the composition
rounds twice).  The channel-sums buffers are not cleared between repetitions (in a program one memset clears all of them).
model: from_config("S_16", 224) at batch 64, bf16, forward under no_grad and forward + backward through the module API, for
ViT, ViT with layer_scale_init=1e-6, DeiT and DeiT3 of the same tree in the same process.  DeiT3-S emits the launch list of
the ViT with LayerScale; DeiT-S differs by one token and the pooled head.

Timing: device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows of >= 4 repetitions each, the variants of a
group ALTERNATING window by window; median, min and max recorded.  Nothing is compared against a threshold."""
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

SHAPES = [(64, 198, 384), (64, 198, 768)]
P, EPS, WINDOW_S, WINDOWS = 2, 1e-6, 0.3, 5
vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731


def _ptrs(tensors):
    arr = (ctypes.c_void_p * 4)()
    for k, t in enumerate(tensors):
        arr[k] = t.data_ptr()
    return arr


def _timed_group(fns: dict, warmup=3) -> dict:
    """every variant warmed up, then WINDOWS rounds in which the variants take turns"""
    reps = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(4, int(WINDOW_S / max(time.perf_counter() - t0, 1e-5)) + 1)
    out = {name: [] for name in fns}
    for _ in range(WINDOWS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps[name])
    return {name: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "repetitions": WINDOWS * reps[name]}
            for name, v in out.items()}


def kernels(out_dir: Path):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    rows = []
    for B, L, C in SHAPES:
        T = L - P
        torch.manual_seed(0)
        embed = torch.randn(B, T, C, device=dev).to(bf)
        pe, cls, dist = torch.randn(T, C, device=dev), torch.randn(C, device=dev), torch.randn(C, device=dev)
        out, out2, mid = (torch.empty(B, n, C, device=dev, dtype=bf) for n in (L, L, L - 1))
        dout = torch.randn(B, L, C, device=dev).to(bf)
        dembed, dembed2, dmid = (torch.empty(B, n, C, device=dev, dtype=bf) for n in (T, T, L - 1))
        dpe, dcls, ddist = torch.zeros(T, C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        prefix, dprefix = _ptrs([cls, dist]), _ptrs([dcls, ddist])

        def tokens_fwd():
            N.check(lib.vt_prefix_tokens_fwd(vp(embed), C, vp(pe), prefix, P, vp(out), C, B, T, C, dt, s()))

        def tokens_fwd_composed():  # [dist | patches + pe], then cls in front
            N.check(lib.vt_vit_tokens_fwd(vp(embed), C, vp(pe), vp(dist), vp(mid), C, B, T, C, dt, s()))
            N.check(lib.vt_token_prepend_fwd(vp(mid), C, None, 0, vp(cls), vp(out2), C, B, T + 1, C, dt, s()))

        def tokens_bwd():
            N.check(lib.vt_prefix_tokens_bwd(vp(dout), C, vp(dembed), C, vp(dpe), dprefix, P, B, T, C, dt, s()))

        def tokens_bwd_composed():
            N.check(lib.vt_token_prepend_bwd(vp(dout), C, vp(dmid), C, 0, None, 0, vp(dcls), B, T + 1, C, dt, s()))
            N.check(lib.vt_vit_tokens_bwd(vp(dmid), C, vp(dembed2), C, vp(dpe), vp(ddist), 1, B, T, C, dt, s()))

        x = (torch.randn(B, L, C, device=dev) * 1.5 + 0.3).to(bf)
        gamma, beta = 1.0 + 0.5 * torch.randn(C, device=dev), 0.2 * torch.randn(C, device=dev)
        y, y2 = torch.empty(B, C, device=dev, dtype=bf), torch.empty(B, C, device=dev, dtype=bf)
        sel, nsel, dnsel, dsel = (torch.empty(B, P, C, device=dev, dtype=bf) for _ in range(4))
        dy = torch.randn(B, C, device=dev).to(bf)
        dx, dx2 = torch.empty(B, L, C, device=dev, dtype=bf), torch.empty(B, L, C, device=dev, dtype=bf)
        sums2 = torch.zeros(N.VT_STAT_REPLICAS, 2, C, 2, dtype=torch.int64, device=dev)
        sums3 = torch.zeros(N.VT_STAT_REPLICAS, 3, C, 2, dtype=torch.int64, device=dev)

        def pool_fwd():
            N.check(lib.vt_prefix_pool_fwd(vp(x), C, vp(gamma), vp(beta), vp(y), C, B, L, P, C, EPS, dt, s()))

        def pool_fwd_composed():
            for p in range(P):
                N.check(lib.vt_token_select_fwd(vp(x), C, vp(sel[:, p]), P * C, B, L, p, C, dt, s()))
            N.check(lib.vt_layernorm_fwd(vp(sel), C, None, vp(gamma), vp(beta), vp(nsel), C, B * P, C, EPS, dt, s()))
            N.check(lib.vt_global_avgpool_fwd(vp(nsel), C, vp(y2), C, B, P, C, dt, s()))

        def pool_bwd():
            N.check(lib.vt_prefix_pool_bwd(vp(dy), C, vp(x), C, vp(gamma), vp(dx), C, 0, vp(sums2), B, L, P, C, EPS, dt, s()))

        def pool_bwd_composed():
            N.check(lib.vt_global_avgpool_bwd(vp(dy), C, vp(dnsel), C, B, P, C, 0, dt, s()))
            N.check(lib.vt_layernorm_bwd(vp(dnsel), C, vp(sel), C, None, vp(gamma), vp(dsel), C, None, 0, vp(sums3), B * P, C, EPS,
                                         dt, s()))
            for p in range(P):  # (the first one zero-fills the other rows)
                N.check(lib.vt_token_select_bwd(vp(dsel[:, p]), P * C, vp(dx2), C, int(p > 0), B, L, p, C, dt, s()))

        # the two forms agree before they are timed
        for fn in (tokens_fwd, tokens_fwd_composed, tokens_bwd, pool_fwd, pool_fwd_composed, pool_bwd, pool_bwd_composed):
            fn()
        torch.cuda.synchronize()
        new_dpe = dpe.clone()
        dpe.zero_(), dcls.zero_(), ddist.zero_()
        tokens_bwd_composed()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
        agree = {"tokens_fwd_equal": bool(torch.equal(out, out2)), "tokens_bwd_dembed_equal": bool(torch.equal(dembed, dembed2)),
                 "tokens_bwd_dpe_equal": bool(torch.equal(new_dpe, dpe)), "pool_fwd_rel": rel(y, y2),
                 "pool_bwd_rel": rel(dx, dx2)}
        agree.update(tokens_fwd_rel=rel(out, out2), tokens_bwd_dembed_rel=rel(dembed, dembed2), tokens_bwd_dpe_rel=rel(new_dpe, dpe))
        assert max(agree["tokens_fwd_rel"], agree["tokens_bwd_dembed_rel"], agree["tokens_bwd_dpe_rel"]) < 1e-5, agree
        assert agree["pool_fwd_rel"] < 1e-2 and agree["pool_bwd_rel"] < 1e-2, agree  # (the composition rounds twice)
        esize = 2
        row = {"B": B, "L": L, "C": C, "P": P, "dtype": "bf16", "agreement": agree,
               # the bytes each op has to move: read embed + write out; read dout + write dembed; the prefix rows and (for
               # the backward) the whole map gradient
               "min_bytes": {"tokens_fwd": (B * T * C + B * L * C) * esize + T * C * 4,
                             "tokens_bwd": (B * L * C + B * T * C) * esize + 2 * T * C * 4,
                             "pool_fwd": (B * P * C + B * C) * esize,
                             "pool_bwd": (B * P * C + B * C + B * L * C) * esize}}
        groups = ({"tokens_fwd": tokens_fwd, "tokens_fwd_composed": tokens_fwd_composed},
                  {"tokens_bwd": tokens_bwd, "tokens_bwd_composed": tokens_bwd_composed},
                  {"pool_fwd": pool_fwd, "pool_fwd_composed": pool_fwd_composed},
                  {"pool_bwd": pool_bwd, "pool_bwd_composed": pool_bwd_composed})
        for fns in groups:
            row.update(_timed_group(fns))
        for name in ("tokens_fwd", "tokens_bwd", "pool_fwd", "pool_bwd"):
            row[name + "_over_composed"] = row[name]["ms_median"] / row[name + "_composed"]["ms_median"]
            row[name + "_GBps"] = row["min_bytes"][name] / (row[name]["ms_median"] * 1e-3) / 1e9
        print(json.dumps(row))
        rows.append(row)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "deit_kernels.json").write_text(json.dumps({"window_s": WINDOW_S, "windows": WINDOWS, "shapes": rows}, indent=1))


def model(out_dir: Path):
    from vision_toolbox.backbones import DeiT, DeiT3, ViT

    torch.manual_seed(0)
    d_model, depth, heads = ViT._VARIANTS["S"]
    models = {"ViT-S/16": ViT.from_config("S_16", 224), "ViT-S/16 layer_scale": ViT(d_model, depth, heads, 16, 224, layer_scale_init=1e-6),
              "DeiT-S/16": DeiT.from_config("S_16", 224), "DeiT3-S/16": DeiT3.from_config("S_16", 224)}
    x = torch.randn(64, 3, 224, 224, device="cuda")
    fwd, fwd_bwd = {}, {}
    for name, m in models.items():
        m = m.cuda().train()
        m.compute_dtype = torch.bfloat16

        def f(m=m):
            with torch.no_grad():
                m(x)

        def fb(m=m):
            m(x).float().square().mean().backward()

        fwd[name], fwd_bwd[name] = f, fb
    res = {"batch": 64, "size": 224, "dtype": "bf16", "window_s": WINDOW_S, "windows": WINDOWS,
           "forward": _timed_group(fwd), "forward_backward": _timed_group(fwd_bwd)}
    for what in ("forward", "forward_backward"):
        for name, r in res[what].items():
            r["images_per_s"] = 64 / r["ms_median"] * 1e3
            print(what, name, json.dumps(r))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "deit_model.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model"])
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_deit.py needs a GPU: nothing is measured without one")
    {"kernels": kernels, "model": model}[a.what](Path(a.out))
