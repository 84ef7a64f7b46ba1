"""Generate tests/golden/convnext_<case>.npz by running the UNMODIFIED reference ConvNeXt
(vision_toolbox/backbones/convnext.py) on CPU.  Same shim as tools/gen_golden.py; run in the build container.

    python tools/gen_golden_convnext.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the head output `y`
(B, C), the last stage's map `f` (B, H, W, C), the image gradient `dx` and every parameter gradient of the loss
(y * r).sum() + (f * r_f).sum() -- NOT y.sum(): the sum over a LayerNorm's output has zero gradient.  Train and eval mode
compute the same function (no BatchNorm, drop rate 0): one mode is stored.

Weights: oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma` (filler gives those
0.1 * N(0, 1): a LayerNorm scale or a layer scale near 0 would make its branch invisible).  tests/test_convnext_*.py apply
the same rule (convnext_util.fill).

Floors (`floor/f32/...`, `floor/bf16/...`): the relative error (norm of the difference over the norm) of the reference in
float32, and of the reference under torch.autocast("cpu", torch.bfloat16) with every module output rounded to bfloat16
(forward hooks), each against the reference in float64 on the same weights and inputs -- per stored array, and `grad_max` =
the maximum over the parameter gradients.  The hooks make the bf16 floor honest for a path that STORES every activation in
bf16: plain autocast keeps LayerNorm outputs and the returned tensors in float32, so e.g. the gradient of the head norm's
bias (the column sums of the projection r, which never touch the network) would have a floor of 1e-7, while any path whose
output tensor is bf16 receives that projection rounded to bf16 (2e-3).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
from oracle import filler  # noqa: E402

cnx = gen_golden.ref_import("vision_toolbox.backbones.convnext")
GOLDEN = ROOT / "tests" / "golden"

CASES = {  # name -> (d_model, depths, constructor kwargs, batch, H, W)
    "a": (16, (1, 1, 1), {}, 2, 32, 32),
    "b": (24, (1, 2), {}, 3, 38, 30),  # 3 chunks per row; the stem and the downsample drop rows / columns
    "c": (16, (1, 1), {"layer_scale_init": None}, 2, 16, 16),
}


def fill(m: torch.nn.Module, prefix: str) -> None:
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run(m, x, r, rf, autocast=False):
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    hooks = [mod.register_forward_hook(_to_bf16) for mod in m.modules()] if autocast else []
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        y = m(x)
        f = m.get_feature_maps(x)[-1]
    loss = (y.to(r.dtype) * r).sum() + (f.to(rf.dtype) * rf).sum()
    loss.backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "f": f.detach(), "dx": x.grad.detach()}
    for k, p in m.named_parameters():
        out["grad/" + k] = p.grad.detach().clone()
    return out


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    for name, (d_model, depths, kw, B, H, W) in CASES.items():
        pre = f"convnext_{name}."
        m = cnx.ConvNeXt(d_model, depths, **kw)
        fill(m, pre)
        m.eval()
        x = filler.tensor(pre + "x", (B, 3, H, W))
        with torch.no_grad():
            y0, f0 = m(x), m.get_feature_maps(x)[-1]
        r, rf = filler.tensor(pre + "r", tuple(y0.shape)), filler.tensor(pre + "rf", tuple(f0.shape))
        res32 = run(m, x, r, rf)
        res16 = run(m, x, r, rf, autocast=True)
        res64 = run(m.double(), x.double(), r.double(), rf.double())
        m.float()
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r", pre + "rf"]),
            "x_shape": np.array([B, 3, H, W]),
        }
        for k, v in res32.items():
            out[k] = v.numpy().copy()
        for tag, res in (("f32", res32), ("bf16", res16)):
            errs = {k: rel(v, res64[k]) for k, v in res.items()}
            for k, e in errs.items():
                out[f"floor/{tag}/{k}"] = np.array(e)
            out[f"floor/{tag}/grad_max"] = np.array(max(e for k, e in errs.items() if k.startswith("grad/")))
            print(name, tag, {k: f"{errs[k]:.2e}" for k in ("y", "f", "dx")}, f"grad_max {float(out[f'floor/{tag}/grad_max']):.2e}")
        out["floor/min_grad_norm64"] = np.array(min(float(v.norm()) for k, v in res64.items() if k.startswith("grad/")))
        path = GOLDEN / f"convnext_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
