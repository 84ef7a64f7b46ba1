"""Generate tests/golden/convnext_train.npz: three AdamW training steps of the UNMODIFIED reference ConvNeXt under the
classifier assembly the reference uses for it, `nn.Sequential(backbone, nn.Linear(C, num_classes))`
(classifier.py:59-64 with include_pool=False), on CPU.  Same shim as tools/gen_golden_convnext.py; runs only where the
reference is present.

    python tools/gen_golden_convnext_train.py

Case: ConvNeXt(24, (1, 2)) + Linear(48, 10), filler.images(3, 64), filler.labels(3, 10), train mode,
F.cross_entropy(label_smoothing=0.1), torch.optim.AdamW over the three weight-decay groups of classifier.py:122-155
(norm 0, bias 0, everything else 0.05), lr 1e-4, 3 steps.  At 64 x 64 the two stages' maps are 16 x 16 and 8 x 8, so every
tap of the 7x7 depthwise filters sees data: at the 2 x 2 maps of the existing 32 x 32 fixtures most taps have an exactly
zero gradient, and Adam's first update is lr * sign(g) -- rounding noise there would become a full-size update.

Weights: oracle/filler.py under the prefix `adamw.`, then +1.0 on every 1-D BACKBONE parameter whose name ends
in `weight` or `gamma` (the rule of tools/gen_golden_convnext.py / tests/convnext_util.fill; the head is left as filled).

Three runs: float64 (the truth), float32, and "bf16" = torch.autocast("cpu", bfloat16) with every module output rounded to
bf16 by forward hooks over float32 master weights (the mode of tools/gen_golden_convnext.py).  Stored: the state_dict keys
and shapes, the recipe strings, the three float64 losses (`loss64`), every parameter's float64 gradient of step 1
(`grad/<key>`), and per stored array the float32 and the bf16 run's relative error against float64
(`floor/f32/...`, `floor/bf16/...`; `loss` = the worst of the three losses).  Arrays and strings only.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
from oracle import filler  # noqa: E402

cnx = gen_golden.ref_import("vision_toolbox.backbones.convnext")
GOLDEN = ROOT / "tests" / "golden"

PRE = "adamw."
D_MODEL, DEPTHS, NCLS, BATCH, SIZE = 24, (1, 2), 10, 3, 64
LR, WD, NORM_WD, BIAS_WD, SMOOTH, STEPS = 1e-4, 0.05, 0.0, 0.0, 0.1, 3
_NORMS = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.LayerNorm, nn.GroupNorm)


def build() -> nn.Module:
    backbone = cnx.ConvNeXt(D_MODEL, DEPTHS)
    model = nn.Sequential(backbone, nn.Linear(2 ** (len(DEPTHS) - 1) * D_MODEL, NCLS))  # (B, 48) -> (B, 10)
    filler.fill_module(model, PRE)
    with torch.no_grad():
        for k, p in backbone.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)
    return model.train()


def groups(model: nn.Module) -> list:
    """the three weight-decay groups of classifier.py:122-155: parameters of normalisation layers; biases of nn.Linear /
    convolutions; everything else (their weights, and whatever a module without children or with children owns itself,
    e.g. a layer scale)"""
    norm, bias, other = [], [], []
    for mod in model.modules():
        own = [p for p in mod.parameters(recurse=False) if p.requires_grad]
        if next(mod.children(), None) is None and isinstance(mod, _NORMS):
            norm += own
        elif next(mod.children(), None) is None and isinstance(mod, (nn.Linear, nn.modules.conv._ConvNd)):
            other += [p for p in own if p is mod.weight]
            bias += [p for p in own if p is mod.bias]
        else:
            other += own
    out = [{"params": norm, "weight_decay": NORM_WD}, {"params": bias, "weight_decay": BIAS_WD},
           {"params": other, "weight_decay": WD}]
    assert sum(len(g["params"]) for g in out) == len(list(model.parameters()))
    return [g for g in out if g["params"]]


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run(mode: str) -> dict:
    model = build()
    x, y = filler.images(BATCH, SIZE), filler.labels(BATCH, NCLS)
    if mode == "f64":
        model, x = model.double(), x.double()
    hooks = [m.register_forward_hook(_to_bf16) for m in model.modules()] if mode == "bf16" else []
    opt = torch.optim.AdamW(groups(model), lr=LR, weight_decay=WD)
    out = {"loss": []}
    for step in range(STEPS):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cpu", torch.bfloat16, enabled=mode == "bf16"):
            logits = model(x)
        loss = F.cross_entropy(logits.float() if mode == "bf16" else logits, y, label_smoothing=SMOOTH)
        loss.backward()
        out["loss"].append(float(loss.detach()))
        if step == 0:
            for k, p in model.named_parameters():
                out["grad/" + k] = p.grad.detach().clone()
        opt.step()
    for h in hooks:
        h.remove()
    out["model"] = model
    return out


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    res = {mode: run(mode) for mode in ("f64", "f32", "bf16")}
    r64 = res["f64"]
    sd = r64["model"].state_dict()
    out = {
        "keys": np.array(list(sd.keys())),
        "shapes": np.array([str(tuple(v.shape)) for v in sd.values()]),
        "recipe": np.array([PRE, f"ConvNeXt({D_MODEL}, {DEPTHS}) + Linear({2 ** (len(DEPTHS) - 1) * D_MODEL}, {NCLS})",
                            f"filler.images({BATCH}, {SIZE})", f"filler.labels({BATCH}, {NCLS})",
                            f"cross_entropy(label_smoothing={SMOOTH})",
                            f"AdamW(lr={LR}, weight_decay={WD}, norm={NORM_WD}, bias={BIAS_WD}), {STEPS} steps, train mode"]),
        "hyper": np.array([LR, WD, NORM_WD, BIAS_WD, SMOOTH, STEPS], dtype=np.float64),
        "loss64": np.array(r64["loss"], dtype=np.float64),
    }
    for k, v in r64.items():
        if k.startswith("grad/"):
            out[k] = v.numpy().copy()
    for tag in ("f32", "bf16"):
        r = res[tag]
        errs = {k: rel(v, r64[k]) for k, v in r.items() if k.startswith("grad/")}
        for k, e in errs.items():
            out[f"floor/{tag}/{k}"] = np.array(e)
        out[f"floor/{tag}/grad_max"] = np.array(max(errs.values()))
        out[f"floor/{tag}/loss"] = np.array(max(abs(a - b) / abs(b) for a, b in zip(r["loss"], r64["loss"])))
        print(tag, "losses", [f"{v:.6f}" for v in r["loss"]], f"loss err {float(out[f'floor/{tag}/loss']):.2e}",
              f"grad_max {float(out[f'floor/{tag}/grad_max']):.2e}")
    print("f64 losses", [f"{v:.6f}" for v in r64["loss"]])
    path = GOLDEN / "convnext_train.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
