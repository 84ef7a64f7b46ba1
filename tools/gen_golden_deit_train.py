"""Generate tests/golden/deit_train.npz: three AdamW training steps of the UNMODIFIED reference DeiT under the classifier
assembly `nn.Sequential(backbone, nn.Linear(d_model, num_classes))` (classifier.py:59-64 with include_pool=False), on CPU, in
the manner of tools/gen_golden_vit_train.py.  Runs only where the reference is present.

    python tools/gen_golden_deit_train.py

Case: DeiT(64, 2, 2, 4, 16, mlp_ratio=2.0) + Linear(64, 10) (case a of tools/gen_golden_deit.py with a narrower MLP, so
that the float64 gradients stay under the size limit of a committed file), filler.images(3, 16), filler.labels(3, 10), train mode,
F.cross_entropy(label_smoothing=0.1), torch.optim.AdamW over the three weight-decay groups of classifier.py:122-155 (norm 0,
bias 0, everything else 0.05 -- `pe`, `cls_token` and `dist_token` among them), lr 1e-4, 3 steps.

The reference's torch.cat of the class and distillation tokens raises at batch > 1, so each step runs the images ONE AT A
TIME and accumulates the gradients of loss_i / B before `AdamW.step()`: the batch-mean loss, as a batched run would compute it.

Weights: oracle/filler.py under the prefix `deit_adamw.`, then +1.0 on every 1-D BACKBONE parameter whose name ends in
`weight` or `gamma`; the head is left as filled.

Three runs: float64 (the truth), float32, and "bf16" = torch.autocast("cpu", bfloat16) with every module output rounded to
bf16 by forward hooks.  Stored: keys, shapes, recipe strings, the three float64 losses (`loss64`), every parameter's float64
gradient of step 1 (`grad/<key>`), `zero_grad_keys` (float64 rms below 1e-12: asserted to be exactly the `k_proj.bias`
keys, see tools/gen_golden_vit.py) and per stored array the float32 and bf16 runs' error against
float64 in the tests' clamped metric (`floor/...`; `loss` = the worst relative error of the three losses; `grad_max` leaves
the zero keys out).  Every stored `floor/bf16/*` of a live key is asserted to be below 0.0625: the cap of the tests' bf16
gradient bound min(4 x floor, 0.25) never binds.
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

deit = gen_golden.ref_import("vision_toolbox.backbones.deit")
GOLDEN = ROOT / "tests" / "golden"

PRE = "deit_adamw."
ARGS, KW, NCLS, BATCH = (64, 2, 2, 4, 16), {"mlp_ratio": 2.0}, 10, 3
FLOOR_CAP = 0.0625
LR, WD, NORM_WD, BIAS_WD, SMOOTH, STEPS = 1e-4, 0.05, 0.0, 0.0, 0.1, 3
_NORMS = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.LayerNorm, nn.GroupNorm)


def build() -> nn.Module:
    backbone = deit.DeiT(*ARGS, **KW)
    model = nn.Sequential(backbone, nn.Linear(ARGS[0], NCLS))
    filler.fill_module(model, PRE)
    with torch.no_grad():
        for k, p in backbone.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)
    return model.train()


def groups(model: nn.Module) -> list:
    """the three weight-decay groups of classifier.py:122-155"""
    norm, bias, other = [], [], []
    for mod in model.modules():
        own = [p for p in mod.parameters(recurse=False) if p.requires_grad]
        leaf = next(mod.children(), None) is None
        if leaf and isinstance(mod, _NORMS):
            norm += own
        elif leaf and isinstance(mod, (nn.Linear, nn.modules.conv._ConvNd)):
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
    x, y = filler.images(BATCH, ARGS[4]), filler.labels(BATCH, NCLS)
    if mode == "f64":
        model, x = model.double(), x.double()
    hooks = [m.register_forward_hook(_to_bf16) for m in model.modules()] if mode == "bf16" else []
    opt = torch.optim.AdamW(groups(model), lr=LR, weight_decay=WD)
    out = {"loss": []}
    for step in range(STEPS):
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for b in range(BATCH):  # one image at a time: the gradients of loss_b / B accumulate
            with torch.autocast("cpu", torch.bfloat16, enabled=mode == "bf16"):
                logits = model(x[b:b + 1])
            loss = F.cross_entropy(logits.float() if mode == "bf16" else logits, y[b:b + 1], label_smoothing=SMOOTH) / BATCH
            loss.backward()
            total += float(loss.detach())
        out["loss"].append(total)
        if step == 0:
            for k, p in model.named_parameters():
                out["grad/" + k] = p.grad.detach().clone()
        opt.step()
    for h in hooks:
        h.remove()
    out["model"] = model
    return out


def gerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))


def main():
    res = {mode: run(mode) for mode in ("f64", "f32", "bf16")}
    r64 = res["f64"]
    sd = r64["model"].state_dict()
    zero = sorted(k[5:] for k, v in r64.items()
                  if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
    assert zero == sorted(f"0.layers.{i}.mha.1.k_proj.bias" for i in range(ARGS[1])), zero
    out = {
        "keys": np.array(list(sd.keys())),
        "shapes": np.array([str(tuple(v.shape)) for v in sd.values()]),
        "recipe": np.array([PRE, f"DeiT{ARGS} {KW} + Linear({ARGS[0]}, {NCLS})",
                            f"filler.images({BATCH}, {ARGS[4]})", f"filler.labels({BATCH}, {NCLS})",
                            f"cross_entropy(label_smoothing={SMOOTH})",
                            f"AdamW(lr={LR}, weight_decay={WD}, norm={NORM_WD}, bias={BIAS_WD}), {STEPS} steps, train mode"]),
        "hyper": np.array([LR, WD, NORM_WD, BIAS_WD, SMOOTH, STEPS], dtype=np.float64),
        "loss64": np.array(r64["loss"], dtype=np.float64),
        "zero_grad_keys": np.array(zero),
    }
    for k, v in r64.items():
        if k.startswith("grad/"):
            out[k] = v.numpy().copy()
    for tag in ("f32", "bf16"):
        r = res[tag]
        errs = {k: gerr(v, r64[k]) for k, v in r.items() if k.startswith("grad/")}
        for k, e in errs.items():
            out[f"floor/{tag}/{k}"] = np.array(e)
        out[f"floor/{tag}/grad_max"] = np.array(max(e for k, e in errs.items() if k[5:] not in zero))
        out[f"floor/{tag}/loss"] = np.array(max(abs(a - b) / abs(b) for a, b in zip(r["loss"], r64["loss"])))
        if tag == "bf16":
            over = {k: e for k, e in errs.items() if k[5:] not in zero and not e < FLOOR_CAP}
            assert not over and float(out["floor/bf16/loss"]) < FLOOR_CAP, f"bf16 floors at or above {FLOOR_CAP}: {over}"
        print(tag, "losses", [f"{v:.6f}" for v in r["loss"]], f"loss err {float(out[f'floor/{tag}/loss']):.2e}",
              f"grad_max {float(out[f'floor/{tag}/grad_max']):.2e}")
    print("f64 losses", [f"{v:.6f}" for v in r64["loss"]], "zero keys", zero)
    path = GOLDEN / "deit_train.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
