"""Generate tests/golden/spp.npz by running the UNMODIFIED reference SPPBlock (vision_toolbox/components.py:139-152) on CPU,
alone (cases a-d of tests/spp_util.py) and between two of the reference's ConvNormAct units in training mode ("chain").
Same shim as tools/gen_golden.py; run in the build container.

    python tools/gen_golden_spp.py

Inputs and the loss weights are filler recipes (tests/spp_util.py: `inputs`, `loss`, rounded to bfloat16 values), so only the
outputs are stored: per case `y` and the input gradient `dx` of (y * r).sum(); for the chain also every parameter gradient
and the BatchNorm buffers after the step.

Floors (`<case>/floor/f32/...`, `<case>/floor/bf16/...`): the recipe of tools/gen_golden_vit.py -- the reference in float32,
and under torch.autocast("cpu", bfloat16) with every module output rounded to bfloat16 by forward hooks, each against the
reference in float64, in the tests' clamped metric (spp_util.gerr).

`chain/zero_grad_keys`: the parameters whose float64 gradient has an rms below 1e-12 (the rule of tools/gen_golden_vit.py).
That is `cv1.norm.bias`: cv2's training-mode BatchNorm makes the gradient of its input sum to zero over the pixels of every
channel, max pooling only moves those terms to their winners, and the winners behind a ReLU are positive, so the sum that
forms d(cv1.norm.bias) is zero in exact arithmetic.  Its floor entry is the largest magnitude the reference leaves there."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
import spp_util as SU  # noqa: E402  (the cases, the inputs and the loss: shared with the tests)

comp = gen_golden.ref_import("vision_toolbox.components")


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run_once(m, case, dtype=torch.float32, autocast=False):
    x = SU.inputs(case, dtype)
    m.zero_grad()
    hooks = [mod.register_forward_hook(_to_bf16) for mod in m.modules()] if autocast else []
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        y = m(x)
    SU.loss(case, y).backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "dx": x.grad.detach()}
    for k, p in m.named_parameters():
        out["grad/" + k] = p.grad.detach().clone()
    return out


def run_case(case, make):
    """float32 results plus the f32 / bf16 floors against float64; `make()` builds a freshly filled module"""
    res32 = run_once(make(), case)
    state = None
    if case == "chain":
        m = make()
        run_once(m, case)
        state = {k: v.detach().clone() for k, v in m.state_dict().items()
                 if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    res16 = run_once(make(), case, autocast=True)
    res64 = run_once(make().double(), case, torch.float64)
    out = {f"{case}/{k}": v.numpy().copy() for k, v in res32.items()}
    for k, v in (state or {}).items():
        out[f"{case}/state/{k}"] = v.numpy().copy()
    zero = sorted(k[5:] for k, v in res64.items() if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
    out[f"{case}/zero_grad_keys"] = np.array(zero, dtype=str)
    for tag, res in (("f32", res32), ("bf16", res16)):
        errs = {k: SU.gerr(v, res64[k]) for k, v in res.items()}
        for k, e in errs.items():
            # (a zero gradient has no relative error: its floor is the largest magnitude the reference itself leaves there)
            out[f"{case}/floor/{tag}/{k}"] = np.array(float(res[k].float().abs().max()) if k[5:] in zero else e)
        print(case, tag, {k: f"{e:.2e}" for k, e in errs.items()})
    return out


def main():
    out = {}
    for case in SU.CASES:
        out.update(run_case(case, lambda case=case: SU.build(comp, case).train()))

    def chain():
        m = SU.build_chain(comp)
        SU.fill(m)
        return m.train()

    out["chain/keys"] = np.array(list(chain().state_dict().keys()))
    out.update(run_case("chain", chain))
    np.savez_compressed(SU.PATH, **out)
    print(f"wrote {SU.PATH}: {len(out)} arrays, {SU.PATH.stat().st_size} bytes")
    assert SU.PATH.stat().st_size < 1_000_000


if __name__ == "__main__":
    main()
