"""Generate tests/golden/bifpn_<case>.npz and bifpn_<case>_eval.npz (the eval-mode arrays) by running the UNMODIFIED reference BiFPN
(vision_toolbox/necks.py:125-215) on CPU with `block=ConvNormAct` -- its default SeparableConv2d cannot be constructed
(components.py:62-72 hands `padding=` / `act_fn=` to ConvNormAct), the ConvNormAct block runs forward and backward in train
and eval mode.  Same shim as tools/gen_golden.py; run in the build container.

    python tools/gen_golden_bifpn.py

Weights: oracle/filler.py, then every fusion-weight vector by the one rule of tests/bifpn_util.py (set_fusion_weights), which
the tests apply to the shipped modules as well."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import bifpn_util as BU  # noqa: E402  (the cases, the weight rule, the inputs and the loss: shared with the tests)
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)

necks = gen_golden.ref_import("vision_toolbox.necks")
comp = gen_golden.ref_import("vision_toolbox.components")
GOLDEN = ROOT / "tests" / "golden"


def np_(t):
    return t.detach().cpu().numpy().copy()


def main():
    for case, (ins, outc, sizes, layers) in BU.CASES.items():
        name, out = f"bifpn_{case}", {}
        torch.manual_seed(0)
        m = necks.BiFPN(list(ins), outc, num_layers=layers, block=comp.ConvNormAct)
        out[f"{name}/keys"] = np.array(list(m.state_dict().keys()))
        out[f"{name}/shapes"] = np.array([str(tuple(v.shape)) for v in m.state_dict().values()])
        for mode in ("train", "eval"):
            BU.fill(m, f"{name}.", case)
            out[f"{name}/min_weight_sum"] = np.array(BU.set_fusion_weights(m, f"{name}.", case))
            m.train(mode == "train")
            xs = BU.inputs(case)
            ys = m(list(xs))
            m.zero_grad()
            BU.loss(case, ys).backward()
            for i, y in enumerate(ys):
                out[f"{name}/{mode}/y{i}"] = np_(y)
            for i, x in enumerate(xs):
                out[f"{name}/{mode}/dx{i}"] = np_(x.grad)
            for k, p in m.named_parameters():
                out[f"{name}/{mode}/grad/{k}"] = np_(p.grad)
            if mode == "train":
                for k, v in m.state_dict().items():
                    if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                        out[f"{name}/train/state/{k}"] = np_(v)
        # two files per case: case b's arrays (random floats do not compress) come to 1.2 MB in one file, over the size limit
        # of a committed file -- the eval-mode arrays go to bifpn_<case>_eval.npz, everything else to bifpn_<case>.npz
        ev = {k: v for k, v in out.items() if k.startswith(f"{name}/eval/")}
        for path, arrays in ((GOLDEN / f"{name}.npz", {k: v for k, v in out.items() if k not in ev}), (GOLDEN / f"{name}_eval.npz", ev)):
            np.savez_compressed(path, **arrays)
            print(f"wrote {path}: {len(arrays)} arrays, {path.stat().st_size} bytes")
            assert path.stat().st_size < 1_000_000
        print(f"{name}: min sum relu(w) {float(out[f'{name}/min_weight_sum']):.3f}")


if __name__ == "__main__":
    main()
