"""TEST INFRASTRUCTURE -- the cases, inputs and loss of the SPPBlock fixtures (tests/golden/spp.npz), shared by the generator
(tools/gen_golden_spp.py, which runs the UNMODIFIED reference) and by the tests.

Inputs come from oracle/filler.py recipe keys and are then rounded to bfloat16 (and kept as float32): the bf16 path stores
exactly these values, so a max-pool winner -- and with it the pixel a whole gradient goes to -- is the same element in both
dtypes.  (With inputs that bf16 has to round, two neighbours a rounding step apart become a tie, torch's tie rule picks
another element than the f32 reference did, and no bound on dx means anything.)  Case a applies a ReLU first: exact zeros
and ties are the normal case behind a ConvNormAct."""
from __future__ import annotations

from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch
from torch import nn

from oracle import filler

# name -> ((kernel_size, repeats, pool), input shape, relu on the input)
CASES = {
    "a": ((5, 3, "max"), (2, 16, 13, 11), True),
    "b": ((3, 4, "max"), (1, 8, 7, 9), False),
    "c": ((5, 3, "avg"), (2, 16, 13, 11), False),
    "d": ((9, 2, "max"), (1, 8, 18, 18), False),
}
CHAIN_SHAPE = (2, 8, 12, 12)  # ConvNormAct(8, 16, 1) -> SPPBlock() -> ConvNormAct(48, 16, 1), training mode
CHAIN_UNITS = ((8, 16, 1), (48, 16, 1))
PATH = Path(__file__).parent / "golden" / "spp.npz"


def load() -> dict:
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def _bf16_values(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


def inputs(case: str, dtype=torch.float32, device="cpu") -> torch.Tensor:
    """the case's input map ("chain": the chain's), requiring a gradient"""
    shape, relu = (CHAIN_SHAPE, False) if case == "chain" else CASES[case][1:]
    x = filler.tensor(f"spp_{case}.x", shape)
    if relu:
        x = torch.relu(x)
    return _bf16_values(x).to(device=device, dtype=dtype).requires_grad_(True)


def loss(case: str, y: torch.Tensor) -> torch.Tensor:
    """(y * r).sum() with r from the filler, rounded to bfloat16 values like the inputs"""
    r = _bf16_values(filler.tensor(f"spp_{case}.r", tuple(y.shape))).to(y.device)
    wide = torch.float64 if y.dtype == torch.float64 else torch.float32
    return (y.to(wide) * r.to(wide)).sum()


def build(comp, case: str) -> nn.Module:
    """the case's SPPBlock from `comp` (the reference's vision_toolbox.components or this package's)"""
    k, repeats, pool = CASES[case][0]
    return comp.SPPBlock() if (k, repeats, pool) == (5, 3, "max") else comp.SPPBlock(k, repeats, pool)


def build_chain(comp, container=None) -> nn.Module:
    """cv1 -> spp -> cv2 out of `comp`'s classes; `container(children)` wraps them (default: nn.Sequential)"""
    children = OrderedDict(cv1=comp.ConvNormAct(*CHAIN_UNITS[0]), spp=comp.SPPBlock(), cv2=comp.ConvNormAct(*CHAIN_UNITS[1]))
    return nn.Sequential(children) if container is None else container(children)


def fill(module: nn.Module, case: str = "chain") -> None:
    filler.fill_module(module, f"spp_{case}.")


def gerr(a: torch.Tensor, b: torch.Tensor) -> float:
    """relative L2 error with the clamped denominator of the module tests (tests/test_convnext_gpu.py `_gerr`)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))
