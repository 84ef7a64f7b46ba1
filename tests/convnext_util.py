"""Shared by tests/test_convnext_cpu.py and tests/test_convnext_gpu.py: the fixture cases of
tools/gen_golden_convnext.py, the weight rule and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import filler

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (d_model, depths, constructor kwargs): the CASES table of tools/gen_golden_convnext.py
CASES = {
    "a": (16, (1, 1, 1), {}),
    "b": (24, (1, 2), {}),
    "c": (16, (1, 1), {"layer_scale_init": None}),
}


def load(name: str):
    return np.load(GOLDEN / f"convnext_{name}.npz")


def build(name: str):
    from vision_toolbox.backbones import ConvNeXt

    d_model, depths, kw = CASES[name]
    return ConvNeXt(d_model, depths, **kw)


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma` -- the SAME rule as
    tools/gen_golden_convnext.py: filler gives those 0.1 * N(0, 1), and a LayerNorm scale or a layer scale near 0 would make
    its branch invisible."""
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)


def inputs(g):
    """(images, projection of y, projection of f) from the recipe stored in the fixture"""
    pre, kx, kr, krf = [str(s) for s in g["recipe"]]
    x = filler.tensor(kx, tuple(int(v) for v in g["x_shape"]))
    return pre, x, filler.tensor(kr, g["y"].shape), filler.tensor(krf, g["f"].shape)


def t(a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a))


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
