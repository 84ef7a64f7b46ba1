"""Shared by tests/test_deit_cpu.py and tests/test_deit_gpu.py: the fixture cases of tools/gen_golden_deit.py, the weight rule
and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import filler

from mlp_mixer_util import gerr, rel, t  # noqa: F401  (the module tests' metrics)

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (class, constructor args (d_model, depth, n_heads, patch, img), constructor kwargs): the CASES table of
# tools/gen_golden_deit.py
CASES = {
    "a": ("DeiT", (64, 2, 2, 4, 16), {}),
    "b": ("DeiT", (64, 1, 1, 4, 32), {"layer_scale_init": 0.5}),
    "c": ("DeiT3", (64, 2, 1, 4, 16), {}),
}
TRAIN_ARGS, TRAIN_KW = (64, 2, 2, 4, 16), {"mlp_ratio": 2.0}


def load(name: str):
    return np.load(GOLDEN / f"deit_{name}.npz")


def build(name: str):
    from vision_toolbox import backbones

    cls, args, kw = CASES[name]
    return getattr(backbones, cls)(*args, **kw)


def depth(name: str) -> int:
    return CASES[name][1][1]


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma`: the rule of
    tools/gen_golden_deit.py"""
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)


def inputs(g):
    """(prefix, images, projection of y) from the recipe stored in the fixture"""
    pre, kx, kr = [str(s) for s in g["recipe"]]
    x = filler.tensor(kx, tuple(int(v) for v in g["x_shape"]))
    return pre, x, filler.tensor(kr, g["y"].shape)


def zero_keys(g, n_layers: int, prefix: str = "") -> "set[str]":
    """the parameters whose gradient is exactly zero in exact arithmetic, as the generator found them (float64 rms below
    1e-12) -- and the assertion that they are the key projections' biases and nothing else"""
    zero = {str(k) for k in g["zero_grad_keys"]}
    assert zero == {f"{prefix}layers.{i}.mha.1.k_proj.bias" for i in range(n_layers)}, zero
    return zero
