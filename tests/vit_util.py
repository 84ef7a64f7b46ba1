"""Shared by tests/test_vit_cpu.py and tests/test_vit_gpu.py: the fixture cases of tools/gen_golden_vit.py, the weight rule
and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import filler

from mlp_mixer_util import gerr, rel, t  # noqa: F401  (the module tests' metrics)

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (constructor args (d_model, depth, n_heads, patch, img), constructor kwargs): the CASES table of
# tools/gen_golden_vit.py
CASES = {
    "a": ((64, 2, 2, 4, 16), {}),
    "b": ((64, 2, 1, 4, 32), {"cls_token": False, "pool_type": "gap"}),
    "c": ((64, 1, 1, 4, 32), {"layer_scale_init": 0.5}),
}
TRAIN_ARGS, TRAIN_KW = (64, 2, 2, 4, 16), {"cls_token": False, "pool_type": "gap"}


def load(name: str):
    return np.load(GOLDEN / f"vit_{name}.npz")


def build(name: str):
    from vision_toolbox.backbones import ViT

    args, kw = CASES[name]
    return ViT(*args, **kw)


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma`: the rule of
    tools/gen_golden_vit.py"""
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


def zero_keys(g, depth: int, prefix: str = "") -> "set[str]":
    """the parameters whose gradient is exactly zero in exact arithmetic, as the generator found them (float64 rms below
    1e-12) -- and the assertion that they are the key projections' biases and nothing else: a constant added to every key
    shifts each row of scores by a constant, which softmax ignores"""
    zero = {str(k) for k in g["zero_grad_keys"]}
    assert zero == {f"{prefix}layers.{i}.mha.1.k_proj.bias" for i in range(depth)}, zero
    return zero
