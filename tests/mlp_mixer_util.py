"""Shared by tests/test_mlp_mixer_cpu.py and tests/test_mlp_mixer_gpu.py: the fixture cases of
tools/gen_golden_mlp_mixer.py, the weight rule and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import filler

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (constructor args, constructor kwargs): the CASES table of tools/gen_golden_mlp_mixer.py
CASES = {
    "a": ((2, 32, 4, 20), {}),
    "b": ((2, 48, 8, 56), {}),
    "c": ((1, 24, 4, 24), {"mlp_ratio": (1.0, 2.0)}),
}


def load(name: str):
    return np.load(GOLDEN / f"mlp_mixer_{name}.npz")


def build(name: str):
    from vision_toolbox.backbones import MLPMixer

    args, kw = CASES[name]
    return MLPMixer(*args, **kw)


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma`: the rule of
    tools/gen_golden_mlp_mixer.py"""
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
    1e-12) -- and the assertion that they are the token-mixing output biases and nothing else"""
    zero = {str(k) for k in g["zero_grad_keys"]}
    assert zero == {f"{prefix}layers.{i}.token_mixing.linear2.bias" for i in range(n_layers)}, zero
    assert len(zero) <= n_layers
    return zero


def t(a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a))


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gerr(got: torch.Tensor, ref: torch.Tensor) -> float:
    """the module tests' gradient metric (`_gerr` of tests/test_convnext_gpu.py)"""
    return ((got.float().cpu() - ref).norm() / ref.norm().clamp_min(1e-3 * (ref.numel() ** 0.5))).item()
