"""Shared by tests/test_swin_cpu.py and tests/test_swin_gpu.py: the fixture cases of tools/gen_golden_swin.py, the weight rule
and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import filler

from mlp_mixer_util import gerr, rel, t  # noqa: F401  (the module tests' metrics)

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (constructor args (img, d_model, n_heads, depths, window_sizes), constructor kwargs): the CASES table of
# tools/gen_golden_swin.py
CASES = {
    "a": ((48, 32, 1, (2, 2), (4, 3)), {}),
    "b": ((56, 64, 2, (2, 1), (7, 7)), {}),
    "c": ((32, 32, 1, (1, 1), (8, 4)), {"layer_scale_init": 0.5}),
}
TRAIN_ARGS, TRAIN_KW = (48, 32, 1, (2, 2), (4, 3)), {}
_CACHE: dict = {}

SAMPLE_ABOVE, SAMPLES = 2048, 1024


def sample(t):
    """(the rule of tools/gen_golden_swin.py) the elements of a gradient that the fixtures store: all of a tensor of at most SAMPLE_ABOVE elements, else every
    s-th of the flattened tensor with s = (numel // SAMPLES) | 1 -- odd, so the samples walk through every row and column
    of the power-of-two-sided weights -- which keeps a fixture at a few hundred KB; EVERY parameter is still compared"""
    flat = t.reshape(-1)
    return flat if flat.numel() <= SAMPLE_ABOVE else flat[:: (flat.numel() // SAMPLES) | 1]


def load(name: str) -> dict:
    """the arrays of swin_<name>.npz, read once"""
    if name not in _CACHE:
        with np.load(GOLDEN / f"swin_{name}.npz") as f:
            _CACHE[name] = {k: f[k] for k in f.files}
    return _CACHE[name]


def build(name: str):
    from vision_toolbox.backbones import SwinTransformer

    args, kw = CASES[name]
    return SwinTransformer(*args, **kw)


def n_blocks(name: str) -> int:
    return sum(CASES[name][0][3])


def fill_backbone(m: torch.nn.Module) -> None:
    """+1.0 on every 1-D parameter whose name ends in `weight` or `gamma`, every `relative_pe_table` times 10"""
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)
            if k.endswith("relative_pe_table"):
                p.mul_(10.0)


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then the rule of tools/gen_golden_swin.py"""
    filler.fill_module(m, prefix)
    fill_backbone(m)


def inputs(g):
    """(prefix, images, projection of y) from the recipe stored in the fixture"""
    pre, kx, kr = [str(s) for s in g["recipe"]]
    x = filler.tensor(kx, tuple(int(v) for v in g["x_shape"]))
    return pre, x, filler.tensor(kr, g["y"].shape)


def block_names(m) -> "list[str]":
    from vision_toolbox.backbones import SwinBlock

    return [k for k, mod in m.named_modules() if isinstance(mod, SwinBlock)]


def zero_keys(g, m) -> "set[str]":
    """the parameters whose gradient is exactly zero in exact arithmetic, as the generator found them (float64 rms below
    1e-12) -- and the assertion that they are the key projections' biases and nothing else: a constant added to every key
    shifts each row of scores by a constant, which softmax ignores"""
    zero = {str(k) for k in g["zero_grad_keys"]}
    assert zero == {f"{b}.mha.1.k_proj.bias" for b in block_names(m)}, zero
    return zero
