"""Shared by tests/test_cait_cpu.py and tests/test_cait_gpu.py: the fixture cases of tools/gen_golden_cait.py, the weight
rule and the input recipe."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from vit_util import fill, gerr, inputs, rel, t  # noqa: F401  (the rule of tools/gen_golden_vit.py, the module tests' metrics)

GOLDEN = Path(__file__).resolve().parent / "golden"

# name -> (constructor args (d_model, sa_depth, ca_depth, n_heads, patch, img), constructor kwargs): the CASES table of
# tools/gen_golden_cait.py
CASES = {
    "a": ((96, 1, 1, 2, 4, 16), {"mlp_ratio": 2.0}),
    "b": ((96, 2, 1, 2, 4, 32), {"mlp_ratio": 1.0}),
    "c": ((96, 1, 2, 2, 4, 36), {"mlp_ratio": 1.0, "layer_scale_init": None}),
}
TRAIN_ARGS, TRAIN_KW = (96, 1, 1, 2, 4, 16), {"mlp_ratio": 0.5}  # tools/gen_golden_cait_train.py


def load(name: str):
    return np.load(GOLDEN / f"cait_{name}.npz")


def build(name: str):
    from vision_toolbox.backbones import CaiT

    args, kw = CASES[name]
    return CaiT(*args, **kw)


def zero_keys(g, sa_depth: int, ca_depth: int, prefix: str = "") -> "set[str]":
    """the parameters whose gradient is exactly zero in exact arithmetic, as the generator found them (float64 rms below
    1e-12) -- and the assertion that they are every key projection's bias and every pre-softmax mixing bias, nothing else: a
    constant added to every key, or to a mixed row of scores, shifts the row by a constant, which softmax ignores"""
    zero = {str(k) for k in g["zero_grad_keys"]}
    want = {f"{prefix}sa_layers.{i}.mha.1.k_proj.bias" for i in range(sa_depth)}
    want |= {f"{prefix}sa_layers.{i}.mha.1.talking_head_proj.0.bias" for i in range(sa_depth)}
    want |= {f"{prefix}ca_layers.{i}.mha.1.k_proj.bias" for i in range(ca_depth)}
    assert zero == want, zero ^ want
    return zero
