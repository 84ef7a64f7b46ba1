"""Shared by tests/test_patchconvnet_cpu.py and tests/test_patchconvnet_gpu.py: the fixture cases of
tools/gen_golden_patchconvnet.py, the weight rule, the input recipe and the rule by which large arrays are sampled."""
from __future__ import annotations

import zlib
from pathlib import Path

import numpy as np
import torch

from oracle import filler

from mlp_mixer_util import gerr, rel, t  # noqa: F401  (the module tests' metrics)

GOLDEN = Path(__file__).resolve().parent / "golden"
SAMPLE = 4096

# name -> (constructor args, constructor kwargs, modes): the CASES table of tools/gen_golden_patchconvnet.py
CASES = {
    "a": ((64, 1), {"mlp_ratio": 2, "drop_path": 0.0, "norm_type": "bn"}, ("train", "eval")),
    "b": ((64, 2), {"mlp_ratio": 1, "drop_path": 0.3, "norm_type": "ln"}, ("eval",)),
    "c": ((128, 1), {"norm_type": "bn", "drop_path": 0.0}, ("train", "eval")),
}
CASE_MODES = [(n, mode) for n, (_, _, modes) in CASES.items() for mode in modes]
TRAIN_ARGS, TRAIN_KW = (64, 1), {"mlp_ratio": 1, "drop_path": 0.0, "norm_type": "bn"}  # tools/gen_golden_patchconvnet_train.py
TRAIN_BATCH, TRAIN_SIZE, TRAIN_CLASSES = 3, 32, 10


def load(name: str):
    return np.load(GOLDEN / f"patchconvnet_{name}.npz")


def build(name: str):
    from vision_toolbox.backbones import PatchConvNet

    args, kw, _ = CASES[name]
    return PatchConvNet(*args, **kw)


def fill(m: torch.nn.Module, prefix: str) -> None:
    """oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma` and on every `layer_scale*`
    parameter: the rule of tools/gen_golden_patchconvnet.py"""
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if (p.dim() == 1 and k.endswith(("weight", "gamma"))) or k.rsplit(".", 1)[-1].startswith("layer_scale"):
                p.add_(1.0)


def inputs(g):
    """(prefix, images, projection of y) from the recipe stored in the fixture"""
    pre, kx, kr = [str(s) for s in g["recipe"]]
    x = filler.tensor(kx, tuple(int(v) for v in g["x_shape"]))
    return pre, x, filler.tensor(kr, tuple(int(v) for v in g["y_shape"]))


def stored(name: str, v: torch.Tensor) -> torch.Tensor:
    """the elements of array `name` that the fixture holds: all of them up to 4096, else 4096 picked by a permutation seeded
    by the CRC32 of the name (`sample_index` of the generator)"""
    v = v.detach()
    if v.numel() <= SAMPLE:
        return v
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    idx = np.sort(rs.permutation(v.numel())[:SAMPLE])
    return v.reshape(-1)[torch.from_numpy(idx).to(v.device)]
