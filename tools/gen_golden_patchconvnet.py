"""Generate tests/golden/patchconvnet_<case>.npz by running the UNMODIFIED reference PatchConvNet
(vision_toolbox/backbones/patchconvnet.py) on CPU.  Runs only where the reference is present.

    python tools/gen_golden_patchconvnet.py

The stand-ins.  The reference module imports `torchvision.ops.StochasticDepth` and `torchvision.ops.misc.SqueezeExcitation`,
and torchvision is not installed.  Inside tools/gen_golden.py's `reference_namespace` (reused unchanged) two stand-ins of our
own are hung on its torchvision stub before the reference source is imported, unmodified:

  * `SqueezeExcitation(input_channels, squeeze_channels)`: `avgpool` (AdaptiveAvgPool2d(1)), `fc1`, `fc2` (1x1 nn.Conv2d),
    `activation` (ReLU), `scale_activation` (Sigmoid); forward = scale * input -- the definition this package ships;
  * `StochasticDepth(p, mode)`: the identity in eval mode, and it RAISES in training mode with p > 0 (no fixture may depend
    on a random mask).

Cases (constructor, input, modes):

    a  (64, 1, mlp_ratio=2, drop_path=0.0, norm_type="bn")   batch 3, 32x32 (2x2 tokens, every pixel on a border)  train, eval
    b  (64, 2, mlp_ratio=1, drop_path=0.3, norm_type="ln")   batch 2, 80x48 (5x3 tokens)                          eval
    c  (128, 1, norm_type="bn", drop_path=0.0)               batch 2, 112x112 (7x7 tokens)                        train, eval

Per case and mode `<mode>/y` (B, C), `<mode>/dx` and `<mode>/grad/<key>` of the loss (y * r).sum(), in float32; for case c also
the BatchNorm buffers after the ONE training forward (`train/running/<key>`).  Every run starts from the same filled state.

Sampling.  An array of more than 4096 elements is stored as 4096 of its elements, picked by `sample_index` (a permutation
seeded by the CRC32 of the array's name, sorted): every gradient of the 128-wide case in two modes is several MB, a committed
file at most 1 MiB.  The tests compare the same elements.

Weights: the rule of tools/gen_golden_vit.py (oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight`
or `gamma`) AND +1.0 on every `layer_scale*` parameter: the filler alone leaves the block branch at a few percent of the
stream's rms, which would hide a block error twentyfold.

Conditions, asserted here and stored (`cond/...`), float64, on the first block and the pool, in each stored mode:
branch rms / stream rms >= 0.15; every SE gate in (0.05, 0.95) with a standard deviation >= 0.02; the standard deviation of
the pool's scores about their row mean in [0.25, 3].

Floors (`floor/f32/<mode>/...`, `floor/bf16/<mode>/...`): the reference in float32, and under torch.autocast("cpu", bfloat16)
with every module output rounded to bfloat16 by forward hooks, each against the reference in float64, in the tests' clamped
metric, on the stored elements.
"""
from __future__ import annotations

import importlib
import sys
import types
import zlib
from pathlib import Path

import numpy as np
import torch
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
from oracle import filler  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
SAMPLE = 4096


class SqueezeExcitation(nn.Module):
    def __init__(self, input_channels, squeeze_channels, activation=nn.ReLU, scale_activation=nn.Sigmoid):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = activation()
        self.scale_activation = scale_activation()

    def forward(self, input):
        return self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(input))))) * input


class StochasticDepth(nn.Module):
    def __init__(self, p, mode):
        super().__init__()
        self.p, self.mode = float(p), mode

    def forward(self, x):
        if self.training and self.p > 0:
            raise RuntimeError("the StochasticDepth stand-in of the fixture tools is the identity: eval mode or p = 0 only")
        return x


def ref_patchconvnet():
    """the unmodified reference module, imported behind the two stand-ins"""
    with gen_golden.reference_namespace():
        ops = sys.modules["torchvision.ops"]
        misc = types.ModuleType("torchvision.ops.misc")
        misc.SqueezeExcitation = SqueezeExcitation
        ops.StochasticDepth, ops.misc = StochasticDepth, misc
        sys.modules["torchvision.ops.misc"] = misc
        return importlib.import_module("vision_toolbox.backbones.patchconvnet")


CASES = {  # name -> (constructor args, constructor kwargs, (batch, H, W), modes)
    "a": ((64, 1), {"mlp_ratio": 2, "drop_path": 0.0, "norm_type": "bn"}, (3, 32, 32), ("train", "eval")),
    "b": ((64, 2), {"mlp_ratio": 1, "drop_path": 0.3, "norm_type": "ln"}, (2, 80, 48), ("eval",)),
    "c": ((128, 1), {"norm_type": "bn", "drop_path": 0.0}, (2, 112, 112), ("train", "eval")),
}


def fill(m: nn.Module, prefix: str) -> None:
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if (p.dim() == 1 and k.endswith(("weight", "gamma"))) or k.rsplit(".", 1)[-1].startswith("layer_scale"):
                p.add_(1.0)


def sample_index(name: str, numel: int):
    """the elements of array `name` that are stored (None: all of them)"""
    if numel <= SAMPLE:
        return None
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return np.sort(rs.permutation(numel)[:SAMPLE])


def stored(name: str, v: torch.Tensor) -> torch.Tensor:
    idx = sample_index(name, v.numel())
    return v if idx is None else v.reshape(-1)[torch.from_numpy(idx)]


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run(m, sd0, x, r, mode, autocast=False):
    m.load_state_dict(sd0)
    m.train(mode == "train")
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    hooks = [mod.register_forward_hook(_to_bf16) for mod in m.modules()] if autocast else []
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        y = m(x)
    (y.to(r.dtype) * r).sum().backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "dx": x.grad.detach()}
    for k, p in m.named_parameters():
        out["grad/" + k] = p.grad.detach().clone()
    if mode == "train":
        for k, v in m.named_buffers():
            out["running/" + k] = v.detach().clone()
    return {k: stored(k, v) for k, v in out.items()}


def gerr(a, b):
    """the tests' metric (tests/test_convnext_gpu.py `_gerr`)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))


def conditions(m, x, mode):
    """(branch rms / stream rms, gate min, gate max, gate std, pool score std) of the first block and the pool, float64"""
    seen = {}
    blk, pool = m.trunk[1], m.pool
    se = next(mod for mod in blk.layers if isinstance(mod, SqueezeExcitation))
    hooks = [
        blk.register_forward_hook(lambda mod, i, o: seen.update(stream=i[0].detach(), branch=(o - i[0]).detach())),
        se.scale_activation.register_forward_hook(lambda mod, i, o: seen.update(gate=o.detach())),
        pool.register_forward_hook(lambda mod, i, o: seen.update(tokens=i[0].detach())),
    ]
    m.train(mode == "train")
    with torch.no_grad():
        m(x)
        for h in hooks:
            h.remove()
        t = seen["tokens"]
        C = t.shape[-1]
        n = pool.norm_1(torch.cat((pool.cls_token.expand(t.shape[0], 1, -1), t), 1))
        w, b = pool.attn.in_proj_weight, pool.attn.in_proj_bias
        q = n[:, :1] @ w[:C].T + b[:C]
        k = n @ w[C:2 * C].T + b[C:2 * C]
        s = (q @ k.transpose(1, 2)) * C ** -0.5
        score_std = float((s - s.mean(-1, keepdim=True)).std())
    rms = lambda v: float(v.pow(2).mean().sqrt())
    g = seen["gate"]
    return rms(seen["branch"]) / rms(seen["stream"]), float(g.min()), float(g.max()), float(g.std()), score_std


def main():
    pcn = ref_patchconvnet()
    for name, (args, kw, (B, H, W), modes) in CASES.items():
        pre = f"patchconvnet_{name}."
        m = pcn.PatchConvNet(*args, **kw)
        fill(m, pre)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        x = filler.tensor(pre + "x", (B, 3, H, W))
        r = filler.tensor(pre + "r", (B, args[0]))
        out = {
            "keys": np.array(list(sd0.keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in sd0.values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, H, W]),
            "y_shape": np.array([B, args[0]]),
            "modes": np.array(list(modes)),
        }
        for mode in modes:
            res32 = run(m, sd0, x, r, mode)
            res16 = run(m, sd0, x, r, mode, autocast=True)
            m.double()
            sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd0.items()}
            res64 = run(m, sd64, x.double(), r.double(), mode)
            m.load_state_dict(sd64)
            ratio, gmin, gmax, gstd, sstd = conditions(m, x.double(), mode)
            m.float()
            print(name, mode, f"branch/stream {ratio:.3f}  gates [{gmin:.3f}, {gmax:.3f}] std {gstd:.3f}  score std {sstd:.3f}")
            assert ratio >= 0.15, ratio
            assert 0.05 < gmin and gmax < 0.95 and gstd >= 0.02, (gmin, gmax, gstd)
            assert 0.25 <= sstd <= 3.0, sstd
            out[f"cond/{mode}"] = np.array([ratio, gmin, gmax, gstd, sstd])
            for k, v in res32.items():
                if k.startswith("running/") and name != "c":
                    continue
                out[f"{mode}/{k}"] = v.numpy().copy()
            for tag, res in (("f32", res32), ("bf16", res16)):
                errs = {k: gerr(v, res64[k]) for k, v in res.items() if not k.startswith("running/")}
                for k, e in errs.items():
                    out[f"floor/{tag}/{mode}/{k}"] = np.array(e)
                gmax_ = max(e for k, e in errs.items() if k.startswith("grad/"))
                out[f"floor/{tag}/{mode}/grad_max"] = np.array(gmax_)
                print(name, mode, tag, {k: f"{errs[k]:.2e}" for k in ("y", "dx")}, f"grad_max {gmax_:.2e}")
        path = GOLDEN / f"patchconvnet_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
