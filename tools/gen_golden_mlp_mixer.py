"""Generate tests/golden/mlp_mixer_<case>.npz and tests/golden/mlp_mixer_flax.npz by running the UNMODIFIED reference
MLPMixer (vision_toolbox/backbones/mlp_mixer.py) on CPU.  Same shim as tools/gen_golden.py; runs only where the reference
is present.

    python tools/gen_golden_mlp_mixer.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the output `y` (B, d_model),
the image gradient `dx` and every parameter gradient of the loss (y * r).sum() -- the class returns no feature map to
project.  Train and eval mode compute the same function (no BatchNorm, dropout 0): one mode is stored.

Weights: the rule of tools/gen_golden_convnext.py -- oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in
`weight` or `gamma`.  tests/mlp_mixer_util.fill applies the same rule.

Floors (`floor/f32/...`, `floor/bf16/...`): the error of the reference in float32, and under torch.autocast("cpu",
bfloat16) with every module output rounded to bfloat16 by forward hooks (the recipe of tools/gen_golden_convnext.py),
each against the reference in float64 -- measured with the TESTS' metric, norm of the difference over
max(norm of the truth, 1e-3 sqrt(numel)) (`_gerr` of tests/test_convnext_gpu.py), not the unclamped relative error.

`zero_grad_keys`: the parameters whose float64 gradient has an rms below 1e-12.  The gradient of
`layers.i.token_mixing.linear2.bias` is exactly zero in exact arithmetic: that bias adds a per-token constant across
channels, which every later LayerNorm removes (the residual stream only carries it to the next LayerNorm).  What any
rounded run reports there is noise of the size of the clamped denominator; the module and trainer tests skip exactly these
keys (and assert which they are), the kernel and builder tests of tests/test_token_mix_gpu.py cover those gradients where
they are not zero.  `grad_max` leaves them out.

The Flax fixture: filler values in the key layout of the official checkpoints (`stem`, `MixerBlock_i/...`,
`pre_head_layer_norm`, kernels input-major) under `flax/<key>`, and under `sd/<key>` the state_dict the reference's
`load_jax_weights` produces from them.
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
from oracle import filler  # noqa: E402

mix = gen_golden.ref_import("vision_toolbox.backbones.mlp_mixer")
GOLDEN = ROOT / "tests" / "golden"

CASES = {  # name -> (constructor args, constructor kwargs, batch)
    "a": ((2, 32, 4, 20), {}, 3),   # 25 tokens -> 16 hidden tokens: a K tail, an odd count
    "b": ((2, 48, 8, 56), {}, 2),   # 49 -> 24, patch rows of 192
    "c": ((1, 24, 4, 24), {"mlp_ratio": (1.0, 2.0)}, 2),  # 36 -> 24
}
FLAX_ARGS = (2, 16, 4, 12)  # 9 tokens -> 8 hidden tokens


def fill(m: torch.nn.Module, prefix: str) -> None:
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run(m, x, r, autocast=False):
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
    return out


def gerr(a, b):
    """the tests' metric (tests/test_convnext_gpu.py `_gerr`)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))


def flax_fixture():
    m = mix.MLPMixer(*FLAX_ARGS)
    pre = "mlp_mixer_flax."
    src = {}

    def put(key, shape):
        src[key] = filler.tensor(pre + key, tuple(shape)).numpy().copy()

    p, d = FLAX_ARGS[2], FLAX_ARGS[1]
    put("stem/kernel", (p, p, 3, d))
    put("stem/bias", (d,))
    put("pre_head_layer_norm/scale", (d,))
    put("pre_head_layer_norm/bias", (d,))
    for i, blk in enumerate(m.layers):
        for j in range(2):
            put(f"MixerBlock_{i}/LayerNorm_{j}/scale", (d,))
            put(f"MixerBlock_{i}/LayerNorm_{j}/bias", (d,))
        for what, mlp in (("token_mixing", blk.token_mixing), ("channel_mixing", blk.channel_mixing)):
            for j, lin in enumerate((mlp.linear1, mlp.linear2)):
                put(f"MixerBlock_{i}/{what}/Dense_{j}/kernel", (lin.in_features, lin.out_features))
                put(f"MixerBlock_{i}/{what}/Dense_{j}/bias", (lin.out_features,))
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "ckpt.npz")
        np.savez(path, **src)
        m.load_jax_weights(path)
    out = {"args": np.array(FLAX_ARGS)}
    for k, v in src.items():
        out["flax/" + k] = v
    for k, v in m.state_dict().items():
        out["sd/" + k] = v.numpy().copy()
    path = GOLDEN / "mlp_mixer_flax.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def main():
    for name, (args, kw, B) in CASES.items():
        pre = f"mlp_mixer_{name}."
        m = mix.MLPMixer(*args, **kw)
        fill(m, pre)
        m.eval()
        S = args[3]
        x = filler.tensor(pre + "x", (B, 3, S, S))
        r = filler.tensor(pre + "r", (B, args[1]))
        res32 = run(m, x, r)
        res16 = run(m, x, r, autocast=True)
        res64 = run(m.double(), x.double(), r.double())
        m.float()
        zero = sorted(k[5:] for k, v in res64.items()
                      if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, S, S]),
            "zero_grad_keys": np.array(zero),
        }
        for k, v in res32.items():
            out[k] = v.numpy().copy()
        for tag, res in (("f32", res32), ("bf16", res16)):
            errs = {k: gerr(v, res64[k]) for k, v in res.items()}
            for k, e in errs.items():
                out[f"floor/{tag}/{k}"] = np.array(e)
            live = [e for k, e in errs.items() if k.startswith("grad/") and k[5:] not in zero]
            out[f"floor/{tag}/grad_max"] = np.array(max(live))
            print(name, tag, {k: f"{errs[k]:.2e}" for k in ("y", "dx")}, f"grad_max {max(live):.2e}",
                  "zero keys", {k: f"{errs['grad/' + k]:.2e}" for k in zero})
        print(name, "float64 rms of the zero gradients",
              [f"{float(res64['grad/' + k].norm()) / res64['grad/' + k].numel() ** 0.5:.1e}" for k in zero])
        path = GOLDEN / f"mlp_mixer_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")
    flax_fixture()


if __name__ == "__main__":
    main()
