"""Generate tests/golden/deit_<case>.npz and tests/golden/deit_ckpt.npz by running the UNMODIFIED reference DeiT / DeiT3
(vision_toolbox/backbones/deit.py) on CPU, in the manner of tools/gen_golden_vit.py.  Same shim as tools/gen_golden.py; runs
only where the reference is present.

    python tools/gen_golden_deit.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the output `y` (B, d_model),
the image gradient `dx` and every parameter gradient of the loss (y * r).sum().  Train and eval mode compute the same
function (no BatchNorm, dropout 0, stochastic depth 0): one mode is stored.

The prefix tokens.  The reference joins its (1, 1, d) parameters to the (N, T, d) patch tokens with torch.cat, which raises at
batch > 1.  Every case is therefore run ONE IMAGE AT A TIME: the outputs and image gradients are stacked, the parameter
gradients summed over the images (`per_image` = 1 in the fixture).

Weights: oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in `weight` or `gamma` (DeiT3's default layer
scale of 1e-6 becomes 1 + filler).  tests/deit_util.fill applies the same rule.

Floors (`floor/f32/...`, `floor/bf16/...`): the reference in float32, and under torch.autocast("cpu", bfloat16) with every
module output rounded to bfloat16 by forward hooks, each against the reference in float64, in the tests' clamped metric.  The
bf16 gradient bound of the module tests is min(4 x floor, 0.25): this generator ASSERTS that every stored `floor/bf16/*` is
below 0.0625, so that the cap never binds.

`zero_grad_keys`: the parameters whose float64 gradient has an rms below 1e-12; asserted to be exactly the `k_proj.bias` keys
(a constant added to every key shifts each row of scores by a constant, which softmax ignores).

The checkpoint fixture: filler values in the key layout of the official DeiT repository for DeiT(32, 1, 1, 4, 8) (`pos_embed`
with T + 2 rows, `dist_token`, `head_dist.*`, `head.*`) and DeiT3(32, 1, 1, 4, 8) (`pos_embed` with T rows, `gamma_1/2`,
`head.*`) under `<tag>/src/<key>`, and the state_dicts the reference's `load_official_ckpt` produces from them under
`<tag>/sd/<key>`.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gen_golden  # noqa: E402  (the import shim for the reference's vision_toolbox.*)
from oracle import filler  # noqa: E402

deit = gen_golden.ref_import("vision_toolbox.backbones.deit")
GOLDEN = ROOT / "tests" / "golden"

CASES = {  # name -> (class, constructor args (d_model, depth, n_heads, patch, img), constructor kwargs, batch)
    "a": ("DeiT", (64, 2, 2, 4, 16), {}, 3),  # L = 18: below one attention tile, two heads of 32
    "b": ("DeiT", (64, 1, 1, 4, 32), {"layer_scale_init": 0.5}, 2),  # L = 66: two keys past a tile, head_dim 64, LayerScale
    "c": ("DeiT3", (64, 2, 1, 4, 16), {}, 2),  # L = 17: the default LayerScale
}
CKPT_ARGS = (32, 1, 1, 4, 8)
FLOOR_CAP = 0.0625


def fill(m: torch.nn.Module, prefix: str) -> None:
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)


def _to_bf16(mod, inputs, out):
    return out.to(torch.bfloat16) if torch.is_tensor(out) and out.is_floating_point() else out


def run_once(m, x, r, autocast=False):
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


def run(m, x, r, autocast=False):
    parts = [run_once(m, x[b:b + 1], r[b:b + 1], autocast) for b in range(x.shape[0])]
    out = {"y": torch.cat([p["y"] for p in parts]), "dx": torch.cat([p["dx"] for p in parts])}
    for k in parts[0]:
        if k.startswith("grad/"):
            out[k] = sum(p[k].double() for p in parts).to(parts[0][k].dtype)
    return out


def gerr(a, b):
    """the tests' metric (tests/test_convnext_gpu.py `_gerr`)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-3 * (b.numel() ** 0.5)))


def official_source(m, pre: str, distilled: bool) -> dict:
    """filler values in the official repository's key layout"""
    d, _, _, p, img = CKPT_ARGS
    T = (img // p) ** 2
    src = {}

    def put(key, shape):
        src[key] = filler.tensor(pre + key, tuple(shape)).clone()

    put("patch_embed.proj.weight", (d, 3, p, p))
    put("patch_embed.proj.bias", (d,))
    put("cls_token", (1, 1, d))
    put("pos_embed", (1, T + 2 if distilled else T, d))
    if distilled:
        put("dist_token", (1, 1, d))
        put("head_dist.weight", (10, d))
        put("head_dist.bias", (10,))
    for i, layer in enumerate(m.layers):
        blk, hidden = f"blocks.{i}.", layer.mlp[1].linear1.out_features
        for key, shape in (("norm1.weight", (d,)), ("norm1.bias", (d,)), ("attn.qkv.weight", (3 * d, d)), ("attn.qkv.bias", (3 * d,)),
                           ("attn.proj.weight", (d, d)), ("attn.proj.bias", (d,)), ("norm2.weight", (d,)), ("norm2.bias", (d,)),
                           ("mlp.fc1.weight", (hidden, d)), ("mlp.fc1.bias", (hidden,)), ("mlp.fc2.weight", (d, hidden)),
                           ("mlp.fc2.bias", (d,))):
            put(blk + key, shape)
        if not distilled:
            put(blk + "gamma_1", (d,))
            put(blk + "gamma_2", (d,))
    put("norm.weight", (d,))
    put("norm.bias", (d,))
    put("head.weight", (10, d))
    put("head.bias", (10,))
    return src


def ckpt_fixture():
    out = {"args": np.array(CKPT_ARGS)}
    for tag, cls, distilled in (("deit", deit.DeiT, True), ("deit3", deit.DeiT3, False)):
        m = cls(*CKPT_ARGS)
        src = official_source(m, f"deit_ckpt.{tag}.", distilled)
        m.load_official_ckpt({k: v.clone() for k, v in src.items()})  # (the reference pops from the dict it is given)
        for k, v in src.items():
            out[f"{tag}/src/{k}"] = v.numpy().copy()
        for k, v in m.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.numpy().copy()
    path = GOLDEN / "deit_ckpt.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def main():
    for name, (cls, args, kw, B) in CASES.items():
        pre = f"deit_{name}."
        m = getattr(deit, cls)(*args, **kw)
        fill(m, pre)
        m.eval()
        S = args[4]
        x = filler.tensor(pre + "x", (B, 3, S, S))
        r = filler.tensor(pre + "r", (B, args[0]))
        res32 = run(m, x, r)
        res16 = run(m, x, r, autocast=True)
        res64 = run(m.double(), x.double(), r.double())
        m.float()
        zero = sorted(k[5:] for k, v in res64.items()
                      if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
        assert zero == sorted(f"layers.{i}.mha.1.k_proj.bias" for i in range(args[1])), zero
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, S, S]),
            "per_image": np.array(1),
            "zero_grad_keys": np.array(zero),
        }
        for k, v in res32.items():
            out[k] = v.numpy().copy()
        for tag, res in (("f32", res32), ("bf16", res16)):
            errs = {k: gerr(v, res64[k]) for k, v in res.items()}
            for k, e in errs.items():
                out[f"floor/{tag}/{k}"] = np.array(e)
            live = {k: e for k, e in errs.items() if k.startswith("grad/") and k[5:] not in zero}
            out[f"floor/{tag}/grad_max"] = np.array(max(live.values()))
            worst = max(live, key=live.get)
            print(name, tag, {k: f"{errs[k]:.2e}" for k in ("y", "dx")}, f"grad_max {live[worst]:.2e} ({worst})")
            if tag == "bf16":
                over = {k: e for k, e in errs.items() if k[5:] not in zero and not e < FLOOR_CAP}
                assert not over, f"case {name}: bf16 floors at or above {FLOOR_CAP}: {over}"
        path = GOLDEN / f"deit_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")
    ckpt_fixture()


if __name__ == "__main__":
    main()
