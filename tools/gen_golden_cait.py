"""Generate tests/golden/cait_<case>.npz and tests/golden/cait_ckpt.npz by running the UNMODIFIED reference CaiT
(vision_toolbox/backbones/cait.py) on CPU.  Same shim as tools/gen_golden.py; runs only where the reference is present.

    python tools/gen_golden_cait.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the output `y` (B, d_model),
the image gradient `dx` and every parameter gradient of the loss (y * r).sum().  Train and eval mode compute the same
function (no BatchNorm, dropout 0, stochastic depth 0): one mode is stored.

The class token.  The reference joins its (1, 1, d) parameter to the (N, L, d) patch tokens with torch.cat, which raises at
batch > 1.  Every case is therefore run ONE IMAGE AT A TIME: the outputs and image gradients are stacked, the parameter
gradients summed over the images.

Weights: the rule of tools/gen_golden_vit.py -- oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in
`weight` or `gamma`.  The filler gives the 4-D [H][H][1][1] head-mixing weights a standard deviation of sqrt(2 / H): both
mixes are non-trivial and non-symmetric.  `m_std` is the standard deviation (about the row mean, float64) of the MIXED scores
M of the first SA block; the generator asserts it lies in [0.3, 3] -- rows neither uniform nor one-hot.

Floors (`floor/f32/...`, `floor/bf16/...`): the reference in float32, and under torch.autocast("cpu", bfloat16) with every
module output rounded to bfloat16 by forward hooks, each against the reference in float64, in the tests' clamped metric.

`zero_grad_keys`: the parameters whose float64 gradient has an rms below 1e-12: every `k_proj.bias` (a constant added to
every key shifts each row of scores by a constant per head, which the mix turns into a constant per mixed row, which softmax
ignores) and every `talking_head_proj.0.bias` (the same constant directly).  tests/cait_util.py asserts that set.

The checkpoint fixture: filler values in the official key layout for CaiT(48, 1, 1, 1, 4, 8), the classifier head included
(`official/<key>`), and the state_dict the reference's `load_official_ckpt` makes of them (`sd/<key>`).
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

cait = gen_golden.ref_import("vision_toolbox.backbones.cait")
GOLDEN = ROOT / "tests" / "golden"

CASES = {  # name -> (constructor args (d_model, sa_depth, ca_depth, n_heads, patch, img), constructor kwargs, batch)
    "a": ((96, 1, 1, 2, 4, 16), {"mlp_ratio": 2.0}, 3),  # L = 16: below a 64-row tile, exactly one 16-row tile
    "b": ((96, 2, 1, 2, 4, 32), {"mlp_ratio": 1.0}, 2),  # L = 64; class attention sees 65 keys
    "c": ((96, 1, 2, 2, 4, 36), {"mlp_ratio": 1.0, "layer_scale_init": None}, 2),  # L = 81, no LayerScale, two CA blocks
}
CKPT_ARGS, CKPT_CLASSES = (48, 1, 1, 1, 4, 8), 10


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


def mixed_score_std(m, x):
    """standard deviation of the first SA block's mixed scores M about their row means (float64)"""
    with torch.no_grad():
        t = m.patch_embed(x).flatten(2).transpose(1, 2) + m.pe
        blk = m.sa_layers[0]
        n, mha = blk.mha[0](t), blk.mha[1]
        q = mha.q_proj(n).unflatten(-1, (mha.n_heads, -1)).transpose(-2, -3)
        k = mha.k_proj(n).unflatten(-1, (mha.n_heads, -1)).transpose(-2, -3)
        s = mha.talking_head_proj[0](mha.scale * q @ k.transpose(-1, -2))
        return float((s - s.mean(-1, keepdim=True)).std())


def ckpt_fixture():
    d, sa, ca, h, p, img = CKPT_ARGS
    m = cait.CaiT(*CKPT_ARGS)
    pre = "cait_ckpt."
    src = {}

    def put(key, shape):
        src[key] = filler.tensor(pre + key, tuple(shape))

    def put_wb(prefix, wshape):
        put(prefix + ".weight", wshape)
        put(prefix + ".bias", wshape[:1])

    def put_common(prefix, blk):
        hidden = blk.mlp[1].linear1.out_features
        put_wb(prefix + "norm1", (d,))
        put_wb(prefix + "attn.proj", (d, d))
        put(prefix + "gamma_1", (d,))
        put_wb(prefix + "norm2", (d,))
        put_wb(prefix + "mlp.fc1", (hidden, d))
        put_wb(prefix + "mlp.fc2", (d, hidden))
        put(prefix + "gamma_2", (d,))

    put_wb("patch_embed.proj", (d, 3, p, p))
    put("cls_token", (1, 1, d))
    put("pos_embed", (1, (img // p) ** 2, d))
    for i, blk in enumerate(m.sa_layers):
        prefix = f"blocks.{i}."
        put_common(prefix, blk)
        put_wb(prefix + "attn.qkv", (3 * d, d))
        put_wb(prefix + "attn.proj_l", (h, h))
        put_wb(prefix + "attn.proj_w", (h, h))
    for i, blk in enumerate(m.ca_layers):
        prefix = f"blocks_token_only.{i}."
        put_common(prefix, blk)
        for what in ("q", "k", "v"):
            put_wb(prefix + "attn." + what, (d, d))
    put_wb("norm", (d,))
    put_wb("head", (CKPT_CLASSES, d))
    out = {"args": np.array(CKPT_ARGS)}
    for k, v in src.items():
        out["official/" + k] = v.numpy().copy()
    m.load_official_ckpt({k: v.clone() for k, v in src.items()})  # (pops what it reads; asserts that the head remains)
    for k, v in m.state_dict().items():
        out["sd/" + k] = v.numpy().copy()
    path = GOLDEN / "cait_ckpt.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def main():
    for name, (args, kw, B) in CASES.items():
        pre = f"cait_{name}."
        m = cait.CaiT(*args, **kw)
        fill(m, pre)
        m.eval()
        S = args[5]
        x = filler.tensor(pre + "x", (B, 3, S, S))
        r = filler.tensor(pre + "r", (B, args[0]))
        res32 = run(m, x, r)
        res16 = run(m, x, r, autocast=True)
        res64 = run(m.double(), x.double(), r.double())
        m_std = mixed_score_std(m, x.double())
        print(name, f"mixed score std (SA block 0, float64) {m_std:.3f}")
        assert 0.3 <= m_std <= 3.0, m_std
        m.float()
        zero = sorted(k[5:] for k, v in res64.items()
                      if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, S, S]),
            "per_image": np.array(1),
            "m_std": np.array(m_std),
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
            print(name, tag, {k: f"{errs[k]:.2e}" for k in ("y", "dx")}, f"grad_max {max(live):.2e}")
        print(name, "zero keys", zero)
        path = GOLDEN / f"cait_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")
    ckpt_fixture()


if __name__ == "__main__":
    main()
