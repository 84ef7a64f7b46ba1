"""Generate tests/golden/swin_<case>.npz and tests/golden/swin_ckpt.npz by running the UNMODIFIED reference Swin Transformer
(vision_toolbox/backbones/swin.py) on CPU.  Same shim as tools/gen_golden.py; runs only where the reference is present.

    python tools/gen_golden_swin.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the output `y` (B, C_last),
the four stage maps' shapes, the image gradient `dx` and every parameter gradient of the loss (y * r).sum().  Train and eval
mode compute the same function (no BatchNorm, dropout 0, stochastic depth 0): one mode is stored.

The shift mask.  The reference adds its (windows, 1, L, L) mask to the (1, heads, L, L) bias and hands the result to
scaled_dot_product_attention over (B * windows, heads, L, head_dim) operands, which cannot broadcast it: a shifted block
raises at batch > 1.  Every case that contains a shifted block is therefore run ONE IMAGE AT A TIME: the outputs and image
gradients are stacked, the parameter gradients summed over the images (`per_image` = 1 in the fixture), exactly as
tools/gen_golden_vit.py does for the class token.  Cases without a shifted block run batched.

Weights: the rule of tools/gen_golden_vit.py -- oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in
`weight` or `gamma` -- and, in addition, every `relative_pe_table` multiplied by 10 (standard deviation 1.0): a wrong bias
index then moves the output by 1e-1, not 1e-3.  tests/swin_util.fill applies the same rule.

Floors (`floor/f32/...`, `floor/bf16/...`) and `zero_grad_keys` (every `k_proj.bias`): as in tools/gen_golden_vit.py.

Parameter gradients are stored SAMPLED (`sample` below; tests/swin_util.sample is the same rule): every parameter, but of a
tensor of more than 2048 elements every s-th element only, and the floors are those of the sampled arrays.

The checkpoint fixture: an official-layout (microsoft/Swin-Transformer) state_dict of filler values for a two-stage model
(`official/<key>`; `attn_mask` and `relative_position_index` are the reference module's own buffers, which
`load_official_ckpt` compares) and the state_dict `load_official_ckpt` makes of it (`sd/<key>`): the merging `rearrange`
and the table transpose.  Also `T_224_params`, the parameter count of from_config("T", 224).
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

swin = gen_golden.ref_import("vision_toolbox.backbones.swin")
GOLDEN = ROOT / "tests" / "golden"
SAMPLE_ABOVE, SAMPLES = 2048, 1024


def sample(t):
    """the elements of a gradient that the fixtures store: all of a tensor of at most SAMPLE_ABOVE elements, else every
    s-th of the flattened tensor with s = (numel // SAMPLES) | 1 -- odd, so the samples walk through every row and column
    of the power-of-two-sided weights -- which keeps a fixture at a few hundred KB; EVERY parameter is still compared"""
    flat = t.reshape(-1)
    return flat if flat.numel() <= SAMPLE_ABOVE else flat[:: (flat.numel() // SAMPLES) | 1]

CASES = {  # name -> (constructor args (img, d_model, n_heads, depths, window_sizes), constructor kwargs, batch)
    "a": ((48, 32, 1, (2, 2), (4, 3)), {}, 2),  # 12x12 in 3x3 windows of 16 tokens, shift 2; then 6x6, ws 3, shift 1
    "b": ((56, 64, 2, (2, 1), (7, 7)), {}, 2),  # the real ws 7 / shift 3 on 14x14; then one unshifted 7x7 window
    "c": ((32, 32, 1, (1, 1), (8, 4)), {"layer_scale_init": 0.5}, 2),  # L = 64, exactly one tile; no shift: batched
}
CKPT_ARGS = (32, 8, 2, (2, 1), (4, 4))  # (CPU only: two heads of 4, so that the table transpose is visible)


def fill(m: torch.nn.Module, prefix: str) -> None:
    filler.fill_module(m, prefix)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and k.endswith(("weight", "gamma")):
                p.add_(1.0)
            if k.endswith("relative_pe_table"):
                p.mul_(10.0)


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


def run(m, x, r, per_image, autocast=False):
    if not per_image:
        return run_once(m, x, r, autocast)
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


def shifted(m) -> bool:
    return any(isinstance(mod, swin.WindowAttention) and mod.shift > 0 for mod in m.modules())


def save(name: str, out: dict) -> None:
    path = GOLDEN / f"swin_{name}.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def ckpt_fixture():
    m = swin.SwinTransformer(*CKPT_ARGS)
    pre, src = "swin_ckpt.", {}

    def put(key, shape):
        src[key] = filler.tensor(pre + key, tuple(shape))

    def put_wb(key, mod):
        put(key + ".weight", mod.weight.shape)
        put(key + ".bias", mod.bias.shape)

    put_wb("patch_embed.proj", m.patch_embed)
    put_wb("patch_embed.norm", m.patch_norm)
    for s, stage in enumerate(m.stages):
        if s > 0:
            put_wb(f"layers.{s - 1}.downsample.norm", stage[0].norm)
            put(f"layers.{s - 1}.downsample.reduction.weight", stage[0].reduction.weight.shape)
        for i in range(1, len(stage)):
            blk, p = stage[i], f"layers.{s}.blocks.{i - 1}."
            attn, d = blk.mha[1], blk.mha[1].q_proj.in_features
            put_wb(p + "norm1", blk.mha[0])
            if attn.attn_mask is not None:
                src[p + "attn_mask"] = attn.attn_mask.clone()
            src[p + "attn.relative_position_index"] = attn.relative_pe_index.clone()
            put(p + "attn.qkv.weight", (3 * d, d))
            put(p + "attn.qkv.bias", (3 * d,))
            put_wb(p + "attn.proj", attn.out_proj)
            put(p + "attn.relative_position_bias_table", (attn.relative_pe_table.shape[2], attn.n_heads))
            put_wb(p + "norm2", blk.mlp[0])
            put_wb(p + "mlp.fc1", blk.mlp[1].linear1)
            put_wb(p + "mlp.fc2", blk.mlp[1].linear2)
    put_wb("norm", m.norm)
    put("head.weight", (10, m.norm.weight.shape[0]))
    put("head.bias", (10,))
    out = {"args": np.array(str(CKPT_ARGS))}
    for k, v in src.items():
        out["official/" + k] = v.numpy().copy()
    m.load_official_ckpt({k: v.clone() for k, v in src.items()})
    for k, v in m.state_dict().items():
        out["sd/" + k] = v.numpy().copy()
    n_t = sum(p.numel() for p in swin.SwinTransformer.from_config("T", 224).parameters())
    print(f"from_config('T', 224): {n_t} parameters")
    out["T_224_params"] = np.array(n_t)
    path = GOLDEN / "swin_ckpt.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def main():
    for name, (args, kw, B) in CASES.items():
        pre = f"swin_{name}."
        m = swin.SwinTransformer(*args, **kw)
        fill(m, pre)
        m.eval()
        S = args[0]
        per_image = shifted(m)
        x = filler.tensor(pre + "x", (B, 3, S, S))
        with torch.no_grad():
            maps = m.get_feature_maps(x[:1])
        r = filler.tensor(pre + "r", (B, maps[-1].shape[-1]))
        res32 = run(m, x, r, per_image)
        res16 = run(m, x, r, per_image, autocast=True)
        res64 = run(m.double(), x.double(), r.double(), per_image)
        m.float()
        zero = sorted(k[5:] for k, v in res64.items()
                      if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
        for res in (res32, res16, res64):
            res.update({k: sample(v) for k, v in res.items() if k.startswith("grad/")})
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, S, S]),
            "map_shapes": np.array([[B] + list(f.shape[1:]) for f in maps]),
            "per_image": np.array(int(per_image)),
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
        print(name, "per_image", per_image, "float64 rms of the zero gradients",
              [f"{float(res64['grad/' + k].norm()) / res64['grad/' + k].numel() ** 0.5:.1e}" for k in zero])
        save(name, out)
    ckpt_fixture()


if __name__ == "__main__":
    main()
