"""Generate tests/golden/vit_<case>.npz, tests/golden/vit_flax.npz and tests/golden/vit_resize.npz by running the UNMODIFIED
reference ViT (vision_toolbox/backbones/vit.py) on CPU.  Same shim as tools/gen_golden.py; runs only where the reference is
present.

    python tools/gen_golden_vit.py

Per case: the state_dict keys and shapes (string arrays), the recipe of the inputs (filler keys), the output `y` (B, d_model),
the image gradient `dx` and every parameter gradient of the loss (y * r).sum().  Train and eval mode compute the same
function (no BatchNorm, dropout 0, stochastic depth 0): one mode is stored.

The class token.  The reference joins its (1, 1, d) parameter to the (N, L, d) patch tokens with torch.cat, which raises at
batch > 1.  Every case with `cls_token=True` is therefore run ONE IMAGE AT A TIME: the outputs and image gradients are
stacked, the parameter gradients summed over the images (`per_image` = 1 in the fixture).  Cases without a class token run
batched.

Weights: the rule of tools/gen_golden_mlp_mixer.py -- oracle/filler.py, then +1.0 on every 1-D parameter whose name ends in
`weight` or `gamma`.  tests/vit_util.fill applies the same rule.  With it the attention scores of these cases have a standard
deviation near 1.0: neither uniform nor one-hot rows.

Floors (`floor/f32/...`, `floor/bf16/...`): the recipe of tools/gen_golden_mlp_mixer.py -- the reference in float32, and under
torch.autocast("cpu", bfloat16) with every module output rounded to bfloat16 by forward hooks, each against the reference in
float64, in the tests' clamped metric.

`zero_grad_keys`: the parameters whose float64 gradient has an rms below 1e-12.  The gradient of every `k_proj.bias` is
exactly zero in exact arithmetic: a constant added to every key shifts each row of scores by a constant, which softmax
ignores.  The module and trainer tests skip exactly these keys (and assert which they are); tests/test_attention_gpu.py
covers dK where it is not zero.  `grad_max` leaves them out.

The Flax fixture: filler values in both key layouts the reference's `load_flax_ckpt` reads (vision_transformer under
`vt/flax/<key>`, big_vision with the attention pooler under `bv/flax/<key>`) and the state_dicts it produces from them
(`vt/sd/<key>`, `bv/sd/<key>`).  `load_flax_ckpt` takes a checkpoint NAME and fetches it: here `torch_hub_download` in the
reference module's namespace is replaced by a function that returns the local temporary file, so nothing is fetched.

The resize fixture: `pe` before and after `resize_pe(16)` on ViT(32, 1, 1, 4, 8).
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

vit = gen_golden.ref_import("vision_toolbox.backbones.vit")
GOLDEN = ROOT / "tests" / "golden"

CASES = {  # name -> (constructor args (d_model, depth, n_heads, patch, img), constructor kwargs, batch)
    "a": ((64, 2, 2, 4, 16), {}, 3),  # L = 17: below one tile, class token, two heads of 32
    "b": ((64, 2, 1, 4, 32), {"cls_token": False, "pool_type": "gap"}, 2),  # L = 64: exactly one tile, head_dim 64
    "c": ((64, 1, 1, 4, 32), {"layer_scale_init": 0.5}, 2),  # L = 65: one key past a tile, LayerScale, class token
}
FLAX_ARGS = (32, 1, 1, 4, 8)
RESIZE_ARGS, RESIZE_TO = (32, 1, 1, 4, 8), 16


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


def score_std(m, x):
    """standard deviation of the first block's scaled attention scores (float64), for the record"""
    with torch.no_grad():
        t = m.patch_embed(x).flatten(2).transpose(1, 2) + m.pe
        if m.cls_token is not None:
            t = torch.cat([m.cls_token.expand(t.shape[0], -1, -1), t], 1)
        blk = m.layers[0]
        n, mha = blk.mha[0](t), blk.mha[1]
        q = mha.q_proj(n).unflatten(-1, (mha.n_heads, -1)).transpose(-2, -3)
        k = mha.k_proj(n).unflatten(-1, (mha.n_heads, -1)).transpose(-2, -3)
        s = mha.scale * q @ k.transpose(-1, -2)
        return float((s - s.mean(-1, keepdim=True)).std())


def flax_source(m, pre, big_vision):
    src = {}

    def put(key, shape):
        src[key] = filler.tensor(pre + key, tuple(shape)).numpy().copy()

    d, _, h, p, img = FLAX_ARGS
    T = (img // p) ** 2
    if big_vision:
        names = ("LayerNorm_0", "MultiHeadDotProductAttention_0", "LayerNorm_1", "MlpBlock_0")
        put("pos_embedding", (1, T, d))
    else:
        names = ("LayerNorm_0", "MultiHeadDotProductAttention_1", "LayerNorm_2", "MlpBlock_3")
        put("cls", (1, 1, d))
        put("Transformer/posembed_input/pos_embedding", (1, T + 1, d))
    put("embedding/kernel", (p, p, 3, d))
    put("embedding/bias", (d,))
    put("Transformer/encoder_norm/scale", (d,))
    put("Transformer/encoder_norm/bias", (d,))

    def put_mha(prefix):
        for what in ("query", "key", "value"):
            put(f"{prefix}/{what}/kernel", (d, h, d // h))
            put(f"{prefix}/{what}/bias", (h, d // h))
        put(f"{prefix}/out/kernel", (h, d // h, d))
        put(f"{prefix}/out/bias", (d,))

    def put_mlp(prefix, mlp):
        put(f"{prefix}/Dense_0/kernel", (d, mlp.linear1.out_features))
        put(f"{prefix}/Dense_0/bias", (mlp.linear1.out_features,))
        put(f"{prefix}/Dense_1/kernel", (mlp.linear1.out_features, d))
        put(f"{prefix}/Dense_1/bias", (d,))

    for i, layer in enumerate(m.layers):
        blk = f"Transformer/encoderblock_{i}"
        for ln in (names[0], names[2]):
            put(f"{blk}/{ln}/scale", (d,))
            put(f"{blk}/{ln}/bias", (d,))
        put_mha(f"{blk}/{names[1]}")
        put_mlp(f"{blk}/{names[3]}", layer.mlp[1])
    if big_vision:
        put("MAPHead_0/probe", (1, 1, d))
        put_mha("MAPHead_0/MultiHeadDotProductAttention_0")
        put("MAPHead_0/LayerNorm_0/scale", (d,))
        put("MAPHead_0/LayerNorm_0/bias", (d,))
        put_mlp("MAPHead_0/MlpBlock_0", m.pooler.mlp)
    return src


def flax_fixture():
    out = {"args": np.array(FLAX_ARGS)}
    for tag, big_vision, kw in (("vt", False, {}), ("bv", True, {"cls_token": False, "pool_type": "mha"})):
        m = vit.ViT(*FLAX_ARGS, **kw)
        src = flax_source(m, f"vit_flax.{tag}.", big_vision)
        with tempfile.TemporaryDirectory() as td:
            path = str(Path(td) / "ckpt.npz")
            np.savez(path, **src)
            fetch = vit.torch_hub_download
            vit.torch_hub_download = lambda url, *a, **k: path  # the local file: nothing is fetched
            try:
                m.load_flax_ckpt("local.npz", big_vision=big_vision)
            finally:
                vit.torch_hub_download = fetch
        for k, v in src.items():
            out[f"{tag}/flax/{k}"] = v
        for k, v in m.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.numpy().copy()
    path = GOLDEN / "vit_flax.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")


def resize_fixture():
    m = vit.ViT(*RESIZE_ARGS)
    fill(m, "vit_resize.")
    before = m.pe.detach().numpy().copy()
    m.resize_pe(RESIZE_TO)
    path = GOLDEN / "vit_resize.npz"
    np.savez_compressed(path, args=np.array(RESIZE_ARGS), size=np.array(RESIZE_TO), recipe=np.array(["vit_resize."]),
                        pe_before=before, pe_after=m.pe.detach().numpy().copy())
    print(f"wrote {path} ({path.stat().st_size // 1024} KB)")


def main():
    for name, (args, kw, B) in CASES.items():
        pre = f"vit_{name}."
        m = vit.ViT(*args, **kw)
        fill(m, pre)
        m.eval()
        S = args[4]
        per_image = m.cls_token is not None
        x = filler.tensor(pre + "x", (B, 3, S, S))
        r = filler.tensor(pre + "r", (B, args[0]))
        res32 = run(m, x, r, per_image)
        res16 = run(m, x, r, per_image, autocast=True)
        res64 = run(m.double(), x.double(), r.double(), per_image)
        print(name, f"attention score std (block 0, float64) {score_std(m, x.double()):.3f}")
        m.float()
        zero = sorted(k[5:] for k, v in res64.items()
                      if k.startswith("grad/") and float(v.norm()) / v.numel() ** 0.5 < 1e-12)
        out = {
            "keys": np.array(list(m.state_dict().keys())),
            "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()]),
            "recipe": np.array([pre, pre + "x", pre + "r"]),
            "x_shape": np.array([B, 3, S, S]),
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
        print(name, "float64 rms of the zero gradients",
              [f"{float(res64['grad/' + k].norm()) / res64['grad/' + k].numel() ** 0.5:.1e}" for k in zero])
        path = GOLDEN / f"vit_{name}.npz"
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({path.stat().st_size // 1024} KB, {len(out)} arrays)")
    flax_fixture()
    resize_fixture()


if __name__ == "__main__":
    main()
