"""Numbers for the "ResNet strikes back" pieces on the GPU (fails without one): python tools/bench_rsb.py [--out DIR] -> rsb_kernels.json

  passes  bf16, the two activation matrices of tools/bench_resnet.py -- (256*56*56, 256) and (256*7*7, 2048), the block ends of
          layer1 and layer4 of a ResNet-50 at batch 256, 224 px: the five keep passes (vt_bn_add_act_keep_*) beside the passes
          without keep on the SAME tensors, with a keep row that drops every tenth image (the others carry 1 / 0.9) and with a
          row of ones.  A dropped image's z is not read by the forward and the reduction, so `keep_drop` moves fewer bytes.
  loss    vt_sigmoid_bce beside vt_softmax_xent_mix at (256, 1000), bf16, mixup header, with gradient
  step    ResNet-50 at batch 128, 224 px, bf16: TrainStep(optimizer="Lamb", loss="bce", mix=True) with
          stochastic_depth=0.05 beside the same step with stochastic_depth=0 and beside loss="ce"

Timing as tools/bench_resnet.py: device events around windows of >= 0.3 s after 3 warm-up calls, 5 windows, the variants of a
group ALTERNATING window by window; median, min and max recorded.  Nothing is compared against a threshold."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tools")]

import torch  # noqa: E402

from bench_resnet import EPS, MOM, SHAPES, WINDOW_S, WINDOWS, _timed_group, vp  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402


def _passes(M, C, HW):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    torch.manual_seed(0)
    B = M // HW
    z = (torch.randn(M, C, device=dev) * 1.5 + 0.3).to(bf)
    r, dy = torch.randn(M, C, device=dev).to(bf), torch.randn(M, C, device=dev).to(bf)
    y, dz, dr = (torch.empty(M, C, device=dev, dtype=bf) for _ in range(3))
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    coef, bcoef = torch.zeros(4, C, device=dev), torch.zeros(3, C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    stats, sums = N.stats_buffer(C), N.stats_buffer(C)
    zz = z.float().double()
    for rep, idx in enumerate(torch.chunk(torch.arange(M, device=dev), N.VT_STAT_REPLICAS)):
        N.stats_encode(stats, 0, zz[idx].sum(0), rep)
        N.stats_encode(stats, 1, (zz[idx] ** 2).sum(0), rep)
    del zz
    N.check(lib.vt_bn_finalize(vp(stats), C, float(M), vp(gamma), vp(beta), EPS, MOM, None, None, None, vp(coef[0]), vp(coef[1]),
                               vp(coef[2]), vp(coef[3]), s()))
    keeps = {"keep_ones": torch.ones(B, device=dev), "keep_drop": torch.full((B,), 1.0 / 0.9, device=dev)}
    keeps["keep_drop"][::10] = 0.0
    fin = lambda: (vp(stats), C, float(M), vp(gamma), vp(beta), EPS, MOM, vp(rm), vp(rv), vp(nbt), vp(coef[0]), vp(coef[1]),  # noqa: E731
                   vp(coef[2]), vp(coef[3]), vp(z), C, vp(r), C, vp(y), C)
    bfin = lambda: (vp(sums), C, float(M), 1.0, vp(coef[0]), vp(coef[2]), vp(coef[3]), 1, vp(dg), vp(db), vp(bcoef), vp(dy), C, vp(y),  # noqa: E731
                    C, vp(z), C, vp(dz), C, vp(dr), C, 0)
    groups = {
        "fwd": {"plain": lambda: N.check(lib.vt_bn_add_act_apply(vp(z), C, vp(coef[0]), vp(coef[1]), vp(r), C, vp(y), C, M, C, dt, s()))},
        "fwd_fin": {"plain": lambda: N.check(lib.vt_bn_add_act_finalize_apply(*fin(), M, dt, s()))},
        "bwd_reduce": {"plain": lambda: N.check(lib.vt_bn_add_act_bwd_reduce(vp(dy), C, vp(y), C, vp(z), C, vp(coef[2]), vp(coef[3]), M, C,
                                                                             dt, vp(sums), s()))},
        "bwd_apply": {"plain": lambda: N.check(lib.vt_bn_add_act_bwd_apply(vp(dy), C, vp(y), C, vp(z), C, vp(bcoef), vp(dz), C, vp(dr), C,
                                                                           0, M, C, dt, s()))},
        "bwd_fin": {"plain": lambda: N.check(lib.vt_bn_add_act_bwd_finalize_apply(*bfin(), M, dt, s()))},
    }
    for name, k in keeps.items():
        groups["fwd"][name] = lambda k=k: N.check(lib.vt_bn_add_act_keep_apply(vp(z), C, vp(coef[0]), vp(coef[1]), vp(r), C, vp(y), C,
                                                                               vp(k), HW, M, C, dt, s()))
        groups["fwd_fin"][name] = lambda k=k: N.check(lib.vt_bn_add_act_keep_finalize_apply(*fin(), vp(k), HW, M, dt, s()))
        groups["bwd_reduce"][name] = lambda k=k: N.check(lib.vt_bn_add_act_keep_bwd_reduce(vp(dy), C, vp(y), C, vp(z), C, vp(coef[2]),
                                                                                           vp(coef[3]), vp(k), HW, M, C, dt, vp(sums), s()))
        groups["bwd_apply"][name] = lambda k=k: N.check(lib.vt_bn_add_act_keep_bwd_apply(vp(dy), C, vp(y), C, vp(z), C, vp(bcoef), vp(dz),
                                                                                         C, vp(dr), C, 0, vp(k), HW, M, C, dt, s()))
        groups["bwd_fin"][name] = lambda k=k: N.check(lib.vt_bn_add_act_keep_bwd_finalize_apply(*bfin(), vp(k), HW, M, dt, s()))
    groups["fwd"]["plain"](), groups["bwd_reduce"]["plain"](), groups["bwd_fin"]["plain"]()  # (y and the coefficients exist)
    torch.cuda.synchronize()
    row = {"M": M, "C": C, "HW": HW, "dtype": "bf16"}
    for g, fns in groups.items():
        res = _timed_group(fns)
        for name in keeps:
            res[name]["ratio_to_plain"] = res[name]["ms_median"] / res["plain"]["ms_median"]
        row[g] = res
    return row


def _loss(B=256, Ncls=1000):
    lib, dev, bf, dt = N.lib(), torch.device("cuda"), torch.bfloat16, N.VT_BF16
    s = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    torch.manual_seed(0)
    x = (torch.randn(B, Ncls, device=dev) * 3).to(bf)
    y = torch.randint(0, Ncls, (B,), device=dev)
    dl = torch.empty(B, Ncls, device=dev, dtype=bf)
    loss = torch.zeros(1, device=dev)
    rows = torch.zeros(B, dtype=torch.float64, device=dev)
    mix = torch.tensor([1.0, 0.3, 0, 0, 0, 0, 0, 0], device=dev)
    fns = {
        "sigmoid_bce": lambda: N.check(lib.vt_sigmoid_bce(vp(x), Ncls, vp(y), 0.1, 1.0 / B, vp(loss), vp(dl), Ncls, B, Ncls, dt, vp(mix), 0,
                                                          0.0, vp(rows), s())),
        "softmax_xent_mix": lambda: N.check(lib.vt_softmax_xent_mix(vp(x), Ncls, vp(y), 0.1, 1.0 / B, vp(loss), vp(dl), Ncls, B, Ncls, dt,
                                                                    vp(mix), s())),
    }
    res = _timed_group(fns)
    res["sigmoid_bce"]["ratio_to_xent"] = res["sigmoid_bce"]["ms_median"] / res["softmax_xent_mix"]["ms_median"]
    return {"B": B, "N": Ncls, "dtype": "bf16", "launches": {"sigmoid_bce": 2, "softmax_xent_mix": 1}, **res}


def _step(batch=128, size=224):
    from vision_toolbox.backbones import ResNetExtractor
    from vision_toolbox.trainer import TrainStep

    torch.manual_seed(0)
    x, y = torch.rand(batch, 3, size, size, device="cuda"), torch.randint(0, 1000, (batch,), device="cuda")
    steps = {}
    for name, sd, loss in (("recipe", 0.05, "bce"), ("no_stochastic_depth", 0.0, "bce"), ("cross_entropy", 0.05, "ce")):
        ts = TrainStep(ResNetExtractor("resnet50", stochastic_depth=sd), 1000, batch, size, torch.bfloat16, lr=5e-3, weight_decay=0.02,
                       optimizer="Lamb", eps=1e-6, loss=loss, mix=True, device="cuda")
        ts.set_mix("mixup", 0.3)
        ts.images.copy_(x)
        ts.labels.copy_(y)
        steps[name] = ts
    res = _timed_group({k: ts.step for k, ts in steps.items()})
    for k, r in res.items():
        r["images_per_s"] = batch / r["ms_median"] * 1e3
    res["losses"] = {k: ts.loss() for k, ts in steps.items()}
    return {"model": "resnet50", "batch": batch, "size": size, "dtype": "bf16", "optimizer": "Lamb", **res}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_rsb.py needs a GPU: nothing is measured without one")
    out = {"window_s": WINDOW_S, "windows": WINDOWS, "passes": []}
    for (M, C), HW in zip(SHAPES, (56 * 56, 7 * 7)):
        out["passes"].append(_passes(M, C, HW))
        print(json.dumps(out["passes"][-1]), flush=True)
    out["loss"] = _loss()
    print(json.dumps(out["loss"]), flush=True)
    if not a.skip_step:
        out["step"] = _step()
        print(json.dumps(out["step"]), flush=True)
    Path(a.out).mkdir(parents=True, exist_ok=True)
    (Path(a.out) / "rsb_kernels.json").write_text(json.dumps(out, indent=1))
