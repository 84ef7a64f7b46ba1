"""SHA-256 digests of compiled launch lists, one line per case: evidence that a change to the launch-list builder
(vision_toolbox/engine.py) leaves every program byte-for-byte as it was.

A compiled program is two flat arrays of vt_op structs (base ids and byte offsets, never pointers) plus a few sizes, so
its bytes are the same from process to process.  Run this file on two trees and `diff` the outputs:

    python tools/program_digest.py > digests.txt        (needs the built library, no GPU)

Only entry points that have existed since the module API and the fused trainer were written are used: a module's
`_vt_runner().program(...)`, a neck's runner `.program(...)`, `TrainStep(..., device="cpu", plan_only=True)` and its
validation program.  The Builder reads its switches in __init__, so every case sets os.environ for itself; VT_PW_MIN_MB is
unset unless the case says otherwise.  The data-parallel plans need a process group and run in a child process (one-rank
gloo group).
"""
import ctypes
import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT), str(ROOT / "tests")]
import torch  # noqa: E402
from vision_toolbox import _native as N  # noqa: E402
from vision_toolbox import backbones, necks  # noqa: E402
from vision_toolbox.backbones import MLPMixer  # noqa: E402
from vision_toolbox.components import ConvNormAct  # noqa: E402
from vision_toolbox.trainer import TrainStep  # noqa: E402

SWITCHES = ("VT_DETERMINISTIC", "VT_PW_MIN_MB", "VT_WGRAD_GROUP", "VT_WGRAD_GROUP_1X1", "VT_WGRAD_INLINE", "VT_FUSE_BNRED",
            "VT_BN_BWD_FUSED", "VT_BN_FIN_APPLY")
DTYPES = (("f32", N.VT_F32, torch.float32), ("bf16", N.VT_BF16, torch.bfloat16))
CPU = torch.device("cpu")


def set_env(env: dict) -> None:
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def _ops_bytes(arr, n: int) -> bytes:
    return ctypes.string_at(ctypes.addressof(arr), n * ctypes.sizeof(N.Op)) if n else b""


def program_digest(prog, store, extra=()) -> str:
    h = hashlib.sha256()
    h.update(_ops_bytes(prog.fwd_ops, prog.n_fwd))
    h.update(_ops_bytes(prog.bwd_ops, prog.n_bwd))
    meta = [prog.n_fwd, prog.n_bwd, prog.arena_bytes, prog.zf_off, prog.zf_bytes, prog.zb_off, prog.zb_bytes, prog.n_units]
    meta.append([(t.B, t.H, t.W, t.C, t.ld, t.coff, t.buf.offset) for t in prog.outs])
    meta.append(sorted((k, t.buf.offset, t.C, t.ld) for k, t in prog.builder.debug_refs.items()))
    meta.append([prog.param_grad_off.get(id(p)) for p in store.params])
    meta.append(list(extra))
    h.update(repr(meta).encode())
    return h.hexdigest()


def report(label: str, fn) -> None:
    try:
        print(f"{label} {fn()}", flush=True)
    except Exception as e:  # a case that raises must raise the same way on both trees
        print(f"{label} RAISES {type(e).__name__}: {e}", flush=True)


# -- module programs -----------------------------------------------------------------------------------------------------
MODES = (("train+grad", True, True, False), ("eval", False, False, False), ("train+grad+dx", True, True, True))


def module_cases(label, make, size, env=None, dtypes=DTYPES, modes=MODES, channels=3, prep=None):
    for dname, dt, _ in dtypes:
        for mname, training, need_grad, x_grad in modes:
            def run():
                set_env(env or {})
                m = make()
                m.train(training)
                if prep is not None:
                    prep(m)
                r = m._vt_runner()
                r.store.ensure(CPU)
                x = torch.zeros(2, channels, size, size, requires_grad=x_grad)
                return program_digest(r.program(x, dt, True, need_grad), r.store)

            tag = "".join(f" {k}={v}" for k, v in sorted((env or {}).items()))
            report(f"module {label} {dname} {mname}{tag}", run)


def convnext(name):
    import convnext_util

    return lambda: convnext_util.build(name)


def vit(name):
    import vit_util

    return lambda: vit_util.build(name)


def vit_size(name):
    import vit_util

    return vit_util.CASES[name][0][4]


def deit(name):
    import deit_util

    return lambda: deit_util.build(name)


def deit_size(name):
    import deit_util

    return deit_util.CASES[name][1][4]


def _freeze_norm(m):
    m.norm.eval()


def _freeze_weight(m):
    m.conv.weight.requires_grad_(False)


UNITS = [  # (label, constructor, input channels, prepare)
    ("groups2", lambda: ConvNormAct(16, 32, groups=2), 16, None),
    ("depthwise", lambda: ConvNormAct(16, 16, groups=16), 16, None),
    ("depthwise_nonorm_relu", lambda: ConvNormAct(16, 16, groups=16, norm="none", act="relu"), 16, None),
    ("depthwise_nonorm_none", lambda: ConvNormAct(16, 16, groups=16, norm="none", act="none"), 16, None),
    ("dil2_s2", lambda: ConvNormAct(16, 32, stride=2, dilation=2), 16, None),
    ("s2_32_64", lambda: ConvNormAct(32, 64, stride=2), 32, None),
    ("s2_64_256", lambda: ConvNormAct(64, 256, stride=2), 64, None),
    ("nonorm_relu", lambda: ConvNormAct(16, 32, norm="none", act="relu"), 16, None),
    ("nonorm_gelu", lambda: ConvNormAct(16, 32, norm="none", act="gelu"), 16, None),
    ("nonorm_none", lambda: ConvNormAct(16, 32, norm="none", act="none"), 16, None),
    ("leaky_relu", lambda: ConvNormAct(16, 32, act="leaky_relu"), 16, None),
    ("silu", lambda: ConvNormAct(16, 32, act="silu"), 16, None),
    ("gelu", lambda: ConvNormAct(16, 32, act="gelu"), 16, None),
    ("act_none", lambda: ConvNormAct(16, 32, act="none"), 16, None),
    ("frozen_norm", lambda: ConvNormAct(16, 32), 16, _freeze_norm),
    ("frozen_weight", lambda: ConvNormAct(16, 32), 16, _freeze_weight),
    ("k3_64_64", lambda: ConvNormAct(64, 64), 64, None),
    ("k1_32_64", lambda: ConvNormAct(32, 64, kernel_size=1), 32, None),
    ("k1_32_64_frozen_norm", lambda: ConvNormAct(32, 64, kernel_size=1), 32, _freeze_norm),
    ("stem_3_32", lambda: ConvNormAct(3, 32), 3, None),
]


def all_module_cases():
    for name in ("darknet19", "darknet53", "cspdarknet53", "darknet_yolov5n", "vovnet19_slim_ese", "vovnet39"):
        module_cases(name, getattr(backbones, name), 64)
        module_cases(name, getattr(backbones, name), 64, env={"VT_PW_MIN_MB": "0"}, dtypes=DTYPES[1:])
    for c in "abc":
        module_cases(f"convnext_{c}", convnext(c), 64)
    module_cases("mlp_mixer", lambda: MLPMixer(2, 32, 4, 20), 20)
    for c in "abc":  # (appended: the lines above keep their order)
        module_cases(f"vit_{c}", vit(c), vit_size(c))
    for c in "abc":
        module_cases(f"deit_{c}", deit(c), deit_size(c))
    for label, make, cin, prep in UNITS:
        module_cases(f"unit {label}", make, 16, channels=cin, prep=prep)
        module_cases(f"unit {label}", make, 16, channels=cin, prep=prep, env={"VT_PW_MIN_MB": "0"}, dtypes=DTYPES[1:])
    switches = [{"VT_PW_MIN_MB": "0"}, {}, {"VT_FUSE_BNRED": "1"}, {"VT_BN_BWD_FUSED": "1"}, {"VT_BN_FIN_APPLY": "0"},
                {"VT_WGRAD_GROUP": "1"}, {"VT_WGRAD_GROUP_1X1": "1"}, {"VT_WGRAD_INLINE": "1"}, {"VT_DETERMINISTIC": "1"}]
    for env in switches:
        module_cases("switch cspdarknet53", backbones.cspdarknet53, 64, env=env, dtypes=DTYPES[1:], modes=MODES[:1])
        if "VT_PW_MIN_MB" not in env:
            module_cases("switch cspdarknet53", backbones.cspdarknet53, 64, env=dict(env, VT_PW_MIN_MB="0"), dtypes=DTYPES[1:],
                         modes=MODES[:1])


# -- necks ---------------------------------------------------------------------------------------------------------------
def neck_cases():
    import test_necks

    for name in test_necks.CASES:
        _, ins, _, _, sizes, B, _, _ = test_necks._case(name)
        for dname, dt, tdt in DTYPES:
            for mname, training, need_grad, x_grad in (("train+grad+dx", True, True, True), ("train+grad", True, True, False),
                                                       ("eval", False, False, False)):
                def run():
                    set_env({})
                    m = test_necks._make(necks, name)
                    m.train(training)
                    r = necks._NeckRunner(m)
                    r.store.ensure(CPU)
                    xs = [torch.zeros(B, c, s, s, dtype=tdt, requires_grad=x_grad) for c, s in zip(ins, sizes)]
                    prog = r.program(xs, dt, need_grad)
                    grads = [None if g is None else (g.buf.offset, g.C, g.ld, g.coff) for g in prog.ext_grads]
                    return program_digest(prog, r.store, extra=grads)

                report(f"neck {name} {dname} {mname}", run)


# -- fused trainer plans ---------------------------------------------------------------------------------------------------
def plan_digest(ts) -> str:
    extra = [ctypes.string_at(ctypes.addressof(ts.opt_ops), ts.n_opt * ctypes.sizeof(N.Op)).hex(),
             bytes(ts.zero_ops).hex(), list(ts.bwd_cuts), [list(c) for c in ts.cut_buckets], list(ts.segments)]
    return program_digest(ts.prog, ts.store, extra=extra)


def plan_case(label, make, env=None, classes=16, batch=2, size=64, dtype=torch.bfloat16, validation=True, **kw):
    made = []

    def run():
        set_env(env or {})
        made.append(TrainStep(make(), classes, batch, size, dtype, device="cpu", plan_only=True, **kw))
        return plan_digest(made[0])

    def run_eval():  # the validation program of the same step (eval mode, forward only)
        made[0]._build_eval()
        return program_digest(made[0]._eval[0], made[0].store)

    report(f"plan {label}", run)
    if validation and made:
        report(f"plan-eval {label}", run_eval)


PLAN_VARIANTS = [("default", {}), ("deterministic", {"deterministic": True}), ("mix", {"mix": True}),
                 ("freeze_bn", {"freeze_bn": True}), ("adamw", {"optimizer": "AdamW"}), ("classes10", {"classes": 10}),
                 ("f32", {"dtype": torch.float32})]


def plan_cases():
    for name in ("cspdarknet53", "vovnet19_slim_ese"):
        for vname, kw in PLAN_VARIANTS:
            plan_case(f"{name} {vname}", getattr(backbones, name), **kw)
            plan_case(f"{name} {vname} VT_PW_MIN_MB=0", getattr(backbones, name), env={"VT_PW_MIN_MB": "0"}, **kw)
    for c in "abc":
        for dname, _, tdt in DTYPES:
            plan_case(f"convnext_{c} {dname} include_pool=False", convnext(c), classes=10, dtype=tdt, include_pool=False,
                      optimizer="AdamW")
    for dname, _, tdt in DTYPES:
        plan_case(f"mlp_mixer {dname} include_pool=False", lambda: MLPMixer(2, 32, 4, 20), classes=10, batch=3, size=20,
                  dtype=tdt, include_pool=False)
    plan_case("bench cspdarknet53 256@224 bf16", backbones.cspdarknet53, classes=1000, batch=256, size=224, lr=0.05,
              momentum=0.9, weight_decay=2e-5, label_smoothing=0.1, use_graphs=False, data_parallel=False, validation=False)


def dist_cases():
    """data-parallel plans over a one-rank gloo group (VT_DP_WORLD1=1); runs in a process of its own"""
    import torch.distributed as dist

    os.environ["VT_DP_WORLD1"] = "1"
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{tmp}/rendezvous", rank=0, world_size=1)
        try:
            for name in ("cspdarknet53", "vovnet19_slim_ese"):
                for vname, kw in (("sync_bn", {"sync_bn": True}), ("sync_bn rccl", {"sync_bn": True, "collectives": "rccl"}),
                                  ("rccl", {"collectives": "rccl"}), ("sharded", {"exchange": "sharded"}),
                                  ("allreduce", {})):
                    plan_case(f"dp {name} {vname}", getattr(backbones, name), bucket_mb=0.5, **kw)
                    plan_case(f"dp {name} {vname} VT_PW_MIN_MB=0", getattr(backbones, name), env={"VT_PW_MIN_MB": "0"},
                              bucket_mb=0.5, **kw)
        finally:
            dist.destroy_process_group()


if __name__ == "__main__":
    if sys.argv[1:] == ["--dist"]:
        dist_cases()
    else:
        all_module_cases()
        neck_cases()
        plan_cases()
        sys.stdout.flush()
        subprocess.run([sys.executable, __file__, "--dist"], check=True)
