"""Fused ImageNet-classifier train step on one MI355X, data-parallel over RCCL.

What the reference does through Lightning (classifier.py:58-64 model assembly, :83-95
training_step, :111-169 three-group SGD, configs/base.yaml:16-23 DDP) is here ONE static
program per rank:

    images -> backbone -> global avg-pool -> linear head -> label-smoothing CE
              (include_pool=False, ConvNeXt / MLPMixer / ViT / SwinTransformer: the backbone's own pooled + normalised (B, C) output -> linear head)
           -> explicit backward into a persistent flat f32 gradient buffer
           -> bucketed gradient all-reduce (RCCL over xGMI); each bucket is issued as soon
              as the backward segment that completes it has been enqueued
           -> the optimiser over the flat buffers, which also refreshes the bf16 weights: SGD(momentum), or
              AdamW / Adam / Lamb (optimizer=...; the step count lives on the device, see _emit_opt), optionally behind
              a clip of the global gradient norm (clip_grad_norm=...; the norm is formed on the device, see _emit_opt)

The step is one launch list cut into segments at the bucket boundaries; every segment runs
through the native executor on two streams (main + filter-gradient side stream, left open
across segments so N > 1 keeps the N = 1 schedule; the bucket all-reduce is issued with the
side stream current).  hipGraph replay of the same segments is OPT-IN (use_graphs=True): it
measured 6 % slower than eager two-stream execution (21.2 against 20.0 ms) and one replay
ended in a host fault inside hipGraphLaunch that five re-runs did not reproduce (NOTEBOOK
R5.18, R6.1), so the default entry never goes through it.  BatchNorm uses per-rank batch statistics by
default; sync_bn=True gives the reference recipe's SyncBatchNorm (configs/base.yaml:22) at the
cost of 134 small collectives per step.

collectives="rccl" (round 4): the library's own RCCL communicator (vt_comm_init) instead of
torch.distributed -- the statistics exchanges and the bucket all-reduces are ops of the launch
lists (VT_OP_STAT_SYNC, VT_OP_ALLREDUCE), a step is three host calls for any world size, and a
SyncBatchNorm exchange stays on the stream of the kernels around it.
"""
from __future__ import annotations

import ctypes
import os
import math
from typing import Optional

import torch
from torch import nn

from . import _native as N
from . import engine as E
from .distributed import GradBucketer, ShardedExchange, plan_buckets
from .program import Program, current_stream_handle, draw_keep_factors

_NORMS = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.LayerNorm, nn.GroupNorm)
GROUP_NORM, GROUP_BIAS, GROUP_OTHER = 0, 1, 2  # flat-buffer order: small, late-produced groups first
# classifier.py:46,157-169 takes the name.  RMSprop is not built; of the timm names (classifier.py:165) only Lamb is
OPTIMIZERS = ("SGD", "AdamW", "Adam", "Lamb")
# the training loss: softmax cross-entropy (classifier.py:92), or binary cross-entropy on the same targets (vt_sigmoid_bce)
LOSSES = ("ce", "bce")
# HYPER buffer (16 floats): [0..3] learning rate; [4] optimiser step count t (int32 bits), [5] 1 - beta1^t,
# [6] sqrt(1 - beta2^t), [7] free (vt_adam_tick / vt_adamw); [8..15] MixUp / CutMix block
HYPER_STEP = 4
# OPTWS buffer (clip_grad_norm / Lamb only), in bytes: the control floats of vt_clip_coef (thresholds in, factor and norm
# out: N.VT_CTL_*), then the double partials of the gradient's sum of squares, then LAMB's partials and work table
OPTWS_CTL_BYTES = 64


def param_groups(model: nn.Module) -> dict:
    """id(param) -> group, the split of classifier.py:111-155 (norm / bias / everything else)."""
    out = {}
    for mod in model.modules():
        for name, p in mod._parameters.items():
            if p is None:
                continue
            if isinstance(mod, _NORMS):
                g = GROUP_NORM
            elif isinstance(mod, (nn.Linear, nn.modules.conv._ConvNd)) and name == "bias":
                g = GROUP_BIAS
            else:
                g = GROUP_OTHER
            out[id(p)] = g
    return out


def warmup_cosine_lr(epoch: int, max_epochs: int, lr: float, warmup_epochs: int = 5, warmup_factor: float = 0.01,
                     decay_factor: float = 0.0) -> float:
    """LinearLR warm-up then CosineAnnealingLR, stepped per epoch (classifier.py:171-190)."""
    if warmup_epochs > 0 and epoch < warmup_epochs:
        return lr * (warmup_factor + (1 - warmup_factor) * epoch / warmup_epochs)
    t, T = epoch - warmup_epochs, max(max_epochs - warmup_epochs, 1)
    eta_min = lr * decay_factor
    return eta_min + (lr - eta_min) * (1 + math.cos(math.pi * t / T)) / 2


def sample_mix(cutmix_alpha: float, mixup_alpha: float, width: int, height: int):
    """Draw (mode, lambda, box) the way RandomCutMixMixUp.forward does (extras.py:96-109), with the
    same torch CPU RNG calls in the same order, so a seeded run pairs with the reference's:
    rand -> choose; then RandomMixup (extras.py:29,37) or RandomCutmix (extras.py:64,72-88)."""
    import math as _m

    if cutmix_alpha == 0 and mixup_alpha == 0:
        raise ValueError
    use_mixup = cutmix_alpha <= 0 or torch.rand(1).item() >= 0.5
    if use_mixup:
        if torch.rand(1).item() >= 1.0:  # p = 1: never taken, but the draw is part of the stream
            return "none", 1.0, (0, 0, 0, 0)
        lam = float(torch._sample_dirichlet(torch.tensor([mixup_alpha, mixup_alpha], dtype=torch.float32))[0])
        return "mixup", lam, (0, 0, 0, 0)
    if torch.rand(1).item() >= 1.0:
        return "none", 1.0, (0, 0, 0, 0)
    lam = float(torch._sample_dirichlet(torch.tensor([cutmix_alpha, cutmix_alpha], dtype=torch.float32))[0])
    r_x = int(torch.randint(width, (1,)))
    r_y = int(torch.randint(height, (1,)))
    r = 0.5 * _m.sqrt(1.0 - lam)
    r_w_half, r_h_half = int(r * width), int(r * height)
    x1, y1 = max(r_x - r_w_half, 0), max(r_y - r_h_half, 0)
    x2, y2 = min(r_x + r_w_half, width), min(r_y + r_h_half, height)
    lam = float(1.0 - (x2 - x1) * (y2 - y1) / (width * height))
    return "cutmix", lam, (x1, y1, x2, y2)


def reduce_validation_sums(sums: torch.Tensor, group=None) -> torch.Tensor:
    """[loss sum, top-1 hits, rows] of this rank's batch -> the same three sums over all ranks of `group` (one scalar-sized
    all-reduce: the `sync_dist=True` of classifier.py:104; SURVEY collective C4).  Without a process group: unchanged."""
    if group is None and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return sums
    if torch.distributed.get_world_size(group) == 1:
        return sums
    t = sums.double()  # (hits and rows are integers: exact in any order)
    if torch.distributed.get_backend(group) != "nccl":
        t = t.cpu()
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM, group=group)
    return t.to(sums.device, torch.float32)


def _grad_write_offsets(op: N.Op) -> list[int]:
    """element offsets in the flat gradient buffer this backward op writes."""
    return [op.ptr[k].offset // 4 for k in range(N.VT_OP_MAX_PTR) if op.ptr[k].base == E.GRADS]


class TrainStep:
    def __init__(
        self,
        backbone: nn.Module,
        num_classes: int = 1000,
        batch_size: int = 256,  # per rank
        image_size: int = 224,
        dtype: torch.dtype = torch.bfloat16,
        lr: float = 0.05,
        momentum: float = 0.9,
        weight_decay: float = 2e-5,
        norm_weight_decay: float = 0.0,
        bias_weight_decay: float = 0.0,
        label_smoothing: float = 0.1,
        device: Optional[torch.device] = None,
        process_group=None,
        bucket_mb: float = 16.0,
        use_graphs: bool = False,  # opt-in: slower than the two-stream executor, see the module docstring
        plan_only: bool = False,
        sync_bn: bool = False,
        mix: bool = False,
        freeze_bn: bool = False,
        deterministic: Optional[bool] = None,
        exchange: str = "allreduce",
        head_bucket_kb: float = 256.0,
        data_parallel: Optional[bool] = None,
        collectives: str = "torch",
        optimizer: str = "SGD",
        betas: "tuple[float, float]" = (0.9, 0.999),
        eps: float = 1e-8,
        include_pool: bool = True,
        drop_seed: int = 0,
        clip_grad_norm: Optional[float] = None,
        lamb_max_grad_norm: Optional[float] = 1.0,
        trust_clip: bool = False,
        always_adapt: bool = False,
        loss: str = "ce",
        bce_target_threshold: Optional[float] = None,
        bce_sum_classes: bool = False,
        ema_decay: Optional[float] = None,
        ema_steps: int = 1,
        accumulate_grad_batches: int = 1,
    ):
        """optimizer="Lamb": LAMB in the form of timm.optim.Lamb(bias_correction=True, grad_averaging=True) as
        include/vt_amd.h states it (timm is no dependency; that statement is the definition).  `lamb_max_grad_norm`,
        `trust_clip` and `always_adapt` are timm's `max_grad_norm`, `trust_clip` and `always_adapt`; timm's default
        `eps` is 1e-6, while the `eps` argument here keeps torch.optim.Adam's 1e-8 as its default -- pass eps=1e-6 for
        timm's recipe.
        clip_grad_norm=C (any optimiser): the averaged gradient is scaled by min(1, C / (norm + 1e-6)) before the optimiser
        sees it, as torch.nn.utils.clip_grad_norm_ (Lightning's gradient_clip_val, "norm" algorithm) does.  None builds
        today's launch lists; float("inf") builds the clipping ops with a factor of exactly 1 / world.  The thresholds
        live on the device: set_clip_grad_norm changes C under a captured graph, last_grad_norm reads the norm back.
        loss="bce": binary cross-entropy against the smoothed (and, with `mix`, mixed) one-hot target, as include/vt_amd.h
        states it (timm.loss.BinaryCrossEntropy behind timm's Mixup; that statement is the definition).
        `bce_target_threshold` and `bce_sum_classes` are timm's `target_threshold` and `sum_classes`.  The loss is a
        fixed-order sum: loss() is bit-identical from run to run.  validate() keeps plain cross-entropy.
        ema_decay=d: an exponential moving average of the weights and BatchNorm statistics as include/vt_amd.h states it
        (torchvision's ExponentialMovingAverage / timm's ModelEmaV2; that statement is the definition), kept in shadow
        buffers by launches at the end of the optimiser list: optimiser steps 0, ema_steps, 2 * ema_steps, .. update it
        (the first update is a copy).  validate(ema=True) scores the average, ema_state_dict() exports it.  Warm-up
        schedules of the decay are the caller's: set_ema_decay changes it under a captured graph.
        accumulate_grad_batches=k: step() stays one forward + backward over one micro-batch of `batch_size`; the gradient
        exchange and the optimiser run on every k-th call, over the mean of the k micro-batch gradients (Lightning's
        accumulate_grad_batches; the calls in between are DDP's no_sync).  steps_done, opt_steps(), the Adam step count
        and the EMA count are optimiser steps; micro_steps_done counts calls."""
        N.lib()
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay={ema_decay!r}: None or a decay in [0, 1)")
        if isinstance(ema_steps, bool) or int(ema_steps) != ema_steps or ema_steps < 1:
            raise ValueError(f"ema_steps={ema_steps!r}: a whole number of optimiser steps >= 1")
        if isinstance(accumulate_grad_batches, bool) or int(accumulate_grad_batches) != accumulate_grad_batches \
                or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches={accumulate_grad_batches!r}: a whole number of micro-batches >= 1")
        if exchange == "sharded" and ema_decay is not None:
            raise NotImplementedError("exchange='sharded' with ema_decay: a rank owns slices of the flat parameter buffer, the "
                                      "average would be formed from stale slices unless the weights were gathered in f32 first; "
                                      "use exchange='allreduce'")
        self._ema_on, self._ema_steps = ema_decay is not None, int(ema_steps)
        self.ema_decay = None  # (set_ema_decay keeps the current value here)
        self._accum = int(accumulate_grad_batches)
        if loss not in LOSSES:
            raise ValueError(f"loss={loss!r}: supported are {', '.join(LOSSES)}")
        if loss != "bce" and (bce_target_threshold is not None or bce_sum_classes):
            raise ValueError(f"bce_target_threshold / bce_sum_classes belong to loss='bce', not to loss={loss!r}")
        if bce_target_threshold is not None and not math.isfinite(float(bce_target_threshold)):
            raise ValueError(f"bce_target_threshold={bce_target_threshold!r}: None or a finite number")
        self.loss_name = loss
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer={optimizer!r}: supported are {', '.join(OPTIMIZERS)}")
        self.optimizer, self._betas, self._eps = optimizer, (float(betas[0]), float(betas[1])), float(eps)
        self._adam = optimizer != "SGD"  # the Adam family keeps m, v and the device step count: AdamW, Adam, Lamb
        self._lamb = optimizer == "Lamb"
        for name, val in (("clip_grad_norm", clip_grad_norm), ("lamb_max_grad_norm", lamb_max_grad_norm)):
            if val is not None and not float(val) >= 0.0:
                raise ValueError(f"{name}={val!r}: a threshold is None or >= 0 (0 or inf: built, but off)")
        self._clip = clip_grad_norm is not None or self._lamb  # the list carries GRAD_SUMSQ / CLIP_COEF
        self._clip_user = clip_grad_norm is not None
        self._lamb_flags = (N.VT_LAMB_TRUST_CLIP if trust_clip else 0) | (N.VT_LAMB_ALWAYS_ADAPT if always_adapt else 0)
        if exchange == "sharded" and self._clip:
            raise NotImplementedError("exchange='sharded' with optimizer='Lamb' or clip_grad_norm: a rank owns slices of the "
                                      "flat buffers, not whole tensors or the whole gradient, and the norms are per tensor / "
                                      "global; use exchange='allreduce'")
        self.include_pool = bool(include_pool)
        if not self.include_pool:
            from .backbones.cait import CaiT
            from .backbones.convnext import ConvNeXt
            from .backbones.mlp_mixer import MLPMixer
            from .backbones.patchconvnet import PatchConvNet
            from .backbones.swin import SwinTransformer
            from .backbones.vit import ViT

            # classifier.py:59-63 with include_pool=False is nn.Sequential(backbone, nn.Linear): right only where
            # forward() already returns the pooled (B, C) vector; a map-returning family would feed nn.Linear a 4-D map
            if not isinstance(backbone, (ConvNeXt, MLPMixer, ViT, SwinTransformer, CaiT, PatchConvNet)):
                raise ValueError(f"include_pool=False needs a backbone whose forward returns (B, C) (ConvNeXt, MLPMixer, ViT, "
                                 f"SwinTransformer, CaiT, PatchConvNet); "
                                 f"{type(backbone).__name__} returns a feature map")
        self.device = torch.device(device if device is not None else "cuda")
        self.plan_only = plan_only  # build launch lists / bucket plan without a GPU (host-logic tests)
        if self.device.type != "cuda" and not plan_only:
            raise RuntimeError("TrainStep runs on the GPU only (no CPU fallback)")
        self.B, self.S = batch_size, image_size
        self.dtype = N.VT_BF16 if dtype == torch.bfloat16 else N.VT_F32
        self.pg = process_group
        self.world = 1
        # data_parallel=False: this rank's program alone, whatever process group exists (bench.py times the N = 1
        # denominator of a weak-scaling run on rank 0 of the same job)
        if data_parallel is not False and torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size(process_group)
        # a one-rank process group still takes the data-parallel schedule (cut lists, bucket collectives on the
        # filter-gradient stream, broadcasts): how the RCCL path is exercised on a one-GPU box (tests)
        self.dp = data_parallel is not False and (
            self.world > 1 or (os.environ.get("VT_DP_WORLD1", "0") != "0" and torch.distributed.is_available()
                               and torch.distributed.is_initialized()))
        # (measurement only, set through the `exchange_skipped()` context manager, which restores the replicas' state)
        self._skip_exchange = False
        head = nn.Linear(backbone.get_last_out_channels(), num_classes)
        if self.include_pool:
            self.model = nn.Sequential(backbone, nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), head)
        else:
            self.model = nn.Sequential(backbone, head)
        self.model.train()
        if freeze_bn:
            # fine-tuning with frozen BatchNorm: every unit normalises with its running statistics (constants
            # in backward) and leaves them untouched, like `bn.eval()` inside a training model
            for m in self.model.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()

        groups = param_groups(self.model)
        self.store = st = E.ParamStore(self.model, order_key=lambda p: groups[id(p)])
        # the kernels address channels in 16-byte chunks: a class count that is no multiple of one (10 classes) runs as
        # the next wider head over zero rows, which stay zero -- the loss reads `num_classes` columns and hands the
        # others a zero gradient, and every optimiser here maps (p, g, state) = 0 to 0
        self.num_classes = num_classes
        self._head_rows = E._round_up(num_classes, E._EPC[self.dtype])
        if self._head_rows != num_classes:
            st.reserve[id(head.weight)] = self._head_rows * head.in_features
            st.reserve[id(head.bias)] = self._head_rows
        # gradient exchange: "allreduce" = one f32 all-reduce per bucket, every rank runs the whole optimiser;
        # "sharded" = reduce-scatter -> SGD on the rank's slice of every bucket -> all-gather of the bf16 weights
        if exchange not in ("allreduce", "sharded"):
            raise ValueError(exchange)
        self.exchange = exchange if self.dp else "allreduce"
        if self.exchange == "sharded":
            from .backbones.convnext import ConvNeXt

            # the sharded exchange refreshes the bf16 mirror of the slices other ranks own, and f32 only for the head bucket
            # (BatchNorm parameters, biases); a ConvNeXt's layer scales and depthwise filters are read as f32 masters and
            # lie in the weight-decay group behind it: they would go stale on every rank but their owner
            if isinstance(backbone, ConvNeXt):
                raise NotImplementedError("exchange='sharded' with a ConvNeXt: its layer scales and depthwise filters are read "
                                          "in f32 outside the head bucket (use exchange='allreduce')")
            from .backbones.vit import ViT

            # (the same holds for a ViT's position embedding, class token and layer scales)
            if isinstance(backbone, ViT):
                raise NotImplementedError("exchange='sharded' with a ViT: its position embedding, class token and layer scales "
                                          "are read in f32 outside the head bucket (use exchange='allreduce')")
            from .backbones.swin import SwinTransformer

            # (... and for a Swin's relative-position tables and layer scales)
            if isinstance(backbone, SwinTransformer):
                raise NotImplementedError("exchange='sharded' with a SwinTransformer: its relative-position tables and layer "
                                          "scales are read in f32 outside the head bucket (use exchange='allreduce')")
            from .backbones.cait import CaiT

            # (... and for a CaiT's position embedding, class token, layer scales and head-mixing weights)
            if isinstance(backbone, CaiT):
                raise NotImplementedError("exchange='sharded' with a CaiT: its position embedding, class token, layer scales and "
                                          "talking-heads weights are read in f32 outside the head bucket (use "
                                          "exchange='allreduce')")
            from .backbones.patchconvnet import PatchConvNet

            # (... and for a PatchConvNet's depthwise filters, class token and layer scales)
            if isinstance(backbone, PatchConvNet):
                raise NotImplementedError("exchange='sharded' with a PatchConvNet: its depthwise filters, class token and layer "
                                          "scales are read in f32 outside the head bucket (use exchange='allreduce')")
            from .backbones.regnet import RegNetExtractor

            # (... and for the Squeeze-Excitation weights of a RegNetY, which vt_se_mlp_fwd reads as f32 masters)
            if isinstance(backbone, RegNetExtractor) and backbone.se_ratio:
                raise NotImplementedError(f"exchange='sharded' with {backbone.model_name}: its Squeeze-Excitation weights are "
                                          "read in f32 outside the head bucket (use exchange='allreduce')")
            from .backbones.mobilenet import MobileNetExtractor

            # (... and for the depthwise filters and Squeeze-Excitation weights of a MobileNet, which vt_dwt_* and vt_se_mlp_fwd
            #  read as f32 masters)
            if isinstance(backbone, MobileNetExtractor):
                raise NotImplementedError(f"exchange='sharded' with {backbone.model_name}: its depthwise filters and "
                                          "Squeeze-Excitation weights are read in f32 outside the head bucket (use "
                                          "exchange='allreduce')")
            from .backbones.efficientnet import EfficientNetExtractor

            # (... and for those of an EfficientNet)
            if isinstance(backbone, EfficientNetExtractor):
                raise NotImplementedError(f"exchange='sharded' with {backbone.model_name}: its depthwise filters and "
                                          "Squeeze-Excitation weights are read in f32 outside the head bucket (use "
                                          "exchange='allreduce')")
        # who issues the collectives: "torch" = torch.distributed calls between segments of the launch lists (any
        # backend: gloo in the CPU tests); "rccl" = the library's own RCCL communicator (vt_comm_init), the collectives are
        # OPS of the lists (VT_OP_STAT_SYNC in front of every BatchNorm finalize, FORK + VT_OP_ALLREDUCE on the
        # filter-gradient stream behind the op that completes a bucket): a step is three host calls whatever the
        # number of ranks and layers, and no collective hops to another library's stream and back
        if collectives not in ("torch", "rccl"):
            raise ValueError(collectives)
        self.collectives = collectives if self.dp else "torch"
        if self.collectives == "rccl":
            if self.exchange != "allreduce":
                raise ValueError("collectives='rccl' carries the all-reduce exchange only")
            if not plan_only:
                from .distributed import ensure_library_comm

                # (with SyncBatchNorm: a second communicator for the statistics exchanges, see vt_comm_init_stat)
                ensure_library_comm(self.pg, self.device, stat_comm=bool(sync_bn) and self.dp)
        self._align = 64 * self.world if self.exchange == "sharded" else 64
        st.pad_multiple = self._align
        with self._dev_ctx():
            st.ensure(self.device)
            self.gflat = torch.zeros_like(st.pflat)
            self.mflat = torch.zeros_like(st.pflat)
            self.vflat = torch.zeros_like(st.pflat) if self._adam else None  # second moment: the Adam family only
            # HYPER buffer: [0] learning rate; [4..6] optimiser step count and bias corrections (HYPER_STEP);
            # [8..13] MixUp / CutMix block (mode, lambda, x1, y1, x2, y2)
            self.lr_dev = torch.zeros(16, dtype=torch.float32, device=self.device)
            self.lr_dev[:4] = lr
            self._optws = None
            if self._clip:
                self._alloc_optws(clip_grad_norm, lamb_max_grad_norm if self._lamb else None, weight_decay, norm_weight_decay,
                                  bias_weight_decay, groups)
            self._ema = None
            if self._ema_on:
                self._alloc_ema(ema_decay)
            self.images = torch.zeros(batch_size, 3, image_size, image_size, device=self.device)
            self.labels = torch.zeros(batch_size, dtype=torch.int64, device=self.device)
        self.lr = lr
        total = st.pflat.numel()  # (padded to the exchange's alignment; parameters end at st.total)

        # ---- forward + loss + backward launch lists ---------------------------------------
        # deterministic=True (default: the VT_DETERMINISTIC environment variable): order-free filter gradients and bias
        # sums on top of the always fixed-point BatchNorm statistics -- bit-identical parameter updates
        b = E.Builder(st, self.dtype, training=True, need_grad=True, grad_base=E.GRADS, deterministic=deterministic)
        self.deterministic = b.deterministic
        b.hoist_dgrad_packs = True
        # SyncBatchNorm, the reference recipe's setting (configs/base.yaml:22): batch statistics over
        # ALL ranks.  Off by default for the throughput metric: it adds two small,
        # strictly sequential collectives per unit (67 + 67 for CSPDarknet-53).
        self.sync_bn = bool(sync_bn) and self.dp
        b.bn_world = self.world if self.sync_bn else 1
        b.bn_sync = bool(self.sync_bn)
        self.mix = bool(mix)  # MixUp / CutMix applied on device from a per-step parameter block
        x = b.input_images(batch_size, 3, image_size, image_size, mix=self.mix)
        fmap = backbone._vt_emit_maps(b, x)[-1]
        # (include_pool=False: the last entry IS the backbone's forward output, [B,1,1,C] -- no pooling launch)
        pooled = b.global_avgpool(fmap, "head.pool") if self.include_pool else fmap
        logits = b.conv_unit(pooled, E.ConvSpec.from_linear(head, self._head_rows), None, False, name="head.linear")
        if loss == "bce":
            self._loss_buf = b.bce(logits, label_smoothing, 1.0 / batch_size, mix=self.mix, num_classes=num_classes,
                                   target_threshold=bce_target_threshold, sum_classes=bool(bce_sum_classes))
        else:
            self._loss_buf = b.xent(logits, label_smoothing, 1.0 / batch_size, mix=self.mix, num_classes=num_classes)
        self._logits = logits
        b.build_backward()
        self.prog = Program(b, [logits], [])
        self.n_units = b.n_units
        # stochastic depth (an EfficientNet's residual blocks, the blocks of a ResNetExtractor(stochastic_depth=...)): the keep
        # table float[n_sites][B] of the training program lives in the arena and is written before every step, outside the
        # launch lists -- drawn from a generator this object owns (seeded with drop_seed, plus the rank under data
        # parallelism: every rank drops its own images), or the values of set_keep_factors.  validate() compiles an eval-mode
        # program, which has no table.
        self._keep_buf, self._keep_rates = b.keep_buf, b.keep_rates
        self._keep_override: Optional[torch.Tensor] = None
        self.drop_seed = int(drop_seed) + (torch.distributed.get_rank(process_group) if self.dp else 0)
        self._keep_gen = None
        # sync points: the statistics a finalize kernel reads must be all-reduced right before it
        self._fwd_sync = self._sync_points(self.prog.fwd_ops, self.prog.n_fwd, N.OP_BN_FINALIZE) if self.sync_bn else []
        self._bwd_sync = self._sync_points(self.prog.bwd_ops, self.prog.n_bwd, N.OP_BN_BWD_FINALIZE) if self.sync_bn else []
        if self.collectives == "rccl" and self.sync_bn:
            # the statistics exchange becomes an op in front of each finalize kernel (same stream: ordered by position)
            self.prog.fwd_ops, self.prog.n_fwd = self._with_stat_sync(self.prog.fwd_ops, self.prog.n_fwd, self._fwd_sync)
            self.prog.bwd_ops, self.prog.n_bwd = self._with_stat_sync(self.prog.bwd_ops, self.prog.n_bwd, self._bwd_sync)
            self._fwd_sync, self._bwd_sync = [], []

        # ---- optimiser launch list: one launch per weight-decay group -------------------------
        wd_of = {GROUP_OTHER: weight_decay, GROUP_NORM: norm_weight_decay, GROUP_BIAS: bias_weight_decay}
        self.segments = []  # (elem start, elem end, weight decay)
        gids = [groups[id(p)] for p in st.params]
        start = 0
        for i, p in enumerate(st.params):
            if i + 1 == len(st.params) or gids[i + 1] != gids[i]:
                end = st.offsets[i] + st.slots[i]
                self.segments.append((start, end, wd_of[gids[i]]))
                start = end
        self._momentum, self._lr0 = momentum, lr
        self._emit_opt([(0, total)])
        zb = E.Builder(st, self.dtype, True, True)
        zb.emit(N.OP_MEMSET, [(E.GRADS, 0)], [0], [total * 4])
        self.zero_ops = E.ops_array(zb.fwd)

        # ---- gradient buckets and the backward segments that complete them --------------------
        self.bucketer = None
        self.bwd_cuts = [self.prog.n_bwd]  # op index after which each segment ends
        self.cut_buckets: list[list[int]] = [[]]
        if self.dp:
            # the bucket that starts at 0 (BatchNorm / bias gradients + the stem-side filters) completes last: keep it
            # small, so that the exposed tail of the step is one latency-bound transfer (< 1 MiB)
            nb_end = next((o for o, g_ in zip(st.offsets, gids) if g_ == GROUP_OTHER), total)  # end of the norm | bias region
            head = max(int(head_bucket_kb * 1024) // 4, nb_end)
            buckets = plan_buckets(total, int(bucket_mb * (1 << 20)) // 4, align=self._align, head_elems=head)
            if self.exchange == "sharded":
                self.bucketer = ShardedExchange(self.gflat, buckets, self.pg)
                self._head_bucket = next((i for i, (b0, _) in enumerate(buckets) if b0 == 0), None)
                assert self._head_bucket is not None and buckets[self._head_bucket][1] >= nb_end, \
                    "the f32-read parameters (BatchNorm, biases) must sit in the head bucket"
                self._emit_opt(self.bucketer.shards)  # the optimiser touches this rank's slices only
            else:
                self.bucketer = GradBucketer(self.gflat, buckets, self.pg)
            ready = [0] * len(buckets)  # last bwd op that writes into each bucket
            # an op names the START of the gradient it writes; the gradient extends over the whole
            # parameter, which may straddle a bucket boundary -- every bucket the parameter
            # overlaps must wait for that op (missing this lets a tail bucket be reduced before
            # the op adds to it: ranks then apply different gradients and drift apart)
            import bisect

            starts = list(st.offsets)
            ends = [o + n for o, n in zip(st.offsets, st.slots)]
            for idx in range(self.prog.n_bwd):
                for off in _grad_write_offsets(self.prog.bwd_ops[idx]):
                    k = bisect.bisect_right(starts, off) - 1
                    lo, hi = (starts[k], ends[k]) if k >= 0 and off < ends[k] else (off, off + 1)
                    for bi, (s0, s1) in enumerate(buckets):
                        if s0 < hi and lo < s1:
                            ready[bi] = max(ready[bi], idx + 1)
            cuts = sorted(set(ready) | {self.prog.n_bwd})
            self.bwd_cuts = [c for c in cuts if c > 0]
            self.cut_buckets = [[bi for bi, r in enumerate(ready) if r == c or (c == self.bwd_cuts[0] and r == 0)]
                                for c in self.bwd_cuts]
            if self.collectives == "rccl":
                self._inline_buckets(buckets)

        with self._dev_ctx():
            self.arena = torch.empty(1 if plan_only else self.prog.arena_bytes, dtype=torch.uint8, device=self.device)
            if self.dtype == N.VT_BF16:
                st.mirror.copy_(st.pflat)  # initial bf16 weights; afterwards SGD keeps them fresh
        self.bases = self.prog.bases(
            self.arena.data_ptr(), PARAMS=st.pflat.data_ptr(), GRADS=self.gflat.data_ptr(),
            STATE=st.sflat.data_ptr(), MIRROR=st.mirror.data_ptr(), COUNTERS=st.nflat.data_ptr(),
            INPUT=self.images.data_ptr(), LABELS=self.labels.data_ptr(), MOMENTUM=self.mflat.data_ptr(),
            HYPER=self.lr_dev.data_ptr(), **({"MOMENT2": self.vflat.data_ptr()} if self._adam else {}),
            **({"OPTWS": self._optws.data_ptr()} if self._clip else {}),
            **({"EMA": self._ema.data_ptr()} if self._ema_on else {}))
        self.use_graphs = use_graphs
        self._master_stale = False
        self.model.register_state_dict_pre_hook(self._refuse_stale_export)
        self._side = None  # side stream for the filter gradients (eager mode; graphs fork internally)
        self._graphs = None
        self.steps_done = 0  # optimiser steps
        self.micro_steps_done = 0  # calls of step(): accumulate_grad_batches of them make one optimiser step

    def _alloc_optws(self, clip, lamb_max, wd, norm_wd, bias_wd, groups):
        """the device buffer behind clip_grad_norm / Lamb (OPTWS_CTL_BYTES): control floats | sum-of-squares partials of the
        flat gradient | LAMB's per-item partials | LAMB's work table (one segment per parameter slot of the store, with
        the weight decay of the parameter's group)"""
        st = self.store
        self._sumsq_items = N.opt_items(st.pflat.numel())
        self._sumsq_off = OPTWS_CTL_BYTES
        nbytes = self._sumsq_off + 8 * self._sumsq_items
        table = None
        if self._lamb:
            wd_of = {GROUP_OTHER: wd, GROUP_NORM: norm_wd, GROUP_BIAS: bias_wd}
            self.lamb_wd = [float(wd_of[groups[id(p)]]) for p in st.params]
            table, self._lamb_items = N.lamb_table(st.offsets, st.slots, self.lamb_wd)
            self._lamb_part_off = nbytes
            self._lamb_table_off = E._round_up(nbytes + 16 * self._lamb_items, 16)
            nbytes = self._lamb_table_off + 4 * len(table)
        self._optws = torch.zeros(E._round_up(nbytes, 16), dtype=torch.uint8, device=self.device)
        self._ctl = self._optws[:32].view(torch.float32)
        self._ctl[N.VT_CTL_CLIP] = 0.0 if clip is None else float(clip)
        self._ctl[N.VT_CTL_LAMB_MAX] = 0.0 if lamb_max is None else float(lamb_max)
        if table is not None:
            self.lamb_table = torch.from_numpy(table)  # (host copy: what the plan tests read)
            self._optws[self._lamb_table_off: self._lamb_table_off + 4 * len(table)].view(torch.int32).copy_(self.lamb_table)

    def _alloc_ema(self, decay):
        """the device buffer behind ema_decay: control words (N.VT_EMA_*, 64 bytes) | shadow of pflat | shadow of sflat |
        shadow of nflat | bf16 mirror of the shadow parameters (bf16 programs only).  One allocation, one base (E.EMA)."""
        st = self.store
        n_p, n_s, n_n = st.pflat.numel(), st.sflat.numel(), st.nflat.numel()
        self._ema_p_off = 64
        self._ema_s_off = self._ema_p_off + 4 * n_p
        self._ema_n_off = E._round_up(self._ema_s_off + 4 * n_s, 16)
        self._ema_m_off = E._round_up(self._ema_n_off + 8 * n_n, 16)
        nbytes = self._ema_m_off + (2 * n_p if self.dtype == N.VT_BF16 else 0)
        self._ema = torch.zeros(E._round_up(nbytes, 16), dtype=torch.uint8, device=self.device)
        self._ema_ctl_f = self._ema[:32].view(torch.float32)
        self._ema_ctl_i = self._ema[:32].view(torch.int32)
        self.ema_pflat = self._ema[self._ema_p_off: self._ema_p_off + 4 * n_p].view(torch.float32)
        self.ema_sflat = self._ema[self._ema_s_off: self._ema_s_off + 4 * n_s].view(torch.float32)
        self.ema_nflat = self._ema[self._ema_n_off: self._ema_n_off + 8 * n_n].view(torch.int64)
        self.ema_mirror = (self._ema[self._ema_m_off: self._ema_m_off + 2 * n_p].view(torch.bfloat16)
                           if self.dtype == N.VT_BF16 else None)
        self._ema_ctl_i[N.VT_EMA_PERIOD] = self._ema_steps
        self.set_ema_decay(decay)

    def _emit_ema(self, ob):
        """behind the optimiser launches: the tick (this step's mode: skip / copy / blend), the average of the parameters
        (with its bf16 mirror in the same pass), of the BatchNorm statistics, and the copy of the batch counters"""
        st, ctl = self.store, (E.EMA, 0)
        ob.emit(N.OP_EMA_TICK, [ctl])
        ob.emit(N.OP_EMA_UPDATE, [(E.EMA, self._ema_p_off), (E.PARAMS, 0),
                                  (E.EMA, self._ema_m_off) if self.dtype == N.VT_BF16 else None, ctl], [], [st.pflat.numel()])
        ob.emit(N.OP_EMA_UPDATE, [(E.EMA, self._ema_s_off), (E.STATE, 0), None, ctl], [], [st.sflat.numel()])
        ob.emit(N.OP_EMA_COPY, [(E.EMA, self._ema_n_off), (E.COUNTERS, 0), ctl], [], [8 * st.nflat.numel()])

    def _emit_opt(self, ranges):
        """optimiser launch list: one launch of the chosen optimiser per (element range, weight-decay segment) overlap.

        With clip_grad_norm or Lamb the list is [ADAM_TICK] GRAD_SUMSQ CLIP_COEF <optimiser launches>: the sum of squares
        of the whole flat gradient as per-item partials, then ONE workgroup that adds them and leaves the factor
        grad_scale * c1 / c2 in the OPTWS buffer, which the *_CLIP / LAMB launches read in the place of the immediate
        1 / world.  Lamb is two launches over ONE work table of all parameter tensors (moments + norms, then apply).

        Adam family: the list opens with ONE VT_OP_ADAM_TICK, which advances the step count in the HYPER buffer and
        leaves the two bias corrections beside it; every VT_OP_ADAMW of the step reads them (and the learning rate)
        from there.  The host passes nothing per step, so an eager run and a replayed hipGraph count alike, and a rank
        that updates only its shards still sees the step count every other rank sees."""
        ob = E.Builder(self.store, self.dtype, True, True, grad_base=E.GRADS)
        # the gradient buffer holds the SUM over the micro-batches of a group: 1 / world becomes 1 / (world * k)
        gs = 1.0 / (self.world * self._accum)
        if self._adam:
            ob.emit(N.OP_ADAM_TICK, [(E.HYPER, 0)], [], [self._betas[0], self._betas[1]])
        mirror = lambda lo: (E.MIRROR, lo * 2) if self.dtype == N.VT_BF16 else None  # noqa: E731
        coef = (E.OPTWS, 4 * N.VT_CTL_FACTOR)
        if self._clip:
            total = self.store.pflat.numel()
            assert list(ranges) == [(0, total)], "the gradient norm is global: one range over the whole flat buffer"
            ob.emit(N.OP_GRAD_SUMSQ, [(E.GRADS, 0), (E.OPTWS, self._sumsq_off)], [], [total])
            ob.emit(N.OP_CLIP_COEF, [(E.OPTWS, self._sumsq_off), (E.OPTWS, 0)], [], [self._sumsq_items, gs])
        if self._lamb:
            part, table = (E.OPTWS, self._lamb_part_off), (E.OPTWS, self._lamb_table_off)
            n_segs, total = len(self.store.params), self.store.pflat.numel()
            ob.emit(N.OP_LAMB_MOMENTS,
                    [(E.PARAMS, 0), (E.GRADS, 0), (E.MOMENTUM, 0), (E.MOMENT2, 0), table, part, coef, (E.HYPER, 0)],
                    [n_segs, self._lamb_flags], [self._lamb_items, total, self._betas[0], self._betas[1], self._eps])
            ob.emit(N.OP_LAMB_APPLY,
                    [(E.PARAMS, 0), (E.MOMENTUM, 0), (E.MOMENT2, 0), mirror(0), table, part, (E.HYPER, 0)],
                    [N.VT_BF16, n_segs, self._lamb_flags], [self._lamb_items, total, self._eps])
            ranges = []
        for r0, r1 in ranges:
            for s0, s1, wd in self.segments:
                lo, hi = max(r0, s0), min(r1, s1)
                if hi > lo and self._clip and self._adam:
                    ob.emit(N.OP_ADAMW_CLIP,
                            [(E.PARAMS, lo * 4), (E.GRADS, lo * 4), (E.MOMENTUM, lo * 4), (E.MOMENT2, lo * 4), mirror(lo),
                             (E.HYPER, 0), coef],
                            [N.VT_BF16, int(self.optimizer == "AdamW")],
                            [hi - lo, self._betas[0], self._betas[1], self._eps, wd])
                elif hi > lo and self._clip:
                    ob.emit(N.OP_SGD_CLIP,
                            [(E.PARAMS, lo * 4), (E.GRADS, lo * 4), (E.MOMENTUM, lo * 4), mirror(lo), (E.HYPER, 0), coef],
                            [N.VT_BF16], [hi - lo, self._lr0, self._momentum, wd])
                elif hi > lo and self._adam:
                    ob.emit(N.OP_ADAMW,
                            [(E.PARAMS, lo * 4), (E.GRADS, lo * 4), (E.MOMENTUM, lo * 4), (E.MOMENT2, lo * 4),
                             (E.MIRROR, lo * 2) if self.dtype == N.VT_BF16 else None, (E.HYPER, 0)],
                            [N.VT_BF16, int(self.optimizer == "AdamW")],
                            [hi - lo, self._betas[0], self._betas[1], self._eps, wd, gs])
                elif hi > lo:
                    ob.emit(N.OP_SGD,
                            [(E.PARAMS, lo * 4), (E.GRADS, lo * 4), (E.MOMENTUM, lo * 4),
                             (E.MIRROR, lo * 2) if self.dtype == N.VT_BF16 else None, (E.HYPER, 0)],
                            [N.VT_BF16], [hi - lo, self._lr0, self._momentum, wd, gs])
        if self._ema_on:
            self._emit_ema(ob)
        self.opt_ops, self.n_opt = E.ops_array(ob.fwd), len(ob.fwd)

    def _gather_weights(self) -> None:
        """sharded exchange: bring the updated weights of the other ranks' slices in -- the bf16 mirror the kernels
        read; f32 for the head bucket (BatchNorm / bias parameters are read in f32), whose mirror is re-cast here"""
        st, ex = self.store, self.bucketer
        if self.dtype == N.VT_BF16:
            rest = [i for i in range(len(ex.buckets)) if i != self._head_bucket]
            ex.gather(st.mirror, rest)
            ex.gather(st.pflat, [self._head_bucket])
            h0, h1 = ex.buckets[self._head_bucket]
            st.mirror[h0:h1].copy_(st.pflat[h0:h1])
        else:
            ex.gather(st.pflat)

    def gather_master(self) -> None:
        """sharded exchange: refresh the f32 master parameters and the momentum of the slices other ranks own (before a
        checkpoint / state_dict; a collective: every rank calls it); a no-op for the all-reduce exchange"""
        if self.exchange == "sharded":
            self.bucketer.gather(self.store.pflat)
            self.bucketer.gather(self.mflat)
            if self._adam:
                self.bucketer.gather(self.vflat)
        self._master_stale = False

    def _refuse_stale_export(self, *_):
        # state_dict() of the wrapped model reads views of the flat f32 buffer: after a sharded step the slices other
        # ranks own hold LAST step's values there, and a checkpoint written from them would silently mix old and new
        if self._master_stale:
            raise RuntimeError("exchange='sharded': the f32 master parameters of the slices other ranks own are stale "
                               "on this rank; call TrainStep.gather_master() on every rank before state_dict()")

    @staticmethod
    def _with_stat_sync(ops, n, points):
        """the launch list with a VT_OP_STAT_SYNC in front of every finalize op of `points` (on that op's stream)"""
        at = {idx for idx, *_ in points}
        out = []
        for idx in range(n):
            op = ops[idx]
            if idx in at:
                so = N.Op()
                so.kind = N.OP_STAT_SYNC | (op.kind & N.OP_SIDE_STREAM)
                so.tag = op.tag
                for k in range(N.VT_OP_MAX_PTR):
                    so.ptr[k].base = -1
                so.ptr[0].base, so.ptr[0].offset = op.ptr[0].base, op.ptr[0].offset
                so.i[0] = op.i[0]
                out.append(so)
            cp = N.Op()
            ctypes.memmove(ctypes.addressof(cp), ctypes.addressof(op), ctypes.sizeof(N.Op))
            out.append(cp)
        return E.ops_array(out), len(out)

    def _inline_buckets(self, buckets):
        """collectives='rccl': behind the op that completes a bucket, FORK (the filter-gradient stream waits for the main
        stream's position: BatchNorm / bias gradients are written there) and the bucket's all-reduce ON that stream --
        the main stream waits for nothing, the list's own JOIN closes the side stream before the optimiser.  The
        segments collapse into one list again."""
        p = self.prog
        after = dict(zip(self.bwd_cuts, self.cut_buckets))
        out = []

        def blank(kind):
            o = N.Op()
            o.kind = kind
            for k in range(N.VT_OP_MAX_PTR):
                o.ptr[k].base = -1
            return o

        open_side = False
        for idx in range(p.n_bwd):
            op = p.bwd_ops[idx]
            cp = N.Op()
            ctypes.memmove(ctypes.addressof(cp), ctypes.addressof(op), ctypes.sizeof(N.Op))
            out.append(cp)
            if (op.kind & 0xFFFF) == N.OP_JOIN:
                open_side = False
            bis = after.get(idx + 1, [])
            if bis:
                out.append(blank(N.OP_FORK))
                for bi in bis:
                    b0, b1 = buckets[bi]
                    o = blank(N.OP_ALLREDUCE | N.OP_SIDE_STREAM)
                    o.ptr[0].base, o.ptr[0].offset = E.GRADS, b0 * 4
                    o.i[0] = N.VT_F32
                    o.f[0] = float(b1 - b0)
                    out.append(o)
                open_side = True
        if open_side:  # (the head bucket completes with the last ops, behind the list's own JOIN)
            out.append(blank(N.OP_JOIN))
        self._bwd_without_exchange = (p.bwd_ops, p.n_bwd)  # (skip_exchange: the measurement of what the exchange exposes)
        p.bwd_ops, p.n_bwd = E.ops_array(out), len(out)
        self.bwd_cuts, self.cut_buckets = [p.n_bwd], [[]]
        self.bucketer = None
        self.inline_buckets = [buckets[bi] for bis in after.values() for bi in bis]

    @staticmethod
    def _sync_points(ops, n, kind):
        """[(op index of the finalize kernel, base id, byte offset, bytes of its [replicas][2][C] sums)]"""
        pts = []
        for idx in range(n):
            op = ops[idx]
            if (op.kind & 0xFFFF) == kind:
                pts.append((idx, op.ptr[0].base, op.ptr[0].offset, N.stat_floats(op.i[0]) * 4))
        return pts

    def _sync_view(self, base, off, nbytes):
        """the statistics of one BatchNorm as the all-reduce sees them: replica 0 of int64[replicas][2][C][2]"""
        start = {E.ZERO_F: self.prog.zf_off, E.ZERO_B: self.prog.zb_off}[base] + off
        # the sums are 64-bit fixed point (vt_amd.h, VT_STAT_REPLICAS): an integer all-reduce, exact and order-free
        return self.arena[start : start + nbytes // N.VT_STAT_REPLICAS].view(torch.int64)

    def _sync_stats(self, base, off, nbytes, stream):
        """SyncBatchNorm exchange of one layer's sums: the VT_STAT_REPLICAS (16) replicas the kernels spread
        their atomics over are folded into replica 0 on the device first (vt_stat_fold), so the collective carries 32 C
        bytes -- the algorithmic payload -- instead of the raw 512 B x C buffer.  Fold and all-reduce add the limbs as
        integers: the marker of a non-finite contribution (vt_amd.h) on any replica or rank survives into every rank's sum"""
        start = {E.ZERO_F: self.prog.zf_off, E.ZERO_B: self.prog.zb_off}[base] + off
        C_ = nbytes // (N.VT_STAT_REPLICAS * 32)
        N.check(N.lib().vt_stat_fold(ctypes.c_void_p(self.arena.data_ptr() + start), C_, ctypes.c_void_p(stream)))
        torch.distributed.all_reduce(self._sync_view(base, off, nbytes), group=self.pg)

    def _run_list(self, ops, n, sync, cuts, cut_buckets, s, side, keep_side_open=True, exchange=True):
        """run a launch list in segments: a segment ends before every finalize kernel whose statistics
        must be all-reduced first (SyncBatchNorm) and after every op that completes a gradient bucket.

        Cutting the list must not cost the N = 1 schedule: an intermediate segment leaves the filter-gradient
        (side) stream open instead of joining it, and a bucket's collective is issued with the SIDE stream current,
        after ordering that stream behind the main stream's position (BatchNorm / bias gradients are written
        there).  RCCL's stream then waits for exactly the producers of the bucket, the main stream for nothing;
        the list's own JOIN op (last segment) and `bucketer.finish()` close both before the optimiser.
        `keep_side_open=False` (the forward list, which carries no JOIN op of its own): every segment joins the side
        stream on return, so the data-gradient filter packs hoisted onto it are ordered before backward reads them."""
        marks = {idx: ("sync", (base, off, nb)) for idx, base, off, nb in sync}
        ends = sorted(set(marks) | set(cuts) | {n})
        lo = 0
        for hi in ends:
            if hi > lo:
                sub = (N.Op * (hi - lo)).from_address(ctypes.addressof(ops) + lo * ctypes.sizeof(N.Op))
                N.run_ops(sub, hi - lo, self.bases, s, side=side, leave_side_open=keep_side_open and hi != n)
            if hi in marks:  # stream-ordered: NCCL makes the launch stream wait, no host sync
                self._sync_stats(*marks[hi][1], s)
            if hi in cut_buckets and cut_buckets[hi] and exchange and not self._skip_exchange:
                if side and self._side is not None:
                    N.stream_wait(side, s)
                    with torch.cuda.stream(self._side):
                        for bi in cut_buckets[hi]:
                            self.bucketer.reduce_bucket(bi)
                else:
                    for bi in cut_buckets[hi]:
                        self.bucketer.reduce_bucket(bi)
            lo = hi

    def _dev_ctx(self):
        import contextlib

        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    # -- data-parallel plumbing ----------------------------------------------------------------
    def exchange_skipped(self):
        """MEASUREMENT ONLY: a context in which step() runs the data-parallel schedule -- cut lists, stream ordering --
        WITHOUT issuing the collectives (step time with them minus step time without = what the exchange leaves exposed).
        Steps taken inside update every replica from its own rank's gradients, which would desynchronise the replicas (and
        under the sharded exchange leave non-owned slices stale): the context snapshots parameters, BatchNorm state, the
        batch counters, momentum and the bf16 mirror (with ema_decay: the shadow buffers and their counts too; with
        accumulate_grad_batches: the gradient buffer, steps_done and micro_steps_done, so a group of micro-steps begun
        outside continues where it was) on entry and restores them on exit."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            st = self.store
            state = (st.pflat, st.sflat, st.nflat, self.mflat, st.mirror) + ((self.vflat, self.lr_dev) if self._adam else ())
            if self._ema_on:  # the shadow buffers with their control words (mode, update and step counts)
                state += (self._ema,)
            keep = [t.clone() for t in state]
            # (accumulate_grad_batches: the position inside a group of micro-steps and the partly accumulated gradient)
            counts, gkeep = (self.steps_done, self.micro_steps_done), (self.gflat.clone() if self._accum > 1 else None)
            self._skip_exchange = True
            try:
                yield self
            finally:
                self._skip_exchange = False
                torch.cuda.synchronize(self.device)
                for dst, src_ in zip(state, keep):
                    dst.copy_(src_)
                if gkeep is not None:
                    self.gflat.copy_(gkeep)
                    self.steps_done, self.micro_steps_done = counts

        return ctx()

    def broadcast_parameters(self, src: int = 0) -> None:
        """initial weights + buffers from rank `src` (what DDP's constructor does)."""
        if self.dp:
            # parameters, BatchNorm buffers (running statistics AND the int64 batch counters) and the optimiser's
            # momentum: a resumed run starts identical on every rank
            torch.distributed.broadcast(self.store.pflat, src, group=self.pg)
            torch.distributed.broadcast(self.store.sflat, src, group=self.pg)
            torch.distributed.broadcast(self.store.nflat, src, group=self.pg)
            torch.distributed.broadcast(self.mflat, src, group=self.pg)
            if self._adam:  # second moment and the step count with its bias corrections
                torch.distributed.broadcast(self.vflat, src, group=self.pg)
                torch.distributed.broadcast(self.lr_dev[HYPER_STEP:HYPER_STEP + 4], src, group=self.pg)
            if self._ema_on:  # the average and its counts: a resumed run keeps averaging alike on every rank
                torch.distributed.broadcast(self._ema, src, group=self.pg)
            if self.dtype == N.VT_BF16:
                self.store.mirror.copy_(self.store.pflat)

    def weights_changed(self) -> None:
        """call after writing parameters from outside (load_state_dict, manual init): refreshes the bf16 mirror.
        Optimiser state (moments, step count) is not reset, as loading weights does not reset it in torch."""
        if self.dtype == N.VT_BF16:
            self.store.mirror.copy_(self.store.pflat)

    def set_keep_factors(self, t: Optional[torch.Tensor]) -> None:
        """the stochastic-depth keep factors of the NEXT step(s): a float[n_sites][B] tensor (one row per residual block in
        emission order, one factor per image) used instead of drawing, or None to draw again"""
        if t is not None:
            if not self._keep_rates:
                raise RuntimeError("this TrainStep's program has no keep table (no stochastic depth in the backbone)")
            if tuple(t.shape) != (len(self._keep_rates), self.B):
                raise ValueError(f"keep factors of shape {tuple(t.shape)}: this program has {len(self._keep_rates)} sites and "
                                 f"{self.B} images")
            t = t.detach().to(device=self.device, dtype=torch.float32).clone()
        self._keep_override = t

    def keep_factors(self) -> Optional[torch.Tensor]:
        """the keep table of the last step, read back from the arena (None: the program has none)"""
        if self._keep_buf is None:
            return None
        n, off = len(self._keep_rates), self._keep_buf.offset
        return self.arena[off : off + n * self.B * 4].view(torch.float32).view(n, self.B).clone()

    def _fill_keep_table(self) -> None:
        n, off = len(self._keep_rates), self._keep_buf.offset
        if self._keep_gen is None:
            self._keep_gen = torch.Generator(device=self.device)
            self._keep_gen.manual_seed(self.drop_seed)
        view = self.arena[off : off + n * self.B * 4].view(torch.float32).view(n, self.B)
        view.copy_(draw_keep_factors(self._keep_rates, self.B, self.device, self._keep_override, self._keep_gen))

    def set_lr(self, lr: float) -> None:
        self.lr = lr
        self.lr_dev[:4] = lr

    def set_clip_grad_norm(self, value: float) -> None:
        """change the clip_grad_norm threshold of the NEXT step(s); like set_lr, a captured graph follows (the value
        lives on the device).  0 or inf switch the clip off without removing its launches."""
        if not self._clip_user:
            raise RuntimeError("this TrainStep was built without clip_grad_norm: its optimiser list has no clipping launches")
        if not float(value) >= 0.0:
            raise ValueError(f"clip_grad_norm={value!r}: a threshold is >= 0")
        self._ctl[N.VT_CTL_CLIP] = float(value)

    # -- weight EMA ------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if not self._ema_on:
            raise RuntimeError(f"{what}: this TrainStep was built without ema_decay and keeps no average of its weights")

    def set_ema_decay(self, decay: float) -> None:
        """change the decay of the NEXT update(s); like set_lr, a captured graph follows (alpha lives on the device).
        alpha = 1 - decay is formed in double here and rounded to f32 once (vt_amd.h)."""
        self._need_ema("set_ema_decay")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"ema_decay={decay!r}: a decay in [0, 1)")
        self.ema_decay = float(decay)
        self._ema_ctl_f[N.VT_EMA_ALPHA] = 1.0 - float(decay)

    def ema_updates(self) -> int:
        """updates of the average made so far, as the DEVICE counts them (vt_ema_tick; synchronises)"""
        self._need_ema("ema_updates")
        return int(self._ema_ctl_i[N.VT_EMA_COUNT].item())

    def _ema_views(self):
        """(state_dict key, shadow tensor in the key's logical shape) for every entry of the model's state_dict"""
        st = self.store
        flat = {E.PARAMS: self.ema_pflat, E.STATE: self.ema_sflat, E.COUNTERS: self.ema_nflat}
        for key, t in self.model.state_dict(keep_vars=True).items():
            base, off, n = st.where(t)
            seg = flat[base][off: off + n]
            if t.dim() == 4:  # held channels_last, [Cout][kh][kw][Cin], like the parameter itself (ParamStore)
                o, i, kh, kw = t.shape
                yield key, seg.view(o, kh, kw, i).permute(0, 3, 1, 2)
            else:
                yield key, seg.view(t.shape)

    def ema_state_dict(self) -> dict:
        """the average under the keys and logical shapes of `model.state_dict()` (copies); load it into a model, or a twin
        TrainStep, with load_state_dict"""
        self._need_ema("ema_state_dict")
        if self.ema_updates() == 0:
            raise RuntimeError("ema_state_dict: no update of the average yet (the first optimiser step makes the first)")
        return {k: v.clone(memory_format=torch.contiguous_format) for k, v in self._ema_views()}

    def load_ema_state_dict(self, sd: dict, updates: Optional[int] = None, steps: Optional[int] = None) -> None:
        """the inverse of ema_state_dict, for resuming: writes the shadow buffers (and their bf16 mirror).  The next update
        blends instead of copying; `updates` also restores the device's update count (default: at least 1) and `steps` its
        count of optimiser steps, which carries the phase of ema_steps > 1 (default: left as it is -- a fresh TrainStep
        starts a new period with its first step; pass the saved run's steps_done to continue the old one)."""
        self._need_ema("load_ema_state_dict")
        views = dict(self._ema_views())
        if set(sd) != set(views):
            raise KeyError(f"load_ema_state_dict: keys differ from the model's state_dict: "
                           f"{sorted(set(sd) ^ set(views))[:8]}")
        with torch.no_grad():
            for k, v in views.items():
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise ValueError(f"load_ema_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(v.shape)}")
                v.copy_(sd[k])
            if self.ema_mirror is not None:
                self.ema_mirror.copy_(self.ema_pflat)
        self._ema_ctl_i[N.VT_EMA_COUNT] = max(self.ema_updates(), 1) if updates is None else int(updates)
        if steps is not None:
            self._ema_ctl_i[N.VT_EMA_STEP] = int(steps)

    def last_grad_norm(self) -> float:
        """the norm N = sqrt(sum g^2) / world of the averaged gradient of the last step, before any clipping, as the device
        formed it (clip_grad_norm or Lamb only; synchronises).  With accumulate_grad_batches = k: of the mean over the
        group's k micro-batches, N = sqrt(sum G^2) / (world * k) for the accumulated G."""
        if not self._clip:
            raise RuntimeError("this TrainStep forms no gradient norm (neither clip_grad_norm nor optimizer='Lamb')")
        return float(self._ctl[N.VT_CTL_NORM].item())

    def opt_steps(self) -> int:
        """optimiser steps taken so far as the DEVICE counts them (Adam family: the int32 in slot HYPER_STEP of the
        HYPER buffer, advanced by the step's own VT_OP_ADAM_TICK; synchronises).  SGD keeps no device count."""
        if not self._adam:
            return self.steps_done
        return int(self.lr_dev[HYPER_STEP:HYPER_STEP + 1].view(torch.int32).item())

    def set_mix(self, mode: str = "none", lam: float = 1.0, box=(0, 0, 0, 0)) -> None:
        """MixUp / CutMix parameters of the NEXT step(s) (TrainStep(mix=True)): mode 'none' | 'mixup' |
        'cutmix'; `lam` as sampled (mixup) or 1 - box area / image area (cutmix, extras.py:88);
        box = (x1, y1, x2, y2).  `sample_mix` draws them exactly as extras.py does."""
        if not self.mix:
            raise RuntimeError("this TrainStep was built without mix=True")
        code = {"none": 0.0, "mixup": 1.0, "cutmix": 2.0}[mode]
        vals = torch.tensor([code, float(lam), *[float(v) for v in box], 0.0, 0.0], dtype=torch.float32)
        self.lr_dev[8:16].copy_(vals, non_blocking=True)

    # -- one step ----------------------------------------------------------------------------------
    def _segment_ops(self):
        """(ops pointer, count) of every backward segment."""
        p = self.prog
        segs, lo = [], 0
        for hi in self.bwd_cuts:
            sub = (N.Op * (hi - lo)).from_address(ctypes.addressof(p.bwd_ops) + lo * ctypes.sizeof(N.Op))
            segs.append((sub, hi - lo))
            lo = hi
        return segs

    def _build_graphs(self):
        p = self.prog
        with self._dev_ctx():
            self._graphs = {
                "head": N.Graph(E.ops_array(list(self.zero_ops[:1]) + [p.fwd_ops[i] for i in range(p.n_fwd)]),
                                1 + p.n_fwd, self.bases),
                # (accumulate_grad_batches: the later micro-steps of a group add to the gradient the first one started)
                "head_keep": N.Graph(p.fwd_ops, p.n_fwd, self.bases) if self._accum > 1 else None,
                "bwd": [N.Graph(ops, n, self.bases) for ops, n in self._segment_ops()],
                "opt": N.Graph(self.opt_ops, self.n_opt, self.bases),
            }

    def step(self, images: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None) -> None:
        """fwd + loss + bwd + gradient all-reduce + optimiser on the resident (or given) batch.  With
        accumulate_grad_batches = k: forward + backward of one micro-batch; the first call of a group of k zeroes the
        gradient buffer, the last one exchanges the accumulated gradient and runs the optimiser."""
        if self.plan_only:
            raise RuntimeError("plan_only TrainStep cannot execute: there is no CPU path")
        micro = self.micro_steps_done % self._accum
        first, last = micro == 0, micro == self._accum - 1
        no_sync = self._skip_exchange or not last  # (micro-steps in front of the last: DDP's no_sync)
        with self._dev_ctx():
            if images is not None:
                self.images.copy_(images, non_blocking=True)
            if labels is not None:
                self.labels.copy_(labels, non_blocking=True)
            s = current_stream_handle()
            p = self.prog
            if self._keep_buf is not None:
                self._fill_keep_table()  # (once per step, on the current stream in front of the lists or the graph)
            graphs = self.use_graphs and not self.sync_bn and self.collectives != "rccl"
            if graphs:
                if self._graphs is None:
                    self._build_graphs()
                self._graphs["head" if first else "head_keep"].launch(s)
                for g, bks in zip(self._graphs["bwd"], self.cut_buckets):
                    g.launch(s)
                    for bi in ([] if no_sync else bks):
                        self.bucketer.reduce_bucket(bi)
            else:
                if self._side is None:
                    self._side = torch.cuda.Stream(self.device)
                side = int(self._side.cuda_stream)
                if first:
                    N.run_ops(self.zero_ops, 1, self.bases, s)
                self._run_list(p.fwd_ops, p.n_fwd, self._fwd_sync, [], {}, s, side, keep_side_open=False)
                bwd_ops, n_bwd = p.bwd_ops, p.n_bwd
                if no_sync and self.collectives == "rccl" and getattr(self, "_bwd_without_exchange", None):
                    bwd_ops, n_bwd = self._bwd_without_exchange
                self._run_list(bwd_ops, n_bwd, self._bwd_sync, [n_bwd] if self.collectives == "rccl" else self.bwd_cuts,
                               dict(zip(self.bwd_cuts, self.cut_buckets)), s, side, exchange=not no_sync)
            if self.bucketer is not None and not no_sync:
                self.bucketer.finish()
            if last:
                if graphs:
                    self._graphs["opt"].launch(s)
                else:
                    N.run_ops(self.opt_ops, self.n_opt, self.bases, s)
                if self.exchange == "sharded" and not self._skip_exchange:
                    self._gather_weights()
                    self._master_stale = True
        self.micro_steps_done += 1
        if last:
            self.steps_done += 1

    # ---- validation step (reference classifier.py:97-109) ----------------------------------------------------------
    def _build_eval(self):
        """The SAME modules and flat parameter store compiled once more in eval mode: every BatchNorm uses its running
        statistics (folded into the conv epilogues: one launch per unit), no gradient bookkeeping, and the loss op is the
        validation one (no label smoothing, top-1 hits).  Its arena is its own (forward only)."""
        was = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        try:
            b = E.Builder(self.store, self.dtype, training=False, need_grad=False)
            x = b.input_images(self.B, 3, self.S, self.S)
            fmap = self.model[0]._vt_emit_maps(b, x)[-1]
            pooled = b.global_avgpool(fmap, "head.pool") if self.include_pool else fmap
            # (the head by position from the end: model[3] with the pooling children, model[1] without)
            logits = b.conv_unit(pooled, E.ConvSpec.from_linear(self.model[-1], self._head_rows), None, False, name="head.linear")
            sums = b.xent_eval(logits, num_classes=self.num_classes)
            b.build_backward()
            prog = Program(b, [logits], [])
        finally:
            for m, t in was:
                m.training = t
        with self._dev_ctx():
            arena = torch.empty(prog.arena_bytes, dtype=torch.uint8, device=self.device)
        bases = prog.bases(arena.data_ptr(), PARAMS=self.store.pflat.data_ptr(), STATE=self.store.sflat.data_ptr(),
                           MIRROR=self.store.mirror.data_ptr(), INPUT=self.images.data_ptr(),
                           COUNTERS=self.store.nflat.data_ptr(), LABELS=self.labels.data_ptr())
        self._eval = (prog, arena, bases, prog.zf_off + sums.offset, logits)

    def validate(self, images: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, ema: bool = False) -> dict:
        """One validation step on the resident (or given) batch: eval-mode forward, cross entropy WITHOUT label smoothing,
        top-1 accuracy -- `validation_step` of classifier.py:97-109.  Data parallel, the three sums (loss, hits, rows) are
        all-reduced over the ranks (its `sync_dist=True`; collective C4 of SURVEY section 2), so every rank returns the
        GLOBAL mean loss and accuracy.  Parameters, BatchNorm statistics and optimiser state are not touched.
        ema=True scores the averaged weights (TrainStep(ema_decay=...)): the SAME program and arena, with the parameter,
        statistics, mirror and counter bases pointing at the shadow buffers."""
        if ema:
            self._need_ema("validate(ema=True)")
        if self.plan_only:
            raise RuntimeError("plan_only TrainStep cannot execute: there is no CPU path")
        if ema and self.ema_updates() == 0:
            raise RuntimeError("validate(ema=True): no update of the average yet (the first optimiser step makes the first)")
        if getattr(self, "_master_stale", False):
            self.gather_master()
        with self._dev_ctx():
            if images is not None:
                self.images.copy_(images, non_blocking=True)
            if labels is not None:
                self.labels.copy_(labels, non_blocking=True)
            if getattr(self, "_eval", None) is None:
                self._build_eval()
            prog, arena, bases, off, _ = self._eval
            if ema:
                bases = self._eval_bases_ema()
            s = current_stream_handle()
            if self._side is None:
                self._side = torch.cuda.Stream(self.device)
            N.run_ops(prog.fwd_ops, prog.n_fwd, bases, s, side=int(self._side.cuda_stream))
            sums = arena[off : off + 12].view(torch.float32).clone()
        sums = reduce_validation_sums(sums, self.pg if self.dp else None)
        loss_sum, hits, rows = (float(v) for v in sums.tolist())
        return {"loss": loss_sum / rows, "acc": hits / rows, "correct": int(round(hits)), "count": int(round(rows))}

    def _eval_bases_ema(self) -> list:
        """the bases of the validation program with PARAMS / STATE / MIRROR / COUNTERS at the shadow buffers (an f32 program
        reads no mirror: its slot keeps the store's)"""
        if getattr(self, "_eval_ema", None) is None:
            prog, arena = self._eval[0], self._eval[1]
            mirror = self.ema_mirror if self.ema_mirror is not None else self.store.mirror
            self._eval_ema = prog.bases(arena.data_ptr(), PARAMS=self.ema_pflat.data_ptr(), STATE=self.ema_sflat.data_ptr(),
                                        MIRROR=mirror.data_ptr(), INPUT=self.images.data_ptr(),
                                        COUNTERS=self.ema_nflat.data_ptr(), LABELS=self.labels.data_ptr())
        return self._eval_ema

    def eval_logits(self) -> torch.Tensor:
        """logits of the last validate() call"""
        _, arena, _, _, logits = self._eval
        return E.tref_to_tensor(arena, logits).reshape(self.B, -1)[:, :self.num_classes]

    def loss(self) -> float:
        """mean loss of the last step (synchronises)."""
        off = self.prog.zf_off + self._loss_buf.offset
        return float(self.arena[off : off + 4].view(torch.float32).item())

    def logits(self) -> torch.Tensor:
        return E.tref_to_tensor(self.arena, self._logits).reshape(self.B, -1)[:, :self.num_classes]
