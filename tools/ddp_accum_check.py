"""Gradient accumulation under data parallelism: two ranks of the fused train step on ONE GPU (gloo moves the buckets),

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
        --master-port 29533 tools/ddp_accum_check.py

each with accumulate_grad_batches = 2.  One optimiser step then consumes four micro-batches (rank r takes micro-batches
r and 2 + r of the group) and divides their summed gradient by world * k = 4.  Checked:
  * the first micro-step of a group reduces NO bucket (DDP's no_sync), the second one every bucket once;
  * the ranks end bit-identical;
  * rank 0 replays the same micro-batches alone with accumulate_grad_batches = 4 (data_parallel=False): the weight
    updates agree within the f32 bound tools/ddp_check.py holds this model to (0.1 of the update's norm; the figure is
    printed -- the two runs add the same four gradients in a different order).
Prints 'DDP_ACCUM_CHECK_OK' on success."""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "vision-toolbox_amd"), str(ROOT)]

import torch
import torch.distributed as dist

from oracle import filler
from vision_toolbox import _native as N
from vision_toolbox import backbones
from vision_toolbox.trainer import TrainStep

NAME, NCLS, B, S, GROUPS, LR, WD = "vovnet19_slim_ese", 16, 4, 64, 2, 2e-3, 1e-3
KEYS = ("0.stem.0.conv.weight", "0.stages.3.module_0.out_conv.conv.weight", "3.weight", "3.bias")


def make(k, **kw):
    return TrainStep(getattr(backbones, NAME)(), NCLS, B, S, torch.float32, lr=LR, momentum=0.9, weight_decay=WD,
                     label_smoothing=0.1, device="cuda:0", bucket_mb=0.25, use_graphs=False, accumulate_grad_batches=k, **kw)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    n_micro = GROUPS * 4
    xs = [filler.images(B, S, seed=1000 + i) for i in range(n_micro)]
    ys = [filler.labels(B, NCLS, seed=2000 + i) for i in range(n_micro)]

    torch.manual_seed(rank)  # ranks start from different weights; the broadcast fixes that
    ts = make(2)
    if rank == 0:
        filler.fill_module(ts.model, "ddpacc.")
        ts.weights_changed()
    ts.broadcast_parameters(0)
    assert ts.world == world and ts.bucketer is not None and len(ts.bucketer.buckets) >= 3, "want several buckets"
    reduced = []
    inner = ts.bucketer.reduce_bucket
    ts.bucketer.reduce_bucket = lambda bi: (reduced.append(bi), inner(bi))[1]
    init = {k: v.detach().clone().cpu() for k, v in ts.model.state_dict().items()}
    before = N.launch_count()
    for g in range(GROUPS):
        for j in range(2):
            i = 4 * g + 2 * j + rank
            reduced.clear()
            ts.step(xs[i].cuda(), ys[i].cuda())
            if j == 0:
                assert reduced == [], f"micro-step 0 of group {g} reduced buckets {reduced}"
            else:
                assert sorted(reduced) == list(range(len(ts.bucketer.buckets))), reduced
    torch.cuda.synchronize()
    assert N.launch_count() > before and ts.steps_done == GROUPS and ts.micro_steps_done == 2 * GROUPS
    mine = torch.cat([p.detach().reshape(-1).cpu() for p in ts.model.parameters()])
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    assert torch.equal(both[0], both[1]), "ranks diverged: they must apply identical averaged gradients"

    if rank == 0:
        solo = make(4, data_parallel=False)
        assert solo.world == 1 and solo.bucketer is None
        filler.fill_module(solo.model, "ddpacc.")
        solo.weights_changed()
        for i in range(n_micro):
            solo.step(xs[i].cuda(), ys[i].cuda())
        torch.cuda.synchronize()
        assert solo.steps_done == GROUPS
        got, ref = ts.model.state_dict(), solo.model.state_dict()
        worst = 0.0
        for k in KEYS:
            d_got, d_ref = got[k].cpu() - init[k], ref[k].cpu() - init[k]
            err = ((d_got - d_ref).norm() / d_ref.norm()).item()
            worst = max(worst, err)
            print(f"  update of {k}: two ranks x k=2 against one rank x k=4: rel err {err:.3e}", flush=True)
            assert d_ref.norm() > 0 and err < 0.1, (k, err)
        print(f"DDP_ACCUM_CHECK_OK world={world} buckets={len(ts.bucketer.buckets)} segments={len(ts.bwd_cuts)} "
              f"worst update rel err {worst:.3e}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
