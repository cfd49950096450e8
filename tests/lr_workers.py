"""Worker bodies of the learning-rate schedule engine tests (gloo; importable by spawned children)."""
from __future__ import annotations

import torch

from clip_workers import build
from dist_workers import LR, full_batch, shard

STEPS, WARMUP, DECAY = 4, 2, 4
HYPER = {False: {}, True: {"weight_decay": 0.1, "betas": (0.8, 0.95)}}  # (default / non-default AdamW)


def schedule(kind="cosine"):
    from distributed_pytorch_cookbook_amd.ops.schedule import LRSchedule

    return LRSchedule(kind, LR, WARMUP, DECAY, 0.1)


def scheduled(kind, world, hyper):
    eng, dp, idx = build(kind, world, max_grad_norm=None, lr_schedule=schedule(), **HYPER[hyper])
    return eng, dp, idx


def run_steps(eng, dp, idx):
    lrs = []
    for s in range(STEPS):
        eng.train_step(*shard(*full_batch(step=s), idx, dp))
        lrs.append(eng.lr)
    return lrs


def single_scheduled(hyper):
    """The one-process scheduled engine on the full batch: (state dict, engine.lr of every step)."""
    eng, dp, idx = scheduled("single", 1, hyper)
    lrs = run_steps(eng, dp, idx)
    return {k: v.clone() for k, v in eng.full_state_dict().items()}, lrs


def worker_lr(rank, world, out, kind, hyper):
    from distributed_pytorch_cookbook_amd.parallel import comm

    comm.init_dist(force_cpu=True)
    eng, dp, idx = scheduled(kind, world, hyper)
    for o, _, _ in eng.parts:
        assert o.lr_schedule == schedule()
        assert (o.weight_decay, tuple(o.betas)) == (HYPER[hyper].get("weight_decay", 1e-2),
                                                    HYPER[hyper].get("betas", (0.9, 0.999)))
    lrs = run_steps(eng, dp, idx)
    sd = eng.full_state_dict()
    torch.save({"lrs": lrs}, f"{out}.{rank}")
    if rank == 0:
        torch.save({k: v.clone() for k, v in sd.items()}, out)
