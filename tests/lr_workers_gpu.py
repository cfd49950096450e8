"""Worker of the two-rank learning-rate schedule test: both ranks run the real HIP kernels on
cuda:0 and talk over the peer-access transport (``--comm ipc``), the step captured into a HIP
graph.  Importable by spawned children."""
from __future__ import annotations

import torch

from clip_workers_gpu import _finish_step
from dist_workers_gpu import LR, _init, full_batch, make_model, shard

STEPS = 4


def schedule():
    from distributed_pytorch_cookbook_amd.ops.schedule import LRSchedule

    return LRSchedule("cosine", LR, 2, 4, 0.1)


def ipc_lr_worker(rank, world, out):
    info = _init()
    assert info.device.type == "cuda"
    from distributed_pytorch_cookbook_amd.engine.fsdp import FSDPEngine

    eng = FSDPEngine(make_model(), "cuda", lr=LR, prefetch=1, graph=True, comm_kind="ipc", lr_schedule=schedule())
    tp = eng.store.tp
    assert tp.kind == "ipc", tp.kind
    lrs = []
    for s in range(STEPS):  # (the first failure raises: nothing more is started on the device)
        eng.train_step(*shard(*full_batch(step=s), rank, world))
        _finish_step(tp, f"fsdp step {s} on rank {rank}")
        lrs.append(eng.lr)
    assert eng._stepper.graph is not None, "the two-rank step was not captured"
    sd = eng.full_state_dict()
    torch.save({"lrs": lrs}, f"{out}.{rank}")
    if rank == 0:
        torch.save({k: v.float().cpu() for k, v in sd.items()}, out)
